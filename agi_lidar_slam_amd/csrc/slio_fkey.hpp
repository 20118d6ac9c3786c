// slio_fkey.hpp -- order-preserving integer keys of floats, for the atomic
// min / max of bounding boxes (the map index, the scan VoxelGrid, the keyframe
// assembly, the cube store) and the sort key of a scan's point times.  HIP
// only; as in slio_search.hpp the device function is __forceinline__ (the
// library is built without relocatable device code).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

namespace slio {

__device__ __forceinline__ int32_t fkey(float f) {
  const int32_t b = __float_as_int(f);
  return b >= 0 ? b : b ^ 0x7FFFFFFF;
}
static inline float fkey_inv(int32_t k) {
  const int32_t b = k >= 0 ? k : k ^ 0x7FFFFFFF;
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

}  // namespace slio
