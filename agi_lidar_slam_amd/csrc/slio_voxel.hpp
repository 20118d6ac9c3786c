// slio_voxel.hpp -- pcl::VoxelGrid's geometry (PCL 1.10 voxel_grid.hpp
// applyFilter), written once for the scan VoxelGrid (k_vg_geom, k_vg_keys:
// slio_scan.hip), the cube store's per-cube one (k_lvx_geom, k_lvx_keys:
// slio_cube_store.hip) and the host restatement of the latter
// (slio_aloam_map.cpp).  Host and device; internal to the library.  Every
// float / int64 step is in PCL's order (the build has -ffp-contract=off).
#pragma once

#include <climits>
#include <cmath>
#include <cstdint>

#include "slio_common.hpp"

namespace slio {

#pragma GCC visibility push(hidden)  // (a host copy the compiler keeps out of line is not an export)

// the grid of one cloud: voxel index = ijk0 * mul[0] + ijk1 * mul[1] + ijk2 * mul[2],
// ijk = int(floor(p * inv) - float(minb))
struct VoxelGeom {
  float inv;    // inverse_leaf_size_ (one leaf for the three axes)
  int minb[3];  // min_b_
  int mul[3];   // divb_mul_
};
enum VoxelKind {
  kVoxelNone = 0,  // no finite point: empty output
  kVoxelPass = 1,  // "leaf size is too small": dx * dy * dz above INT32_MAX, output = input
  kVoxelGrid = 2
};

// box[0..2] / box[3..5]: the finite points' minimum / maximum per axis as
// order-preserving keys (fkey, slio_fkey.hpp), box[6]: how many are finite.
// Only with kVoxelGrid do minb and mul mean anything (0 and 1 otherwise).
SLIO_HD inline VoxelKind voxel_geometry(const int32_t box[7], float leaf, VoxelGeom* g) {
  g->inv = 1.0f / leaf;
  for (int a = 0; a < 3; ++a) {
    g->minb[a] = 0;
    g->mul[a] = 1;
  }
  if (box[6] == 0) return kVoxelNone;
  float mn[3], mx[3];
  int64_t dd[3];
  for (int a = 0; a < 3; ++a) {
    const int32_t lo = box[a] >= 0 ? box[a] : box[a] ^ 0x7FFFFFFF;
    const int32_t hi = box[3 + a] >= 0 ? box[3 + a] : box[3 + a] ^ 0x7FFFFFFF;
    __builtin_memcpy(&mn[a], &lo, 4);
    __builtin_memcpy(&mx[a], &hi, 4);
    const float span = (mx[a] - mn[a]) * g->inv;
    dd[a] = std::isfinite(span) && span < 9.2e18f ? (int64_t)span + 1 : INT64_MAX / 4;
  }
  bool pass = dd[0] > INT32_MAX || dd[1] > INT32_MAX || dd[2] > INT32_MAX;
  if (!pass) {
    const int64_t d01 = dd[0] * dd[1];  // (<= 2^62)
    pass = d01 > INT32_MAX || d01 * dd[2] > (int64_t)INT32_MAX;
  }
  if (pass) return kVoxelPass;
  int div[3];
  for (int a = 0; a < 3; ++a) {
    g->minb[a] = (int)floorf(mn[a] * g->inv);
    div[a] = (int)floorf(mx[a] * g->inv) - g->minb[a] + 1;
  }
  g->mul[1] = div[0];
  g->mul[2] = div[0] * div[1];
  return kVoxelGrid;
}

SLIO_HD inline uint32_t voxel_index(float x, float y, float z, float inv, const int minb[3], const int mul[3]) {
  const int i0 = (int)(floorf(x * inv) - (float)minb[0]);
  const int i1 = (int)(floorf(y * inv) - (float)minb[1]);
  const int i2 = (int)(floorf(z * inv) - (float)minb[2]);
  return (uint32_t)(i0 * mul[0] + i1 * mul[1] + i2 * mul[2]);
}

#pragma GCC visibility pop

}  // namespace slio
