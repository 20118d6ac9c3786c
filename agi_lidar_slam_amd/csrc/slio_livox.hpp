// slio_livox.hpp -- what the host formulas (slio_livox.cpp) and the device cube
// map (slio_livox.hip) of livox_mapping's laserMapping share: the cube array's
// shape and the cube index of a coordinate.  Internal to the library.
#pragma once

#include <cmath>
#include <cstdint>

#include "slio_common.hpp"

namespace slio {
namespace lvx {

// laserCloudWidth / Height / Depth and laserCloudNum (laserMapping.cpp:67-72)
constexpr int kW = 21, kH = 11, kD = 21, kNum = kW * kH * kD;

// int((t + 25.0) / 50.0) + cen, one less when t + 25.0 < 0 (:482-491,
// :1162-1168): the sum and the quotient in double, the conversion truncating.
// false for a coordinate the conversion is not defined for (not finite, or
// beyond 1e6 m, which no cube array reaches); the callers drop such a point.
SLIO_HD inline bool cube_of(float t, int cen, int* cube) {
  const double v = (double)t + 25.0;
  if (!(fabs(v) < 1.0e6)) return false;
  int c = (int)(v / 50.0) + cen;
  if (v < 0) --c;
  *cube = c;
  return true;
}

// the host side of slio_lvx_select_cubes (slio_livox.cpp): centre cube, shift
// bookkeeping on cen, the valid and surround lists.  Non-zero: cube_of failed.
int select_host(const float tf[6], int32_t cen[3], int32_t center[3], int32_t shift[3], int32_t* valid,
                int32_t* nvalid, int32_t* surround, int32_t* nsurround);

}  // namespace lvx
}  // namespace slio

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace slio {
namespace lvx {

#if defined(__HIPCC__)
// The search grid over a gathered map (slio_cube_store.hip builds it, k_lvx_pass in
// slio_mapopt.hip reads it): cells of edge h, x fastest, cell of a coordinate
// v = floorf((v - o) * inv_h), the map's points in cells 1 .. n - 3 of every
// axis at least (two cells of padding below, two above), pts sorted by cell
// with .w = bits(index in the gathered map), start = ncells + 1 offsets.
struct GridView {
  const float4* pts;
  const uint32_t* start;
  float o[3], h, inv_h;
  int nx, ny, nz;
  int64_t n;
};
// What a pass leaves per scan point (n = scan size, K = 5 corner / 8 surf):
// world n x 3, nbr_idx / nbr_sqd n x K, coeff, sel, and 28 sums per workgroup
struct PassOut {
  float* world;
  int32_t* nbr_idx;
  float* nbr_sqd;
  float4* coeff;
  uint8_t* sel;
  double* partial;
};
// enqueue k_lvx_pass<kind> (slio_mapopt.hip); tf = transformTobeMapped
int pass_launch(int kind, const GridView& g, const float* body_xyz, int64_t n, const float tf[6], const PassOut& out,
                hipStream_t st);
// the minimum cell edges the exactness argument needs (gates sqrt(1.5), sqrt(5))
constexpr float kCellCorner = 1.25f, kCellSurf = 2.25f;
constexpr float kCellTol = 1.0e-3f;
#endif

}  // namespace lvx
}  // namespace slio
