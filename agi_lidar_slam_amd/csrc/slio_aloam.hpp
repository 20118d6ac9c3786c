// slio_aloam.hpp -- the per-point formulas of A-LOAM's scanRegistration
// (src/A-LOAM/src/scanRegistration.cpp, laserCloudHandler :124-432), written
// once for the host restatement (slio_aloam.cpp) and for the kernels
// (slio_aloam.hip).  Internal to the library.
//
// A cloud is n x {x, y, z, intensity} float32, interleaved.  Every expression
// keeps the reference's type and association order: float sums left to right,
// floats widened where the reference meets a double literal (M_PI, 0.5, 3.0,
// 0.05, 0.1) and rounded back on assignment to a float.  atan2 of two floats
// is the double function rounded to float, as everywhere in this library;
// atan(z / sqrt(..)) is the double function of the float quotient (the
// departure stated in slio_frontend.h).
#pragma once

#include <cmath>
#include <cstdint>

#include "slio_common.hpp"
#include "slio_voxel.hpp"

namespace slio {
namespace aloam {

constexpr int kMaxPoints = 400000;  // cloudCurvature[400000] (:65-68)
constexpr int kMaxScans = 64;
constexpr int kBlk = 256;       // threads (= points) per workgroup of the per-point passes
constexpr int kSortCap = 2048;  // the longest list one LDS sort takes; longer ones are merged in global memory
constexpr int kNumStats = 18;
// per scan: 6 sectors x (2 sharp, 20 less sharp, 4 flat) picks
constexpr int kSharpPerScan = 12, kLessSharpPerScan = 120, kFlatPerScan = 24;

// (x - x is 0 for a finite x and NaN for an infinite or NaN one)
SLIO_HD inline bool finite3(float x, float y, float z) { return x - x == 0.f && y - y == 0.f && z - z == 0.f; }

// removeClosedPointCloud :102-105 (thres is MINIMUM_RANGE as a float)
SLIO_HD inline bool too_close(float x, float y, float z, float thres) { return x * x + y * y + z * z < thres * thres; }

// :177-178
SLIO_HD inline float elevation_deg(float x, float y, float z) {
  const float q = z / sqrtf(x * x + y * y);
  return (float)(atan((double)q) * 180 / M_PI);
}

// the value int() truncates at :183 / :189 / :196 / :198
SLIO_HD inline double scan_value(int n_scans, float angle) {
  if (n_scans == 16) return (double)((angle + 15) / 2) + 0.5;
  if (n_scans == 32) return ((double)angle + 92.0 / 3.0) * 3.0 / 4.0;
  if ((double)angle >= -8.83) return (double)(2 - angle) * 3.0 + 0.5;
  return (-8.83 - (double)angle) * 2.0 + 0.5;
}

// :181-204: the scan id, or -1 for a point the handler drops.  over50 (may be
// null) is set where only the 64-line layout's `scanID > 50` drops it.  A NaN
// elevation (x = y = z = 0 with minimum_range 0) is dropped: int(NaN) is
// undefined in the reference.
SLIO_HD inline int scan_id(int n_scans, float angle, int* over50) {
  if (angle != angle) return -1;
  const double v = scan_value(n_scans, angle);  // |angle| <= 90: v fits an int
  int id = (int)v;
  if (n_scans == 64) {
    if (!((double)angle >= -8.83)) id = n_scans / 2 + id;
    const bool out = angle > 2 || (double)angle < -24.33;
    if (!out && id > 50 && over50) *over50 = 1;
    if (out || id > 50 || id < 0) return -1;
    return id;
  }
  if (id > n_scans - 1 || id < 0) return -1;
  return id;
}

// :155, :212: -atan2(y, x)
SLIO_HD inline float raw_ori(float x, float y) { return -(float)atan2((double)y, (double)x); }

// :156-163 from the raw orientation of the last point.  branch: 0 none, 1 "-= 2 pi", 2 "+= 2 pi"
SLIO_HD inline float end_ori(float start_ori, float raw_last, int* branch) {
  float e = (float)((double)raw_last + 2 * M_PI);
  *branch = 0;
  if ((double)(e - start_ori) > 3 * M_PI) {
    e = (float)((double)e - 2 * M_PI);
    *branch = 1;
  } else if ((double)(e - start_ori) < M_PI) {
    e = (float)((double)e + 2 * M_PI);
    *branch = 2;
  }
  return e;
}

// :215-219.  branch: 0 none, 1 "+= 2 pi", 2 "-= 2 pi"
SLIO_HD inline float first_branch(float ori, float start_ori, int* branch) {
  *branch = 0;
  if ((double)ori < (double)start_ori - M_PI / 2) {
    ori = (float)((double)ori + 2 * M_PI);
    *branch = 1;
  } else if ((double)ori > (double)start_ori + M_PI * 3 / 2) {
    ori = (float)((double)ori - 2 * M_PI);
    *branch = 2;
  }
  return ori;
}
// :221
SLIO_HD inline bool half_passed(float ori1, float start_ori) { return (double)(ori1 - start_ori) > M_PI; }

// :226-231.  branch as above
SLIO_HD inline float second_branch(float ori, float end_ori_, int* branch) {
  *branch = 0;
  ori = (float)((double)ori + 2 * M_PI);
  if ((double)ori < (double)end_ori_ - M_PI * 3 / 2) {
    ori = (float)((double)ori + 2 * M_PI);
    *branch = 1;
  } else if ((double)ori > (double)end_ori_ + M_PI / 2) {
    ori = (float)((double)ori - 2 * M_PI);
    *branch = 2;
  }
  return ori;
}

// :234-236
SLIO_HD inline float intensity_of(int id, float ori, float start_ori, float end_ori_, double scan_period) {
  const float rel = (ori - start_ori) / (end_ori_ - start_ori);
  return (float)((double)id + scan_period * (double)rel);
}

// :255-274: i in [5, n - 5)
SLIO_HD inline float curvature(const float* c, int i) {
  float d[3];
  for (int a = 0; a < 3; ++a) {
    const float* p = c + 4 * i + a;
    d[a] = p[-20] + p[-16] + p[-12] + p[-8] + p[-4] - 10 * p[0] + p[4] + p[8] + p[12] + p[16] + p[20];
  }
  return d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
}

// :341-349 and its three repeats: the squared step from b to a stops the marks
SLIO_HD inline bool gap(const float* c, int a, int b) {
  const float dx = c[4 * a] - c[4 * b], dy = c[4 * a + 1] - c[4 * b + 1], dz = c[4 * a + 2] - c[4 * b + 2];
  return (double)(dx * dx + dy * dy + dz * dz) > 0.05;
}

// :314 / :375: the thresholds against the double literal
SLIO_HD inline bool is_sharp(float curv) { return (double)curv > 0.1; }
SLIO_HD inline bool is_flat(float curv) { return (double)curv < 0.1; }

// :298-300
SLIO_HD inline void sector(int start, int end, int j, int* sp, int* ep) {
  *sp = start + (end - start) * j / 6;
  *ep = start + (end - start) * (j + 1) / 6 - 1;
}

// pcl::VoxelGrid<PointXYZI>::applyFilter's grid from the list's bounding box
// (the restatement the LeGO front-end's per-ring filter uses, slio_lio.hip)
// Kept apart from voxel_geometry (slio_voxel.hpp): float min / max in, no guard for a span that is not finite.
struct Grid {
  float inv;
  int minb[3], mul[3];
  bool overflow;  // "Integer indices would overflow": output = input
};
SLIO_HD inline Grid make_grid(const float mn[3], const float mx[3], float leaf) {
  Grid g;
  g.inv = 1.0f / leaf;
  const int64_t dx = (int64_t)((mx[0] - mn[0]) * g.inv) + 1;
  const int64_t dy = (int64_t)((mx[1] - mn[1]) * g.inv) + 1;
  const int64_t dz = (int64_t)((mx[2] - mn[2]) * g.inv) + 1;
  g.overflow = dx * dy * dz > (int64_t)2147483647;
  int divb[3];
  for (int a = 0; a < 3; ++a) {
    g.minb[a] = (int)floorf(mn[a] * g.inv);
    divb[a] = (int)floorf(mx[a] * g.inv) - g.minb[a] + 1;
  }
  g.mul[0] = 1;
  g.mul[1] = divb[0];
  g.mul[2] = (int)((int64_t)divb[0] * divb[1]);
  return g;
}
SLIO_HD inline uint32_t voxel_of(const Grid& g, float x, float y, float z) {
  return voxel_index(x, y, z, g.inv, g.minb, g.mul);
}

}  // namespace aloam
}  // namespace slio
