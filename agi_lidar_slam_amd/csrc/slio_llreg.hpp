// slio_llreg.hpp -- the per-point and per-part formulas of LIO-Livox's
// ScanRegistration for Use_seg = 0 (src/LIO-Livox/src/lio/LidarFeatureExtractor.cpp:
// detectFeaturePoint :93-614, FeatureExtract :1218-1291, FeatureExtract_Mid
// :1352-1401; ScanRegistration.cpp lidarCallBackPc2 :61-93), written once for the
// host restatement (slio_llreg.cpp) and for the kernels (slio_llreg.hip).
// Internal to the library.
//
// A line is m x {x, y, z, intensity} float32, interleaved: the finite points of
// vlines[line] in the message's order.  Every expression keeps the reference's
// type and association order, with the conventions of slio_lreg.hpp, whose
// Vector3d helpers (slio::lreg::V3, diff, dot, norm, normalized, axpy, abs_cos)
// and curvature stencils are used here as they are.
//
// Undefined behaviour in the reference, and what this library does instead:
//  - cloudAngle[] and CloudFeatureFlag[] are stack arrays that are never
//    initialised (:96, :102; :129 zeroes the flag at the index BEFORE the
//    non-finite points are dropped): both are zero before use;
//  - thNumCurvSize is a member that the per-line threads all write (:176-178,
//    :1264-1272): each line uses its own value, in the serial order of its own
//    loops.  The picking loops (:245, :259) therefore run with the K that the
//    line's last loop position m - 6 left behind, whatever the picked point's
//    own K was, and the constructor's NumCurvSize never has an effect (parts
//    are not empty only when the per-point loop has run);
//  - a line of more than 20000 points after ingest overruns the arrays (:96):
//    SLIO_ECAPACITY, nothing is truncated;
//  - a line index >= N_SCANS in the Pc2 path indexes past vlines (:1372): the
//    Pc2 entries want n_scans >= 4 (line = i % 4) and return SLIO_EINVAL
//    otherwise;
//  - an empty message calls points.back() (:1238): zero counts.
// Not built: plane_judge (:473, :512), whose result is dead in both branches.
#pragma once

#include <cmath>
#include <cstdint>

#include "slio_common.hpp"
#include "slio_lreg.hpp"

struct slio_llreg_params;

namespace slio {
namespace llreg {

using lreg::V3;

constexpr int kMaxScans = 6;        // N_SCANS: Used_Line is 1 .. 6
constexpr int kMaxLine = 20000;     // CloudFeatureFlag[20000] (:96)
constexpr int kMaxPoints = kMaxScans * kMaxLine;
// the chain kernel: one workgroup per line, thread t owns the loop positions
// [5 + t * kChainPerThread, 5 + (t + 1) * kChainPerThread)
constexpr int kChainPerThread = 80, kChainThreads = 256, kChainSpan = kChainPerThread * kChainThreads;
static_assert(kChainSpan >= kMaxLine, "one workgroup resolves a line's whole chain");
// the picking kernel: one wavefront per line; a part of up to kPickFast points
// is resolved in registers, lane = position - (sp - 3), so that the three
// positions either side that a neighbour mark can reach are in the window; a
// longer part runs pick_part below on one lane
constexpr int kPickWindow = 64, kPickFast = kPickWindow - 6;
// ingest, features, ranks, flags and collection: kBlk inputs per workgroup
constexpr int kBlk = 256;

// what the per-point pass leaves for the later stages (bits of attr)
enum : uint32_t {
  kCand = 1u << 0,     // cloudCurvature < (thFlatThreshold * cloudDepth)^2 (:241)
  kFar = 1u << 1,      // cloudDepth > thDistanceFaraway (:253, :280)
  kAngle = 1u << 2,    // cloudAngle == 1 (:181)
  kRcand = 1u << 3,    // the reflectivity pick's two tests that need no counter (:290-292)
  kFwdShift = 4,       // 2 bits: pairs (i, i+1), (i+1, i+2), .. without a gap, up to 3
  kBwdShift = 6,       // 2 bits: pairs (i-1, i), (i-2, i-1), .. without a gap, up to 3
  kK3 = 1u << 8,       // thNumCurvSize = 3 here (:174-179)
  kStride4 = 1u << 9,  // right_curvature < thFlatThreshold * depth: count_num = 4 (:347-353)
  kAttrBits = 16,      // the picking kernel's word: attr | curvature rank << 16 | reflectivity rank << 22
};

struct Params {
  int n_scans, lidar_type, num_flat, part_num;
  float far, flat, break_dis, nearest;
};

// ros::Time().fromNSec(t).toSec() (:1238, :1253): sec + 1e-9 * nsec in double
SLIO_HD inline double to_sec(uint32_t offset_time) {
  const uint32_t sec = offset_time / 1000000000u, nsec = offset_time % 1000000000u;
  return (double)sec + 1e-9 * (double)nsec;
}
// :1243-1247 and ScanRegistration.cpp:72-76.  NaN passes both tests.
SLIO_HD inline bool x_kept(float x, int lidar_type) {
  if (lidar_type == 0 || lidar_type == 1) return !(x < 0.01);
  if (lidar_type == 2) return !(fabs(x) < 0.01);
  return true;
}
// pcl_isfinite on the three coordinates (:123): v - v is 0 for a finite v only
SLIO_HD inline bool finite_xyz(float x, float y, float z) { return x - x == 0.0f && y - y == 0.0f && z - z == 0.0f; }

// scanStartInd + (scanEndInd - scanStartInd) * j / thPartNum (:206-208), int
SLIO_HD inline int part_sp(int m, int j, int part_num) { return 5 + (m - 11) * j / part_num; }
SLIO_HD inline int part_ep(int m, int j, int part_num) { return 5 + (m - 11) * (j + 1) / part_num - 1; }
// the part that holds position i, 5 <= i < m - 6 (m >= 12)
SLIO_HD inline int part_of(int m, int i, int part_num) {
  const int D = m - 11;
  int j = (int)((int64_t)(i - 5) * part_num / D);
  if (j > part_num - 1) j = part_num - 1;
  while (j + 1 < part_num && part_sp(m, j + 1, part_num) <= i) ++j;
  while (j > 0 && part_sp(m, j, part_num) > i) --j;
  return j;
}

// (pt_a - pt_cur).dot(pt_cur) / ((pt_a - pt_cur).norm() * pt_cur.norm()), the
// vectors widened BEFORE the subtraction (:160-172).  0 / 0 = NaN for a
// repeated point.
SLIO_HD inline double ray_cos(const float* c, int a, int i) {
  const V3 cur{(double)c[4 * i], (double)c[4 * i + 1], (double)c[4 * i + 2]};
  const V3 d{(double)c[4 * a] - cur.x, (double)c[4 * a + 1] - cur.y, (double)c[4 * a + 2] - cur.z};
  return lreg::dot(d, cur) / (lreg::norm(d) * lreg::norm(cur));
}

// the squared step between neighbours a and b, float (:246-252, :260-266)
SLIO_HD inline bool gap(const float* c, int a, int b) {
  const float dx = c[4 * a] - c[4 * b], dy = c[4 * a + 1] - c[4 * b + 1], dz = c[4 * a + 2] - c[4 * b + 2];
  return dx * dx + dy * dy + dz * dz > 0.02;
}

// The order of the two sorts (:211-232).  The reference swaps neighbours on a
// strict `<`, a stable ascending sort as long as `<` orders the values; a NaN
// (a non-finite intensity on the Pc2 path makes diffR NaN or infinite for the
// points around it; coordinates near FLT_MAX do the same to the curvature)
// leaves its result to the order of the swaps.  Here NaN is one class after
// every number: a strict weak order, so the stable sort is defined, the places
// of a part are always a permutation, and host, device and model agree.
SLIO_HD inline bool sort_before(float a, float b) { return a < b || (a == a && b != b); }
// the place of (v, i) among the part's values: o counts when it sorts before i
SLIO_HD inline bool sorts_ahead(float vo, int o, float vi, int i) {
  return sort_before(vo, vi) || (!sort_before(vi, vo) && o < i);
}

struct Feature {
  float depth, curv, refl;
  uint32_t attr;
};

// The per-point pass (:151-203) at a loop position 5 <= i < m - 5, and the
// right-hand flatness of the line-feature loop (:333-358) at the same i.
SLIO_HD inline Feature point_feature(const float* c, int i, const Params& p) {
  Feature f;
  const float dis = lreg::depth_of(c, i);
  const double angle_last = ray_cos(c, i - 1, i), angle_next = ray_cos(c, i + 1, i);
  const bool steep = fabs(angle_last) > 0.966 && fabs(angle_next) > 0.966;
  const int K = (dis > p.far || steep) ? 2 : 3;
  float d[3] = {0, 0, 0};
  float diffR = -2 * K * c[4 * i + 3];
  for (int j = 1; j <= K; ++j) {
    for (int a = 0; a < 3; ++a) d[a] += c[4 * (i - j) + a] + c[4 * (i + j) + a];
    diffR += c[4 * (i - j) + 3] + c[4 * (i + j) + 3];
  }
  for (int a = 0; a < 3; ++a) d[a] -= 2 * K * c[4 * i + a];
  f.depth = dis;
  f.curv = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  f.refl = diffR;
  uint32_t at = 0;
  if (f.curv < p.flat * dis * p.flat * dis) at |= kCand;
  if (dis > p.far) at |= kFar;
  if (steep) at |= kAngle;
  if (f.curv < 0.7 * p.flat * dis * p.flat * dis && diffR > 20.0) at |= kRcand;
  if (K == 3) at |= kK3;
  if (lreg::right_curvature(c, i) < p.flat * dis) at |= kStride4;
  f.attr = at;
  return f;
}

// how far a neighbour mark travels to position i of a line of m points: the
// number of gap-free pairs from i rightwards (what a pick at i + l must cross
// to reach i, :259-272) and leftwards (:245-258), up to 3
SLIO_HD inline uint32_t reach_bits(const float* c, int i, int m) {
  uint32_t fwd = 0, bwd = 0;
  while (fwd < 3 && i + (int)fwd + 1 < m && !gap(c, i + (int)fwd + 1, i + (int)fwd)) ++fwd;
  while (bwd < 3 && i - (int)bwd - 1 >= 0 && !gap(c, i - (int)bwd - 1, i - (int)bwd)) ++bwd;
  return fwd << kFwdShift | bwd << kBwdShift;
}

// One part of the picking stage after its two sorts (:234-296), as written.
// csort / rsort are cloudSortInd / reflectSortInd; flag is the line's
// CloudFeatureFlag (int32_t on the host, uint16_t in the kernel's LDS); K is
// the line's thNumCurvSize.
template <typename FlagT>
SLIO_HD inline void pick_part(const float* c, const float* curv, const float* depth, const float* refl,
                              const uint16_t* attr, const int* csort, const int* rsort, FlagT* flag, int sp, int ep,
                              int K, const Params& p) {
  int smallestPickedNum = 1, sharpestPickedNum = 1;
  for (int k = sp; k <= ep; ++k) {
    const int ind = csort[k];
    if (flag[ind] != 0) continue;
    if (curv[ind] < p.flat * depth[ind] * p.flat * depth[ind]) {
      flag[ind] = 3;
      for (int l = 1; l <= K; ++l) {
        if (gap(c, ind + l, ind + l - 1) || depth[ind] > p.far) break;
        flag[ind + l] = 1;
      }
      for (int l = -1; l >= -K; --l) {
        if (gap(c, ind + l, ind + l + 1) || depth[ind] > p.far) break;
        flag[ind + l] = 1;
      }
    }
  }
  for (int k = sp; k <= ep; ++k) {
    const int ind = csort[k];
    if ((flag[ind] == 3 && smallestPickedNum <= p.num_flat) || (flag[ind] == 3 && depth[ind] > p.far) ||
        (attr[ind] & kAngle)) {
      ++smallestPickedNum;
      flag[ind] = 2;
    }
    const int idx = rsort[k];
    if (curv[idx] < 0.7 * p.flat * depth[idx] * p.flat * depth[idx] && sharpestPickedNum <= 3 && refl[idx] > 20.0) {
      ++sharpestPickedNum;
      flag[idx] = 300;
    }
  }
}

// The line-feature test of a visited i (:301-403): both sides flat and the
// included angle sharp.  (The right side is attr's kStride4.)
SLIO_HD inline bool line_corner(const float* c, int i, const Params& p) {
  const float depth = lreg::depth_of(c, i);
  return lreg::left_curvature(c, i) < p.flat * depth && lreg::right_curvature(c, i) < p.flat * depth &&
         lreg::surf_surf_corner(c, i);
}

// One turn of the break-point loop (:407-578) at 5 <= i < m - 5: the flag the
// earlier stages left goes in, the final flag comes out.
SLIO_HD inline int break_point(const float* c, int i, int flag, const Params& p) {
  float dr[3], dl[3];
  for (int a = 0; a < 3; ++a) {
    dr[a] = c[4 * (i + 1) + a] - c[4 * i + a];
    dl[a] = c[4 * (i - 1) + a] - c[4 * i + a];
  }
  const float diff_right = sqrtf(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2]);
  const float diff_left = sqrtf(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
  const float depth_right = lreg::depth_of(c, i + 1), depth_left = lreg::depth_of(c, i - 1);
  if (fabs(diff_right - diff_left) > p.break_dis) {
    const bool left = diff_right > diff_left;
    const V3 surf_vector = lreg::diff(c, left ? i - 1 : i + 1, i);
    const V3 lidar_vector{(double)c[4 * i], (double)c[4 * i + 1], (double)c[4 * i + 2]};
    const double cc = lreg::abs_cos(surf_vector, lidar_vector);
    if (cc < 0.95) {
      if (left) {
        if (depth_right > depth_left) flag = 100;
        else if (depth_right == 0) flag = 100;
      } else {
        if (depth_right < depth_left) flag = 100;
        else if (depth_left == 0) flag = 100;
      }
    }
  }
  // break points select (:527-577); temp_depth reads i - k in BOTH loops
  if (flag == 100) {
    V3 norm_front{0, 0, 0}, norm_back{0, 0, 0};
    for (int k = 1; k < 4; ++k) {
      if (lreg::depth_of(c, i - k) < 1) continue;
      lreg::axpy(norm_front, k / 6.0, lreg::normalized(lreg::diff(c, i - k, i)));
    }
    for (int k = 1; k < 4; ++k) {
      if (lreg::depth_of(c, i - k) < 1) continue;
      lreg::axpy(norm_back, k / 6.0, lreg::normalized(lreg::diff(c, i + k, i)));
    }
    const double cc = lreg::abs_cos(norm_front, norm_back);
    if (!(cc < 0.95)) flag = 101;
  }
  return flag;
}

// the collection (:591-613): 1 corner, 2 surf, 0 neither
SLIO_HD inline int label_of(const float* c, int i, int flag, const Params& p) {
  const float dis = c[4 * i] * c[4 * i] + c[4 * i + 1] * c[4 * i + 1] + c[4 * i + 2] * c[4 * i + 2];
  if (dis < p.nearest * p.nearest) return 0;
  if (flag == 2) return 2;
  if (flag == 100 || flag == 150) return 1;
  return 0;
}

// a cloud point: {x, y, z, intensity, normal_x, normal_y, normal_z, curvature = 0}
constexpr int kPointFloats = 8;

// checks the parameters every entry takes; the message goes to set_error
int check_params(const slio_llreg_params* p, const char* who, Params* out);

}  // namespace llreg
}  // namespace slio

#if defined(__HIPCC__)
struct slio_llreg_view;
namespace slio {
namespace llreg {
// What a consumer on the device reads: the three clouds of the handle's last
// run (n x kPointFloats floats each), complete when slio_llreg_run /
// slio_llreg_run_pc2 has returned.  SLIO_EINVAL for a handle that is not live,
// SLIO_ESTATE without a run.
int view(void* handle, slio_llreg_view* v, const char* who);
}  // namespace llreg
}  // namespace slio
#endif
