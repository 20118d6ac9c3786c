// slio_lreg.hpp -- the per-point formulas of livox_mapping's scanRegistration
// (src/livox_mapping/src/scanRegistration.cpp, laserCloudHandler :152-534),
// written once for the host restatement (slio_lreg.cpp) and for the kernels
// (slio_lreg.hip).  Internal to the library.
//
// A cloud is n x {x, y, z, intensity} float32, interleaved.  Every expression
// keeps the reference's type and association order: float sums left to right,
// float values compared against double literals after widening, and
// Eigen::Vector3d arithmetic with the unrolled 3-term order a0 + (a1 + a2) for
// dot / squaredNorm, true division in normalize(), and Eigen 3.3's
// normalize(), which leaves a zero vector as it is (3.2 would give NaN).
// sqrt of a float is sqrtf (the double function rounded to float is the same
// value); atan2 of two floats is the double function rounded to float, as
// everywhere in this library.
#pragma once

#include <cmath>
#include <cstdint>

#include "slio_common.hpp"
#include "slio_cvsolve.hpp"

namespace slio {
namespace lreg {

constexpr int kMaxPoints = 32000;  // CloudFeatureFlag[32000] (:53, :158)
// the chain kernel: thread t owns the loop positions
// [5 + t * kChainPerThread, 5 + (t + 1) * kChainPerThread), one workgroup all
constexpr int kChainPerThread = 128, kChainThreads = 256, kChainSpan = kChainPerThread * kChainThreads;
static_assert(kChainSpan >= kMaxPoints, "one workgroup resolves the whole chain");

struct V3 {
  double x, y, z;
};

// Eigen::Vector3d(p[a].x - p[b].x, ...): the differences in float, then widened
SLIO_HD inline V3 diff(const float* c, int a, int b) {
  return V3{(double)(c[4 * a] - c[4 * b]), (double)(c[4 * a + 1] - c[4 * b + 1]),
            (double)(c[4 * a + 2] - c[4 * b + 2])};
}
SLIO_HD inline double dot(const V3& a, const V3& b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
SLIO_HD inline double norm(const V3& a) { return sqrt(dot(a, a)); }
SLIO_HD inline V3 normalized(V3 a) {
  const double z = dot(a, a);
  if (z > 0.0) {
    const double s = sqrt(z);
    a.x = a.x / s;
    a.y = a.y / s;
    a.z = a.z / s;
  }
  return a;
}
// acc += w * v
SLIO_HD inline void axpy(V3& acc, double w, const V3& v) {
  acc.x = acc.x + w * v.x;
  acc.y = acc.y + w * v.y;
  acc.z = acc.z + w * v.z;
}
// fabs(a.dot(b) / (a.norm() * b.norm()))
SLIO_HD inline double abs_cos(const V3& a, const V3& b) { return fabs(dot(a, b) / (norm(a) * norm(b))); }

// :166-178: scanID + intensity / 10000 (int + float / int: float)
SLIO_HD inline float scan_intensity(float y, float z, float intensity) {
  const float at = (float)atan2((double)y, (double)z);
  const double theta = (double)at / M_PI * 180 + 180;
  const int scan_id = (int)floor(theta / 9);
  return (float)scan_id + intensity / 10000.0f;
}

SLIO_HD inline float depth_of(const float* c, int i) {
  return sqrtf(c[4 * i] * c[4 * i] + c[4 * i + 1] * c[4 * i + 1] + c[4 * i + 2] * c[4 * i + 2]);
}

// :220-232 (s = -1) and :251-263 (s = +1): p[i+4s] + p[i+3s] - 4 p[i+2s] + p[i+s] + p[i]
SLIO_HD inline float curvature(const float* c, int i, int s) {
  float d[3];
  for (int a = 0; a < 3; ++a)
    d[a] = c[4 * (i + 4 * s) + a] + c[4 * (i + 3 * s) + a] - 4 * c[4 * (i + 2 * s) + a] + c[4 * (i + s) + a] +
           c[4 * i + a];
  return d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
}
SLIO_HD inline float left_curvature(const float* c, int i) { return curvature(c, i, -1); }
SLIO_HD inline float right_curvature(const float* c, int i) { return curvature(c, i, +1); }
// count_num = 4 (:265-280)
SLIO_HD inline bool stride4(const float* c, int i) { return right_curvature(c, i) < 0.01; }

// the weighted direction sums of :286-303 (K = 4, w = 10) and :452-472 (K = 3,
// w = 6): fabs(cos) between sum_k (k / w) normalized(p[i-k] - p[i]) and the
// same over p[i+k]
template <int K>
SLIO_HD inline double fan_cos(const float* c, int i, double w) {
  V3 a{0, 0, 0}, b{0, 0, 0};
  for (int k = 1; k <= K; ++k) axpy(a, k / w, normalized(diff(c, i - k, i)));
  for (int k = 1; k <= K; ++k) axpy(b, k / w, normalized(diff(c, i + k, i)));
  return abs_cos(a, b);
}

// :283-324 once both curvatures are below 0.01
SLIO_HD inline bool surf_surf_corner(const float* c, int i) {
  const double cc = fan_cos<4>(c, i, 10.0);
  const double last_dis = norm(diff(c, i - 4, i)), current_dis = norm(diff(c, i + 4, i));
  return cc < 0.5 && last_dis > 0.05 && current_dis > 0.05;
}

// what a visited i of loop 1 writes (:212-325): bit 0 flag[i-2] = 1, bit 1
// flag[i+2] = 1, bit 2 flag[i] = 150
SLIO_HD inline int loop1_writes(const float* c, int i) {
  const float lc = left_curvature(c, i), rc = right_curvature(c, i);
  int w = 0;
  if (lc < 0.001) w |= 1;
  if (rc < 0.001) w |= 2;
  if (lc < 0.01 && rc < 0.01 && surf_surf_corner(c, i)) w |= 4;
  return w;
}

// plane_judge (:64-120) on num points of stride 4 floats: float centroid and
// covariance in list order, cv::eigen, D[0] > threshold * D[1] (int * float)
SLIO_HD inline bool plane_judge(const float* list, int num, int threshold) {
  float cx = 0, cy = 0, cz = 0;
  for (int j = 0; j < num; ++j) {
    cx += list[4 * j];
    cy += list[4 * j + 1];
    cz += list[4 * j + 2];
  }
  cx /= num;
  cy /= num;
  cz /= num;
  float a11 = 0, a12 = 0, a13 = 0, a22 = 0, a23 = 0, a33 = 0;
  for (int j = 0; j < num; ++j) {
    const float ax = list[4 * j] - cx, ay = list[4 * j + 1] - cy, az = list[4 * j + 2] - cz;
    a11 += ax * ax;
    a12 += ax * ay;
    a13 += ax * az;
    a22 += ay * ay;
    a23 += ay * az;
    a33 += az * az;
  }
  a11 /= num;
  a12 /= num;
  a13 /= num;
  a22 /= num;
  a23 /= num;
  a33 /= num;
  float A[9] = {a11, a12, a13, a12, a22, a23, a13, a23, a33}, D[3], V[9];
  cvs::jacobi<3>(A, D, V);
  return D[0] > threshold * D[1];
}

// branch counters of loop 2, for the tests' fitness conditions
enum { kOutlier = 0, kBreakLeft, kBreakRight, kSet100, kKept100, kReset100, kResetErased, kNumStats };

// One turn of loop 2 (:327-483) at i in [5, N - 5): the flag loop 1 left goes
// in, the final flag comes out.  stats may be null.
SLIO_HD inline int loop2(const float* c, int i, int flag, int* stats) {
  const float depth = depth_of(c, i);
  float dr[3], dl[3];
  for (int a = 0; a < 3; ++a) {
    dr[a] = c[4 * (i + 1) + a] - c[4 * i + a];
    dl[a] = c[4 * (i - 1) + a] - c[4 * i + a];
  }
  const float diff_right = sqrtf(dr[0] * dr[0] + dr[1] * dr[1] + dr[2] * dr[2]);
  const float diff_left = sqrtf(dl[0] * dl[0] + dl[1] * dl[1] + dl[2] * dl[2]);
  const float depth_right = depth_of(c, i + 1), depth_left = depth_of(c, i - 1);
  // outliers (:358)
  if (diff_right > 0.1 * depth && diff_left > 0.1 * depth) {
    if (stats) ++stats[kOutlier];
    return 250;
  }
  const int before = flag;
  // break points (:365-446)
  if (fabs(diff_right - diff_left) > 0.1) {
    const bool left = diff_right > diff_left;
    if (stats) ++stats[left ? kBreakLeft : kBreakRight];
    const int s = left ? -1 : +1;
    const V3 surf_vector = diff(c, i + 4 * s, i);
    const V3 lidar_vector{(double)c[4 * i], (double)c[4 * i + 1], (double)c[4 * i + 2]};
    const double surf_dis = norm(surf_vector);
    const double cc = abs_cos(surf_vector, lidar_vector);
    // the list is p[i], p[i-1], p[i-2], p[i-3] on BOTH sides (:384, :423); the
    // `j == 3` break comes before the update, so three gaps count
    float list[16];
    double min_dis = 10000, max_dis = 0;
    for (int j = 0; j < 4; ++j) {
      for (int a = 0; a < 4; ++a) list[4 * j + a] = c[4 * (i - j) + a];
      if (j == 3) break;
      const double temp_dis = norm(diff(c, i + s * j, i + s * (j + 1)));
      if (temp_dis < min_dis) min_dis = temp_dis;
      if (temp_dis > max_dis) max_dis = temp_dis;
    }
    const bool is_plane = plane_judge(list, 4, 100);
    if (is_plane && max_dis < 2 * min_dis && surf_dis < 0.05 * depth && cc < 0.8) {
      if (left) {
        if (depth_right > depth_left) flag = 100;
        else if (depth_right == 0) flag = 100;
      } else {
        if (depth_right < depth_left) flag = 100;
        else if (depth_left == 0) flag = 100;
      }
    }
  }
  // break point select (:449-482): a point that fails goes back to 0, whatever
  // loop 1 had left there
  if (flag == 100) {
    if (stats) ++stats[kSet100];
    const double cc = fan_cos<3>(c, i, 6.0);
    if (cc < 0.8) {
      if (stats) ++stats[kKept100];
    } else {
      flag = 0;
      if (stats) {
        ++stats[kReset100];
        if (before != 0) ++stats[kResetErased];
      }
    }
  }
  return flag;
}

}  // namespace lreg
}  // namespace slio

#if defined(__HIPCC__)
struct slio_lreg;
namespace slio {
namespace lreg {
// What a consumer on the device (slio_lvx_feed_device) reads: the corner and
// surf clouds of the handle's last run (n x {x, y, z, intensity}), complete
// when slio_lreg_run has returned.  SLIO_EINVAL for a handle that is not live,
// SLIO_ESTATE without a run.
struct View {
  const float* corner_xyzi;
  const float* surf_xyzi;
  int32_t n_corner, n_surf, device;
};
int view(void* handle, View* v, const char* who);
// the device of a live handle (SLIO_EINVAL otherwise), whether it has run or not
int device_of(void* handle, int32_t* device, const char* who);
}  // namespace lreg
}  // namespace slio
#endif
