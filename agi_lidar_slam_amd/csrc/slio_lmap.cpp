// slio_lmap.cpp -- the host formulas of LeGO-LOAM's mapping back-end
// (src/LeGO-LOAM/LeGO-LOAM/src/mapOptmization.cpp, transformFusion.cpp),
// callable without a GPU: transformAssociateToMap (written once, used by the
// mapper and by transformFusion), transformUpdate, transformFusion's two
// handlers and saveKeyFramesAndFactor's decision.  Float arithmetic in the
// reference's expression order; sin / cos / atan2 / asin of a float are the
// double functions rounded to float, as everywhere in this project.
//
// Stated departure: the key pose is transformTobeMapped itself.  The
// reference passes it through an iSAM2 chain of one prior and successive
// between-factors (mapOptmization.cpp:1656-1749); without loop closures that
// chain's optimum is the composed odometry, so GTSAM returns the same pose up
// to its own rounding.  GTSAM is third-party and absent.
#include <cmath>
#include <cstring>

#include "slio.h"
#include "slio_common.hpp"
#include "slio_cvsolve.hpp"

using slio::set_error;

namespace {

using slio::fcos;
using slio::fsin;
inline float fasin(float a) { return (float)std::asin((double)a); }
inline float fatan2(float y, float x) { return (float)std::atan2((double)y, (double)x); }

// mapOptmization.cpp:394-519 == transformFusion.cpp:91-215
void associate_to_map(const float ts[6], const float tb[6], const float ta[6], float tm[6]) {
  float x1 = fcos(ts[1]) * (tb[3] - ts[3]) - fsin(ts[1]) * (tb[5] - ts[5]);
  float y1 = tb[4] - ts[4];
  float z1 = fsin(ts[1]) * (tb[3] - ts[3]) + fcos(ts[1]) * (tb[5] - ts[5]);

  float x2 = x1;
  float y2 = fcos(ts[0]) * y1 + fsin(ts[0]) * z1;
  float z2 = -fsin(ts[0]) * y1 + fcos(ts[0]) * z1;

  float ti[6];
  ti[3] = fcos(ts[2]) * x2 + fsin(ts[2]) * y2;
  ti[4] = -fsin(ts[2]) * x2 + fcos(ts[2]) * y2;
  ti[5] = z2;

  const float sbcx = fsin(ts[0]), cbcx = fcos(ts[0]);
  const float sbcy = fsin(ts[1]), cbcy = fcos(ts[1]);
  const float sbcz = fsin(ts[2]), cbcz = fcos(ts[2]);

  const float sblx = fsin(tb[0]), cblx = fcos(tb[0]);
  const float sbly = fsin(tb[1]), cbly = fcos(tb[1]);
  const float sblz = fsin(tb[2]), cblz = fcos(tb[2]);

  const float salx = fsin(ta[0]), calx = fcos(ta[0]);
  const float saly = fsin(ta[1]), caly = fcos(ta[1]);
  const float salz = fsin(ta[2]), calz = fcos(ta[2]);

  const float srx = -sbcx * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz) -
                    cbcx * sbcy *
                        (calx * calz * (cbly * sblz - cblz * sblx * sbly) -
                         calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly) -
                    cbcx * cbcy *
                        (calx * salz * (cblz * sbly - cbly * sblx * sblz) -
                         calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx);
  tm[0] = -fasin(srx);

  const float srycrx = sbcx * (cblx * cblz * (caly * salz - calz * salx * saly) -
                               cblx * sblz * (caly * calz + salx * saly * salz) + calx * saly * sblx) -
                       cbcx * cbcy *
                           ((caly * calz + salx * saly * salz) * (cblz * sbly - cbly * sblx * sblz) +
                            (caly * salz - calz * salx * saly) * (sbly * sblz + cbly * cblz * sblx) -
                            calx * cblx * cbly * saly) +
                       cbcx * sbcy *
                           ((caly * calz + salx * saly * salz) * (cbly * cblz + sblx * sbly * sblz) +
                            (caly * salz - calz * salx * saly) * (cbly * sblz - cblz * sblx * sbly) +
                            calx * cblx * saly * sbly);
  const float crycrx = sbcx * (cblx * sblz * (calz * saly - caly * salx * salz) -
                               cblx * cblz * (saly * salz + caly * calz * salx) + calx * caly * sblx) +
                       cbcx * cbcy *
                           ((saly * salz + caly * calz * salx) * (sbly * sblz + cbly * cblz * sblx) +
                            (calz * saly - caly * salx * salz) * (cblz * sbly - cbly * sblx * sblz) +
                            calx * caly * cblx * cbly) -
                       cbcx * sbcy *
                           ((saly * salz + caly * calz * salx) * (cbly * sblz - cblz * sblx * sbly) +
                            (calz * saly - caly * salx * salz) * (cbly * cblz + sblx * sbly * sblz) -
                            calx * caly * cblx * sbly);
  tm[1] = fatan2(srycrx / fcos(tm[0]), crycrx / fcos(tm[0]));

  const float srzcrx = (cbcz * sbcy - cbcy * sbcx * sbcz) *
                           (calx * salz * (cblz * sbly - cbly * sblx * sblz) -
                            calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx) -
                       (cbcy * cbcz + sbcx * sbcy * sbcz) *
                           (calx * calz * (cbly * sblz - cblz * sblx * sbly) -
                            calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly) +
                       cbcx * sbcz * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz);
  const float crzcrx = (cbcy * sbcz - cbcz * sbcx * sbcy) *
                           (calx * calz * (cbly * sblz - cblz * sblx * sbly) -
                            calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly) -
                       (sbcy * sbcz + cbcy * cbcz * sbcx) *
                           (calx * salz * (cblz * sbly - cbly * sblx * sblz) -
                            calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx) +
                       cbcx * cbcz * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz);
  tm[2] = fatan2(srzcrx / fcos(tm[0]), crzcrx / fcos(tm[0]));

  x1 = fcos(tm[2]) * ti[3] - fsin(tm[2]) * ti[4];
  y1 = fsin(tm[2]) * ti[3] + fcos(tm[2]) * ti[4];
  z1 = ti[5];

  x2 = x1;
  y2 = fcos(tm[0]) * y1 - fsin(tm[0]) * z1;
  z2 = fsin(tm[0]) * y1 + fcos(tm[0]) * z1;

  tm[3] = ta[3] - (fcos(tm[1]) * x2 + fsin(tm[1]) * z2);
  tm[4] = ta[4] - y2;
  tm[5] = ta[5] - (-fsin(tm[1]) * x2 + fcos(tm[1]) * z2);
}

// pcl::getTransformation (pcl/common/impl/eigen.hpp) in float: rows 0..2 of the affine
void get_transformation(float x, float y, float z, float roll, float pitch, float yaw, float t[12]) {
  const float A = fcos(yaw), B = fsin(yaw), C = fcos(pitch), D = fsin(pitch), E = fcos(roll), F = fsin(roll),
              DE = D * E, DF = D * F;
  t[0] = A * C, t[1] = A * DF - B * E, t[2] = B * F + A * DE, t[3] = x;
  t[4] = B * C, t[5] = A * E + B * DF, t[6] = B * DE - A * F, t[7] = y;
  t[8] = -D, t[9] = C * F, t[10] = C * E, t[11] = z;
}

// pcl::getTranslationAndEulerAngles
void translation_and_euler(const float t[12], float& x, float& y, float& z, float& roll, float& pitch, float& yaw) {
  x = t[3];
  y = t[7];
  z = t[11];
  roll = fatan2(t[9], t[10]);
  pitch = fasin(-t[8]);
  yaw = fatan2(t[4], t[0]);
}

}  // namespace

extern "C" {

int slio_lmap_associate_to_map(const float transform_sum[6], const float transform_bef_mapped[6],
                               const float transform_aft_mapped[6], float transform_tobe_mapped[6]) {
  if (!transform_sum || !transform_bef_mapped || !transform_aft_mapped || !transform_tobe_mapped) {
    set_error("slio_lmap_associate_to_map: null argument");
    return SLIO_EINVAL;
  }
  float out[6];
  associate_to_map(transform_sum, transform_bef_mapped, transform_aft_mapped, out);
  std::memcpy(transform_tobe_mapped, out, sizeof(out));
  return SLIO_OK;
}

int slio_lmap_transform_update(float tm[6], const float transform_sum[6], double time_odometry, float scan_period,
                               const double* imu_time, const float* imu_roll, const float* imu_pitch,
                               int32_t imu_len, int32_t imu_last, int32_t* imu_front, float bef[6], float aft[6]) {
  if (!tm || !transform_sum || !bef || !aft) {
    set_error("slio_lmap_transform_update: null argument");
    return SLIO_EINVAL;
  }
  if (imu_last >= 0 && (!imu_time || !imu_roll || !imu_pitch || !imu_front || imu_len < 1 || imu_last >= imu_len ||
                        *imu_front < 0 || *imu_front >= imu_len)) {
    set_error("slio_lmap_transform_update: bad IMU ring");
    return SLIO_EINVAL;
  }
  if (imu_last >= 0) {  // :522-554
    float imuRollLast = 0, imuPitchLast = 0;
    int front = *imu_front;
    while (front != imu_last) {
      if (time_odometry + scan_period < imu_time[front]) break;
      front = (front + 1) % imu_len;
    }
    if (time_odometry + scan_period > imu_time[front]) {
      imuRollLast = imu_roll[front];
      imuPitchLast = imu_pitch[front];
    } else {
      const int back = (front + imu_len - 1) % imu_len;
      const float ratioFront =
          (float)((time_odometry + scan_period - imu_time[back]) / (imu_time[front] - imu_time[back]));
      const float ratioBack =
          (float)((imu_time[front] - time_odometry - scan_period) / (imu_time[front] - imu_time[back]));
      imuRollLast = imu_roll[front] * ratioFront + imu_roll[back] * ratioBack;
      imuPitchLast = imu_pitch[front] * ratioFront + imu_pitch[back] * ratioBack;
    }
    tm[0] = (float)(0.998 * tm[0] + 0.002 * imuPitchLast);
    tm[2] = (float)(0.998 * tm[2] + 0.002 * imuRollLast);
    *imu_front = front;
  }
  for (int i = 0; i < 6; ++i) {
    bef[i] = transform_sum[i];
    aft[i] = tm[i];
  }
  return SLIO_OK;
}

int slio_lmap_fuse(slio_lmap_fusion* f, const float transform_sum[6], const float aft_mapped[6],
                   const float bef_mapped[6]) {
  if (!f || (!transform_sum && !(aft_mapped && bef_mapped)) || (transform_sum && (aft_mapped || bef_mapped))) {
    set_error("slio_lmap_fuse: give either transform_sum or aft_mapped and bef_mapped");
    return SLIO_EINVAL;
  }
  if (transform_sum) {  // laserOdometryHandler (transformFusion.cpp:217-254)
    std::memcpy(f->transform_sum, transform_sum, 24);
    associate_to_map(f->transform_sum, f->transform_bef_mapped, f->transform_aft_mapped, f->transform_mapped);
  } else {  // odomAftMappedHandler (:256-277)
    std::memcpy(f->transform_aft_mapped, aft_mapped, 24);
    std::memcpy(f->transform_bef_mapped, bef_mapped, 24);
  }
  return SLIO_OK;
}

int slio_lmap_keyframe_decision(const float prev_pos[3], const float cur_pos[3], int32_t nkeys, double distance,
                                int* save) {
  if (!prev_pos || !cur_pos || !save || nkeys < 0) {
    set_error("slio_lmap_keyframe_decision: bad arguments");
    return SLIO_EINVAL;
  }
  // :1633-1643
  const float dx = prev_pos[0] - cur_pos[0], dy = prev_pos[1] - cur_pos[1], dz = prev_pos[2] - cur_pos[2];
  const float d = std::sqrt(dx * dx + dy * dy + dz * dz);
  bool save_this = true;
  if ((double)d < distance) save_this = false;
  *save = (save_this || nkeys == 0) ? 1 : 0;
  return SLIO_OK;
}

int slio_lmap_detect_loop(const float* key_xyz, const double* key_time, int32_t nkeys, const float cur_pos[3],
                          double t, float radius, double time_diff, int32_t* closest) {
  if (!closest || !cur_pos || nkeys < 0 || (nkeys > 0 && (!key_xyz || !key_time)) || !(radius >= 0.0f) ||
      !(time_diff >= 0.0)) {
    set_error("slio_lmap_detect_loop: bad arguments");
    return SLIO_EINVAL;
  }
  // :871-883: the radius search's results in ascending squared distance (equal
  // distances: the lower key); the first one far enough in time wins.  Picking
  // the smallest (distance, key) among the keys that pass both tests is the
  // same key.
  *closest = -1;
  const float r2 = radius * radius;
  float best = 0.0f;
  for (int32_t k = 0; k < nkeys; ++k) {
    const float dx = key_xyz[3 * k] - cur_pos[0], dy = key_xyz[3 * k + 1] - cur_pos[1],
                dz = key_xyz[3 * k + 2] - cur_pos[2];
    const float d = (dx * dx + dy * dy) + dz * dz;
    if (!(d < r2)) continue;
    if (!(std::fabs(key_time[k] - t) > time_diff)) continue;
    if (*closest < 0 || d < best) {
      *closest = k;
      best = d;
    }
  }
  return SLIO_OK;
}

int slio_lmap_loop_correction(const float final_T[16], const float latest_pose6[6], const float closest_pose6[6],
                              double fitness, float pose_from[6], float pose_to[6], float* noise) {
  if (!final_T || !latest_pose6 || !closest_pose6 || !pose_from || !pose_to || !noise) {
    set_error("slio_lmap_loop_correction: null argument");
    return SLIO_EINVAL;
  }
  float x, y, z, roll, pitch, yaw;
  translation_and_euler(final_T, x, y, z, roll, pitch, yaw);  // :994-997 (rows 0..2 of the 4x4)
  float corr[12], wrong[12], ok[12];
  get_transformation(z, x, y, yaw, roll, pitch, corr);  // correctionLidarFrame (:998-999)
  const float* p = latest_pose6;                        // {rx, ry, rz, tx, ty, tz} = {roll, pitch, yaw, x, y, z}
  get_transformation(p[5], p[3], p[4], p[2], p[0], p[1], wrong);  // tWrong (:1032-1036)
  // tCorrect = correctionLidarFrame * tWrong (:1002), an affine product:
  // linear = L1 L2, translation = L1 t2 + t1, every sum in index order
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c)
      ok[4 * r + c] = (corr[4 * r] * wrong[c] + corr[4 * r + 1] * wrong[4 + c]) + corr[4 * r + 2] * wrong[8 + c];
    ok[4 * r + 3] =
        ((corr[4 * r] * wrong[3] + corr[4 * r + 1] * wrong[7]) + corr[4 * r + 2] * wrong[11]) + corr[4 * r + 3];
  }
  translation_and_euler(ok, x, y, z, roll, pitch, yaw);  // :1003
  const float from[6] = {x, y, z, roll, pitch, yaw};
  const float* q = closest_pose6;
  const float to[6] = {q[5], q[3], q[4], q[2], q[0], q[1]};  // pclPointTogtsamPose3 (:1025-1030)
  std::memcpy(pose_from, from, sizeof(from));
  std::memcpy(pose_to, to, sizeof(to));
  *noise = (float)fitness;  // float noiseScore = icp.getFitnessScore() (:1009)
  return SLIO_OK;
}

int slio_lmap_qr_solve(int m, int n, const float* A, const float* b, float* x) {
  if (!A || !b || !x) {
    set_error("slio_lmap_qr_solve: null argument");
    return SLIO_EINVAL;
  }
  bool ok;
  if (m == 5 && n == 3) {
    ok = slio::cvs::qr_solve_mn<5, 3>(A, b, x);
  } else if (m == 3 && n == 3) {
    ok = slio::cvs::qr_solve<3>(A, b, x);
  } else if (m == 6 && n == 6) {
    ok = slio::cvs::qr_solve<6>(A, b, x);
  } else {
    set_error("slio_lmap_qr_solve: (m, n) must be (5, 3), (3, 3) or (6, 6)");
    return SLIO_EINVAL;
  }
  if (!ok)
    for (int i = 0; i < n; ++i) x[i] = 0.0f;
  return ok ? SLIO_OK : 1;
}

}  // extern "C"
