// slio_lego_odom.hpp -- what the LeGO-LOAM front-end (slio_lio.hip) and its
// scan-to-scan odometry (slio_lego_odom.hip) share: the IMU state
// adjustDistortion leaves on the device, and a view of the handle's feature
// clouds.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

struct slio_lego;

namespace slio {
namespace lego {

struct LegoImuOutDev {
  float rpy_start[3], rpy_cur[3], velo_from_start[3], angular_from_start[3], ang_last[3];
};

struct LegoOdom;  // slio_lego_odom.hip

struct LegoOdomView {
  int device;
  hipStream_t stream;
  int64_t cap_corner, cap_flat, cap_surf;  // points: sharp / less sharp, flat, less flat
  float4 *c_sharp, *c_flat;
  float4 **c_less_sharp, **c_less_flat;  // swapped by pointer against the last clouds
  const float4* outlier;
  const int32_t* nseg;    // [1]: outlier points
  int64_t* counts;        // n_sharp, n_less_sharp, n_flat, n_less_flat
  const LegoImuOutDev* io;
  bool* ran;              // a sweep has been enqueued since the last upload
  bool* odom_fresh;       // ... and the odometry has not consumed it yet
  LegoOdom** odom;
};

void lego_odom_view(slio_lego* h, LegoOdomView* v);  // slio_lio.hip
void lego_odom_free(LegoOdom* o);                    // slio_lego_odom.hip

}  // namespace lego
}  // namespace slio
