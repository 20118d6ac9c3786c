// slio_lreg.cpp -- livox_mapping's scanRegistration on the host, callable
// without a GPU (src/livox_mapping/src/scanRegistration.cpp, laserCloudHandler
// :152-534): the handler as its literal serial loops over the formulas of
// slio_lreg.hpp, which the kernels of slio_lreg.hip share.  It is what checks
// the device's parallel chain where there is no GPU.
#include <cmath>
#include <cstring>
#include <vector>

#include "slio_frontend.h"
#include "slio_lreg.hpp"

using slio::set_error;
using namespace slio::lreg;

extern "C" {

int slio_lreg_classify_host(const float* xyzi, int64_t n, int32_t* flags, uint8_t* visited, float* cloud,
                            float* corner, float* surf, int32_t counts[3], int32_t* stats) {
  if (n < 0 || (n && !xyzi) || !counts) {
    set_error("slio_lreg_classify_host: negative size, null cloud or null counts");
    return SLIO_EINVAL;
  }
  // :157-187: the first 32000 points, the finite ones, with the new intensity
  const int cap = (int)(n < kMaxPoints ? n : kMaxPoints);
  std::vector<float> pts;
  pts.reserve(4 * (size_t)cap);
  for (int i = 0; i < cap; ++i) {
    const float x = xyzi[4 * i], y = xyzi[4 * i + 1], z = xyzi[4 * i + 2];
    if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) continue;
    pts.push_back(x);
    pts.push_back(y);
    pts.push_back(z);
    pts.push_back(scan_intensity(y, z, xyzi[4 * i + 3]));
  }
  const int N = (int)(pts.size() / 4);
  const float* c = pts.data();
  std::vector<int32_t> flag((size_t)N, 0);
  std::vector<uint8_t> vis((size_t)N, 0);
  int32_t st[5 + kNumStats] = {0};
  // loop 1 (:212-325)
  int count_num = 1;
  for (int i = 5; i < N - 5; i += count_num) {
    vis[i] = 1;
    const int w = loop1_writes(c, i);
    if (w & 1) flag[i - 2] = 1, ++st[2];
    if (w & 2) flag[i + 2] = 1, ++st[3];
    count_num = stride4(c, i) ? 4 : 1;
    ++st[count_num == 4 ? 1 : 0];
    if (w & 4) flag[i] = 150, ++st[4];
  }
  // loop 2 (:327-483)
  for (int i = 5; i < N - 5; ++i) flag[i] = loop2(c, i, flag[i], st + 5);
  // :486-508
  int ns = 0, nc = 0;
  for (int i = 0; i < N; ++i) {
    if (flag[i] == 1) {
      if (surf) std::memcpy(surf + 4 * ns, c + 4 * i, 16);
      ++ns;
    } else if (flag[i] == 100 || flag[i] == 150) {
      if (corner) std::memcpy(corner + 4 * nc, c + 4 * i, 16);
      ++nc;
    }
  }
  if (N) {
    if (flags) std::memcpy(flags, flag.data(), 4 * (size_t)N);
    if (visited) std::memcpy(visited, vis.data(), (size_t)N);
    if (cloud) std::memcpy(cloud, c, 16 * (size_t)N);
  }
  counts[0] = N;
  counts[1] = nc;
  counts[2] = ns;
  if (stats) std::memcpy(stats, st, sizeof st);
  return SLIO_OK;
}

int slio_lreg_plane_judge(const float* xyz, int32_t num, int32_t threshold, int32_t* is_plane) {
  if (!xyz || !is_plane || num < 1 || num > 64) {
    set_error("slio_lreg_plane_judge: null argument or a list outside 1 .. 64 points");
    return SLIO_EINVAL;
  }
  float list[4 * 64];
  for (int j = 0; j < num; ++j) {
    for (int a = 0; a < 3; ++a) list[4 * j + a] = xyz[3 * j + a];
    list[4 * j + 3] = 0.0f;
  }
  *is_plane = plane_judge(list, num, threshold) ? 1 : 0;
  return SLIO_OK;
}

int slio_lreg_chain_tile(int32_t* per_thread, int32_t* per_workgroup) {
  if (!per_thread || !per_workgroup) {
    set_error("slio_lreg_chain_tile: null output");
    return SLIO_EINVAL;
  }
  *per_thread = kChainPerThread;
  *per_workgroup = kChainSpan;
  return SLIO_OK;
}

int slio_lreg_params_default(slio_lreg_params* p) {
  if (!p) {
    set_error("slio_lreg_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->device = 0;
  p->max_points = kMaxPoints;
  return SLIO_OK;
}

}  // extern "C"
