// slio_llreg.cpp -- LIO-Livox's ScanRegistration for Use_seg = 0 on the host,
// callable without a GPU (src/LIO-Livox/src/lio/LidarFeatureExtractor.cpp:
// FeatureExtract :1218-1291, FeatureExtract_Mid :1352-1401, detectFeaturePoint
// :93-614; ScanRegistration.cpp lidarCallBackPc2 :61-93): the node as its literal
// serial loops over the formulas of slio_llreg.hpp, which the kernels of
// slio_llreg.hip share.  It is what checks the device's parallel picking and
// chain where there is no GPU.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "slio_frontend.h"
#include "slio_llreg.hpp"

using slio::set_error;
using namespace slio::llreg;

namespace slio {
namespace llreg {

int check_params(const slio_llreg_params* p, const char* who, Params* out) {
  const auto fin = [](float v) { return v - v == 0.0f; };
  if (!p || p->n_scans < 1 || p->n_scans > kMaxScans || p->lidar_type < 0 || p->lidar_type > 2 || p->num_flat < 0 ||
      p->part_num < 1 || p->part_num > kMaxLine || !fin(p->distance_faraway) || !fin(p->flat_threshold) ||
      !fin(p->break_corner_dis) || !fin(p->lidar_nearest_dis)) {
    set_error(std::string(who) +
              ": bad parameters (n_scans in 1 .. 6, lidar_type in 0 .. 2, num_flat >= 0, part_num in 1 .. 20000, "
              "finite thresholds)");
    return SLIO_EINVAL;
  }
  out->n_scans = p->n_scans;
  out->lidar_type = p->lidar_type;
  out->num_flat = p->num_flat;
  out->part_num = p->part_num;
  out->far = p->distance_faraway;
  out->flat = p->flat_threshold;
  out->break_dis = p->break_corner_dis;
  out->nearest = p->lidar_nearest_dis;
  return SLIO_OK;
}

}  // namespace llreg
}  // namespace slio

namespace {

struct Outputs {
  float *cloud, *corner, *surf;
  int32_t *counts, *line_size, *finite_size, *flags;
  uint8_t* visited;
  float* lines;
};

// detectFeaturePoint (:93-614) on the m finite points c of one line
void detect(const float* c, int m, const Params& P, int32_t* flag, uint8_t* vis, std::vector<int>& corner,
            std::vector<int>& surf) {
  std::vector<float> curv((size_t)m, 0.f), depth((size_t)m, 0.f), refl((size_t)m, 0.f);
  std::vector<uint16_t> attr((size_t)m, 0);
  std::vector<int> csort((size_t)m, 0), rsort((size_t)m, 0);
  int K = 0;  // (read only once the loop below has run)
  // :151-203
  for (int i = 5; i < m - 5; ++i) {
    const Feature f = point_feature(c, i, P);
    K = (f.attr & kK3) ? 3 : 2;
    depth[i] = f.depth;
    curv[i] = f.curv;
    refl[i] = f.refl;
    attr[i] = (uint16_t)f.attr;
    csort[i] = i;
    rsort[i] = i;
  }
  // :205-297
  for (int j = 0; j < P.part_num; ++j) {
    const int sp = part_sp(m, j, P.part_num), ep = part_ep(m, j, P.part_num);
    for (int k = sp + 1; k <= ep; ++k)
      for (int l = k; l >= sp + 1; --l)
        if (sort_before(curv[csort[l]], curv[csort[l - 1]])) std::swap(csort[l - 1], csort[l]);
    for (int k = sp + 1; k <= ep; ++k)
      for (int l = k; l >= sp + 1; --l)
        if (sort_before(refl[rsort[l]], refl[rsort[l - 1]])) std::swap(rsort[l - 1], rsort[l]);
    pick_part(c, curv.data(), depth.data(), refl.data(), attr.data(), csort.data(), rsort.data(), flag, sp, ep, K, P);
  }
  // :301-403
  int count_num = 1;
  for (int i = 5; i < m - 5; i += count_num) {
    vis[i] = 1;
    count_num = (attr[i] & kStride4) ? 4 : 1;
    if (line_corner(c, i, P)) flag[i] = 150;
  }
  // :407-578
  for (int i = 5; i < m - 5; ++i) flag[i] = break_point(c, i, flag[i], P);
  // :591-613
  for (int i = 5; i < m - 5; ++i) {
    const int lab = label_of(c, i, flag[i], P);
    if (lab == 2) surf.push_back(i);
    if (lab == 1) corner.push_back(i);
  }
}

// FeatureExtract / FeatureExtract_Mid from the ingested cloud on: cloud is the
// kept points (8 floats each, normal_z = 0), line_of their lines
int extract(const Params& P, std::vector<float>& cloud, const std::vector<int>& line_of, const Outputs& o,
            const char* who) {
  const int n = (int)line_of.size();
  // :1258-1263
  std::vector<std::vector<int>> vlines((size_t)kMaxScans);
  for (int i = 0; i < n; ++i) vlines[(size_t)line_of[i]].push_back(i);
  for (int l = 0; l < kMaxScans; ++l)
    if ((int)vlines[(size_t)l].size() > kMaxLine) {
      set_error(std::string(who) + ": a line of more than 20000 points");
      return SLIO_ECAPACITY;
    }
  int done = 0;
  for (int l = 0; l < kMaxScans; ++l) {
    const std::vector<int>& vl = vlines[(size_t)l];
    // :112-130
    std::vector<float> c;
    c.reserve(4 * vl.size());
    for (int ci : vl) {
      const float* q = &cloud[(size_t)kPointFloats * ci];
      if (!finite_xyz(q[0], q[1], q[2])) continue;
      c.insert(c.end(), q, q + 4);
    }
    const int m = (int)(c.size() / 4);
    std::vector<int32_t> flag((size_t)m, 0);
    std::vector<uint8_t> vis((size_t)m, 0);
    std::vector<int> corner, surf;
    detect(c.data(), m, P, flag.data(), vis.data(), corner, surf);
    // :1273-1283: idx counts the line's finite points, vlines[l] all of them
    for (int idx : corner) cloud[(size_t)kPointFloats * vl[(size_t)idx] + 6] = 1.0f;
    for (int idx : surf) cloud[(size_t)kPointFloats * vl[(size_t)idx] + 6] = 2.0f;
    if (o.line_size) o.line_size[l] = (int32_t)vl.size();
    if (o.finite_size) o.finite_size[l] = m;
    if (m) {
      if (o.flags) std::memcpy(o.flags + done, flag.data(), 4 * (size_t)m);
      if (o.visited) std::memcpy(o.visited + done, vis.data(), (size_t)m);
      if (o.lines) std::memcpy(o.lines + 4 * (size_t)done, c.data(), 16 * (size_t)m);
    }
    done += m;
  }
  // :1285-1290
  int nc = 0, ns = 0;
  for (int i = 0; i < n; ++i) {
    const float* q = &cloud[(size_t)kPointFloats * i];
    if (std::fabs(q[6] - 1.0) < 1e-5) {
      if (o.corner) std::memcpy(o.corner + (size_t)kPointFloats * nc, q, 4 * kPointFloats);
      ++nc;
    }
  }
  for (int i = 0; i < n; ++i) {
    const float* q = &cloud[(size_t)kPointFloats * i];
    if (std::fabs(q[6] - 2.0) < 1e-5) {
      if (o.surf) std::memcpy(o.surf + (size_t)kPointFloats * ns, q, 4 * kPointFloats);
      ++ns;
    }
  }
  if (n && o.cloud) std::memcpy(o.cloud, cloud.data(), 4 * (size_t)kPointFloats * n);
  o.counts[0] = n;
  o.counts[1] = nc;
  o.counts[2] = ns;
  return SLIO_OK;
}

}  // namespace

extern "C" {

int slio_llreg_extract_host(const slio_llreg_params* p, const float* xyz, const uint8_t* reflectivity,
                            const uint8_t* line, const uint32_t* offset_time, int64_t n, float* cloud, float* corner,
                            float* surf, int32_t counts[3], int32_t* line_size, int32_t* finite_size, int32_t* flags,
                            uint8_t* visited, float* lines) {
  Params P;
  const int rc = check_params(p, "slio_llreg_extract_host", &P);
  if (rc) return rc;
  if (n < 0 || n > kMaxPoints || (n && (!xyz || !reflectivity || !line || !offset_time)) || !counts) {
    set_error("slio_llreg_extract_host: size outside 0 .. 120000, null array or null counts");
    return n > kMaxPoints ? SLIO_ECAPACITY : SLIO_EINVAL;
  }
  // :1237-1256
  std::vector<float> pts;
  std::vector<int> line_of;
  const double timeSpan = n ? to_sec(offset_time[n - 1]) : 0.0;
  for (int64_t i = 0; i < n; ++i) {
    const int line_num = (int)line[i];
    if (line_num > P.n_scans - 1) continue;
    if (!x_kept(xyz[3 * i], P.lidar_type)) continue;
    float q[kPointFloats] = {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (float)reflectivity[i],
                             (float)(to_sec(offset_time[i]) / timeSpan), 0.f, 0.f, 0.f};
    const int32_t bits = line_num;  // _int_as_float (:1254)
    std::memcpy(&q[5], &bits, 4);
    pts.insert(pts.end(), q, q + kPointFloats);
    line_of.push_back(line_num);
  }
  return extract(P, pts, line_of, Outputs{cloud, corner, surf, counts, line_size, finite_size, flags, visited, lines},
                 "slio_llreg_extract_host");
}

int slio_llreg_extract_pc2_host(const slio_llreg_params* p, const float* xyzi, int64_t n, float* cloud, float* corner,
                                float* surf, int32_t counts[3], int32_t* line_size, int32_t* finite_size,
                                int32_t* flags, uint8_t* visited, float* lines) {
  Params P;
  const int rc = check_params(p, "slio_llreg_extract_pc2_host", &P);
  if (rc) return rc;
  if (P.n_scans < 4) {
    set_error("slio_llreg_extract_pc2_host: line = i % 4 needs n_scans >= 4");
    return SLIO_EINVAL;
  }
  if (n < 0 || n > kMaxPoints || (n && !xyzi) || !counts) {
    set_error("slio_llreg_extract_pc2_host: size outside 0 .. 120000, null cloud or null counts");
    return n > kMaxPoints ? SLIO_ECAPACITY : SLIO_EINVAL;
  }
  // ScanRegistration.cpp:69-84
  std::vector<float> pts;
  std::vector<int> line_of;
  for (int64_t i = 0; i < n; ++i) {
    if (!x_kept(xyzi[4 * i], P.lidar_type)) continue;
    const float q[kPointFloats] = {xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], xyzi[4 * i + 3],
                                   (float)i / (float)n,  (float)(i % 4),  0.f,             0.f};
    pts.insert(pts.end(), q, q + kPointFloats);
    line_of.push_back((int)(i % 4));
  }
  return extract(P, pts, line_of, Outputs{cloud, corner, surf, counts, line_size, finite_size, flags, visited, lines},
                 "slio_llreg_extract_pc2_host");
}

int slio_llreg_tiles(int32_t* chain_per_thread, int32_t* chain_per_workgroup, int32_t* pick_fast, int32_t* block) {
  if (!chain_per_thread || !chain_per_workgroup || !pick_fast || !block) {
    set_error("slio_llreg_tiles: null output");
    return SLIO_EINVAL;
  }
  *chain_per_thread = kChainPerThread;
  *chain_per_workgroup = kChainSpan;
  *pick_fast = kPickFast;
  *block = kBlk;
  return SLIO_OK;
}

int slio_llreg_params_default(slio_llreg_params* p) {
  if (!p) {
    set_error("slio_llreg_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->device = 0;
  p->max_points = kMaxPoints;
  p->n_scans = 6;
  p->lidar_type = 0;
  p->num_curv_size = 2;
  p->num_flat = 3;
  p->part_num = 150;
  p->distance_faraway = 100.0f;
  p->flat_threshold = 0.02f;
  p->break_corner_dis = 1.0f;
  p->lidar_nearest_dis = 1.0f;
  p->kdtree_corner_outlier_dis = 0.2f;
  return SLIO_OK;
}

}  // extern "C"
