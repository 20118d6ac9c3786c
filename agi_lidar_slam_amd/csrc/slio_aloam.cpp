// slio_aloam.cpp -- A-LOAM's scanRegistration on the host, callable without a
// GPU (src/A-LOAM/src/scanRegistration.cpp, laserCloudHandler :124-432): the
// handler as its literal serial loops over the formulas of slio_aloam.hpp,
// which the kernels of slio_aloam.hip share.  It is what checks the device's
// parallel restatement where there is no GPU.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "slio_aloam.hpp"
#include "slio_frontend.h"

using slio::set_error;
using namespace slio::aloam;

namespace {

enum {
  kDropNonFinite, kDropRange, kDropScan, kDropOver50, kEndMinus, kEndPlus, kFirstPlus, kFirstMinus, kSecondPlus,
  kSecondMinus, kHalfPassed, kScansSkipped, kBreak21, kFlat, kBreak4, kSeamMarks, kSeamSuppressed, kVgOverflow
};
static_assert(kVgOverflow + 1 == kNumStats, "stats");

struct Picker {
  const float* c;
  std::vector<int>& picked;
  std::vector<int>& origin;  // the sector (scan * 6 + j) that set the mark first
  int32_t* st;
  int sp, ep, sec;
  void mark(int q) {
    if (!picked[q]) origin[q] = sec;
    picked[q] = 1;
    if (q < sp || q > ep) ++st[kSeamMarks];
  }
  // :340-366
  void neighbours(int ind) {
    for (int l = 1; l <= 5; ++l) {
      if (gap(c, ind + l, ind + l - 1)) break;
      mark(ind + l);
    }
    for (int l = -1; l >= -5; --l) {
      if (gap(c, ind + l, ind + l + 1)) break;
      mark(ind + l);
    }
  }
};

// pcl::VoxelGrid<PointXYZI> at leaf 0.2 over the points list[0 .. m) of c
void voxel_grid(const float* c, const std::vector<int>& list, std::vector<float>& out, int32_t* st) {
  const int m = (int)list.size();
  if (!m) return;
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int q : list)
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], c[4 * q + a]);
      mx[a] = fmaxf(mx[a], c[4 * q + a]);
    }
  const Grid g = make_grid(mn, mx, 0.2f);
  if (g.overflow) {
    ++st[kVgOverflow];
    for (int q : list) out.insert(out.end(), c + 4 * q, c + 4 * q + 4);
    return;
  }
  std::vector<uint32_t> vox((size_t)m);
  for (int k = 0; k < m; ++k) vox[k] = voxel_of(g, c[4 * list[k]], c[4 * list[k] + 1], c[4 * list[k] + 2]);
  std::vector<int> ord((size_t)m);
  std::iota(ord.begin(), ord.end(), 0);
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return vox[a] < vox[b]; });
  for (int k = 0; k < m;) {
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    int e = k;
    for (; e < m && vox[ord[e]] == vox[ord[k]]; ++e)
      for (int a = 0; a < 4; ++a) s[a] += c[4 * list[ord[e]] + a];
    const float cnt = (float)(e - k);
    for (int a = 0; a < 4; ++a) out.push_back(s[a] / cnt);
    k = e;
  }
}

}  // namespace

extern "C" {

int slio_aloam_params_default(slio_aloam_params* p) {
  if (!p) {
    set_error("slio_aloam_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->device = 0;
  p->n_scans = 16;
  p->max_points = kMaxPoints;
  p->minimum_range = 0.1;
  p->scan_period = 0.1;
  return SLIO_OK;
}

int slio_aloam_tile(int32_t* block, int32_t* sort_cap) {
  if (!block || !sort_cap) {
    set_error("slio_aloam_tile: null output");
    return SLIO_EINVAL;
  }
  *block = kBlk;
  *sort_cap = kSortCap;
  return SLIO_OK;
}

int slio_aloam_register_host(const slio_aloam_params* p, const float* xyz, int64_t n, float* laser_cloud,
                             float* corner_sharp, float* corner_less_sharp, float* surf_flat,
                             float* surf_less_flat, int32_t* scan_start, int32_t* scan_end, float* curvature_out,
                             int32_t* label_out, uint8_t* picked_out, int32_t counts[5], int32_t* stats) {
  if (!p || n < 0 || (n && !xyz) || !counts) {
    set_error("slio_aloam_register_host: null params, negative size, null cloud or null counts");
    return SLIO_EINVAL;
  }
  if (p->n_scans != 16 && p->n_scans != 32 && p->n_scans != 64) {
    set_error("slio_aloam_register_host: n_scans is not 16, 32 or 64");
    return SLIO_EINVAL;
  }
  if (p->max_points < 1 || p->max_points > kMaxPoints) {
    set_error("slio_aloam_register_host: max_points outside 1 .. 400000");
    return SLIO_EINVAL;
  }
  if (n > p->max_points) {
    set_error("slio_aloam_register_host: more points than max_points");
    return SLIO_ECAPACITY;
  }
  const int S = p->n_scans;
  int32_t st[kNumStats] = {0};
  // :145-148
  const float thres = (float)p->minimum_range;
  std::vector<float> in;
  in.reserve(3 * (size_t)n);
  for (int64_t i = 0; i < n; ++i) {
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    if (!finite3(x, y, z)) {
      ++st[kDropNonFinite];
      continue;
    }
    if (too_close(x, y, z, thres)) {
      ++st[kDropRange];
      continue;
    }
    in.insert(in.end(), {x, y, z});
  }
  int cloud_size = (int)(in.size() / 3);
  std::vector<std::vector<float>> scans((size_t)S);
  if (cloud_size) {
    // :155-163
    const float start_ori = raw_ori(in[0], in[1]);
    int br;
    const float end_ori_ = end_ori(start_ori, raw_ori(in[3 * (cloud_size - 1)], in[3 * (cloud_size - 1) + 1]), &br);
    if (br) ++st[br == 1 ? kEndMinus : kEndPlus];
    // :166-239
    bool half = false;
    for (int i = 0; i < cloud_size; ++i) {
      const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
      int over50 = 0;
      const int id = scan_id(S, elevation_deg(x, y, z), &over50);
      if (id < 0) {
        ++st[kDropScan];
        st[kDropOver50] += over50;
        continue;
      }
      float ori = raw_ori(x, y);
      if (!half) {
        ori = first_branch(ori, start_ori, &br);
        if (br) ++st[br == 1 ? kFirstPlus : kFirstMinus];
        if (half_passed(ori, start_ori)) {
          half = true;
          ++st[kHalfPassed];
        }
      } else {
        ori = second_branch(ori, end_ori_, &br);
        if (br) ++st[br == 1 ? kSecondPlus : kSecondMinus];
      }
      const float it = intensity_of(id, ori, start_ori, end_ori_, p->scan_period);
      scans[id].insert(scans[id].end(), {x, y, z, it});
    }
  }
  // :244-250
  std::vector<float> cloud;
  std::vector<int> s_ind((size_t)S), e_ind((size_t)S);
  for (int i = 0; i < S; ++i) {
    s_ind[i] = (int)(cloud.size() / 4) + 5;
    cloud.insert(cloud.end(), scans[i].begin(), scans[i].end());
    e_ind[i] = (int)(cloud.size() / 4) - 6;
  }
  cloud_size = (int)(cloud.size() / 4);
  const float* c = cloud.data();
  // :254-278
  std::vector<float> curv((size_t)cloud_size, 0.f);
  std::vector<int> sort_ind((size_t)cloud_size, 0), picked((size_t)cloud_size, 0), label((size_t)cloud_size, 0),
      origin((size_t)cloud_size, -1);
  for (int i = 5; i < cloud_size - 5; ++i) {
    curv[i] = curvature(c, i);
    sort_ind[i] = i;
  }
  // :282-432
  std::vector<float> sharp, less_sharp, flat, less_flat;
  auto push = [&](std::vector<float>& v, int ind) { v.insert(v.end(), c + 4 * ind, c + 4 * ind + 4); };
  for (int i = 0; i < S; ++i) {
    if (e_ind[i] - s_ind[i] < 6) {
      ++st[kScansSkipped];
      continue;
    }
    std::vector<int> less_flat_scan;
    for (int j = 0; j < 6; ++j) {
      int sp, ep;
      sector(s_ind[i], e_ind[i], j, &sp, &ep);
      // (std::sort on the value alone; here stable, ties by position)
      std::stable_sort(sort_ind.begin() + sp, sort_ind.begin() + ep + 1,
                       [&](int a, int b) { return curv[a] < curv[b]; });
      Picker pk{c, picked, origin, st, sp, ep, i * 6 + j};
      int largest = 0;
      for (int k = ep; k >= sp; --k) {
        const int ind = sort_ind[k];
        if (picked[ind] != 0 && is_sharp(curv[ind]) && origin[ind] != pk.sec) ++st[kSeamSuppressed];
        if (picked[ind] == 0 && is_sharp(curv[ind])) {
          ++largest;
          if (largest <= 2) {
            label[ind] = 2;
            push(sharp, ind);
            push(less_sharp, ind);
          } else if (largest <= 20) {
            label[ind] = 1;
            push(less_sharp, ind);
          } else {
            ++st[kBreak21];
            break;
          }
          pk.mark(ind);
          pk.neighbours(ind);
        }
      }
      int smallest = 0;
      for (int k = sp; k <= ep; ++k) {
        const int ind = sort_ind[k];
        if (picked[ind] != 0 && is_flat(curv[ind]) && origin[ind] != pk.sec) ++st[kSeamSuppressed];
        if (picked[ind] == 0 && is_flat(curv[ind])) {
          label[ind] = -1;
          push(flat, ind);
          ++st[kFlat];
          ++smallest;
          if (smallest >= 4) {
            ++st[kBreak4];
            break;
          }
          pk.mark(ind);
          pk.neighbours(ind);
        }
      }
      for (int k = sp; k <= ep; ++k)
        if (label[k] <= 0) less_flat_scan.push_back(k);
    }
    voxel_grid(c, less_flat_scan, less_flat, st);
  }
  const std::vector<float>* outs[5] = {&cloud, &sharp, &less_sharp, &flat, &less_flat};
  float* dsts[5] = {laser_cloud, corner_sharp, corner_less_sharp, surf_flat, surf_less_flat};
  for (int k = 0; k < 5; ++k) {
    counts[k] = (int32_t)(outs[k]->size() / 4);
    if (dsts[k] && counts[k]) std::memcpy(dsts[k], outs[k]->data(), 4 * outs[k]->size());
  }
  for (int i = 0; i < S; ++i) {
    if (scan_start) scan_start[i] = s_ind[i];
    if (scan_end) scan_end[i] = e_ind[i];
  }
  for (int i = 0; i < cloud_size; ++i) {
    if (curvature_out) curvature_out[i] = curv[i];
    if (label_out) label_out[i] = label[i];
    if (picked_out) picked_out[i] = (uint8_t)picked[i];
  }
  if (stats) std::memcpy(stats, st, sizeof st);
  return SLIO_OK;
}

}  // extern "C"
