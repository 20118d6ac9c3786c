// slio_aloam_map.cpp -- A-LOAM's laserMapping on the host, callable without a
// GPU (src/A-LOAM/src/laserMapping.cpp :326-893): the cube array as one vector
// per cube, the 5-NN as a brute-force scan of the valid cubes, the VoxelGrid
// as the cube store states it (slio_cube_store.hip), and the fits, the factors, the
// sums and the Levenberg-Marquardt over the formulas of slio_aloam_map.hpp,
// which the kernels of slio_aloam_map.hip share.  It is what checks the
// device's parallel restatement where there is no GPU.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "slio_aloam_map.hpp"
#include "slio_frontend.h"
#include "slio_livox.hpp"
#include "slio_voxel.hpp"

using slio::set_error;
using namespace slio::amap;
namespace aodom = slio::aodom;

namespace {

bool finite_pose(const double* q, const double* t) {
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(q[k])) return false;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k])) return false;
  return true;
}

// The cube store's VoxelGrid of one cloud (n x 3): k_lvx_box's box in key
// order, the geometry and the voxel index k_lvx_geom and k_lvx_keys call
// (slio_voxel.hpp), a stable sort, k_lvx_centroids' float sums in the sorted
// order; a leaf too small for the cloud passes it through.  Points that are
// not finite are dropped first.
void voxel_grid(const std::vector<float>& in, float leaf, std::vector<float>& out) {
  std::vector<float> p;
  for (size_t i = 0; i + 2 < in.size(); i += 3)
    if (std::isfinite(in[i]) && std::isfinite(in[i + 1]) && std::isfinite(in[i + 2]))
      p.insert(p.end(), in.begin() + i, in.begin() + i + 3);
  const size_t n = p.size() / 3;
  out.clear();
  // (the count, box[6], is only tested against 0)
  int32_t box[7] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, n ? 1 : 0};
  for (size_t i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      int32_t k;  // (fkey of slio_fkey.hpp, which is HIP only)
      std::memcpy(&k, &p[3 * i + a], 4);
      k = k >= 0 ? k : k ^ 0x7FFFFFFF;
      box[a] = std::min(box[a], k);
      box[3 + a] = std::max(box[3 + a], k);
    }
  slio::VoxelGeom g;
  const slio::VoxelKind kind = slio::voxel_geometry(box, leaf, &g);
  if (kind == slio::kVoxelNone) return;
  if (kind == slio::kVoxelPass) {
    out = p;
    return;
  }
  std::vector<std::pair<uint32_t, uint32_t>> key(n);
  for (size_t i = 0; i < n; ++i) {
    key[i] = {slio::voxel_index(p[3 * i], p[3 * i + 1], p[3 * i + 2], g.inv, g.minb, g.mul), (uint32_t)i};
  }
  std::stable_sort(key.begin(), key.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
  for (size_t i = 0; i < n;) {
    size_t j = i;
    float s[3] = {0.0f, 0.0f, 0.0f};
    for (; j < n && key[j].first == key[i].first; ++j)
      for (int a = 0; a < 3; ++a) s[a] = s[a] + p[3 * key[j].second + a];
    const float cnt = (float)(j - i);
    for (int a = 0; a < 3; ++a) out.push_back(s[a] / cnt);
    i = j;
  }
}

struct Assoc {
  std::vector<uint8_t> kind;
  std::vector<double> rec;
  std::vector<int32_t> idx;
  std::vector<float> sqd;
  void resize(size_t n) {
    kind.assign(n, kNone);
    rec.assign(6 * n, 0.0);
    idx.assign(kK * n, -1);
    sqd.assign(kK * n, INFINITY);
  }
};

// one class: pointAssociateToMap, the exact 5-NN over map (n x 3) with ties
// to the lower index, the gate, the fit
void associate(int surf, const float* stack, int n, const std::vector<float>& map, const double q[4],
               const double t[3], Assoc* a, int slot0) {
  const int nm = (int)(map.size() / 3);
  for (int i = 0; i < n; ++i) {
    const int s = slot0 + i;
    float w[3];
    aodom::to_start(q, t, stack + 3 * i, w);
    uint64_t top[kK];
    for (int j = 0; j < kK; ++j) top[j] = ~0ull;
    if (std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]))
      for (int m = 0; m < nm; ++m) {
        const float dx = map[3 * m] - w[0], dy = map[3 * m + 1] - w[1], dz = map[3 * m + 2] - w[2];
        const float d2 = (dx * dx + dy * dy) + dz * dz;
        uint32_t bits;
        std::memcpy(&bits, &d2, 4);
        uint64_t key = ((uint64_t)bits << 32) | (uint32_t)m;
        for (int j = 0; j < kK; ++j)
          if (key < top[j]) std::swap(key, top[j]);
      }
    float d2k = INFINITY;
    if (top[kK - 1] != ~0ull) {
      const uint32_t bits = (uint32_t)(top[kK - 1] >> 32);
      std::memcpy(&d2k, &bits, 4);
    }
    if (!(d2k < kGate)) continue;
    double nb[kK][3];
    for (int j = 0; j < kK; ++j) {
      const uint32_t m = (uint32_t)top[j], bits = (uint32_t)(top[j] >> 32);
      a->idx[kK * s + j] = (int32_t)m;
      std::memcpy(&a->sqd[kK * s + j], &bits, 4);
      for (int k = 0; k < 3; ++k) nb[j][k] = (double)map[3 * m + k];
    }
    a->kind[s] = (uint8_t)fit(surf, nb, &a->rec[6 * s]);
  }
}

// the 28 sums and the counts {edge, plane, degenerate, outliers} over n slots, in the header's order
void evaluate(const float* xyz, const uint8_t* kind, const double* rec, int n, const double q[4], const double t[3],
              double sums[kSums], int32_t cnt[4]) {
  const int nwg = (n + kWg - 1) / kWg;
  std::vector<double> P((size_t)nwg * kSums);
  cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0;
  for (int w = 0; w < nwg; ++w) {
    static thread_local double c[kSums][kWg];
    uint8_t valid[kWg];
    const int m = std::min(kWg, n - w * kWg);
    for (int i = 0; i < m; ++i) {
      const int s = w * kWg + i;
      Factor f;
      cnt[0] += kind[s] == kEdge;
      cnt[1] += kind[s] == kPlane;
      cnt[2] += kind[s] == kDegenerate;
      valid[i] = slot_factor(q, t, xyz + 3 * s, kind[s], rec + 6 * s, &f) != 0;
      if (!valid[i]) continue;
      double v[kSums];
      cnt[3] += aodom::contributions(f, v);
      for (int k = 0; k < kSums; ++k) c[k][i] = v[k];
    }
    for (int k = 0; k < kSums; ++k) {
      double part[kLanes];
      for (int l = 0; l < kLanes; ++l) part[l] = lane_sum(c[k], 1, valid, 0, m, l);
      P[(size_t)w * kSums + k] = lanes_total(part);
    }
  }
  for (int k = 0; k < kSums; ++k) {
    double part[kLanes];
    for (int l = 0; l < kLanes; ++l) part[l] = lane_sum(P.data() + k, kSums, nullptr, 0, nwg, l);
    sums[k] = lanes_total(part);
  }
}

}  // namespace

struct slio_aloam_map_host {
  slio_aloam_map_params prm{};
  std::vector<float> cube[2][kNum];
  int32_t cen[3] = {10, 10, 5};
  double q_wmap[4] = {0, 0, 0, 1}, t_wmap[3] = {0, 0, 0};
  std::vector<float> stack[2];
  Assoc assoc;
  bool has_run = false;
};

extern "C" {

int slio_aloam_map_params_default(slio_aloam_map_params* p) {
  if (!p) {
    set_error("slio_aloam_map_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof *p);
  p->device = 0;
  p->max_points = 1 << 21;
  p->max_scan = 400000;
  p->leaf_corner = 0.4f;
  p->leaf_surf = 0.8f;
  return SLIO_OK;
}

int slio_aloam_map_predict(const double q_wmap_wodom[4], const double t_wmap_wodom[3], const double q_wodom_curr[4],
                           const double t_wodom_curr[3], double q_w_curr[4], double t_w_curr[3]) {
  if (!q_wmap_wodom || !t_wmap_wodom || !q_wodom_curr || !t_wodom_curr || !q_w_curr || !t_w_curr) {
    set_error("slio_aloam_map_predict: null argument");
    return SLIO_EINVAL;
  }
  associate_to_map(q_wmap_wodom, t_wmap_wodom, q_wodom_curr, t_wodom_curr, q_w_curr, t_w_curr);
  return SLIO_OK;
}

int slio_aloam_map_host_select(const double t_w_curr[3], int32_t cen[3], int32_t center[3], int32_t shift[3],
                               int32_t* list, int32_t* n) {
  if (!t_w_curr || !cen || !center || !shift || !list || !n) {
    set_error("slio_aloam_map_host_select: null argument");
    return SLIO_EINVAL;
  }
  int32_t c2[3] = {cen[0], cen[1], cen[2]};
  if (select(t_w_curr, c2, center, shift, list, n)) {
    set_error("slio_aloam_map_host_select: position not finite or beyond 1e6 m");
    return SLIO_EINVAL;
  }
  std::memcpy(cen, c2, sizeof c2);
  return SLIO_OK;
}

int slio_aloam_map_host_fit_line(const double* nb, double a[3], double b[3], double* lam, double* vec) {
  if (!nb || !a || !b) {
    set_error("slio_aloam_map_host_fit_line: null argument");
    return SLIO_EINVAL;
  }
  double m[kK][3], rec[6];
  std::memcpy(m, nb, sizeof m);
  const int kind = fit(0, m, rec);
  std::memcpy(a, rec, 3 * sizeof(double));
  std::memcpy(b, rec + 3, 3 * sizeof(double));
  if (lam || vec) {  // the eigen-solve alone, on the same covariance
    double c[3] = {0.0, 0.0, 0.0}, cov[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, l[3], V[3][3];
    for (int j = 0; j < kK; ++j)
      for (int k = 0; k < 3; ++k) c[k] = c[k] + m[j][k];
    for (int k = 0; k < 3; ++k) c[k] = c[k] / 5.0;
    for (int j = 0; j < kK; ++j) {
      const double z0 = m[j][0] - c[0], z1 = m[j][1] - c[1], z2 = m[j][2] - c[2];
      cov[0] = cov[0] + z0 * z0;
      cov[1] = cov[1] + z0 * z1;
      cov[2] = cov[2] + z0 * z2;
      cov[3] = cov[3] + z1 * z1;
      cov[4] = cov[4] + z1 * z2;
      cov[5] = cov[5] + z2 * z2;
    }
    jacobi3(cov, l, V);
    if (lam) std::memcpy(lam, l, sizeof l);
    if (vec) std::memcpy(vec, V, sizeof V);
  }
  return kind;
}

int slio_aloam_map_host_fit_plane(const double* nb, double normal[3], double* d, double* x) {
  if (!nb || !normal || !d) {
    set_error("slio_aloam_map_host_fit_plane: null argument");
    return SLIO_EINVAL;
  }
  double m[kK][3];
  std::memcpy(m, nb, sizeof m);
  if (x) qr_solve_m1(m, x);
  return fit_plane(m, normal, d);
}

int slio_aloam_map_host_evaluate(const float* xyz, const uint8_t* kind, const double* rec, int64_t n,
                                 const double q[4], const double t[3], double A[21], double g[6], double* cost,
                                 int32_t counts[4]) {
  if (n < 0 || (n && (!xyz || !kind || !rec)) || !q || !t || !A || !g || !cost || !counts) {
    set_error("slio_aloam_map_host_evaluate: negative size or null argument");
    return SLIO_EINVAL;
  }
  if (n > 2 * 400000) {
    set_error("slio_aloam_map_host_evaluate: more than 800000 slots");
    return SLIO_ECAPACITY;
  }
  double sums[kSums];
  evaluate(xyz, kind, rec, (int)n, q, t, sums, counts);
  std::memcpy(A, sums, 21 * sizeof(double));
  std::memcpy(g, sums + 21, 6 * sizeof(double));
  *cost = 0.5 * sums[27];
  return SLIO_OK;
}

int slio_aloam_map_host_create(slio_aloam_map_host_handle* out, const slio_aloam_map_params* p) {
  if (!out || !p || p->max_points < 1 || p->max_scan < 1 || p->max_scan > 400000 || !(p->leaf_corner > 0.0f) ||
      !(p->leaf_surf > 0.0f) || !std::isfinite(p->leaf_corner) || !std::isfinite(p->leaf_surf)) {
    set_error("slio_aloam_map_host_create: bad arguments (max_points >= 1, max_scan in 1 .. 400000, finite leaves "
              "> 0)");
    return SLIO_EINVAL;
  }
  slio_aloam_map_host* h = new slio_aloam_map_host();
  h->prm = *p;
  *out = h;
  return SLIO_OK;
}

int slio_aloam_map_host_destroy(slio_aloam_map_host_handle h) {
  delete h;
  return SLIO_OK;
}

int slio_aloam_map_host_run(slio_aloam_map_host_handle h, const float* corner_last, int64_t n_corner,
                            const float* surf_last, int64_t n_surf, const double q_wodom_curr[4],
                            const double t_wodom_curr[3], slio_aloam_map_result* res) {
  if (!h || !res || n_corner < 0 || n_surf < 0 || (n_corner && !corner_last) || (n_surf && !surf_last) ||
      !q_wodom_curr || !t_wodom_curr || !finite_pose(q_wodom_curr, t_wodom_curr) || !(sqnorm4(q_wodom_curr) > 0.0)) {
    set_error("slio_aloam_map_host_run: null handle or result, negative size, null cloud, or a pose that is null, "
              "not finite or of zero norm");
    return SLIO_EINVAL;
  }
  if (n_corner > h->prm.max_scan || n_surf > h->prm.max_scan) {
    set_error("slio_aloam_map_host_run: a cloud beyond max_scan");
    return SLIO_ECAPACITY;
  }
  const int64_t nin[2] = {n_corner, n_surf};
  for (int k = 0; k < 2; ++k) {
    int64_t stored = 0;
    for (const auto& c : h->cube[k]) stored += (int64_t)(c.size() / 3);
    if (stored + nin[k] > h->prm.max_points) {
      set_error("slio_aloam_map_host_run: map and scan exceed max_points");
      return SLIO_ECAPACITY;
    }
  }
  slio_aloam_map_result r;
  std::memset(&r, 0, sizeof r);
  double q[4], t[3];
  associate_to_map(h->q_wmap, h->t_wmap, q_wodom_curr, t_wodom_curr, q, t);
  int32_t cen[3] = {h->cen[0], h->cen[1], h->cen[2]}, list[kMaxListed], nlist = 0;
  if (select(t, cen, r.center, r.shift, list, &nlist)) {
    set_error("slio_aloam_map_host_run: position not finite or beyond 1e6 m");
    return SLIO_EINVAL;
  }
  std::memcpy(h->cen, cen, sizeof cen);
  r.nvalid = nlist;
  if (r.shift[0] || r.shift[1] || r.shift[2])
    for (int k = 0; k < 2; ++k) {
      std::vector<std::vector<float>> moved(kNum);
      for (int c = 0; c < kNum; ++c) {
        const int i = c % kW + r.shift[0], j = c / kW % kH + r.shift[1], l = c / (kW * kH) + r.shift[2];
        if (i >= 0 && i < kW && j >= 0 && j < kH && l >= 0 && l < kD)
          moved[i + kW * j + kW * kH * l].swap(h->cube[k][c]);
      }
      for (int c = 0; c < kNum; ++c) h->cube[k][c].swap(moved[c]);
    }
  std::vector<float> map[2];
  const float* src[2] = {corner_last, surf_last};
  const float leaf[2] = {h->prm.leaf_corner, h->prm.leaf_surf};
  for (int k = 0; k < 2; ++k) {
    for (int i = 0; i < nlist; ++i) map[k].insert(map[k].end(), h->cube[k][list[i]].begin(), h->cube[k][list[i]].end());
    r.map_size[k] = (int32_t)(map[k].size() / 3);
    std::vector<float> xyz;
    for (int64_t i = 0; i < nin[k]; ++i) xyz.insert(xyz.end(), src[k] + 4 * i, src[k] + 4 * i + 3);
    voxel_grid(xyz, leaf[k], h->stack[k]);
    r.stack_size[k] = (int32_t)(h->stack[k].size() / 3);
  }
  const int nc = r.stack_size[0], ns = r.stack_size[1], slots = nc + ns;
  std::vector<float> all(h->stack[0]);
  all.insert(all.end(), h->stack[1].begin(), h->stack[1].end());
  h->assoc.resize((size_t)slots);
  r.optimized = r.map_size[0] > 10 && r.map_size[1] > 50;  // :613
  if (r.optimized)
    for (int pass = 0; pass < 2; ++pass) {
      slio_aloam_odom_pass* out = &r.pass[pass];
      h->assoc.resize((size_t)slots);
      associate(0, h->stack[0].data(), nc, map[0], q, t, &h->assoc, 0);
      associate(1, h->stack[1].data(), ns, map[1], q, t, &h->assoc, nc);
      double sums[kSums];
      int32_t cnt[4];
      evaluate(all.data(), h->assoc.kind.data(), h->assoc.rec.data(), slots, q, t, sums, cnt);
      aodom::Lm s;
      aodom::lm_init(&s, q, t);
      std::memcpy(s.A, sums, sizeof s.A);
      std::memcpy(s.g, sums + 21, sizeof s.g);
      s.cost = 0.5 * sums[27];
      out->corner = cnt[0];
      out->plane = cnt[1];
      out->degenerate = cnt[2];
      out->outliers = cnt[3];
      out->cost_first = s.cost;
      while (aodom::lm_propose(&s)) {
        evaluate(all.data(), h->assoc.kind.data(), h->assoc.rec.data(), slots, s.qn, s.tn, sums, cnt);
        aodom::lm_decide(&s, sums, sums + 21, 0.5 * sums[27]);
        if (s.last_accepted) out->outliers = cnt[3];
        const int k = s.iterations - 1;
        std::memcpy(out->it_q[k], s.q, sizeof s.q);
        std::memcpy(out->it_t[k], s.t, sizeof s.t);
        out->it_cost[k] = s.cost;
        out->it_mu[k] = s.mu;
      }
      out->iterations = s.iterations;
      out->accepted = s.accepted;
      out->stop = s.stop;
      out->cost_last = s.cost;
      std::memcpy(q, s.q, sizeof s.q);
      std::memcpy(t, s.t, sizeof s.t);
    }
  transform_update(q, t, q_wodom_curr, t_wodom_curr, h->q_wmap, h->t_wmap);
  // :835-892: both stacks into their cubes at the solved pose, then the VoxelGrid of the valid cubes
  for (int k = 0; k < 2; ++k) {
    const int n = r.stack_size[k];
    for (int i = 0; i < n; ++i) {
      float w[3];
      int c[3];
      aodom::to_start(q, t, h->stack[k].data() + 3 * i, w);
      if (!(std::isfinite(w[0]) && std::isfinite(w[1]) && std::isfinite(w[2]))) continue;
      if (slio::lvx::cube_of(w[0], h->cen[0], &c[0]) && slio::lvx::cube_of(w[1], h->cen[1], &c[1]) &&
          slio::lvx::cube_of(w[2], h->cen[2], &c[2]) && c[0] >= 0 && c[0] < kW && c[1] >= 0 && c[1] < kH &&
          c[2] >= 0 && c[2] < kD) {
        std::vector<float>& dst = h->cube[k][c[0] + kW * c[1] + kW * kH * c[2]];
        dst.insert(dst.end(), w, w + 3);
      }
    }
    for (int i = 0; i < nlist; ++i) {
      std::vector<float> out;
      voxel_grid(h->cube[k][list[i]], leaf[k], out);
      h->cube[k][list[i]].swap(out);
    }
  }
  std::memcpy(r.q_w_curr, q, sizeof q);
  std::memcpy(r.t_w_curr, t, sizeof t);
  std::memcpy(r.q_wmap_wodom, h->q_wmap, sizeof h->q_wmap);
  std::memcpy(r.t_wmap_wodom, h->t_wmap, sizeof h->t_wmap);
  h->has_run = true;
  *res = r;
  return SLIO_OK;
}

static int copy_out(const std::vector<float>& src, float* xyz, int64_t cap, int64_t* n, const char* who) {
  if (n) *n = (int64_t)(src.size() / 3);
  if (!xyz) return SLIO_OK;
  if (cap < (int64_t)(src.size() / 3)) {
    set_error(std::string(who) + ": the output holds fewer points than the cloud");
    return SLIO_ECAPACITY;
  }
  if (!src.empty()) std::memcpy(xyz, src.data(), 4 * src.size());
  return SLIO_OK;
}

int slio_aloam_map_host_get_cube(slio_aloam_map_host_handle h, int kind, int32_t cube, float* xyz, int64_t cap,
                                 int64_t* n) {
  if (!h || (kind != 0 && kind != 1) || cube < 0 || cube >= kNum || cap < 0) {
    set_error("slio_aloam_map_host_get_cube: null handle, kind outside {0, 1}, cube outside the array or negative "
              "capacity");
    return SLIO_EINVAL;
  }
  return copy_out(h->cube[kind][cube], xyz, cap, n, "slio_aloam_map_host_get_cube");
}

int slio_aloam_map_host_get_stack(slio_aloam_map_host_handle h, int kind, float* xyz, int64_t cap, int64_t* n) {
  if (!h || (kind != 0 && kind != 1) || cap < 0) {
    set_error("slio_aloam_map_host_get_stack: null handle, kind outside {0, 1} or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_host_get_stack: no sweep before");
    return SLIO_ESTATE;
  }
  return copy_out(h->stack[kind], xyz, cap, n, "slio_aloam_map_host_get_stack");
}

int slio_aloam_map_host_get_association(slio_aloam_map_host_handle h, uint8_t* kind, double* rec, int32_t* nbr_idx,
                                        float* nbr_sqd, int64_t cap_slots, int32_t* n) {
  if (!h || !n || cap_slots < 0) {
    set_error("slio_aloam_map_host_get_association: null handle or count, or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_host_get_association: no sweep before");
    return SLIO_ESTATE;
  }
  const size_t m = h->assoc.kind.size();
  *n = (int32_t)m;
  if ((int64_t)m > cap_slots) {
    set_error("slio_aloam_map_host_get_association: the output holds fewer slots than the association");
    return SLIO_ECAPACITY;
  }
  if (!m) return SLIO_OK;
  if (kind) std::memcpy(kind, h->assoc.kind.data(), m);
  if (rec) std::memcpy(rec, h->assoc.rec.data(), 48 * m);
  if (nbr_idx) std::memcpy(nbr_idx, h->assoc.idx.data(), 4 * kK * m);
  if (nbr_sqd) std::memcpy(nbr_sqd, h->assoc.sqd.data(), 4 * kK * m);
  return SLIO_OK;
}

}  // extern "C"
