// slio_aloam_odom.cpp -- A-LOAM's laserOdometry on the host, callable without
// a GPU (src/A-LOAM/src/laserOdometry.cpp :304-695): the association as the
// reference's literal serial loops, the factors, the sums and the
// Levenberg-Marquardt over the formulas of slio_aloam_odom.hpp, which the
// kernels of slio_aloam_odom.hip share.  It is what checks the device's
// parallel restatement where there is no GPU.  The solve is this library's
// own; parity with Ceres' iterates is unpinned.
#include <cstring>
#include <vector>

#include "slio_aloam_odom.hpp"
#include "slio_frontend.h"

using slio::set_error;
using namespace slio::aodom;

static_assert(sizeof(slio_aloam_odom_lm) == sizeof(Lm), "slio_aloam_odom_lm mirrors aodom::Lm");

namespace {

struct Clouds {
  const float *sharp, *flat, *corner_last, *surf_last;
  int n_sharp, n_flat, n_corner, n_surf;
};

// the kd-tree's nearestKSearch(.., 1, ..) restated exactly: ties to the lower index
int nearest(const float* last, int n, const float sel[3], float* d_out) {
  int best = -1;
  float bd = INFINITY;
  for (int j = 0; j < n; ++j) {
    const float d = dist2(last + 4 * j, sel);
    if (d < bd) {
      bd = d;
      best = j;
    }
  }
  *d_out = bd;
  return best;
}

void associate(const Clouds& c, const double q[4], const double t[3], int32_t* corr) {
  // :341-450
  for (int i = 0; i < c.n_sharp; ++i) {
    float sel[3], d0;
    to_start(q, t, c.sharp + 4 * i, sel);
    int closest = nearest(c.corner_last, c.n_corner, sel, &d0), ind2 = -1;
    if (closest >= 0 && d0 < kDistSq) {
      const float* L = c.corner_last;
      const int cs = (int)L[4 * closest + 3];
      float min2 = kDistSq;
      for (int j = closest + 1; j < c.n_corner; ++j) {
        if ((int)L[4 * j + 3] <= cs) continue;
        if ((double)(int)L[4 * j + 3] > cs + 2.5) break;
        const float d = dist2(L + 4 * j, sel);
        if (d < min2) {
          min2 = d;
          ind2 = j;
        }
      }
      for (int j = closest - 1; j >= 0; --j) {
        if ((int)L[4 * j + 3] >= cs) continue;
        if ((double)(int)L[4 * j + 3] < cs - 2.5) break;
        const float d = dist2(L + 4 * j, sel);
        if (d < min2) {
          min2 = d;
          ind2 = j;
        }
      }
    } else {
      closest = -1;
    }
    corr[3 * i] = closest;
    corr[3 * i + 1] = ind2;
    corr[3 * i + 2] = -1;
  }
  // :454-573
  for (int i = 0; i < c.n_flat; ++i) {
    float sel[3], d0;
    to_start(q, t, c.flat + 4 * i, sel);
    int closest = nearest(c.surf_last, c.n_surf, sel, &d0), ind2 = -1, ind3 = -1;
    if (closest >= 0 && d0 < kDistSq) {
      const float* L = c.surf_last;
      const int cs = (int)L[4 * closest + 3];
      float min2 = kDistSq, min3 = kDistSq;
      for (int j = closest + 1; j < c.n_surf; ++j) {
        const int id = (int)L[4 * j + 3];
        if ((double)id > cs + 2.5) break;
        const float d = dist2(L + 4 * j, sel);
        if (id <= cs && d < min2) {
          min2 = d;
          ind2 = j;
        } else if (id > cs && d < min3) {
          min3 = d;
          ind3 = j;
        }
      }
      for (int j = closest - 1; j >= 0; --j) {
        const int id = (int)L[4 * j + 3];
        if ((double)id < cs - 2.5) break;
        const float d = dist2(L + 4 * j, sel);
        if (id >= cs && d < min2) {
          min2 = d;
          ind2 = j;
        } else if (id < cs && d < min3) {
          min3 = d;
          ind3 = j;
        }
      }
    } else {
      closest = -1;
    }
    int32_t* o = corr + 3 * (c.n_sharp + i);
    o[0] = closest;
    o[1] = ind2;
    o[2] = ind3;
  }
}

// sums[28] in the fixed order; counts = corner, plane, degenerate, outliers
void evaluate(const Clouds& c, const int32_t* corr, const double q[4], const double t[3], double sums[kSums],
              int32_t counts[4]) {
  static thread_local double part[kLanes][kSums];
  std::memset(part, 0, sizeof part);
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  const int slots = c.n_sharp + c.n_flat;
  for (int s = 0; s < slots; ++s) {
    Factor f;
    int matched, deg;
    const int rows = slot_factor(q, t, s, c.n_sharp, c.sharp, c.flat, c.corner_last, c.surf_last, corr, &f, &matched,
                                 &deg);
    if (matched) ++counts[s < c.n_sharp ? 0 : 1];
    counts[2] += deg;
    if (!rows) continue;
    double v[kSums];
    counts[3] += contributions(f, v);
    for (int k = 0; k < kSums; ++k) part[s % kLanes][k] = part[s % kLanes][k] + v[k];
  }
  for (int k = 0; k < kSums; ++k) {
    double tot = 0.0;
    for (int l = 0; l < kLanes; ++l) tot = tot + part[l][k];
    sums[k] = tot;
  }
}

void one_pass(const Clouds& c, double q[4], double t[3], slio_aloam_odom_pass* out, std::vector<int32_t>& corr) {
  std::memset(out, 0, sizeof *out);
  corr.assign(3 * (size_t)(c.n_sharp + c.n_flat) + 3, -1);
  associate(c, q, t, corr.data());
  double sums[kSums];
  int32_t cnt[4];
  evaluate(c, corr.data(), q, t, sums, cnt);
  Lm s;
  lm_init(&s, q, t);
  std::memcpy(s.A, sums, sizeof s.A);
  std::memcpy(s.g, sums + 21, sizeof s.g);
  s.cost = 0.5 * sums[27];
  out->corner = cnt[0];
  out->plane = cnt[1];
  out->degenerate = cnt[2];
  out->outliers = cnt[3];
  out->few = cnt[0] + cnt[1] < 10;
  out->cost_first = s.cost;
  while (lm_propose(&s)) {
    evaluate(c, corr.data(), s.qn, s.tn, sums, cnt);
    lm_decide(&s, sums, sums + 21, 0.5 * sums[27]);
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

bool bad_cloud(const float* p, int64_t n) { return n < 0 || (n && !p); }

}  // namespace

extern "C" {

int slio_aloam_odom_params_default(slio_aloam_odom_params* p) {
  if (!p) {
    set_error("slio_aloam_odom_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->n_scans = 16;
  p->max_points = 400000;
  p->skip_frame_num = 2;
  return SLIO_OK;
}

int slio_aloam_odom_lm_step(slio_aloam_odom_lm* lm, int phase, const double A[21], const double g[6], double cost) {
  if (!lm || phase < 0 || phase > 2 || (phase == 2 && (!A || !g))) {
    set_error("slio_aloam_odom_lm_step: null state, phase outside 0 .. 2, or phase 2 without an evaluation");
    return SLIO_EINVAL;
  }
  Lm* s = reinterpret_cast<Lm*>(lm);
  if (phase == 0) {
    double q[4], t[3];
    std::memcpy(q, s->q, sizeof q);
    std::memcpy(t, s->t, sizeof t);
    lm_init(s, q, t);
  } else if (phase == 1) {
    lm_propose(s);
  } else {
    if (s->done) {
      set_error("slio_aloam_odom_lm_step: the solve has stopped");
      return SLIO_ESTATE;
    }
    lm_decide(s, A, g, cost);
  }
  return SLIO_OK;
}

int slio_aloam_odom_host_associate(const float* sharp, int64_t n_sharp, const float* flat, int64_t n_flat,
                                   const float* corner_last, int64_t n_corner, const float* surf_last,
                                   int64_t n_surf, const double q[4], const double t[3], int32_t* corr) {
  if (bad_cloud(sharp, n_sharp) || bad_cloud(flat, n_flat) || bad_cloud(corner_last, n_corner) ||
      bad_cloud(surf_last, n_surf) || !q || !t || (!corr && n_sharp + n_flat > 0)) {
    set_error("slio_aloam_odom_host_associate: negative size, null cloud, null pose or null output");
    return SLIO_EINVAL;
  }
  if (n_sharp > kMaxScans * kSharpPerScan || n_flat > kMaxScans * kFlatPerScan || n_corner > 400000 ||
      n_surf > 400000) {
    set_error("slio_aloam_odom_host_associate: more points than any handle takes");
    return SLIO_ECAPACITY;
  }
  if (!ids_ok(corner_last, n_corner) || !ids_ok(surf_last, n_surf)) {
    set_error("slio_aloam_odom_host_associate: scan ids of a last cloud decreasing or outside [0, 64)");
    return SLIO_EINVAL;
  }
  const Clouds c{sharp, flat, corner_last, surf_last, (int)n_sharp, (int)n_flat, (int)n_corner, (int)n_surf};
  associate(c, q, t, corr);
  return SLIO_OK;
}

int slio_aloam_odom_host_evaluate(const float* sharp, int64_t n_sharp, const float* flat, int64_t n_flat,
                                  const float* corner_last, int64_t n_corner, const float* surf_last,
                                  int64_t n_surf, const int32_t* corr, const double q[4], const double t[3],
                                  double A[21], double g[6], double* cost, int32_t counts[4]) {
  if (bad_cloud(sharp, n_sharp) || bad_cloud(flat, n_flat) || bad_cloud(corner_last, n_corner) ||
      bad_cloud(surf_last, n_surf) || !q || !t || (!corr && n_sharp + n_flat > 0) || !A || !g || !cost || !counts) {
    set_error("slio_aloam_odom_host_evaluate: negative size, null cloud, null pose or null output");
    return SLIO_EINVAL;
  }
  if (n_sharp > kMaxScans * kSharpPerScan || n_flat > kMaxScans * kFlatPerScan || n_corner > 400000 ||
      n_surf > 400000) {
    set_error("slio_aloam_odom_host_evaluate: more points than any handle takes");
    return SLIO_ECAPACITY;
  }
  for (int64_t s = 0; s < n_sharp + n_flat; ++s) {
    const int64_t n = s < n_sharp ? n_corner : n_surf;
    for (int k = 0; k < 3; ++k)
      if (corr[3 * s + k] < -1 || corr[3 * s + k] >= n) {
        set_error("slio_aloam_odom_host_evaluate: a correspondence outside its last cloud");
        return SLIO_EINVAL;
      }
    if (corr[3 * s] < 0 && corr[3 * s + 1] >= 0) {
      set_error("slio_aloam_odom_host_evaluate: a second point without a closest one");
      return SLIO_EINVAL;
    }
  }
  const Clouds c{sharp, flat, corner_last, surf_last, (int)n_sharp, (int)n_flat, (int)n_corner, (int)n_surf};
  double sums[kSums];
  evaluate(c, corr, q, t, sums, counts);
  std::memcpy(A, sums, 21 * sizeof(double));
  std::memcpy(g, sums + 21, 6 * sizeof(double));
  *cost = 0.5 * sums[27];
  return SLIO_OK;
}

int slio_aloam_odom_host_init(slio_aloam_odom_state* st) {
  if (!st) {
    set_error("slio_aloam_odom_host_init: null");
    return SLIO_EINVAL;
  }
  std::memset(st, 0, sizeof *st);
  st->q_w_curr[3] = st->para_q[3] = 1.0;
  return SLIO_OK;
}

int slio_aloam_odom_host_run(const slio_aloam_odom_params* p, slio_aloam_odom_state* st, const float* sharp,
                             int64_t n_sharp, const float* flat, int64_t n_flat, const float* corner_last,
                             int64_t n_corner, const float* surf_last, int64_t n_surf,
                             slio_aloam_odom_result* res) {
  if (!p || !st || !res || bad_cloud(sharp, n_sharp) || bad_cloud(flat, n_flat) || bad_cloud(corner_last, n_corner) ||
      bad_cloud(surf_last, n_surf)) {
    set_error("slio_aloam_odom_host_run: null params, state or result, negative size or null cloud");
    return SLIO_EINVAL;
  }
  if (p->n_scans < 1 || p->n_scans > kMaxScans || p->max_points < 1 || p->max_points > 400000 ||
      p->skip_frame_num < 1) {
    set_error("slio_aloam_odom_host_run: n_scans outside 1 .. 64, max_points outside 1 .. 400000 or "
              "skip_frame_num < 1");
    return SLIO_EINVAL;
  }
  if (n_sharp > p->n_scans * kSharpPerScan || n_flat > p->n_scans * kFlatPerScan || n_corner > p->max_points ||
      n_surf > p->max_points) {
    set_error("slio_aloam_odom_host_run: more points than the capacity (12 / 24 per scan, max_points)");
    return SLIO_ECAPACITY;
  }
  if (!ids_ok(corner_last, n_corner) || !ids_ok(surf_last, n_surf)) {
    set_error("slio_aloam_odom_host_run: scan ids of a last cloud decreasing or outside [0, 64)");
    return SLIO_EINVAL;
  }
  std::memset(res, 0, sizeof *res);
  res->inited = st->inited;
  if (!st->inited) {
    st->inited = 1;  // :307-309
  } else {
    const Clouds c{sharp, flat, corner_last, surf_last, (int)n_sharp, (int)n_flat, (int)n_corner, (int)n_surf};
    std::vector<int32_t> corr;
    for (int k = 0; k < 2; ++k) one_pass(c, st->para_q, st->para_t, &res->pass[k], corr);
    integrate(st->q_w_curr, st->t_w_curr, st->para_q, st->para_t);
  }
  // :667-695
  res->published = st->frame_count % p->skip_frame_num == 0;
  if (res->published) st->frame_count = 0;
  ++st->frame_count;
  res->frame_count = st->frame_count;
  std::memcpy(res->q_w_curr, st->q_w_curr, sizeof st->q_w_curr);
  std::memcpy(res->t_w_curr, st->t_w_curr, sizeof st->t_w_curr);
  std::memcpy(res->q_last_curr, st->para_q, sizeof st->para_q);
  std::memcpy(res->t_last_curr, st->para_t, sizeof st->para_t);
  return SLIO_OK;
}

}  // extern "C"
