// slio_aloam_odom.hpp -- the formulas of A-LOAM's laserOdometry
// (src/A-LOAM/src/laserOdometry.cpp, the opti loop :317-593 with the factors of
// lidarFactor.hpp:12-125, the integration :600-601), written once for the host
// restatement (slio_aloam_odom.cpp) and for the kernels (slio_aloam_odom.hip).
// Internal to the library.
//
// Everything from the association to the pose is + - * / sqrt in IEEE double
// (the distances in float, as the reference has them), every sum written out
// in one association order, so that under -ffp-contract=off the device, the
// host and a numpy model agree to the bit.  A quaternion is (x, y, z, w), as
// para_q (:55).  DISTORTION is 0 (:52): s = 1 everywhere.
//
// The solve is this library's own Levenberg-Marquardt in the shape of Ceres'
// trust-region defaults; parity with Ceres' own iterates is unpinned.
#pragma once

#include <cmath>
#include <cstdint>

#include "slio_common.hpp"

namespace slio {
namespace aodom {

constexpr int kMaxScans = 64;
constexpr int kSharpPerScan = 12, kFlatPerScan = 24;  // scanRegistration's picks per scan
constexpr int kMaxSlots = kMaxScans * (kSharpPerScan + kFlatPerScan);  // 2304
constexpr int kLanes = 32;   // strided partial sums per entry
constexpr int kSums = 28;    // A (21, upper triangle row-major), g (6), sum of rho
constexpr int kMaxIter = 4;  // max_num_iterations (:588)
constexpr float kDistSq = 25.f;  // DISTANCE_SQ_THRESHOLD (:53)
constexpr int kNearby = 2;   // ids within +-NEARBY_SCAN = 2.5 (:54) of an int id
enum { kStopMaxIter = 0, kStopGradient = 1, kStopFunction = 2, kStopParameter = 3 };

SLIO_HD inline void cross3(const double a[3], const double b[3], double o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// Eigen's Quaternion::_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv
SLIO_HD inline void rotate(const double q[4], const double v[3], double o[3]) {
  double uv[3], c[3];
  cross3(q, v, uv);
  for (int a = 0; a < 3; ++a) uv[a] = uv[a] + uv[a];
  cross3(q, uv, c);
  for (int a = 0; a < 3; ++a) o[a] = (v[a] + q[3] * uv[a]) + c[a];
}

// Eigen's quaternion product a * b
SLIO_HD inline void qmul(const double a[4], const double b[4], double o[4]) {
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[0] = x;
  o[1] = y;
  o[2] = z;
  o[3] = w;
}

// TransformToStart (:105-126) at s = 1: q * p + t in double, rounded to float
SLIO_HD inline void to_start(const double q[4], const double t[3], const float* p, float o[3]) {
  const double v[3] = {(double)p[0], (double)p[1], (double)p[2]};
  double r[3];
  rotate(q, v, r);
  for (int a = 0; a < 3; ++a) o[a] = (float)(r[a] + t[a]);
}

// the squared distance of :376-382 (and of the kd-tree's L2), in float
SLIO_HD inline float dist2(const float* l, const float s[3]) {
  const float dx = l[0] - s[0], dy = l[1] - s[1], dz = l[2] - s[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// int(intensity) (:355), or -1 for an id outside [0, 64) (a NaN included)
SLIO_HD inline int scan_of(float intensity) {
  if (!(intensity >= 0.f && intensity < (float)kMaxScans)) return -1;
  return (int)intensity;
}

// what a cloud must satisfy to become a last cloud: ids non-decreasing in the index, inside [0, 64)
inline bool ids_ok(const float* c, int64_t n) {
  int prev = 0;
  for (int64_t i = 0; i < n; ++i) {
    const int id = scan_of(c[4 * i + 3]);
    if (id < 0 || id < prev) return false;
    prev = id;
  }
  return true;
}

// With scan ids non-decreasing in the index and ring_start[s] = the first
// index whose id is >= s (ring_start[64] = n), the `continue`s and `break`s of
// :361-418 / :476-539 cut index ranges [lo, hi):
//   fwd_far   ids cs + 1 .. cs + 2   (the corner's forward scan; the surf's minPointInd3)
//   bwd_far   ids cs - 2 .. cs - 1
//   same scan [closest + 1, rs[cs + 1]) forward and [rs[cs], closest) backward (minPointInd2 of a surf)
SLIO_HD inline void fwd_far(const int* rs, int cs, int* lo, int* hi) {
  *lo = rs[cs + 1];
  *hi = rs[cs + kNearby + 1 < kMaxScans ? cs + kNearby + 1 : kMaxScans];
}
SLIO_HD inline void bwd_far(const int* rs, int cs, int* lo, int* hi) {
  *lo = rs[cs - kNearby > 0 ? cs - kNearby : 0];
  *hi = rs[cs];
}

struct Factor {
  double r[3];     // residuals (a plane's in r[0])
  double J[3][6];  // rows [d theta (3), d t (3)]
  int rows;        // 3 edge, 1 plane, 0 degenerate
};

// LidarEdgeFactor (lidarFactor.hpp:12-67) at (q, t): cp the query, a the
// closest point, b the second
SLIO_HD inline void edge_factor(const double q[4], const double t[3], const float* cpf, const float* af,
                                const float* bf, Factor* f) {
  const double cp[3] = {(double)cpf[0], (double)cpf[1], (double)cpf[2]};
  double rc[3], lp[3], d1[3], d2[3], de[3], nu[3];
  rotate(q, cp, rc);
  for (int k = 0; k < 3; ++k) {
    lp[k] = rc[k] + t[k];
    d1[k] = lp[k] - (double)af[k];
    d2[k] = lp[k] - (double)bf[k];
    de[k] = (double)af[k] - (double)bf[k];
  }
  const double n = sqrt((de[0] * de[0] + de[1] * de[1]) + de[2] * de[2]);
  if (n == 0.0) {
    f->rows = 0;
    return;
  }
  cross3(d1, d2, nu);
  const double m[3] = {((double)bf[0] - (double)af[0]) / n, ((double)bf[1] - (double)af[1]) / n,
                       ((double)bf[2] - (double)af[2]) / n};
  const double E[3][3] = {{0.0, -m[2], m[1]}, {m[2], 0.0, -m[0]}, {-m[1], m[0], 0.0}};  // [b - a]x / |a - b|
  f->rows = 3;
  for (int i = 0; i < 3; ++i) {
    f->r[i] = nu[i] / n;
    cross3(rc, E[i], f->J[i]);  // row i of -E [q*cp]x
    for (int k = 0; k < 3; ++k) f->J[i][3 + k] = E[i][k];
  }
}

// LidarPlaneFactor (lidarFactor.hpp:69-125): j the closest point, l and m the other two
SLIO_HD inline void plane_factor(const double q[4], const double t[3], const float* cpf, const float* jf,
                                 const float* lf, const float* mf, Factor* f) {
  const double cp[3] = {(double)cpf[0], (double)cpf[1], (double)cpf[2]};
  double rc[3], jl[3], jm[3], nr[3], n[3];
  for (int k = 0; k < 3; ++k) {
    jl[k] = (double)jf[k] - (double)lf[k];
    jm[k] = (double)jf[k] - (double)mf[k];
  }
  cross3(jl, jm, nr);
  const double len = sqrt((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2]);
  for (int k = 0; k < 3; ++k) n[k] = nr[k] / len;
  if (!(n[0] - n[0] == 0.0 && n[1] - n[1] == 0.0 && n[2] - n[2] == 0.0)) {
    f->rows = 0;
    return;
  }
  rotate(q, cp, rc);
  double d[3];
  for (int k = 0; k < 3; ++k) d[k] = (rc[k] + t[k]) - (double)jf[k];
  f->rows = 1;
  f->r[0] = (d[0] * n[0] + d[1] * n[1]) + d[2] * n[2];
  cross3(rc, n, f->J[0]);
  for (int k = 0; k < 3; ++k) f->J[0][3 + k] = n[k];
}

// HuberLoss(0.1) on s = |r|^2 and the factor's 28 contributions: w J^T J
// (upper triangle, row-major), w J^T r, rho.  Returns 1 for an outlier (s >
// 0.01).  rows > 0.
SLIO_HD inline int contributions(const Factor& f, double c[kSums]) {
  double s = f.r[0] * f.r[0];
  if (f.rows == 3) s = (s + f.r[1] * f.r[1]) + f.r[2] * f.r[2];
  double rho = s, w = 1.0;
  const int out = s > 0.01;
  if (out) {
    const double sq = sqrt(s);
    rho = 0.2 * sq - 0.01;
    w = 0.1 / sq;
  }
  int k = 0;
  for (int a = 0; a < 6; ++a)
    for (int b = a; b < 6; ++b) {
      double h = f.J[0][a] * f.J[0][b];
      if (f.rows == 3) h = (h + f.J[1][a] * f.J[1][b]) + f.J[2][a] * f.J[2][b];
      c[k++] = w * h;
    }
  for (int a = 0; a < 6; ++a) {
    double h = f.J[0][a] * f.r[0];
    if (f.rows == 3) h = (h + f.J[1][a] * f.r[1]) + f.J[2][a] * f.r[2];
    c[k++] = w * h;
  }
  c[k] = rho;
  return out;
}

// One factor slot from its correspondence (closest, second, third; -1: none):
// slot < n_sharp is a corner query, else a surf query.  Returns rows (0:
// unmatched or degenerate); *deg set for a matched but degenerate one.
SLIO_HD inline int slot_factor(const double q[4], const double t[3], int slot, int n_sharp, const float* sharp,
                               const float* flat, const float* corner_last, const float* surf_last,
                               const int* corr, Factor* f, int* matched, int* deg) {
  const int i0 = corr[3 * slot], i1 = corr[3 * slot + 1], i2 = corr[3 * slot + 2];
  *matched = 0;
  *deg = 0;
  f->rows = 0;
  if (slot < n_sharp) {
    if (i1 < 0) return 0;  // :423
    *matched = 1;
    edge_factor(q, t, sharp + 4 * slot, corner_last + 4 * i0, corner_last + 4 * i1, f);
  } else {
    if (i1 < 0 || i2 < 0) return 0;  // :541
    *matched = 1;
    plane_factor(q, t, flat + 4 * (slot - n_sharp), surf_last + 4 * i0, surf_last + 4 * i1, surf_last + 4 * i2, f);
  }
  *deg = f->rows == 0;
  return f->rows;
}

// The controller's state across the iterations of one solve
struct Lm {
  double mu, nu;           // trust-region radius and its shrink factor
  double q[4], t[3];       // the current point
  double A[21], g[6], cost;
  double delta[6], model, xnorm;  // the proposed step
  double qn[4], tn[3];     // the proposed point
  int32_t pivots_ok, iterations, accepted, stop, done, last_accepted;
};

// the place of A(a, b) in the 21 entries
SLIO_HD inline int tri(int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
}

SLIO_HD inline void lm_init(Lm* s, const double q[4], const double t[3]) {
  s->mu = 1e4;
  s->nu = 2.0;
  for (int k = 0; k < 4; ++k) s->q[k] = s->qn[k] = q[k];
  for (int k = 0; k < 3; ++k) s->t[k] = s->tn[k] = t[k];
  for (int k = 0; k < 6; ++k) s->delta[k] = 0.0;
  s->model = s->xnorm = 0.0;
  s->pivots_ok = s->iterations = s->accepted = s->done = s->last_accepted = 0;
  s->stop = kStopMaxIter;
}

// (A + D^2 / mu) delta = -g by LDL^T; false where a pivot is not positive (delta = 0 then)
SLIO_HD inline bool ldlt_solve(const double A[21], const double g[6], double mu, double delta[6]) {
  double M[6][6], L[6][6], d[6], y[6];
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) M[i][j] = A[tri(i, j)];
  for (int i = 0; i < 6; ++i) {
    double D2 = M[i][i];
    if (!(D2 >= 1e-6)) D2 = 1e-6;
    if (D2 > 1e32) D2 = 1e32;
    M[i][i] = M[i][i] + D2 / mu;
    delta[i] = 0.0;
  }
  for (int j = 0; j < 6; ++j) {
    double v = M[j][j];
    for (int k = 0; k < j; ++k) v = v - (L[j][k] * L[j][k]) * d[k];
    if (!(v > 0.0)) return false;
    d[j] = v;
    for (int i = j + 1; i < 6; ++i) {
      double s = M[i][j];
      for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * d[k];
      L[i][j] = s / v;
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = -g[i];
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s;
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i] / d[i];
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * delta[k];
    delta[i] = s;
  }
  return true;
}

// q' = normalize((d theta / 2, 1)) * q, t' = t + d t
SLIO_HD inline void retract(const double q[4], const double t[3], const double delta[6], double qn[4],
                            double tn[3]) {
  double dq[4] = {delta[0] / 2.0, delta[1] / 2.0, delta[2] / 2.0, 1.0};
  const double n = sqrt(((dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]) + dq[3] * dq[3]);
  for (int k = 0; k < 4; ++k) dq[k] = dq[k] / n;
  qmul(dq, q, qn);
  for (int k = 0; k < 3; ++k) tn[k] = t[k] + delta[3 + k];
}

// First half of an iteration: the gradient stop, the damped solve, the model
// decrease and the proposed point.  Returns false when the solve has stopped
// (s->done), and no evaluation at (qn, tn) is wanted.
SLIO_HD inline bool lm_propose(Lm* s) {
  if (s->done) return false;
  if (s->iterations >= kMaxIter) {
    s->done = 1;
    s->stop = kStopMaxIter;
    return false;
  }
  double gmax = 0.0;
  for (int k = 0; k < 6; ++k) {
    const double a = fabs(s->g[k]);
    if (a > gmax) gmax = a;
  }
  if (gmax <= 1e-10) {
    s->done = 1;
    s->stop = kStopGradient;
    return false;
  }
  s->pivots_ok = ldlt_solve(s->A, s->g, s->mu, s->delta) ? 1 : 0;
  double gd = 0.0, dAd = 0.0;
  for (int i = 0; i < 6; ++i) {
    gd = gd + s->g[i] * s->delta[i];
    double Ad = 0.0;
    for (int j = 0; j < 6; ++j) Ad = Ad + s->A[tri(i, j)] * s->delta[j];
    dAd = dAd + s->delta[i] * Ad;
  }
  s->model = -gd - 0.5 * dAd;
  double xn = 0.0;
  for (int k = 0; k < 4; ++k) xn = xn + s->q[k] * s->q[k];
  for (int k = 0; k < 3; ++k) xn = xn + s->t[k] * s->t[k];
  s->xnorm = sqrt(xn);
  retract(s->q, s->t, s->delta, s->qn, s->tn);
  return true;
}

// Second half: (An, gn, costn) is the evaluation at the proposed point.
SLIO_HD inline void lm_decide(Lm* s, const double An[21], const double gn[6], double costn) {
  ++s->iterations;
  const double rho = (s->cost - costn) / s->model;
  const bool accept = s->pivots_ok && s->model > 0.0 && rho > 1e-3;
  s->last_accepted = accept;
  if (accept) {
    const double tmp = 2.0 * rho - 1.0;
    double f = 1.0 - (tmp * tmp) * tmp;
    if (!(f >= 1.0 / 3.0)) f = 1.0 / 3.0;
    double mu = s->mu / f;
    if (mu > 1e16) mu = 1e16;
    s->mu = mu;
    s->nu = 2.0;
    const double old = s->cost;
    for (int k = 0; k < 4; ++k) s->q[k] = s->qn[k];
    for (int k = 0; k < 3; ++k) s->t[k] = s->tn[k];
    for (int k = 0; k < 21; ++k) s->A[k] = An[k];
    for (int k = 0; k < 6; ++k) s->g[k] = gn[k];
    s->cost = costn;
    ++s->accepted;
    if (fabs(old - costn) <= 1e-6 * old) {
      s->done = 1;
      s->stop = kStopFunction;
      return;
    }
  } else {
    s->mu = s->mu / s->nu;
    s->nu = 2.0 * s->nu;
  }
  double dn = 0.0;
  for (int k = 0; k < 6; ++k) dn = dn + s->delta[k] * s->delta[k];
  if (sqrt(dn) <= 1e-8 * (s->xnorm + 1e-8)) {
    s->done = 1;
    s->stop = kStopParameter;
    return;
  }
  if (s->iterations >= kMaxIter) {
    s->done = 1;
    s->stop = kStopMaxIter;
  }
}

// :600-601, in that order, unnormalised
SLIO_HD inline void integrate(double q_w[4], double t_w[3], const double q_lc[4], const double t_lc[3]) {
  double r[3], qn[4];
  rotate(q_w, t_lc, r);
  for (int k = 0; k < 3; ++k) t_w[k] = t_w[k] + r[k];
  qmul(q_w, q_lc, qn);
  for (int k = 0; k < 4; ++k) q_w[k] = qn[k];
}

}  // namespace aodom
}  // namespace slio
