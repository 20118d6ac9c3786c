// slio_aloam_map.hpp -- the formulas of A-LOAM's laserMapping
// (src/A-LOAM/src/laserMapping.cpp, the loop body of process() :326-893 with
// LidarEdgeFactor and LidarPlaneNormFactor of lidarFactor.hpp), written once
// for the host restatement (slio_aloam_map.cpp) and for the kernels
// (slio_aloam_map.hip).  Internal to the library.
//
// As in slio_aloam_odom.hpp everything is + - * / sqrt in IEEE double (float
// where the reference holds floats), every sum written out in one association
// order, so that under -ffp-contract=off the device, the host and a numpy
// model agree to the bit.  A quaternion is (x, y, z, w).  The weighting
// (HuberLoss 0.1), the controller and the retraction are slio_aloam_odom.hpp's,
// unchanged; max_num_iterations is 4 here too (:811).
//
// The 3 x 3 eigen-solve (jacobi3) and the 5 x 3 least-squares solve
// (qr_solve_m1) are this library's text: Eigen is third-party and absent, so
// parity with SelfAdjointEigenSolver and with Eigen's own summation order
// inside colPivHouseholderQr is unpinned.  jacobi3 IS the specification of the
// eigen-solve.
#pragma once

#include <cmath>
#include <cstdint>

#include "slio_aloam_odom.hpp"
#include "slio_common.hpp"

namespace slio {
namespace amap {

using aodom::Factor;
using aodom::kSums;

// laserCloudWidth / Height / Depth (:105-107) and laserCloudNum (:109), index i + 21 j + 441 k
constexpr int kW = 21, kH = 21, kD = 11, kNum = kW * kH * kD;
constexpr int kMaxListed = 75;     // 5 x 5 x 3 (:566-583)
constexpr int kK = 5;              // nearestKSearch(.., 5, ..)
constexpr float kGate = 1.0f;      // pointSearchSqDis[4] < 1.0 (:647, :730)
constexpr int kWg = 256;           // factor slots per workgroup of the evaluation
constexpr int kLanes = 32;         // strided partial sums per entry, at both levels
constexpr int kJacobiSweeps = 8;
// what a factor slot holds after the association
enum { kNone = 0, kEdge = 1, kPlane = 2, kDegenerate = 3, kRejected = 4 };

// ---- poses ----------------------------------------------------------------
SLIO_HD inline double sqnorm4(const double q[4]) { return ((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]; }

// transformAssociateToMap (:148-152), and the high-frequency pose of
// laserOdometryHandler (:222-223), which is the same expression
SLIO_HD inline void associate_to_map(const double q_wmap[4], const double t_wmap[3], const double q_wodom[4],
                                     const double t_wodom[3], double q_w[4], double t_w[3]) {
  double r[3];
  aodom::qmul(q_wmap, q_wodom, q_w);
  aodom::rotate(q_wmap, t_wodom, r);
  for (int a = 0; a < 3; ++a) t_w[a] = r[a] + t_wmap[a];
}

// transformUpdate (:155-158); Eigen's inverse() is the conjugate over the squared norm
SLIO_HD inline void transform_update(const double q_w[4], const double t_w[3], const double q_wodom[4],
                                     const double t_wodom[3], double q_wmap[4], double t_wmap[3]) {
  const double n2 = sqnorm4(q_wodom);
  const double inv[4] = {-q_wodom[0] / n2, -q_wodom[1] / n2, -q_wodom[2] / n2, q_wodom[3] / n2};
  double r[3];
  aodom::qmul(q_w, inv, q_wmap);
  aodom::rotate(q_wmap, t_wodom, r);
  for (int a = 0; a < 3; ++a) t_wmap[a] = t_w[a] - r[a];
}

// pointAssociateToMap (:160-168) is q * p + t in double, rounded to float: aodom::to_start.

// ---- cube indices -----------------------------------------------------------
// The centre cube (:331-338) comes from the DOUBLE t_w_curr; a point's cube
// (:839-845) from its float coordinate, which is slio::lvx::cube_of.
SLIO_HD inline bool cube_of(double t, int cen, int* cube) {
  const double v = t + 25.0;
  if (!(fabs(v) < 1.0e6)) return false;
  int c = (int)(v / 50.0) + cen;
  if (v < 0) --c;
  *cube = c;
  return true;
}

// :331-583: the centre cube, the six shift loops composed (every cube moves by
// shift, cen with it), and the cubes i +- 2, j +- 2, k +- 1 inside the array,
// k innermost: each is both valid and surround.  No field-of-view test.
// Non-zero: a coordinate beyond 1e6 m.
inline int select(const double t_w[3], int32_t cen[3], int32_t center[3], int32_t shift[3], int32_t* list,
                  int32_t* n) {
  const int dim[3] = {kW, kH, kD};
  int c[3];
  for (int a = 0; a < 3; ++a) {
    if (!cube_of(t_w[a], cen[a], &c[a])) return 1;
    shift[a] = 0;
    while (c[a] < 3) {
      ++c[a];
      ++cen[a];
      ++shift[a];
    }
    while (c[a] >= dim[a] - 3) {
      --c[a];
      --cen[a];
      --shift[a];
    }
    center[a] = c[a];
  }
  int m = 0;
  for (int i = c[0] - 2; i <= c[0] + 2; ++i)
    for (int j = c[1] - 2; j <= c[1] + 2; ++j)
      for (int k = c[2] - 1; k <= c[2] + 1; ++k)
        if (i >= 0 && i < kW && j >= 0 && j < kH && k >= 0 && k < kD) list[m++] = i + kW * j + kW * kH * k;
  *n = m;
  return 0;
}

// ---- the line fit (:648-691) ------------------------------------------------
// One rotation of the cyclic Jacobi method on the symmetric A, in the plane
// (P, Q), R the third index; V's columns follow.  Nothing happens for a zero
// off-diagonal entry.  (theta * theta may overflow to +inf: t is then 0.)
template <int P, int Q, int R>
SLIO_HD inline void jacobi_rotate(double (&A)[3][3], double (&V)[3][3]) {
  const double apq = A[P][Q];
  if (apq == 0.0) return;
  const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
  double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  A[P][P] = A[P][P] - t * apq;
  A[Q][Q] = A[Q][Q] + t * apq;
  A[P][Q] = A[Q][P] = 0.0;
  const double arp = A[R][P], arq = A[R][Q];
  A[R][P] = A[P][R] = c * arp - s * arq;
  A[R][Q] = A[Q][R] = s * arp + c * arq;
  for (int k = 0; k < 3; ++k) {
    const double vp = V[k][P], vq = V[k][Q];
    V[k][P] = c * vp - s * vq;
    V[k][Q] = s * vp + c * vq;
  }
}

// eigenvalues lam and eigenvectors (the columns of V) of the symmetric matrix
// m = {xx, xy, xz, yy, yz, zz}: kJacobiSweeps sweeps over (0,1), (0,2), (1,2)
SLIO_HD inline void jacobi3(const double m[6], double lam[3], double (&V)[3][3]) {
  double A[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = i == j ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    jacobi_rotate<0, 1, 2>(A, V);
    jacobi_rotate<0, 2, 1>(A, V);
    jacobi_rotate<1, 2, 0>(A, V);
  }
  for (int i = 0; i < 3; ++i) lam[i] = A[i][i];
}

// nb: the five neighbours, nearest first.  kEdge with the end points a, b =
// centre +- 0.1 direction; kRejected where the largest eigenvalue is not above
// three times the middle one; kDegenerate for a zero (or non-finite)
// covariance.  The sign of the direction is free: it swaps a and b, which
// flips r and J of the edge factor together and leaves J^T J and J^T r unchanged.
SLIO_HD inline int fit_line(const double (&nb)[kK][3], double a[3], double b[3]) {
  double c[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < kK; ++j)
    for (int k = 0; k < 3; ++k) c[k] = c[k] + nb[j][k];
  for (int k = 0; k < 3; ++k) c[k] = c[k] / 5.0;
  double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int j = 0; j < kK; ++j) {
    const double z0 = nb[j][0] - c[0], z1 = nb[j][1] - c[1], z2 = nb[j][2] - c[2];
    m[0] = m[0] + z0 * z0;
    m[1] = m[1] + z0 * z1;
    m[2] = m[2] + z0 * z2;
    m[3] = m[3] + z1 * z1;
    m[4] = m[4] + z1 * z2;
    m[5] = m[5] + z2 * z2;
  }
  double lam[3], V[3][3];
  jacobi3(m, lam, V);
  // the largest (the first of equal ones) and the larger of the other two
  const int hi = lam[1] > lam[0] ? (lam[2] > lam[1] ? 2 : 1) : (lam[2] > lam[0] ? 2 : 0);
  const int o1 = hi == 0 ? 1 : 0, o2 = hi == 2 ? 1 : 2;
  const double mid = lam[o2] > lam[o1] ? lam[o2] : lam[o1];
  if (!(lam[hi] > 0.0) || !(lam[hi] - lam[hi] == 0.0)) return kDegenerate;
  if (!(lam[hi] > 3.0 * mid)) return kRejected;
  for (int k = 0; k < 3; ++k) {
    const double d = hi == 0 ? V[k][0] : hi == 1 ? V[k][1] : V[k][2];
    a[k] = 0.1 * d + c[k];
    b[k] = -0.1 * d + c[k];
  }
  return kEdge;
}

// ---- the plane fit (:725-766) -----------------------------------------------
SLIO_HD inline void qr_swap_cols(double (&a)[3][kK], double (&nu)[3], double (&nd)[3], int c0, int c1) {
  for (int r = 0; r < kK; ++r) {
    const double x = a[c0][r];
    a[c0][r] = a[c1][r];
    a[c1][r] = x;
  }
  double x = nu[c0];
  nu[c0] = nu[c1];
  nu[c1] = x;
  x = nd[c0];
  nd[c0] = nd[c1];
  nd[c1] = x;
}

// A x = -1 for the 5 x 3 A of the neighbours: slio_plane.hpp's algorithm
// (Eigen's ColPivHouseholderQR: computeInPlace with the LAPACK norm downdate,
// makeHouseholder, the Householder sequence applied H_0 first, back
// substitution on the leading rank rows, the column permutation) on doubles,
// every reduction summed left to right.  Returns the rank Eigen would report
// (nonzeroPivots); sol is Eigen's solve() for that rank.
SLIO_HD inline int qr_solve_m1(const double (&nb)[kK][3], double sol[3]) {
  const double kEps = 2.220446049250313e-16;     // DBL_EPSILON
  const double kTiny = 2.2250738585072014e-308;  // DBL_MIN
  double a[3][kK];  // a[column][row]
  for (int c = 0; c < 3; ++c)
    for (int r = 0; r < kK; ++r) a[c][r] = nb[r][c];
  double nd[3], nu[3];
  for (int c = 0; c < 3; ++c) {
    double s = a[c][0] * a[c][0];
    for (int r = 1; r < kK; ++r) s = s + a[c][r] * a[c][r];
    nd[c] = sqrt(s);
    nu[c] = nd[c];
  }
  double mx = nu[0];
  if (nu[1] > mx) mx = nu[1];
  if (nu[2] > mx) mx = nu[2];
  const double th_tmp = mx * kEps;
  const double threshold_helper = (th_tmp * th_tmp) / 5.0;
  const double norm_downdate_threshold = sqrt(kEps);
  int nzp = 3;
  int perm[3] = {0, 1, 2};
  double hc[3];
  for (int k = 0; k < 3; ++k) {
    int big = k;  // the biggest remaining column norm, the first maximum wins
    double bv = nu[k];
    for (int j = k + 1; j < 3; ++j)
      if (nu[j] > bv) {
        bv = nu[j];
        big = j;
      }
    if (nzp == 3 && bv * bv < threshold_helper * (double)(kK - k)) nzp = k;
    for (int j = k + 1; j < 3; ++j)  // (indices known after unrolling: the tile stays in registers on the device)
      if (big == j) {
        qr_swap_cols(a, nu, nd, k, j);
        const int p = perm[k];
        perm[k] = perm[j];
        perm[j] = p;
      }
    // makeHouseholderInPlace on a[k][k .. 4]
    double tail_sq = 0.0;
    for (int r = k + 1; r < kK; ++r) tail_sq = r == k + 1 ? a[k][r] * a[k][r] : tail_sq + a[k][r] * a[k][r];
    const double c0 = a[k][k];
    double tau, beta;
    if (tail_sq <= kTiny) {
      tau = 0.0;
      beta = c0;
      for (int r = k + 1; r < kK; ++r) a[k][r] = 0.0;
    } else {
      beta = sqrt(c0 * c0 + tail_sq);
      if (c0 >= 0.0) beta = -beta;
      const double den = c0 - beta;
      for (int r = k + 1; r < kK; ++r) a[k][r] = a[k][r] / den;
      tau = (beta - c0) / beta;
    }
    a[k][k] = beta;
    hc[k] = tau;
    // applyHouseholderOnTheLeft to the trailing columns
    if (tau != 0.0)
      for (int j = k + 1; j < 3; ++j) {
        double t = 0.0;
        for (int r = k + 1; r < kK; ++r) t = r == k + 1 ? a[k][r] * a[j][r] : t + a[k][r] * a[j][r];
        t = t + a[j][k];
        a[j][k] = a[j][k] - tau * t;
        for (int r = k + 1; r < kK; ++r) a[j][r] = a[j][r] - (tau * a[k][r]) * t;
      }
    // the column-norm downdate (LAPACK lawn176)
    for (int j = k + 1; j < 3; ++j)
      if (nu[j] != 0.0) {
        double temp = fabs(a[j][k]) / nu[j];
        temp = (1.0 + temp) * (1.0 - temp);
        temp = temp < 0.0 ? 0.0 : temp;
        const double q = nu[j] / nd[j];
        const double temp2 = temp * (q * q);
        if (temp2 <= norm_downdate_threshold) {
          double s = 0.0;
          for (int r = k + 1; r < kK; ++r) s = r == k + 1 ? a[j][r] * a[j][r] : s + a[j][r] * a[j][r];
          nd[j] = sqrt(s);
          nu[j] = nd[j];
        } else {
          nu[j] = nu[j] * sqrt(temp);
        }
      }
  }
  sol[0] = sol[1] = sol[2] = 0.0;
  if (nzp > 0) {
    double c[kK] = {-1.0, -1.0, -1.0, -1.0, -1.0};
    for (int k = 0; k < 3; ++k)  // c = Q^T c, H_0 first
      if (k < nzp && hc[k] != 0.0) {
        const double tau = hc[k];
        double t = 0.0;
        for (int r = k + 1; r < kK; ++r) t = r == k + 1 ? a[k][r] * c[r] : t + a[k][r] * c[r];
        t = t + c[k];
        c[k] = c[k] - tau * t;
        for (int r = k + 1; r < kK; ++r) c[r] = c[r] - (tau * a[k][r]) * t;
      }
    for (int i = 2; i >= 0; --i)  // back substitution on the leading nzp rows
      if (i < nzp && c[i] != 0.0) {
        c[i] = c[i] / a[i][i];
        for (int r = 0; r < i; ++r) c[r] = c[r] - c[i] * a[i][r];
      }
    for (int i = 0; i < 3; ++i)
      if (i < nzp)
        for (int k = 0; k < 3; ++k) sol[k] = perm[i] == k ? c[i] : sol[k];
  }
  return nzp;
}

// kPlane with the unit normal n and d = 1 / |x| where every neighbour lies
// within 0.2 of the plane; kRejected where one does not; kDegenerate for a
// rank-deficient system or a normal that is not finite.
SLIO_HD inline int fit_plane(const double (&nb)[kK][3], double n[3], double* d) {
  double sol[3];
  const int rank = qr_solve_m1(nb, sol);
  const double len = sqrt((sol[0] * sol[0] + sol[1] * sol[1]) + sol[2] * sol[2]);
  *d = 1.0 / len;
  for (int k = 0; k < 3; ++k) n[k] = sol[k] / len;
  if (rank < 3 || !(n[0] - n[0] == 0.0 && n[1] - n[1] == 0.0 && n[2] - n[2] == 0.0 && *d - *d == 0.0))
    return kDegenerate;
  for (int j = 0; j < kK; ++j)
    if (fabs(((n[0] * nb[j][0] + n[1] * nb[j][1]) + n[2] * nb[j][2]) + *d) > 0.2) return kRejected;
  return kPlane;
}

// the fit of one class on the five neighbours: the slot's kind and its record
// (edge: a, b; plane: n, d, two zeros)
SLIO_HD inline int fit(int surf, const double (&nb)[kK][3], double rec[6]) {
  for (int k = 0; k < 6; ++k) rec[k] = 0.0;
  const int kind = surf ? fit_plane(nb, rec, rec + 3) : fit_line(nb, rec, rec + 3);
  if (kind != kEdge && kind != kPlane)
    for (int k = 0; k < 6; ++k) rec[k] = 0.0;
  return kind;
}

// ---- factors ------------------------------------------------------------------
// LidarEdgeFactor (lidarFactor.hpp:12-67) with DOUBLE end points:
// aodom::edge_factor's expressions on doubles
SLIO_HD inline void edge_factor(const double q[4], const double t[3], const float* cpf, const double a[3],
                                const double b[3], Factor* f) {
  const double cp[3] = {(double)cpf[0], (double)cpf[1], (double)cpf[2]};
  double rc[3], lp[3], d1[3], d2[3], de[3], nu[3];
  aodom::rotate(q, cp, rc);
  for (int k = 0; k < 3; ++k) {
    lp[k] = rc[k] + t[k];
    d1[k] = lp[k] - a[k];
    d2[k] = lp[k] - b[k];
    de[k] = a[k] - b[k];
  }
  const double n = sqrt((de[0] * de[0] + de[1] * de[1]) + de[2] * de[2]);
  if (n == 0.0) {
    f->rows = 0;
    return;
  }
  aodom::cross3(d1, d2, nu);
  const double m[3] = {(b[0] - a[0]) / n, (b[1] - a[1]) / n, (b[2] - a[2]) / n};
  const double E[3][3] = {{0.0, -m[2], m[1]}, {m[2], 0.0, -m[0]}, {-m[1], m[0], 0.0}};
  f->rows = 3;
  for (int i = 0; i < 3; ++i) {
    f->r[i] = nu[i] / n;
    aodom::cross3(rc, E[i], f->J[i]);
    for (int k = 0; k < 3; ++k) f->J[i][3 + k] = E[i][k];
  }
}

// LidarPlaneNormFactor (lidarFactor.hpp:127-164): r = n . (q cp + t) + d, J = [(q cp) x n, n]
SLIO_HD inline void plane_norm_factor(const double q[4], const double t[3], const float* cpf, const double n[3],
                                      double d, Factor* f) {
  const double cp[3] = {(double)cpf[0], (double)cpf[1], (double)cpf[2]};
  double rc[3], lp[3];
  aodom::rotate(q, cp, rc);
  for (int k = 0; k < 3; ++k) lp[k] = rc[k] + t[k];
  f->rows = 1;
  f->r[0] = ((n[0] * lp[0] + n[1] * lp[1]) + n[2] * lp[2]) + d;
  aodom::cross3(rc, n, f->J[0]);
  for (int k = 0; k < 3; ++k) f->J[0][3 + k] = n[k];
}

// the factor of a slot at (q, t): rows (0: the slot holds none)
SLIO_HD inline int slot_factor(const double q[4], const double t[3], const float* cpf, int kind, const double rec[6],
                               Factor* f) {
  f->rows = 0;
  if (kind == kEdge) edge_factor(q, t, cpf, rec, rec + 3, f);
  else if (kind == kPlane) plane_norm_factor(q, t, cpf, rec, rec[3], f);
  return f->rows;
}

// ---- the order of the sums --------------------------------------------------------
// A function of the slot index only.  Slots are the corner stack, then the
// surf stack.  Level 1, per group w of kWg slots: lane l adds the valid slots
// kWg w + l, + kLanes, ... in ascending order, the kLanes lanes are added in
// ascending order: the group's partial.  Level 2, over the groups' partials:
// the same two steps with the group index in the place of the slot.
//
// lane_sum: the items begin + lane, + kLanes, ... < end of v (stride doubles
// apart), skipping those whose valid byte is 0 (valid null: none skipped)
SLIO_HD inline double lane_sum(const double* v, int stride, const uint8_t* valid, int begin, int end, int lane) {
  double acc = 0.0;
  for (int s = begin + lane; s < end; s += kLanes)
    if (!valid || valid[s]) acc = acc + v[(int64_t)s * stride];
  return acc;
}
SLIO_HD inline double lanes_total(const double* part) {
  double tot = 0.0;
  for (int l = 0; l < kLanes; ++l) tot = tot + part[l];
  return tot;
}

}  // namespace amap
}  // namespace slio
