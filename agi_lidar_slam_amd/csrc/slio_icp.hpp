// slio_icp.hpp -- one turn of pcl::IterativeClosestPoint's loop after the
// correspondences, shared by the host export (slio_icp_step, slio_s2m.cpp) and
// the device-resident loop (k_icp_tail, slio_mapopt.hip): the rigid fit of
// TransformationEstimationSVD (pcl::umeyama without scaling), the running
// product final_transformation_ and DefaultConvergenceCriteria::hasConverged.
// PCL is third-party and absent (the reference tree carries no PCL source):
// PCL 1.10's rules are restated here and in slio.h.  One stated difference:
// PCL runs the fit in float (Eigen::JacobiSVD<Matrix3f> on demeaned points);
// here it runs in double on sums of exact products and is rounded to float
// once, at the end.
// Both sides are built with -ffp-contract=off -fno-fast-math, and double
// division and sqrt are correctly rounded on gfx950, so the device step gives
// the host step's bits.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "slio_common.hpp"

namespace slio {
namespace icp {

// R (row-major) = U S V^T of the 3x3 A = U D V^T, S = diag(1, 1, det U det V),
// singular values descending: one-sided Jacobi (Hestenes) on the columns of A.
// Only the two leading left vectors are taken from A V; the third is their
// cross product, whose sign S absorbs:
//   R = u1 v1^T + u2 v2^T + det(V) (u1 x u2) v3^T,
// which also covers a rank-2 A (a planar cloud), where u3 has no column to
// come from.
SLIO_HD inline void umeyama_rotation(const double A[9], double R[9]) {
  double B[3][3], V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      B[i][j] = A[3 * i + j];
      V[i][j] = i == j ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < 60; ++sweep) {
    bool rotated = false;
    for (int p = 0; p < 2; ++p)
      for (int q = p + 1; q < 3; ++q) {
        double alpha = 0, beta = 0, gamma = 0;
        for (int i = 0; i < 3; ++i) {
          alpha += B[i][p] * B[i][p];
          beta += B[i][q] * B[i][q];
          gamma += B[i][p] * B[i][q];
        }
        if (gamma == 0.0 || fabs(gamma) <= DBL_EPSILON * sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int i = 0; i < 3; ++i) {
          const double bp = B[i][p], bq = B[i][q];
          B[i][p] = c * bp - s * bq;
          B[i][q] = s * bp + c * bq;
          const double vp = V[i][p], vq = V[i][q];
          V[i][p] = c * vp - s * vq;
          V[i][q] = s * vp + c * vq;
        }
      }
    if (!rotated) break;
  }
  double nrm[3];
  int ord[3] = {0, 1, 2};
  for (int j = 0; j < 3; ++j) nrm[j] = sqrt(B[0][j] * B[0][j] + B[1][j] * B[1][j] + B[2][j] * B[2][j]);
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (nrm[ord[b]] > nrm[ord[a]]) {
        const int o = ord[a];
        ord[a] = ord[b];
        ord[b] = o;
      }
  double v[3][3], u[3][3];  // v[k], u[k]: k-th right / left singular vector
  for (int k = 0; k < 3; ++k)
    for (int i = 0; i < 3; ++i) v[k][i] = V[i][ord[k]];
  const double s1 = nrm[ord[0]], s2 = nrm[ord[1]];
  if (!(s1 > 0.0)) {  // A == 0 (or not finite): no rotation to find
    for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    return;
  }
  for (int i = 0; i < 3; ++i) u[0][i] = B[i][ord[0]] / s1;
  {
    double w[3] = {B[0][ord[1]], B[1][ord[1]], B[2][ord[1]]};
    if (!(s2 > s1 * 1e-150)) {  // rank 1: any unit vector orthogonal to u1
      const int m = fabs(u[0][0]) <= fabs(u[0][1]) ? (fabs(u[0][0]) <= fabs(u[0][2]) ? 0 : 2)
                                                   : (fabs(u[0][1]) <= fabs(u[0][2]) ? 1 : 2);
      w[0] = w[1] = w[2] = 0.0;
      w[m] = 1.0;
    }
    const double d = w[0] * u[0][0] + w[1] * u[0][1] + w[2] * u[0][2];
    for (int i = 0; i < 3; ++i) w[i] -= d * u[0][i];
    const double l = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    for (int i = 0; i < 3; ++i) u[1][i] = w[i] / l;
  }
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  const double detV = v[0][0] * (v[1][1] * v[2][2] - v[1][2] * v[2][1]) -
                      v[0][1] * (v[1][0] * v[2][2] - v[1][2] * v[2][0]) +
                      v[0][2] * (v[1][0] * v[2][1] - v[1][1] * v[2][0]);
  const double sg = detV < 0.0 ? -1.0 : 1.0;
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) R[3 * r + c] = (u[0][r] * v[0][c] + u[1][r] * v[1][c]) + sg * u[2][r] * v[2][c];
}

// slio_icp_step's body (slio.h holds the specification); the arguments have
// been checked
SLIO_HD inline void step(const double sums[16], int64_t ncorr, const slio_icp_params* params, slio_icp_state* st,
                         float delta[16], int* done) {
  for (int i = 0; i < 16; ++i) delta[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  st->convergence_state = SLIO_ICP_NOT_CONVERGED;
  // min_number_correspondences_ = 3 (icp.hpp: "Not enough correspondences found")
  if (ncorr < 3) {
    st->convergence_state = SLIO_ICP_NO_CORRESPONDENCES;
    st->converged = 0;
    *done = 1;
    return;
  }
  // TransformationEstimationSVD = pcl::umeyama(src, tgt, false), in double
  const double n = (double)ncorr;
  double mp[3], mq[3], A[9], R[9], t[3];
  for (int a = 0; a < 3; ++a) {
    mp[a] = sums[a] / n;
    mq[a] = sums[3 + a] / n;
  }
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) A[3 * r + c] = sums[6 + 3 * r + c] / n - mq[r] * mp[c];
  umeyama_rotation(A, R);
  for (int r = 0; r < 3; ++r) t[r] = mq[r] - ((R[3 * r] * mp[0] + R[3 * r + 1] * mp[1]) + R[3 * r + 2] * mp[2]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) delta[4 * r + c] = (float)R[3 * r + c];
    delta[4 * r + 3] = (float)t[r];
  }
  // final_transformation_ = transformation_ * final_transformation_ (float)
  float F[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      float s = delta[4 * r] * st->final_T[c];
      for (int k = 1; k < 4; ++k) s = s + delta[4 * r + k] * st->final_T[4 * k + c];
      F[4 * r + c] = s;
    }
  for (int i = 0; i < 16; ++i) st->final_T[i] = F[i];
  ++st->iterations;
  // DefaultConvergenceCriteria::hasConverged (max_iterations_similar_transforms_ = 0:
  // the first criterion met converges)
  int state = SLIO_ICP_NOT_CONVERGED;
  const double cosang = 0.5 * (((double)delta[0] + (double)delta[5] + (double)delta[10]) - 1.0);
  const double t2 = ((double)delta[3] * (double)delta[3] + (double)delta[7] * (double)delta[7]) +
                    (double)delta[11] * (double)delta[11];
  const double mse = sums[15] / n;
  if (st->iterations >= params->max_iterations)
    state = SLIO_ICP_ITERATIONS;
  else if (cosang >= 0.99999 && t2 <= params->transformation_epsilon)
    state = SLIO_ICP_TRANSFORM;
  else if (fabs(mse - st->prev_mse) < params->euclidean_fitness_epsilon)
    state = SLIO_ICP_ABS_MSE;
  else if (fabs(mse - st->prev_mse) / st->prev_mse < 1e-5)
    state = SLIO_ICP_REL_MSE;
  if (state != SLIO_ICP_NOT_CONVERGED) {
    st->convergence_state = state;
    st->converged = 1;
    *done = 1;
    return;
  }
  st->similar = 0;
  st->prev_mse = mse;
  st->converged = 0;
  *done = 0;
}

}  // namespace icp
}  // namespace slio
