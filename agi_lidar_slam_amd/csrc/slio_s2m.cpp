// slio_s2m.cpp -- host side of LIO-SAM's LMOptimization
// (src/LIO-SAM/src/mapOptmization.cpp:1627-1700): the 6x6 Gauss-Newton step
// on the normal equations the device forms (slio_s2m_normal_equations), the
// degeneracy projection of the first iteration and the convergence test.
// OpenCV (cv::solve DECOMP_QR, cv::eigen, cv::Mat::inv) is third-party and
// absent; its algorithms are restated in float: Householder QR, the Jacobi
// eigensolver of hal::Jacobi, LU inverse with partial pivoting -- in
// slio_cvsolve.hpp, shared with LeGO-LOAM's 3x3 step.  Below it, the host step
// of the loop-closure ICP (slio_icp_step) and LeGO-LOAM's scan-to-scan step
// (slio_lego_odom_step).
#include <cfloat>
#include <cmath>
#include <cstring>

#include <string>
#include <utility>

#include "slio_common.hpp"
#include "slio_cvsolve.hpp"
#include "slio_frontend.h"

using slio::set_error;
using slio::cvs::inv_lu;
using slio::cvs::jacobi;
using slio::cvs::qr_solve;

// The step LIO-SAM's LMOptimization, LeGO-LOAM's (mapOptmization.cpp:1539-1600)
// and livox_mapping's laserMapping (:1040-1150) share.  They differ in the
// eigenvalue threshold of the degeneracy test (100, 100, 1) and in deltaR:
// pcl::rad2deg(float) is a float product, livox_mapping's own rad2deg (:139)
// a double expression (deg_double).
static int lm_step(const char* who, const float AtA[36], const float AtB[6], int64_t nsel, int iter_count,
                   float transform[6], int* is_degenerate, float matP[36], int* converged, float eig_threshold,
                   bool deg_double) {
  if (!AtA || !AtB || !transform || !is_degenerate || !matP || !converged) {
    set_error(std::string(who) + ": bad arguments");
    return SLIO_EINVAL;
  }
  *converged = 0;
  if (nsel < 50) return 1;  // :1573-1576: too few correspondences, no update
  float X[6];
  // cv::solve(matAtA, matAtB, matX, DECOMP_QR) (:1620): on a (numerically)
  // singular A^T A it returns false with matX zeroed, and LMOptimization
  // ignores the return value -- a zero step, which then reads as converged
  if (!qr_solve<6>(AtA, AtB, X))
    for (float& v : X) v = 0.0f;
  if (iter_count == 0) {
    // :1633-1656: eigen-decomposition of A^T A; directions with eigenvalue
    // below the threshold (100; smallest first) are not updated
    float A[36], E[6], V[36], V2[36];
    std::memcpy(A, AtA, sizeof A);
    jacobi<6>(A, E, V);
    std::memcpy(V2, V, sizeof V);
    *is_degenerate = 0;
    for (int i = 5; i >= 0; --i) {
      if (E[i] < eig_threshold) {
        for (int j = 0; j < 6; ++j) V2[6 * i + j] = 0;
        *is_degenerate = 1;
      } else {
        break;
      }
    }
    float Vi[36];
    if (!inv_lu<6>(V, Vi)) {
      set_error(std::string(who) + ": singular eigenvector matrix");
      return SLIO_EINVAL;
    }
    for (int i = 0; i < 6; ++i)
      for (int j = 0; j < 6; ++j) {
        double s = 0;
        for (int k = 0; k < 6; ++k) s += (double)Vi[6 * i + k] * (double)V2[6 * k + j];
        matP[6 * i + j] = (float)s;
      }
  }
  if (*is_degenerate) {
    float X2[6];
    for (int i = 0; i < 6; ++i) {
      double s = 0;
      for (int k = 0; k < 6; ++k) s += (double)matP[6 * i + k] * (double)X[k];
      X2[i] = (float)s;
    }
    std::memcpy(X, X2, sizeof X);
  }
  for (int k = 0; k < 6; ++k) transform[k] += X[k];
  const float r2d = (float)(180.0 / M_PI);
  float deltaR;
  if (deg_double) {
    auto deg = [](float r) { return (double)r * 180.0 / M_PI; };
    deltaR = std::sqrt(std::pow(deg(X[0]), 2) + std::pow(deg(X[1]), 2) + std::pow(deg(X[2]), 2));
  } else {
    deltaR = std::sqrt(std::pow(X[0] * r2d, 2) + std::pow(X[1] * r2d, 2) + std::pow(X[2] * r2d, 2));
  }
  const float deltaT = std::sqrt(std::pow(X[3] * 100, 2) + std::pow(X[4] * 100, 2) + std::pow(X[5] * 100, 2));
  *converged = (deltaR < 0.05 && deltaT < 0.05) ? 1 : 0;
  return SLIO_OK;
}

extern "C" int slio_s2m_lm_step(const float AtA[36], const float AtB[6], int64_t nsel, int iter_count,
                                float transform[6], int* is_degenerate, float matP[36], int* converged) {
  return lm_step("slio_s2m_lm_step", AtA, AtB, nsel, iter_count, transform, is_degenerate, matP, converged, 100.0f,
                 false);
}

// livox_mapping's step (laserMapping.cpp:1040-1150): eignThre = 1 (:1114), and
// fewer than 50 rows is a `continue` (:1040-1042) -- the turn counts and
// nothing moves, which is what the return value 1 already means to a caller's
// loop.
extern "C" int slio_lvx_lm_step(const float AtA[36], const float AtB[6], int64_t nsel, int iter_count,
                                float transform[6], int* is_degenerate, float matP[36], int* converged) {
  return lm_step("slio_lvx_lm_step", AtA, AtB, nsel, iter_count, transform, is_degenerate, matP, converged, 1.0f,
                 true);
}

// LeGO-LOAM's calculateTransformationSurf / Corner after the normal equations
// (featureAssociation.cpp:1649-1695 / :1764-1814): the host export of the
// code the device loop calls in-kernel (slio::lego::odom_step)
extern "C" int slio_lego_odom_step(int kind, const float AtA[9], const float AtB[3], int32_t nsel, int iter_count,
                                   float transform_cur[6], int* is_degenerate, float matP[9], int* keep_going) {
  if (!AtA || !AtB || !transform_cur || !is_degenerate || !matP || !keep_going ||
      (kind != SLIO_LEGO_ODOM_SURF && kind != SLIO_LEGO_ODOM_CORNER) || iter_count < 0) {
    set_error("slio_lego_odom_step: bad arguments");
    return SLIO_EINVAL;
  }
  *keep_going = 1;
  if (nsel < 10) return 1;  // :2048 / :2061: `continue`
  *keep_going = slio::lego::odom_step(kind, AtA, AtB, iter_count, transform_cur, is_degenerate, matP) ? 1 : 0;
  return SLIO_OK;
}

// ---------------------------------------------------------------- loop-closure ICP, host side
// The host side of LIO-SAM's loop-closure ICP
// (src/LIO-SAM/src/mapOptmization.cpp:766-780, pcl::IterativeClosestPoint):
// one turn of IterativeClosestPoint::computeTransformation's loop on the sums
// the device forms (slio_icp_correspond) -- the rigid fit of
// TransformationEstimationSVD (pcl::umeyama without scaling), the running
// product final_transformation_ and DefaultConvergenceCriteria::hasConverged.
// PCL is third-party and absent (the reference tree carries no PCL source):
// PCL 1.10's rules are restated here and in slio.h.  One stated difference:
// PCL runs the fit in float (Eigen::JacobiSVD<Matrix3f> on demeaned points);
// here it runs in double on sums of exact products and is rounded to float
// once, at the end.

namespace {

// R (row-major) = U S V^T of the 3x3 A = U D V^T, S = diag(1, 1, det U det V),
// singular values descending: one-sided Jacobi (Hestenes) on the columns of A.
// Only the two leading left vectors are taken from A V; the third is their
// cross product, whose sign S absorbs:
//   R = u1 v1^T + u2 v2^T + det(V) (u1 x u2) v3^T,
// which also covers a rank-2 A (a planar cloud), where u3 has no column to
// come from.
void umeyama_rotation(const double A[9], double R[9]) {
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
        if (gamma == 0.0 || std::fabs(gamma) <= DBL_EPSILON * std::sqrt(alpha * beta)) continue;
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
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
  for (int j = 0; j < 3; ++j) nrm[j] = std::sqrt(B[0][j] * B[0][j] + B[1][j] * B[1][j] + B[2][j] * B[2][j]);
  for (int a = 0; a < 2; ++a)
    for (int b = a + 1; b < 3; ++b)
      if (nrm[ord[b]] > nrm[ord[a]]) std::swap(ord[a], ord[b]);
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
      const int m = std::fabs(u[0][0]) <= std::fabs(u[0][1])
                        ? (std::fabs(u[0][0]) <= std::fabs(u[0][2]) ? 0 : 2)
                        : (std::fabs(u[0][1]) <= std::fabs(u[0][2]) ? 1 : 2);
      w[0] = w[1] = w[2] = 0.0;
      w[m] = 1.0;
    }
    const double d = w[0] * u[0][0] + w[1] * u[0][1] + w[2] * u[0][2];
    for (int i = 0; i < 3; ++i) w[i] -= d * u[0][i];
    const double l = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
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

}  // namespace

extern "C" {

int slio_icp_params_default(slio_icp_params* p) {
  if (!p) {
    set_error("slio_icp_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 100;                // icp.setMaximumIterations(100)        (:768)
  p->transformation_epsilon = 1e-6;       // icp.setTransformationEpsilon(1e-6)   (:769)
  p->euclidean_fitness_epsilon = 1e-6;    // icp.setEuclideanFitnessEpsilon(1e-6) (:770)
  return SLIO_OK;
}

int slio_icp_state_init(slio_icp_state* s, const float guess[16]) {
  if (!s) {
    set_error("slio_icp_state_init: null");
    return SLIO_EINVAL;
  }
  std::memset(s, 0, sizeof(*s));
  for (int i = 0; i < 16; ++i) s->final_T[i] = guess ? guess[i] : (i % 5 == 0 ? 1.0f : 0.0f);
  s->prev_mse = DBL_MAX;  // correspondences_prev_mse_ (std::numeric_limits<double>::max())
  return SLIO_OK;
}

int slio_icp_step(const double sums[16], int64_t ncorr, const slio_icp_params* params, slio_icp_state* st,
                  float delta[16], int* done) {
  if (!sums || !params || !st || !delta || !done || ncorr < 0) {
    set_error("slio_icp_step: bad arguments");
    return SLIO_EINVAL;
  }
  for (int i = 0; i < 16; ++i) delta[i] = (i % 5 == 0) ? 1.0f : 0.0f;
  st->convergence_state = SLIO_ICP_NOT_CONVERGED;
  // min_number_correspondences_ = 3 (icp.hpp: "Not enough correspondences found")
  if (ncorr < 3) {
    st->convergence_state = SLIO_ICP_NO_CORRESPONDENCES;
    st->converged = 0;
    *done = 1;
    return SLIO_OK;
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
  std::memcpy(st->final_T, F, sizeof(F));
  ++st->iterations;
  // DefaultConvergenceCriteria::hasConverged (max_iterations_similar_transforms_ = 0:
  // the first criterion met converges)
  auto converge = [&](int state) {
    st->convergence_state = state;
    st->converged = 1;
    *done = 1;
    return SLIO_OK;
  };
  if (st->iterations >= params->max_iterations) return converge(SLIO_ICP_ITERATIONS);
  const double cosang = 0.5 * (((double)delta[0] + (double)delta[5] + (double)delta[10]) - 1.0);
  const double t2 = ((double)delta[3] * (double)delta[3] + (double)delta[7] * (double)delta[7]) +
                    (double)delta[11] * (double)delta[11];
  if (cosang >= 0.99999 && t2 <= params->transformation_epsilon) return converge(SLIO_ICP_TRANSFORM);
  const double mse = sums[15] / n;
  if (std::fabs(mse - st->prev_mse) < params->euclidean_fitness_epsilon) return converge(SLIO_ICP_ABS_MSE);
  if (std::fabs(mse - st->prev_mse) / st->prev_mse < 1e-5) return converge(SLIO_ICP_REL_MSE);
  st->similar = 0;
  st->prev_mse = mse;
  st->converged = 0;
  *done = 0;
  return SLIO_OK;
}

}  // extern "C"
