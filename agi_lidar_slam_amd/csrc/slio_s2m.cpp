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

#include "slio_common.hpp"
#include "slio_cvsolve.hpp"
#include "slio_frontend.h"
#include "slio_icp.hpp"

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
// The host side of the loop-closure ICP (LIO-SAM mapOptmization.cpp:766-780,
// LeGO-LOAM mapOptmization.cpp:957-975, pcl::IterativeClosestPoint): one turn
// of IterativeClosestPoint::computeTransformation's loop on the sums the
// device forms (slio_icp_correspond).  The step itself is slio::icp::step
// (slio_icp.hpp), which the device-resident loop (slio_icp_align) runs
// in-kernel.

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
  slio::icp::step(sums, ncorr, params, st, delta, done);
  return SLIO_OK;
}

}  // extern "C"
