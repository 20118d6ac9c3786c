// slio_cvsolve.hpp -- the small dense solvers the LOAM-family optimisers take
// from OpenCV (cv::solve DECOMP_QR, cv::eigen, cv::Mat::inv), restated in
// float and templated on the size: 6 for LIO-SAM's LMOptimization
// (slio_s2m.cpp), 3 for LeGO-LOAM's two-stage scan-to-scan step, which is
// written here once for the host entry (slio_lego_odom_step) and for the
// device loop (slio_lego_odom.hip); 5 x 3 for the plane fit of LeGO-LOAM's
// mapping (slio_mapopt.hip, k_lmap_coeff). OpenCV is third-party and absent:
// what is written here is the specification of these solvers.
#pragma once

#include <cfloat>
#include <cmath>

#include "slio_common.hpp"

namespace slio {
namespace cvs {

template <class T>
SLIO_HD inline void swap_(T& a, T& b) {
  const T t = a;
  a = b;
  b = t;
}

// OpenCV lapack.cpp hypot
SLIO_HD inline float cv_hypot(float a, float b) {
  a = fabsf(a);
  b = fabsf(b);
  if (a > b) {
    b /= a;
    return a * sqrtf(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * sqrtf(1 + a * a);
  }
  return 0;
}

// OpenCV hal::Jacobi (JacobiImpl_) on an N x N symmetric float matrix:
// eigenvalues W descending, eigenvectors the rows of V
template <int N>
SLIO_HD inline void jacobi(float* A, float* W, float* V) {
  constexpr int n = N;
  const float eps = 1.1920928955078125e-07f;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) V[i * n + j] = (i == j) ? 1.0f : 0.0f;
  int indR[N], indC[N];
  float mv;
  for (int k = 0; k < n; ++k) {
    W[k] = A[(n + 1) * k];
    if (k < n - 1) {
      int m = k + 1;
      mv = fabsf(A[n * k + m]);
      for (int i = k + 2; i < n; ++i) {
        const float val = fabsf(A[n * k + i]);
        if (mv < val) mv = val, m = i;
      }
      indR[k] = m;
    }
    if (k > 0) {
      int m = 0;
      mv = fabsf(A[k]);
      for (int i = 1; i < k; ++i) {
        const float val = fabsf(A[n * i + k]);
        if (mv < val) mv = val, m = i;
      }
      indC[k] = m;
    }
  }
  if (n > 1)
    for (int iters = 0; iters < n * n * 30; ++iters) {
      int k = 0;
      mv = fabsf(A[indR[0]]);
      for (int i = 1; i < n - 1; ++i) {
        const float val = fabsf(A[n * i + indR[i]]);
        if (mv < val) mv = val, k = i;
      }
      int l = indR[k];
      for (int i = 1; i < n; ++i) {
        const float val = fabsf(A[n * indC[i] + i]);
        if (mv < val) mv = val, k = indC[i], l = i;
      }
      const float p = A[n * k + l];
      if (fabsf(p) <= eps) break;
      float y = (float)((W[l] - W[k]) * 0.5);
      float t = fabsf(y) + cv_hypot(p, y);
      float s = cv_hypot(p, t);
      const float c = t / s;
      s = p / s;
      t = (p / t) * p;
      if (y < 0) s = -s, t = -t;
      A[n * k + l] = 0;
      W[k] -= t;
      W[l] += t;
      float a0, b0;
#define SLIO_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * s, v1 = a0 * s + b0 * c
      for (int i = 0; i < k; ++i) SLIO_ROT(A[n * i + k], A[n * i + l]);
      for (int i = k + 1; i < l; ++i) SLIO_ROT(A[n * k + i], A[n * i + l]);
      for (int i = l + 1; i < n; ++i) SLIO_ROT(A[n * k + i], A[n * l + i]);
      for (int i = 0; i < n; ++i) SLIO_ROT(V[n * k + i], V[n * l + i]);
#undef SLIO_ROT
      for (int j = 0; j < 2; ++j) {
        const int idx = j == 0 ? k : l;
        if (idx < n - 1) {
          int m = idx + 1;
          mv = fabsf(A[n * idx + m]);
          for (int i = idx + 2; i < n; ++i) {
            const float val = fabsf(A[n * idx + i]);
            if (mv < val) mv = val, m = i;
          }
          indR[idx] = m;
        }
        if (idx > 0) {
          int m = 0;
          mv = fabsf(A[idx]);
          for (int i = 1; i < idx; ++i) {
            const float val = fabsf(A[n * i + idx]);
            if (mv < val) mv = val, m = i;
          }
          indC[idx] = m;
        }
      }
    }
  for (int k = 0; k < n - 1; ++k) {
    int m = k;
    for (int i = k + 1; i < n; ++i)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      swap_(W[m], W[k]);
      for (int i = 0; i < n; ++i) swap_(V[n * m + i], V[n * k + i]);
    }
  }
}

// A x = b (M x N, M >= N, float, A row-major) by Householder QR, in the least
// squares sense when M > N: cv::solve(A, b, x, cv::DECOMP_QR).  OpenCV is
// third-party and absent here, so THIS RESTATEMENT IS THE SPECIFICATION of
// the solve: one Householder reflection per column k over rows k..M-1, applied
// to the remaining columns and to b, then back-substitution on the top N rows
// of R.  false where OpenCV's QRImpl gives up (hal::QR32f with eps =
// 10 * FLT_EPSILON: a diagonal entry of R below eps in magnitude); the caller
// zeroes x then, as cv::solve leaves matX.  M == N is LIO-SAM's 6 x 6 and
// LeGO-LOAM's 3 x 3 step; M = 5, N = 3 is the plane fit of LeGO-LOAM's
// surfOptimization (mapOptmization.cpp:1395).
template <int M, int N>
SLIO_HD inline bool qr_solve_mn(const float* A_in, const float* b_in, float* x) {
  static_assert(M >= N, "qr_solve_mn: M >= N");
  float A[M * N], b[M];
  for (int i = 0; i < M * N; ++i) A[i] = A_in[i];
  for (int i = 0; i < M; ++i) b[i] = b_in[i];
  for (int k = 0; k < N; ++k) {
    float nrm = 0;
    for (int i = k; i < M; ++i) nrm += A[N * i + k] * A[N * i + k];
    nrm = sqrtf(nrm);
    if (nrm == 0) return false;
    const float alpha = A[N * k + k] > 0 ? -nrm : nrm;
    float v[M];
    for (int i = 0; i < M; ++i) v[i] = 0;
    for (int i = k; i < M; ++i) v[i] = A[N * i + k];
    v[k] -= alpha;
    float vv = 0;
    for (int i = k; i < M; ++i) vv += v[i] * v[i];
    if (vv == 0) continue;
    for (int j = k; j < N; ++j) {
      float d = 0;
      for (int i = k; i < M; ++i) d += v[i] * A[N * i + j];
      const float f = 2 * d / vv;
      for (int i = k; i < M; ++i) A[N * i + j] -= f * v[i];
    }
    float d = 0;
    for (int i = k; i < M; ++i) d += v[i] * b[i];
    const float f = 2 * d / vv;
    for (int i = k; i < M; ++i) b[i] -= f * v[i];
  }
  for (int i = N - 1; i >= 0; --i) {
    float s = b[i];
    for (int j = i + 1; j < N; ++j) s -= A[N * i + j] * x[j];
    if (fabsf(A[N * i + i]) < 10.0f * FLT_EPSILON) return false;
    x[i] = s / A[N * i + i];
  }
  return true;
}

// the square case
template <int N>
SLIO_HD inline bool qr_solve(const float* A_in, const float* b_in, float* x) {
  return qr_solve_mn<N, N>(A_in, b_in, x);
}

// inverse by LU with partial pivoting (cv::Mat::inv, DECOMP_LU, N > 3)
template <int N>
SLIO_HD inline bool inv_lu(const float* M, float* out) {
  float a[N * N], b[N * N];
  for (int i = 0; i < N * N; ++i) a[i] = M[i];
  for (int i = 0; i < N * N; ++i) b[i] = (i % (N + 1) == 0) ? 1.0f : 0.0f;
  for (int k = 0; k < N; ++k) {
    int p = k;
    for (int i = k + 1; i < N; ++i)
      if (fabsf(a[N * i + k]) > fabsf(a[N * p + k])) p = i;
    if (a[N * p + k] == 0) return false;
    if (p != k)
      for (int j = 0; j < N; ++j) {
        swap_(a[N * p + j], a[N * k + j]);
        swap_(b[N * p + j], b[N * k + j]);
      }
    for (int i = k + 1; i < N; ++i) {
      const float f = a[N * i + k] / a[N * k + k];
      for (int j = k; j < N; ++j) a[N * i + j] -= f * a[N * k + j];
      for (int j = 0; j < N; ++j) b[N * i + j] -= f * b[N * k + j];
    }
  }
  for (int c = 0; c < N; ++c)
    for (int i = N - 1; i >= 0; --i) {
      float s = b[N * i + c];
      for (int j = i + 1; j < N; ++j) s -= a[N * i + j] * out[N * j + c];
      out[N * i + c] = s / a[N * i + i];
    }
  return true;
}

// cv::invert on a 3 x 3 float matrix: OpenCV does not run LU there but the
// adjugate over the determinant, both in double, each entry rounded to float
// once; a zero determinant gives the zero matrix
SLIO_HD inline bool inv3(const float* S, float* t) {
#define SLIO_S(r, c) ((double)S[3 * (r) + (c)])
  double d = SLIO_S(0, 0) * (SLIO_S(1, 1) * SLIO_S(2, 2) - SLIO_S(1, 2) * SLIO_S(2, 1)) -
             SLIO_S(0, 1) * (SLIO_S(1, 0) * SLIO_S(2, 2) - SLIO_S(1, 2) * SLIO_S(2, 0)) +
             SLIO_S(0, 2) * (SLIO_S(1, 0) * SLIO_S(2, 1) - SLIO_S(1, 1) * SLIO_S(2, 0));
  if (d == 0.0) {
    for (int i = 0; i < 9; ++i) t[i] = 0.0f;
    return false;
  }
  d = 1.0 / d;
  t[0] = (float)((SLIO_S(1, 1) * SLIO_S(2, 2) - SLIO_S(1, 2) * SLIO_S(2, 1)) * d);
  t[1] = (float)((SLIO_S(0, 2) * SLIO_S(2, 1) - SLIO_S(0, 1) * SLIO_S(2, 2)) * d);
  t[2] = (float)((SLIO_S(0, 1) * SLIO_S(1, 2) - SLIO_S(0, 2) * SLIO_S(1, 1)) * d);
  t[3] = (float)((SLIO_S(1, 2) * SLIO_S(2, 0) - SLIO_S(1, 0) * SLIO_S(2, 2)) * d);
  t[4] = (float)((SLIO_S(0, 0) * SLIO_S(2, 2) - SLIO_S(0, 2) * SLIO_S(2, 0)) * d);
  t[5] = (float)((SLIO_S(0, 2) * SLIO_S(1, 0) - SLIO_S(0, 0) * SLIO_S(1, 2)) * d);
  t[6] = (float)((SLIO_S(1, 0) * SLIO_S(2, 1) - SLIO_S(1, 1) * SLIO_S(2, 0)) * d);
  t[7] = (float)((SLIO_S(0, 1) * SLIO_S(2, 0) - SLIO_S(0, 0) * SLIO_S(2, 1)) * d);
  t[8] = (float)((SLIO_S(0, 0) * SLIO_S(1, 1) - SLIO_S(0, 1) * SLIO_S(1, 0)) * d);
#undef SLIO_S
  return true;
}

}  // namespace cvs

namespace lego {

enum { kOdomSurf = 0, kOdomCorner = 1 };

// calculateTransformationSurf / calculateTransformationCorner after the
// normal equations (featureAssociation.cpp:1649-1695 / :1764-1814): the 3 x 3
// solve, on iteration 0 the eigen-decomposition and matP (thresholds
// {10, 10, 10}), the isDegenerate projection, the update of the kind's three
// components of transformCur (surf: rx, rz, ty; corner: ry, tx, tz), the isnan
// reset and the convergence test.  Returns the function's bool: false =
// converged (the caller breaks).  A singular AtA leaves matX zero, as
// cv::solve does when it fails; that zero step reads as converged.
// Float matrix products accumulate in double and round once (cv::gemm's
// worktype), pow(x, 2) is x * x in double.
SLIO_HD inline bool odom_step(int kind, const float AtA[9], const float AtB[3], int iter_count, float tc[6],
                              int* is_degenerate, float matP[9]) {
  float X[3];
  if (!cvs::qr_solve<3>(AtA, AtB, X)) X[0] = X[1] = X[2] = 0.0f;
  if (iter_count == 0) {
    float A[9], E[3], V[9], V2[9], Vi[9];
    for (int i = 0; i < 9; ++i) A[i] = AtA[i];
    cvs::jacobi<3>(A, E, V);
    for (int i = 0; i < 9; ++i) V2[i] = V[i];
    *is_degenerate = 0;
    for (int i = 2; i >= 0; --i) {
      if (E[i] < 10.0f) {
        for (int j = 0; j < 3; ++j) V2[3 * i + j] = 0;
        *is_degenerate = 1;
      } else {
        break;
      }
    }
    cvs::inv3(V, Vi);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double s = 0;
        for (int k = 0; k < 3; ++k) s += (double)Vi[3 * i + k] * (double)V2[3 * k + j];
        matP[3 * i + j] = (float)s;
      }
  }
  if (*is_degenerate) {
    float X2[3];
    for (int i = 0; i < 3; ++i) {
      double s = 0;
      for (int k = 0; k < 3; ++k) s += (double)matP[3 * i + k] * (double)X[k];
      X2[i] = (float)s;
    }
    for (int i = 0; i < 3; ++i) X[i] = X2[i];
  }
  if (kind == kOdomSurf) {
    tc[0] += X[0];
    tc[2] += X[1];
    tc[4] += X[2];
  } else {
    tc[1] += X[0];
    tc[3] += X[1];
    tc[5] += X[2];
  }
  for (int i = 0; i < 6; ++i)
    if (tc[i] != tc[i]) tc[i] = 0;
  float deltaR, deltaT;
  if (kind == kOdomSurf) {
    const double r0 = (double)X[0] * 180.0 / M_PI, r1 = (double)X[1] * 180.0 / M_PI;
    const double t0 = (double)(X[2] * 100);
    deltaR = (float)sqrt(r0 * r0 + r1 * r1);
    deltaT = (float)sqrt(t0 * t0);
  } else {
    const double r0 = (double)X[0] * 180.0 / M_PI;
    const double t0 = (double)(X[1] * 100), t1 = (double)(X[2] * 100);
    deltaR = (float)sqrt(r0 * r0);
    deltaT = (float)sqrt(t0 * t0 + t1 * t1);
  }
  return !((double)deltaR < 0.1 && (double)deltaT < 0.1);
}

}  // namespace lego
}  // namespace slio
