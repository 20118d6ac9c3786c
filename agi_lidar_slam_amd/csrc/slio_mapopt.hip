// slio_mapopt.hip -- the mapping back-ends on top of the IKF runtime
// (slio_device.hip, slio_map.hip and slio_scan.hip, reached through
// slio_device.hpp): LIO-SAM's scan-to-map optimisation, its loop-closure ICP pass, its keyframe store and
// the local-map / loop-cloud assembly, and LeGO-LOAM's mapping (slio_lmap_*).
// The two mappers share one scan-to-map path: the map-frame scan and its 5-NN
// (s2m_search), the per-point coefficient (s2m_point_coeff), the LM row
// (s2m_lm_rot, s2m_products), the workgroup reduction (block_sums_256) and the
// normal equations' readback (s2m_sum).  Built like slio_device.hip, with
// -ffp-contract=off: every float expression is evaluated as written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "slio_common.hpp"
#include "slio_cvsolve.hpp"
#include "slio_device.hpp"
#include "slio_frontend.h"
#include "slio_icp.hpp"
#include "slio_livox.hpp"
#include "slio_plane.hpp"

using namespace slio;

// ---------------------------------------------------------------- LIO-SAM scan-to-map
// mapOptmization.cpp cornerOptimization (:1303-1432), surfOptimization
// (:1438-1515) and the rows / normal equations of LMOptimization
// (:1552-1626) on the device; the 6x6 solve stays on the host
// (slio_s2m_lm_step).  One handle per feature class: its map is
// laserCloud{Corner,Surf}FromMapDS, its scan laserCloud{Corner,Surf}LastDS.

// pointAssociateToMap (:359-373) with the float affine of
// pcl::getTransformation(transformTobeMapped)
struct Aff12 {
  float m[12];
};
__global__ void k_s2m_transform(const float* __restrict__ bx, const float* __restrict__ by,
                                const float* __restrict__ bz, int64_t n, Aff12 T, float* __restrict__ wx,
                                float* __restrict__ wy, float* __restrict__ wz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = bx[i], y = by[i], z = bz[i];
  wx[i] = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
  wy[i] = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
  wz[i] = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
}

// OpenCV's hypot (lapack.cpp): scaled, in the element type
__device__ __forceinline__ float cv_hypot(float a, float b) {
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

// cv::eigen of a symmetric 3x3 float matrix: OpenCV hal::Jacobi
// (JacobiImpl_, lapack.cpp) -- eigenvalues W descending, eigenvectors the
// rows of V.  Fully unrolled over compile-time indices (n = 3).
__device__ __forceinline__ void cv_jacobi3(float A[9], float W[3], float V[9]) {
  const float eps = 1.1920928955078125e-07f;
#pragma unroll
  for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0f : 0.0f;
  int indR[3], indC[3];
  W[0] = A[0];
  W[1] = A[4];
  W[2] = A[8];
  // k = 0: row max over cols 1..2; k = 1: col 2 and column max over rows 0
  indR[0] = (fabsf(A[1]) < fabsf(A[2])) ? 2 : 1;
  indR[1] = 2;
  indC[1] = 0;
  indC[2] = (fabsf(A[2]) < fabsf(A[5])) ? 1 : 0;
  for (int iters = 0; iters < 3 * 3 * 30; ++iters) {
    int k = 0;
    float mv = fabsf(A[indR[0]]);
    {
      const float val = fabsf(A[3 + indR[1]]);
      if (mv < val) mv = val, k = 1;
    }
    int l = indR[k];
    for (int i = 1; i < 3; ++i) {
      const float val = fabsf(A[3 * indC[i] + i]);
      if (mv < val) mv = val, k = indC[i], l = i;
    }
    const float p = A[3 * k + l];
    if (fabsf(p) <= eps) break;
    float y = (float)((W[l] - W[k]) * 0.5);
    float t = fabsf(y) + cv_hypot(p, y);
    float sn = cv_hypot(p, t);
    const float c = t / sn;
    sn = p / sn;
    t = (p / t) * p;
    if (y < 0) sn = -sn, t = -t;
    A[3 * k + l] = 0;
    W[k] -= t;
    W[l] += t;
    float a0, b0;
#define SLIO_ROT(v0, v1) a0 = v0, b0 = v1, v0 = a0 * c - b0 * sn, v1 = a0 * sn + b0 * c
    for (int i = 0; i < k; ++i) SLIO_ROT(A[3 * i + k], A[3 * i + l]);
    for (int i = k + 1; i < l; ++i) SLIO_ROT(A[3 * k + i], A[3 * i + l]);
    for (int i = l + 1; i < 3; ++i) SLIO_ROT(A[3 * k + i], A[3 * l + i]);
    for (int i = 0; i < 3; ++i) SLIO_ROT(V[3 * k + i], V[3 * l + i]);
#undef SLIO_ROT
    for (int j = 0; j < 2; ++j) {
      const int idx = j == 0 ? k : l;
      if (idx < 2) {
        int m = idx + 1;
        float mvv = fabsf(A[3 * idx + m]);
        for (int i = idx + 2; i < 3; ++i) {
          const float val = fabsf(A[3 * idx + i]);
          if (mvv < val) mvv = val, m = i;
        }
        indR[idx] = m;
      }
      if (idx > 0) {
        int m = 0;
        float mvv = fabsf(A[idx]);
        for (int i = 1; i < idx; ++i) {
          const float val = fabsf(A[3 * i + idx]);
          if (mvv < val) mvv = val, m = i;
        }
        indC[idx] = m;
      }
    }
  }
  for (int k = 0; k < 2; ++k) {
    int m = k;
    for (int i = k + 1; i < 3; ++i)
      if (W[m] < W[i]) m = i;
    if (k != m) {
      const float tw = W[m];
      W[m] = W[k];
      W[k] = tw;
      for (int i = 0; i < 3; ++i) {
        const float tv = V[3 * m + i];
        V[3 * m + i] = V[3 * k + i];
        V[3 * k + i] = tv;
      }
    }
  }
}

// cornerOptimization's point-to-line coefficient from the five neighbours
// (LIO-SAM :1332-1425; LeGO-LOAM's :1237-1365 is the same arithmetic)
__device__ __forceinline__ uint8_t s2m_corner_coeff(const float (&nb)[5][3], float x0, float y0, float z0,
                                                    float4& cf) {
  uint8_t ok = 0;
  float cx = 0, cy = 0, cz = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    cx += nb[j][0];
    cy += nb[j][1];
    cz += nb[j][2];
  }
  cx /= 5;
  cy /= 5;
  cz /= 5;
  float a11 = 0, a12 = 0, a13 = 0, a22 = 0, a23 = 0, a33 = 0;
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const float ax = nb[j][0] - cx, ay = nb[j][1] - cy, az = nb[j][2] - cz;
    a11 += ax * ax;
    a12 += ax * ay;
    a13 += ax * az;
    a22 += ay * ay;
    a23 += ay * az;
    a33 += az * az;
  }
  a11 /= 5;
  a12 /= 5;
  a13 /= 5;
  a22 /= 5;
  a23 /= 5;
  a33 /= 5;
  float A[9] = {a11, a12, a13, a12, a22, a23, a13, a23, a33}, W[3], V[9];
  cv_jacobi3(A, W, V);
  if (W[0] > 3 * W[1]) {
    const float x1 = cx + 0.1 * V[0], y1 = cy + 0.1 * V[1], z1 = cz + 0.1 * V[2];
    const float x2 = cx - 0.1 * V[0], y2 = cy - 0.1 * V[1], z2 = cz - 0.1 * V[2];
    const float u = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1);
    const float v = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1);
    const float w = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1);
    const float a012 = sqrtf(u * u + v * v + w * w);
    const float l12 = sqrtf((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2));
    const float la = ((y1 - y2) * u + (z1 - z2) * v) / a012 / l12;
    const float lb = -((x1 - x2) * u - (z1 - z2) * w) / a012 / l12;
    const float lc = -((x1 - x2) * v + (y1 - y2) * w) / a012 / l12;
    const float ld2 = a012 / l12;
    const float s = 1 - 0.9 * fabsf(ld2);
    cf = make_float4(s * la, s * lb, s * lc, s * ld2);
    ok = s > 0.1;
  }
  return ok;
}

// surfOptimization after the plane solve (LIO-SAM :1470-1508, LeGO-LOAM
// :1403-1447): sol = the solve's x for b = -1
__device__ __forceinline__ uint8_t s2m_surf_coeff(const float (&sol)[3], const float (&nb)[5][3], float x0, float y0,
                                                  float z0, float4& cf) {
  uint8_t ok = 0;
  float pa = sol[0], pb = sol[1], pc = sol[2], pd = 1;
  const float ps = sqrtf(pa * pa + pb * pb + pc * pc);
  pa /= ps;
  pb /= ps;
  pc /= ps;
  pd /= ps;
  bool valid = true;
#pragma unroll
  for (int j = 0; j < 5; ++j)
    if (fabsf(pa * nb[j][0] + pb * nb[j][1] + pc * nb[j][2] + pd) > 0.2) valid = false;
  if (valid) {
    const float pd2 = pa * x0 + pb * y0 + pc * z0 + pd;
    const float s = 1 - 0.9 * fabsf(pd2) / sqrtf(sqrtf(x0 * x0 + y0 * y0 + z0 * z0));
    cf = make_float4(s * pa, s * pb, s * pc, s * pd2);
    ok = s > 0.1;
  }
  return ok;
}

// the five neighbours of scan point i, if the fifth lies within 1 m
// (LIO-SAM :1330 / :1457, LeGO-LOAM :1236 / :1385)
__device__ __forceinline__ bool s2m_gather5(const uint32_t* __restrict__ nbr_pos, const float* __restrict__ nbr_sqd,
                                            const float4* __restrict__ pts, int64_t i, float (&nb)[5][3]) {
  if (!(nbr_sqd[i * 5 + 4] < 1.0f)) return false;  // (< 1.0 is false for +inf: fewer than 5 map points)
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const float4 p = pts[nbr_pos[i * 5 + j]];
    nb[j][0] = p.x;
    nb[j][1] = p.y;
    nb[j][2] = p.z;
  }
  return true;
}

// Coefficient (coeff.x, y, z, intensity) and selection of scan point i, whose
// map-frame position is (x0, y0, z0), written to coeff[i] / sel[i].
// KIND 0: corner (point-to-line), 1: surf (point-to-plane).  The plane of a
// surf point is LIO-SAM's matA0.colPivHouseholderQr().solve(matB0)
// (qr_solve_m1_dev) or, LEGO, cv::solve(DECOMP_QR) on the 5 x 3 system
// (cvs::qr_solve_mn<5, 3>), a failed solve leaving x = 0 as cv::solve does: ps
// is then 0, everything NaN, and `s > 0.1` is false.
template <int KIND, bool LEGO>
__device__ __forceinline__ uint8_t s2m_point_coeff(int64_t i, float x0, float y0, float z0,
                                                   const uint32_t* __restrict__ nbr_pos,
                                                   const float* __restrict__ nbr_sqd,
                                                   const float4* __restrict__ pts, float4* __restrict__ coeff,
                                                   uint8_t* __restrict__ sel, float4& cf) {
  uint8_t ok = 0;
  cf = make_float4(0, 0, 0, 0);
  float nb[5][3];
  if (s2m_gather5(nbr_pos, nbr_sqd, pts, i, nb)) {
    if (KIND == 0) {
      ok = s2m_corner_coeff(nb, x0, y0, z0, cf);
    } else {
      float sol[3];
      if (LEGO) {
        const float m1[5] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
        if (!slio::cvs::qr_solve_mn<5, 3>(&nb[0][0], m1, sol)) sol[0] = sol[1] = sol[2] = 0.0f;
      } else {
        qr_solve_m1_dev(nb, sol);
      }
      ok = s2m_surf_coeff(sol, nb, x0, y0, z0, cf);
    }
  }
  coeff[i] = cf;
  sel[i] = ok;
  return ok;
}

template <int KIND>
__global__ void k_s2m_coeff(const float* __restrict__ wx, const float* __restrict__ wy,
                            const float* __restrict__ wz, int64_t n, const uint32_t* __restrict__ nbr_pos,
                            const float* __restrict__ nbr_sqd, const float4* __restrict__ pts,
                            float4* __restrict__ coeff, uint8_t* __restrict__ sel) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float4 cf;
  s2m_point_coeff<KIND, false>(i, wx[i], wy[i], wz[i], nbr_pos, nbr_sqd, pts, coeff, sel, cf);
}

// The sums of a 256-thread workgroup, in double and in a fixed tree: a
// butterfly over each wavefront's lanes, then the four wavefronts in order,
// one partial (K sums) per workgroup.  (The 28 sequential block-wide LDS trees
// this replaces -- 252 barriers -- took 27.8 us per launch for 20k points,
// profiles/r05_final_s2m_kernel_stats.csv.)
template <int K>
__device__ __forceinline__ void block_sums_256(double (&v)[K], double* __restrict__ partial) {
  __shared__ double red[4 * K];
  // (a + b == b + a: both lanes of a butterfly pair hold the same sum)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = v[k] + __shfl_xor(v[k], off);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) red[w * K + k] = v[k];
  __syncthreads();
  if (threadIdx.x < K) {
    const int k = threadIdx.x;
    partial[(int64_t)blockIdx.x * K + k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
  }
}

// LMOptimization's rotation part of a row (LIO-SAM :1583-1599, LeGO-LOAM
// :1498-1514): point (px, py, pz) and coefficient (cx, cy, cz) in the camera
// frame, T the sines and cosines of the three angles
struct S2mTrig {
  float srx, crx, sry, cry, srz, crz;
};
struct S2mRot {
  float arx, ary, arz;
};
__device__ __forceinline__ S2mRot s2m_lm_rot(const S2mTrig& T, float px, float py, float pz, float cx, float cy,
                                             float cz) {
  const float srx = T.srx, crx = T.crx, sry = T.sry, cry = T.cry, srz = T.srz, crz = T.crz;
  const float arx = (crx * sry * srz * px + crx * crz * sry * py - srx * sry * pz) * cx +
                    (-srx * srz * px - crz * srx * py - crx * pz) * cy +
                    (crx * cry * srz * px + crx * cry * crz * py - cry * srx * pz) * cz;
  const float ary = ((cry * srx * srz - crz * sry) * px + (sry * srz + cry * crz * srx) * py + crx * cry * pz) * cx +
                    ((-cry * crz - srx * sry * srz) * px + (cry * srz - crz * srx * sry) * py - crx * sry * pz) * cz;
  const float arz = ((crz * srx * sry - cry * srz) * px + (-cry * crz - srx * sry * srz) * py) * cx +
                    (crx * crz * px - crx * srz * py) * cy +
                    ((sry * srz + cry * crz * srx) * px + (crz * sry - cry * srx * srz) * py) * cz;
  return S2mRot{arx, ary, arz};
}

// one row's A^T A (21, upper triangle) / A^T B (6) / count, in double
constexpr int kS2mSums = 28;
__device__ __forceinline__ void s2m_products(const float (&a)[6], float b, double (&v)[kS2mSums]) {
  int q = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c) v[q++] = (double)a[r] * (double)a[c];
#pragma unroll
  for (int r = 0; r < 6; ++r) v[21 + r] = (double)a[r] * (double)b;
  v[27] = 1.0;
}

// LMOptimization rows (:1583-1626, lidar <-> camera axis swap included) of the
// selected points and their normal equations, one partial per workgroup
__global__ __launch_bounds__(256) void k_s2m_rows(const float* __restrict__ bx, const float* __restrict__ by,
                                                  const float* __restrict__ bz, const float4* __restrict__ coeff,
                                                  const uint8_t* __restrict__ sel, int64_t n, S2mTrig T,
                                                  double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v[kS2mSums];
#pragma unroll
  for (int k = 0; k < kS2mSums; ++k) v[k] = 0.0;
  if (i < n && sel[i]) {
    const float4 cs = coeff[i];
    const float cx = cs.y, cy = cs.z, cz = cs.x;  // lidar -> camera
    const S2mRot r = s2m_lm_rot(T, by[i], bz[i], bx[i], cx, cy, cz);
    const float a[6] = {r.arz, r.arx, r.ary, cz, cx, cy};
    s2m_products(a, -cs.w, v);
  }
  block_sums_256(v, partial);
}

// ---- LeGO-LOAM mapping (LeGO-LOAM/src/mapOptmization.cpp) -------------------
// pointAssociateToMap (:578-607) of the scan: see lego_to_map
__global__ void k_lmap_transform(const float* __restrict__ bx, const float* __restrict__ by,
                                 const float* __restrict__ bz, int64_t n, LegoRot T, float* __restrict__ wx,
                                 float* __restrict__ wy, float* __restrict__ wz) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  lego_to_map(T, bx[i], by[i], bz[i], wx[i], wy[i], wz[i]);
}

// cornerOptimization (:1222-1370) / surfOptimization (:1372-1450) after the
// search, and LMOptimization's rows (:1477-1537) of the same points, in ONE
// launch: a row needs only the body point and the coefficient its thread has
// just computed.  The rows use pointOri and coeff as they are (LeGO-LOAM works
// in its camera-like frame throughout: no axis swap) and are summed exactly as
// k_s2m_rows sums them.
template <int KIND>
__global__ __launch_bounds__(256) void k_lmap_coeff(
    const float* __restrict__ bx, const float* __restrict__ by, const float* __restrict__ bz,
    const float* __restrict__ wx, const float* __restrict__ wy, const float* __restrict__ wz, int64_t n,
    const uint32_t* __restrict__ nbr_pos, const float* __restrict__ nbr_sqd, const float4* __restrict__ pts,
    float4* __restrict__ coeff, uint8_t* __restrict__ sel, S2mTrig T, double* __restrict__ partial) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v[kS2mSums];
#pragma unroll
  for (int k = 0; k < kS2mSums; ++k) v[k] = 0.0;
  float4 cf;
  if (i < n && s2m_point_coeff<KIND, true>(i, wx[i], wy[i], wz[i], nbr_pos, nbr_sqd, pts, coeff, sel, cf)) {
    const S2mRot r = s2m_lm_rot(T, bx[i], by[i], bz[i], cf.x, cf.y, cf.z);
    const float a[6] = {r.arx, r.ary, r.arz, cf.x, cf.y, cf.z};
    s2m_products(a, -cf.w, v);
  }
  block_sums_256(v, partial);
}

// float4 xyzi (the front-end's clouds) -> SoA, for the VoxelGrid
// ---- livox_mapping laserMapping (livox_mapping/src/laserMapping.cpp) --------
// A sorted list of the K smallest 64-bit keys (bits(d^2) << 32) | position:
// totally ordered, so the result does not depend on the order of insertion
// (ties at equal float distance go to the lower position in the cell-sorted
// map).  A sibling of Top5 for K = 5 and 8; insertion is a compare-exchange
// chain without data-dependent branches.
template <int K>
struct TopK {
  uint64_t k[K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < K; ++j) k[j] = ~0ull;
  }
  __device__ __forceinline__ void insert(uint64_t key) {
    k[K - 1] = key < k[K - 1] ? key : k[K - 1];
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      const uint64_t lo = k[j] < k[j - 1] ? k[j] : k[j - 1], hi = k[j] < k[j - 1] ? k[j - 1] : k[j];
      k[j - 1] = lo;
      k[j] = hi;
    }
  }
};

// surfOptimization after the plane solve on EIGHT neighbours (:977-1026):
// s2m_surf_coeff's arithmetic (the `break` of :1000 changes no result)
__device__ __forceinline__ uint8_t lvx_surf_coeff(const float (&sol)[3], const float (&nb)[8][3], float x0, float y0,
                                                  float z0, float4& cf) {
  uint8_t ok = 0;
  float pa = sol[0], pb = sol[1], pc = sol[2], pd = 1;
  const float ps = sqrtf(pa * pa + pb * pb + pc * pc);
  pa /= ps;
  pb /= ps;
  pc /= ps;
  pd /= ps;
  bool valid = true;
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (fabsf(pa * nb[j][0] + pb * nb[j][1] + pc * nb[j][2] + pd) > 0.2) valid = false;
  if (valid) {
    const float pd2 = pa * x0 + pb * y0 + pc * z0 + pd;
    const float s = 1 - 0.9 * fabsf(pd2) / sqrtf(sqrtf(x0 * x0 + y0 * y0 + z0 * z0));
    cf = make_float4(s * pa, s * pb, s * pc, s * pd2);
    ok = s > 0.1;
  }
  return ok;
}

// One pass of the optimisation loop for one class (:825-950 corner, :954-1028
// surf) and its rows (:1059-1095, which read beside s2m_lm_rot are the same
// expressions in the same order), one thread per scan point:
// pointAssociateToMap, the exact K-NN, the gate, the coefficient, the row, and
// the 28 fp64 sums of the workgroup as k_lmap_coeff leaves them.
//
// Exactness of the K-NN without refinement.  The query lies in the centre cell
// of its 3 x 3 x 3 block of cells of edge h, so every map point outside the
// block is at least `bound` away, bound = the query's distance to the nearest
// face of the block less kCellTol (the float rounding of the cell function is
// ~3e-5 m at 300 m), and bound >= h - kCellTol > sqrt(gate) (h = 1.25 against
// sqrt(1.5) = 1.2247, 2.25 against sqrt(5) = 2.2361).  If the K-th distance
// inside the block is <= bound, the block's K nearest are the map's.  If not,
// the map's K-th distance is > sqrt(gate) whichever points it is made of, and
// the reference drops the query at :833 / :961.  A query whose cell is not in
// 1 .. n - 2 of an axis is a full cell away from every map point (the grid
// has two cells of padding): dropped the same way, nothing is read.  Nobody
// waits on anybody.  A query that is not proven, or that the gate rejects,
// leaves index -1 and distance +inf.
template <int KIND>
__global__ __launch_bounds__(256) void k_lvx_pass(const slio::lvx::GridView g, const float* __restrict__ body,
                                                  int64_t n, LegoRot T, S2mTrig trig, slio::lvx::PassOut o) {
  constexpr int K = KIND == 0 ? 5 : 8;
  constexpr float kGate = KIND == 0 ? 1.5f : 5.0f;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double v[kS2mSums];
#pragma unroll
  for (int k = 0; k < kS2mSums; ++k) v[k] = 0.0;
  if (i < n) {
    const float bx = body[3 * i], by = body[3 * i + 1], bz = body[3 * i + 2];
    float w[3];
    lego_to_map(T, bx, by, bz, w[0], w[1], w[2]);
    o.world[3 * i] = w[0];
    o.world[3 * i + 1] = w[1];
    o.world[3 * i + 2] = w[2];
    TopK<K> top;
    top.init();
    bool near = false;
    if (g.n > 0) {
      const int dim[3] = {g.nx, g.ny, g.nz};
      int c[3];
      bool inside = true;
      float bound = g.h;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        const float fc = floorf((w[a] - g.o[a]) * g.inv_h);
        inside = inside && fc >= 1.0f && fc <= (float)(dim[a] - 2);  // (false for NaN)
        c[a] = (int)fminf(fmaxf(fc, 1.0f), (float)(dim[a] - 2));
        bound = fminf(bound, w[a] - (g.o[a] + (float)(c[a] - 1) * g.h));
        bound = fminf(bound, (g.o[a] + (float)(c[a] + 2) * g.h) - w[a]);
      }
      bound -= slio::lvx::kCellTol;
      if (inside) {
        for (int dz = -1; dz <= 1; ++dz)
          for (int dy = -1; dy <= 1; ++dy) {
            const int64_t base = ((int64_t)(c[2] + dz) * g.ny + (c[1] + dy)) * g.nx + (c[0] - 1);
            const uint32_t p0 = g.start[base], p1 = g.start[base + 3];
            for (uint32_t p = p0; p < p1; ++p) {
              const float4 q = g.pts[p];
              const float dx = q.x - w[0], dy2 = q.y - w[1], dz2 = q.z - w[2];
              const float d2 = (dx * dx + dy2 * dy2) + dz2 * dz2;
              top.insert(((uint64_t)__float_as_uint(d2) << 32) | p);
            }
          }
        const uint64_t kth = top.k[K - 1];
        const float d2k = __uint_as_float((uint32_t)(kth >> 32));
        near = kth != ~0ull && bound > 0.0f && d2k <= bound * bound && d2k < kGate;
      }
    }
    uint8_t ok = 0;
    float4 cf = make_float4(0, 0, 0, 0);
    if (near) {
      float nb[K][3];
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const float4 q = g.pts[(uint32_t)top.k[j]];
        nb[j][0] = q.x;
        nb[j][1] = q.y;
        nb[j][2] = q.z;
        o.nbr_idx[i * K + j] = (int32_t)__float_as_uint(q.w);
        o.nbr_sqd[i * K + j] = __uint_as_float((uint32_t)(top.k[j] >> 32));
      }
      if constexpr (KIND == 0) {
        ok = s2m_corner_coeff(nb, w[0], w[1], w[2], cf);
      } else {
        // matA0 is 10 x 3 with two zero rows against -1 (:423-425); the 8 x 3
        // system gives the same bits (slio_lvx_plane_solve).  A failed solve
        // leaves x = 0: ps = 0, NaNs, `s > 0.1` false.
        const float m1[8] = {-1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f, -1.0f};
        float sol[3];
        if (!slio::cvs::qr_solve_mn<8, 3>(&nb[0][0], m1, sol)) sol[0] = sol[1] = sol[2] = 0.0f;
        ok = lvx_surf_coeff(sol, nb, w[0], w[1], w[2], cf);
      }
    } else {
#pragma unroll
      for (int j = 0; j < K; ++j) {
        o.nbr_idx[i * K + j] = -1;
        o.nbr_sqd[i * K + j] = INFINITY;
      }
    }
    o.coeff[i] = cf;
    o.sel[i] = ok;
    if (ok) {
      const S2mRot r = s2m_lm_rot(trig, bx, by, bz, cf.x, cf.y, cf.z);
      const float a[6] = {r.arx, r.ary, r.arz, cf.x, cf.y, cf.z};
      s2m_products(a, -cf.w, v);
    }
  }
  block_sums_256(v, o.partial);
}

__global__ void k_lmap_split4(const float4* __restrict__ in, int64_t n, float* __restrict__ x,
                              float* __restrict__ y, float* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  x[i] = p.x;
  y[i] = p.y;
  z[i] = p.z;
}

// the six cached float sines and cosines (:562-576 / :609-622) of
// {rx, ry, rz, tx, ty, tz}: roll = rx, pitch = ry, yaw = rz
static LegoRot lmap_rot(const float tf[6]) {
  return LegoRot{fcos(tf[0]), fsin(tf[0]), fcos(tf[1]), fsin(tf[1]), fcos(tf[2]), fsin(tf[2]), tf[3], tf[4], tf[5]};
}

// pcl::getTransformation (pcl/common/impl/eigen.hpp) in float, the trig
// correctly rounded (evaluated in double)
static Aff12 s2m_affine(const float tf[6]) {
  const float x = tf[3], y = tf[4], z = tf[5], roll = tf[0], pitch = tf[1], yaw = tf[2];
  const float A = fcos(yaw), B = fsin(yaw), C = fcos(pitch), D = fsin(pitch), E = fcos(roll), F = fsin(roll),
              DE = D * E, DF = D * F;
  Aff12 t;
  t.m[0] = A * C, t.m[1] = A * DF - B * E, t.m[2] = B * F + A * DE, t.m[3] = x;
  t.m[4] = B * C, t.m[5] = A * E + B * DF, t.m[6] = B * DE - A * F, t.m[7] = y;
  t.m[8] = -D, t.m[9] = C * F, t.m[10] = C * E, t.m[11] = z;
  return t;
}

// LMOptimization's trig of the three angles (float sin / cos)
static S2mTrig s2m_trig(float rx, float ry, float rz) {
  return S2mTrig{fsin(rx), fcos(rx), fsin(ry), fcos(ry), fsin(rz), fcos(rz)};
}

int slio::lvx::pass_launch(int kind, const GridView& g, const float* body_xyz, int64_t n, const float tf[6],
                           const PassOut& out, hipStream_t st) {
  if (n == 0) return SLIO_OK;
  const LegoRot T = lmap_rot(tf);
  const S2mTrig trig = s2m_trig(tf[0], tf[1], tf[2]);
  const int nb = (int)((n + 255) / 256);
  if (kind == 0)
    k_lvx_pass<0><<<nb, 256, 0, st>>>(g, body_xyz, n, T, trig, out);
  else
    k_lvx_pass<1><<<nb, 256, 0, st>>>(g, body_xyz, n, T, trig, out);
  SLIO_HIP(hipGetLastError());
  return SLIO_OK;
}

// The scan of c in the map frame and its 5-NN: to_map() launches the kernel
// that writes c.wbx / wby / wbz (allocated here), the search pass runs on them
// in kNN-only mode with the identity pose (body -> world of an identity pose
// is exact in float), and coeff() launches the kernel that reads the
// neighbours, under the map's read lock.  Nothing runs for an empty scan.
template <class ToMap, class Coeff>
static int s2m_search(Ctx& c, const char* who, ToMap to_map, Coeff coeff) {
  if (!c.wbx) {
    const int64_t cap = c.prm.max_points;
    hipError_t e;
    if ((e = hipMalloc(&c.wbx, 4 * cap)) || (e = hipMalloc(&c.wby, 4 * cap)) || (e = hipMalloc(&c.wbz, 4 * cap))) {
      set_error(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
  }
  if (c.n == 0) return SLIO_OK;
  to_map();
  slio_pose idp{};
  idp.rot[0] = 1.0;
  idp.rli[0] = 1.0;
  const PoseDev P = make_pose(&idp);
  const ScanDev sd{c.wbx, c.wby, c.wbz, c.n};
  if (int rc = enqueue_pass(c, &P, nullptr, 1, 0, nullptr, false, true, &sd)) return rc;
  std::shared_lock<std::shared_mutex> lk(c.map->mu);
  if (int rc = map_read_sync(c)) return rc;
  coeff();
  SLIO_HIP(hipGetLastError());
  return SLIO_OK;
}

// the number of selected points of c's scan (waits for the stream)
static int s2m_count_sel(Ctx& c, int64_t* nsel) {
  std::vector<uint8_t> sl((size_t)c.n);
  if (c.n) {
    SLIO_HIP(hipStreamSynchronize(c.stream));
    SLIO_HIP(hipMemcpy(sl.data(), c.sel, c.n, hipMemcpyDeviceToHost));
  }
  int64_t k = 0;
  for (uint8_t v : sl) k += v;
  *nsel = k;
  return SLIO_OK;
}

// The normal equations of the rows in cs[0..ncs)'s chunk_part (k_s2m_rows,
// k_lmap_coeff): the workgroups' partials summed in order, handle after handle
// (null handles and empty scans skipped)
static int s2m_sum(Ctx* const* cs, int ncs, float AtA[36], float AtB[6], int64_t* nsel) {
  double acc[kS2mSums] = {0};
  for (int h = 0; h < ncs; ++h) {
    if (!cs[h] || cs[h]->n == 0) continue;
    Ctx& c = *cs[h];
    const int nb = (int)((c.n + 255) / 256);
    std::vector<double> part((size_t)nb * kS2mSums);
    const Rb rb{part.data(), c.chunk_part, 8 * part.size()};
    SLIO_HIP(readback(c.stream, &rb, 1));
    for (int b = 0; b < nb; ++b)
      for (int k = 0; k < kS2mSums; ++k) acc[k] = acc[k] + part[(size_t)b * kS2mSums + k];
  }
  int q = 0;
  for (int r = 0; r < 6; ++r)
    for (int cc = r; cc < 6; ++cc, ++q) AtA[6 * r + cc] = AtA[6 * cc + r] = (float)acc[q];
  for (int r = 0; r < 6; ++r) AtB[r] = (float)acc[21 + r];
  if (nsel) *nsel = (int64_t)llround(acc[27]);
  return SLIO_OK;
}

extern "C" {

int slio_s2m_coeffs(slio_handle h, int kind, const float transform[6], int64_t* nsel) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if ((kind != 0 && kind != 1) || !transform) {
    set_error("slio_s2m_coeffs: bad arguments");
    return SLIO_EINVAL;
  }
  if (!c.map || !c.bx) {
    set_error("slio_s2m_coeffs: map and scan needed");
    return SLIO_ESTATE;
  }
  if (c.prm.nranks != 1) {
    set_error("slio_s2m_coeffs: single-rank handles only");
    return SLIO_EINVAL;
  }
  const int64_t n = c.n;
  const int rc = s2m_search(
      c, "slio_s2m_coeffs",
      [&] {
        k_s2m_transform<<<grid_blocks(n), 256, 0, c.stream>>>(c.bx, c.by, c.bz, n, s2m_affine(transform), c.wbx,
                                                               c.wby, c.wbz);
      },
      [&] {
        auto* k = kind == 0 ? k_s2m_coeff<0> : k_s2m_coeff<1>;
        k<<<grid_blocks(n), 256, 0, c.stream>>>(c.wbx, c.wby, c.wbz, n, c.nbr_pos, c.nbr_sqd, c.map->pts, c.plane,
                                                c.sel);
      });
  if (rc) return rc;
  c.s2m_kind = kind;
  return nsel ? s2m_count_sel(c, nsel) : SLIO_OK;
}

int slio_s2m_get_coeffs(slio_handle h, float* coeff, uint8_t* sel) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (c.n > 0) {
    SLIO_HIP(hipStreamSynchronize(c.stream));
    if (coeff) SLIO_HIP(hipMemcpy(coeff, c.plane, 16 * c.n, hipMemcpyDeviceToHost));
    if (sel) SLIO_HIP(hipMemcpy(sel, c.sel, c.n, hipMemcpyDeviceToHost));
  }
  return SLIO_OK;
}

int slio_s2m_normal_equations(slio_handle h_corner, slio_handle h_surf, const float transform[6], float AtA[36],
                              float AtB[6], int64_t* nsel) {
  if (!transform || !AtA || !AtB) {
    set_error("slio_s2m_normal_equations: bad arguments");
    return SLIO_EINVAL;
  }
  // the camera-frame trig of LMOptimization (:1564-1569), float sin / cos
  const S2mTrig T = s2m_trig(transform[1], transform[2], transform[0]);
  // corners first, then surfs (combineOptimizationCoeffs :1517-1543); both
  // clouds' rows launched before either is read back (their own streams)
  Ctx* const cs[2] = {h_corner ? &h_corner->c : nullptr, h_surf ? &h_surf->c : nullptr};
  for (Ctx* c : cs) {
    if (!c || c->n == 0) continue;
    const int nb = (int)((c->n + 255) / 256);
    k_s2m_rows<<<nb, 256, 0, c->stream>>>(c->bx, c->by, c->bz, c->plane, c->sel, c->n, T, c->chunk_part);
    SLIO_HIP(hipGetLastError());
  }
  return s2m_sum(cs, 2, AtA, AtB, nsel);
}

}  // extern "C"

// ---------------------------------------------------------------- LIO-SAM loop closure: one ICP pass
// performLoopClosure's pcl::IterativeClosestPoint (mapOptmization.cpp:766-780)
// as PCL 1.10 runs it (the reference tree carries no PCL source; slio.h
// restates the rules): per iteration transformCloud of the working cloud,
// CorrespondenceEstimation::determineCorrespondences (1-NN, distance gate)
// and the sums TransformationEstimationSVD needs -- ONE launch.  The handle's
// map is the target, its scan the source.  One query per lane on the 3x3x3
// fine cells around it; a query whose nearest is not certified there
// (outside_bound, as the search pass's block step) is deferred to the
// workgroup's far queue and answered by a whole wavefront on the coarse level
// (far_search<U, 1>).  A loop candidate starts metres from where it belongs:
// in the first passes most queries take the far path.  Keys are those of the
// search pass (float squared distance, then position in the cell-sorted
// points), so the nearest point equals entry 0 of slio_get_neighbors for the
// same world point, ties included.
// The 16 sums (+ the count, + the far queries) are reduced as k_s2m_rows
// reduces its rows (block_sums_256), one partial per workgroup.
constexpr int kIcpSums = 18;  // p (3), q (3), q p^T (9), sqd, correspondences, far queries
// (sx / sy / sz may be wx / wy / wz: no __restrict__ on the six)
__device__ __forceinline__ void icp_pass_body(const MapView& map, const float* sx, const float* sy, const float* sz,
                                              int64_t n, const Aff12& T, double max_sq, float* wx, float* wy,
                                              float* wz, int32_t* __restrict__ idx, float* __restrict__ sqd,
                                              double* __restrict__ partial) {
  __shared__ int far_cnt;
  __shared__ float4 far_q[256];
  __shared__ uint8_t far_slot[256];
  __shared__ uint64_t far_key[256];
  __shared__ uint32_t far_pre[4][64], far_beg[4][64];
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + tid;
  const GridGeom g = map.g;
  const float INF = __int_as_float(0x7f800000);
  if (tid == 0) far_cnt = 0;
  __syncthreads();
  const bool live = i < n;
  float qx = 0.0f, qy = 0.0f, qz = 0.0f;
  if (live) {
    // (in place when sx is wx: each lane reads its own point before it writes it)
    const float x = sx[i], y = sy[i], z = sz[i];
    qx = ((T.m[0] * x + T.m[1] * y) + T.m[2] * z) + T.m[3];
    qy = ((T.m[4] * x + T.m[5] * y) + T.m[6] * z) + T.m[7];
    qz = ((T.m[8] * x + T.m[9] * y) + T.m[10] * z) + T.m[11];
    wx[i] = qx;
    wy[i] = qy;
    wz[i] = qz;
  }
  const bool finite = live && isfinite(qx) && isfinite(qy) && isfinite(qz) && map.n > 0;
  uint64_t best = kInfKey;
  bool done = !finite;
  if (finite) {
    const int cx = cell_coord(qx, g.ox, g.inv_h), cy = cell_coord(qy, g.oy, g.inv_h),
              cz = cell_coord(qz, g.oz, g.inv_h);
    const int x0 = max(cx - 1, 0), x1 = min(cx + 1, g.dx - 1);
    if (x0 <= x1)
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
          const int y = cy + dy, z = cz + dz;
          if (y < 0 || y >= g.dy || z < 0 || z >= g.dz) continue;
          const int64_t rb = ((int64_t)z * g.dy + y) * g.dx;
          const uint32_t s = map.start[rb + x0], e = map.start[rb + x1 + 1];
          for (uint32_t a = s; a < e; ++a) {
            const float4 c = map.pts[a];
            const float ddx = qx - c.x, ddy = qy - c.y, ddz = qz - c.z;
            const float d = (ddx * ddx + ddy * ddy) + ddz * ddz;  // as consider()
            const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)a;
            best = key < best ? key : best;
          }
        }
    bool covers;
    const float b1 = outside_bound(g, cx, cy, cz, 1, qx, qy, qz, covers);
    const float d1 = __uint_as_float((uint32_t)(best >> 32));
    done = covers || (best != kInfKey && b1 > 0.0f && d1 < (b1 * b1) * 0.99999f);
    if (!done) {
      const int k = atomicAdd(&far_cnt, 1);
      far_slot[k] = (uint8_t)tid;
      far_q[k] = make_float4(qx, qy, qz, best != kInfKey ? d1 : INF);  // a real point's distance bounds the search
    }
  }
  __syncthreads();
  const int nfar = far_cnt;
  for (int k = tid >> 6; k < nfar; k += 4) {  // (uniform per wavefront)
    const float4 q = far_q[k];
    Top5 tf;
    far_search<4, 1>(map, q.x, q.y, q.z, q.w, far_pre[tid >> 6], far_beg[tid >> 6], tf);
    if ((tid & 63) == 0) far_key[far_slot[k]] = tf.k[0];
  }
  __syncthreads();
  const bool was_far = finite && !done;
  if (was_far) best = far_key[tid];
  double v[kIcpSums];
#pragma unroll
  for (int k = 0; k < kIcpSums; ++k) v[k] = 0.0;
  if (live) {
    int32_t id = -1;
    float d = INF;
    if (best != kInfKey) {
      const float4 c = map.pts[(uint32_t)best];
      d = __uint_as_float((uint32_t)(best >> 32));
      // CorrespondenceEstimation: `if (distance > max_dist_sqr) continue;`
      if ((double)d <= max_sq) {
        id = (int32_t)__float_as_uint(c.w);
        const float p[3] = {qx, qy, qz}, m[3] = {c.x, c.y, c.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
          v[a] = (double)p[a];
          v[3 + a] = (double)m[a];
#pragma unroll
          for (int b = 0; b < 3; ++b) v[6 + 3 * a + b] = (double)m[a] * (double)p[b];
        }
        v[15] = (double)d;
        v[16] = 1.0;
      }
    }
    idx[i] = id;
    sqd[i] = d;
  }
  v[17] = was_far ? 1.0 : 0.0;
  block_sums_256(v, partial);
}

// the lockstep path's pass (slio_icp_correspond): the transform is a kernel argument
__global__ __launch_bounds__(256) void k_icp_pass(const MapView map, const float* sx, const float* sy,
                                                  const float* sz, int64_t n, Aff12 T, double max_sq, float* wx,
                                                  float* wy, float* wz, int32_t* __restrict__ idx,
                                                  float* __restrict__ sqd, double* __restrict__ partial) {
  icp_pass_body(map, sx, sy, sz, n, T, max_sq, wx, wy, wz, idx, sqd, partial);
}

// ---------------------------------------------------------------- the device-resident ICP loop
// slio_icp_align: icp.align and getFitnessScore without a host wait per
// iteration.  The loop's state lives in one small struct in HBM; an iteration
// is two launches on the handle's stream, the wide pass (k_icp_pass_dev: the
// lockstep pass's body, its transform read from the struct) and a
// one-workgroup tail (k_icp_tail: the workgroups' partials added in ascending
// workgroup order, one lane per entry, then slio::icp::step on one thread).
// Stream order is the only synchronisation: no kernel waits for another
// workgroup, and a launch that finds `done` set returns at once, so the host
// may enqueue a batch of iterations past the end of the loop.
struct IcpDev {
  slio_icp_state st;
  slio_icp_params prm;
  float delta[16];       // the next pass's transform (the guess before the first pass)
  int32_t done;
  int32_t fit_done;      // the fitness pass's tail has run
  int64_t ncorr;         // correspondences of the last loop pass
  int64_t far_first;     // far queries of the first pass
  double fit[kIcpSums];  // the fitness pass: sums, correspondences, far queries
};

// fit == 0: a loop pass, T = delta, nothing happens once `done` is set;
// fit == 1: the fitness pass, T = final_T
__global__ __launch_bounds__(256) void k_icp_pass_dev(const IcpDev* __restrict__ dev, int fit, const MapView map,
                                                      const float* sx, const float* sy, const float* sz, int64_t n,
                                                      double max_sq, float* wx, float* wy, float* wz,
                                                      int32_t* __restrict__ idx, float* __restrict__ sqd,
                                                      double* __restrict__ partial) {
  if (!fit && dev->done) return;  // (uniform over the launch, before any barrier)
  Aff12 T;
  const float* m = fit ? dev->st.final_T : dev->delta;
#pragma unroll
  for (int k = 0; k < 12; ++k) T.m[k] = m[k];
  icp_pass_body(map, sx, sy, sz, n, T, max_sq, wx, wy, wz, idx, sqd, partial);
}

// <<<1, 64>>>.  The sums as slio_icp_correspond forms them on the host:
// acc[k] = 0, then acc[k] = acc[k] + partial[b][k] for b = 0 .. nb - 1.
__global__ __launch_bounds__(64) void k_icp_tail(IcpDev* __restrict__ dev, int fit, int first,
                                                 const double* __restrict__ partial, int nb) {
  if (!fit && dev->done) return;  // (uniform, before the barrier)
  __shared__ double acc_s[kIcpSums];
  const int k = threadIdx.x;
  if (k < kIcpSums) {
    double acc = 0.0;
    for (int b = 0; b < nb; ++b) acc = acc + partial[(int64_t)b * kIcpSums + k];
    acc_s[k] = acc;
    if (fit) dev->fit[k] = acc;
  }
  __syncthreads();
  if (k != 0) return;
  if (fit) {
    dev->fit_done = 1;
    return;
  }
  double sums[16];
  for (int a = 0; a < 16; ++a) sums[a] = acc_s[a];
  const int64_t ncorr = (int64_t)llround(acc_s[16]);
  dev->ncorr = ncorr;
  if (first) dev->far_first = (int64_t)llround(acc_s[17]);
  slio_icp_state st = dev->st;
  const slio_icp_params prm = dev->prm;
  float delta[16];
  int done = 0;
  slio::icp::step(sums, ncorr, &prm, &st, delta, &done);
  dev->st = st;
  for (int a = 0; a < 16; ++a) dev->delta[a] = delta[a];
  dev->done = done;
}

constexpr int kIcpBatchDefault = 8;  // iterations enqueued between two reads of the state

extern "C" {

int slio_icp_align(slio_handle h, const slio_icp_params* prm, const float guess[16], double max_dist, int32_t batch,
                   slio_icp_state* out, double* fitness, int64_t* far_first) {
  if (!h) {
    set_error("null handle");
    return SLIO_EINVAL;
  }
  if (!prm || !out || !(max_dist >= 0.0) || h->c.prm.nranks != 1) {
    set_error("slio_icp_align: bad arguments");
    return SLIO_EINVAL;
  }
  Ctx& c = h->c;
  if (!c.map || (!c.bx && c.n > 0)) {
    set_error("slio_icp_align: map and scan needed");
    return SLIO_ESTATE;
  }
  if (batch <= 0) batch = kIcpBatchDefault;
  IcpDev hd;
  std::memset(&hd, 0, sizeof(hd));
  slio_icp_state_init(&hd.st, guess);
  hd.prm = *prm;
  std::memcpy(hd.delta, hd.st.final_T, sizeof(hd.delta));
  const int64_t n = c.n;
  c.icp_far = 0;
  c.icp_n = n;
  if (fitness) *fitness = DBL_MAX;  // getFitnessScore without a correspondence
  if (far_first) *far_first = 0;
  if (n == 0) {
    // the lockstep loop's first step on zero sums: NO_CORRESPONDENCES
    hd.st.convergence_state = SLIO_ICP_NO_CORRESPONDENCES;
    *out = hd.st;
    return SLIO_OK;
  }
  SLIO_HIP(hipSetDevice(c.prm.device));
  const int nb = (int)((n + 255) / 256);
  hipError_t e;
  if ((e = MapDev::take(c.icp[0], 12 * n)) || (e = MapDev::take(c.icp[1], 4 * n)) ||
      (e = MapDev::take(c.icp[2], 4 * n)) || (e = MapDev::take(c.icp[3], 8 * (size_t)kIcpSums * nb)) ||
      (e = MapDev::take(c.icp[4], sizeof(IcpDev)))) {
    c.icp_n = -1;
    set_error(std::string("slio_icp_align: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  float* wx = (float*)c.icp[0].p;
  float* wy = wx + n;
  float* wz = wx + 2 * n;
  int32_t* idx = (int32_t*)c.icp[1].p;
  float* sqd = (float*)c.icp[2].p;
  double* part = (double*)c.icp[3].p;
  IcpDev* dev = (IcpDev*)c.icp[4].p;
  if (int rc = map_refresh(c); rc) return rc;
  std::shared_lock<std::shared_mutex> lk(c.map->mu);
  if (int rc = map_read_sync(c)) return rc;
  const CoarseView cv{c.map->cg, c.map->clo, c.map->chi};
  const MapView mv{c.map->g,      c.map->n,    c.map->pts,    c.map->start, c.map->blk,
                   c.map->bstart, c.map->nblk, c.map->ncells, cv};
  // (pageable source: the copy has left `hd` when the call returns)
  SLIO_HIP(hipMemcpyAsync(dev, &hd, sizeof(hd), hipMemcpyHostToDevice, c.stream));
  const double max_sq = max_dist * max_dist;
  // every turn of the loop ends it or counts one iteration, so max_iterations
  // turns (one, where that is not positive) always set `done`
  const int64_t most = std::max<int64_t>(prm->max_iterations, 1);
  const Rb rb{&hd, dev, sizeof(hd)};
  int64_t turns = 0;
  while (!hd.done) {
    if (turns >= most) {
      c.icp_n = -1;
      set_error("slio_icp_align: the device loop did not end");
      return SLIO_EDEVICE;
    }
    for (int32_t b = 0; b < batch && turns < most; ++b, ++turns) {
      const bool first = turns == 0;
      k_icp_pass_dev<<<nb, 256, 0, c.stream>>>(dev, 0, mv, first ? c.bx : wx, first ? c.by : wy, first ? c.bz : wz,
                                               n, max_sq, wx, wy, wz, idx, sqd, part);
      k_icp_tail<<<1, 64, 0, c.stream>>>(dev, 0, first ? 1 : 0, part, nb);
    }
    SLIO_HIP(hipGetLastError());
    SLIO_HIP(readback(c.stream, &rb, 1));
  }
  // getFitnessScore: the source at final_T, no gate
  k_icp_pass_dev<<<nb, 256, 0, c.stream>>>(dev, 1, mv, c.bx, c.by, c.bz, n, (double)INFINITY, wx, wy, wz, idx, sqd,
                                           part);
  k_icp_tail<<<1, 64, 0, c.stream>>>(dev, 1, 0, part, nb);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(readback(c.stream, &rb, 1));
  *out = hd.st;
  const int64_t nfit = (int64_t)llround(hd.fit[16]);
  c.icp_far = (int64_t)llround(hd.fit[17]);
  if (fitness && nfit > 0) *fitness = hd.fit[15] / (double)nfit;
  if (far_first) *far_first = hd.far_first;
  return SLIO_OK;
}

int slio_icp_correspond(slio_handle h, const float T[16], int from_scan, double max_dist, double sums[16],
                        int64_t* ncorr) {
  if (!h) {
    set_error("null handle");
    return SLIO_EINVAL;
  }
  if (!T || !sums || !ncorr || (from_scan != 0 && from_scan != 1) || !(max_dist >= 0.0) ||
      h->c.prm.nranks != 1) {
    set_error("slio_icp_correspond: bad arguments");
    return SLIO_EINVAL;
  }
  Ctx& c = h->c;
  if (!c.map || (from_scan && !c.bx && c.n > 0) || (!from_scan && c.icp_n < 0)) {
    set_error(from_scan || !c.map ? "slio_icp_correspond: map and scan needed"
                                  : "slio_icp_correspond: no working cloud (from_scan = 1 first)");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(c.prm.device));
  const int64_t n = from_scan ? c.n : c.icp_n;
  for (int k = 0; k < 16; ++k) sums[k] = 0.0;
  *ncorr = 0;
  c.icp_far = 0;
  c.icp_n = n;
  if (n == 0) return SLIO_OK;
  const int nb = (int)((n + 255) / 256);
  hipError_t e;
  if ((e = MapDev::take(c.icp[0], 12 * n)) || (e = MapDev::take(c.icp[1], 4 * n)) ||
      (e = MapDev::take(c.icp[2], 4 * n)) || (e = MapDev::take(c.icp[3], 8 * (size_t)kIcpSums * nb))) {
    c.icp_n = -1;
    set_error(std::string("slio_icp_correspond: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  float* wx = (float*)c.icp[0].p;
  float* wy = wx + n;
  float* wz = wx + 2 * n;
  double* part = (double*)c.icp[3].p;
  Aff12 A;
  std::memcpy(A.m, T, sizeof(A.m));
  if (int rc = map_refresh(c); rc) return rc;
  {
    std::shared_lock<std::shared_mutex> lk(c.map->mu);
    if (int rc = map_read_sync(c)) return rc;
    const CoarseView cv{c.map->cg, c.map->clo, c.map->chi};
    const MapView mv{c.map->g,      c.map->n,    c.map->pts,    c.map->start, c.map->blk,
                     c.map->bstart, c.map->nblk, c.map->ncells, cv};
    k_icp_pass<<<nb, 256, 0, c.stream>>>(mv, from_scan ? c.bx : wx, from_scan ? c.by : wy, from_scan ? c.bz : wz, n,
                                         A, max_dist * max_dist, wx, wy, wz, (int32_t*)c.icp[1].p,
                                         (float*)c.icp[2].p, part);
    SLIO_HIP(hipGetLastError());
  }
  std::vector<double> hp((size_t)nb * kIcpSums);
  const Rb rb{hp.data(), part, 8 * hp.size()};
  SLIO_HIP(readback(c.stream, &rb, 1));
  double acc[kIcpSums] = {0};
  for (int b = 0; b < nb; ++b)
    for (int k = 0; k < kIcpSums; ++k) acc[k] = acc[k] + hp[(size_t)b * kIcpSums + k];
  for (int k = 0; k < 16; ++k) sums[k] = acc[k];
  *ncorr = (int64_t)llround(acc[16]);
  c.icp_far = (int64_t)llround(acc[17]);
  return SLIO_OK;
}

int slio_icp_get_correspondences(slio_handle h, int32_t* idx, float* sqd) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (c.icp_n < 0) {
    set_error("slio_icp_get_correspondences: no pass yet");
    return SLIO_ESTATE;
  }
  if (c.icp_n > 0) {
    SLIO_HIP(hipStreamSynchronize(c.stream));
    if (idx) SLIO_HIP(hipMemcpy(idx, c.icp[1].p, 4 * c.icp_n, hipMemcpyDeviceToHost));
    if (sqd) SLIO_HIP(hipMemcpy(sqd, c.icp[2].p, 4 * c.icp_n, hipMemcpyDeviceToHost));
  }
  return SLIO_OK;
}

int slio_icp_get_working(slio_handle h, float* x, float* y, float* z, int64_t cap, int64_t* n) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (c.icp_n < 0) {
    set_error("slio_icp_get_working: no pass yet");
    return SLIO_ESTATE;
  }
  if (n) *n = c.icp_n;
  if (cap < c.icp_n || (c.icp_n > 0 && (!x || !y || !z))) {
    set_error("slio_icp_get_working: buffer too small");
    return SLIO_ECAPACITY;
  }
  if (c.icp_n > 0) {
    const float* w = (const float*)c.icp[0].p;
    SLIO_HIP(hipStreamSynchronize(c.stream));
    SLIO_HIP(hipMemcpy(x, w, 4 * c.icp_n, hipMemcpyDeviceToHost));
    SLIO_HIP(hipMemcpy(y, w + c.icp_n, 4 * c.icp_n, hipMemcpyDeviceToHost));
    SLIO_HIP(hipMemcpy(z, w + 2 * c.icp_n, 4 * c.icp_n, hipMemcpyDeviceToHost));
  }
  return SLIO_OK;
}

int slio_icp_far_queries(slio_handle h, int64_t* n) {
  if (!h || !n) {
    set_error(h ? "slio_icp_far_queries: bad arguments" : "null handle");
    return SLIO_EINVAL;
  }
  *n = h->c.icp_far;
  return SLIO_OK;
}

}  // extern "C"

// ---------------------------------------------------------------- LIO-SAM keyframe store and local map
// saveKeyFramesAndFactor's cornerCloudKeyFrames / surfCloudKeyFrames
// (mapOptmization.cpp:2069-2077) and extractCloud (:1204-1251) on the device.

// room for n more points in the arena (grown by half, the stored keyframes
// copied on the stream; hipFree waits for the copy)
static int kf_reserve(Ctx& c, int64_t n, const char* who) {
  if (c.kf_used + n <= c.kf_cap) return SLIO_OK;
  const int64_t cap = std::max<int64_t>(c.kf_used + n + (c.kf_used + n) / 2, 1 << 16);
  float* q[3] = {nullptr, nullptr, nullptr};
  float* const old[3] = {c.kfx, c.kfy, c.kfz};
  hipError_t e = hipSuccess;
  for (int a = 0; a < 3 && !e; ++a) {
    e = hipMalloc(&q[a], 4 * cap);
    if (!e && c.kf_used > 0) e = hipMemcpyAsync(q[a], old[a], 4 * c.kf_used, hipMemcpyDeviceToDevice, c.stream);
  }
  if (!e) e = hipStreamSynchronize(c.stream);
  if (e) {
    (void)hipGetLastError();
    for (float* p : q)
      if (p) (void)hipFree(p);
    set_error(std::string(who) + ": keyframe arena: " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? SLIO_ENOMEM : SLIO_EDEVICE;
  }
  for (float* p : old)
    if (p) (void)hipFree(p);
  c.kfx = q[0];
  c.kfy = q[1];
  c.kfz = q[2];
  c.kf_cap = cap;
  return SLIO_OK;
}

static void kf_append(Ctx& c, int64_t n, int32_t* key_index) {
  if (key_index) *key_index = (int32_t)c.kf_off.size();
  c.kf_off.push_back(c.kf_used);
  c.kf_len.push_back(n);
  c.kf_used += n;
}

#define SLIO_KF_ARGS(cond, who)                  \
  do {                                           \
    if (!h) {                                    \
      set_error("null handle");                  \
      return SLIO_EINVAL;                        \
    }                                            \
    if (cond) {                                  \
      set_error(who ": bad arguments");          \
      return SLIO_EINVAL;                        \
    }                                            \
  } while (0)

extern "C" {

int slio_s2m_kf_push(slio_handle h, const float* x, const float* y, const float* z, int64_t n,
                     int32_t* key_index) {
  SLIO_KF_ARGS(n < 0 || (n > 0 && (!x || !y || !z)) || n > INT32_MAX, "slio_s2m_kf_push");
  Ctx& c = h->c;
  if (c.kf_off.size() >= (size_t)INT32_MAX) {
    set_error("slio_s2m_kf_push: too many keyframes");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(c.prm.device));
  if (n > 0) {
    if (int rc = kf_reserve(c, n, "slio_s2m_kf_push")) return rc;
    const int64_t o = c.kf_used;
    SLIO_HIP(hipMemcpyAsync(c.kfx + o, x, 4 * n, hipMemcpyHostToDevice, c.stream));
    SLIO_HIP(hipMemcpyAsync(c.kfy + o, y, 4 * n, hipMemcpyHostToDevice, c.stream));
    SLIO_HIP(hipMemcpyAsync(c.kfz + o, z, 4 * n, hipMemcpyHostToDevice, c.stream));
  }
  kf_append(c, n, key_index);
  return SLIO_OK;
}

int slio_s2m_kf_push_scan(slio_handle h, int32_t* key_index) {
  SLIO_KF_ARGS(false, "slio_s2m_kf_push_scan");
  Ctx& c = h->c;
  if (!c.bx) {
    set_error("slio_s2m_kf_push_scan: no scan uploaded");
    return SLIO_ESTATE;
  }
  if (c.kf_off.size() >= (size_t)INT32_MAX) {
    set_error("slio_s2m_kf_push_scan: too many keyframes");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(c.prm.device));
  const int64_t n = c.n;
  if (n > 0) {
    if (int rc = kf_reserve(c, n, "slio_s2m_kf_push_scan")) return rc;
    const int64_t o = c.kf_used;
    SLIO_HIP(hipMemcpyAsync(c.kfx + o, c.bx, 4 * n, hipMemcpyDeviceToDevice, c.stream));
    SLIO_HIP(hipMemcpyAsync(c.kfy + o, c.by, 4 * n, hipMemcpyDeviceToDevice, c.stream));
    SLIO_HIP(hipMemcpyAsync(c.kfz + o, c.bz, 4 * n, hipMemcpyDeviceToDevice, c.stream));
  }
  kf_append(c, n, key_index);
  return SLIO_OK;
}

int slio_s2m_kf_info(slio_handle h, int32_t* nkeys, int64_t* npoints) {
  SLIO_KF_ARGS(false, "slio_s2m_kf_info");
  if (nkeys) *nkeys = (int32_t)h->c.kf_off.size();
  if (npoints) *npoints = h->c.kf_used;
  return SLIO_OK;
}

int slio_s2m_kf_sizes(slio_handle h, int64_t* sizes, int64_t cap) {
  SLIO_KF_ARGS(cap < 0 || (cap > 0 && !sizes), "slio_s2m_kf_sizes");
  const auto& len = h->c.kf_len;
  if (cap < (int64_t)len.size()) {
    set_error("slio_s2m_kf_sizes: buffer too small");
    return SLIO_ECAPACITY;
  }
  for (size_t k = 0; k < len.size(); ++k) sizes[k] = len[k];
  return SLIO_OK;
}

int slio_s2m_kf_clear(slio_handle h) {
  SLIO_KF_ARGS(false, "slio_s2m_kf_clear");
  // (the arena stays allocated; an assembly still in flight on the stream
  // reads it before any later push writes it: one stream)
  h->c.kf_off.clear();
  h->c.kf_len.clear();
  h->c.kf_used = 0;
  return SLIO_OK;
}

int slio_s2m_kf_get(slio_handle h, int32_t key, float* x, float* y, float* z, int64_t cap, int64_t* n) {
  SLIO_KF_ARGS(key < 0 || (size_t)key >= h->c.kf_off.size() || cap < 0, "slio_s2m_kf_get");
  Ctx& c = h->c;
  const int64_t len = c.kf_len[key], o = c.kf_off[key];
  if (n) *n = len;
  if (cap < len || (len > 0 && (!x || !y || !z))) {
    set_error("slio_s2m_kf_get: buffer too small");
    return SLIO_ECAPACITY;
  }
  if (len > 0) {
    SLIO_HIP(hipSetDevice(c.prm.device));
    SLIO_HIP(hipStreamSynchronize(c.stream));
    SLIO_HIP(hipMemcpy(x, c.kfx + o, 4 * len, hipMemcpyDeviceToHost));
    SLIO_HIP(hipMemcpy(y, c.kfy + o, 4 * len, hipMemcpyDeviceToHost));
    SLIO_HIP(hipMemcpy(z, c.kfz + o, 4 * len, hipMemcpyDeviceToHost));
  }
  return SLIO_OK;
}

}  // extern "C"

// The segment table of an assembly: for i in list order keyframe key_ind[i]
// of every store in src[0..nsrc), at pose poses6[6 i ..]; non-empty entries
// only, so a tile of the gather touches at most one segment per point.  No
// device call.
// form 0: poses6 = {roll, pitch, yaw, x, y, z} as a float affine (LIO-SAM);
// form 1: poses6 = LeGO-LOAM's {rx, ry, rz, tx, ty, tz} as a LegoRot
static int kf_segments(const Ctx* const* src, int nsrc, const int32_t* key_ind, const float* poses6, int32_t nsel,
                       std::vector<KfSeg>& seg, int64_t& n, const char* who, int form = 0) {
  n = 0;
  for (int32_t i = 0; i < nsel; ++i) {
    const int32_t k = key_ind[i];
    if (k < 0 || (size_t)k >= src[0]->kf_off.size()) {
      set_error(std::string(who) + ": key index " + std::to_string(k) + " out of range");
      return SLIO_EINVAL;
    }
    Aff12 T{};
    if (form == 0) {
      T = s2m_affine(poses6 + 6 * (int64_t)i);
    } else {
      const LegoRot R = lmap_rot(poses6 + 6 * (int64_t)i);
      std::memcpy(T.m, &R, sizeof(R));
    }
    for (int a = 0; a < nsrc; ++a) {
      const Ctx& sc = *src[a];
      if (sc.kf_len[k] == 0) continue;
      // the (int)n radix sorts of the VoxelGrid and of build_index
      if (n + sc.kf_len[k] > (int64_t)INT32_MAX) {
        set_error(std::string(who) + ": more than 2^31 - 1 points selected");
        return SLIO_ECAPACITY;
      }
      KfSeg s;
      s.x = sc.kfx + sc.kf_off[k];
      s.y = sc.kfy + sc.kf_off[k];
      s.z = sc.kfz + sc.kf_off[k];
      s.off = (uint32_t)n;
      s.pad = 0;
      std::memcpy(s.m, T.m, sizeof(s.m));
      seg.push_back(s);
      n += sc.kf_len[k];
    }
  }
  return SLIO_OK;
}

extern "C" {

int slio_s2m_map_from_keyframes(slio_handle h, const int32_t* key_ind, const float* poses6, int32_t nsel,
                                float leaf, int64_t counts[2]) {
  static const char* who = "slio_s2m_map_from_keyframes";
  SLIO_KF_ARGS(nsel < 0 || (nsel > 0 && (!key_ind || !poses6)) || !(leaf > 0.0f), "slio_s2m_map_from_keyframes");
  Ctx& c = h->c;
  std::vector<KfSeg> seg;
  int64_t n = 0;
  const Ctx* src[1] = {&c};
  if (int rc = kf_segments(src, 1, key_ind, poses6, nsel, seg, n, who)) return rc;
  SLIO_HIP(hipSetDevice(c.prm.device));
  return kf_assemble(c, seg, n, leaf, false, counts, who);
}

int slio_s2m_loop_cloud(slio_handle h_dst, slio_handle h_corner, slio_handle h_surf, const int32_t* key_ind,
                        const float* poses6, int32_t nsel, float leaf, int as_scan, int64_t counts[2]) {
  static const char* who = "slio_s2m_loop_cloud";
  if (!h_dst || !h_corner || !h_surf) {
    set_error("null handle");
    return SLIO_EINVAL;
  }
  if (nsel < 0 || (nsel > 0 && (!key_ind || !poses6)) || !(leaf > 0.0f) || (as_scan != 0 && as_scan != 1)) {
    set_error("slio_s2m_loop_cloud: bad arguments");
    return SLIO_EINVAL;
  }
  Ctx& c = h_dst->c;
  Ctx* const srcs[2] = {&h_corner->c, &h_surf->c};
  for (const Ctx* s : {(const Ctx*)&c, (const Ctx*)srcs[0], (const Ctx*)srcs[1]})
    if (s->prm.nranks != 1 || s->prm.device != c.prm.device) {
      set_error("slio_s2m_loop_cloud: single-rank handles on one device only");
      return SLIO_EINVAL;
    }
  if (srcs[0]->kf_off.size() != srcs[1]->kf_off.size()) {
    set_error("slio_s2m_loop_cloud: the corner and surf stores hold different numbers of keyframes");
    return SLIO_EINVAL;
  }
  std::vector<KfSeg> seg;
  int64_t n = 0;
  const Ctx* src[2] = {srcs[0], srcs[1]};
  if (int rc = kf_segments(src, 2, key_ind, poses6, nsel, seg, n, who)) return rc;
  SLIO_HIP(hipSetDevice(c.prm.device));
  // the stores' pushes (copies on their own streams) come before the gather
  if (n > 0)
    for (Ctx* s : srcs) {
      if (s == &c || s->stream == c.stream || (s == srcs[1] && srcs[1] == srcs[0])) continue;
      if (!s->kf_ev) SLIO_HIP(hipEventCreateWithFlags(&s->kf_ev, hipEventDisableTiming));
      SLIO_HIP(hipEventRecord(s->kf_ev, s->stream));
      SLIO_HIP(hipStreamWaitEvent(c.stream, s->kf_ev, 0));
    }
  return kf_assemble(c, seg, n, leaf, as_scan != 0, counts, who);
}

}  // extern "C"

// ---------------------------------------------------------------- LeGO-LOAM mapping
// mapOptmization.cpp of LeGO-LOAM with loopClosureEnableFlag = false
// (slio_lmap_*, slio.h): downsampleCurrentScan from the front-end's device
// clouds, extractSurroundingKeyFrames' map assembly from three keyframe
// stores, cornerOptimization / surfOptimization / LMOptimization's rows
// (k_lmap_coeff) and scan2MapOptimization's loop.  The mapper owns four
// handles that share one stream, so every stage is ordered by the stream
// alone.  The host formulas (transformAssociateToMap, transformUpdate,
// transformFusion, the keyframe decision) are in slio_lmap.cpp.
struct slio_lmap {
  slio_lmap_params prm{};
  // (h[SLIO_LMAP_LOOP] is created on first use: a mapper without loop closure
  // allocates what it always did)
  slio_handle h[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  std::vector<float> poses6;   // cloudKeyPoses6D: {rx, ry, rz, tx, ty, tz} per key
  bool coeff_ok[2] = {false, false};
};

static int lmap_check(slio_lmap_handle m, const char* who) {
  if (!m) {
    set_error(std::string(who) + ": null mapper");
    return SLIO_EINVAL;
  }
  return SLIO_OK;
}

// VoxelGrid of n device points (float4 xyzi) into handle c's scan
static int lmap_voxel4(Ctx& c, const float4* src, int64_t n, float leaf, int64_t* n_down) {
  float *dx_ = nullptr, *dy_ = nullptr, *dz_ = nullptr;
  if (n > 0) {
    hipError_t e;
    if ((e = MapDev::take(c.pre[0], 12 * n))) {
      set_error(std::string("slio_lmap_feed: hipMalloc: ") + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
    dx_ = (float*)c.pre[0].p;
    dy_ = dx_ + n;
    dz_ = dx_ + 2 * n;
    k_lmap_split4<<<grid_blocks(n), 256, 0, c.stream>>>(src, n, dx_, dy_, dz_);
    SLIO_HIP(hipGetLastError());
  }
  return voxel_device(c, dx_, dy_, dz_, n, leaf, n_down);
}

// downsampleCurrentScan (:1197-1220) from three device clouds
static int lmap_feed_dev(slio_lmap* m, const float4* corner, int64_t nc, const float4* surf, int64_t ns,
                         const float4* outlier, int64_t no, int64_t counts[4]) {
  m->coeff_ok[0] = m->coeff_ok[1] = false;
  int64_t k[4] = {0, 0, 0, 0};
  Ctx& cc = m->h[SLIO_LMAP_CORNER]->c;
  Ctx& ct = m->h[SLIO_LMAP_SURF_TOTAL]->c;
  Ctx& cs = m->h[SLIO_LMAP_SURF]->c;
  Ctx& co = m->h[SLIO_LMAP_OUTLIER]->c;
  if (int rc = lmap_voxel4(cc, corner, nc, m->prm.leaf_corner, &k[0])) return rc;
  if (int rc = lmap_voxel4(cs, surf, ns, m->prm.leaf_surf, &k[2])) return rc;
  if (int rc = lmap_voxel4(co, outlier, no, m->prm.leaf_outlier, &k[3])) return rc;
  // laserCloudSurfTotalLast = surfLastDS ++ outlierLastDS (:1215-1216), then
  // downSizeFilterSurf again (:1217-1218)
  const int64_t nt = k[2] + k[3];
  float *tx = nullptr, *ty = nullptr, *tz = nullptr;
  if (nt > 0) {
    hipError_t e;
    if ((e = MapDev::take(ct.pre[0], 12 * nt))) {
      set_error(std::string("slio_lmap_feed: hipMalloc: ") + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
    tx = (float*)ct.pre[0].p;
    ty = tx + nt;
    tz = tx + 2 * nt;
    const Ctx* src[2] = {&cs, &co};
    int64_t o = 0;
    for (const Ctx* s : src) {
      if (s->n == 0) continue;
      SLIO_HIP(hipMemcpyAsync(tx + o, s->bx, 4 * s->n, hipMemcpyDeviceToDevice, ct.stream));
      SLIO_HIP(hipMemcpyAsync(ty + o, s->by, 4 * s->n, hipMemcpyDeviceToDevice, ct.stream));
      SLIO_HIP(hipMemcpyAsync(tz + o, s->bz, 4 * s->n, hipMemcpyDeviceToDevice, ct.stream));
      o += s->n;
    }
  }
  if (int rc = voxel_device(ct, tx, ty, tz, nt, m->prm.leaf_surf, &k[1])) return rc;
  if (counts)
    for (int i = 0; i < 4; ++i) counts[i] = k[i];
  return SLIO_OK;
}

// one kind's transform, search and coefficient + rows launch, enqueued
static int lmap_coeffs_enqueue(slio_lmap* m, int kind, const float transform[6]) {
  Ctx& c = m->h[kind == 0 ? SLIO_LMAP_CORNER : SLIO_LMAP_SURF_TOTAL]->c;
  const int64_t n = c.n;
  const int rc = s2m_search(
      c, "slio_lmap_coeffs",
      [&] {
        k_lmap_transform<<<grid_blocks(n), 256, 0, c.stream>>>(c.bx, c.by, c.bz, n, lmap_rot(transform), c.wbx,
                                                               c.wby, c.wbz);
      },
      [&] {
        // LMOptimization's trig, from transformTobeMapped[0..2] as written (:1457-1462)
        const S2mTrig T = s2m_trig(transform[0], transform[1], transform[2]);
        auto* k = kind == 0 ? k_lmap_coeff<0> : k_lmap_coeff<1>;
        k<<<(int)((n + 255) / 256), 256, 0, c.stream>>>(c.bx, c.by, c.bz, c.wbx, c.wby, c.wbz, n, c.nbr_pos,
                                                        c.nbr_sqd, c.map->pts, c.plane, c.sel, T, c.chunk_part);
      });
  if (rc) return rc;
  c.s2m_kind = kind;
  m->coeff_ok[kind] = true;
  return SLIO_OK;
}

// the two kinds' partials summed in the fixed order (corners, then surfs)
static int lmap_sum(slio_lmap* m, float AtA[36], float AtB[6], int64_t* nsel) {
  Ctx* const cs[2] = {&m->h[SLIO_LMAP_CORNER]->c, &m->h[SLIO_LMAP_SURF_TOTAL]->c};
  return s2m_sum(cs, 2, AtA, AtB, nsel);
}

static int lmap_coeff_state(slio_lmap* m, int kind, const char* who) {
  Ctx& c = m->h[kind == 0 ? SLIO_LMAP_CORNER : SLIO_LMAP_SURF_TOTAL]->c;
  if (!c.map || !c.bx) {
    set_error(std::string(who) + ": map and scan needed");
    return SLIO_ESTATE;
  }
  return SLIO_OK;
}

// the loop closure's handle (map = nearHistorySurfKeyFrameCloudDS, scan =
// latestSurfKeyFrameCloud), on the mapper's stream
static int lmap_loop_handle(slio_lmap* m) {
  if (m->h[SLIO_LMAP_LOOP]) return SLIO_OK;
  slio_params sp;
  slio_params_default(&sp);
  sp.device = m->prm.device;
  sp.max_points = m->prm.max_points;
  sp.grid_cell = m->prm.grid_cell;
  slio_handle h = nullptr;
  int rc = slio_create(&h, &sp);
  if (!rc) rc = slio_set_stream(h, (void*)m->h[0]->c.stream);
  if (!rc) rc = ensure_scan_buffers(h->c);
  if (rc) {
    if (h) {
      (void)slio_set_stream(h, nullptr);
      (void)slio_destroy(h);
    }
    return rc;
  }
  m->h[SLIO_LMAP_LOOP] = h;
  return SLIO_OK;
}

extern "C" {

int slio_lmap_params_default(slio_lmap_params* p) {
  if (!p) {
    set_error("slio_lmap_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->device = 0;
  p->max_points = 100000;
  p->leaf_corner = 0.2f;
  p->leaf_surf = 0.4f;
  p->leaf_outlier = 0.4f;
  p->pose_leaf = 1.0f;
  p->search_radius = 50.0f;
  p->max_iterations = 10;
  p->mapping_interval = 0.3f;
  p->scan_period = 0.1f;
  p->keyframe_distance = 0.3f;
  p->grid_cell = 0.0f;
  return SLIO_OK;
}

int slio_lmap_destroy(slio_lmap_handle m) {
  if (!m) return SLIO_OK;
  int rc = SLIO_OK;
  // (handle 0 owns the stream the others borrow: destroyed last)
  for (int i = 4; i >= 0; --i)
    if (m->h[i]) {
      if (i > 0) (void)slio_set_stream(m->h[i], nullptr);
      const int r = slio_destroy(m->h[i]);
      if (r && !rc) rc = r;
    }
  delete m;
  return rc;
}

int slio_lmap_create(slio_lmap_handle* out, const slio_lmap_params* p) {
  if (!out || !p) {
    set_error("slio_lmap_create: null argument");
    return SLIO_EINVAL;
  }
  *out = nullptr;
  if (p->max_points < 1 || !(p->leaf_corner > 0.0f) || !(p->leaf_surf > 0.0f) || !(p->leaf_outlier > 0.0f) ||
      p->max_iterations < 0 || p->device < 0 || !(p->grid_cell >= 0.0f)) {
    set_error("slio_lmap_create: bad max_points / leaves / max_iterations / device / grid_cell");
    return SLIO_EINVAL;
  }
  auto* m = new slio_lmap();
  m->prm = *p;
  slio_params sp;
  slio_params_default(&sp);
  sp.device = p->device;
  sp.max_points = p->max_points;
  sp.grid_cell = p->grid_cell;
  for (int i = 0; i < 4; ++i) {
    int rc = slio_create(&m->h[i], &sp);
    if (!rc && i > 0) rc = slio_set_stream(m->h[i], (void*)m->h[0]->c.stream);
    if (!rc) rc = ensure_scan_buffers(m->h[i]->c);
    if (rc) {
      (void)slio_lmap_destroy(m);
      return rc;
    }
  }
  *out = m;
  return SLIO_OK;
}

int slio_lmap_get_handle(slio_lmap_handle m, int which, slio_handle* out) {
  if (int rc = lmap_check(m, "slio_lmap_get_handle")) return rc;
  if (which < 0 || which > SLIO_LMAP_LOOP || !out) {
    set_error("slio_lmap_get_handle: bad arguments");
    return SLIO_EINVAL;
  }
  if (which == SLIO_LMAP_LOOP)
    if (int rc = lmap_loop_handle(m)) return rc;
  // the caller may upload a scan or a map through it: nothing cached here survives that
  m->coeff_ok[0] = m->coeff_ok[1] = false;
  *out = m->h[which];
  return SLIO_OK;
}

int slio_lmap_feed_lego(slio_lmap_handle m, void* lego, int64_t counts[4]) {
  if (int rc = lmap_check(m, "slio_lmap_feed_lego")) return rc;
  if (!lego) {
    set_error("slio_lmap_feed_lego: null front-end handle");
    return SLIO_EINVAL;
  }
  slio_lego_last_view v;
  if (int rc = slio_lego_odom_last_view((slio_lego_handle)lego, &v)) return rc;
  if (!v.published) {
    set_error("slio_lmap_feed_lego: the last odometry call did not publish");
    return SLIO_ESTATE;
  }
  if (v.device != m->prm.device) {
    set_error("slio_lmap_feed_lego: the front-end is on another device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  return lmap_feed_dev(m, (const float4*)v.corner_xyzi, v.n_corner, (const float4*)v.surf_xyzi, v.n_surf,
                       (const float4*)v.outlier_xyzi, v.n_outlier, counts);
}

int slio_lmap_feed_host(slio_lmap_handle m, const float* corner_xyzi, int64_t n_corner, const float* surf_xyzi,
                        int64_t n_surf, const float* outlier_xyzi, int64_t n_outlier, int64_t counts[4]) {
  if (int rc = lmap_check(m, "slio_lmap_feed_host")) return rc;
  const float* src[3] = {corner_xyzi, surf_xyzi, outlier_xyzi};
  const int64_t n[3] = {n_corner, n_surf, n_outlier};
  for (int i = 0; i < 3; ++i)
    if (n[i] < 0 || (n[i] > 0 && !src[i]) || n[i] > INT32_MAX) {
      set_error("slio_lmap_feed_host: bad arguments");
      return SLIO_EINVAL;
    }
  SLIO_HIP(hipSetDevice(m->prm.device));
  // staged in the surf-total handle's temporaries (its own VoxelGrid runs last
  // and uses pre[0] and pre[8..])
  Ctx& ct = m->h[SLIO_LMAP_SURF_TOTAL]->c;
  float4* d[3] = {nullptr, nullptr, nullptr};
  for (int i = 0; i < 3; ++i) {
    if (n[i] == 0) continue;
    hipError_t e;
    if ((e = MapDev::take(ct.pre[1 + i], 16 * n[i]))) {
      set_error(std::string("slio_lmap_feed_host: hipMalloc: ") + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
    d[i] = (float4*)ct.pre[1 + i].p;
    SLIO_HIP(hipMemcpyAsync(d[i], src[i], 16 * n[i], hipMemcpyHostToDevice, ct.stream));
  }
  return lmap_feed_dev(m, d[0], n[0], d[1], n[1], d[2], n[2], counts);
}

int slio_lmap_extract(slio_lmap_handle m, const int32_t* key_ind, int32_t nsel, int64_t counts[4]) {
  static const char* who = "slio_lmap_extract";
  if (int rc = lmap_check(m, who)) return rc;
  if (nsel < 0 || (nsel > 0 && !key_ind)) {
    set_error("slio_lmap_extract: bad arguments");
    return SLIO_EINVAL;
  }
  Ctx& cc = m->h[SLIO_LMAP_CORNER]->c;
  Ctx& ct = m->h[SLIO_LMAP_SURF_TOTAL]->c;
  const int32_t nkeys = (int32_t)(m->poses6.size() / 6);
  std::vector<float> poses((size_t)nsel * 6);
  for (int32_t i = 0; i < nsel; ++i) {
    if (key_ind[i] < 0 || key_ind[i] >= nkeys) {
      set_error("slio_lmap_extract: key index " + std::to_string(key_ind[i]) + " out of range");
      return SLIO_EINVAL;
    }
    std::memcpy(&poses[6 * (size_t)i], &m->poses6[6 * (size_t)key_ind[i]], 24);
  }
  std::vector<KfSeg> segc, segs;
  int64_t nc = 0, ns = 0;
  const Ctx* srcc[1] = {&cc};
  const Ctx* srcs[2] = {&m->h[SLIO_LMAP_SURF]->c, &m->h[SLIO_LMAP_OUTLIER]->c};
  if (int rc = kf_segments(srcc, 1, key_ind, poses.data(), nsel, segc, nc, who, 1)) return rc;
  if (int rc = kf_segments(srcs, 2, key_ind, poses.data(), nsel, segs, ns, who, 1)) return rc;
  SLIO_HIP(hipSetDevice(m->prm.device));
  m->coeff_ok[0] = m->coeff_ok[1] = false;
  int64_t k[4] = {0, 0, 0, 0};
  if (int rc = kf_assemble(cc, segc, nc, m->prm.leaf_corner, false, k, who, 1)) return rc;
  if (int rc = kf_assemble(ct, segs, ns, m->prm.leaf_surf, false, k + 2, who, 1)) return rc;
  if (counts)
    for (int i = 0; i < 4; ++i) counts[i] = k[i];
  return SLIO_OK;
}

int slio_lmap_coeffs(slio_lmap_handle m, int kind, const float transform[6], int64_t* nsel) {
  if (int rc = lmap_check(m, "slio_lmap_coeffs")) return rc;
  if ((kind != 0 && kind != 1) || !transform) {
    set_error("slio_lmap_coeffs: bad arguments");
    return SLIO_EINVAL;
  }
  if (int rc = lmap_coeff_state(m, kind, "slio_lmap_coeffs")) return rc;
  SLIO_HIP(hipSetDevice(m->prm.device));
  if (int rc = lmap_coeffs_enqueue(m, kind, transform)) return rc;
  return nsel ? s2m_count_sel(m->h[kind == 0 ? SLIO_LMAP_CORNER : SLIO_LMAP_SURF_TOTAL]->c, nsel) : SLIO_OK;
}

int slio_lmap_get_coeffs(slio_lmap_handle m, int kind, float* coeff, uint8_t* sel) {
  if (int rc = lmap_check(m, "slio_lmap_get_coeffs")) return rc;
  if (kind != 0 && kind != 1) {
    set_error("slio_lmap_get_coeffs: bad arguments");
    return SLIO_EINVAL;
  }
  if (!m->coeff_ok[kind]) {
    set_error("slio_lmap_get_coeffs: no coefficients of that kind");
    return SLIO_ESTATE;
  }
  return slio_s2m_get_coeffs(m->h[kind == 0 ? SLIO_LMAP_CORNER : SLIO_LMAP_SURF_TOTAL], coeff, sel);
}

int slio_lmap_normal_equations(slio_lmap_handle m, float AtA[36], float AtB[6], int64_t* nsel) {
  if (int rc = lmap_check(m, "slio_lmap_normal_equations")) return rc;
  if (!AtA || !AtB) {
    set_error("slio_lmap_normal_equations: bad arguments");
    return SLIO_EINVAL;
  }
  if (!m->coeff_ok[0] || !m->coeff_ok[1]) {
    set_error("slio_lmap_normal_equations: slio_lmap_coeffs of both kinds first");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  return lmap_sum(m, AtA, AtB, nsel);
}

int slio_lmap_optimize(slio_lmap_handle m, float transform[6], int32_t* iterations, int32_t* is_degenerate) {
  if (int rc = lmap_check(m, "slio_lmap_optimize")) return rc;
  if (!transform || !iterations || !is_degenerate) {
    set_error("slio_lmap_optimize: bad arguments");
    return SLIO_EINVAL;
  }
  for (int kind = 0; kind < 2; ++kind)
    if (int rc = lmap_coeff_state(m, kind, "slio_lmap_optimize")) return rc;
  *iterations = 0;
  *is_degenerate = 0;
  // :1606
  if (!(m->h[SLIO_LMAP_CORNER]->c.map->n > 10 && m->h[SLIO_LMAP_SURF_TOTAL]->c.map->n > 100)) return SLIO_OK;
  SLIO_HIP(hipSetDevice(m->prm.device));
  float matP[36] = {0};
  int deg = 0;
  for (int it = 0; it < m->prm.max_iterations; ++it) {
    if (int rc = lmap_coeffs_enqueue(m, 0, transform)) return rc;
    if (int rc = lmap_coeffs_enqueue(m, 1, transform)) return rc;
    float AtA[36], AtB[6];
    int64_t nsel = 0;
    if (int rc = lmap_sum(m, AtA, AtB, &nsel)) return rc;
    int conv = 0;
    const int rc = slio_s2m_lm_step(AtA, AtB, nsel, it, transform, &deg, matP, &conv);
    if (rc < 0) return rc;
    *iterations = it + 1;
    if (conv) break;
  }
  *is_degenerate = deg;
  return SLIO_OK;
}

int slio_lmap_save_keyframe(slio_lmap_handle m, const float pose6[6], int32_t* key) {
  if (int rc = lmap_check(m, "slio_lmap_save_keyframe")) return rc;
  if (!pose6) {
    set_error("slio_lmap_save_keyframe: null pose");
    return SLIO_EINVAL;
  }
  const int which[3] = {SLIO_LMAP_CORNER, SLIO_LMAP_SURF, SLIO_LMAP_OUTLIER};
  int32_t k = -1;
  for (int w : which) {
    int32_t kk = -1;
    if (int rc = slio_s2m_kf_push_scan(m->h[w], &kk)) return rc;
    k = kk;
  }
  m->poses6.insert(m->poses6.end(), pose6, pose6 + 6);
  if (key) *key = k;
  return SLIO_OK;
}

int slio_lmap_get_key_poses(slio_lmap_handle m, float* poses6, int32_t cap, int32_t* nkeys) {
  if (int rc = lmap_check(m, "slio_lmap_get_key_poses")) return rc;
  const int32_t nk = (int32_t)(m->poses6.size() / 6);
  if (nkeys) *nkeys = nk;
  if (poses6) {
    if (cap < nk) {
      set_error("slio_lmap_get_key_poses: buffer too small");
      return SLIO_ECAPACITY;
    }
    if (nk) std::memcpy(poses6, m->poses6.data(), sizeof(float) * m->poses6.size());
  }
  return SLIO_OK;
}

int slio_lmap_set_key_poses(slio_lmap_handle m, const float* poses6, int32_t nkeys) {
  if (int rc = lmap_check(m, "slio_lmap_set_key_poses")) return rc;
  if (nkeys < 0 || (nkeys > 0 && !poses6) || (size_t)nkeys * 6 != m->poses6.size()) {
    set_error("slio_lmap_set_key_poses: nkeys must equal the key-pose table's length (" +
              std::to_string(m->poses6.size() / 6) + ")");
    return SLIO_EINVAL;
  }
  if (nkeys) std::memcpy(m->poses6.data(), poses6, sizeof(float) * m->poses6.size());
  return SLIO_OK;
}

int slio_lmap_loop_clouds(slio_lmap_handle m, int32_t latest, int32_t closest, int32_t search_num, float leaf,
                          int64_t counts[4]) {
  static const char* who = "slio_lmap_loop_clouds";
  if (int rc = lmap_check(m, who)) return rc;
  const int32_t nkeys = (int32_t)(m->poses6.size() / 6);
  if (latest < 0 || latest >= nkeys || closest < 0 || closest >= nkeys || search_num < 0 || !(leaf > 0.0f)) {
    set_error("slio_lmap_loop_clouds: key out of range, negative search_num or bad leaf");
    return SLIO_EINVAL;
  }
  // :914-918: closest - search_num .. closest + search_num, skipping k < 0 and k > latest
  std::vector<int32_t> tkeys;
  for (int64_t k = (int64_t)closest - search_num; k <= (int64_t)closest + search_num; ++k)
    if (k >= 0 && k <= latest) tkeys.push_back((int32_t)k);
  std::vector<float> tposes(tkeys.size() * 6);
  for (size_t i = 0; i < tkeys.size(); ++i) std::memcpy(&tposes[6 * i], &m->poses6[6 * (size_t)tkeys[i]], 24);
  const Ctx* src[2] = {&m->h[SLIO_LMAP_CORNER]->c, &m->h[SLIO_LMAP_SURF]->c};
  std::vector<KfSeg> sseg, tseg;
  int64_t ns = 0, nt = 0;
  if (int rc = kf_segments(src, 2, &latest, &m->poses6[6 * (size_t)latest], 1, sseg, ns, who, 1)) return rc;
  if (int rc = kf_segments(src, 2, tkeys.data(), tposes.data(), (int32_t)tkeys.size(), tseg, nt, who, 1)) return rc;
  if (int rc = lmap_loop_handle(m)) return rc;
  SLIO_HIP(hipSetDevice(m->prm.device));
  Ctx& cl = m->h[SLIO_LMAP_LOOP]->c;
  int64_t k[4] = {0, 0, 0, 0};
  if (int rc = kf_assemble(cl, sseg, ns, leaf, true, k, who, 1, true)) return rc;
  if (int rc = kf_assemble(cl, tseg, nt, leaf, false, k + 2, who, 1)) return rc;
  if (counts)
    for (int i = 0; i < 4; ++i) counts[i] = k[i];
  return SLIO_OK;
}

int slio_lmap_clear(slio_lmap_handle m) {
  if (int rc = lmap_check(m, "slio_lmap_clear")) return rc;
  const int which[3] = {SLIO_LMAP_CORNER, SLIO_LMAP_SURF, SLIO_LMAP_OUTLIER};
  for (int w : which)
    if (int rc = slio_s2m_kf_clear(m->h[w])) return rc;
  m->poses6.clear();
  m->coeff_ok[0] = m->coeff_ok[1] = false;
  return SLIO_OK;
}

}  // extern "C"

