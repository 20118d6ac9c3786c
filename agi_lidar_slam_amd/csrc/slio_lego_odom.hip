// slio_lego_odom.hip -- LeGO-LOAM scan-to-scan odometry on gfx950: the back
// half of FeatureAssociation::runFeatureAssociation
// (LeGO-LOAM/src/featureAssociation.cpp:2232-2248; C-ABI and the stated
// departures: include/slio_frontend.h; layout and summation order: DESIGN.md
// §3.12).
//
// Layout.  updateTransformation is at most 25 + 25 strictly sequential
// Gauss-Newton iterations over <= 192 / 384 queries; an iteration is far
// smaller than a launch, and a grid-wide seam per iteration would cost more
// than the iteration.  So the whole loop -- updateInitialGuess, both loops
// with their `continue` / `break`, integrateTransformation -- is ONE
// workgroup of 512 threads in one launch (k_lego_odom_loop); the only
// synchronisation is __syncthreads, and the per-sweep host traffic is one
// slio_lego_odom_out.  A second, wide launch (k_lego_odom_publish) runs
// TransformToEnd over the less clouds and permutes the outlier cloud.
//
// One iteration (odom_pass), all phases separated by __syncthreads:
//   0  a thread per query: TransformToStart (:1041-1070) -> psel
//   1  search iterations only (iter % 5 == 0): a wavefront per query.  Exact
//      1-NN over the last cloud as a packed (distance bits << 32 | index)
//      minimum (ties: lower index), then the two ring-bounded scans as
//      packed minima per direction and class -- forward (bits << 32 | j),
//      lowest j on a tie; backward (bits << 32 | ~j), highest j on a tie; the
//      backward winner replaces the forward one only on a strictly smaller
//      distance, which is what the sequential `<` updates give.  The rings
//      are non-decreasing in the index, so the reference's `break`s cut
//      exactly the points the ring filter drops.
//   2  a thread per query: the point-to-plane / point-to-line coefficient,
//      the s > 0.1 && d != 0 selection and the Jacobian row
//   3  normal equations: 13 rows of 32 lanes; lane s of row k adds, in
//      ascending query order, the fp64 products of the selected queries
//      q = s, s + 32, ...; then one thread per row adds the 32 partials in
//      ascending s and rounds to float.  No part of the order depends on the
//      launch geometry.
//   4  thread 0: the step (slio::lego::odom_step, slio_cvsolve.hpp)
// LDS: 13 * 32 doubles of partials + the 3 x 3 system and the transform:
// under 4 KiB.  The clouds stay in global memory (L2-resident: a few thousand
// float4).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <utility>

#include "slio_common.hpp"
#include "slio_cvsolve.hpp"
#include "slio_frontend.h"
#include "slio_lego_odom.hpp"

namespace slio {
namespace lego {

#define ODOM_HIP(call)                                              \
  do {                                                              \
    hipError_t e_ = (call);                                         \
    if (e_ != hipSuccess) {                                         \
      set_error(std::string(#call) + ": " + hipGetErrorString(e_)); \
      return SLIO_EDEVICE;                                          \
    }                                                               \
  } while (0)

constexpr int kOdomThreads = 512;
constexpr int kOdomWaves = kOdomThreads / 64;
constexpr int kOdomLanes = 32;  // partial sums per normal-equation entry
constexpr int kOdomSums = 13;   // AtA (9), AtB (3), the row count
constexpr int kOdomMaxIter = 64;

// device-resident state: the member variables, the last result, and the
// single-pass outputs of the lockstep entry
struct OdomDev {
  slio_lego_odom_state st;
  slio_lego_odom_out out;
  float pass_AtA[9], pass_AtB[3];
  int32_t pass_nsel;
};

struct OdomArgs {
  const float4 *sharp, *flat, *corner_last, *surf_last;
  const int64_t* counts;  // n_sharp [0], n_less_sharp [1], n_flat [2], n_less_flat [3]
  float4* psel;           // [cap_q] TransformToStart of the queries
  int32_t* ind;           // [2][3 * cap_q] pointSearch{Surf,Corner}Ind1 / Ind2 / Ind3, one set per kind
  float4* coeff;          // [cap_q]
  float4* rows;           // [cap_q] the Jacobian row and B
  uint8_t* sel;           // [cap_q]
  OdomDev* dev;
  const LegoImuOutDev* io;
  float gate, scan_period;
  int max_iter, period, skip, cap_q, cap_flat;  // cap_q: sharp capacity (>= cap_flat)
  int64_t cap_corner, cap_surf;
};

struct Tc6 {
  float v[6];
};

__device__ __forceinline__ float dcos(float a) { return (float)cos((double)a); }
__device__ __forceinline__ float dsin(float a) { return (float)sin((double)a); }
__device__ __forceinline__ float dasin(float a) { return (float)asin((double)a); }
__device__ __forceinline__ float datan2(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ __forceinline__ float dsqrt(float a) { return (float)sqrt((double)a); }

// TransformToStart (:1041-1070)
__device__ float4 to_start(const float4 pi, const float* tc) {
  const float s = 10 * (pi.w - (float)(int)pi.w);
  const float rx = s * tc[0], ry = s * tc[1], rz = s * tc[2];
  const float tx = s * tc[3], ty = s * tc[4], tz = s * tc[5];
  const float crz = dcos(rz), srz = dsin(rz), crx = dcos(rx), srx = dsin(rx), cry = dcos(ry), sry = dsin(ry);
  const float x1 = crz * (pi.x - tx) + srz * (pi.y - ty);
  const float y1 = -srz * (pi.x - tx) + crz * (pi.y - ty);
  const float z1 = (pi.z - tz);
  const float x2 = x1;
  const float y2 = crx * y1 + srx * z1;
  const float z2 = -srx * y1 + crx * z1;
  return make_float4(cry * x2 - sry * z2, y2, sry * x2 + cry * z2, pi.w);
}

__device__ __forceinline__ float sqdist(const float4 a, const float4 p) {
  return (a.x - p.x) * (a.x - p.x) + (a.y - p.y) * (a.y - p.y) + (a.z - p.z) * (a.z - p.z);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)(v & 0xffffffffull), o, 64);
    const unsigned hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long w = ((unsigned long long)hi << 32) | lo;
    v = w < v ? w : v;
  }
  return v;
}

constexpr unsigned long long kNoKey = ~0ull;

// the winner of a forward key (index in the low word) and a backward key
// (~index in the low word): forward first, backward only on a strictly
// smaller distance
__device__ __forceinline__ int pick_dir(unsigned long long kf, unsigned long long kb) {
  int r = -1;
  if (kf != kNoKey) r = (int)(unsigned)(kf & 0xffffffffull);
  if (kb != kNoKey && (kf == kNoKey || (unsigned)(kb >> 32) < (unsigned)(kf >> 32)))
    r = (int)(~(unsigned)(kb & 0xffffffffull));
  return r;
}

// One findCorresponding*Features(iter) pass + the rows and normal equations;
// every thread of the workgroup calls it.  Returns the selected-row count.
__device__ int odom_pass(const OdomArgs& a, int kind, int iter, const float* tc, float* s_AtA, float* s_AtB,
                         double* s_part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool corner = kind == kOdomCorner;
  const float4* qry = corner ? a.sharp : a.flat;
  const float4* last = corner ? a.corner_last : a.surf_last;
  int nq = (int)a.counts[corner ? 0 : 2];
  const int cap = corner ? a.cap_q : a.cap_flat;  // the query buffer's capacity
  nq = nq < 0 ? 0 : (nq > cap ? cap : nq);
  const int nl = corner ? a.dev->st.n_corner_last : a.dev->st.n_surf_last;
  // the reference bounds the forward scan by the CURRENT feature count; the
  // clamp to the last cloud's size is where it would read out of bounds
  const int fwd_end = nq < nl ? nq : nl;
  int32_t* const ind1 = a.ind + (size_t)kind * 3 * a.cap_q;  // the kind's own persistent indices
  int32_t *const ind2 = ind1 + a.cap_q, *const ind3 = ind1 + 2 * a.cap_q;

  for (int q = tid; q < nq; q += kOdomThreads) a.psel[q] = to_start(qry[q], tc);
  __syncthreads();

  if (iter % a.period == 0) {
    for (int q = wave; q < nq; q += kOdomWaves) {
      const float4 p = a.psel[q];
      unsigned long long best = kNoKey;
#pragma unroll 4  // independent loads in flight
      for (int j = lane; j < nl; j += 64) {
        const float d = sqdist(last[j], p);
        if (d < a.gate) {
          const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
          best = k < best ? k : best;
        }
      }
      best = wave_min(best);
      int c = -1, i2 = -1, i3 = -1;
      if (best != kNoKey) {
        c = (int)(unsigned)(best & 0xffffffffull);
        const int sc = (int)last[c].w;
        unsigned long long k2f = kNoKey, k2b = kNoKey, k3f = kNoKey, k3b = kNoKey;
        for (int j = c + 1 + lane; j < fwd_end; j += 64) {
          const float4 l = last[j];
          const int r = (int)l.w;
          if ((double)r > (double)sc + 2.5) break;  // the reference's break: rings do not decrease
          const float d = sqdist(l, p);
          if (!(d < a.gate)) continue;
          const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)j;
          if (corner) {
            if (r > sc) k2f = k < k2f ? k : k2f;
          } else if (r <= sc) {
            k2f = k < k2f ? k : k2f;
          } else {
            k3f = k < k3f ? k : k3f;
          }
        }
#pragma unroll 4
        for (int j = c - 1 - lane; j >= 0; j -= 64) {
          const float4 l = last[j];
          const int r = (int)l.w;
          if ((double)r < (double)sc - 2.5) break;  // every lower index is on a lower ring still
          const float d = sqdist(l, p);
          if (!(d < a.gate)) continue;
          const unsigned long long k = ((unsigned long long)__float_as_uint(d) << 32) | (~(unsigned)j);
          if (corner) {
            if (r < sc) k2b = k < k2b ? k : k2b;
          } else if (r >= sc) {
            k2b = k < k2b ? k : k2b;
          } else {
            k3b = k < k3b ? k : k3b;
          }
        }
        k2f = wave_min(k2f);
        k2b = wave_min(k2b);
        i2 = pick_dir(k2f, k2b);
        if (!corner) {
          k3f = wave_min(k3f);
          k3b = wave_min(k3b);
          i3 = pick_dir(k3f, k3b);
        }
      }
      if (lane == 0) {
        ind1[q] = c;
        ind2[q] = i2;
        ind3[q] = i3;
      }
    }
    __syncthreads();
  }

  // Jacobian constants (:1583-1618 / :1716-1735)
  const float srx = dsin(tc[0]), crx = dcos(tc[0]), sry = dsin(tc[1]), cry = dcos(tc[1]);
  const float srz = dsin(tc[2]), crz = dcos(tc[2]);
  const float tx = tc[3], ty = tc[4], tz = tc[5];
  const float b1 = -crz * sry - cry * srx * srz;
  const float b2 = cry * crz * srx - sry * srz;
  const float b5 = cry * crz - srx * sry * srz;
  const float b6 = cry * srz + crz * srx * sry;
  const float c5 = crx * srz;

  for (int q = tid; q < nq; q += kOdomThreads) {
    const float4 p = a.psel[q], po = qry[q];
    const int i1 = ind1[q], i2 = ind2[q], i3 = ind3[q];
    float4 co = make_float4(0.f, 0.f, 0.f, 0.f), row = co;
    uint8_t ok = 0;
    const bool in1 = i1 >= 0 && i1 < nl, in2 = i2 >= 0 && i2 < nl, in3 = i3 >= 0 && i3 < nl;
    if (corner) {
      if (in1 && in2) {
        const float4 t1 = last[i1], t2 = last[i2];
        const float x0 = p.x, y0 = p.y, z0 = p.z, x1 = t1.x, y1 = t1.y, z1 = t1.z, x2 = t2.x, y2 = t2.y,
                    z2 = t2.z;
        const float m11 = ((x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1));
        const float m22 = ((x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1));
        const float m33 = ((y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1));
        const float a012 = dsqrt(m11 * m11 + m22 * m22 + m33 * m33);
        const float l12 = dsqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2));
        const float la = ((y1 - y2) * m11 + (z1 - z2) * m22) / a012 / l12;
        const float lb = -((x1 - x2) * m11 - (z1 - z2) * m33) / a012 / l12;
        const float lc = -((x1 - x2) * m22 + (y1 - y2) * m33) / a012 / l12;
        const float ld2 = a012 / l12;
        float s = 1;
        if (iter >= 5) s = (float)(1 - 1.8 * fabs((double)ld2));
        if ((double)s > 0.1 && ld2 != 0) {
          co = make_float4(s * la, s * lb, s * lc, s * ld2);
          ok = 1;
          const float b3 = crx * cry;
          const float b4 = tx * -b1 + ty * -b2 + tz * b3;
          const float b7 = crx * sry;
          const float b8 = tz * b7 - ty * b6 - tx * b5;
          const float ary = (b1 * po.x + b2 * po.y - b3 * po.z + b4) * co.x +
                            (b5 * po.x + b6 * po.y - b7 * po.z + b8) * co.z;
          const float atx = -b5 * co.x + c5 * co.y + b1 * co.z;
          const float atz = b7 * co.x - srx * co.y - b3 * co.z;
          row = make_float4(ary, atx, atz, (float)(-0.05 * (double)co.w));
        }
      }
    } else if (in1 && in2 && in3) {
      const float4 t1 = last[i1], t2 = last[i2], t3 = last[i3];
      float pa = (t2.y - t1.y) * (t3.z - t1.z) - (t3.y - t1.y) * (t2.z - t1.z);
      float pb = (t2.z - t1.z) * (t3.x - t1.x) - (t3.z - t1.z) * (t2.x - t1.x);
      float pc = (t2.x - t1.x) * (t3.y - t1.y) - (t3.x - t1.x) * (t2.y - t1.y);
      float pd = -(pa * t1.x + pb * t1.y + pc * t1.z);
      const float ps = dsqrt(pa * pa + pb * pb + pc * pc);
      pa /= ps;
      pb /= ps;
      pc /= ps;
      pd /= ps;
      const float pd2 = pa * p.x + pb * p.y + pc * p.z + pd;
      float s = 1;
      if (iter >= 5)
        s = (float)(1 - 1.8 * fabs((double)pd2) / (double)dsqrt(dsqrt(p.x * p.x + p.y * p.y + p.z * p.z)));
      if ((double)s > 0.1 && pd2 != 0) {
        co = make_float4(s * pa, s * pb, s * pc, s * pd2);
        ok = 1;
        const float a1 = crx * sry * srz, a2 = crx * crz * sry, a3 = srx * sry;
        const float a4 = tx * a1 - ty * a2 - tz * a3;
        const float a5 = srx * srz, a6 = crz * srx;
        const float a7 = ty * a6 - tz * crx - tx * a5;
        const float a8 = crx * cry * srz, a9 = crx * cry * crz, a10 = cry * srx;
        const float a11 = tz * a10 + ty * a9 - tx * a8;
        const float c1 = -b6, c2 = b5, c3 = tx * b6 - ty * b5, c4 = -crx * crz;
        const float c6 = ty * c5 + tx * -c4, c7 = b2, c8 = -b1, c9 = tx * -b2 - ty * -b1;
        const float arx = (-a1 * po.x + a2 * po.y + a3 * po.z + a4) * co.x +
                          (a5 * po.x - a6 * po.y + crx * po.z + a7) * co.y +
                          (a8 * po.x - a9 * po.y - a10 * po.z + a11) * co.z;
        const float arz = (c1 * po.x + c2 * po.y + c3) * co.x + (c4 * po.x - c5 * po.y + c6) * co.y +
                          (c7 * po.x + c8 * po.y + c9) * co.z;
        const float aty = -b6 * co.x + c4 * co.y + b2 * co.z;
        row = make_float4(arx, arz, aty, (float)(-0.05 * (double)co.w));
      }
    }
    a.coeff[q] = co;
    a.rows[q] = row;
    a.sel[q] = ok;
  }
  __syncthreads();

  // normal equations in the fixed order of the header
  if (tid < kOdomSums * kOdomLanes) {
    const int k = tid / kOdomLanes, s = tid % kOdomLanes;
    double acc = 0.0;
    for (int q = s; q < nq; q += kOdomLanes) {
      if (!a.sel[q]) continue;
      const float4 r = a.rows[q];
      const float v[4] = {r.x, r.y, r.z, r.w};
      if (k < 9)
        acc += (double)v[k / 3] * (double)v[k % 3];
      else if (k < 12)
        acc += (double)v[k - 9] * (double)v[3];
      else
        acc += 1.0;
    }
    s_part[tid] = acc;
  }
  __syncthreads();
  __shared__ int s_nsel;
  if (tid < kOdomSums) {
    double t = 0.0;
    for (int s = 0; s < kOdomLanes; ++s) t += s_part[tid * kOdomLanes + s];
    if (tid < 9)
      s_AtA[tid] = (float)t;
    else if (tid < 12)
      s_AtB[tid - 9] = (float)t;
    else
      s_nsel = (int)t;
  }
  __syncthreads();
  return s_nsel;
}

// AccumulateRotation (:1246-1285)
__device__ void accumulate_rotation(float cx, float cy, float cz, float lx, float ly, float lz, float& ox,
                                    float& oy, float& oz) {
  const float scx = dsin(cx), ccx = dcos(cx), scy = dsin(cy), ccy = dcos(cy), scz = dsin(cz), ccz = dcos(cz);
  const float slx = dsin(lx), clx = dcos(lx), sly = dsin(ly), cly = dcos(ly), slz = dsin(lz), clz = dcos(lz);
  const float srx = clx * ccx * sly * scz - ccx * ccz * slx - clx * cly * scx;
  ox = -dasin(srx);
  const float srycrx = slx * (ccy * scz - ccz * scx * scy) + clx * sly * (ccy * ccz + scx * scy * scz) +
                       clx * cly * ccx * scy;
  const float crycrx = clx * cly * ccx * ccy - clx * sly * (ccz * scy - ccy * scx * scz) -
                       slx * (scy * scz + ccy * ccz * scx);
  oy = datan2(srycrx / dcos(ox), crycrx / dcos(ox));
  const float srzcrx = scx * (clz * sly - cly * slx * slz) + ccx * scz * (cly * clz + slx * sly * slz) +
                       clx * ccx * ccz * slz;
  const float crzcrx = clx * clz * ccx * ccz - ccx * scz * (cly * slz - clz * slx * sly) -
                       scx * (sly * slz + cly * clz * slx);
  oz = datan2(srzcrx / dcos(ox), crzcrx / dcos(ox));
}

// PluginIMURotation (:1145-1244), its repeated factors named once (u*, v*,
// T*: each is evaluated as the reference's parenthesised sub-expression)
__device__ void plugin_imu_rotation(float bcx, float bcy, float bcz, float blx, float bly, float blz, float alx,
                                    float aly, float alz, float& acx, float& acy, float& acz) {
  const float sbcx = dsin(bcx), cbcx = dcos(bcx), sbcy = dsin(bcy), cbcy = dcos(bcy), sbcz = dsin(bcz),
              cbcz = dcos(bcz);
  const float sblx = dsin(blx), cblx = dcos(blx), sbly = dsin(bly), cbly = dcos(bly), sblz = dsin(blz),
              cblz = dcos(blz);
  const float salx = dsin(alx), calx = dcos(alx), saly = dsin(aly), caly = dcos(aly), salz = dsin(alz),
              calz = dcos(alz);
  const float u1 = cbly * sblz - cblz * sblx * sbly;
  const float u2 = sbly * sblz + cbly * cblz * sblx;
  const float u3 = cblz * sbly - cbly * sblx * sblz;
  const float u4 = cbly * cblz + sblx * sbly * sblz;
  const float T1 = calx * saly * u1 - calx * caly * u2 + cblx * cblz * salx;
  const float T2 = calx * caly * u3 - calx * saly * u4 + cblx * salx * sblz;
  const float T3 = salx * sblx + calx * caly * cblx * cbly + calx * cblx * saly * sbly;
  const float srx = -sbcx * T3 - cbcx * cbcz * T1 - cbcx * sbcz * T2;
  acx = -dasin(srx);
  const float srycrx = (cbcy * sbcz - cbcz * sbcx * sbcy) * T1 - (cbcy * cbcz + sbcx * sbcy * sbcz) * T2 +
                       cbcx * sbcy * T3;
  const float crycrx = (cbcz * sbcy - cbcy * sbcx * sbcz) * T2 - (sbcy * sbcz + cbcy * cbcz * sbcx) * T1 +
                       cbcx * cbcy * T3;
  acy = datan2(srycrx / dcos(acx), crycrx / dcos(acx));
  const float v1 = caly * calz + salx * saly * salz;
  const float v2 = calz * saly - caly * salx * salz;
  const float v3 = saly * salz + caly * calz * salx;
  const float v4 = caly * salz - calz * salx * saly;
  const float srzcrx = sbcx * (cblx * cbly * v2 - cblx * sbly * v1 + calx * salz * sblx) -
                       cbcx * cbcz * (v1 * u1 + v2 * u2 - calx * cblx * cblz * salz) +
                       cbcx * sbcz * (v1 * u4 + v2 * u3 + calx * cblx * salz * sblz);
  const float crzcrx = sbcx * (cblx * sbly * v4 - cblx * cbly * v3 + calx * calz * sblx) +
                       cbcx * cbcz * (v3 * u2 + v4 * u1 + calx * calz * cblx * cblz) -
                       cbcx * sbcz * (v3 * u3 + v4 * u4 - calx * calz * cblx * sblz);
  acz = datan2(srzcrx / dcos(acx), crzcrx / dcos(acx));
}

// updateInitialGuess (:1999-2030), updateTransformation (:2036-2065),
// integrateTransformation (:2068-2104) and the scalar part of
// publishCloudsLast (:2166-2177): one workgroup
__global__ __launch_bounds__(kOdomThreads) void k_lego_odom_loop(OdomArgs a) {
  __shared__ float s_tc[6], s_AtA[9], s_AtB[3], s_P[9];
  __shared__ double s_part[kOdomSums * kOdomLanes];
  __shared__ int s_deg, s_keep;
  const int tid = threadIdx.x;
  slio_lego_odom_state& st = a.dev->st;
  slio_lego_odom_out& out = a.dev->out;
  if (tid == 0) {
    const LegoImuOutDev io = *a.io;
    st.imu_last[0] = io.rpy_cur[0];
    st.imu_last[1] = io.rpy_cur[1];
    st.imu_last[2] = io.rpy_cur[2];
    for (int k = 0; k < 3; ++k) st.imu_shift_from_start[k] = 0.0f;  // imuShiftFromStart*Cur is 0
    for (int k = 0; k < 3; ++k) st.imu_velo_from_start[k] = io.velo_from_start[k];
    for (int k = 0; k < 6; ++k) s_tc[k] = st.transform_cur[k];
    // imuAngularFromStart{X,Y,Z} = angular_from_start[0..2]
    if (io.angular_from_start[0] != 0 || io.angular_from_start[1] != 0 || io.angular_from_start[2] != 0) {
      s_tc[0] = -io.angular_from_start[1];
      s_tc[1] = -io.angular_from_start[2];
      s_tc[2] = -io.angular_from_start[0];
    }
    if (io.velo_from_start[0] != 0 || io.velo_from_start[1] != 0 || io.velo_from_start[2] != 0) {
      s_tc[3] -= io.velo_from_start[0] * a.scan_period;
      s_tc[4] -= io.velo_from_start[1] * a.scan_period;
      s_tc[5] -= io.velo_from_start[2] * a.scan_period;
    }
    s_deg = st.is_degenerate;
    for (int k = 0; k < 9; ++k) s_P[k] = st.mat_p[k];
    for (int k = 0; k < 2; ++k) out.iters[k] = out.rows[k] = out.degenerate[k] = 0;
  }
  __syncthreads();
  if (!(st.n_corner_last < 10 || st.n_surf_last < 100)) {
    for (int kind = kOdomSurf; kind <= kOdomCorner; ++kind) {
      for (int it = 0; it < a.max_iter; ++it) {
        const int nsel = odom_pass(a, kind, it, s_tc, s_AtA, s_AtB, s_part);
        if (tid == 0) {
          out.iters[kind] = it + 1;
          out.rows[kind] = nsel;
        }
        if (nsel < 10) continue;
        if (tid == 0) {
          s_keep = odom_step(kind, s_AtA, s_AtB, it, s_tc, &s_deg, s_P) ? 1 : 0;
          if (it == 0) out.degenerate[kind] = s_deg;
        }
        __syncthreads();
        if (!s_keep) break;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    float rx, ry, rz;
    float* ts = st.transform_sum;
    accumulate_rotation(ts[0], ts[1], ts[2], -s_tc[0], -s_tc[1], -s_tc[2], rx, ry, rz);
    const float* sh = st.imu_shift_from_start;
    const float x1 = dcos(rz) * (s_tc[3] - sh[0]) - dsin(rz) * (s_tc[4] - sh[1]);
    const float y1 = dsin(rz) * (s_tc[3] - sh[0]) + dcos(rz) * (s_tc[4] - sh[1]);
    const float z1 = s_tc[5] - sh[2];
    const float x2 = x1;
    const float y2 = dcos(rx) * y1 - dsin(rx) * z1;
    const float z2 = dsin(rx) * y1 + dcos(rx) * z1;
    const float tx = ts[3] - (dcos(ry) * x2 + dsin(ry) * z2);
    const float ty = ts[4] - y2;
    const float tz = ts[5] - (-dsin(ry) * x2 + dcos(ry) * z2);
    const LegoImuOutDev io = *a.io;
    // (imuPitchStart, imuYawStart, imuRollStart), (imuPitchLast, imuYawLast, imuRollLast)
    plugin_imu_rotation(rx, ry, rz, io.rpy_start[1], io.rpy_start[2], io.rpy_start[0], st.imu_last[1],
                        st.imu_last[2], st.imu_last[0], rx, ry, rz);
    ts[0] = rx;
    ts[1] = ry;
    ts[2] = rz;
    ts[3] = tx;
    ts[4] = ty;
    ts[5] = tz;
    for (int k = 0; k < 6; ++k) st.transform_cur[k] = s_tc[k];
    st.is_degenerate = s_deg;
    for (int k = 0; k < 9; ++k) st.mat_p[k] = s_P[k];
    // the scalar part of publishCloudsLast: the swapped clouds' sizes and the frame gate.
    // Stated departure: the reference re-seats its kd-trees only above 10 / 100 points
    // (:2169) and would search the previous sweep's trees at exactly 10 / 100; here the
    // search always runs on the new last clouds
    int64_t ncl = a.counts[1], nsl = a.counts[3];
    ncl = ncl < 0 ? 0 : (ncl > a.cap_corner ? a.cap_corner : ncl);
    nsl = nsl < 0 ? 0 : (nsl > a.cap_surf ? a.cap_surf : nsl);
    st.n_corner_last = (int32_t)ncl;
    st.n_surf_last = (int32_t)nsl;
    st.frame_count += 1;
    out.published = 0;
    if (st.frame_count >= a.skip + 1) {
      st.frame_count = 0;
      out.published = 1;
    }
    for (int k = 0; k < 6; ++k) {
      out.transform_cur[k] = s_tc[k];
      out.transform_sum[k] = ts[k];
    }
    out.inited = 1;
    out.n_corner_last = st.n_corner_last;
    out.n_surf_last = st.n_surf_last;
  }
}

// checkSystemInitialization (:1964-1997) without the swap, which the host does
__global__ void k_lego_odom_init(OdomArgs a) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  slio_lego_odom_state& st = a.dev->st;
  slio_lego_odom_out& out = a.dev->out;
  int64_t ncl = a.counts[1], nsl = a.counts[3];
  ncl = ncl < 0 ? 0 : (ncl > a.cap_corner ? a.cap_corner : ncl);
  nsl = nsl < 0 ? 0 : (nsl > a.cap_surf ? a.cap_surf : nsl);
  st.n_corner_last = (int32_t)ncl;
  st.n_surf_last = (int32_t)nsl;
  st.transform_sum[0] += a.io->rpy_start[1];  // imuPitchStart
  st.transform_sum[2] += a.io->rpy_start[0];  // imuRollStart
  st.system_inited = 1;
  const int32_t nol = out.n_outlier_last;
  out = slio_lego_odom_out{};
  for (int k = 0; k < 6; ++k) {
    out.transform_cur[k] = st.transform_cur[k];
    out.transform_sum[k] = st.transform_sum[k];
  }
  out.n_corner_last = st.n_corner_last;
  out.n_surf_last = st.n_surf_last;
  out.n_outlier_last = nol;
}

// TransformToEnd (:1073-1141), in place
__device__ float4 to_end(const float4 pi, const float* tc, const float* st_sc, const float* sh, const float* last) {
  const float4 p3 = to_start(pi, tc);
  const float rx = tc[0], ry = tc[1], rz = tc[2], tx = tc[3], ty = tc[4], tz = tc[5];
  const float x4 = dcos(ry) * p3.x + dsin(ry) * p3.z;
  const float y4 = p3.y;
  const float z4 = -dsin(ry) * p3.x + dcos(ry) * p3.z;
  const float x5 = x4;
  const float y5 = dcos(rx) * y4 - dsin(rx) * z4;
  const float z5 = dsin(rx) * y4 + dcos(rx) * z4;
  const float x6 = dcos(rz) * x5 - dsin(rz) * y5 + tx;
  const float y6 = dsin(rz) * x5 + dcos(rz) * y5 + ty;
  const float z6 = z5 + tz;
  // st_sc: cos / sin of imuRollStart, imuPitchStart, imuYawStart
  const float cR = st_sc[0], sR = st_sc[1], cP = st_sc[2], sP = st_sc[3], cY = st_sc[4], sY = st_sc[5];
  const float x7 = cR * (x6 - sh[0]) - sR * (y6 - sh[1]);
  const float y7 = sR * (x6 - sh[0]) + cR * (y6 - sh[1]);
  const float z7 = z6 - sh[2];
  const float x8 = x7;
  const float y8 = cP * y7 - sP * z7;
  const float z8 = sP * y7 + cP * z7;
  const float x9 = cY * x8 + sY * z8;
  const float y9 = y8;
  const float z9 = -sY * x8 + cY * z8;
  // last: imuRollLast, imuPitchLast, imuYawLast
  const float x10 = dcos(last[2]) * x9 - dsin(last[2]) * z9;
  const float y10 = y9;
  const float z10 = dsin(last[2]) * x9 + dcos(last[2]) * z9;
  const float x11 = x10;
  const float y11 = dcos(last[1]) * y10 + dsin(last[1]) * z10;
  const float z11 = -dsin(last[1]) * y10 + dcos(last[1]) * z10;
  return make_float4(dcos(last[0]) * x11 + dsin(last[0]) * y11, -dsin(last[0]) * x11 + dcos(last[0]) * y11, z11,
                     (float)(int)pi.w);
}

// publishCloudsLast's point work (:2145-2156, :2180): TransformToEnd over the
// two less clouds in place and, when the frame gate opened, adjustOutlierCloud
// into the published outlier buffer.  Runs after k_lego_odom_loop.
__global__ __launch_bounds__(256) void k_lego_odom_publish(OdomArgs a, float4* less_sharp, float4* less_flat,
                                                           const float4* outlier, const int32_t* nseg,
                                                           float4* outlier_last, int64_t cap_outlier) {
  __shared__ float s_tc[6], s_sc[6], s_sh[3], s_last[3];
  if (threadIdx.x == 0) {
    const slio_lego_odom_state& st = a.dev->st;
    for (int k = 0; k < 6; ++k) s_tc[k] = st.transform_cur[k];
    for (int k = 0; k < 3; ++k) {
      s_sc[2 * k] = dcos(a.io->rpy_start[k]);
      s_sc[2 * k + 1] = dsin(a.io->rpy_start[k]);
      s_sh[k] = st.imu_shift_from_start[k];
      s_last[k] = st.imu_last[k];
    }
  }
  __syncthreads();
  const int64_t ncl = a.dev->st.n_corner_last, nsl = a.dev->st.n_surf_last;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x, t0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < ncl; i += stride) less_sharp[i] = to_end(less_sharp[i], s_tc, s_sc, s_sh, s_last);
  for (int64_t i = t0; i < nsl; i += stride) less_flat[i] = to_end(less_flat[i], s_tc, s_sc, s_sh, s_last);
  if (a.dev->out.published) {
    int64_t no = nseg ? nseg[1] : 0;  // null: injected clouds, no sweep's outlier cloud
    no = no < 0 ? 0 : (no > cap_outlier ? cap_outlier : no);
    for (int64_t i = t0; i < no; i += stride) {
      const float4 p = outlier[i];
      outlier_last[i] = make_float4(p.y, p.z, p.x, p.w);
    }
  }
}

// after k_lego_odom_publish (which reads out.published while other blocks run)
__global__ void k_lego_odom_outlier_count(OdomArgs a, const int32_t* nseg, int64_t cap_outlier) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (a.dev->out.published) {
    int64_t no = nseg ? nseg[1] : 0;  // null: injected clouds, no sweep's outlier cloud
    no = no < 0 ? 0 : (no > cap_outlier ? cap_outlier : no);
    a.dev->out.n_outlier_last = (int32_t)no;
  }
}

// the lockstep entry: one pass at a given transform
__global__ __launch_bounds__(kOdomThreads) void k_lego_odom_pass(OdomArgs a, int kind, int iter, Tc6 tc) {
  __shared__ float s_tc[6], s_AtA[9], s_AtB[3];
  __shared__ double s_part[kOdomSums * kOdomLanes];
  if (threadIdx.x < 6) s_tc[threadIdx.x] = tc.v[threadIdx.x];
  __syncthreads();
  const int nsel = odom_pass(a, kind, iter, s_tc, s_AtA, s_AtB, s_part);
  if (threadIdx.x < 9) a.dev->pass_AtA[threadIdx.x] = s_AtA[threadIdx.x];
  if (threadIdx.x < 3) a.dev->pass_AtB[threadIdx.x] = s_AtB[threadIdx.x];
  if (threadIdx.x == 0) a.dev->pass_nsel = nsel;
}

struct LegoOdom {
  slio_lego_odom_params prm{};
  float4 *corner_last = nullptr, *surf_last = nullptr, *outlier_last = nullptr;
  float4 *psel = nullptr, *coeff = nullptr, *rows = nullptr;
  int32_t* ind = nullptr;
  uint8_t* sel = nullptr;
  OdomDev* dev = nullptr;
  int cap_q = 0;
  bool inited = false;    // host mirror of systemInitedLM
  bool injected = false;  // slio_lego_odom_set_clouds stands in for a sweep
};

void lego_odom_free(LegoOdom* o) {
  if (!o) return;
  void* dev[] = {o->corner_last, o->surf_last, o->outlier_last, o->psel, o->coeff, o->rows, o->ind, o->sel, o->dev};
  for (void* p : dev)
    if (p) (void)hipFree(p);
  delete o;
}

namespace {

OdomArgs make_args(const LegoOdomView& v, const LegoOdom* o) {
  OdomArgs a{};
  a.sharp = v.c_sharp;
  a.flat = v.c_flat;
  a.corner_last = o->corner_last;
  a.surf_last = o->surf_last;
  a.counts = v.counts;
  a.psel = o->psel;
  a.ind = o->ind;
  a.coeff = o->coeff;
  a.rows = o->rows;
  a.sel = o->sel;
  a.dev = o->dev;
  a.io = v.io;
  a.gate = o->prm.nearest_feature_sq_dist;
  a.scan_period = o->prm.scan_period;
  a.max_iter = o->prm.max_iterations;
  a.period = o->prm.search_period;
  a.skip = o->prm.skip_frame_num;
  a.cap_q = o->cap_q;
  a.cap_flat = (int)v.cap_flat;
  a.cap_corner = v.cap_corner;
  a.cap_surf = v.cap_surf;
  return a;
}

int odom_clear(const LegoOdomView& v, LegoOdom* o) {
  // the constructor's state (:318-354): everything 0 / false but frameCount = skipFrameNum,
  // so that the first sweep after checkSystemInitialization publishes
  OdomDev init{};
  init.st.frame_count = o->prm.skip_frame_num;
  ODOM_HIP(hipMemcpyAsync(o->dev, &init, sizeof(OdomDev), hipMemcpyHostToDevice, v.stream));
  if (!*v.ran) ODOM_HIP(hipMemsetAsync(v.counts, 0, 4 * sizeof(int64_t), v.stream));  // no sweep yet: no features
  ODOM_HIP(hipMemsetAsync(o->ind, 0xff, sizeof(int32_t) * 6 * (size_t)o->cap_q, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  o->inited = false;
  o->injected = false;
  return SLIO_OK;
}

}  // namespace

}  // namespace lego
}  // namespace slio

using namespace slio::lego;
using slio::set_error;

#define ODOM_CHECK(h, v, o, what)                                   \
  LegoOdomView v;                                                   \
  if (!(h)) {                                                       \
    set_error("null slio_lego handle");                             \
    return SLIO_EINVAL;                                             \
  }                                                                 \
  lego_odom_view((h), &v);                                          \
  ODOM_HIP(hipSetDevice(v.device));                                 \
  LegoOdom* o = *v.odom;                                            \
  if (!o) {                                                         \
    set_error(what ": odometry not enabled (slio_lego_odom_enable)"); \
    return SLIO_ESTATE;                                             \
  }

extern "C" {

int slio_lego_odom_params_default(slio_lego_odom_params* p) {
  if (!p) {
    set_error("slio_lego_odom_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->nearest_feature_sq_dist = 25.0f;
  p->max_iterations = 25;
  p->search_period = 5;
  p->skip_frame_num = 1;
  p->scan_period = 0.1f;
  return SLIO_OK;
}

int slio_lego_odom_enable(slio_lego_handle h, const slio_lego_odom_params* p) {
  if (!h || !p) {
    set_error("slio_lego_odom_enable: null argument");
    return SLIO_EINVAL;
  }
  if (!(p->nearest_feature_sq_dist > 0.0f) || p->max_iterations < 1 || p->max_iterations > kOdomMaxIter ||
      p->search_period < 1 || p->skip_frame_num < 0 || !(p->scan_period > 0.0f)) {
    set_error("slio_lego_odom_enable: bad gate / max_iterations (1..64) / search_period / skip_frame_num / scan_period");
    return SLIO_EINVAL;
  }
  LegoOdomView v;
  lego_odom_view(h, &v);
  ODOM_HIP(hipSetDevice(v.device));
  if (*v.odom) {
    (*v.odom)->prm = *p;
    return odom_clear(v, *v.odom);
  }
  auto* o = new LegoOdom();
  o->prm = *p;
  o->cap_q = (int)(v.cap_corner > v.cap_flat ? v.cap_corner : v.cap_flat);
  hipError_t e = hipSuccess;
#define A(ptr, bytes) \
  if (!e) e = hipMalloc(reinterpret_cast<void**>(&(ptr)), (bytes))
  A(o->corner_last, 16 * v.cap_corner);
  A(o->surf_last, 16 * v.cap_surf);
  A(o->outlier_last, 16 * v.cap_surf);
  A(o->psel, 16 * (size_t)o->cap_q);
  A(o->coeff, 16 * (size_t)o->cap_q);
  A(o->rows, 16 * (size_t)o->cap_q);
  A(o->ind, 24 * (size_t)o->cap_q);
  A(o->sel, (size_t)o->cap_q);
  A(o->dev, sizeof(OdomDev));
#undef A
  if (e) {
    set_error(std::string("slio_lego_odom_enable: ") + hipGetErrorString(e));
    lego_odom_free(o);
    return SLIO_ENOMEM;
  }
  const int rc = odom_clear(v, o);
  if (rc) {
    lego_odom_free(o);
    return rc;
  }
  *v.odom = o;
  return SLIO_OK;
}

int slio_lego_odom_reset(slio_lego_handle h) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_reset");
  *v.odom_fresh = false;
  return odom_clear(v, o);
}

int slio_lego_odom_run_async(slio_lego_handle h) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_run_async");
  if (!*v.odom_fresh || !(*v.ran || o->injected)) {
    set_error("slio_lego_odom_run: no new sweep to run the odometry on");
    return SLIO_ESTATE;
  }
  const OdomArgs a = make_args(v, o);
  if (!o->inited) {
    k_lego_odom_init<<<1, 64, 0, v.stream>>>(a);
  } else {
    k_lego_odom_loop<<<1, kOdomThreads, 0, v.stream>>>(a);
    const int32_t* nseg = *v.ran ? v.nseg : nullptr;
    k_lego_odom_publish<<<64, 256, 0, v.stream>>>(a, *v.c_less_sharp, *v.c_less_flat, v.outlier, nseg,
                                                  o->outlier_last, v.cap_surf);
    k_lego_odom_outlier_count<<<1, 64, 0, v.stream>>>(a, nseg, v.cap_surf);
  }
  ODOM_HIP(hipGetLastError());
  // the pointer swap (:1966-1973 / :2158-2164)
  std::swap(*v.c_less_sharp, o->corner_last);
  std::swap(*v.c_less_flat, o->surf_last);
  o->inited = true;
  o->injected = false;
  *v.odom_fresh = false;
  return SLIO_OK;
}

int slio_lego_odom_run(slio_lego_handle h, slio_lego_odom_out* out) {
  const int rc = slio_lego_odom_run_async(h);
  if (rc) return rc;
  LegoOdomView v;
  lego_odom_view(h, &v);
  LegoOdom* o = *v.odom;
  slio_lego_odom_out r;
  ODOM_HIP(hipMemcpyAsync(&r, &o->dev->out, sizeof(r), hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  if (out) *out = r;
  return SLIO_OK;
}

int slio_lego_odom_get_last(slio_lego_handle h, float* corner_xyzi, float* surf_xyzi, float* outlier_xyzi) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_get_last");
  OdomDev d;
  ODOM_HIP(hipMemcpyAsync(&d, o->dev, sizeof(d), hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  const int64_t nc = d.st.n_corner_last, ns = d.st.n_surf_last, no = d.out.n_outlier_last;
  if (corner_xyzi && nc > 0)
    ODOM_HIP(hipMemcpyAsync(corner_xyzi, o->corner_last, 16 * nc, hipMemcpyDeviceToHost, v.stream));
  if (surf_xyzi && ns > 0)
    ODOM_HIP(hipMemcpyAsync(surf_xyzi, o->surf_last, 16 * ns, hipMemcpyDeviceToHost, v.stream));
  if (outlier_xyzi && no > 0)
    ODOM_HIP(hipMemcpyAsync(outlier_xyzi, o->outlier_last, 16 * no, hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  return SLIO_OK;
}

int slio_lego_odom_last_view(slio_lego_handle h, slio_lego_last_view* view) {
  if (!view) {
    set_error("slio_lego_odom_last_view: null");
    return SLIO_EINVAL;
  }
  ODOM_CHECK(h, v, o, "slio_lego_odom_last_view");
  slio_lego_odom_out r;
  ODOM_HIP(hipMemcpyAsync(&r, &o->dev->out, sizeof(r), hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  std::memset(view, 0, sizeof(*view));
  view->corner_xyzi = reinterpret_cast<const float*>(o->corner_last);
  view->surf_xyzi = reinterpret_cast<const float*>(o->surf_last);
  view->outlier_xyzi = reinterpret_cast<const float*>(o->outlier_last);
  view->n_corner = r.n_corner_last;
  view->n_surf = r.n_surf_last;
  view->n_outlier = r.n_outlier_last;
  view->published = o->inited ? r.published : 0;
  view->device = v.device;
  return SLIO_OK;
}

int slio_lego_odom_get_state(slio_lego_handle h, slio_lego_odom_state* s) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_get_state");
  if (!s) {
    set_error("slio_lego_odom_get_state: null");
    return SLIO_EINVAL;
  }
  ODOM_HIP(hipMemcpyAsync(s, &o->dev->st, sizeof(*s), hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  return SLIO_OK;
}

int slio_lego_odom_set_state(slio_lego_handle h, const slio_lego_odom_state* s) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_set_state");
  if (!s || s->n_corner_last < 0 || s->n_corner_last > v.cap_corner || s->n_surf_last < 0 ||
      s->n_surf_last > v.cap_surf || s->frame_count < 0) {
    set_error("slio_lego_odom_set_state: null or sizes out of range");
    return SLIO_EINVAL;
  }
  ODOM_HIP(hipMemcpyAsync(&o->dev->st, s, sizeof(*s), hipMemcpyHostToDevice, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  o->inited = s->system_inited != 0;
  return SLIO_OK;
}

int slio_lego_odom_set_clouds(slio_lego_handle h, const float* sharp, int32_t n_sharp, const float* flat,
                              int32_t n_flat, const float* corner_last, int32_t n_corner_last,
                              const float* surf_last, int32_t n_surf_last) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_set_clouds");
  if (n_sharp < 0 || n_flat < 0 || n_corner_last < 0 || n_surf_last < 0 || (n_sharp && !sharp) ||
      (n_flat && !flat) || (n_corner_last && !corner_last) || (n_surf_last && !surf_last)) {
    set_error("slio_lego_odom_set_clouds: bad arguments");
    return SLIO_EINVAL;
  }
  if (n_sharp > v.cap_corner || n_flat > v.cap_flat || n_corner_last > v.cap_corner || n_surf_last > v.cap_surf) {
    set_error("slio_lego_odom_set_clouds: cloud exceeds the handle's capacity");
    return SLIO_ECAPACITY;
  }
  for (int c = 0; c < 2; ++c) {
    const float* p = c ? surf_last : corner_last;
    const int n = c ? n_surf_last : n_corner_last;
    for (int i = 0; i < n; ++i) {
      const float w = p[4 * i + 3];
      if (!(w >= 0.0f && w < 65536.0f) || (i > 0 && (int)w < (int)p[4 * i - 1])) {
        set_error("slio_lego_odom_set_clouds: int(intensity) of a last cloud must be in [0, 65536) and not decrease");
        return SLIO_EINVAL;
      }
    }
  }
  slio_lego_odom_state st;
  ODOM_HIP(hipMemcpyAsync(&st, &o->dev->st, sizeof(st), hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  st.n_corner_last = n_corner_last;
  st.n_surf_last = n_surf_last;
  st.system_inited = 1;
  const int64_t counts[4] = {n_sharp, 0, n_flat, 0};
  if (n_sharp) ODOM_HIP(hipMemcpyAsync(v.c_sharp, sharp, 16 * (size_t)n_sharp, hipMemcpyHostToDevice, v.stream));
  if (n_flat) ODOM_HIP(hipMemcpyAsync(v.c_flat, flat, 16 * (size_t)n_flat, hipMemcpyHostToDevice, v.stream));
  if (n_corner_last)
    ODOM_HIP(hipMemcpyAsync(o->corner_last, corner_last, 16 * (size_t)n_corner_last, hipMemcpyHostToDevice, v.stream));
  if (n_surf_last)
    ODOM_HIP(hipMemcpyAsync(o->surf_last, surf_last, 16 * (size_t)n_surf_last, hipMemcpyHostToDevice, v.stream));
  ODOM_HIP(hipMemcpyAsync(v.counts, counts, sizeof(counts), hipMemcpyHostToDevice, v.stream));
  ODOM_HIP(hipMemcpyAsync(&o->dev->st, &st, sizeof(st), hipMemcpyHostToDevice, v.stream));
  ODOM_HIP(hipMemsetAsync(o->ind, 0xff, sizeof(int32_t) * 6 * (size_t)o->cap_q, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  o->inited = true;
  o->injected = true;
  *v.ran = false;  // the front-end's sweep is replaced
  *v.odom_fresh = true;
  return SLIO_OK;
}

int slio_lego_odom_pass(slio_lego_handle h, int kind, int iter_count, const float transform_cur[6], int32_t* ind,
                        float* coeff, uint8_t* sel, float AtA[9], float AtB[3], int32_t* nsel) {
  ODOM_CHECK(h, v, o, "slio_lego_odom_pass");
  if ((kind != SLIO_LEGO_ODOM_SURF && kind != SLIO_LEGO_ODOM_CORNER) || iter_count < 0 || !transform_cur) {
    set_error("slio_lego_odom_pass: bad kind / iter_count / transform");
    return SLIO_EINVAL;
  }
  if (!(*v.ran || o->injected || o->inited)) {
    set_error("slio_lego_odom_pass: no clouds");
    return SLIO_ESTATE;
  }
  int64_t counts[4];
  ODOM_HIP(hipMemcpyAsync(counts, v.counts, sizeof(counts), hipMemcpyDeviceToHost, v.stream));
  ODOM_HIP(hipStreamSynchronize(v.stream));
  int64_t n = counts[kind == SLIO_LEGO_ODOM_CORNER ? 0 : 2];
  const int64_t cap = kind == SLIO_LEGO_ODOM_CORNER ? o->cap_q : v.cap_flat;
  n = n < 0 ? 0 : (n > cap ? cap : n);
  Tc6 tc;
  for (int k = 0; k < 6; ++k) tc.v[k] = transform_cur[k];
  k_lego_odom_pass<<<1, kOdomThreads, 0, v.stream>>>(make_args(v, o), kind, iter_count, tc);
  ODOM_HIP(hipGetLastError());
  OdomDev d;
  ODOM_HIP(hipMemcpyAsync(&d, o->dev, sizeof(d), hipMemcpyDeviceToHost, v.stream));
  if (n > 0) {
    if (ind)
      for (int k = 0; k < 3; ++k)
        ODOM_HIP(hipMemcpyAsync(ind + k * n, o->ind + ((size_t)kind * 3 + k) * o->cap_q, 4 * n, hipMemcpyDeviceToHost, v.stream));
    if (coeff) ODOM_HIP(hipMemcpyAsync(coeff, o->coeff, 16 * n, hipMemcpyDeviceToHost, v.stream));
    if (sel) ODOM_HIP(hipMemcpyAsync(sel, o->sel, n, hipMemcpyDeviceToHost, v.stream));
  }
  ODOM_HIP(hipStreamSynchronize(v.stream));
  if (AtA) std::memcpy(AtA, d.pass_AtA, sizeof(d.pass_AtA));
  if (AtB) std::memcpy(AtB, d.pass_AtB, sizeof(d.pass_AtB));
  if (nsel) *nsel = d.pass_nsel;
  return SLIO_OK;
}

}  // extern "C"
