// slio_llreg.hip -- LIO-Livox's ScanRegistration for Use_seg = 0 on the device
// (src/LIO-Livox/src/lio/LidarFeatureExtractor.cpp: FeatureExtract :1218-1291,
// FeatureExtract_Mid :1352-1401, detectFeaturePoint :93-614; ScanRegistration.cpp
// lidarCallBackPc2 :61-93).  The formulas are slio_llreg.hpp's, shared with the
// host restatement (slio_llreg.cpp).  One message is nine launches, whatever n,
// and one host wait (the counts):
//
//   k_llreg_count    per block of 256 inputs and per line: kept points, and
//                    the finite ones among them
//   k_llreg_ingest   the three stable compactions (a block's threads share the
//                    sum of the counts of the blocks before it): the cloud, vlines[l] as cloud
//                    indices, the lines' finite points; writes the sizes
//   k_llreg_feature  per finite point: depth, curvature, diffR and the bits of
//                    attr (slio_llreg.hpp), which hold everything the picking
//                    and the chain ask of a point
//   k_llreg_rank     per point of a part: its place in the part's two stable
//                    sorts, by counting; cloudSortInd and reflectSortInd
//   k_llreg_pick     ONE wavefront per line: the parts in order
//   k_llreg_chain    one workgroup per line: the visited set of the
//                    line-feature loop, a scan of 4-state entry maps
//   k_llreg_flags    150 on the visited positions, the break-point loop, the
//                    collection, the labels on the cloud
//   k_llreg_tally    corner and surf labels per block of 256 cloud points
//   k_llreg_collect  the two stable compactions; writes the two counts
//
// No kernel holds a grid barrier and no workgroup waits for another.
//
// The sorts.  The reference's insertion sort swaps neighbours on a strict `<`,
// so it is a stable ascending sort, and the place of point i is the number of
// points of its part that are smaller, or equal and earlier, with NaN as one
// class after every number (sort_before, slio_llreg.hpp), so that the places
// are a permutation of the part whatever the values.  That needs no flag, so
// every part of every line is ranked at once.
//
// The picking.  A part's loops read and write CloudFeatureFlag within three
// positions of the part, and the part before it has written there, so the
// parts of a line run in the serial order, on one wavefront, with the line's
// flags in LDS.  Within a part of up to kPickFast points lane q holds position
// sp - 3 + q and the state is five 64-bit masks (flag 1 / 2 / 3 / 300 and the
// points' attr bits), uniform over the wavefront: the k-th step of the flag
// loop finds the lane whose curvature rank is k with one ballot, tests its
// bits, and the lanes that a neighbour mark reaches answer a second ballot
// (lane q is reached from p when |p - q| is within q's own gap-free run
// towards p, the same pairs that the reference walks from p).  The pick loop
// is the same walk with the two counters.  The masks are then written back to
// LDS, so the next part starts from exactly the flags the serial code would
// see: the marks this part left on its first positions (it skips them), and
// the marks this part left on the previous part's last positions, which
// overwrite its 2 / 3 / 300 there in LDS as the serial store does.  Nothing is
// reordered: within a part the steps run in rank order, and the parts in part
// order.  A longer part runs pick_part (the host's code) on lane 0 over the
// same LDS flags.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include "slio_device.hpp"
#include "slio_frontend.h"
#include "slio_llreg.hpp"

using slio::set_error;
using namespace slio::llreg;

namespace {

constexpr int kWaves = kBlk / 64;
// meta: the sizes the kernels hand on, and the host reads after its one wait
enum { kNCloud = 0, kNCorner, kNSurf, kErr, kVSize, kFSize = kVSize + kMaxScans, kMeta = kFSize + kMaxScans };

struct Input {
  const float* xyz;         // n x 3 (CustomMsg) or n x 4 (Pc2)
  const uint32_t* offset;   // CustomMsg only
  const uint8_t* refl;
  const uint8_t* line;
  int n, pc2;
  double time_span;
};

struct Point8 {
  float4 a, b;
};

// the rank of this thread among the threads before it in the block whose pred
// is set and whose key (0 .. kMaxScans - 1) is the same; tot[k] = the block's
// count of key k
__device__ __forceinline__ int keyed_rank(bool pred, int key, int* tot) {
  __shared__ int ws[kWaves][kMaxScans];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int r = 0;
#pragma unroll
  for (int k = 0; k < kMaxScans; ++k) {
    const unsigned long long b = __ballot(pred && key == k);
    if (key == k) r = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) ws[w][k] = __popcll(b);
  }
  __syncthreads();
  int base = 0;
  for (int v = 0; v < w; ++v) base += ws[v][pred ? key : 0];
  if (threadIdx.x < kMaxScans) {
    int t = 0;
    for (int v = 0; v < kWaves; ++v) t += ws[v][threadIdx.x];
    tot[threadIdx.x] = t;
  }
  __syncthreads();  // (ws is free for the next call, tot is written)
  return base + r;
}

struct Kept {
  float x, y, z, w;
  int line;
  bool kept, finite;
};

__device__ __forceinline__ Kept read_input(const Input& in, int i, const Params& P) {
  Kept k{0.f, 0.f, 0.f, 0.f, 0, false, false};
  if (i >= in.n) return k;
  if (in.pc2) {
    const float4 p = ((const float4*)in.xyz)[i];
    k.x = p.x, k.y = p.y, k.z = p.z, k.w = p.w;
    k.line = i % 4;
    k.kept = x_kept(k.x, P.lidar_type);
  } else {
    k.x = in.xyz[3 * i], k.y = in.xyz[3 * i + 1], k.z = in.xyz[3 * i + 2];
    k.w = (float)in.refl[i];
    k.line = (int)in.line[i];
    k.kept = k.line <= P.n_scans - 1 && x_kept(k.x, P.lidar_type);
  }
  if (!k.kept) k.line = 0;
  k.finite = k.kept && finite_xyz(k.x, k.y, k.z);
  return k;
}

// cnt: per block, kMaxScans kept counts then kMaxScans finite counts
__global__ void __launch_bounds__(kBlk) k_llreg_count(Input in, Params P, int* __restrict__ cnt) {
  __shared__ int tk[kMaxScans], tf[kMaxScans];
  const Kept k = read_input(in, blockIdx.x * kBlk + threadIdx.x, P);
  (void)keyed_rank(k.kept, k.line, tk);
  (void)keyed_rank(k.finite, k.line, tf);
  if (threadIdx.x < kMaxScans) {
    cnt[blockIdx.x * 2 * kMaxScans + threadIdx.x] = tk[threadIdx.x];
    cnt[blockIdx.x * 2 * kMaxScans + kMaxScans + threadIdx.x] = tf[threadIdx.x];
  }
}

__global__ void __launch_bounds__(kBlk)
k_llreg_ingest(Input in, Params P, const int* __restrict__ cnt, Point8* __restrict__ cloud, int* __restrict__ vl_cloud,
               float4* __restrict__ fin, int* __restrict__ meta) {
  __shared__ int tk[kMaxScans], tf[kMaxScans], before[2 * kMaxScans], total[2 * kMaxScans];
  const int i = blockIdx.x * kBlk + threadIdx.x;
  const Kept k = read_input(in, i, P);
  const int vr = keyed_rank(k.kept, k.line, tk);
  const int fr = keyed_rank(k.finite, k.line, tf);
  // the counts of the blocks before this one, and of all blocks: the block's threads share the
  // blocks between them and add up in LDS (integer sums: the order does not matter)
  if (threadIdx.x < 2 * kMaxScans) before[threadIdx.x] = total[threadIdx.x] = 0;
  __syncthreads();
  for (int g = threadIdx.x; g < (int)gridDim.x; g += kBlk)
    for (int q = 0; q < 2 * kMaxScans; ++q) {
      const int v = cnt[g * 2 * kMaxScans + q];
      if (!v) continue;
      if (g < (int)blockIdx.x) atomicAdd(&before[q], v);
      atomicAdd(&total[q], v);
    }
  __syncthreads();
  // the cloud keeps the message's order over all lines: the kept points of the
  // blocks before, then the kept threads before this one
  int cbase = 0, voff = 0, foff = 0, ncloud = 0;
  bool over = false;
  for (int l = 0; l < kMaxScans; ++l) {
    cbase += before[l];
    ncloud += total[l];
    if (l < k.line) voff += total[l], foff += total[kMaxScans + l];
    over |= total[l] > kMaxLine;
  }
  int any;
  {
    __shared__ int wa[kWaves];
    const unsigned long long b = __ballot(k.kept);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) wa[w] = __popcll(b);
    __syncthreads();
    any = __popcll(b & ((1ull << lane) - 1ull));
    for (int v = 0; v < w; ++v) any += wa[v];
  }
  if (k.kept) {
    // every index below is less than the number of kept inputs <= n <= max_points
    const int ci = cbase + any;
    float nx, ny;
    if (in.pc2) {
      nx = (float)i / (float)in.n;
      ny = (float)k.line;
    } else {
      nx = (float)(to_sec(in.offset[i]) / in.time_span);
      ny = __int_as_float(k.line);
    }
    Point8 q;
    q.a = make_float4(k.x, k.y, k.z, k.w);
    q.b = make_float4(nx, ny, 0.f, 0.f);
    cloud[ci] = q;
    vl_cloud[voff + before[k.line] + vr] = ci;
    if (k.finite) fin[foff + before[kMaxScans + k.line] + fr] = q.a;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    meta[kNCloud] = ncloud;
    meta[kNCorner] = 0;
    meta[kNSurf] = 0;
    meta[kErr] = over ? 1 : 0;
    for (int l = 0; l < kMaxScans; ++l) {
      meta[kVSize + l] = total[l];
      meta[kFSize + l] = total[kMaxScans + l];
    }
  }
}

// the line of the g-th finite point and its index there; false past the last
struct Where {
  int line, idx, m, off, voff;
};
__device__ __forceinline__ bool locate(const int* __restrict__ meta, int g, Where* w) {
  int off = 0, voff = 0;
  for (int l = 0; l < kMaxScans; ++l) {
    const int m = meta[kFSize + l];
    if (g < off + m) {
      *w = Where{l, g - off, m, off, voff};
      return true;
    }
    off += m;
    voff += meta[kVSize + l];
  }
  return false;
}

__global__ void __launch_bounds__(kBlk)
k_llreg_feature(const float* __restrict__ fin, const int* __restrict__ meta, Params P, float* __restrict__ curv,
                float* __restrict__ depth, float* __restrict__ refl, uint16_t* __restrict__ attr,
                uint8_t* __restrict__ vis) {
  const int g = blockIdx.x * kBlk + threadIdx.x;
  Where w;
  if (meta[kErr] || !locate(meta, g, &w)) return;
  const float* c = fin + 4 * (size_t)w.off;
  Feature f{0.f, 0.f, 0.f, 0u};
  // a loop position lies in [5, m - 5): every index its formulas read is inside the line
  if (w.idx >= 5 && w.idx < w.m - 5) f = point_feature(c, w.idx, P);
  f.attr |= reach_bits(c, w.idx, w.m);
  curv[g] = f.curv;
  depth[g] = f.depth;
  refl[g] = f.refl;
  attr[g] = (uint16_t)f.attr;
  vis[g] = 0;
}

__global__ void __launch_bounds__(kBlk)
k_llreg_rank(const int* __restrict__ meta, Params P, const float* __restrict__ curv, const float* __restrict__ refl,
             const uint16_t* __restrict__ attr, int* __restrict__ csort, int* __restrict__ rsort,
             uint32_t* __restrict__ word) {
  const int g = blockIdx.x * kBlk + threadIdx.x;
  Where w;
  if (meta[kErr] || !locate(meta, g, &w)) return;
  uint32_t wd = attr[g];
  const int i = w.idx;
  if (w.m >= 12 && i >= 5 && i < w.m - 6) {
    const int j = part_of(w.m, i, P.part_num);
    const int sp = part_sp(w.m, j, P.part_num), ep = part_ep(w.m, j, P.part_num);
    const float ci = curv[g], ri = refl[g];
    int rc = 0, rr = 0;
    for (int o = sp; o <= ep; ++o) {
      const float co = curv[w.off + o], ro = refl[w.off + o];
      rc += sorts_ahead(co, o, ci, i) ? 1 : 0;
      rr += sorts_ahead(ro, o, ri, i) ? 1 : 0;
    }
    // (sort_before is a strict weak order, NaN included: the places of a part are a permutation of it,
    // and both are below the part's length: sp + rank <= ep < m)
    csort[w.off + sp + rc] = i;
    rsort[w.off + sp + rr] = i;
    if (ep - sp + 1 <= kPickFast) wd |= (uint32_t)rc << kAttrBits | (uint32_t)rr << (kAttrBits + 6);
  }
  word[g] = wd;
}

__global__ void __launch_bounds__(kPickWindow)
k_llreg_pick(const float* __restrict__ fin, const int* __restrict__ meta, Params P, const float* __restrict__ curv,
             const float* __restrict__ depth, const float* __restrict__ refl, const uint16_t* __restrict__ attr,
             const uint32_t* __restrict__ word, const int* __restrict__ csort, const int* __restrict__ rsort,
             int* __restrict__ flags) {
  __shared__ uint16_t fl[kMaxLine];
  if (meta[kErr]) return;
  const int line = blockIdx.x, lane = threadIdx.x;
  int off = 0;
  for (int l = 0; l < line; ++l) off += meta[kFSize + l];
  const int m = meta[kFSize + line];  // <= vlines[line]'s size <= kMaxLine
  for (int i = lane; i < m; i += kPickWindow) fl[i] = 0;
  __syncthreads();
  if (m >= 12) {
    const int K = (attr[off + m - 6] & kK3) ? 3 : 2;  // the line's last loop position
    const int np = P.part_num;
    // the window's word of part j for this lane (0 outside it, or when the part takes the serial path)
    const auto load = [&](int j) -> uint32_t {
      if (j >= np) return 0u;
      const int sp = part_sp(m, j, np), len = part_ep(m, j, np) - sp + 1;
      return (len >= 1 && len <= kPickFast && lane < len + 6) ? word[off + sp - 3 + lane] : 0u;
    };
    uint32_t next = load(0);
    for (int j = 0; j < np; ++j) {
      const uint32_t wd = next;
      next = load(j + 1);
      const int sp = part_sp(m, j, np), ep = part_ep(m, j, np), len = ep - sp + 1;
      if (len < 1) continue;
      if (len > kPickFast) {
        if (lane == 0)
          pick_part(fin + 4 * (size_t)off, curv + off, depth + off, refl + off, attr + off, csort + off, rsort + off,
                    fl, sp, ep, K, P);
        __syncthreads();
        continue;
      }
      // sp - 3 >= 2 and ep + 3 <= m - 4: the window is inside the line
      const bool inwin = lane < len + 6, inpart = lane >= 3 && lane < 3 + len;
      const int pos = sp - 3 + lane;
      const int f0 = inwin ? (int)fl[pos] : 0;
      const int crank = (int)(wd >> kAttrBits) & 63, rrank = (int)(wd >> (kAttrBits + 6)) & 63;
      const int fwd = min((int)(wd >> kFwdShift) & 3, K), bwd = min((int)(wd >> kBwdShift) & 3, K);
      const unsigned long long CAND = __ballot(inpart && (wd & kCand)), FAR = __ballot(inpart && (wd & kFar));
      const unsigned long long ANG = __ballot(inpart && (wd & kAngle)), RC = __ballot(inpart && (wd & kRcand));
      unsigned long long F1 = __ballot(f0 == 1), F2 = __ballot(f0 == 2), F3 = __ballot(f0 == 3),
                         F300 = __ballot(f0 == 300);
      // the flag loop (:236-274)
      for (int k = 0; k < len; ++k) {
        const unsigned long long pm = __ballot(inpart && crank == k);
        if (((F1 | F2 | F3 | F300) & pm) || !(CAND & pm)) continue;
        F3 |= pm;
        if (FAR & pm) continue;
        const int p = __ffsll((long long)pm) - 1;
        const unsigned long long mark =
            __ballot(inwin && ((lane > p && lane - p <= bwd) || (lane < p && p - lane <= fwd)));
        F1 |= mark;
        F2 &= ~mark;
        F3 &= ~mark;
        F300 &= ~mark;
      }
      // the pick loop (:276-296)
      int picked = 1, sharp = 1;
      for (int k = 0; k < len; ++k) {
        const unsigned long long pm = __ballot(inpart && crank == k);
        if (((F3 & pm) && (picked <= P.num_flat || (FAR & pm))) || (ANG & pm)) {
          ++picked;
          F2 |= pm;
          F1 &= ~pm;
          F3 &= ~pm;
          F300 &= ~pm;
        }
        const unsigned long long rm = __ballot(inpart && rrank == k);
        if ((RC & rm) && sharp <= 3) {
          ++sharp;
          F300 |= rm;
          F1 &= ~rm;
          F2 &= ~rm;
          F3 &= ~rm;
        }
      }
      const unsigned long long me = 1ull << lane;
      if (inwin) fl[pos] = (uint16_t)((F300 & me) ? 300 : (F2 & me) ? 2 : (F3 & me) ? 3 : (F1 & me) ? 1 : 0);
      __syncthreads();
    }
  }
  for (int i = lane; i < m; i += kPickWindow) flags[off + i] = fl[i];
}

__device__ __forceinline__ int map_apply(uint32_t m, int e) { return (int)((m >> (2 * e)) & 3u); }
// first, then second
__device__ __forceinline__ uint32_t map_compose(uint32_t first, uint32_t second) {
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) m |= (uint32_t)map_apply(second, map_apply(first, e)) << (2 * e);
  return m;
}

// The line-feature loop is `for (i = 5; i < m - 5; i += count_num)` with
// count_num = 4 after a flat right side and 1 elsewhere (:301, :347-358), and
// nothing else survives an iteration: over a run of positions the chain is a
// map from the entry offset (0 .. 3) to the exit offset, the maps compose, and
// the chain is a scan, as in slio_lreg.hip.
__global__ void __launch_bounds__(kChainThreads)
k_llreg_chain(const int* __restrict__ meta, const uint16_t* __restrict__ attr, uint8_t* __restrict__ vis) {
  __shared__ uint8_t mp[2][kChainThreads];
  if (meta[kErr]) return;
  const int line = blockIdx.x, t = threadIdx.x;
  int off = 0;
  for (int l = 0; l < line; ++l) off += meta[kFSize + l];
  const int M = meta[kFSize + line] - 10;  // loop positions: i = 5 + q, q < M
  const int q0 = t * kChainPerThread;
  unsigned long long w0 = 0, w1 = 0;
  for (int pos = 0; pos < kChainPerThread && q0 + pos < M; ++pos)
    if (attr[off + 5 + q0 + pos] & kStride4) {
      if (pos < 64) w0 |= 1ull << pos;
      else w1 |= 1ull << (pos - 64);
    }
  auto step = [&](int pos) { return ((pos < 64 ? w0 >> pos : w1 >> (pos - 64)) & 1ull) ? 4 : 1; };
  uint32_t mm = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int pos = e;
    while (pos < kChainPerThread) pos += step(pos);
    mm |= (uint32_t)(pos - kChainPerThread) << (2 * e);
  }
  // inclusive scan under composition (Hillis-Steele, earlier runs first)
  int cur = 0;
  mp[0][t] = (uint8_t)mm;
  __syncthreads();
  for (int d = 1; d < kChainThreads; d <<= 1) {
    uint32_t v = mp[cur][t];
    if (t >= d) v = map_compose(mp[cur][t - d], v);
    mp[cur ^ 1][t] = (uint8_t)v;
    cur ^= 1;
    __syncthreads();
  }
  // the chain enters the first run at offset 0 (i = 5)
  const int entry = t == 0 ? 0 : map_apply(mp[cur][t - 1], 0);
  for (int pos = entry; pos < kChainPerThread && q0 + pos < M; pos += step(pos)) vis[off + 5 + q0 + pos] = 1;
}

__global__ void __launch_bounds__(kBlk)
k_llreg_flags(const float* __restrict__ fin, const int* __restrict__ meta, Params P, const uint8_t* __restrict__ vis,
              const int* __restrict__ vl_cloud, int* __restrict__ flags, Point8* __restrict__ cloud) {
  const int g = blockIdx.x * kBlk + threadIdx.x;
  Where w;
  if (meta[kErr] || !locate(meta, g, &w)) return;
  if (w.idx < 5 || w.idx >= w.m - 5) return;
  const float* c = fin + 4 * (size_t)w.off;
  int f = flags[g];
  if (vis[g] && line_corner(c, w.idx, P)) f = 150;
  f = break_point(c, w.idx, f, P);
  flags[g] = f;
  const int lab = label_of(c, w.idx, f, P);
  // :1273-1283: idx < m <= vlines[line]'s size, so the index is inside the line's list
  if (lab) cloud[vl_cloud[w.voff + w.idx]].b.z = (float)lab;
}

__device__ __forceinline__ int block_rank(bool pred, int* total) {
  __shared__ int wsum[kWaves];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(pred);
  const int r = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    if (k < w) base += wsum[k];
    tot += wsum[k];
  }
  __syncthreads();
  *total = tot;
  return base + r;
}

// :1285-1290: fabs(normal_z - 1.0) < 1e-5 on a label that is exactly 0, 1 or 2
__global__ void __launch_bounds__(kBlk)
k_llreg_tally(const Point8* __restrict__ cloud, const int* __restrict__ meta, int* __restrict__ cnt) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  const float lab = (!meta[kErr] && i < meta[kNCloud]) ? cloud[i].b.z : 0.f;
  int tc, ts;
  (void)block_rank(lab == 1.0f, &tc);
  (void)block_rank(lab == 2.0f, &ts);
  if (threadIdx.x == 0) {
    cnt[2 * blockIdx.x] = tc;
    cnt[2 * blockIdx.x + 1] = ts;
  }
}

__global__ void __launch_bounds__(kBlk)
k_llreg_collect(const Point8* __restrict__ cloud, int* __restrict__ meta, const int* __restrict__ cnt,
                Point8* __restrict__ corner, Point8* __restrict__ surf) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  Point8 q{};
  if (!meta[kErr] && i < meta[kNCloud]) q = cloud[i];
  const bool isc = q.b.z == 1.0f, iss = q.b.z == 2.0f;
  int tc, ts;
  const int rc = block_rank(isc, &tc), rs = block_rank(iss, &ts);
  // the labels of the blocks before this one, summed as in k_llreg_ingest
  __shared__ int sum[2];
  if (threadIdx.x < 2) sum[threadIdx.x] = 0;
  __syncthreads();
  for (int b = threadIdx.x; b < (int)blockIdx.x; b += kBlk) {
    if (cnt[2 * b]) atomicAdd(&sum[0], cnt[2 * b]);
    if (cnt[2 * b + 1]) atomicAdd(&sum[1], cnt[2 * b + 1]);
  }
  __syncthreads();
  const int bc = sum[0], bs = sum[1];
  // (both totals are at most the cloud's size <= max_points, the clouds' capacity)
  if (isc) corner[bc + rc] = q;
  if (iss) surf[bs + rs] = q;
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    meta[kNCorner] = bc + tc;
    meta[kNSurf] = bs + ts;
  }
}

std::mutex g_live_mu;
std::set<void*> g_live;

}  // namespace

struct slio_llreg {
  slio_llreg_params prm{};
  Params P{};
  bool dev_counted = false;
  hipStream_t stream = nullptr;
  uint8_t* in = nullptr;  // the staged message
  Point8 *cloud = nullptr, *corner = nullptr, *surf = nullptr;
  float4* fin = nullptr;
  float *curv = nullptr, *depth = nullptr, *refl = nullptr;
  uint16_t* attr = nullptr;
  uint32_t* word = nullptr;
  uint8_t* vis = nullptr;
  int *vl_cloud = nullptr, *csort = nullptr, *rsort = nullptr, *flags = nullptr, *cnt = nullptr, *meta = nullptr;
  uint8_t* h_in = nullptr;  // pinned staging of the input
  int* h_meta = nullptr;
  int32_t meta_host[kMeta] = {0};
  bool has_run = false;
};

namespace {

void llreg_free(slio_llreg* h) {
  for (void* p : {(void*)h->in, (void*)h->cloud, (void*)h->corner, (void*)h->surf, (void*)h->fin, (void*)h->curv,
                  (void*)h->depth, (void*)h->refl, (void*)h->attr, (void*)h->word, (void*)h->vis, (void*)h->vl_cloud,
                  (void*)h->csort, (void*)h->rsort, (void*)h->flags, (void*)h->cnt, (void*)h->meta})
    if (p) (void)hipFree(p);
  if (h->h_in) (void)hipHostFree(h->h_in);
  if (h->h_meta) (void)hipHostFree(h->h_meta);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

bool is_live(void* h) {
  std::lock_guard<std::mutex> g(g_live_mu);
  return g_live.count(h) != 0;
}

// the nine launches and the one wait; in.n > 0 points are staged in h->h_in
int run(slio_llreg* h, Input in, size_t bytes, int32_t counts[3], const char* who) {
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t st = h->stream;
  h->has_run = false;
  if (in.n == 0) {  // (:1238 would call back() on an empty vector)
    std::memset(h->meta_host, 0, sizeof h->meta_host);
    counts[0] = counts[1] = counts[2] = 0;
    h->has_run = true;
    return SLIO_OK;
  }
  SLIO_HIP(hipMemcpyAsync(h->in, h->h_in, bytes, hipMemcpyHostToDevice, st));
  const int nb = (in.n + kBlk - 1) / kBlk;
  const float* c = (const float*)h->fin;
  k_llreg_count<<<nb, kBlk, 0, st>>>(in, h->P, h->cnt);
  k_llreg_ingest<<<nb, kBlk, 0, st>>>(in, h->P, h->cnt, h->cloud, h->vl_cloud, h->fin, h->meta);
  k_llreg_feature<<<nb, kBlk, 0, st>>>(c, h->meta, h->P, h->curv, h->depth, h->refl, h->attr, h->vis);
  k_llreg_rank<<<nb, kBlk, 0, st>>>(h->meta, h->P, h->curv, h->refl, h->attr, h->csort, h->rsort, h->word);
  k_llreg_pick<<<h->P.n_scans, kPickWindow, 0, st>>>(c, h->meta, h->P, h->curv, h->depth, h->refl, h->attr, h->word,
                                                     h->csort, h->rsort, h->flags);
  k_llreg_chain<<<h->P.n_scans, kChainThreads, 0, st>>>(h->meta, h->attr, h->vis);
  k_llreg_flags<<<nb, kBlk, 0, st>>>(c, h->meta, h->P, h->vis, h->vl_cloud, h->flags, h->cloud);
  k_llreg_tally<<<nb, kBlk, 0, st>>>(h->cloud, h->meta, h->cnt);
  k_llreg_collect<<<nb, kBlk, 0, st>>>(h->cloud, h->meta, h->cnt, h->corner, h->surf);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(h->h_meta, h->meta, 4 * kMeta, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));  // the message's one wait
  if (h->h_meta[kErr]) {
    set_error(std::string(who) + ": a line of more than 20000 points");
    return SLIO_ECAPACITY;
  }
  for (int k = 0; k < kMeta; ++k) h->meta_host[k] = h->h_meta[k];
  for (int k = 0; k < 3; ++k) counts[k] = h->meta_host[k];
  h->has_run = true;
  return SLIO_OK;
}

}  // namespace

namespace slio {
namespace llreg {

int view(void* handle, slio_llreg_view* v, const char* who) {
  if (!handle || !is_live(handle) || !v) {
    set_error(std::string(who) + ": the registration handle is null or destroyed, or the view is null");
    return SLIO_EINVAL;
  }
  const slio_llreg* h = (const slio_llreg*)handle;
  if (!h->has_run) {
    set_error(std::string(who) + ": no run on the registration handle");
    return SLIO_ESTATE;
  }
  v->cloud = (const float*)h->cloud;
  v->corner = (const float*)h->corner;
  v->surf = (const float*)h->surf;
  v->n_cloud = h->meta_host[kNCloud];
  v->n_corner = h->meta_host[kNCorner];
  v->n_surf = h->meta_host[kNSurf];
  v->device = h->prm.device;
  return SLIO_OK;
}

}  // namespace llreg
}  // namespace slio

#define LLREG_CHECK(h, who)                            \
  do {                                                 \
    if (!(h) || !is_live(h)) {                         \
      set_error(who ": null or destroyed handle");     \
      return SLIO_EINVAL;                              \
    }                                                  \
  } while (0)

extern "C" {

int slio_llreg_create(slio_llreg_handle* out, const slio_llreg_params* p) {
  if (!out || !p) {
    set_error("slio_llreg_create: null argument");
    return SLIO_EINVAL;
  }
  Params P;
  const int rc = check_params(p, "slio_llreg_create", &P);
  if (rc) return rc;
  if (p->max_points < 1 || p->max_points > kMaxPoints || p->device < 0) {
    set_error("slio_llreg_create: bad arguments (max_points in 1 .. 120000, device >= 0)");
    return SLIO_EINVAL;
  }
  int ndev = 0;
  SLIO_HIP(hipGetDeviceCount(&ndev));
  if (p->device >= ndev) {
    set_error("slio_llreg_create: no such device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(p->device));
  slio_llreg* h = new slio_llreg();
  h->prm = *p;
  h->P = P;
  const size_t cap = (size_t)p->max_points, nb = (cap + kBlk - 1) / kBlk;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (!e) e = hipMalloc(&h->in, 18 * cap);
  if (!e) e = hipMalloc(&h->cloud, 32 * cap);
  if (!e) e = hipMalloc(&h->corner, 32 * cap);
  if (!e) e = hipMalloc(&h->surf, 32 * cap);
  if (!e) e = hipMalloc(&h->fin, 16 * cap);
  if (!e) e = hipMalloc(&h->curv, 4 * cap);
  if (!e) e = hipMalloc(&h->depth, 4 * cap);
  if (!e) e = hipMalloc(&h->refl, 4 * cap);
  if (!e) e = hipMalloc(&h->attr, 2 * cap);
  if (!e) e = hipMalloc(&h->word, 4 * cap);
  if (!e) e = hipMalloc(&h->vis, cap);
  if (!e) e = hipMalloc(&h->vl_cloud, 4 * cap);
  if (!e) e = hipMalloc(&h->csort, 4 * cap);
  if (!e) e = hipMalloc(&h->rsort, 4 * cap);
  if (!e) e = hipMalloc(&h->flags, 4 * cap);
  if (!e) e = hipMalloc(&h->cnt, 4 * 2 * kMaxScans * nb);
  if (!e) e = hipMalloc(&h->meta, 4 * kMeta);
  if (!e) e = hipHostMalloc(&h->h_in, 18 * cap, hipHostMallocDefault);
  if (!e) e = hipHostMalloc(&h->h_meta, 4 * kMeta, hipHostMallocDefault);
  if (e) {
    set_error(std::string("slio_llreg_create: ") + hipGetErrorString(e));
    llreg_free(h);
    delete h;
    return SLIO_ENOMEM;
  }
  // (every entry of a part is written before it is read; a zero is an index inside any line all the same)
  if (!e) e = hipMemset(h->csort, 0, 4 * cap);
  if (!e) e = hipMemset(h->rsort, 0, 4 * cap);
  if (e) {
    set_error(std::string("slio_llreg_create: ") + hipGetErrorString(e));
    llreg_free(h);
    delete h;
    return SLIO_EDEVICE;
  }
  h->dev_counted = true;
  slio::dev_users(p->device, +1);
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    g_live.insert(h);
  }
  *out = h;
  return SLIO_OK;
}

int slio_llreg_destroy(slio_llreg_handle h) {
  if (!h) return SLIO_OK;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (!g_live.erase(h)) {
      set_error("slio_llreg_destroy: not a live handle");
      return SLIO_EINVAL;
    }
  }
  (void)hipSetDevice(h->prm.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  llreg_free(h);
  if (h->dev_counted) slio::dev_users(h->prm.device, -1);
  delete h;
  return SLIO_OK;
}

int slio_llreg_run(slio_llreg_handle h, const float* xyz, const uint8_t* reflectivity, const uint8_t* line,
                   const uint32_t* offset_time, int64_t n, int32_t counts[3]) {
  LLREG_CHECK(h, "slio_llreg_run");
  if (n < 0 || (n && (!xyz || !reflectivity || !line || !offset_time)) || !counts) {
    set_error("slio_llreg_run: negative size, null array or null counts");
    return SLIO_EINVAL;
  }
  if (n > h->prm.max_points) {
    set_error("slio_llreg_run: more points than max_points");
    return SLIO_ECAPACITY;
  }
  // (the previous run ended with a wait: the staging buffer is free)
  const size_t N = (size_t)n;
  Input in{};
  in.n = (int)n;
  in.pc2 = 0;
  if (n) {
    std::memcpy(h->h_in, xyz, 12 * N);
    std::memcpy(h->h_in + 12 * N, offset_time, 4 * N);
    std::memcpy(h->h_in + 16 * N, reflectivity, N);
    std::memcpy(h->h_in + 17 * N, line, N);
    in.xyz = (const float*)h->in;
    in.offset = (const uint32_t*)(h->in + 12 * N);
    in.refl = h->in + 16 * N;
    in.line = h->in + 17 * N;
    in.time_span = to_sec(offset_time[n - 1]);  // :1237
  }
  return run(h, in, 18 * N, counts, "slio_llreg_run");
}

int slio_llreg_run_pc2(slio_llreg_handle h, const float* xyzi, int64_t n, int32_t counts[3]) {
  LLREG_CHECK(h, "slio_llreg_run_pc2");
  if (n < 0 || (n && !xyzi) || !counts) {
    set_error("slio_llreg_run_pc2: negative size, null cloud or null counts");
    return SLIO_EINVAL;
  }
  if (h->P.n_scans < 4) {
    set_error("slio_llreg_run_pc2: line = i % 4 needs n_scans >= 4");
    return SLIO_EINVAL;
  }
  if (n > h->prm.max_points) {
    set_error("slio_llreg_run_pc2: more points than max_points");
    return SLIO_ECAPACITY;
  }
  Input in{};
  in.n = (int)n;
  in.pc2 = 1;
  if (n) {
    std::memcpy(h->h_in, xyzi, 16 * (size_t)n);
    in.xyz = (const float*)h->in;
  }
  return run(h, in, 16 * (size_t)n, counts, "slio_llreg_run_pc2");
}

int slio_llreg_get_cloud(slio_llreg_handle h, int kind, float* points, int64_t cap) {
  LLREG_CHECK(h, "slio_llreg_get_cloud");
  if (kind < 0 || kind > 2 || !points || cap < 0) {
    set_error("slio_llreg_get_cloud: kind outside {0, 1, 2}, null output or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_llreg_get_cloud: no run before");
    return SLIO_ESTATE;
  }
  const int n = h->meta_host[kind];
  if (cap < n) {
    set_error("slio_llreg_get_cloud: the output holds fewer points than the cloud");
    return SLIO_ECAPACITY;
  }
  if (!n) return SLIO_OK;
  const Point8* src = kind == 0 ? h->cloud : kind == 1 ? h->corner : h->surf;
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipMemcpyAsync(points, src, 32 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_llreg_get_lines(slio_llreg_handle h, int32_t line_size[6], int32_t finite_size[6]) {
  LLREG_CHECK(h, "slio_llreg_get_lines");
  if (!h->has_run) {
    set_error("slio_llreg_get_lines: no run before");
    return SLIO_ESTATE;
  }
  for (int l = 0; l < kMaxScans; ++l) {
    if (line_size) line_size[l] = h->meta_host[kVSize + l];
    if (finite_size) finite_size[l] = h->meta_host[kFSize + l];
  }
  return SLIO_OK;
}

int slio_llreg_get_flags(slio_llreg_handle h, int32_t l, int32_t* flags, uint8_t* visited, float* xyzi, int64_t cap) {
  LLREG_CHECK(h, "slio_llreg_get_flags");
  if (l < 0 || l >= kMaxScans || cap < 0) {
    set_error("slio_llreg_get_flags: line outside 0 .. 5 or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_llreg_get_flags: no run before");
    return SLIO_ESTATE;
  }
  const int m = h->meta_host[kFSize + l];
  if (cap < m) {
    set_error("slio_llreg_get_flags: the outputs hold fewer points than the line");
    return SLIO_ECAPACITY;
  }
  if (!m) return SLIO_OK;
  size_t off = 0;
  for (int k = 0; k < l; ++k) off += (size_t)h->meta_host[kFSize + k];
  SLIO_HIP(hipSetDevice(h->prm.device));
  if (flags) SLIO_HIP(hipMemcpyAsync(flags, h->flags + off, 4 * (size_t)m, hipMemcpyDeviceToHost, h->stream));
  if (visited) SLIO_HIP(hipMemcpyAsync(visited, h->vis + off, (size_t)m, hipMemcpyDeviceToHost, h->stream));
  if (xyzi) SLIO_HIP(hipMemcpyAsync(xyzi, h->fin + off, 16 * (size_t)m, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_llreg_get_view(slio_llreg_handle h, slio_llreg_view* v) { return view(h, v, "slio_llreg_get_view"); }

}  // extern "C"
