// slio_aloam.hip -- A-LOAM's scanRegistration on the device
// (src/A-LOAM/src/scanRegistration.cpp, laserCloudHandler :124-432) for the
// 16-, 32- and 64-line layouts.  The per-point formulas are slio_aloam.hpp's,
// shared with the host restatement (slio_aloam.cpp).  One registration is
// seven launches, whatever n, on one stream, and one host wait (the five
// counts):
//
//   k_aloam_point    filters, scan id, raw orientation; per block of 256
//                    inputs the count per scan id and the first / last
//                    survivor of the filters
//   k_aloam_offsets  ONE workgroup: the stable offset of every (block, scan
//                    id), scanStartInd / scanEndInd, startOri / endOri
//   k_aloam_switch   the first kept point whose first-branch ori passes
//                    startOri + pi (halfPassed, :221): a min over the grid
//   k_aloam_scatter  the branch by the switch point, relTime, intensity; the
//                    stable scatter into laserCloud
//   k_aloam_curv     the 11-tap curvature; label and picked cleared
//   k_aloam_scan     one workgroup per scan: the six sectors in order (sort,
//                    the two greedy passes by one wavefront, the less-flat
//                    list), then the scan's VoxelGrid
//   k_aloam_concat   the four feature clouds in scan order; the counts
//
// No workgroup waits for another.  The sort (block_sort) takes a list of any
// length: pieces of kSortCap keys are ranked in LDS (a stable counting rank),
// and more than one piece is merged pairwise in global memory, each element
// finding its place by a binary search in the other run.  A sector of a usual
// sweep is one piece.
//
// The greedy passes.  A wavefront reads 64 sorted candidates at a time; the
// first lane whose candidate passes the curvature test and is unmarked is the
// serial loop's next pick (marks only grow, so the lanes before it fail
// exactly as the serial loop would have found them).  The pick's +-5 marks
// are written by 11 lanes, and the remaining lanes are tested again.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstring>
#include <mutex>
#include <set>
#include <string>

#include "slio_aloam.hpp"
#include "slio_device.hpp"
#include "slio_frontend.h"

using slio::set_error;
using namespace slio::aloam;

namespace {

constexpr int kOffThreads = 1024;                  // k_aloam_offsets: 64 scan ids x 16 runs of blocks
constexpr int kOffRuns = kOffThreads / kMaxScans;  // 16

struct Hdr {
  float start_ori, end_ori;
  int sw, N;  // the switch point (input index, INT_MAX: none); laserCloud's size
  int base[kMaxScans], tot[kMaxScans], sstart[kMaxScans], send[kMaxScans];
  int nsharp[kMaxScans], nless[kMaxScans], nflat[kMaxScans], nds[kMaxScans];
  int counts[5];
};

// the number of threads before this one, in thread order, whose pred is set;
// *total = the block's count (kBlk threads)
__device__ __forceinline__ int block_rank(bool pred, int* total) {
  __shared__ int wsum[kBlk / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long b = __ballot(pred);
  const int r = __popcll(b & ((1ull << lane) - 1ull));
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kBlk / 64; ++k) {
    if (k < w) base += wsum[k];
    tot += wsum[k];
  }
  __syncthreads();
  *total = tot;
  return base + r;
}

// exclusive scan of one int per thread over the block (kBlk threads); returns the total
__device__ __forceinline__ int block_scan(int v, int* excl) {
  __shared__ int wtot[kBlk / 64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(x, o, 64);
    if (lane >= o) x += y;
  }
  if (lane == 63) wtot[w] = x;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < kBlk / 64; ++k) {
    if (k < w) base += wtot[k];
    tot += wtot[k];
  }
  __syncthreads();
  *excl = base + x - v;
  return tot;
}

__global__ void __launch_bounds__(kBlk)
k_aloam_point(const float* __restrict__ in, int n, int S, float thres, int8_t* __restrict__ sid,
              float* __restrict__ ori, int* __restrict__ bcnt, int* __restrict__ bfirst, int* __restrict__ blast) {
  __shared__ int cnt[kMaxScans];
  __shared__ int s_first, s_last;
  const int t = threadIdx.x, i = blockIdx.x * kBlk + t;
  if (t < kMaxScans) cnt[t] = 0;
  if (t == 0) {
    s_first = INT_MAX;
    s_last = -1;
  }
  __syncthreads();
  if (i < n) {
    const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    int id = -1;
    float o = 0.f;
    if (finite3(x, y, z) && !too_close(x, y, z, thres)) {
      id = scan_id(S, elevation_deg(x, y, z), nullptr);
      o = raw_ori(x, y);
      atomicMin(&s_first, i);
      atomicMax(&s_last, i);
      if (id >= 0) atomicAdd(&cnt[id], 1);  // id < S <= kMaxScans
    }
    sid[i] = (int8_t)id;
    ori[i] = o;
  }
  __syncthreads();
  if (t < kMaxScans) bcnt[blockIdx.x * kMaxScans + t] = cnt[t];
  if (t == 0) {
    bfirst[blockIdx.x] = s_first;
    blast[blockIdx.x] = s_last;
  }
}

__global__ void __launch_bounds__(kOffThreads)
k_aloam_offsets(const int* __restrict__ bcnt, const int* __restrict__ bfirst, const int* __restrict__ blast, int nblk,
                const float* __restrict__ ori, int* __restrict__ boff, Hdr* __restrict__ hdr) {
  __shared__ int part[kOffRuns][kMaxScans];
  __shared__ int tot[kMaxScans];
  __shared__ int s_first, s_last;
  const int t = threadIdx.x, s = t & (kMaxScans - 1), run = t / kMaxScans;
  const int per = (nblk + kOffRuns - 1) / kOffRuns;
  const int b0 = min(run * per, nblk), b1 = min(b0 + per, nblk);
  if (t == 0) {
    s_first = INT_MAX;
    s_last = -1;
  }
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += bcnt[b * kMaxScans + s];
  part[run][s] = sum;
  __syncthreads();
  int f = INT_MAX, l = -1;
  for (int b = t; b < nblk; b += kOffThreads) {
    f = min(f, bfirst[b]);
    l = max(l, blast[b]);
  }
  if (f != INT_MAX) atomicMin(&s_first, f);
  if (l >= 0) atomicMax(&s_last, l);
  int before = 0, all = 0;
  for (int r = 0; r < kOffRuns; ++r) {
    if (r < run) before += part[r][s];
    all += part[r][s];
  }
  if (run == 0) tot[s] = all;
  __syncthreads();
  int base = 0;
  for (int q = 0; q < s; ++q) base += tot[q];
  int at = base + before;
  for (int b = b0; b < b1; ++b) {
    boff[b * kMaxScans + s] = at;
    at += bcnt[b * kMaxScans + s];
  }
  if (run == 0) {
    hdr->base[s] = base;
    hdr->tot[s] = all;
    hdr->sstart[s] = base + 5;      // :247
    hdr->send[s] = base + all - 6;  // :249
    if (s == kMaxScans - 1) hdr->N = base + all;
  }
  if (t == 0) {
    hdr->sw = INT_MAX;
    float so = 0.f, eo = 0.f;
    if (s_first != INT_MAX) {  // :155-163
      int br;
      so = ori[s_first];
      eo = end_ori(so, ori[s_last], &br);
    }
    hdr->start_ori = so;
    hdr->end_ori = eo;
  }
}

__global__ void __launch_bounds__(kBlk)
k_aloam_switch(const int8_t* __restrict__ sid, const float* __restrict__ ori, int n, Hdr* hdr) {
  __shared__ int s_min;
  const int t = threadIdx.x, i = blockIdx.x * kBlk + t;
  if (t == 0) s_min = INT_MAX;
  __syncthreads();
  if (i < n && sid[i] >= 0) {
    const float so = hdr->start_ori;
    int br;
    if (half_passed(first_branch(ori[i], so, &br), so)) atomicMin(&s_min, i);
  }
  __syncthreads();
  if (t == 0 && s_min != INT_MAX) atomicMin(&hdr->sw, s_min);
}

__global__ void __launch_bounds__(kBlk)
k_aloam_scatter(const float* __restrict__ in, int n, const int8_t* __restrict__ sid, const float* __restrict__ ori,
                const int* __restrict__ boff, const Hdr* __restrict__ hdr, double scan_period,
                float4* __restrict__ cloud) {
  __shared__ int wcnt[kBlk / 64][kMaxScans];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, i = blockIdx.x * kBlk + t;
  wcnt[w][lane] = 0;
  __syncthreads();
  const int id = i < n ? (int)sid[i] : -1;
  const bool ok = id >= 0;
  // this wavefront's lanes with the same scan id
  unsigned long long peers = __ballot(ok);
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const unsigned long long m = __ballot(ok && ((id >> b) & 1));
    peers &= ((id >> b) & 1) ? m : ~m;
  }
  const unsigned long long lt = (1ull << lane) - 1ull;
  if (ok && (peers & lt) == 0) wcnt[w][id] = __popcll(peers);
  __syncthreads();
  if (!ok) return;
  int at = boff[blockIdx.x * kMaxScans + id] + __popcll(peers & lt);
  for (int k = 0; k < w; ++k) at += wcnt[k][id];
  const float so = hdr->start_ori, eo = hdr->end_ori;
  int br;
  // up to and including the switch point: the first branch (:213-223)
  const float o = i <= hdr->sw ? first_branch(ori[i], so, &br) : second_branch(ori[i], eo, &br);
  // (at < the number of kept points <= n <= max_points, the cloud's capacity)
  cloud[at] = make_float4(in[3 * i], in[3 * i + 1], in[3 * i + 2], intensity_of(id, o, so, eo, scan_period));
}

__global__ void __launch_bounds__(kBlk)
k_aloam_curv(const float4* __restrict__ cloud, const Hdr* __restrict__ hdr, float* __restrict__ curv,
             int* __restrict__ label, uint8_t* __restrict__ picked) {
  const int p = blockIdx.x * kBlk + threadIdx.x, N = hdr->N;
  if (p >= N) return;
  curv[p] = (p >= 5 && p < N - 5) ? curvature((const float*)cloud, p) : 0.f;
  label[p] = 0;
  picked[p] = 0;
}

// Stable sort of n (key, value) pairs in global memory by key, ascending, by
// one workgroup of kBlk threads.  The pairs are in (k0, v0); the result is in
// the pair of buffers returned through *ks, *vs (either the inputs or k1, v1).
// skey: kSortCap keys of LDS.  Barriers on entry and exit.
__device__ __forceinline__ void block_sort(uint32_t* k0, int* v0, uint32_t* k1, int* v1, int n, uint32_t* skey,
                                           uint32_t** ks_out, int** vs_out) {
  const int t = threadIdx.x;
  __syncthreads();
  for (int c0 = 0; c0 < n; c0 += kSortCap) {
    const int m = min(kSortCap, n - c0), m4 = (m + 3) & ~3;
    for (int q = t; q < m4; q += kBlk) skey[q] = q < m ? k0[c0 + q] : 0xffffffffu;
    __syncthreads();
    const uint4* k4 = reinterpret_cast<const uint4*>(skey);
    for (int i = t; i < m; i += kBlk) {
      const uint32_t ki = skey[i];
      int c = 0;
      for (int j = 0; j < m4; j += 4) {  // (the same address in every lane: broadcast reads)
        const uint4 q = k4[j >> 2];
        c += (q.x < ki || (q.x == ki && j < i)) + (q.y < ki || (q.y == ki && j + 1 < i)) +
             (q.z < ki || (q.z == ki && j + 2 < i)) + (q.w < ki || (q.w == ki && j + 3 < i));
      }
      k1[c0 + c] = ki;  // c < m
      v1[c0 + c] = v0[c0 + i];
    }
    __syncthreads();
  }
  uint32_t *ks = k1, *kd = k0;
  int *vs = v1, *vd = v0;
  for (long long wdt = kSortCap; wdt < n; wdt <<= 1) {
    for (int i = t; i < n; i += kBlk) {
      const long long lo0 = (i / (2 * wdt)) * (2 * wdt);
      const int base = (int)lo0, mid = (int)min(lo0 + wdt, (long long)n), hi = (int)min(lo0 + 2 * wdt, (long long)n);
      const uint32_t ki = ks[i];
      int dst;
      if (i < mid) {  // the right run's keys below this one
        int lo = mid, h = hi;
        while (lo < h) {
          const int md = (lo + h) >> 1;
          if (ks[md] < ki) lo = md + 1;
          else h = md;
        }
        dst = i + (lo - mid);
      } else {  // the left run's keys not above this one
        int lo = base, h = mid;
        while (lo < h) {
          const int md = (lo + h) >> 1;
          if (ks[md] <= ki) lo = md + 1;
          else h = md;
        }
        dst = lo + (i - mid);
      }
      kd[dst] = ki;  // base <= dst < hi <= n
      vd[dst] = vs[i];
    }
    __syncthreads();
    uint32_t* tk = ks;
    ks = kd;
    kd = tk;
    int* tv = vs;
    vs = vd;
    vd = tv;
  }
  *ks_out = ks;
  *vs_out = vs;
}

// :335-366 by one wavefront: the pick's own mark and its +-5 neighbours up to
// the first gap.  ind - 5 >= the scan's first point and ind + 5 <= its last.
__device__ __forceinline__ void mark_pick(const float* c, volatile uint8_t* picked, int ind, int lane) {
  bool g = false;
  if (lane < 5) g = gap(c, ind + lane + 1, ind + lane);
  else if (lane < 10) g = gap(c, ind - (lane - 4), ind - (lane - 4) + 1);
  const unsigned long long gb = __ballot(g);
  const int fr = __builtin_ctz((unsigned)(gb & 31u) | 32u);         // marks ahead, 0 .. 5
  const int bk = __builtin_ctz((unsigned)((gb >> 5) & 31u) | 32u);  // marks behind
  if (lane <= fr) picked[ind + lane] = 1;                           // (lane 0: the pick itself)
  if (lane >= 8 && lane - 7 <= bk) picked[ind - (lane - 7)] = 1;
  __threadfence_block();
}

__global__ void __launch_bounds__(kBlk)
k_aloam_scan(Hdr* hdr, const float4* __restrict__ cloud, const float* __restrict__ curv, int* label,
             uint8_t* picked_, uint32_t* kA, int* pA, uint32_t* kB, int* pB, int* lf, float4* ds, int* sharp_idx,
             int* less_idx, int* flat_idx) {
  __shared__ __attribute__((aligned(16))) uint32_t skey[kSortCap];
  __shared__ float wmn[kBlk / 64][3], wmx[kBlk / 64][3];
  __shared__ Grid s_grid;
  const int s = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int start = hdr->sstart[s], end = hdr->send[s], lfb = hdr->base[s];
  const float* c = (const float*)cloud;
  volatile uint8_t* picked = picked_;
  if (end - start < 6) {  // :291
    if (t == 0) hdr->nsharp[s] = hdr->nless[s] = hdr->nflat[s] = hdr->nds[s] = 0;
    return;
  }
  int nsharp = 0, nless = 0, nflat = 0, m = 0;
  for (int j = 0; j < 6; ++j) {
    int sp, ep;
    sector(start, end, j, &sp, &ep);
    const int len = ep - sp + 1;
    for (int q = t; q < len; q += kBlk) {
      kA[sp + q] = __float_as_uint(curv[sp + q]);  // (a sum of squares: the bits order as the values)
      pA[sp + q] = sp + q;
    }
    uint32_t* ks;
    int* sorted;
    block_sort(kA + sp, pA + sp, kB + sp, pB + sp, len, skey, &ks, &sorted);
    if (w == 0) {
      // :308-368, from the largest curvature down
      int largest = 0;
      bool stop = false;
      for (int k0 = len - 1; k0 >= 0 && !stop; k0 -= 64) {
        const int k = k0 - lane;
        const int ind = k >= 0 ? sorted[k] : -1;
        const bool thr = ind >= 0 && is_sharp(curv[ind]);
        unsigned long long open = ~0ull;
        while (true) {
          const unsigned long long b = __ballot(thr && picked[ind] == 0) & open;
          if (!b) break;
          const int L = __ffsll((long long)b) - 1;
          const int pind = __shfl(ind, L, 64);
          if (++largest > 20) {  // :331: the 21st breaks unmarked
            stop = true;
            break;
          }
          if (lane == 0) {
            label[pind] = largest <= 2 ? 2 : 1;
            if (largest <= 2) sharp_idx[s * kSharpPerScan + nsharp] = pind;
            less_idx[s * kLessSharpPerScan + nless] = pind;
          }
          nsharp += largest <= 2;
          ++nless;
          mark_pick(c, picked, pind, lane);
          open = L == 63 ? 0ull : ~((2ull << L) - 1ull);
        }
      }
      // :371-414, from the smallest curvature up
      int smallest = 0;
      stop = false;
      for (int k0 = 0; k0 < len && !stop; k0 += 64) {
        const int k = k0 + lane;
        const int ind = k < len ? sorted[k] : -1;
        const bool thr = ind >= 0 && is_flat(curv[ind]);
        unsigned long long open = ~0ull;
        while (true) {
          const unsigned long long b = __ballot(thr && picked[ind] == 0) & open;
          if (!b) break;
          const int L = __ffsll((long long)b) - 1;
          const int pind = __shfl(ind, L, 64);
          if (lane == 0) {
            label[pind] = -1;
            flat_idx[s * kFlatPerScan + nflat] = pind;
          }
          ++nflat;
          if (++smallest >= 4) {  // :382: the 4th breaks before its marks
            stop = true;
            break;
          }
          mark_pick(c, picked, pind, lane);
          open = L == 63 ? 0ull : ~((2ull << L) - 1ull);
        }
      }
    }
    __syncthreads();
    // :416-421: the sector's positions with label <= 0, in order
    for (int q0 = 0; q0 < len; q0 += kBlk) {
      const int q = q0 + t;
      const bool keep = q < len && label[sp + q] <= 0;
      int total;
      const int r = block_rank(keep, &total);
      if (keep) lf[lfb + m + r] = sp + q;  // m + r < the scan's size
      m += total;
    }
  }
  if (t == 0) {
    hdr->nsharp[s] = nsharp;
    hdr->nless[s] = nless;
    hdr->nflat[s] = nflat;
  }
  if (m == 0) {
    if (t == 0) hdr->nds[s] = 0;
    return;
  }
  __syncthreads();  // the list
  // :424-431
  {
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int q = t; q < m; q += kBlk) {
      const float4 p = cloud[lf[lfb + q]];
      mn[0] = fminf(mn[0], p.x);
      mn[1] = fminf(mn[1], p.y);
      mn[2] = fminf(mn[2], p.z);
      mx[0] = fmaxf(mx[0], p.x);
      mx[1] = fmaxf(mx[1], p.y);
      mx[2] = fmaxf(mx[2], p.z);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) {
        mn[a] = fminf(mn[a], __shfl_xor(mn[a], o, 64));
        mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o, 64));
      }
    }
    if (lane == 0)
      for (int a = 0; a < 3; ++a) {
        wmn[w][a] = mn[a];
        wmx[w][a] = mx[a];
      }
    __syncthreads();
    if (t == 0) {
      float a0[3], a1[3];
      for (int a = 0; a < 3; ++a) {
        a0[a] = wmn[0][a];
        a1[a] = wmx[0][a];
        for (int q = 1; q < kBlk / 64; ++q) {
          a0[a] = fminf(a0[a], wmn[q][a]);
          a1[a] = fmaxf(a1[a], wmx[q][a]);
        }
      }
      s_grid = make_grid(a0, a1, 0.2f);
    }
    __syncthreads();
  }
  const Grid g = s_grid;
  if (g.overflow) {  // PCL: "Integer indices would overflow", output = input
    for (int q = t; q < m; q += kBlk) ds[lfb + q] = cloud[lf[lfb + q]];
    if (t == 0) hdr->nds[s] = m;
    return;
  }
  for (int q = t; q < m; q += kBlk) {
    const int pos = lf[lfb + q];
    const float4 p = cloud[pos];
    kA[lfb + q] = voxel_of(g, p.x, p.y, p.z);
    pA[lfb + q] = pos;
  }
  uint32_t* vk;
  int* vp;
  block_sort(kA + lfb, pA + lfb, kB + lfb, pB + lfb, m, skey, &vk, &vp);
  // one thread per voxel run start sums the run in list order (CentroidPoint);
  // voxels go out in ascending index
  const int per = (m + kBlk - 1) / kBlk;
  const int q0 = min(t * per, m), q1 = min(q0 + per, m);
  int starts = 0;
  for (int q = q0; q < q1; ++q) starts += q == 0 || vk[q] != vk[q - 1];
  int o;
  const int nvox = block_scan(starts, &o);
  for (int q = q0; q < q1; ++q) {
    if (!(q == 0 || vk[q] != vk[q - 1])) continue;
    const uint32_t id = vk[q];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int e = q;
    for (; e < m && vk[e] == id; ++e) {
      const float4 p = cloud[vp[e]];
      s0 += p.x;
      s1 += p.y;
      s2 += p.z;
      s3 += p.w;
    }
    const float cnt = (float)(e - q);
    ds[lfb + o++] = make_float4(s0 / cnt, s1 / cnt, s2 / cnt, s3 / cnt);  // o < nvox <= m
  }
  if (t == 0) hdr->nds[s] = nvox;
}

__global__ void __launch_bounds__(kBlk)
k_aloam_concat(Hdr* hdr, int S, const float4* __restrict__ cloud, const float4* __restrict__ ds,
               const int* __restrict__ sharp_idx, const int* __restrict__ less_idx,
               const int* __restrict__ flat_idx, float4* __restrict__ sharp, float4* __restrict__ less_sharp,
               float4* __restrict__ flat, float4* __restrict__ less_flat) {
  const int s = blockIdx.x, t = threadIdx.x;
  int o1 = 0, o2 = 0, o3 = 0, o4 = 0;
  for (int q = 0; q < s; ++q) {
    o1 += hdr->nsharp[q];
    o2 += hdr->nless[q];
    o3 += hdr->nflat[q];
    o4 += hdr->nds[q];
  }
  const int n1 = hdr->nsharp[s], n2 = hdr->nless[s], n3 = hdr->nflat[s], n4 = hdr->nds[s], lfb = hdr->base[s];
  // (n1 <= 12, n2 <= 120, n3 <= 24 per scan: the clouds hold kMaxScans times that; o4 + n4 <= N)
  if (t < n1) sharp[o1 + t] = cloud[sharp_idx[s * kSharpPerScan + t]];
  if (t < n2) less_sharp[o2 + t] = cloud[less_idx[s * kLessSharpPerScan + t]];
  if (t < n3) flat[o3 + t] = cloud[flat_idx[s * kFlatPerScan + t]];
  for (int q = t; q < n4; q += kBlk) less_flat[o4 + q] = ds[lfb + q];
  if (s == S - 1 && t == 0) {
    hdr->counts[0] = hdr->N;
    hdr->counts[1] = o1 + n1;
    hdr->counts[2] = o2 + n2;
    hdr->counts[3] = o3 + n3;
    hdr->counts[4] = o4 + n4;
  }
}

std::mutex g_live_mu;
std::set<void*> g_live;

}  // namespace

struct slio_aloam {
  slio_aloam_params prm{};
  bool dev_counted = false;
  hipStream_t stream = nullptr;
  int nblk = 0;
  float *in = nullptr, *ori = nullptr, *curv = nullptr;
  int8_t* sid = nullptr;
  int *bcnt = nullptr, *boff = nullptr, *bfirst = nullptr, *blast = nullptr;
  Hdr* hdr = nullptr;
  float4 *cloud = nullptr, *ds = nullptr, *out[4] = {nullptr, nullptr, nullptr, nullptr};
  int *label = nullptr, *pA = nullptr, *pB = nullptr, *lf = nullptr, *pick_idx = nullptr;
  uint32_t *kA = nullptr, *kB = nullptr;
  uint8_t* picked = nullptr;
  float* h_in = nullptr;  // pinned staging of the input
  int* h_counts = nullptr;
  int32_t counts[5] = {0, 0, 0, 0, 0};
  bool has_run = false;
};

namespace {

void aloam_free(slio_aloam* h) {
  for (void* p : {(void*)h->in, (void*)h->ori, (void*)h->curv, (void*)h->sid, (void*)h->bcnt, (void*)h->boff,
                  (void*)h->bfirst, (void*)h->blast, (void*)h->hdr, (void*)h->cloud, (void*)h->ds, (void*)h->out[0],
                  (void*)h->out[1], (void*)h->out[2], (void*)h->out[3], (void*)h->label, (void*)h->pA, (void*)h->pB,
                  (void*)h->lf, (void*)h->pick_idx, (void*)h->kA, (void*)h->kB, (void*)h->picked})
    if (p) (void)hipFree(p);
  if (h->h_in) (void)hipHostFree(h->h_in);
  if (h->h_counts) (void)hipHostFree(h->h_counts);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

bool is_live(void* h) {
  std::lock_guard<std::mutex> g(g_live_mu);
  return g_live.count(h) != 0;
}

const float4* cloud_of(const slio_aloam* h, int kind) { return kind == 0 ? h->cloud : h->out[kind - 1]; }

}  // namespace

#define ALOAM_CHECK(h, who)                               \
  do {                                                    \
    if (!(h) || !is_live(h)) {                            \
      set_error(who ": null or destroyed handle");        \
      return SLIO_EINVAL;                                 \
    }                                                     \
  } while (0)

#define ALOAM_RUN_BEFORE(h, who)                          \
  do {                                                    \
    if (!(h)->has_run) {                                  \
      set_error(who ": no slio_aloam_run before");        \
      return SLIO_ESTATE;                                 \
    }                                                     \
  } while (0)

extern "C" {

int slio_aloam_create(slio_aloam_handle* out, const slio_aloam_params* p) {
  if (!out || !p || (p->n_scans != 16 && p->n_scans != 32 && p->n_scans != 64) || p->max_points < 1 ||
      p->max_points > kMaxPoints || p->device < 0) {
    set_error("slio_aloam_create: bad arguments (n_scans 16 / 32 / 64, max_points in 1 .. 400000, device >= 0)");
    return SLIO_EINVAL;
  }
  int ndev = 0;
  SLIO_HIP(hipGetDeviceCount(&ndev));
  if (p->device >= ndev) {
    set_error("slio_aloam_create: no such device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(p->device));
  slio_aloam* h = new slio_aloam();
  h->prm = *p;
  const size_t cap = (size_t)p->max_points;
  h->nblk = (int)((cap + kBlk - 1) / kBlk);
  const size_t nb = (size_t)h->nblk;
  const size_t picks = (size_t)kMaxScans * (kSharpPerScan + kLessSharpPerScan + kFlatPerScan);
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (!e) e = hipMalloc(&h->in, 12 * cap);
  if (!e) e = hipMalloc(&h->ori, 4 * cap);
  if (!e) e = hipMalloc(&h->curv, 4 * cap);
  if (!e) e = hipMalloc(&h->sid, cap);
  if (!e) e = hipMalloc(&h->bcnt, 4 * nb * kMaxScans);
  if (!e) e = hipMalloc(&h->boff, 4 * nb * kMaxScans);
  if (!e) e = hipMalloc(&h->bfirst, 4 * nb);
  if (!e) e = hipMalloc(&h->blast, 4 * nb);
  if (!e) e = hipMalloc(&h->hdr, sizeof(Hdr));
  if (!e) e = hipMalloc(&h->cloud, 16 * cap);
  if (!e) e = hipMalloc(&h->ds, 16 * cap);
  if (!e) e = hipMalloc(&h->out[0], 16 * (size_t)kMaxScans * kSharpPerScan);
  if (!e) e = hipMalloc(&h->out[1], 16 * (size_t)kMaxScans * kLessSharpPerScan);
  if (!e) e = hipMalloc(&h->out[2], 16 * (size_t)kMaxScans * kFlatPerScan);
  if (!e) e = hipMalloc(&h->out[3], 16 * cap);
  if (!e) e = hipMalloc(&h->label, 4 * cap);
  if (!e) e = hipMalloc(&h->pA, 4 * cap);
  if (!e) e = hipMalloc(&h->pB, 4 * cap);
  if (!e) e = hipMalloc(&h->lf, 4 * cap);
  if (!e) e = hipMalloc(&h->pick_idx, 4 * picks);
  if (!e) e = hipMalloc(&h->kA, 4 * cap);
  if (!e) e = hipMalloc(&h->kB, 4 * cap);
  if (!e) e = hipMalloc(&h->picked, cap);
  if (!e) e = hipHostMalloc(&h->h_in, 12 * cap, hipHostMallocDefault);
  if (!e) e = hipHostMalloc(&h->h_counts, 4 * 8, hipHostMallocDefault);
  if (e) {
    set_error(std::string("slio_aloam_create: ") + hipGetErrorString(e));
    aloam_free(h);
    delete h;
    return SLIO_ENOMEM;
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

int slio_aloam_destroy(slio_aloam_handle h) {
  if (!h) return SLIO_OK;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (!g_live.erase(h)) {
      set_error("slio_aloam_destroy: not a live handle");
      return SLIO_EINVAL;
    }
  }
  (void)hipSetDevice(h->prm.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  aloam_free(h);
  if (h->dev_counted) slio::dev_users(h->prm.device, -1);
  delete h;
  return SLIO_OK;
}

int slio_aloam_run(slio_aloam_handle h, const float* xyz, int64_t n64, int32_t counts[5]) {
  ALOAM_CHECK(h, "slio_aloam_run");
  if (n64 < 0 || (n64 && !xyz) || !counts) {
    set_error("slio_aloam_run: negative size, null cloud or null counts");
    return SLIO_EINVAL;
  }
  if (n64 > h->prm.max_points) {
    set_error("slio_aloam_run: more points than max_points");
    return SLIO_ECAPACITY;
  }
  const int n = (int)n64, S = h->prm.n_scans, nblk = h->nblk;
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t st = h->stream;
  h->has_run = false;
  if (n) {
    // (the previous run ended with a wait: the staging buffer is free)
    std::memcpy(h->h_in, xyz, 12 * (size_t)n);
    SLIO_HIP(hipMemcpyAsync(h->in, h->h_in, 12 * (size_t)n, hipMemcpyHostToDevice, st));
  }
  int* sharp_idx = h->pick_idx;
  int* less_idx = sharp_idx + kMaxScans * kSharpPerScan;
  int* flat_idx = less_idx + kMaxScans * kLessSharpPerScan;
  k_aloam_point<<<nblk, kBlk, 0, st>>>(h->in, n, S, (float)h->prm.minimum_range, h->sid, h->ori, h->bcnt, h->bfirst,
                                        h->blast);
  k_aloam_offsets<<<1, kOffThreads, 0, st>>>(h->bcnt, h->bfirst, h->blast, nblk, h->ori, h->boff, h->hdr);
  k_aloam_switch<<<nblk, kBlk, 0, st>>>(h->sid, h->ori, n, h->hdr);
  k_aloam_scatter<<<nblk, kBlk, 0, st>>>(h->in, n, h->sid, h->ori, h->boff, h->hdr, h->prm.scan_period, h->cloud);
  k_aloam_curv<<<nblk, kBlk, 0, st>>>(h->cloud, h->hdr, h->curv, h->label, h->picked);
  k_aloam_scan<<<S, kBlk, 0, st>>>(h->hdr, h->cloud, h->curv, h->label, h->picked, h->kA, h->pA, h->kB, h->pB,
                                    h->lf, h->ds, sharp_idx, less_idx, flat_idx);
  k_aloam_concat<<<S, kBlk, 0, st>>>(h->hdr, S, h->cloud, h->ds, sharp_idx, less_idx, flat_idx, h->out[0], h->out[1],
                                      h->out[2], h->out[3]);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(h->h_counts, h->hdr->counts, 4 * 5, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));  // the registration's one wait
  for (int k = 0; k < 5; ++k) counts[k] = h->counts[k] = h->h_counts[k];
  h->has_run = true;
  return SLIO_OK;
}

int slio_aloam_get_cloud(slio_aloam_handle h, int kind, float* xyzi, int64_t cap) {
  ALOAM_CHECK(h, "slio_aloam_get_cloud");
  if (kind < 0 || kind > 4 || !xyzi || cap < 0) {
    set_error("slio_aloam_get_cloud: kind outside 0 .. 4, null output or negative capacity");
    return SLIO_EINVAL;
  }
  ALOAM_RUN_BEFORE(h, "slio_aloam_get_cloud");
  const int n = h->counts[kind];
  if (cap < n) {
    set_error("slio_aloam_get_cloud: the output holds fewer points than the cloud");
    return SLIO_ECAPACITY;
  }
  if (!n) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipMemcpyAsync(xyzi, cloud_of(h, kind), 16 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_aloam_get_scan_index(slio_aloam_handle h, int32_t* start, int32_t* end) {
  ALOAM_CHECK(h, "slio_aloam_get_scan_index");
  if (!start || !end) {
    set_error("slio_aloam_get_scan_index: null output");
    return SLIO_EINVAL;
  }
  ALOAM_RUN_BEFORE(h, "slio_aloam_get_scan_index");
  const size_t nb = 4 * (size_t)h->prm.n_scans;
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipMemcpyAsync(start, h->hdr->sstart, nb, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipMemcpyAsync(end, h->hdr->send, nb, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_aloam_get_work(slio_aloam_handle h, float* curvature_out, int32_t* label, uint8_t* picked) {
  ALOAM_CHECK(h, "slio_aloam_get_work");
  ALOAM_RUN_BEFORE(h, "slio_aloam_get_work");
  const size_t N = (size_t)h->counts[0];
  if (!N) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  if (curvature_out) SLIO_HIP(hipMemcpyAsync(curvature_out, h->curv, 4 * N, hipMemcpyDeviceToHost, h->stream));
  if (label) SLIO_HIP(hipMemcpyAsync(label, h->label, 4 * N, hipMemcpyDeviceToHost, h->stream));
  if (picked) SLIO_HIP(hipMemcpyAsync(picked, h->picked, N, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_aloam_get_view(slio_aloam_handle h, slio_aloam_view* v) {
  ALOAM_CHECK(h, "slio_aloam_get_view");
  if (!v) {
    set_error("slio_aloam_get_view: null view");
    return SLIO_EINVAL;
  }
  ALOAM_RUN_BEFORE(h, "slio_aloam_get_view");
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < 5; ++k) {
    v->cloud[k] = (const float*)cloud_of(h, k);
    v->count[k] = h->counts[k];
  }
  v->device = h->prm.device;
  return SLIO_OK;
}

}  // extern "C"
