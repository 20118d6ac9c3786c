// slio_aloam_odom.hip -- A-LOAM's laserOdometry on the device
// (src/A-LOAM/src/laserOdometry.cpp, the loop body :304-695).  The formulas
// are slio_aloam_odom.hpp's, shared with the host restatement
// (slio_aloam_odom.cpp).  One sweep is, on the handle's stream,
//
//   k_aodom_store_last  the sweep's sharp and flat points into the handle's
//                       query buffers and its two less clouds into the SPARE
//                       pair of last buffers (device to device; the caller's
//                       view may be overwritten afterwards), the table
//                       ring_start[65] of each, and the flag of a scan id that
//                       decreases or lies outside [0, 64)
//   k_aodom_assoc       one wavefront per query: TransformToStart, the exact
//                       1-NN over the whole last cloud as a packed (distance
//                       bits << 32 | index) minimum, then the ring-bounded
//                       scans as packed minima over index ranges of
//                       ring_start (forward | j, backward | ~j)
//   k_aodom_solve       ONE workgroup: the whole <= 4-iteration
//                       Levenberg-Marquardt.  Per evaluation: a factor per
//                       thread into a global scratch (28 contributions per
//                       slot), then 28 x 32 strided partial sums in ascending
//                       slot order and 28 totals in ascending lane, whatever
//                       the launch geometry; one thread runs the 6 x 6 LDL^T
//                       and the controller.  Phases are separated by
//                       __syncthreads only.  The second pass's solve ends
//                       with the integration (:600-601) and the result.
//
// assoc, solve, assoc, solve: no workgroup waits for another, and the host
// waits once, for the result.  A set flag makes every later kernel of the
// sweep return at once, so a refused sweep changes nothing; the spare buffers
// become the last clouds on the host only after the wait.  The last clouds
// stay in L2 (typically well under 1 MB); the 1-NN is brute force.
//
// The solve is this library's own; parity with Ceres' iterates is unpinned.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <set>
#include <string>

#include "slio_aloam_odom.hpp"
#include "slio_device.hpp"
#include "slio_frontend.h"

using slio::set_error;
using namespace slio::aodom;

namespace {

constexpr int kBlk = 256;          // k_aodom_assoc: four queries per workgroup
constexpr int kSolveThreads = 512;
constexpr int kMaxLast = 400000;
constexpr unsigned long long kNone = ~0ull;

struct DevState {
  double q_w[4], t_w[3], para_q[4], para_t[3];
  double pose[7];  // the lockstep entries' (q, t)
  double sums[kSums];
  int cnt[4];
  int flag;
  int ring[2][2][kMaxScans + 1];  // [buffer pair][corner, surf]
  slio_aloam_odom_result res;
};

struct Sweep {  // what the association and the evaluation read
  const float *sharp, *flat, *corner_last, *surf_last;
  const int *ring_c, *ring_s;
  int n_sharp, n_flat, n_corner, n_surf;
};

__device__ __forceinline__ unsigned long long wave_min(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned lo = __shfl_xor((unsigned)v, o, 64), hi = __shfl_xor((unsigned)(v >> 32), o, 64);
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    v = u < v ? u : v;
  }
  return v;
}

// the packed minimum of the points [lo, hi) nearer than the gate: forward the
// lowest index wins a tie, backward the highest
__device__ __forceinline__ unsigned long long scan_range(const float* L, int lo, int hi, const float sel[3], int lane,
                                                         bool backward) {
  unsigned long long best = kNone;
  for (int j = lo + lane; j < hi; j += 64) {
    const float d = dist2(L + 4 * j, sel);
    if (d < kDistSq) {
      const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (backward ? ~(unsigned)j : (unsigned)j);
      best = key < best ? key : best;
    }
  }
  return wave_min(best);
}

// forward first, then backward into the same running minimum (strict <)
__device__ __forceinline__ int pick(unsigned long long f, unsigned long long b) {
  if (b != kNone && (f == kNone || (unsigned)(b >> 32) < (unsigned)(f >> 32))) return (int)~(unsigned)b;
  return f == kNone ? -1 : (int)(unsigned)f;
}

__global__ void __launch_bounds__(kBlk)
k_aodom_store_last(const float4* __restrict__ src_sharp, const float4* __restrict__ src_flat,
                   const float4* __restrict__ src_c, const float4* __restrict__ src_s, int n_sharp, int n_flat, int n_c,
                   int n_s, float4* dst_sharp, float4* dst_flat, float4* dst_c, float4* dst_s, int* ring_c, int* ring_s,
                   int* flag) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  // (the destinations hold 12 / 24 points per scan and max_points: checked by the caller)
  if (src_sharp && i < n_sharp) dst_sharp[i] = src_sharp[i];
  if (src_flat && i < n_flat) dst_flat[i] = src_flat[i];
  for (int kind = 0; kind < 2; ++kind) {
    const float4* src = kind ? src_s : src_c;
    float4* dst = kind ? dst_s : dst_c;
    int* ring = kind ? ring_s : ring_c;
    const int n = kind ? n_s : n_c;
    if (n == 0 && i <= kMaxScans) ring[i] = 0;
    if (i >= n) continue;
    const float4* from = src ? src : dst;
    const float4 p = from[i];
    if (src) dst[i] = p;
    const int id = scan_of(p.w), prev = i ? scan_of(from[i - 1].w) : -1;
    if (id < 0 || (i && prev >= 0 && id < prev)) {
      atomicOr(flag, 1);
      continue;
    }
    if (i && prev < 0) continue;  // (flagged by the thread of i - 1)
    for (int s = prev + 1; s <= id; ++s) ring[s] = i;  // 0 <= s <= 63
    if (i == n - 1)
      for (int s = id + 1; s <= kMaxScans; ++s) ring[s] = n;
  }
}

__global__ void __launch_bounds__(kBlk)
k_aodom_assoc(Sweep w, const double* __restrict__ pose, int* __restrict__ corr, const int* __restrict__ flag) {
  if (*flag) return;
  const int lane = threadIdx.x & 63, slot = blockIdx.x * (kBlk / 64) + (threadIdx.x >> 6);
  if (slot >= w.n_sharp + w.n_flat) return;
  const bool corner = slot < w.n_sharp;
  const float* L = corner ? w.corner_last : w.surf_last;
  const int* rs = corner ? w.ring_c : w.ring_s;
  const int n = corner ? w.n_corner : w.n_surf;
  const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
  float sel[3];
  to_start(q, t, corner ? w.sharp + 4 * slot : w.flat + 4 * (slot - w.n_sharp), sel);
  // the 1-NN: every distance takes part, the gate comes after (:350)
  unsigned long long best = kNone;
  for (int j = lane; j < n; j += 64) {
    const unsigned long long key = ((unsigned long long)__float_as_uint(dist2(L + 4 * j, sel)) << 32) | (unsigned)j;
    best = key < best ? key : best;
  }
  best = wave_min(best);
  int closest = -1, ind2 = -1, ind3 = -1;
  // (an empty cloud leaves kNone, whose distance bits are a NaN's: the gate fails)
  if (__uint_as_float((unsigned)(best >> 32)) < kDistSq) {
    closest = (int)(unsigned)best;  // < n
    const int cs = (int)L[4 * closest + 3];  // in [0, 64): the cloud passed k_aodom_store_last
    int flo, fhi, blo, bhi;
    fwd_far(rs, cs, &flo, &fhi);
    bwd_far(rs, cs, &blo, &bhi);
    const int far = pick(scan_range(L, flo, fhi, sel, lane, false), scan_range(L, blo, bhi, sel, lane, true));
    if (corner) {
      ind2 = far;
    } else {
      ind3 = far;
      ind2 = pick(scan_range(L, closest + 1, rs[cs + 1], sel, lane, false),
                  scan_range(L, rs[cs], closest, sel, lane, true));
    }
  }
  if (lane == 0) {
    corr[3 * slot] = closest;
    corr[3 * slot + 1] = ind2;
    corr[3 * slot + 2] = ind3;
  }
}

struct EvalShared {
  double part[kSums][kLanes];
  double sums[kSums];
  int cnt[4];
  uint8_t valid[kMaxSlots];
};

// One evaluation at (q, t) by the whole workgroup: sums and cnt of *e.
// contrib: kSums x kMaxSlots doubles of global scratch.  Barriers on entry
// and exit.
__device__ void eval_block(const Sweep& w, const int* corr, const double* qt, double* contrib, EvalShared* e) {
  const int tid = threadIdx.x, nth = blockDim.x, slots = w.n_sharp + w.n_flat;  // slots <= kMaxSlots
  __syncthreads();
  if (tid < 4) e->cnt[tid] = 0;
  const double q[4] = {qt[0], qt[1], qt[2], qt[3]}, t[3] = {qt[4], qt[5], qt[6]};
  __syncthreads();
  for (int s = tid; s < slots; s += nth) {
    Factor f;
    int matched, deg;
    const int rows =
        slot_factor(q, t, s, w.n_sharp, w.sharp, w.flat, w.corner_last, w.surf_last, corr, &f, &matched, &deg);
    if (matched) atomicAdd(&e->cnt[s < w.n_sharp ? 0 : 1], 1);
    if (deg) atomicAdd(&e->cnt[2], 1);
    e->valid[s] = rows != 0;
    if (!rows) continue;
    double v[kSums];
    if (contributions(f, v)) atomicAdd(&e->cnt[3], 1);
    for (int k = 0; k < kSums; ++k) contrib[k * kMaxSlots + s] = v[k];
  }
  __syncthreads();
  for (int task = tid; task < kSums * kLanes; task += nth) {
    const int k = task / kLanes, l = task % kLanes;
    double acc = 0.0;
    for (int s = l; s < slots; s += kLanes)
      if (e->valid[s]) acc = acc + contrib[k * kMaxSlots + s];
    e->part[k][l] = acc;
  }
  __syncthreads();
  if (tid < kSums) {
    double tot = 0.0;
    for (int l = 0; l < kLanes; ++l) tot = tot + e->part[tid][l];
    e->sums[tid] = tot;
  }
  __syncthreads();
}

__global__ void __launch_bounds__(kSolveThreads)
k_aodom_eval(Sweep w, const int* __restrict__ corr, double* contrib, DevState* st) {
  __shared__ EvalShared e;
  __shared__ double qt[7];
  if (threadIdx.x < 7) qt[threadIdx.x] = st->pose[threadIdx.x];
  eval_block(w, corr, qt, contrib, &e);
  if (threadIdx.x < kSums) st->sums[threadIdx.x] = e.sums[threadIdx.x];
  if (threadIdx.x < 4) st->cnt[threadIdx.x] = e.cnt[threadIdx.x];
}

__global__ void __launch_bounds__(kSolveThreads)
k_aodom_solve(Sweep w, const int* __restrict__ corr, double* contrib, DevState* st, int pass) {
  __shared__ EvalShared e;
  __shared__ Lm s;
  __shared__ double qt[7];
  __shared__ int go;
  if (st->flag) return;
  const int tid = threadIdx.x;
  slio_aloam_odom_pass* out = &st->res.pass[pass];
  if (tid < 4) qt[tid] = st->para_q[tid];
  else if (tid < 7) qt[tid] = st->para_t[tid - 4];
  eval_block(w, corr, qt, contrib, &e);
  if (tid == 0) {
    lm_init(&s, qt, qt + 4);
    for (int k = 0; k < 21; ++k) s.A[k] = e.sums[k];
    for (int k = 0; k < 6; ++k) s.g[k] = e.sums[21 + k];
    s.cost = 0.5 * e.sums[27];
    out->corner = e.cnt[0];
    out->plane = e.cnt[1];
    out->degenerate = e.cnt[2];
    out->outliers = e.cnt[3];
    out->few = e.cnt[0] + e.cnt[1] < 10;
    out->cost_first = s.cost;
    for (int k = 0; k < kMaxIter; ++k) {
      for (int a = 0; a < 4; ++a) out->it_q[k][a] = 0.0;
      for (int a = 0; a < 3; ++a) out->it_t[k][a] = 0.0;
      out->it_cost[k] = out->it_mu[k] = 0.0;
    }
    go = lm_propose(&s);
    for (int k = 0; k < 4; ++k) qt[k] = s.qn[k];
    for (int k = 0; k < 3; ++k) qt[4 + k] = s.tn[k];
  }
  __syncthreads();
  while (go) {  // (uniform: go changes only between the barriers of eval_block and the one below)
    eval_block(w, corr, qt, contrib, &e);
    if (tid == 0) {
      lm_decide(&s, e.sums, e.sums + 21, 0.5 * e.sums[27]);
      if (s.last_accepted) out->outliers = e.cnt[3];
      const int k = s.iterations - 1;  // 0 .. kMaxIter - 1
      for (int a = 0; a < 4; ++a) out->it_q[k][a] = s.q[a];
      for (int a = 0; a < 3; ++a) out->it_t[k][a] = s.t[a];
      out->it_cost[k] = s.cost;
      out->it_mu[k] = s.mu;
      go = lm_propose(&s);
      for (int a = 0; a < 4; ++a) qt[a] = s.qn[a];
      for (int a = 0; a < 3; ++a) qt[4 + a] = s.tn[a];
    }
    __syncthreads();
  }
  if (tid == 0) {
    out->iterations = s.iterations;
    out->accepted = s.accepted;
    out->stop = s.stop;
    out->cost_last = s.cost;
    for (int a = 0; a < 4; ++a) st->para_q[a] = s.q[a];
    for (int a = 0; a < 3; ++a) st->para_t[a] = s.t[a];
    if (pass == 1) {
      double qw[4], tw[3];
      for (int a = 0; a < 4; ++a) qw[a] = st->q_w[a];
      for (int a = 0; a < 3; ++a) tw[a] = st->t_w[a];
      integrate(qw, tw, s.q, s.t);
      for (int a = 0; a < 4; ++a) st->q_w[a] = st->res.q_w_curr[a] = qw[a];
      for (int a = 0; a < 3; ++a) st->t_w[a] = st->res.t_w_curr[a] = tw[a];
      for (int a = 0; a < 4; ++a) st->res.q_last_curr[a] = s.q[a];
      for (int a = 0; a < 3; ++a) st->res.t_last_curr[a] = s.t[a];
    }
  }
}

std::mutex g_live_mu;
std::set<void*> g_live;

struct HostBlock {  // pinned
  slio_aloam_odom_result res;
  double sums[kSums];
  int cnt[4];
  int flag;
};

}  // namespace

struct slio_aloam_odom {
  slio_aloam_odom_params prm{};
  bool dev_counted = false;
  hipStream_t stream = nullptr;
  DevState* st = nullptr;
  HostBlock* hb = nullptr;
  float4* last[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};
  float4 *q_sharp = nullptr, *q_flat = nullptr;
  int* corr = nullptr;
  double* contrib = nullptr;
  int cur = 0;
  int n_last[2] = {0, 0}, n_sharp = 0, n_flat = 0;
  bool inited = false, has_sweep = false, has_queries = false, has_assoc = false;
  int frame_count = 0;
  double poses[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0};  // q_w, t_w, para_q, para_t
};

namespace {

void odom_free(slio_aloam_odom* h) {
  for (void* p : {(void*)h->st, (void*)h->last[0][0], (void*)h->last[0][1], (void*)h->last[1][0],
                  (void*)h->last[1][1], (void*)h->q_sharp, (void*)h->q_flat, (void*)h->corr, (void*)h->contrib})
    if (p) (void)hipFree(p);
  if (h->hb) (void)hipHostFree(h->hb);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

bool is_live(void* h) {
  std::lock_guard<std::mutex> g(g_live_mu);
  return g_live.count(h) != 0;
}

Sweep sweep_of(const slio_aloam_odom* h) {
  Sweep w;
  w.sharp = (const float*)h->q_sharp;
  w.flat = (const float*)h->q_flat;
  w.corner_last = (const float*)h->last[h->cur][0];
  w.surf_last = (const float*)h->last[h->cur][1];
  w.ring_c = h->st->ring[h->cur][0];
  w.ring_s = h->st->ring[h->cur][1];
  w.n_sharp = h->n_sharp;
  w.n_flat = h->n_flat;
  w.n_corner = h->n_last[0];
  w.n_surf = h->n_last[1];
  return w;
}

int reset_device(slio_aloam_odom* h) {
  const double id[14] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0};
  std::memcpy(h->poses, id, sizeof id);
  SLIO_HIP(hipMemcpyAsync(h->st, h->poses, sizeof id, hipMemcpyHostToDevice, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  h->inited = h->has_sweep = h->has_queries = h->has_assoc = false;
  h->frame_count = 0;
  h->n_last[0] = h->n_last[1] = h->n_sharp = h->n_flat = 0;
  return SLIO_OK;
}

int check_sizes(const slio_aloam_odom* h, int64_t n_sharp, int64_t n_less_sharp, int64_t n_flat, int64_t n_less_flat,
                const char* who) {
  if (n_sharp > (int64_t)h->prm.n_scans * kSharpPerScan || n_flat > (int64_t)h->prm.n_scans * kFlatPerScan ||
      n_less_sharp > h->prm.max_points || n_less_flat > h->prm.max_points) {
    set_error(std::string(who) + ": more points than the capacity (12 sharp / 24 flat per scan, max_points per less "
                                 "cloud)");
    return SLIO_ECAPACITY;
  }
  return SLIO_OK;
}

// The sweep once the sizes are checked.  dev: the four clouds are device
// pointers, copied by k_aodom_store_last; else host pointers, uploaded here.
int sweep(slio_aloam_odom* h, const float* sharp, int n_sharp, const float* less_sharp, int n_c, const float* flat,
          int n_flat, const float* less_flat, int n_s, bool dev, slio_aloam_odom_result* res, const char* who) {
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t s = h->stream;
  const int alt = h->cur ^ 1;
  SLIO_HIP(hipMemsetAsync(&h->st->flag, 0, sizeof(int), s));
  if (!dev) {
    if (n_sharp) SLIO_HIP(hipMemcpyAsync(h->q_sharp, sharp, 16 * (size_t)n_sharp, hipMemcpyHostToDevice, s));
    if (n_flat) SLIO_HIP(hipMemcpyAsync(h->q_flat, flat, 16 * (size_t)n_flat, hipMemcpyHostToDevice, s));
    if (n_c) SLIO_HIP(hipMemcpyAsync(h->last[alt][0], less_sharp, 16 * (size_t)n_c, hipMemcpyHostToDevice, s));
    if (n_s) SLIO_HIP(hipMemcpyAsync(h->last[alt][1], less_flat, 16 * (size_t)n_s, hipMemcpyHostToDevice, s));
  }
  int most = kMaxScans + 1;
  for (int v : {n_sharp, n_flat, n_c, n_s}) most = v > most ? v : most;
  k_aodom_store_last<<<(most + kBlk - 1) / kBlk, kBlk, 0, s>>>(
      dev ? (const float4*)sharp : nullptr, dev ? (const float4*)flat : nullptr,
      dev ? (const float4*)less_sharp : nullptr, dev ? (const float4*)less_flat : nullptr, n_sharp, n_flat, n_c, n_s,
      h->q_sharp, h->q_flat, h->last[alt][0], h->last[alt][1], h->st->ring[alt][0], h->st->ring[alt][1],
      &h->st->flag);
  const bool solve = h->inited;
  h->n_sharp = n_sharp;  // (the queries are overwritten either way)
  h->n_flat = n_flat;
  if (solve) {
    const Sweep w = sweep_of(h);
    const int slots = n_sharp + n_flat, nb = (slots + kBlk / 64 - 1) / (kBlk / 64);
    for (int pass = 0; pass < 2; ++pass) {
      if (nb) k_aodom_assoc<<<nb, kBlk, 0, s>>>(w, h->st->para_q, h->corr, &h->st->flag);
      k_aodom_solve<<<1, kSolveThreads, 0, s>>>(w, h->corr, h->contrib, h->st, pass);
    }
    SLIO_HIP(hipMemcpyAsync(&h->hb->res, &h->st->res, sizeof(slio_aloam_odom_result), hipMemcpyDeviceToHost, s));
  }
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(&h->hb->flag, &h->st->flag, sizeof(int), hipMemcpyDeviceToHost, s));
  SLIO_HIP(hipStreamSynchronize(s));  // the sweep's one wait
  if (h->hb->flag) {
    h->has_queries = h->has_assoc = false;  // (the query buffers hold the refused sweep)
    h->n_sharp = h->n_flat = 0;
    set_error(std::string(who) + ": scan ids of a less cloud decreasing or outside [0, 64); the sweep is refused and "
                                 "the poses and last clouds are unchanged");
    return SLIO_EINVAL;
  }
  std::memset(res, 0, sizeof *res);
  if (solve) {
    *res = h->hb->res;
    std::memcpy(h->poses, res->q_w_curr, 4 * sizeof(double));
    std::memcpy(h->poses + 4, res->t_w_curr, 3 * sizeof(double));
    std::memcpy(h->poses + 7, res->q_last_curr, 4 * sizeof(double));
    std::memcpy(h->poses + 11, res->t_last_curr, 3 * sizeof(double));
  } else {
    std::memcpy(res->q_w_curr, h->poses, 4 * sizeof(double));
    std::memcpy(res->t_w_curr, h->poses + 4, 3 * sizeof(double));
    std::memcpy(res->q_last_curr, h->poses + 7, 4 * sizeof(double));
    std::memcpy(res->t_last_curr, h->poses + 11, 3 * sizeof(double));
  }
  res->inited = solve;
  h->inited = true;  // :307-309
  h->cur = alt;      // :650-659
  h->n_last[0] = n_c;
  h->n_last[1] = n_s;
  h->has_sweep = h->has_queries = true;
  h->has_assoc = false;  // (the correspondences index the previous last clouds)
  res->published = h->frame_count % h->prm.skip_frame_num == 0;  // :667
  if (res->published) h->frame_count = 0;
  res->frame_count = ++h->frame_count;
  res->reserved = 0;
  return SLIO_OK;
}

}  // namespace

#define AODOM_CHECK(h, who)                               \
  do {                                                    \
    if (!(h) || !is_live(h)) {                            \
      set_error(who ": null or destroyed handle");        \
      return SLIO_EINVAL;                                 \
    }                                                     \
  } while (0)

extern "C" {

int slio_aloam_odom_create(slio_aloam_odom_handle* out, const slio_aloam_odom_params* p) {
  if (!out || !p || p->n_scans < 1 || p->n_scans > kMaxScans || p->max_points < 1 || p->max_points > kMaxLast ||
      p->skip_frame_num < 1 || p->device < 0) {
    set_error("slio_aloam_odom_create: bad arguments (n_scans in 1 .. 64, max_points in 1 .. 400000, "
              "skip_frame_num >= 1, device >= 0)");
    return SLIO_EINVAL;
  }
  int ndev = 0;
  SLIO_HIP(hipGetDeviceCount(&ndev));
  if (p->device >= ndev) {
    set_error("slio_aloam_odom_create: no such device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(p->device));
  slio_aloam_odom* h = new slio_aloam_odom();
  h->prm = *p;
  const size_t cap = (size_t)p->max_points, S = (size_t)p->n_scans;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (!e) e = hipMalloc(&h->st, sizeof(DevState));
  for (int b = 0; b < 2 && !e; ++b)
    for (int k = 0; k < 2 && !e; ++k) e = hipMalloc(&h->last[b][k], 16 * cap);
  if (!e) e = hipMalloc(&h->q_sharp, 16 * S * kSharpPerScan);
  if (!e) e = hipMalloc(&h->q_flat, 16 * S * kFlatPerScan);
  if (!e) e = hipMalloc(&h->corr, 4 * 3 * (size_t)kMaxSlots);
  if (!e) e = hipMalloc(&h->contrib, 8 * (size_t)kSums * kMaxSlots);
  if (!e) e = hipHostMalloc(&h->hb, sizeof(HostBlock), hipHostMallocDefault);
  if (!e) e = hipMemsetAsync(h->st, 0, sizeof(DevState), h->stream);
  if (e) {
    set_error(std::string("slio_aloam_odom_create: ") + hipGetErrorString(e));
    odom_free(h);
    delete h;
    return SLIO_ENOMEM;
  }
  const int rc = reset_device(h);
  if (rc != SLIO_OK) {
    odom_free(h);
    delete h;
    return rc;
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

int slio_aloam_odom_destroy(slio_aloam_odom_handle h) {
  if (!h) return SLIO_OK;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (!g_live.erase(h)) {
      set_error("slio_aloam_odom_destroy: not a live handle");
      return SLIO_EINVAL;
    }
  }
  (void)hipSetDevice(h->prm.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  odom_free(h);
  if (h->dev_counted) slio::dev_users(h->prm.device, -1);
  delete h;
  return SLIO_OK;
}

int slio_aloam_odom_reset(slio_aloam_odom_handle h) {
  AODOM_CHECK(h, "slio_aloam_odom_reset");
  SLIO_HIP(hipSetDevice(h->prm.device));
  return reset_device(h);
}

int slio_aloam_odom_run(slio_aloam_odom_handle h, const float* sharp, int64_t n_sharp, const float* less_sharp,
                        int64_t n_less_sharp, const float* flat, int64_t n_flat, const float* less_flat,
                        int64_t n_less_flat, slio_aloam_odom_result* res) {
  AODOM_CHECK(h, "slio_aloam_odom_run");
  if (!res || n_sharp < 0 || n_less_sharp < 0 || n_flat < 0 || n_less_flat < 0 || (n_sharp && !sharp) ||
      (n_less_sharp && !less_sharp) || (n_flat && !flat) || (n_less_flat && !less_flat)) {
    set_error("slio_aloam_odom_run: null result, negative size or null cloud");
    return SLIO_EINVAL;
  }
  const int rc = check_sizes(h, n_sharp, n_less_sharp, n_flat, n_less_flat, "slio_aloam_odom_run");
  if (rc != SLIO_OK) return rc;
  if (!ids_ok(less_sharp, n_less_sharp) || !ids_ok(less_flat, n_less_flat)) {
    set_error("slio_aloam_odom_run: scan ids of a less cloud decreasing or outside [0, 64)");
    return SLIO_EINVAL;
  }
  return sweep(h, sharp, (int)n_sharp, less_sharp, (int)n_less_sharp, flat, (int)n_flat, less_flat, (int)n_less_flat,
               false, res, "slio_aloam_odom_run");
}

int slio_aloam_odom_run_view(slio_aloam_odom_handle h, const slio_aloam_view* v, slio_aloam_odom_result* res) {
  AODOM_CHECK(h, "slio_aloam_odom_run_view");
  if (!v || !res) {
    set_error("slio_aloam_odom_run_view: null view or result");
    return SLIO_EINVAL;
  }
  for (int k = 1; k < 5; ++k)
    if (v->count[k] < 0 || (v->count[k] && !v->cloud[k])) {
      set_error("slio_aloam_odom_run_view: negative size or null cloud in the view");
      return SLIO_EINVAL;
    }
  if (v->device != h->prm.device) {
    set_error("slio_aloam_odom_run_view: the view is of another device");
    return SLIO_EINVAL;
  }
  const int rc = check_sizes(h, v->count[1], v->count[2], v->count[3], v->count[4], "slio_aloam_odom_run_view");
  if (rc != SLIO_OK) return rc;
  return sweep(h, v->cloud[1], v->count[1], v->cloud[2], v->count[2], v->cloud[3], v->count[3], v->cloud[4],
               v->count[4], true, res, "slio_aloam_odom_run_view");
}

int slio_aloam_odom_get_last(slio_aloam_odom_handle h, float* corner_last, int64_t cap_corner, float* surf_last,
                             int64_t cap_surf, int32_t counts[2]) {
  AODOM_CHECK(h, "slio_aloam_odom_get_last");
  if (!counts || cap_corner < 0 || cap_surf < 0) {
    set_error("slio_aloam_odom_get_last: null counts or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_sweep) {
    set_error("slio_aloam_odom_get_last: no sweep before");
    return SLIO_ESTATE;
  }
  counts[0] = h->n_last[0];
  counts[1] = h->n_last[1];
  if ((corner_last && cap_corner < counts[0]) || (surf_last && cap_surf < counts[1])) {
    set_error("slio_aloam_odom_get_last: an output holds fewer points than its cloud");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  if (corner_last && counts[0])
    SLIO_HIP(hipMemcpyAsync(corner_last, h->last[h->cur][0], 16 * (size_t)counts[0], hipMemcpyDeviceToHost, h->stream));
  if (surf_last && counts[1])
    SLIO_HIP(hipMemcpyAsync(surf_last, h->last[h->cur][1], 16 * (size_t)counts[1], hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_aloam_odom_get_view(slio_aloam_odom_handle h, slio_aloam_odom_view* v) {
  AODOM_CHECK(h, "slio_aloam_odom_get_view");
  if (!v) {
    set_error("slio_aloam_odom_get_view: null view");
    return SLIO_EINVAL;
  }
  if (!h->has_sweep) {
    set_error("slio_aloam_odom_get_view: no sweep before");
    return SLIO_ESTATE;
  }
  v->corner_last = (const float*)h->last[h->cur][0];
  v->surf_last = (const float*)h->last[h->cur][1];
  v->n_corner = h->n_last[0];
  v->n_surf = h->n_last[1];
  v->device = h->prm.device;
  v->reserved = 0;
  return SLIO_OK;
}

int slio_aloam_odom_get_correspondences(slio_aloam_odom_handle h, int32_t* corr, int64_t cap_slots, int32_t* n) {
  AODOM_CHECK(h, "slio_aloam_odom_get_correspondences");
  if (!n || cap_slots < 0 || (!corr && cap_slots)) {
    set_error("slio_aloam_odom_get_correspondences: null count, negative capacity or null output");
    return SLIO_EINVAL;
  }
  if (!h->has_assoc) {
    set_error("slio_aloam_odom_get_correspondences: no association on the present last clouds");
    return SLIO_ESTATE;
  }
  *n = h->n_sharp + h->n_flat;
  if (cap_slots < *n) {
    set_error("slio_aloam_odom_get_correspondences: the output holds fewer slots than the association");
    return SLIO_ECAPACITY;
  }
  if (!*n) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipMemcpyAsync(corr, h->corr, 12 * (size_t)*n, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

int slio_aloam_odom_associate(slio_aloam_odom_handle h, const double q[4], const double t[3]) {
  AODOM_CHECK(h, "slio_aloam_odom_associate");
  if (!q || !t) {
    set_error("slio_aloam_odom_associate: null pose");
    return SLIO_EINVAL;
  }
  if (!h->has_queries) {
    set_error("slio_aloam_odom_associate: no sweep before, or the last one was refused");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  double* pose = h->hb->sums;  // (pinned; the stream is idle between calls)
  std::memcpy(pose, q, 4 * sizeof(double));
  std::memcpy(pose + 4, t, 3 * sizeof(double));
  SLIO_HIP(hipMemcpyAsync(h->st->pose, pose, 7 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  const Sweep w = sweep_of(h);
  const int slots = h->n_sharp + h->n_flat, nb = (slots + kBlk / 64 - 1) / (kBlk / 64);
  if (nb) k_aodom_assoc<<<nb, kBlk, 0, h->stream>>>(w, h->st->pose, h->corr, &h->st->flag);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipStreamSynchronize(h->stream));
  h->has_assoc = true;
  return SLIO_OK;
}

int slio_aloam_odom_evaluate(slio_aloam_odom_handle h, const double q[4], const double t[3], double A[21],
                             double g[6], double* cost, int32_t counts[4]) {
  AODOM_CHECK(h, "slio_aloam_odom_evaluate");
  if (!q || !t || !A || !g || !cost || !counts) {
    set_error("slio_aloam_odom_evaluate: null pose or output");
    return SLIO_EINVAL;
  }
  if (!h->has_assoc) {
    set_error("slio_aloam_odom_evaluate: no association on the present last clouds");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  double* pose = h->hb->sums;
  std::memcpy(pose, q, 4 * sizeof(double));
  std::memcpy(pose + 4, t, 3 * sizeof(double));
  SLIO_HIP(hipMemcpyAsync(h->st->pose, pose, 7 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  k_aodom_eval<<<1, kSolveThreads, 0, h->stream>>>(sweep_of(h), h->corr, h->contrib, h->st);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(h->hb->sums, h->st->sums, sizeof(double) * kSums + sizeof(int) * 4, hipMemcpyDeviceToHost,
                          h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  std::memcpy(A, h->hb->sums, 21 * sizeof(double));
  std::memcpy(g, h->hb->sums + 21, 6 * sizeof(double));
  *cost = 0.5 * h->hb->sums[27];
  for (int k = 0; k < 4; ++k) counts[k] = h->hb->cnt[k];
  return SLIO_OK;
}

}  // extern "C"
