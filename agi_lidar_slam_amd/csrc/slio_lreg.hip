// slio_lreg.hip -- livox_mapping's scanRegistration on the device
// (src/livox_mapping/src/scanRegistration.cpp, laserCloudHandler :152-534).
// The per-point formulas are slio_lreg.hpp's, shared with the host restatement
// (slio_lreg.cpp).  One registration is six launches, whatever n, and one host
// wait (the three counts):
//
//   k_lreg_count    finite points per block of 256 inputs
//   k_lreg_prepare  stable compaction (a block sums the counts of the blocks
//                   before it), new intensity; writes N
//   k_lreg_stride   bit q = right_curvature(5 + q) < 0.01 for every loop
//                   position: the stride of loop 1 there, were it visited
//   k_lreg_chain    ONE workgroup: the visited set of loop 1
//   k_lreg_flags    loop 1's writes in gather form, then loop 2; counts of
//                   surf and corner points per block
//   k_lreg_collect  the two stable compactions; writes the two counts
//
// The chain.  Loop 1 is `for (i = 5; i < N - 5; i += count_num)` with
// count_num = 4 where right_curvature(i) < 0.01 and 1 elsewhere, and nothing
// else survives an iteration.  The stride bits do not depend on the chain.
// Over a run of positions [a, b) the chain is a map from the entry offset (the
// first visited position at or after a, minus a: 0 .. 3) to the exit offset
// (the first visited position at or after b, minus b: 0 .. 3 again, as a step
// is at most 4).  These maps compose associatively, so the chain is a scan:
// each of the 256 threads folds its 128 positions into one map (four 2-bit
// values in a byte), the workgroup scans the bytes under composition in LDS,
// and each thread replays its run from its entry offset, marking the visited
// bits.  256 x 128 = 32768 positions cover the 32000 the reference allows
// (:53), so one workgroup sees the whole chain: no grid barrier, and no
// workgroup waits for another anywhere in this file.
//
// Loop 1's writes in gather form.  Position p receives flag 1 from a visited
// p - 2 with right_curvature < 0.001, flag 1 from a visited p + 2 with
// left_curvature < 0.001, and 150 from itself when visited.  Different values
// never meet: a visited i with right_curvature < 0.01 steps to i + 4, so i + 1
// .. i + 3 are not visited; hence a visited p - 2 that writes p is followed by
// p + 2 (p is not visited: no 150), and a p that becomes 150 is followed by
// p + 4 (p + 2 is not visited: no later 1).  The value is therefore 150 if p
// qualifies, else 1 if either neighbour writes, else 0, with no priority rule.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <set>
#include <vector>

#include "slio_device.hpp"
#include "slio_frontend.h"
#include "slio_lreg.hpp"

using slio::set_error;
using namespace slio::lreg;

namespace {

constexpr int kBlk = 256;
constexpr int kNumBlk = (kMaxPoints + kBlk - 1) / kBlk;  // 125
constexpr int kWords = kChainSpan / 64;                  // 512

// the number of threads of the block before this one, in thread order, whose
// pred is set; *total = the block's count
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
  __syncthreads();  // (the array is free for the next call)
  *total = tot;
  return base + r;
}

__device__ __forceinline__ bool finite_xyz(const float4& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

__global__ void __launch_bounds__(kBlk) k_lreg_count(const float4* __restrict__ in, int n, int* __restrict__ cnt) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  int total;
  (void)block_rank(i < n && finite_xyz(in[i]), &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kBlk)
k_lreg_prepare(const float4* __restrict__ in, int n, const int* __restrict__ cnt, float4* __restrict__ cloud,
               int* __restrict__ dN) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
  bool ok = false;
  if (i < n) {
    p = in[i];
    ok = finite_xyz(p);
  }
  int total;
  const int r = block_rank(ok, &total);
  int base = 0;
  for (int b = 0; b < (int)blockIdx.x; ++b) base += cnt[b];
  if (ok) {
    p.w = scan_intensity(p.y, p.z, p.w);
    cloud[base + r] = p;  // base + r < the number of finite inputs <= n <= kMaxPoints
  }
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) dN[0] = base + total;
}

__global__ void __launch_bounds__(kBlk)
k_lreg_stride(const float* __restrict__ c, const int* __restrict__ dN, unsigned long long* __restrict__ sbits) {
  const int q = blockIdx.x * kBlk + threadIdx.x;  // < kChainSpan
  const int N = dN[0], i = q + 5;
  const bool s4 = i < N - 5 && stride4(c, i);
  const unsigned long long b = __ballot(s4);
  if ((threadIdx.x & 63) == 0) sbits[q >> 6] = b;
}

__device__ __forceinline__ int map_apply(uint32_t m, int e) { return (int)((m >> (2 * e)) & 3u); }
// first, then second
__device__ __forceinline__ uint32_t map_compose(uint32_t first, uint32_t second) {
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) m |= (uint32_t)map_apply(second, map_apply(first, e)) << (2 * e);
  return m;
}

__global__ void __launch_bounds__(kChainThreads)
k_lreg_chain(const unsigned long long* __restrict__ sbits, const int* __restrict__ dN,
             unsigned long long* __restrict__ vbits) {
  __shared__ uint8_t mp[2][kChainThreads];
  const int t = threadIdx.x;
  const unsigned long long w0 = sbits[2 * t], w1 = sbits[2 * t + 1];
  auto step = [&](int pos) { return ((pos < 64 ? w0 >> pos : w1 >> (pos - 64)) & 1ull) ? 4 : 1; };
  uint32_t m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    int pos = e;
    while (pos < kChainPerThread) pos += step(pos);
    m |= (uint32_t)(pos - kChainPerThread) << (2 * e);
  }
  // inclusive scan under composition (Hillis-Steele, earlier runs first)
  int cur = 0;
  mp[0][t] = (uint8_t)m;
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
  const int M = dN[0] - 10;  // loop positions: i = 5 + q, q < M
  unsigned long long v0 = 0, v1 = 0;
  for (int pos = entry; pos < kChainPerThread && t * kChainPerThread + pos < M; pos += step(pos)) {
    if (pos < 64) v0 |= 1ull << pos;
    else v1 |= 1ull << (pos - 64);
  }
  vbits[2 * t] = v0;
  vbits[2 * t + 1] = v1;
}

__device__ __forceinline__ bool visited_at(const unsigned long long* __restrict__ vbits, int i, int N) {
  if (i < 5 || i >= N - 5) return false;
  const int q = i - 5;
  return (vbits[q >> 6] >> (q & 63)) & 1ull;
}

__global__ void __launch_bounds__(kBlk)
k_lreg_flags(const float* __restrict__ c, const int* __restrict__ dN, const unsigned long long* __restrict__ vbits,
             int* __restrict__ flags, int* __restrict__ cnt_corner, int* __restrict__ cnt_surf) {
  const int p = blockIdx.x * kBlk + threadIdx.x;
  const int N = dN[0];
  int f = 0;
  if (p < N) {
    // a visited i lies in [5, N - 5): every index its formulas read is inside the cloud
    if (visited_at(vbits, p - 2, N) && right_curvature(c, p - 2) < 0.001) f = 1;
    if (visited_at(vbits, p + 2, N) && left_curvature(c, p + 2) < 0.001) f = 1;
    if (visited_at(vbits, p, N) && left_curvature(c, p) < 0.01 && right_curvature(c, p) < 0.01 &&
        surf_surf_corner(c, p))
      f = 150;
    if (p >= 5 && p < N - 5) f = loop2(c, p, f, nullptr);
    flags[p] = f;
  }
  int tc, ts;
  (void)block_rank(p < N && (f == 100 || f == 150), &tc);
  (void)block_rank(p < N && f == 1, &ts);
  if (threadIdx.x == 0) {
    cnt_corner[blockIdx.x] = tc;
    cnt_surf[blockIdx.x] = ts;
  }
}

__global__ void __launch_bounds__(kBlk)
k_lreg_collect(const float4* __restrict__ cloud, int* __restrict__ dN, const int* __restrict__ flags,
               const int* __restrict__ cnt_corner, const int* __restrict__ cnt_surf, float4* __restrict__ corner,
               float4* __restrict__ surf) {
  const int p = blockIdx.x * kBlk + threadIdx.x;
  const int N = dN[0];
  const int f = p < N ? flags[p] : 0;
  int tc, ts;
  const int rc = block_rank(f == 100 || f == 150, &tc);
  const int rs = block_rank(f == 1, &ts);
  int bc = 0, bs = 0;
  for (int b = 0; b < (int)blockIdx.x; ++b) {
    bc += cnt_corner[b];
    bs += cnt_surf[b];
  }
  // (both totals are at most N <= kMaxPoints, the clouds' capacity)
  if (f == 100 || f == 150) corner[bc + rc] = cloud[p];
  if (f == 1) surf[bs + rs] = cloud[p];
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
    dN[1] = bc + tc;
    dN[2] = bs + ts;
  }
}

std::mutex g_live_mu;
std::set<void*> g_live;

}  // namespace

struct slio_lreg {
  slio_lreg_params prm{};
  bool dev_counted = false;
  hipStream_t stream = nullptr;
  float4 *in = nullptr, *cloud = nullptr, *corner = nullptr, *surf = nullptr;
  int *cnt = nullptr, *flags = nullptr, *dN = nullptr;  // cnt: 3 x kNumBlk
  unsigned long long *sbits = nullptr, *vbits = nullptr;
  float4* h_in = nullptr;  // pinned staging of the input
  int* h_counts = nullptr;
  int32_t counts[3] = {0, 0, 0};
  bool has_run = false;
};

namespace {

void lreg_free(slio_lreg* h) {
  for (void* p : {(void*)h->in, (void*)h->cloud, (void*)h->corner, (void*)h->surf, (void*)h->cnt, (void*)h->flags,
                  (void*)h->dN, (void*)h->sbits, (void*)h->vbits})
    if (p) (void)hipFree(p);
  if (h->h_in) (void)hipHostFree(h->h_in);
  if (h->h_counts) (void)hipHostFree(h->h_counts);
  if (h->stream) (void)hipStreamDestroy(h->stream);
}

bool is_live(void* h) {
  std::lock_guard<std::mutex> g(g_live_mu);
  return g_live.count(h) != 0;
}

int download(slio_lreg* h, const float4* src, int n, float* dst, int64_t cap, const char* who) {
  if (!h->has_run) {
    set_error(std::string(who) + ": no slio_lreg_run before");
    return SLIO_ESTATE;
  }
  if (cap < n) {
    set_error(std::string(who) + ": the output holds fewer points than the cloud");
    return SLIO_ECAPACITY;
  }
  if (!n) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipMemcpyAsync(dst, src, 16 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  return SLIO_OK;
}

}  // namespace

namespace slio {
namespace lreg {

int view(void* handle, View* v, const char* who) {
  if (!handle || !is_live(handle)) {
    set_error(std::string(who) + ": the registration handle is null or destroyed");
    return SLIO_EINVAL;
  }
  const slio_lreg* h = (const slio_lreg*)handle;
  if (!h->has_run) {
    set_error(std::string(who) + ": no slio_lreg_run on the registration handle");
    return SLIO_ESTATE;
  }
  v->corner_xyzi = (const float*)h->corner;
  v->surf_xyzi = (const float*)h->surf;
  v->n_corner = h->counts[1];
  v->n_surf = h->counts[2];
  v->device = h->prm.device;
  return SLIO_OK;
}

int device_of(void* handle, int32_t* device, const char* who) {
  if (!handle || !is_live(handle)) {
    set_error(std::string(who) + ": the registration handle is null or destroyed");
    return SLIO_EINVAL;
  }
  *device = ((const slio_lreg*)handle)->prm.device;
  return SLIO_OK;
}

}  // namespace lreg
}  // namespace slio

#define LREG_CHECK(h, who)                                \
  do {                                                    \
    if (!(h) || !is_live(h)) {                            \
      set_error(who ": null or destroyed handle");        \
      return SLIO_EINVAL;                                 \
    }                                                     \
  } while (0)

extern "C" {

int slio_lreg_create(slio_lreg_handle* out, const slio_lreg_params* p) {
  if (!out || !p || p->max_points < 1 || p->max_points > kMaxPoints || p->device < 0) {
    set_error("slio_lreg_create: bad arguments (max_points in 1 .. 32000, device >= 0)");
    return SLIO_EINVAL;
  }
  int ndev = 0;
  SLIO_HIP(hipGetDeviceCount(&ndev));
  if (p->device >= ndev) {
    set_error("slio_lreg_create: no such device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(p->device));
  slio_lreg* h = new slio_lreg();
  h->prm = *p;
  const size_t cap = kMaxPoints;
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (!e) e = hipMalloc(&h->in, 16 * cap);
  if (!e) e = hipMalloc(&h->cloud, 16 * cap);
  if (!e) e = hipMalloc(&h->corner, 16 * cap);
  if (!e) e = hipMalloc(&h->surf, 16 * cap);
  if (!e) e = hipMalloc(&h->cnt, 4 * 3 * kNumBlk);
  if (!e) e = hipMalloc(&h->flags, 4 * cap);
  if (!e) e = hipMalloc(&h->dN, 4 * 4);
  if (!e) e = hipMalloc(&h->sbits, 8 * kWords);
  if (!e) e = hipMalloc(&h->vbits, 8 * kWords);
  if (!e) e = hipHostMalloc(&h->h_in, 16 * cap, hipHostMallocDefault);
  if (!e) e = hipHostMalloc(&h->h_counts, 4 * 4, hipHostMallocDefault);
  if (e) {
    set_error(std::string("slio_lreg_create: ") + hipGetErrorString(e));
    lreg_free(h);
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

int slio_lreg_destroy(slio_lreg_handle h) {
  if (!h) return SLIO_OK;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (!g_live.erase(h)) {
      set_error("slio_lreg_destroy: not a live handle");
      return SLIO_EINVAL;
    }
  }
  (void)hipSetDevice(h->prm.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  lreg_free(h);
  if (h->dev_counted) slio::dev_users(h->prm.device, -1);
  delete h;
  return SLIO_OK;
}

int slio_lreg_run(slio_lreg_handle h, const float* xyzi, int64_t n, int32_t counts[3]) {
  LREG_CHECK(h, "slio_lreg_run");
  if (n < 0 || (n && !xyzi) || !counts) {
    set_error("slio_lreg_run: negative size, null cloud or null counts");
    return SLIO_EINVAL;
  }
  const int m = (int)(n < h->prm.max_points ? n : h->prm.max_points);  // :158
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t st = h->stream;
  h->has_run = false;
  if (m) {
    // (the previous run ended with a wait: the staging buffer is free)
    std::memcpy(h->h_in, xyzi, 16 * (size_t)m);
    SLIO_HIP(hipMemcpyAsync(h->in, h->h_in, 16 * (size_t)m, hipMemcpyHostToDevice, st));
  }
  int* cnt_fin = h->cnt;
  int* cnt_corner = h->cnt + kNumBlk;
  int* cnt_surf = h->cnt + 2 * kNumBlk;
  const float* c = (const float*)h->cloud;
  k_lreg_count<<<kNumBlk, kBlk, 0, st>>>(h->in, m, cnt_fin);
  k_lreg_prepare<<<kNumBlk, kBlk, 0, st>>>(h->in, m, cnt_fin, h->cloud, h->dN);
  k_lreg_stride<<<kChainSpan / kBlk, kBlk, 0, st>>>(c, h->dN, h->sbits);
  k_lreg_chain<<<1, kChainThreads, 0, st>>>(h->sbits, h->dN, h->vbits);
  k_lreg_flags<<<kNumBlk, kBlk, 0, st>>>(c, h->dN, h->vbits, h->flags, cnt_corner, cnt_surf);
  k_lreg_collect<<<kNumBlk, kBlk, 0, st>>>(h->cloud, h->dN, h->flags, cnt_corner, cnt_surf, h->corner, h->surf);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(h->h_counts, h->dN, 4 * 3, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));  // the registration's one wait
  for (int k = 0; k < 3; ++k) counts[k] = h->counts[k] = h->h_counts[k];
  h->has_run = true;
  return SLIO_OK;
}

int slio_lreg_get_cloud(slio_lreg_handle h, float* xyzi, int64_t cap) {
  LREG_CHECK(h, "slio_lreg_get_cloud");
  if (!xyzi || cap < 0) {
    set_error("slio_lreg_get_cloud: null output or negative capacity");
    return SLIO_EINVAL;
  }
  return download(h, h->cloud, h->counts[0], xyzi, cap, "slio_lreg_get_cloud");
}

int slio_lreg_get_features(slio_lreg_handle h, int kind, float* xyzi, int64_t cap) {
  LREG_CHECK(h, "slio_lreg_get_features");
  if ((kind != 0 && kind != 1) || !xyzi || cap < 0) {
    set_error("slio_lreg_get_features: kind outside {0, 1}, null output or negative capacity");
    return SLIO_EINVAL;
  }
  return download(h, kind == 0 ? h->corner : h->surf, h->counts[1 + kind], xyzi, cap, "slio_lreg_get_features");
}

int slio_lreg_get_flags(slio_lreg_handle h, int32_t* flags, uint8_t* visited) {
  LREG_CHECK(h, "slio_lreg_get_flags");
  if (!h->has_run) {
    set_error("slio_lreg_get_flags: no slio_lreg_run before");
    return SLIO_ESTATE;
  }
  const int N = h->counts[0];
  if (!N) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  std::vector<unsigned long long> vb(kWords);
  if (flags) SLIO_HIP(hipMemcpyAsync(flags, h->flags, 4 * (size_t)N, hipMemcpyDeviceToHost, h->stream));
  if (visited) SLIO_HIP(hipMemcpyAsync(vb.data(), h->vbits, 8 * kWords, hipMemcpyDeviceToHost, h->stream));
  SLIO_HIP(hipStreamSynchronize(h->stream));
  if (visited)
    for (int i = 0; i < N; ++i) {
      const int q = i - 5;
      visited[i] = q >= 0 ? (uint8_t)((vb[q >> 6] >> (q & 63)) & 1ull) : 0;  // (as the kernel left it)
    }
  return SLIO_OK;
}

}  // extern "C"
