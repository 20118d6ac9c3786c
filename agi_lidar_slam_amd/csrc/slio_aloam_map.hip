// slio_aloam_map.hip -- A-LOAM's laserMapping on the device
// (src/A-LOAM/src/laserMapping.cpp, the loop body of process() :326-893 and
// the cloud outputs of :898-939).  The formulas are slio_aloam_map.hpp's,
// shared with the host restatement (slio_aloam_map.cpp); the cube map is the
// store of slio_cube_store.hpp with the extents 21 x 21 x 11.  This file adds
// only what differs from livox_mapping's mapper: the append kernel (the double
// quaternion transform, then the cube index), the list of cubes to filter, and
// the scan-to-map solve:
//
//   k_amap_associate<KIND>  one thread per point of a down-sampled cloud:
//                           pointAssociateToMap at the pose in device memory,
//                           the exact 5-NN in the class's search grid, the fit,
//                           one factor record per slot
//   k_amap_evaluate         one thread per slot, 256 slots per workgroup: the
//                           factor at the evaluation pose, its 28
//                           contributions into LDS, the workgroup's partial
//                           in the header's order (32 strided lanes, then the
//                           lanes in ascending order)
//   k_amap_control          ONE wavefront: the same two steps over the
//                           workgroups' partials, then lm_init / lm_decide /
//                           lm_propose on the sums, the next evaluation pose,
//                           and after the last iteration of the second pass
//                           transformUpdate and the result
//
// Exactness of the 5-NN: slio_mapopt.hip's argument for k_lvx_pass with the
// gate 1.0 and the cell edge kCell = 1.0625 (kCell - kCellTol > 1 = sqrt(gate)):
// the query lies in the centre cell of its 3 x 3 x 3 block, every map point
// outside the block is at least `bound` >= kCell - kCellTol away, so a fifth
// distance below the gate proves the block's five nearest are the map's, and a
// query that is not proven has a fifth distance above the gate whichever points
// it is made of.  The keys are (bits(d^2) << 32) | index in the concatenation
// of the valid cubes: ties go to the lower index.
//
// A sweep is enqueued on the handle's stream without a host wait inside the
// solve: per pass associate x 2, evaluate, control, 4 x (evaluate, control);
// evaluate returns at once when the solve has stopped.  No workgroup waits for
// another; there is no floating-point atomic; every loop is bounded by a size
// known at launch.  Host waits per sweep: the two VoxelGrids of the incoming
// clouds (2), a shift (0 to 2), the bounding boxes of the two search grids
// (2), the result (1), the map update (2).
//
// The solve is this library's own; parity with Ceres' iterates is unpinned.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <set>
#include <string>

#include "slio_aloam_map.hpp"
#include "slio_cube_store.hpp"
#include "slio_device.hpp"
#include "slio_frontend.h"

using slio::MapDev;
using slio::set_error;
using namespace slio::amap;
namespace aodom = slio::aodom;
namespace lvx = slio::lvx;

namespace {

constexpr float kCell = 1.0625f;
static_assert(kCell - lvx::kCellTol > 1.0f, "the cell edge must exceed the square root of the gate");
static_assert(kW * kH * kD == lvx::kNum, "the store holds 4851 cubes");
enum { kPhaseFirst = 0, kPhaseStep = 1, kPhaseReduce = 2, kPhaseFinish = 3 };

struct MapState {
  double q[4], t[3];          // q_w_curr, t_w_curr: where the association runs
  double eval[7];             // where the evaluation runs
  double q_wodom[4], t_wodom[3];
  aodom::Lm lm;
  int go;                     // the evaluation is wanted
  double sums[kSums];
  int cnt[4];
  slio_aloam_map_result res;
};

struct Slots {  // the factor slots: the corner stack, then the surf stack
  const float *corner, *surf;  // n x 3, body frame
  int n_corner, n_surf;
  uint8_t* kind;
  double* rec;
  int32_t* idx;
  float* sqd;
};

template <int KIND>
__global__ void __launch_bounds__(256)
k_amap_associate(const lvx::GridView g, const float* __restrict__ map_xyz, Slots s, const double* __restrict__ pose) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = KIND == 0 ? s.n_corner : s.n_surf;
  if (i >= n) return;
  const int slot = KIND == 0 ? i : s.n_corner + i;
  const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
  float w[3];
  aodom::to_start(q, t, (KIND == 0 ? s.corner : s.surf) + 3 * i, w);
  uint64_t top[kK];
#pragma unroll
  for (int j = 0; j < kK; ++j) top[j] = ~0ull;
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
    bound -= lvx::kCellTol;
    if (inside) {
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy) {
          const int64_t base = ((int64_t)(c[2] + dz) * g.ny + (c[1] + dy)) * g.nx + (c[0] - 1);
          const uint32_t p0 = g.start[base], p1 = g.start[base + 3];  // (<= g.n: the start table's own bound)
          for (uint32_t p = p0; p < p1; ++p) {
            const float4 m = g.pts[p];
            const float dx = m.x - w[0], dy2 = m.y - w[1], dz2 = m.z - w[2];
            const float d2 = (dx * dx + dy2 * dy2) + dz2 * dz2;
            uint64_t key = ((uint64_t)__float_as_uint(d2) << 32) | __float_as_uint(m.w);
#pragma unroll
            for (int j = 0; j < kK; ++j) {  // a sorted insertion without data-dependent branches
              const uint64_t lo = key < top[j] ? key : top[j], hi = key < top[j] ? top[j] : key;
              top[j] = lo;
              key = hi;
            }
          }
        }
      const uint64_t kth = top[kK - 1];
      const float d2k = __uint_as_float((uint32_t)(kth >> 32));
      near = kth != ~0ull && bound > 0.0f && d2k <= bound * bound && d2k < kGate;
    }
  }
  double rec[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int kind = kNone;
  if (near) {
    double nb[kK][3];
#pragma unroll
    for (int j = 0; j < kK; ++j) {
      const uint32_t m = (uint32_t)top[j];  // < g.n: an index of the gathered map
      nb[j][0] = (double)map_xyz[3 * (int64_t)m];
      nb[j][1] = (double)map_xyz[3 * (int64_t)m + 1];
      nb[j][2] = (double)map_xyz[3 * (int64_t)m + 2];
      s.idx[kK * (int64_t)slot + j] = (int32_t)m;
      s.sqd[kK * (int64_t)slot + j] = __uint_as_float((uint32_t)(top[j] >> 32));
    }
    kind = fit(KIND, nb, rec);
  } else {
#pragma unroll
    for (int j = 0; j < kK; ++j) {
      s.idx[kK * (int64_t)slot + j] = -1;
      s.sqd[kK * (int64_t)slot + j] = INFINITY;
    }
  }
  s.kind[slot] = (uint8_t)kind;
#pragma unroll
  for (int k = 0; k < 6; ++k) s.rec[6 * (int64_t)slot + k] = rec[k];
}

// P: kSums doubles per workgroup, cntP: 4 ints per workgroup
__global__ void __launch_bounds__(kWg)
k_amap_evaluate(Slots s, const MapState* __restrict__ st, double* __restrict__ P, int* __restrict__ cntP) {
  __shared__ double c[kSums][kWg];
  __shared__ double part[kSums][kLanes];
  __shared__ uint8_t valid[kWg];
  __shared__ int cnt[4];
  if (!st->go) return;  // (uniform: the solve has stopped)
  const int tid = threadIdx.x, slots = s.n_corner + s.n_surf, base = blockIdx.x * kWg, slot = base + tid;
  const int m = min(kWg, slots - base);
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();
  bool ok = false;
  if (slot < slots) {
    const double q[4] = {st->eval[0], st->eval[1], st->eval[2], st->eval[3]},
                 t[3] = {st->eval[4], st->eval[5], st->eval[6]};
    const float* p = slot < s.n_corner ? s.corner + 3 * (int64_t)slot : s.surf + 3 * (int64_t)(slot - s.n_corner);
    const int kind = s.kind[slot];
    double rec[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) rec[k] = s.rec[6 * (int64_t)slot + k];
    Factor f;
    ok = slot_factor(q, t, p, kind, rec, &f) != 0;
    if (kind == kEdge) atomicAdd(&cnt[0], 1);
    if (kind == kPlane) atomicAdd(&cnt[1], 1);
    if (kind == kDegenerate) atomicAdd(&cnt[2], 1);
    if (ok) {
      double v[kSums];
      if (aodom::contributions(f, v)) atomicAdd(&cnt[3], 1);
#pragma unroll
      for (int k = 0; k < kSums; ++k) c[k][tid] = v[k];
    }
  }
  valid[tid] = ok;
  __syncthreads();
  for (int task = tid; task < kSums * kLanes; task += kWg) {
    const int k = task / kLanes, l = task % kLanes;
    part[k][l] = lane_sum(c[k], 1, valid, 0, m, l);
  }
  __syncthreads();
  if (tid < kSums) P[(int64_t)blockIdx.x * kSums + tid] = lanes_total(part[tid]);
  if (tid < 4) cntP[4 * blockIdx.x + tid] = cnt[tid];
}

// One wavefront.  first / step: the controller's half steps around the sums
// of the evaluation just made; `last` ends a pass (and, for the second pass,
// the sweep); reduce: the sums alone, for the lockstep entry; finish:
// transformUpdate alone, for a sweep whose gate stayed shut.
__global__ void __launch_bounds__(64)
k_amap_control(MapState* st, const double* __restrict__ P, const int* __restrict__ cntP, int nwg, int phase, int pass,
               int last) {
  __shared__ double part[kSums][kLanes];
  __shared__ double sums[kSums];
  __shared__ int cnt[4];
  const int tid = threadIdx.x;
  const int go = st->go;
  if (go && phase != kPhaseFinish) {
    for (int task = tid; task < kSums * kLanes; task += 64) {
      const int k = task / kLanes, l = task % kLanes;
      part[k][l] = lane_sum(P + k, kSums, nullptr, 0, nwg, l);
    }
    if (tid < 4) {
      int v = 0;
      for (int w = 0; w < nwg; ++w) v += cntP[4 * w + tid];
      cnt[tid] = v;
    }
    __syncthreads();
    if (tid < kSums) sums[tid] = lanes_total(part[tid]);
  }
  __syncthreads();
  if (tid != 0) return;
  aodom::Lm* s = &st->lm;
  if (phase == kPhaseReduce) {
    for (int k = 0; k < kSums; ++k) st->sums[k] = sums[k];
    for (int k = 0; k < 4; ++k) st->cnt[k] = cnt[k];
    return;
  }
  slio_aloam_odom_pass* out = &st->res.pass[pass];
  if (phase == kPhaseFirst) {
    aodom::lm_init(s, st->eval, st->eval + 4);
    for (int k = 0; k < 21; ++k) s->A[k] = sums[k];
    for (int k = 0; k < 6; ++k) s->g[k] = sums[21 + k];
    s->cost = 0.5 * sums[27];
    out->corner = cnt[0];
    out->plane = cnt[1];
    out->degenerate = cnt[2];
    out->outliers = cnt[3];
    out->few = 0;
    out->cost_first = s->cost;
    for (int k = 0; k < aodom::kMaxIter; ++k) {
      for (int a = 0; a < 4; ++a) out->it_q[k][a] = 0.0;
      for (int a = 0; a < 3; ++a) out->it_t[k][a] = 0.0;
      out->it_cost[k] = out->it_mu[k] = 0.0;
    }
  } else if (phase == kPhaseStep && go) {
    aodom::lm_decide(s, sums, sums + 21, 0.5 * sums[27]);
    if (s->last_accepted) out->outliers = cnt[3];
    const int k = s->iterations - 1;  // 0 .. kMaxIter - 1
    for (int a = 0; a < 4; ++a) out->it_q[k][a] = s->q[a];
    for (int a = 0; a < 3; ++a) out->it_t[k][a] = s->t[a];
    out->it_cost[k] = s->cost;
    out->it_mu[k] = s->mu;
  }
  if (phase != kPhaseFinish && (phase == kPhaseFirst || go)) {
    st->go = aodom::lm_propose(s) ? 1 : 0;
    for (int a = 0; a < 4; ++a) st->eval[a] = s->qn[a];
    for (int a = 0; a < 3; ++a) st->eval[4 + a] = s->tn[a];
  }
  if (!last) return;
  if (phase != kPhaseFinish) {  // the pass ends: its pose is where the next association runs
    out->iterations = s->iterations;
    out->accepted = s->accepted;
    out->stop = s->stop;
    out->cost_last = s->cost;
    for (int a = 0; a < 4; ++a) st->q[a] = st->eval[a] = s->q[a];
    for (int a = 0; a < 3; ++a) st->t[a] = st->eval[4 + a] = s->t[a];
    st->go = 1;
  }
  if (pass == 1) {
    double qm[4], tm[3];
    transform_update(st->q, st->t, st->q_wodom, st->t_wodom, qm, tm);
    for (int a = 0; a < 4; ++a) {
      st->res.q_w_curr[a] = st->q[a];
      st->res.q_wmap_wodom[a] = qm[a];
    }
    for (int a = 0; a < 3; ++a) {
      st->res.t_w_curr[a] = st->t[a];
      st->res.t_wmap_wodom[a] = tm[a];
    }
  }
}

// :835-873 for one class: pointAssociateToMap at the solved pose, the cube of
// the float coordinate; outside the array or not finite = dropped
__global__ void k_amap_append(const float* __restrict__ in, int n, const double* __restrict__ pose, int cenI, int cenJ,
                              int cenK, float* __restrict__ x, float* __restrict__ y, float* __restrict__ z,
                              uint32_t* __restrict__ id) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
  float w[3];
  aodom::to_start(q, t, in + 3 * i, w);
  int ci, cj, ck;
  uint32_t c = lvx::kDrop;
  if (isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2]) && lvx::cube_of(w[0], cenI, &ci) &&
      lvx::cube_of(w[1], cenJ, &cj) && lvx::cube_of(w[2], cenK, &ck) && ci >= 0 && ci < kW && cj >= 0 && cj < kH &&
      ck >= 0 && ck < kD)
    c = (uint32_t)(ci + kW * cj + kW * kH * ck);
  x[i] = w[0];
  y[i] = w[1];
  z[i] = w[2];
  id[i] = c;
}

// :929-933: n x {x, y, z, intensity} into the map frame, the intensity kept
__global__ void k_amap_register(const float4* __restrict__ in, int64_t n, const double* __restrict__ pose,
                                float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double q[4] = {pose[0], pose[1], pose[2], pose[3]}, t[3] = {pose[4], pose[5], pose[6]};
  const float4 p = in[i];
  const float b[3] = {p.x, p.y, p.z};
  float w[3];
  aodom::to_start(q, t, b, w);
  out[i] = make_float4(w[0], w[1], w[2], p.w);
}

// a class of the store (SoA) as n x 3
__global__ void k_amap_interleave(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                  int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[3 * i] = x[i];
  out[3 * i + 1] = y[i];
  out[3 * i + 2] = z[i];
}

using lvx::blocks;

std::mutex g_live_mu;
std::set<void*> g_live;

struct HostBlock {  // pinned
  MapState st;
};

}  // namespace

struct slio_aloam_map {
  slio_aloam_map_params prm{};
  bool dev_counted = false;
  lvx::CubeStore store;
  MapState* st = nullptr;
  HostBlock* hb = nullptr;
  MapDev::Buf raw, stack[2], tmp;
  uint8_t* kind = nullptr;
  double *rec = nullptr, *P = nullptr;
  int32_t *idx = nullptr, *cntP = nullptr;
  float* sqd = nullptr;
  int n_stack[2] = {0, 0};
  int32_t cen[3] = {10, 10, 5};
  int32_t list[kMaxListed];
  int32_t nlist = 0;
  double q_wmap[4] = {0, 0, 0, 1}, t_wmap[3] = {0, 0, 0};
  double q_w[4] = {0, 0, 0, 1}, t_w[3] = {0, 0, 0};
  bool has_run = false, has_grid = false, has_assoc = false;
};

namespace {

void map_free(slio_aloam_map* h) {
  for (void* p : {(void*)h->st, (void*)h->kind, (void*)h->rec, (void*)h->P, (void*)h->idx, (void*)h->cntP,
                  (void*)h->sqd})
    if (p) (void)hipFree(p);
  for (MapDev::Buf* b : {&h->raw, &h->stack[0], &h->stack[1], &h->tmp})
    if (b->p) (void)hipFree(b->p);
  if (h->hb) (void)hipHostFree(h->hb);
  lvx::store_free(&h->store);
}

bool is_live(void* h) {
  std::lock_guard<std::mutex> g(g_live_mu);
  return g_live.count(h) != 0;
}

void reset_host(slio_aloam_map* h) {
  lvx::store_clear(&h->store);
  h->cen[0] = 10;
  h->cen[1] = 10;
  h->cen[2] = 5;
  const double id[7] = {0, 0, 0, 1, 0, 0, 0};
  std::memcpy(h->q_wmap, id, sizeof h->q_wmap);
  std::memcpy(h->t_wmap, id + 4, sizeof h->t_wmap);
  std::memcpy(h->q_w, id, sizeof h->q_w);
  std::memcpy(h->t_w, id + 4, sizeof h->t_w);
  h->n_stack[0] = h->n_stack[1] = 0;
  h->nlist = 0;
  h->has_run = h->has_grid = h->has_assoc = false;
}

Slots slots_of(const slio_aloam_map* h) {
  Slots s;
  s.corner = (const float*)h->stack[0].p;
  s.surf = (const float*)h->stack[1].p;
  s.n_corner = h->n_stack[0];
  s.n_surf = h->n_stack[1];
  s.kind = h->kind;
  s.rec = h->rec;
  s.idx = h->idx;
  s.sqd = h->sqd;
  return s;
}

// the association of both classes at the pose in device memory; no wait
void enqueue_associate(slio_aloam_map* h, const double* pose) {
  const Slots s = slots_of(h);
  hipStream_t st = h->store.stream;
  if (s.n_corner)
    k_amap_associate<0><<<blocks(s.n_corner), 256, 0, st>>>(h->store.grid[0].view,
                                                            (const float*)h->store.grid[0].xyz.p, s, pose);
  if (s.n_surf)
    k_amap_associate<1><<<blocks(s.n_surf), 256, 0, st>>>(h->store.grid[1].view, (const float*)h->store.grid[1].xyz.p,
                                                          s, pose);
}

int nwg_of(const slio_aloam_map* h) { return (h->n_stack[0] + h->n_stack[1] + kWg - 1) / kWg; }

void enqueue_evaluate(slio_aloam_map* h) {
  const int nwg = nwg_of(h);
  if (nwg) k_amap_evaluate<<<nwg, kWg, 0, h->store.stream>>>(slots_of(h), h->st, h->P, h->cntP);
}

bool finite_pose(const double* q, const double* t) {
  for (int k = 0; k < 4; ++k)
    if (!std::isfinite(q[k])) return false;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(t[k])) return false;
  return true;
}

// The sweep once the arguments are checked.  dev: the two clouds are device
// pointers (n x 4).
int sweep(slio_aloam_map* h, const float* corner, int n_corner, const float* surf, int n_surf, bool dev,
          const double q_wodom[4], const double t_wodom[3], slio_aloam_map_result* res, const char* who) {
  lvx::CubeStore* S = &h->store;
  hipStream_t st = S->stream;
  const int nin[2] = {n_corner, n_surf};
  for (int k = 0; k < 2; ++k)
    if (S->cls[k].n + nin[k] > h->prm.max_points) {
      set_error(std::string(who) + ": map and scan exceed max_points");
      return SLIO_ECAPACITY;
    }
  slio_aloam_map_result r;
  std::memset(&r, 0, sizeof r);
  double q[4], t[3];
  associate_to_map(h->q_wmap, h->t_wmap, q_wodom, t_wodom, q, t);  // :326
  int32_t cen[3] = {h->cen[0], h->cen[1], h->cen[2]}, list[kMaxListed], nlist = 0;
  if (select(t, cen, r.center, r.shift, list, &nlist)) {
    set_error(std::string(who) + ": position not finite or beyond 1e6 m");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  h->has_run = h->has_grid = h->has_assoc = false;  // (from here on the handle changes)
  std::memcpy(h->cen, cen, sizeof cen);
  std::memcpy(h->list, list, sizeof list);
  h->nlist = r.nvalid = nlist;
  if (r.shift[0] || r.shift[1] || r.shift[2])
    if (int rc = lvx::store_shift(S, r.shift, who)) return rc;
  // :597-607: the VoxelGrid of both incoming clouds
  const float* src[2] = {corner, surf};
  const float leaf[2] = {h->prm.leaf_corner, h->prm.leaf_surf};
  for (int k = 0; k < 2; ++k) {
    h->n_stack[k] = 0;
    if (!nin[k]) continue;
    hipError_t e = MapDev::take(h->tmp, 12 * (size_t)nin[k]);
    if (!e && !dev) e = MapDev::take(h->raw, 16 * (size_t)nin[k]);
    if (e) {
      set_error(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
    const float* d_src = src[k];
    if (!dev) {
      SLIO_HIP(hipMemcpyAsync(h->raw.p, src[k], 16 * (size_t)nin[k], hipMemcpyHostToDevice, st));
      d_src = (const float*)h->raw.p;
    }
    lvx::store_take_xyz(d_src, nin[k], (float*)h->tmp.p, st);
    int64_t total = 0;
    if (int rc = lvx::store_scan_voxel(S, (const float*)h->tmp.p, nin[k], leaf[k], &h->stack[k], &total, who))
      return rc;
    h->n_stack[k] = (int)total;
  }
  for (int k = 0; k < 2; ++k) {
    r.stack_size[k] = h->n_stack[k];
    int64_t m = 0;
    for (int i = 0; i < nlist; ++i) m += S->cls[k].off[list[i] + 1] - S->cls[k].off[list[i]];
    r.map_size[k] = (int32_t)m;
  }
  r.optimized = r.map_size[0] > 10 && r.map_size[1] > 50;  // :613
  // the sweep's state: the pose, the odometry's pose, go
  MapState* hs = &h->hb->st;
  std::memset(hs, 0, sizeof *hs);
  std::memcpy(hs->q, q, sizeof q);
  std::memcpy(hs->t, t, sizeof t);
  std::memcpy(hs->eval, q, sizeof q);
  std::memcpy(hs->eval + 4, t, sizeof t);
  std::memcpy(hs->q_wodom, q_wodom, sizeof hs->q_wodom);
  std::memcpy(hs->t_wodom, t_wodom, sizeof hs->t_wodom);
  hs->go = 1;
  hs->res = r;
  SLIO_HIP(hipMemcpyAsync(h->st, hs, sizeof *hs, hipMemcpyHostToDevice, st));
  if (r.optimized) {
    for (int k = 0; k < 2; ++k)
      if (int rc = lvx::store_build_grid(S, k, list, nlist, kCell, who)) return rc;
    h->has_grid = true;
    const int nwg = nwg_of(h);
    for (int pass = 0; pass < 2; ++pass) {
      enqueue_associate(h, h->st->q);
      enqueue_evaluate(h);
      k_amap_control<<<1, 64, 0, st>>>(h->st, h->P, h->cntP, nwg, kPhaseFirst, pass, 0);
      for (int it = 0; it < aodom::kMaxIter; ++it) {
        enqueue_evaluate(h);
        k_amap_control<<<1, 64, 0, st>>>(h->st, h->P, h->cntP, nwg, kPhaseStep, pass, it == aodom::kMaxIter - 1);
      }
    }
  } else {
    k_amap_control<<<1, 64, 0, st>>>(h->st, h->P, h->cntP, 0, kPhaseFinish, 1, 1);
  }
  SLIO_HIP(hipGetLastError());
  // :835-892: both stacks at the solved pose (read from device memory) behind
  // the stored points, then the VoxelGrid of the valid cubes
  for (int k = 0; k < 2; ++k) {
    lvx::StoreClass& c = S->cls[k];
    if (h->n_stack[k]) {
      float** s = c.xyz[c.cur];
      k_amap_append<<<blocks(h->n_stack[k]), 256, 0, st>>>((const float*)h->stack[k].p, h->n_stack[k], h->st->q,
                                                           h->cen[0], h->cen[1], h->cen[2], s[0] + c.n, s[1] + c.n,
                                                           s[2] + c.n, c.id[c.cur] + c.n);
    }
  }
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(&hs->res, &h->st->res, sizeof hs->res, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));  // the result
  if (int rc = lvx::store_upload_filter(S, list, nlist)) return rc;
  for (int k = 0; k < 2; ++k)
    if (int rc = lvx::store_rebuild(S, k, S->cls[k].n + h->n_stack[k], true, leaf[k], who)) return rc;
  *res = hs->res;
  std::memcpy(h->q_w, res->q_w_curr, sizeof h->q_w);
  std::memcpy(h->t_w, res->t_w_curr, sizeof h->t_w);
  std::memcpy(h->q_wmap, res->q_wmap_wodom, sizeof h->q_wmap);
  std::memcpy(h->t_wmap, res->t_wmap_wodom, sizeof h->t_wmap);
  h->has_run = true;
  return SLIO_OK;
}

int check_run_args(const slio_aloam_map* h, int64_t n_corner, int64_t n_surf, const double* q, const double* t,
                   const void* res, const char* who) {
  if (!res || n_corner < 0 || n_surf < 0 || !q || !t || !finite_pose(q, t) || !(sqnorm4(q) > 0.0)) {
    set_error(std::string(who) + ": null result, negative size, or a pose that is null, not finite or of zero norm");
    return SLIO_EINVAL;
  }
  if (n_corner > h->prm.max_scan || n_surf > h->prm.max_scan) {
    set_error(std::string(who) + ": a cloud beyond max_scan");
    return SLIO_ECAPACITY;
  }
  return SLIO_OK;
}

// the device pose block (7 doubles) of a lockstep call, through the pinned block
int upload_pose(slio_aloam_map* h, const double q[4], const double t[3], double* dst) {
  double* pose = h->hb->st.eval;  // (pinned; the stream is idle between calls)
  std::memcpy(pose, q, 4 * sizeof(double));
  std::memcpy(pose + 4, t, 3 * sizeof(double));
  SLIO_HIP(hipMemcpyAsync(dst, pose, 7 * sizeof(double), hipMemcpyHostToDevice, h->store.stream));
  return SLIO_OK;
}

}  // namespace

#define AMAP_CHECK(h, who)                                \
  do {                                                    \
    if (!(h) || !is_live(h)) {                            \
      set_error(who ": null or destroyed handle");        \
      return SLIO_EINVAL;                                 \
    }                                                     \
  } while (0)

extern "C" {

int slio_aloam_map_create(slio_aloam_map_handle* out, const slio_aloam_map_params* p) {
  if (!out || !p || p->max_points < 1 || p->max_scan < 1 || p->max_scan > 400000 || !(p->leaf_corner > 0.0f) ||
      !(p->leaf_surf > 0.0f) || !std::isfinite(p->leaf_corner) || !std::isfinite(p->leaf_surf) || p->device < 0) {
    set_error("slio_aloam_map_create: bad arguments (max_points >= 1, max_scan in 1 .. 400000, finite leaves > 0, "
              "device >= 0)");
    return SLIO_EINVAL;
  }
  int ndev = 0;
  SLIO_HIP(hipGetDeviceCount(&ndev));
  if (p->device >= ndev) {
    set_error("slio_aloam_map_create: no such device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(p->device));
  slio_aloam_map* h = new slio_aloam_map();
  h->prm = *p;
  h->store.W = kW;
  h->store.H = kH;
  h->store.D = kD;
  // (the store's class 2 takes a whole incoming cloud for its VoxelGrid)
  const size_t cap = (size_t)std::max(p->max_points, p->max_scan), slots = 2 * (size_t)p->max_scan;
  hipError_t e = lvx::store_alloc(&h->store, cap);
  if (!e) e = hipMalloc(&h->st, sizeof(MapState));
  if (!e) e = hipMalloc(&h->kind, slots);
  if (!e) e = hipMalloc(&h->rec, 48 * slots);
  if (!e) e = hipMalloc(&h->idx, 4 * kK * slots);
  if (!e) e = hipMalloc(&h->sqd, 4 * kK * slots);
  if (!e) e = hipMalloc(&h->P, 8 * kSums * ((slots + kWg - 1) / kWg));
  if (!e) e = hipMalloc(&h->cntP, 16 * ((slots + kWg - 1) / kWg));
  if (!e) e = hipHostMalloc(&h->hb, sizeof(HostBlock), hipHostMallocDefault);
  if (!e) e = hipMemsetAsync(h->st, 0, sizeof(MapState), h->store.stream);
  if (!e) e = hipStreamSynchronize(h->store.stream);
  if (e) {
    set_error(std::string("slio_aloam_map_create: ") + hipGetErrorString(e));
    map_free(h);
    delete h;
    return SLIO_ENOMEM;
  }
  reset_host(h);
  h->dev_counted = true;
  slio::dev_users(p->device, +1);
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    g_live.insert(h);
  }
  *out = h;
  return SLIO_OK;
}

int slio_aloam_map_destroy(slio_aloam_map_handle h) {
  if (!h) return SLIO_OK;
  {
    std::lock_guard<std::mutex> g(g_live_mu);
    if (!g_live.erase(h)) {
      set_error("slio_aloam_map_destroy: not a live handle");
      return SLIO_EINVAL;
    }
  }
  (void)hipSetDevice(h->prm.device);
  if (h->store.stream) (void)hipStreamSynchronize(h->store.stream);
  map_free(h);
  if (h->dev_counted) slio::dev_users(h->prm.device, -1);
  delete h;
  return SLIO_OK;
}

int slio_aloam_map_reset(slio_aloam_map_handle h) {
  AMAP_CHECK(h, "slio_aloam_map_reset");
  reset_host(h);
  return SLIO_OK;
}

int slio_aloam_map_run(slio_aloam_map_handle h, const float* corner_last, int64_t n_corner, const float* surf_last,
                       int64_t n_surf, const double q_wodom_curr[4], const double t_wodom_curr[3],
                       slio_aloam_map_result* res) {
  AMAP_CHECK(h, "slio_aloam_map_run");
  if ((n_corner > 0 && !corner_last) || (n_surf > 0 && !surf_last)) {
    set_error("slio_aloam_map_run: null cloud");
    return SLIO_EINVAL;
  }
  if (int rc = check_run_args(h, n_corner, n_surf, q_wodom_curr, t_wodom_curr, res, "slio_aloam_map_run")) return rc;
  return sweep(h, corner_last, (int)n_corner, surf_last, (int)n_surf, false, q_wodom_curr, t_wodom_curr, res,
               "slio_aloam_map_run");
}

int slio_aloam_map_run_view(slio_aloam_map_handle h, const slio_aloam_odom_view* v, const double q_wodom_curr[4],
                            const double t_wodom_curr[3], slio_aloam_map_result* res) {
  AMAP_CHECK(h, "slio_aloam_map_run_view");
  if (!v || v->n_corner < 0 || v->n_surf < 0 || (v->n_corner && !v->corner_last) || (v->n_surf && !v->surf_last)) {
    set_error("slio_aloam_map_run_view: null view, negative size or null cloud in the view");
    return SLIO_EINVAL;
  }
  if (v->device != h->prm.device) {
    set_error("slio_aloam_map_run_view: the view is of another device");
    return SLIO_EINVAL;
  }
  if (int rc = check_run_args(h, v->n_corner, v->n_surf, q_wodom_curr, t_wodom_curr, res, "slio_aloam_map_run_view"))
    return rc;
  return sweep(h, v->corner_last, v->n_corner, v->surf_last, v->n_surf, true, q_wodom_curr, t_wodom_curr, res,
               "slio_aloam_map_run_view");
}

int slio_aloam_map_register_cloud(slio_aloam_map_handle h, const float* xyzi, int64_t n, int on_device, float* out) {
  AMAP_CHECK(h, "slio_aloam_map_register_cloud");
  if (n < 0 || (n && (!xyzi || !out))) {
    set_error("slio_aloam_map_register_cloud: negative size or null cloud");
    return SLIO_EINVAL;
  }
  if (n > h->prm.max_scan) {
    set_error("slio_aloam_map_register_cloud: a cloud beyond max_scan");
    return SLIO_ECAPACITY;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_register_cloud: no sweep before");
    return SLIO_ESTATE;
  }
  if (!n) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t st = h->store.stream;
  hipError_t e = MapDev::take(h->tmp, 16 * (size_t)n);
  if (!e && !on_device) e = MapDev::take(h->raw, 16 * (size_t)n);
  if (e) {
    set_error(std::string("slio_aloam_map_register_cloud: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  const float* src = xyzi;
  if (!on_device) {
    SLIO_HIP(hipMemcpyAsync(h->raw.p, xyzi, 16 * (size_t)n, hipMemcpyHostToDevice, st));
    src = (const float*)h->raw.p;
  }
  k_amap_register<<<blocks(n), 256, 0, st>>>((const float4*)src, n, h->st->q, (float4*)h->tmp.p);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(out, h->tmp.p, 16 * (size_t)n, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));
  return SLIO_OK;
}

int slio_aloam_map_get_cube(slio_aloam_map_handle h, int kind, int32_t cube, float* xyz, int64_t cap, int64_t* n) {
  AMAP_CHECK(h, "slio_aloam_map_get_cube");
  if ((kind != 0 && kind != 1) || cube < 0 || cube >= kNum || cap < 0) {
    set_error("slio_aloam_map_get_cube: kind outside {0, 1}, cube outside the array or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_get_cube: no sweep before");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  return lvx::store_download(&h->store, kind, &cube, 1, xyz, cap, n, "slio_aloam_map_get_cube");
}

int slio_aloam_map_cube_sizes(slio_aloam_map_handle h, int kind, int32_t* sizes) {
  AMAP_CHECK(h, "slio_aloam_map_cube_sizes");
  if ((kind != 0 && kind != 1) || !sizes) {
    set_error("slio_aloam_map_cube_sizes: kind outside {0, 1} or null output");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_cube_sizes: no sweep before");
    return SLIO_ESTATE;
  }
  const lvx::StoreClass& c = h->store.cls[kind];
  for (int i = 0; i < kNum; ++i) sizes[i] = (int32_t)(c.off[i + 1] - c.off[i]);
  return SLIO_OK;
}

int slio_aloam_map_get_surround(slio_aloam_map_handle h, int kind, float* xyz, int64_t cap, int64_t* n) {
  AMAP_CHECK(h, "slio_aloam_map_get_surround");
  if ((kind != 0 && kind != 1) || cap < 0) {
    set_error("slio_aloam_map_get_surround: kind outside {0, 1} or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_get_surround: no sweep before");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  return lvx::store_download(&h->store, kind, h->list, h->nlist, xyz, cap, n, "slio_aloam_map_get_surround");
}

int slio_aloam_map_get_map(slio_aloam_map_handle h, int kind, float* xyz, int64_t cap, int64_t* n) {
  AMAP_CHECK(h, "slio_aloam_map_get_map");
  if ((kind != 0 && kind != 1) || cap < 0) {
    set_error("slio_aloam_map_get_map: kind outside {0, 1} or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_get_map: no sweep before");
    return SLIO_ESTATE;
  }
  const lvx::StoreClass& c = h->store.cls[kind];  // (sorted by cube: the whole class is the cubes in index order)
  if (n) *n = c.n;
  if (!xyz || !c.n) return SLIO_OK;
  if (cap < c.n) {
    set_error("slio_aloam_map_get_map: the output holds fewer points than the map");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  if (hipError_t e = MapDev::take(h->store.out, 12 * (size_t)c.n)) {
    set_error(std::string("slio_aloam_map_get_map: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  float* const* s = c.xyz[c.cur];
  k_amap_interleave<<<blocks(c.n), 256, 0, h->store.stream>>>(s[0], s[1], s[2], c.n, (float*)h->store.out.p);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(xyz, h->store.out.p, 12 * (size_t)c.n, hipMemcpyDeviceToHost, h->store.stream));
  SLIO_HIP(hipStreamSynchronize(h->store.stream));
  return SLIO_OK;
}

int slio_aloam_map_get_stack(slio_aloam_map_handle h, int kind, float* xyz, int64_t cap, int64_t* n) {
  AMAP_CHECK(h, "slio_aloam_map_get_stack");
  if ((kind != 0 && kind != 1) || cap < 0) {
    set_error("slio_aloam_map_get_stack: kind outside {0, 1} or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_run) {
    set_error("slio_aloam_map_get_stack: no sweep before");
    return SLIO_ESTATE;
  }
  const int m = h->n_stack[kind];
  if (n) *n = m;
  if (!xyz || !m) return SLIO_OK;
  if (cap < m) {
    set_error("slio_aloam_map_get_stack: the output holds fewer points than the cloud");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  SLIO_HIP(hipMemcpyAsync(xyz, h->stack[kind].p, 12 * (size_t)m, hipMemcpyDeviceToHost, h->store.stream));
  SLIO_HIP(hipStreamSynchronize(h->store.stream));
  return SLIO_OK;
}

int slio_aloam_map_associate(slio_aloam_map_handle h, const double q[4], const double t[3]) {
  AMAP_CHECK(h, "slio_aloam_map_associate");
  if (!q || !t || !finite_pose(q, t)) {
    set_error("slio_aloam_map_associate: a pose that is null or not finite");
    return SLIO_EINVAL;
  }
  if (!h->has_run || !h->has_grid) {
    set_error("slio_aloam_map_associate: no sweep before, or its gate stayed shut");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  if (int rc = upload_pose(h, q, t, h->st->eval)) return rc;  // (the sweep's pose stays in st->q)
  enqueue_associate(h, h->st->eval);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipStreamSynchronize(h->store.stream));
  h->has_assoc = true;
  return SLIO_OK;
}

int slio_aloam_map_get_association(slio_aloam_map_handle h, uint8_t* kind, double* rec, int32_t* nbr_idx,
                                   float* nbr_sqd, int64_t cap_slots, int32_t* n) {
  AMAP_CHECK(h, "slio_aloam_map_get_association");
  if (!n || cap_slots < 0) {
    set_error("slio_aloam_map_get_association: null count or negative capacity");
    return SLIO_EINVAL;
  }
  if (!h->has_assoc) {
    set_error("slio_aloam_map_get_association: no association since the last sweep");
    return SLIO_ESTATE;
  }
  const size_t m = (size_t)(h->n_stack[0] + h->n_stack[1]);
  *n = (int32_t)m;
  if ((int64_t)m > cap_slots) {
    set_error("slio_aloam_map_get_association: the output holds fewer slots than the association");
    return SLIO_ECAPACITY;
  }
  if (!m) return SLIO_OK;
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t st = h->store.stream;
  if (kind) SLIO_HIP(hipMemcpyAsync(kind, h->kind, m, hipMemcpyDeviceToHost, st));
  if (rec) SLIO_HIP(hipMemcpyAsync(rec, h->rec, 48 * m, hipMemcpyDeviceToHost, st));
  if (nbr_idx) SLIO_HIP(hipMemcpyAsync(nbr_idx, h->idx, 4 * kK * m, hipMemcpyDeviceToHost, st));
  if (nbr_sqd) SLIO_HIP(hipMemcpyAsync(nbr_sqd, h->sqd, 4 * kK * m, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));
  return SLIO_OK;
}

int slio_aloam_map_evaluate(slio_aloam_map_handle h, const double q[4], const double t[3], double A[21], double g[6],
                            double* cost, int32_t counts[4]) {
  AMAP_CHECK(h, "slio_aloam_map_evaluate");
  if (!q || !t || !A || !g || !cost || !counts || !finite_pose(q, t)) {
    set_error("slio_aloam_map_evaluate: null output, or a pose that is null or not finite");
    return SLIO_EINVAL;
  }
  if (!h->has_assoc) {
    set_error("slio_aloam_map_evaluate: no association since the last sweep");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(h->prm.device));
  hipStream_t st = h->store.stream;
  if (int rc = upload_pose(h, q, t, h->st->eval)) return rc;
  h->hb->st.go = 1;
  SLIO_HIP(hipMemcpyAsync(&h->st->go, &h->hb->st.go, sizeof(int), hipMemcpyHostToDevice, st));
  enqueue_evaluate(h);
  k_amap_control<<<1, 64, 0, st>>>(h->st, h->P, h->cntP, nwg_of(h), kPhaseReduce, 0, 0);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(h->hb->st.sums, h->st->sums, sizeof(double) * kSums + sizeof(int) * 4, hipMemcpyDeviceToHost,
                          st));
  SLIO_HIP(hipStreamSynchronize(st));
  std::memcpy(A, h->hb->st.sums, 21 * sizeof(double));
  std::memcpy(g, h->hb->st.sums + 21, 6 * sizeof(double));
  *cost = 0.5 * h->hb->st.sums[27];
  for (int k = 0; k < 4; ++k) counts[k] = h->hb->st.cnt[k];
  return SLIO_OK;
}

}  // extern "C"
