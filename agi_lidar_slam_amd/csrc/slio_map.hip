// slio_map.hip -- the map of the IKF runtime on the MI355X (gfx950): the dense
// uniform-grid index the search pass (slio_device.hip) reads, and its upkeep.
//
//   * the index build: cell-sorted points {x, y, z, bits(id)}, the cell table,
//     the coarse level (cells of edge 4h with tight boxes) and the block rows
//     (build_index, build_blk);
//   * the live map: ikd-Tree's Add_Points and Delete_Point_Boxes and
//     laserMapping's map_incremental (k_ds_*, k_map_*, k_append*), applied as
//     keep flags and pending additions;
//   * the rebuild before the next search pass or download (map_refresh): a
//     merge into the kept grid (k_merge_*) or a sorting rebuild;
//   * sharing one map among handles (map_write_begin / _end, map_read_sync,
//     map_attach) and the slio_map_* C ABI.
//
// What this file, slio_device.hip, slio_scan.hip and the mapping back-ends use
// of one another is declared in slio_device.hpp.
// Built like slio_device.hip, with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "slio_common.hpp"
#include "slio_device.hpp"
#include "slio_fkey.hpp"

namespace slio {

// ---------------------------------------------------------------- map index
// per-cell counts of SORTED keys (cell = key >> shift): one atomic per run of
// equal cells inside a wavefront (sorted keys put up to 64 lanes on one
// counter; per-lane atomics serialised there: 0.64 ms for the coarse level
// of a 10M map)
template <typename K>
__global__ void k_cell_hist_sorted(const K* __restrict__ keys, int64_t n, int shift,
                                   uint32_t* __restrict__ counts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = i < n;
  const uint32_t c = live ? (uint32_t)(keys[i] >> shift) : 0xFFFFFFFFu;
  const int lane = threadIdx.x & 63;
  const uint32_t prev = __shfl_up(c, 1, 64);
  const bool head = live && (lane == 0 || prev != c);
  const uint64_t heads = __ballot(head);
  const uint64_t livem = __ballot(live);
  if (head) {
    const uint64_t above = lane == 63 ? 0ull : heads & ~((2ull << lane) - 1ull);
    const int end = above ? __ffsll((long long)above) - 1 : 64 - __clzll((long long)livem);
    atomicAdd(&counts[c], (uint32_t)(end - lane));
  }
}

// block rows: entry sizes, then the fill, one thread per cell.  A source
// row (y + j, z + k) whose start[] is equal at both ends of a segment of
// kBlkSeg x cells is empty there: k_blk_live marks the live rows per segment
// (2 loads a row), and the cell threads read only those (95 % of a 10M
// street map's 33M cells are empty; every cell thread used to spend 18 loads).
// Sources in (z, y) order, each cell's points in pts order.
constexpr int kBlkSeg = 16;
__device__ __forceinline__ uint32_t blk_rows_live(const uint32_t* __restrict__ start, GridGeom g, int x0,
                                                  int x1, int y, int z) {
  uint32_t live = 0;
  for (int k = -1; k <= 1; ++k)
    for (int j = -1; j <= 1; ++j) {
      const int yy = y + j, zz = z + k;
      const int q = (k + 1) * 3 + (j + 1);
      if (yy < 0 || yy >= g.dy || zz < 0 || zz >= g.dz) continue;
      const int64_t rb = ((int64_t)zz * g.dy + yy) * g.dx;
      if (start[rb + x1] != start[rb + x0]) live |= 1u << q;
    }
  return live;
}

// live source rows of every segment (9 bits)
__global__ void k_blk_live(const uint32_t* __restrict__ start, GridGeom g, int64_t nseg,
                           uint16_t* __restrict__ live) {
  const int64_t sg = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (sg >= nseg) return;
  const int segs = (g.dx + kBlkSeg - 1) / kBlkSeg;
  const int x0 = (int)(sg % segs) * kBlkSeg, x1 = min(x0 + kBlkSeg, g.dx);
  const int y = (int)((sg / segs) % g.dy);
  const int z = (int)(sg / ((int64_t)segs * g.dy));
  live[sg] = (uint16_t)blk_rows_live(start, g, x0, x1, y, z);
}

// one thread per cell; only the segment's live source rows are read
__global__ void k_blk_count(const uint32_t* __restrict__ start, const uint16_t* __restrict__ live,
                            GridGeom g, int64_t ncells, uint32_t* __restrict__ cnt9) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  const int x = (int)(c % g.dx);
  const int64_t row = c / g.dx;
  const int segs = (g.dx + kBlkSeg - 1) / kBlkSeg;
  uint32_t m = live[row * segs + x / kBlkSeg];
  uint32_t s = 0;
  const int y = (int)(row % g.dy), z = (int)(row / g.dy);
  for (; m; m &= m - 1) {
    const int q = __ffs(m) - 1;
    const int64_t sc = ((int64_t)(z + q / 3 - 1) * g.dy + (y + q % 3 - 1)) * g.dx + x;
    s += start[sc + 1] - start[sc];
  }
  cnt9[c] = s;
}

__global__ void k_blk_fill(const float4* __restrict__ pts, const uint32_t* __restrict__ start,
                           const uint16_t* __restrict__ live, const uint32_t* __restrict__ bstart,
                           GridGeom g, int64_t ncells, float4* __restrict__ blk) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  const int x = (int)(c % g.dx);
  const int64_t row = c / g.dx;
  const int segs = (g.dx + kBlkSeg - 1) / kBlkSeg;
  uint32_t m = live[row * segs + x / kBlkSeg];
  if (!m) return;
  const int y = (int)(row % g.dy), z = (int)(row / g.dy);
  uint32_t o = bstart[c];
  for (; m; m &= m - 1) {
    const int q = __ffs(m) - 1;
    const int64_t sc = ((int64_t)(z + q / 3 - 1) * g.dy + (y + q % 3 - 1)) * g.dx + x;
    for (uint32_t p = start[sc]; p < start[sc + 1]; ++p) {
      const float4 v = pts[p];
      blk[o++] = make_float4(v.x, v.y, v.z, __uint_as_float(p));
    }
  }
}

// coarse level: cell keys of the fine-sorted points, then the gather (values
// are fine positions, ascending inside a coarse cell after the stable sort)
__global__ void k_coarse_keys(const float4* __restrict__ pts, int64_t n, GridGeom cg,
                              uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = pts[i];
  int cx = min(max(cell_coord(p.x, cg.ox, cg.inv_h), 0), cg.dx - 1);
  int cy = min(max(cell_coord(p.y, cg.oy, cg.inv_h), 0), cg.dy - 1);
  int cz = min(max(cell_coord(p.z, cg.oz, cg.inv_h), 0), cg.dz - 1);
  keys[i] = ((uint32_t)cz * (uint32_t)cg.dy + (uint32_t)cy) * (uint32_t)cg.dx + (uint32_t)cx;
  vals[i] = (uint32_t)i;
}

// Coarse level without a sort.  A coarse cell (edge 4h, same origin) is the
// 4x4x4 fine cells [4c, 4c + 4) per axis, clipped to the fine grid, so its
// points are the fine runs of its 16 (y, z) rows -- each a contiguous x-range
// of cells of the cell-sorted pts -- and taking the rows in order lists them in
// fine position order, the order a stable sort by coarse cell gave.  (A point
// lies within tol of its fine cell, hence of that cell's coarse cell; the far
// search's bounds carry the same tol.)
__device__ __forceinline__ void coarse_decode(const GridGeom& cg, int64_t c, int& x, int& y, int& z) {
  x = (int)(c % cg.dx);
  const int64_t t = c / cg.dx;
  y = (int)(t % cg.dy);
  z = (int)(t / cg.dy);
}
__global__ void k_coarse_count(const uint32_t* __restrict__ start, GridGeom g, GridGeom cg, int64_t nc,
                               uint32_t* __restrict__ cnt) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c == 0) cnt[nc] = 0;
  if (c >= nc) return;
  int cx, cy, cz;
  coarse_decode(cg, c, cx, cy, cz);
  const int x0 = 4 * cx, x1 = min(4 * cx + 4, g.dx);
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const int fy = 4 * cy + (k & 3), fz = 4 * cz + (k >> 2);
    if (fy < g.dy && fz < g.dz) {
      const int64_t rb = ((int64_t)fz * g.dy + fy) * g.dx;
      sum += start[rb + x1] - start[rb + x0];
    }
  }
  cnt[c] = sum;
}
// one wavefront per 64 coarse cells: each lane reads its cell's size
// (k_coarse_count; empty cells -- most of a surface map's -- are written by
// their lane at once), then 16-lane groups read the non-empty cells' rows,
// four cells at a time, and form their tight boxes (count in lo.w).
__global__ void k_coarse_boxes(const float4* __restrict__ pts, const uint32_t* __restrict__ start, GridGeom g,
                               GridGeom cg, const uint32_t* __restrict__ cnt, int64_t nc,
                               float4* __restrict__ lo, float4* __restrict__ hi) {
  const int64_t c_base = (((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) << 6;
  const int lane = threadIdx.x & 63;
  const float INF = __int_as_float(0x7f800000);
  const int64_t mc = c_base + lane;
  uint32_t mt = 0;
  if (mc < nc) {
    mt = cnt[mc];
    if (mt == 0) {
      lo[mc] = make_float4(INF, INF, INF, __uint_as_float(0u));
      hi[mc] = make_float4(-INF, -INF, -INF, 0.0f);
    }
  }
  // the non-empty cells, four at a time: 16 lanes per cell (lane r of a
  // group fetches row r's bounds), most cells hold a few dozen points
  const uint64_t busy = __ballot(mc < nc && mt != 0);
  const int nbusy = __popcll(busy);
  const int gi = lane >> 4, sl = lane & 15;
  for (int k0 = 0; k0 < nbusy; k0 += 4) {
    const int kk = k0 + gi;
    const bool act = kk < nbusy;
    uint64_t bm = busy;
    for (int q = 0; q < kk && bm; ++q) bm &= bm - 1;  // the kk-th set bit
    const int l = (act && bm) ? __ffsll((unsigned long long)bm) - 1 : 0;
    const int64_t c = c_base + l;
    // (every lane shuffles: a cross-lane read inside a condition would read
    // lanes the condition turned off)
    const uint32_t tsrc = __shfl(mt, l, 64);
    const uint32_t total = act ? tsrc : 0u;
    int cx, cy, cz;
    coarse_decode(cg, c, cx, cy, cz);
    const int x0 = 4 * cx, x1 = min(4 * cx + 4, g.dx);
    uint32_t rs = 0, len = 0;
    {
      const int fy = 4 * cy + (sl & 3), fz = 4 * cz + (sl >> 2);
      if (act && fy < g.dy && fz < g.dz) {
        const int64_t rb = ((int64_t)fz * g.dy + fy) * g.dx;
        rs = start[rb + x0];
        len = start[rb + x1] - rs;
      }
    }
    uint32_t inc = len;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const uint32_t v = __shfl_up(inc, o, 16);
      if (sl >= o) inc += v;
    }
    const uint32_t excl = inc - len;
    float l3[3] = {INF, INF, INF}, u3[3] = {-INF, -INF, -INF};
    // the cell's points as one flat list over its rows: lane j of the group
    // takes list entries j, j + 16, ... (row r = the last row starting at or
    // before the entry)
    uint32_t E[16], S[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      E[r] = __shfl(excl, r, 16);
      S[r] = __shfl(rs, r, 16) - E[r];  // list entry j of row r is pts[S[r] + j]
    }
    for (uint32_t j = sl; j < total; j += 16) {
      uint32_t src = S[0] + j;
#pragma unroll
      for (int r = 1; r < 16; ++r) src = (j >= E[r]) ? S[r] + j : src;
      const float4 v = pts[src];
      l3[0] = fminf(l3[0], v.x);
      l3[1] = fminf(l3[1], v.y);
      l3[2] = fminf(l3[2], v.z);
      u3[0] = fmaxf(u3[0], v.x);
      u3[1] = fmaxf(u3[1], v.y);
      u3[2] = fmaxf(u3[2], v.z);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) {
        l3[a] = fminf(l3[a], __shfl_xor(l3[a], o, 16));
        u3[a] = fmaxf(u3[a], __shfl_xor(u3[a], o, 16));
      }
    if (sl == 0 && act) {
      lo[c] = make_float4(l3[0], l3[1], l3[2], __uint_as_float(total));
      hi[c] = make_float4(u3[0], u3[1], u3[2], 0.0f);
    }
  }
}

// float min / max by compare-and-swap (vector atomics): the coarse boxes of
// a merge rebuild's additions
__device__ __forceinline__ void atomic_fmin(float* a, float v) {
  int* ai = reinterpret_cast<int*>(a);
  int old = __hip_atomic_load(ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (v < __int_as_float(old)) {
    const int prev = atomicCAS(ai, old, __float_as_int(v));
    if (prev == old) break;
    old = prev;
  }
}
__device__ __forceinline__ void atomic_fmax(float* a, float v) {
  int* ai = reinterpret_cast<int*>(a);
  int old = __hip_atomic_load(ai, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (v > __int_as_float(old)) {
    const int prev = atomicCAS(ai, old, __float_as_int(v));
    if (prev == old) break;
    old = prev;
  }
}
// widen the boxes (and counts) of the coarse cells the na additions fall in;
// a point's coarse cell is its (clamped) fine cell / 4 on every axis
__global__ void k_coarse_extend(const float4* __restrict__ adds, const uint8_t* __restrict__ keep, int64_t na,
                                GridGeom g, float4* __restrict__ lo, float4* __restrict__ hi, GridGeom cg) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= na || (keep && !keep[i])) return;
  const float4 v = adds[i];
  const int fx = min(max(cell_coord(v.x, g.ox, g.inv_h), 0), g.dx - 1);
  const int fy = min(max(cell_coord(v.y, g.oy, g.inv_h), 0), g.dy - 1);
  const int fz = min(max(cell_coord(v.z, g.oz, g.inv_h), 0), g.dz - 1);
  const int64_t c = ((int64_t)(fz >> 2) * cg.dy + (fy >> 2)) * cg.dx + (fx >> 2);
  float* l = reinterpret_cast<float*>(lo + c);
  float* h = reinterpret_cast<float*>(hi + c);
  atomic_fmin(l + 0, v.x);
  atomic_fmin(l + 1, v.y);
  atomic_fmin(l + 2, v.z);
  atomic_fmax(h + 0, v.x);
  atomic_fmax(h + 1, v.y);
  atomic_fmax(h + 2, v.z);
  atomicAdd(reinterpret_cast<unsigned int*>(l + 3), 1u);
}

// Map sharing: stream ordering of changes and reads (MapDev::mu held by the
// caller: exclusively for map_write_begin / _end, either way for
// map_read_sync).
int map_write_begin(Ctx& c) {
  MapDev& m = *c.map;
  for (Ctx* u : m.users) {
    if (u == &c || u->stream == c.stream) continue;
    if (!u->map_ev) SLIO_HIP(hipEventCreateWithFlags(&u->map_ev, hipEventDisableTiming));
    SLIO_HIP(hipEventRecord(u->map_ev, u->stream));
    SLIO_HIP(hipStreamWaitEvent(c.stream, u->map_ev, 0));
  }
  if (m.ready && c.seen_epoch != m.epoch) SLIO_HIP(hipStreamWaitEvent(c.stream, m.ready, 0));
  return SLIO_OK;
}
int map_write_end(Ctx& c) {
  MapDev& m = *c.map;
  if (!m.ready) SLIO_HIP(hipEventCreateWithFlags(&m.ready, hipEventDisableTiming));
  SLIO_HIP(hipEventRecord(m.ready, c.stream));
  c.seen_epoch = ++m.epoch;
  return SLIO_OK;
}
int map_read_sync(Ctx& c) {
  MapDev& m = *c.map;
  if (c.seen_epoch != m.epoch) {
    if (m.ready) SLIO_HIP(hipStreamWaitEvent(c.stream, m.ready, 0));
    c.seen_epoch = m.epoch;
  }
  if (m.broken) {
    set_error("slio map: an index rebuild failed part-way; upload the map again");
    return SLIO_EDEVICE;
  }
  return SLIO_OK;
}
// attach c to map m (nullptr: detach), keeping the users list
void map_attach(Ctx& c, std::shared_ptr<MapDev> m) {
  if (c.map) {
    std::unique_lock<std::shared_mutex> lk(c.map->mu);
    auto& u = c.map->users;
    u.erase(std::remove(u.begin(), u.end(), &c), u.end());
  }
  c.map = std::move(m);
  c.seen_epoch = 0;  // the new map's last change is not yet waited for
  if (c.map) {
    std::unique_lock<std::shared_mutex> lk(c.map->mu);
    c.map->users.push_back(&c);
  }
}

// ---------------------------------------------------------------- map index build

__global__ void k_pack_ids(const float* __restrict__ x, const float* __restrict__ y,
                           const float* __restrict__ z, int64_t n, uint32_t id0, float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = make_float4(x[i], y[i], z[i], __uint_as_float(id0 + (uint32_t)i));
}

// sort key (cell << idbits) | id: the cell-sorted map keeps ascending ids
// inside a cell (the tie order of the kNN keys), whatever order the points
// come in
__global__ void k_cell_keys64(const float4* __restrict__ in, int64_t n, GridGeom g, int idbits,
                              uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  const int cx = min(max(cell_coord(p.x, g.ox, g.inv_h), 0), g.dx - 1);
  const int cy = min(max(cell_coord(p.y, g.oy, g.inv_h), 0), g.dy - 1);
  const int cz = min(max(cell_coord(p.z, g.oz, g.inv_h), 0), g.dz - 1);
  const uint64_t cell = ((uint64_t)cz * (uint64_t)g.dy + (uint64_t)cy) * (uint64_t)g.dx + (uint64_t)cx;
  keys[i] = (cell << idbits) | (uint64_t)__float_as_uint(p.w);
  vals[i] = (uint32_t)i;
}

__global__ void k_gather4(const float4* __restrict__ in, const uint32_t* __restrict__ order, int64_t n,
                          float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = in[order[i]];
}

// bounding box: out[0..2] min keys, out[3..5] max keys; out[6] = 1 if a
// coordinate is not finite
__global__ void k_bbox4(const float4* __restrict__ in, int64_t n, int32_t* __restrict__ out) {
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  int bad = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = in[i];
    const float c[3] = {p.x, p.y, p.z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      bad |= !isfinite(c[a]);
      const int32_t k = fkey(c[a]);
      lo[a] = min(lo[a], k);
      hi[a] = max(hi[a], k);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int d = 32; d > 0; d >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], d, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], d, 64));
    }
  }
  bad = __any(bad);
  // one set of atomics per workgroup: the 6 counters are shared by the
  // whole grid, and same-address atomics serialise (one per wavefront of a
  // 2048-block grid took 0.58 ms on a 10M-point map)
  __shared__ int32_t wl[3][4], wh[3][4];
  __shared__ int wb[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      wl[a][w] = lo[a];
      wh[a][w] = hi[a];
    }
    wb[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int a = threadIdx.x;
    int32_t l = wl[a][0], h = wh[a][0];
    for (int q = 1; q < (int)(blockDim.x >> 6); ++q) {
      l = min(l, wl[a][q]);
      h = max(h, wh[a][q]);
    }
    atomicMin(out + a, l);
    atomicMax(out + 3 + a, h);
  } else if (threadIdx.x == 3) {
    int b = 0;
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) b |= wb[q];
    if (b) atomicOr(out + 6, 1);
  }
}

__global__ void k_fill_u8(uint8_t* __restrict__ p, int64_t n, uint8_t v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

__global__ void k_widen_flags(const uint8_t* __restrict__ k, int64_t n, uint32_t* __restrict__ f) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) f[i] = k[i] ? 1u : 0u;
}

int grid_blocks(int64_t n) { return (int)std::max<int64_t>(1, (n + 255) / 256); }

void pack_ids(const float* x, const float* y, const float* z, int64_t n, float4* out, hipStream_t st) {
  k_pack_ids<<<grid_blocks(n), 256, 0, st>>>(x, y, z, n, 0u, out);
}

// ---- survivor ranks straight from the keep bytes (the merge rebuild's
// exclusive prefix count of the stored points): per-tile counts, one
// workgroup's scan of the tile counts, then each tile's ranks -- 10 + 10 MB
// read and 40 MB written for the 10M map (the flags widened to 32 bits and a
// device-wide scan moved ~170 MB in ~110 us)
constexpr int kRankTile = 4096;  // keep bytes per workgroup: 256 threads x 16
__device__ __forceinline__ uint32_t nz_bytes(uint32_t w) {  // per byte: 0x80 when non-zero
  return (((w & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | w) & 0x80808080u;
}
__device__ __forceinline__ uint4 load_keep16(const uint8_t* __restrict__ keep, int64_t i, int64_t n) {
  if (i + 16 <= n) return *reinterpret_cast<const uint4*>(keep + i);
  uint32_t w[4] = {0, 0, 0, 0};
  for (int b = 0; b < 16 && i + b < n; ++b) w[b >> 2] |= (uint32_t)(keep[i + b] != 0) << (8 * (b & 3));
  return make_uint4(w[0], w[1], w[2], w[3]);
}
// block-wide exclusive sum of one value per thread (256 threads); *total gets the sum
__device__ __forceinline__ uint32_t block_excl_256(uint32_t v, uint32_t* total) {
  __shared__ uint32_t ws[4];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  uint32_t s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t u = __shfl_up(s, d, 64);
    if (lane >= d) s += u;
  }
  if (lane == 63) ws[w] = s;
  __syncthreads();
  uint32_t off = 0;
  for (int k = 0; k < w; ++k) off += ws[k];
  if (total) *total = ws[0] + ws[1] + ws[2] + ws[3];
  __syncthreads();
  return off + s - v;
}
// tcnt[t] = tile t's survivors; tcnt[nt + 1], tcnt[nt + 2] zeroed (k_merge_keys'
// live count and edge flag)
__global__ __launch_bounds__(256) void k_keep_tiles(const uint8_t* __restrict__ keep, int64_t n, int64_t nt,
                                                    uint32_t* __restrict__ tcnt) {
  const uint4 v = load_keep16(keep, (int64_t)blockIdx.x * kRankTile + threadIdx.x * 16, n);
  const uint32_t c = __popc(nz_bytes(v.x)) + __popc(nz_bytes(v.y)) + __popc(nz_bytes(v.z)) + __popc(nz_bytes(v.w));
  uint32_t tot;
  (void)block_excl_256(c, &tot);
  if (threadIdx.x == 0) tcnt[blockIdx.x] = tot;
  if (blockIdx.x == 0 && threadIdx.x < 2) tcnt[nt + 1 + threadIdx.x] = 0;
}
// in place: tcnt[0..nt) -> exclusive prefix, tcnt[nt] = the total (one
// workgroup: O(nt); summing the earlier tiles' counts in every rank
// workgroup instead was O(nt^2) -- 73M loads for a 50M map)
__global__ __launch_bounds__(256) void k_tile_scan(uint32_t* __restrict__ tcnt, int64_t nt) {
  const int64_t per = (nt + 255) / 256, a = min((int64_t)threadIdx.x * per, nt), b = min(a + per, nt);
  uint32_t s = 0;
  for (int64_t i = a; i < b; ++i) s += tcnt[i];
  uint32_t tot;
  uint32_t run = block_excl_256(s, &tot);
  for (int64_t i = a; i < b; ++i) {
    const uint32_t v = tcnt[i];
    tcnt[i] = run;
    run += v;
  }
  if (threadIdx.x == 0) tcnt[nt] = tot;
}
// rank[i] = survivors before i: the tile's base plus the exclusive count
// within the tile
__global__ __launch_bounds__(256) void k_keep_rank(const uint8_t* __restrict__ keep, int64_t n,
                                                   const uint32_t* __restrict__ tbase, uint32_t* __restrict__ rank) {
  const int64_t i0 = (int64_t)blockIdx.x * kRankTile + threadIdx.x * 16;
  const uint4 v = load_keep16(keep, i0, n);
  const uint32_t m[4] = {nz_bytes(v.x), nz_bytes(v.y), nz_bytes(v.z), nz_bytes(v.w)};
  const uint32_t c = __popc(m[0]) + __popc(m[1]) + __popc(m[2]) + __popc(m[3]);
  uint32_t r = tbase[blockIdx.x] + block_excl_256(c, nullptr);
  uint32_t o[16];
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    o[b] = r;
    r += (m[b >> 2] >> (8 * (b & 3) + 7)) & 1u;
  }
  if (i0 + 16 <= n) {
    uint4* d = reinterpret_cast<uint4*>(rank + i0);
#pragma unroll
    for (int q = 0; q < 4; ++q) d[q] = make_uint4(o[4 * q], o[4 * q + 1], o[4 * q + 2], o[4 * q + 3]);
  } else {
    for (int b = 0; b < 16 && i0 + b < n; ++b) rank[i0 + b] = o[b];
  }
}

// Build the grid index of m from the n points in `in` (device, x y z
// bits(id), any order, all ids distinct) with bounding box mn / mx: the cell
// table, the cell-sorted points, the coarse level and (speed only) the
// block rows; keep flags all set.  m's index arrays must be empty.
// block rows wanted: not disabled, positions fit 32 bits
static bool block_rows_wanted(const MapDev& m) {
  const char* nb9 = std::getenv("SLIO_NO_BLOCK_ROWS");
  return !(nb9 && nb9[0] && nb9[0] != '0') && m.n > 0 && 9 * m.n < (int64_t)0xFFFFFFF0ll;
}

// Block rows of m's current index (speed only: on any failure the map just
// goes without them).  The views are published after the stream has
// finished them, so a handle sharing the map sees either no block rows or
// complete ones.
int build_blk(MapDev& m, hipStream_t st, const char* who) {
  m.blk_deferred = false;
  const GridGeom g = m.g;
  const int64_t nseg = (int64_t)((g.dx + kBlkSeg - 1) / kBlkSeg) * g.dy * g.dz;
  size_t t3 = 0;
  hipError_t e;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, t3, (uint32_t*)nullptr, (uint32_t*)nullptr,
                                            (int)(m.ncells + 1), st)) ||
      (e = m.take(m.b_tmp[6], 4 * (m.ncells + 1))) || (e = m.take(m.b_tmp[7], t3)) ||
      (e = m.take(m.b_bstart, sizeof(uint32_t) * (m.ncells + 1)))) {
    (void)hipGetLastError();
    return SLIO_OK;
  }
  uint32_t* cnt = (uint32_t*)m.b_tmp[6].p;
  uint32_t* bstart = (uint32_t*)m.b_bstart.p;
  if ((e = m.take(m.b_tmp[5], 2 * nseg))) {
    (void)hipGetLastError();
    return SLIO_OK;
  }
  uint16_t* live = (uint16_t*)m.b_tmp[5].p;
  if ((e = hipMemsetAsync(cnt + m.ncells, 0, 4, st))) {
    set_error(std::string(who) + ": block rows: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  k_blk_live<<<grid_blocks(nseg), 256, 0, st>>>(m.start, g, nseg, live);
  k_blk_count<<<grid_blocks(m.ncells), 256, 0, st>>>(m.start, live, g, m.ncells, cnt);
  size_t tb = m.b_tmp[7].cap;
  if ((e = hipcub::DeviceScan::ExclusiveSum(m.b_tmp[7].p, tb, cnt, bstart, (int)(m.ncells + 1), st))) {
    set_error(std::string(who) + ": block-row scan: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  uint32_t total = 0;  // <= 9 n < 2^32 (block_rows_wanted): the scan cannot wrap
  if ((e = hipMemcpyAsync(&total, bstart + m.ncells, sizeof(uint32_t), hipMemcpyDeviceToHost, st)) ||
      (e = hipStreamSynchronize(st))) {
    set_error(std::string(who) + ": block-row total: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  if (m.take(m.b_blk, sizeof(float4) * std::max<uint32_t>(total, 1u))) {
    (void)hipGetLastError();
    return SLIO_OK;
  }
  k_blk_fill<<<grid_blocks(m.ncells), 256, 0, st>>>(m.pts, m.start, live, bstart, g, m.ncells,
                                                     (float4*)m.b_blk.p);
  if ((e = hipGetLastError()) || (e = hipStreamSynchronize(st))) {
    set_error(std::string(who) + ": block-row kernels: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  m.bstart = bstart;
  m.nblk = (int64_t)total;
  m.blk = (float4*)m.b_blk.p;
  return SLIO_OK;
}

// in_id_order: `in` is the map's previous cell-sorted points (survivors, in
// their stored order) followed by points with larger ids in id order -- then,
// when the grid comes out the same as before (or the map was empty), a STABLE
// sort by cell alone yields (cell, id) order, and the 32-bit cell key needs
// about half the radix passes of the 64-bit (cell, id) key.
int build_index(MapDev& m, const float4* in, int64_t n, const float mn[3], const float mx[3], hipStream_t st,
                const char* who, bool with_blk, bool in_id_order, bool had_points) {
  m.blk_deferred = false;
  const GridGeom g_old = m.g;
  GridGeom g;
  // cell edge: the caller's, or auto (cell0 == 0): 1.0 m -- the best edge for the
  // 10M-point, 0.5 m map (cell edge) -- unless that grid has more
  // than 2^27 cells, whose tables overflow the Infinity Cache and slow every
  // query's first loads: then 1.25 m (the 50M-point map's best)
  const bool auto_cell = !(m.cell0 > 0.0f);
  float hcell = auto_cell ? 1.0f : m.cell0;
  // kGridPad empty cells around the map's bounding box: scan points just
  // outside it (ground returns below a flat map's lowest point, range noise)
  // still get a query cell inside the grid, so they take the 3x3x3 fast path
  // A rebuild keeps the previous grid while the points still lie at least one
  // cell inside it (the grid need not be tight: every bound is conservative),
  // so the cell-only sort below applies; when they do not, the new grid gets
  // twice the padding, and a map growing slowly at an edge re-grids rarely.
  const int kGridPad = in_id_order ? 4 : 2;
  bool keep_grid = in_id_order && had_points;
  if (keep_grid) {
    const float o[3] = {g_old.ox, g_old.oy, g_old.oz};
    const int d[3] = {g_old.dx, g_old.dy, g_old.dz};
    for (int a = 0; a < 3; ++a)
      keep_grid = keep_grid && mn[a] >= o[a] + g_old.h && mx[a] <= o[a] + (float)(d[a] - 1) * g_old.h;
  }
  for (; !keep_grid;) {
    g.ox = mn[0] - kGridPad * hcell;
    g.oy = mn[1] - kGridPad * hcell;
    g.oz = mn[2] - kGridPad * hcell;
    g.h = hcell;
    g.inv_h = 1.0f / hcell;
    g.dx = cell_coord(mx[0], g.ox, g.inv_h) + 1 + kGridPad;
    g.dy = cell_coord(mx[1], g.oy, g.inv_h) + 1 + kGridPad;
    g.dz = cell_coord(mx[2], g.oz, g.inv_h) + 1 + kGridPad;
    const int64_t nc = (int64_t)g.dx * g.dy * g.dz;
    if (auto_cell && hcell == 1.0f && nc > ((int64_t)1 << 27)) {
      hcell = 1.25f;
      continue;
    }
    if (nc <= m.max_cells && nc < (int64_t)0xFFFFFFF0ll) break;
    hcell *= 1.25f;  // grow cells until the dense table fits the budget
  }
  if (keep_grid) g = g_old;
  // largest |coordinate| a cell face can have: |origin| + dims * h per axis
  // (kept grid: the same tol as before)
  const float mag = std::max(std::fabs(g.ox) + (float)g.dx * g.h,
                             std::max(std::fabs(g.oy) + (float)g.dy * g.h, std::fabs(g.oz) + (float)g.dz * g.h));
  g.tol = mag * 3.814697265625e-06f + 1.0e-5f;  // 2^-18 relative: >= 64 ulps
  const bool cell_only =
      in_id_order && (!had_points || (g.ox == g_old.ox && g.oy == g_old.oy && g.oz == g_old.oz &&
                                      g.h == g_old.h && g.dx == g_old.dx && g.dy == g_old.dy &&
                                      g.dz == g_old.dz));
  if (in_id_order && std::getenv("SLIO_DEBUG_REBUILD"))
    std::fprintf(stderr, "slio rebuild: n %lld cell_only %d grid %d %d %d (was %d %d %d) origin %.6g %.6g %.6g (was %.6g %.6g %.6g)\n",
                 (long long)n, (int)cell_only, g.dx, g.dy, g.dz, g_old.dx, g_old.dy, g_old.dz, g.ox, g.oy, g.oz,
                 g_old.ox, g_old.oy, g_old.oz);
  m.g = g;
  m.n = n;
  m.ncells = (int64_t)g.dx * g.dy * g.dz;
  // coarse level geometry (cells of edge 4h on the same origin)
  GridGeom cg = g;
  cg.h = 4.0f * g.h;
  cg.inv_h = 1.0f / cg.h;
  cg.dx = (g.dx + 3) / 4;
  cg.dy = (g.dy + 3) / 4;
  cg.dz = (g.dz + 3) / 4;
  m.cg = cg;
  m.nccells = (int64_t)cg.dx * cg.dy * cg.dz;

  auto fail = [&](const char* what, hipError_t e) {
    set_error(std::string(who) + ": " + what + ": " + hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? SLIO_ENOMEM : SLIO_EDEVICE;
  };
  hipError_t e;
  if ((e = m.take(m.b_start, sizeof(uint32_t) * (m.ncells + 1))) ||
      (e = m.take(m.b_clo, sizeof(float4) * m.nccells)) || (e = m.take(m.b_chi, sizeof(float4) * m.nccells)))
    return fail("hipMalloc", e);
  m.start = (uint32_t*)m.b_start.p;
  m.clo = (float4*)m.b_clo.p;
  m.chi = (float4*)m.b_chi.p;
  if (n == 0) {
    if ((e = hipMemsetAsync(m.start, 0, sizeof(uint32_t) * (m.ncells + 1), st)) ||
        (e = hipMemsetAsync(m.clo, 0, sizeof(float4) * m.nccells, st)) || (e = hipStreamSynchronize(st)))
      return fail("empty map", e);
    return SLIO_OK;
  }
  if ((e = m.take(m.b_pts, sizeof(float4) * n)) || (e = m.take(m.b_keep, n)))
    return fail("hipMalloc", e);
  m.pts = (float4*)m.b_pts.p;
  m.keep = (uint8_t*)m.b_keep.p;
  uint64_t *k0 = nullptr, *k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr, *cnt = nullptr, *c0 = nullptr, *c1 = nullptr;
  void* tmp = nullptr;
  int rc = SLIO_OK;
  const int64_t maxc = std::max(m.ncells, m.nccells) + 1;
  do {
    if ((e = m.take(m.b_tmp[0], 8 * n)) || (e = m.take(m.b_tmp[1], 8 * n)) || (e = m.take(m.b_tmp[2], 4 * n)) ||
        (e = m.take(m.b_tmp[3], 4 * n)) || (e = m.take(m.b_tmp[4], 4 * n)) || (e = m.take(m.b_tmp[5], 4 * n)) ||
        (e = m.take(m.b_tmp[6], 4 * maxc))) {
      rc = fail("hipMalloc", e);
      break;
    }
    k0 = (uint64_t*)m.b_tmp[0].p;
    k1 = (uint64_t*)m.b_tmp[1].p;
    v0 = (uint32_t*)m.b_tmp[2].p;
    v1 = (uint32_t*)m.b_tmp[3].p;
    c0 = (uint32_t*)m.b_tmp[4].p;
    c1 = (uint32_t*)m.b_tmp[5].p;
    cnt = (uint32_t*)m.b_tmp[6].p;
    int idbits = 1;
    while (idbits < 32 && ((int64_t)1 << idbits) <= (int64_t)m.next_id) ++idbits;
    int cbits = 1;
    while (cbits < 32 && ((int64_t)1 << cbits) < m.ncells) ++cbits;
    int ccbits = 1;
    while (ccbits < 32 && ((int64_t)1 << ccbits) < m.nccells) ++ccbits;
    size_t t1 = 0, t2 = 0, t3 = 0, t4 = 0, t5 = 0;
    if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, t1, k0, k1, v0, v1, (int)n, 0, idbits + cbits, st)) ||
        (e = hipcub::DeviceRadixSort::SortPairs(nullptr, t2, c0, c1, v0, v1, (int)n, 0, ccbits, st)) ||
        (e = hipcub::DeviceRadixSort::SortPairs(nullptr, t5, c0, c1, v0, v1, (int)n, 0, cbits, st)) ||
        (e = hipcub::DeviceScan::ExclusiveSum(nullptr, t3, cnt, m.start, (int)maxc, st))) {
      rc = fail("sort size", e);
      break;
    }
    t4 = std::max(std::max(std::max(t1, t2), t3), t5);
    if ((e = m.take(m.b_tmp[7], t4))) {
      rc = fail("hipMalloc tmp", e);
      break;
    }
    tmp = m.b_tmp[7].p;
    const int nb = grid_blocks(n);
    if (cell_only) {
      k_coarse_keys<<<nb, 256, 0, st>>>(in, n, g, c0, v0);  // fine cell keys (same formula)
      if ((e = hipcub::DeviceRadixSort::SortPairs(tmp, t4, c0, c1, v0, v1, (int)n, 0, cbits, st)) ||
          (e = hipMemsetAsync(cnt, 0, 4 * (m.ncells + 1), st))) {
        rc = fail("sort", e);
        break;
      }
      k_cell_hist_sorted<uint32_t><<<nb, 256, 0, st>>>(c1, n, 0, cnt);
    } else {
      k_cell_keys64<<<nb, 256, 0, st>>>(in, n, g, idbits, k0, v0);
      if ((e = hipcub::DeviceRadixSort::SortPairs(tmp, t4, k0, k1, v0, v1, (int)n, 0, idbits + cbits, st)) ||
          (e = hipMemsetAsync(cnt, 0, 4 * (m.ncells + 1), st))) {
        rc = fail("sort", e);
        break;
      }
      k_cell_hist_sorted<uint64_t><<<nb, 256, 0, st>>>(k1, n, idbits, cnt);
    }
    if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, t4, cnt, m.start, (int)(m.ncells + 1), st))) {
      rc = fail("scan", e);
      break;
    }
    k_gather4<<<nb, 256, 0, st>>>(in, v1, n, m.pts);
    k_fill_u8<<<nb, 256, 0, st>>>(m.keep, n, 1);
    // coarse level from the fine cell table (k_coarse_count / k_coarse_boxes:
    // no sort), tight boxes
    k_coarse_count<<<grid_blocks(m.nccells), 256, 0, st>>>(m.start, g, cg, m.nccells, cnt);
    k_coarse_boxes<<<grid_blocks(m.nccells), 256, 0, st>>>(m.pts, m.start, g, cg, cnt, m.nccells, m.clo,
                                                                   m.chi);
    m.del_loose = 0;
    if ((e = hipGetLastError()) || (e = hipStreamSynchronize(st))) {
      rc = fail("build kernels", e);
      break;
    }
    // block rows (speed only): now for an uploaded map; a map rebuilt by
    // the live-map maintenance gets them once it has stopped changing
    m.blk_deferred = block_rows_wanted(m);
    m.stable_passes = 0;
    if (with_blk && m.blk_deferred) rc = build_blk(m, st, who);
  } while (0);
#ifdef SLIO_BOUNDS_CHECK
  if (!rc) dbg_set_bounds(n, m.ncells);
#endif
  return rc;
}

// ---------------------------------------------------------------- map maintenance
// Device mirror of the map changes laserMapping makes every scan
// (map_incremental laserMapping.cpp:382-433, KD_TREE::Add_Points
// ikd_Tree.cpp:419-512, Delete_Point_Boxes ikd_Tree.cpp:559-579), with the
// set semantics the oracle (oracle/map_oracle.cpp) restates.

__device__ __forceinline__ float map_dist(float ax, float ay, float az, float bx, float by, float bz) {
  // calc_dist (ikd_Tree.cpp:1539-1544, common_lib.h:86-90)
  return (ax - bx) * (ax - bx) + (ay - by) * (ay - by) + (az - bz) * (az - bz);
}
__device__ __forceinline__ bool map_same(float ax, float ay, float az, float bx, float by, float bz) {
  // same_point (ikd_Tree.cpp:1533-1536), EPSS 1e-6
  return fabsf(ax - bx) < 1e-6 && fabsf(ay - by) < 1e-6 && fabsf(az - bz) < 1e-6;
}

// Delete_Point_Boxes: half-open boxes [min, max) (the Delete_by_range
// predicate); boxes in constant-size batches
struct Boxes8 {
  float b[8][6];
  int n;
};
__global__ void k_map_delete(const float4* __restrict__ pts, uint8_t* __restrict__ keep, int64_t n, Boxes8 bx,
                             unsigned long long* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool del = false;
  if (i < n && keep[i]) {
    const float4 p = pts[i];
    for (int k = 0; k < bx.n; ++k) {
      const float* b = bx.b[k];
      if (b[0] <= p.x && b[3] > p.x && b[1] <= p.y && b[4] > p.y && b[2] <= p.z && b[5] > p.z) del = true;
    }
    if (del) keep[i] = 0;
  }
  const unsigned long long m = __ballot(del);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
}

// downsample voxel key of a point: the three floor(p / ds) (ikd_Tree.cpp:430-441)
__device__ __forceinline__ uint64_t ds_key(int64_t kx, int64_t ky, int64_t kz) {
  return ((uint64_t)((kx + (1 << 20)) & 0x1FFFFF) << 42) | ((uint64_t)((ky + (1 << 20)) & 0x1FFFFF) << 21) |
         (uint64_t)((kz + (1 << 20)) & 0x1FFFFF);
}

// the call's voxel-key range per axis (atomic min / max of floor(p / ds),
// reduced per wavefront first)
__global__ void k_ds_range(const float4* __restrict__ in, int64_t n, float ds, int32_t* __restrict__ rg) {
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float4 p = in[i];
    const int32_t k[3] = {(int32_t)floorf(p.x / ds), (int32_t)floorf(p.y / ds), (int32_t)floorf(p.z / ds)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lo[a] = min(lo[a], k[a]);
      hi[a] = max(hi[a], k[a]);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int d = 32; d > 0; d >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], d, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], d, 64));
    }
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(&rg[a], lo[a]);
      atomicMax(&rg[3 + a], hi[a]);
    }
}
// keys packed relative to the call's range (groups by equality only)
struct DsPack {
  int32_t mx, my, mz;
  int sy, sz;  // shifts of the x and y fields
};
__global__ void k_ds_keys_packed(const float4* __restrict__ in, int64_t n, float ds, DsPack pk,
                                 uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  const uint64_t kx = (uint64_t)((int64_t)(int32_t)floorf(p.x / ds) - pk.mx);
  const uint64_t ky = (uint64_t)((int64_t)(int32_t)floorf(p.y / ds) - pk.my);
  const uint64_t kz = (uint64_t)((int64_t)(int32_t)floorf(p.z / ds) - pk.mz);
  keys[i] = (kx << pk.sy) | (ky << pk.sz) | kz;
  vals[i] = (uint32_t)i;
}

__global__ void k_ds_keys(const float4* __restrict__ in, int64_t n, float ds, uint64_t* __restrict__ keys,
                          uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float4 p = in[i];
  const int64_t kx = (int64_t)floorf(p.x / ds), ky = (int64_t)floorf(p.y / ds), kz = (int64_t)floorf(p.z / ds);
  keys[i] = ds_key(kx, ky, kz);
  vals[i] = (uint32_t)i;
}

// The downsample box of key (kx, ky, kz): [floor * ds, floor * ds + ds) per
// axis in float, as Add_Points forms it from a point of that key
// (ikd_Tree.cpp:430-441); Search_by_range's predicate is half-open
// (:1127-1128).  For a downsample size that is not a power of two,
// neighbouring float boxes can overlap by an ulp (or leave an ulp gap).
struct DsBox {
  float lo[3], hi[3];
};
__device__ __forceinline__ DsBox ds_box(int64_t kx, int64_t ky, int64_t kz, float ds) {
  DsBox b;
  const int64_t k[3] = {kx, ky, kz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    b.lo[a] = (float)k[a] * ds;
    b.hi[a] = b.lo[a] + ds;
  }
  return b;
}
__device__ __forceinline__ bool ds_inside(const DsBox& b, float x, float y, float z) {
  return b.lo[0] <= x && b.hi[0] > x && b.lo[1] <= y && b.hi[1] > y && b.lo[2] <= z && b.hi[2] > z;
}
__device__ __forceinline__ int64_t ds_find(const uint64_t* __restrict__ keys, int64_t n, uint64_t k) {
  int64_t a = 0, b = n;  // first index with keys[i] >= k
  while (a < b) {
    const int64_t m = (a + b) >> 1;
    if (keys[m] < k) a = m + 1; else b = m;
  }
  return (a < n && keys[a] == k) ? a : -1;
}
// p lies in the box of a key other than `own` that this call also holds a
// point of (the boxes of the 27 keys around p's own key)
__device__ __forceinline__ bool ds_shared(float x, float y, float z, uint64_t own, float ds,
                                          const uint64_t* __restrict__ keys, int64_t n) {
  const int64_t kx = (int64_t)floorf(x / ds), ky = (int64_t)floorf(y / ds), kz = (int64_t)floorf(z / ds);
  for (int dz = -1; dz <= 1; ++dz)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const uint64_t k = ds_key(kx + dx, ky + dy, kz + dz);
        if (k == own || !ds_inside(ds_box(kx + dx, ky + dy, kz + dz, ds), x, y, z)) continue;
        if (ds_find(keys, n, k) >= 0) return true;
      }
  return false;
}

// Groups are independent (k_ds_groups) unless some point -- stored and alive
// in a group's box, or one of the call's new points -- lies in the boxes of
// two keys of this call (float boxes overlapping by an ulp, or a new point
// past its own box's upper face inside the next box), or a new point lies
// outside its own box (an ulp gap): then the call's sequential order
// matters.  One thread per group; flag[0] = 1 on any.
__global__ void k_ds_conflicts(const float4* __restrict__ in, const uint64_t* __restrict__ keys,
                               const uint32_t* __restrict__ order, int64_t n, float ds, MapView map,
                               const uint8_t* __restrict__ keep, unsigned long long* __restrict__ flag) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 >= n || (i0 > 0 && keys[i0] == keys[i0 - 1])) return;
  const uint64_t own = keys[i0];
  bool hit = false;
  {
    const float4 q0 = in[order[i0]];
    const DsBox ob = ds_box((int64_t)floorf(q0.x / ds), (int64_t)floorf(q0.y / ds), (int64_t)floorf(q0.z / ds), ds);
    for (int64_t j = i0; j < n && keys[j] == own && !hit; ++j) {
      const float4 q = in[order[j]];
      // a new point outside its own box (an ulp gap past the upper face):
      // the group's later points do not see it (k_ds_groups assumes they do)
      hit = !ds_inside(ob, q.x, q.y, q.z) || ds_shared(q.x, q.y, q.z, own, ds, keys, n);
    }
  }
  if (!hit && map.n > 0) {
    const float4 q0 = in[order[i0]];
    const DsBox bx = ds_box((int64_t)floorf(q0.x / ds), (int64_t)floorf(q0.y / ds), (int64_t)floorf(q0.z / ds), ds);
    const GridGeom g = map.g;
    int ca[3], cb[3];
    const float og[3] = {g.ox, g.oy, g.oz};
    const int dg[3] = {g.dx, g.dy, g.dz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ca[a] = min(max(cell_coord(bx.lo[a], og[a], g.inv_h), 0), dg[a] - 1);
      cb[a] = min(max(cell_coord(bx.hi[a], og[a], g.inv_h), 0), dg[a] - 1);
    }
    for (int z = ca[2]; z <= cb[2] && !hit; ++z)
      for (int y = ca[1]; y <= cb[1] && !hit; ++y) {
        const uint32_t rb = ((uint32_t)z * (uint32_t)g.dy + (uint32_t)y) * (uint32_t)g.dx;
        for (uint32_t ps = map.start[rb + ca[0]]; ps < map.start[rb + cb[0] + 1] && !hit; ++ps) {
          if (!keep[ps]) continue;
          const float4 p = map.pts[ps];
          if (ds_inside(bx, p.x, p.y, p.z)) hit = ds_shared(p.x, p.y, p.z, own, ds, keys, n);
        }
      }
  }
  if (hit) atomicExch(flag, 1ull);
}

// The call's exact sequential Add_Points (ikd_Tree.cpp:428-512, the set
// restatement of oracle/map_oracle.cpp) by ONE thread, point by point in list
// order, for a call whose groups interact (k_ds_conflicts): stored points in
// storage order (ascending id), then this call's earlier survivors in list
// order; the new point wins ties, a stored one only when strictly nearer.
// Slow (one thread) and rare: only ulp-wide float overlaps of downsample
// boxes can interact, and only for a size that is not a power of two.
__global__ void k_ds_sequential(const float4* __restrict__ in, const uint64_t* __restrict__ keys,
                                const uint32_t* __restrict__ order, int64_t n, float ds, MapView map,
                                uint8_t* __restrict__ keep, uint32_t* __restrict__ surv,
                                unsigned long long* __restrict__ counter) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const GridGeom g = map.g;
  const float og[3] = {g.ox, g.oy, g.oz};
  const int dg[3] = {g.dx, g.dy, g.dz};
  unsigned long long ops = 0;
  for (int64_t li = 0; li < n; ++li) {
    const float4 q = in[li];
    const int64_t kx = (int64_t)floorf(q.x / ds), ky = (int64_t)floorf(q.y / ds), kz = (int64_t)floorf(q.z / ds);
    const DsBox bx = ds_box(kx, ky, kz, ds);
    const float mx = (float)((double)bx.lo[0] + (double)(bx.hi[0] - bx.lo[0]) / 2.0);
    const float my = (float)((double)bx.lo[1] + (double)(bx.hi[1] - bx.lo[1]) / 2.0);
    const float mz = (float)((double)bx.lo[2] + (double)(bx.hi[2] - bx.lo[2]) / 2.0);
    int ca[3], cb[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      ca[a] = min(max(cell_coord(bx.lo[a], og[a], g.inv_h), 0), dg[a] - 1);
      cb[a] = min(max(cell_coord(bx.hi[a], og[a], g.inv_h), 0), dg[a] - 1);
    }
    // winner: the new point unless a storage entry is strictly nearer; among
    // entries, the first minimum in storage order
    int64_t cnt = 0;
    float bd = map_dist(q.x, q.y, q.z, mx, my, mz);
    int wk = 0;  // 0: the new point, 1: stored (bpos), 2: this call's earlier survivor (blj)
    uint32_t bid = 0;
    int64_t bpos = -1, blj = -1;
    float4 bp = q;
    if (map.n > 0)
      for (int z = ca[2]; z <= cb[2]; ++z)
        for (int y = ca[1]; y <= cb[1]; ++y) {
          const uint32_t rb = ((uint32_t)z * (uint32_t)g.dy + (uint32_t)y) * (uint32_t)g.dx;
          for (uint32_t ps = map.start[rb + ca[0]]; ps < map.start[rb + cb[0] + 1]; ++ps) {
            if (!keep[ps]) continue;
            const float4 p = map.pts[ps];
            if (!ds_inside(bx, p.x, p.y, p.z)) continue;
            ++cnt;
            const float d = map_dist(p.x, p.y, p.z, mx, my, mz);
            const uint32_t id = __float_as_uint(p.w);
            if (d < bd || (wk == 1 && d == bd && id < bid)) {
              bd = d;
              bid = id;
              bpos = ps;
              bp = p;
              wk = 1;
            }
          }
        }
    // earlier survivors of this call inside the box: their keys are among
    // the 27 around q's key; storage order after every stored point, in list order
    for (int dz = -1; dz <= 1; ++dz)
      for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
          int64_t j = ds_find(keys, n, ds_key(kx + dx, ky + dy, kz + dz));
          if (j < 0) continue;
          const uint64_t k = keys[j];
          for (; j < n && keys[j] == k; ++j) {
            const uint32_t lj = order[j];
            if ((int64_t)lj >= li || !surv[lj]) continue;
            const float4 p = in[lj];
            if (!ds_inside(bx, p.x, p.y, p.z)) continue;
            ++cnt;
            const float d = map_dist(p.x, p.y, p.z, mx, my, mz);
            // strictly nearer than the best so far, or as near as the best
            // earlier survivor but earlier in list order (storage order)
            if (d < bd || (wk == 2 && d == bd && (int64_t)lj < blj)) {
              bd = d;
              blj = lj;
              bp = p;
              wk = 2;
            }
          }
        }
    if (cnt > 1 || map_same(q.x, q.y, q.z, bp.x, bp.y, bp.z)) {
      ++ops;
      // every storage entry but the winner goes
      if (map.n > 0)
        for (int z = ca[2]; z <= cb[2]; ++z)
          for (int y = ca[1]; y <= cb[1]; ++y) {
            const uint32_t rb = ((uint32_t)z * (uint32_t)g.dy + (uint32_t)y) * (uint32_t)g.dx;
            for (uint32_t ps = map.start[rb + ca[0]]; ps < map.start[rb + cb[0] + 1]; ++ps)
              if (keep[ps] && !(wk == 1 && (int64_t)ps == bpos) && ds_inside(bx, map.pts[ps].x, map.pts[ps].y,
                                                                                  map.pts[ps].z))
                keep[ps] = 0;
          }
      for (int dz = -1; dz <= 1; ++dz)
        for (int dy = -1; dy <= 1; ++dy)
          for (int dx = -1; dx <= 1; ++dx) {
            int64_t j = ds_find(keys, n, ds_key(kx + dx, ky + dy, kz + dz));
            if (j < 0) continue;
            const uint64_t k = keys[j];
            for (; j < n && keys[j] == k; ++j) {
              const uint32_t lj = order[j];
              if ((int64_t)lj >= li || !surv[lj] || (wk == 2 && (int64_t)lj == blj)) continue;
              if (ds_inside(bx, in[lj].x, in[lj].y, in[lj].z)) surv[lj] = 0;
            }
          }
      if (wk == 0) surv[li] = 1;
    }
  }
  counter[0] = ops;
}

// One thread per voxel group of the sorted list (the points of one
// Add_Points call that share a downsample box, in list order): the
// sequential rules of Add_Points on the box's stored points and the group's
// points.  Stored points in storage order = ascending id; a stored point
// wins only when strictly nearer the box centre (ties: the lower id).
// One downsample group (the points of one voxel key) against the stored
// map, in list order -- the sequential rules of Add_Points (ikd_Tree.cpp:
// 428-512) for a group no other group interacts with.  member(j) is the
// list index of the group's j-th point in list order, j < m.
template <typename Member>
__device__ __forceinline__ void ds_group(const float4* __restrict__ in, float ds, const MapView& map,
                                         uint8_t* __restrict__ keep, uint32_t* __restrict__ surv,
                                         unsigned long long* __restrict__ counter, int64_t m, Member member) {
  const uint32_t li0 = member(0);
  const float4 q0 = in[li0];
  float lo[3], hi[3];
  const float c0[3] = {q0.x, q0.y, q0.z};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    lo[a] = floorf(c0[a] / ds) * ds;
    hi[a] = lo[a] + ds;
  }
  const float mx = (float)((double)lo[0] + (double)(hi[0] - lo[0]) / 2.0);
  const float my = (float)((double)lo[1] + (double)(hi[1] - lo[1]) / 2.0);
  const float mz = (float)((double)lo[2] + (double)(hi[2] - lo[2]) / 2.0);
  const GridGeom g = map.g;
  int ca[3], cb[3];
  const float og[3] = {g.ox, g.oy, g.oz};
  const int dg[3] = {g.dx, g.dy, g.dz};
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    ca[a] = min(max(cell_coord(lo[a], og[a], g.inv_h), 0), dg[a] - 1);
    cb[a] = min(max(cell_coord(hi[a], og[a], g.inv_h), 0), dg[a] - 1);
  }
  auto inside = [&](const float4& p) {
    return lo[0] <= p.x && hi[0] > p.x && lo[1] <= p.y && hi[1] > p.y && lo[2] <= p.z && hi[2] > p.z;
  };
  // stored points in the box: count and the one nearest the centre
  int64_t cnt = 0;
  float bd = 0.0f;
  uint32_t bid = 0xFFFFFFFFu;
  int64_t bpos = -1;
  float4 bp = make_float4(0, 0, 0, 0);
  if (map.n > 0)
    for (int z = ca[2]; z <= cb[2]; ++z)
      for (int y = ca[1]; y <= cb[1]; ++y) {
        const uint32_t rb = ((uint32_t)z * (uint32_t)g.dy + (uint32_t)y) * (uint32_t)g.dx;
        for (uint32_t ps = map.start[rb + ca[0]]; ps < map.start[rb + cb[0] + 1]; ++ps) {
          if (!keep[ps]) continue;
          const float4 p = map.pts[ps];
          if (!inside(p)) continue;
          ++cnt;
          const float d = map_dist(p.x, p.y, p.z, mx, my, mz);
          const uint32_t id = __float_as_uint(p.w);
          if (bpos < 0 || d < bd || (d == bd && id < bid)) {
            bd = d;
            bid = id;
            bpos = ps;
            bp = p;
          }
        }
      }
  // the group's points, in list order
  bool orig_all = true;       // every stored point still alive
  int64_t orig_keep = -1;     // else: the one stored point kept (or none)
  int64_t cur_new = -1;       // list index of this call's surviving new point
  bool best_new = false;
  unsigned long long ops = 0;
  for (int64_t j = 0; j < m; ++j) {
    const uint32_t li = j == 0 ? li0 : member(j);  // member() is called once per j, in order
    const float4 q = in[li];
    const float dq = map_dist(q.x, q.y, q.z, mx, my, mz);
    const bool stored_wins = cnt > 0 && bd < dq;
    const float4 w = stored_wins ? bp : q;
    if (cnt > 1 || map_same(q.x, q.y, q.z, w.x, w.y, w.z)) {
      ++ops;
      if (!stored_wins) {
        orig_all = false;
        orig_keep = -1;
        cur_new = li;
        best_new = true;
        bd = dq;
        bp = q;
      } else if (!best_new && orig_all) {
        orig_all = false;
        orig_keep = bpos;
      }
      cnt = 1;
    }
  }
  if (!orig_all && map.n > 0)
    for (int z = ca[2]; z <= cb[2]; ++z)
      for (int y = ca[1]; y <= cb[1]; ++y) {
        const uint32_t rb = ((uint32_t)z * (uint32_t)g.dy + (uint32_t)y) * (uint32_t)g.dx;
        for (uint32_t ps = map.start[rb + ca[0]]; ps < map.start[rb + cb[0] + 1]; ++ps)
          if (keep[ps] && (int64_t)ps != orig_keep && inside(map.pts[ps])) keep[ps] = 0;
      }
  if (cur_new >= 0) surv[cur_new] = 1;
  if (ops) atomicAdd(counter, ops);
}

// groups from the keys sorted stably (keys, order = list indices): one
// thread per group head
__global__ void k_ds_groups(const float4* __restrict__ in, const uint64_t* __restrict__ keys,
                            const uint32_t* __restrict__ order, int64_t n, float ds, MapView map,
                            uint8_t* __restrict__ keep, uint32_t* __restrict__ surv,
                            unsigned long long* __restrict__ counter) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 >= n || (i0 > 0 && keys[i0] == keys[i0 - 1])) return;
  if (counter[1]) return;  // interacting groups: k_ds_sequential instead
  int64_t m = 1;
  while (i0 + m < n && keys[i0 + m] == keys[i0]) ++m;
  ds_group(in, ds, map, keep, surv, counter, m, [&](int64_t j) { return order[i0 + j]; });
}

// Grouping without a sort (exact boxes: groups are independent and need no
// global order, only their own points in list order).  Open-addressing hash
// of the voxel key (ds_key) into H = 2^hb slots: each point claims or finds
// its key's slot (atomicCAS), takes a member position (atomicAdd) and stores
// its list index there (up to kDsInline per slot); a slot with more members
// rescans the list for its key (rare: a 0.5 m voxel of a downsampled scan).
// A key outside ds_key's 21-bit range sets *flag (counter[2] of the groups
// kernel): the caller then takes the sorting path.
constexpr int kDsInline = 16;
constexpr uint64_t kDsEmpty = ~0ull;
// (nl: when set, the list holds nl[0] + nl[1] points -- an exclusive scan's
// last rank and flag -- of the n it has room for)
__global__ void k_ds_hash(const float4* __restrict__ in, int64_t n, float ds, int hb, uint64_t* __restrict__ hkey,
                          uint32_t* __restrict__ hcnt, uint32_t* __restrict__ hmem,
                          unsigned long long* __restrict__ flag, const uint32_t* __restrict__ nl_rank = nullptr,
                          const uint32_t* __restrict__ nl_flag = nullptr) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (nl_rank ? (int64_t)(*nl_rank + *nl_flag) : n)) return;
  const float4 p = in[i];
  const int64_t kx = (int64_t)floorf(p.x / ds), ky = (int64_t)floorf(p.y / ds), kz = (int64_t)floorf(p.z / ds);
  constexpr int64_t kLim = (1 << 20) - 1;
  if (kx < -kLim || kx > kLim || ky < -kLim || ky > kLim || kz < -kLim || kz > kLim) {
    atomicExch(flag, 1ull);
    return;
  }
  const uint64_t key = ds_key(kx, ky, kz);
  const uint64_t mask = ((uint64_t)1 << hb) - 1;
  uint64_t h = (key * 0x9E3779B97F4A7C15ull) >> (64 - hb);
  for (;;) {
    const unsigned long long prev = atomicCAS((unsigned long long*)&hkey[h], kDsEmpty, key);
    if (prev == kDsEmpty || prev == key) break;
    h = (h + 1) & mask;
  }
  const uint32_t pos = atomicAdd(&hcnt[h], 1u);
  if (pos < (uint32_t)kDsInline) hmem[h * kDsInline + pos] = (uint32_t)i;
}

// the hash table emptied, survivor flags and counters zeroed: one launch
// (four fills were four launches in a row)
__global__ void k_ds_init(uint64_t* __restrict__ hkey, uint32_t* __restrict__ hcnt, int64_t H,
                          uint32_t* __restrict__ surv, int64_t n, unsigned long long* __restrict__ dcount) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, st = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = i0; i < H; i += st) {
    hkey[i] = kDsEmpty;
    hcnt[i] = 0;
  }
  for (int64_t i = i0; i < n; i += st) surv[i] = 0;
  if (i0 < 3) dcount[i0] = 0;
}

// one thread per occupied slot: its members sorted into list order, then
// ds_group
__global__ void k_ds_groups_hash(const float4* __restrict__ in, int64_t n, float ds, int hb,
                                 const uint64_t* __restrict__ hkey, const uint32_t* __restrict__ hcnt,
                                 const uint32_t* __restrict__ hmem, MapView map, uint8_t* __restrict__ keep,
                                 uint32_t* __restrict__ surv, unsigned long long* __restrict__ counter) {
  const int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (h >= ((int64_t)1 << hb) || counter[2]) return;  // counter[2]: a key out of range
  const uint64_t key = hkey[h];
  if (key == kDsEmpty) return;
  const int64_t m = hcnt[h];
  if (m <= kDsInline) {
    uint32_t mem[kDsInline];
#pragma unroll
    for (int j = 0; j < kDsInline; ++j) mem[j] = j < m ? hmem[h * kDsInline + j] : 0xFFFFFFFFu;
    // insertion sort into list order (m is small)
    for (int j = 1; j < m; ++j) {
      const uint32_t v = mem[j];
      int k = j - 1;
      for (; k >= 0 && mem[k] > v; --k) mem[k + 1] = mem[k];
      mem[k + 1] = v;
    }
    ds_group(in, ds, map, keep, surv, counter, m, [&](int64_t j) { return mem[j]; });
  } else {
    // more members than the slot holds: the list in order, filtered by key
    int64_t next = 0;
    auto member = [&](int64_t j) {
      (void)j;  // called with j = 0, 1, ... in order
      for (;; ++next) {
        const float4 p = in[next];
        const uint64_t k = ds_key((int64_t)floorf(p.x / ds), (int64_t)floorf(p.y / ds), (int64_t)floorf(p.z / ds));
        if (k == key) return (uint32_t)next++;
      }
    };
    ds_group(in, ds, map, keep, surv, counter, m, member);
  }
}

// surviving points -> add4[base + rank] with id next_id + rank
__global__ void k_append(const float4* __restrict__ in, const uint32_t* __restrict__ surv,
                         const uint32_t* __restrict__ rank, int64_t n, float4* __restrict__ add4,
                         uint8_t* __restrict__ akeep, int64_t base, uint32_t next_id) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || (surv && !surv[i])) return;
  const uint32_t r = rank ? rank[i] : (uint32_t)i;
  const float4 p = in[i];
  add4[base + r] = make_float4(p.x, p.y, p.z, __uint_as_float(next_id + r));
  akeep[base + r] = 1;
}

// map_incremental's PointNoNeedDownsample after its PointToAdd survivors,
// both counts on the device: cnt = *cr + *cf points of `in`, placed after
// the *sr + *sf survivors at add4[base ...] with ids continuing next_id
__global__ void k_append_after(const float4* __restrict__ in, int64_t n, const uint32_t* __restrict__ cr,
                               const uint32_t* __restrict__ cf, const uint32_t* __restrict__ sr,
                               const uint32_t* __restrict__ sf, float4* __restrict__ add4,
                               uint8_t* __restrict__ akeep, int64_t base, uint32_t next_id) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || i >= (int64_t)(*cr + *cf)) return;
  const uint32_t r = *sr + *sf + (uint32_t)i;
  const float4 p = in[i];
  add4[base + r] = make_float4(p.x, p.y, p.z, __uint_as_float(next_id + r));
  akeep[base + r] = 1;
}
// the six scan totals (rank + flag of the last entry) map_incremental reads back
__global__ void k_inc_counts(const uint32_t* __restrict__ a0, const uint32_t* __restrict__ a1,
                             const uint32_t* __restrict__ b0, const uint32_t* __restrict__ b1,
                             const uint32_t* __restrict__ c0, const uint32_t* __restrict__ c1,
                             uint32_t* __restrict__ out) {
  if (threadIdx.x == 0) {
    out[0] = *a0 + *a1;
    out[1] = *b0 + *b1;
    out[2] = *c0 + *c1;
  }
}

// pointBodyToWorld (laserMapping.cpp:276-287) with the rotation matrices
// (Sophus SO3::matrix = Eigen toRotationMatrix) and map_incremental's
// classification (laserMapping.cpp:388-423): flag 1 = PointToAdd,
// 2 = PointNoNeedDownsample, 0 = not added.
struct WorldMat {
  double R[9], RL[9], pos[3], tli[3];
};
__global__ void k_map_classify(const float* __restrict__ bx, const float* __restrict__ by,
                               const float* __restrict__ bz, int64_t n, WorldMat W,
                               const uint32_t* __restrict__ nbr_pos, const float4* __restrict__ pts, double fs,
                               int ekf_inited, float4* __restrict__ wpts, uint32_t* __restrict__ f_add,
                               uint32_t* __restrict__ f_no) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double pb[3] = {(double)bx[i], (double)by[i], (double)bz[i]};
  double a[3], w[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) a[r] = ((W.RL[3 * r] * pb[0] + W.RL[3 * r + 1] * pb[1]) + W.RL[3 * r + 2] * pb[2]) + W.tli[r];
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = ((W.R[3 * r] * a[0] + W.R[3 * r + 1] * a[1]) + W.R[3 * r + 2] * a[2]) + W.pos[r];
  const float px = (float)w[0], py = (float)w[1], pz = (float)w[2];
  wpts[i] = make_float4(px, py, pz, 0.0f);
  int nn = 0;
  float4 nb[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) {
    const uint32_t ps = nbr_pos[i * 5 + j];
    nb[j] = make_float4(0, 0, 0, 0);
    if (ps != 0xFFFFFFFFu && nn == j) {
      nb[j] = pts[ps];
      ++nn;
    }
  }
  uint32_t fa = 0, fn = 0;
  if (nn > 0 && ekf_inited) {
    const float mx = (float)(floor((double)px / fs) * fs + 0.5 * fs);
    const float my = (float)(floor((double)py / fs) * fs + 0.5 * fs);
    const float mz = (float)(floor((double)pz / fs) * fs + 0.5 * fs);
    const float dist = map_dist(px, py, pz, mx, my, mz);
    if ((double)fabsf(nb[0].x - mx) > 0.5 * fs && (double)fabsf(nb[0].y - my) > 0.5 * fs &&
        (double)fabsf(nb[0].z - mz) > 0.5 * fs) {
      fn = 1;
    } else {
      bool need_add = true;
      if (nn >= 5) {
#pragma unroll
        for (int j = 0; j < 5; ++j)
          if (need_add && map_dist(nb[j].x, nb[j].y, nb[j].z, mx, my, mz) < dist) need_add = false;
      }
      fa = need_add ? 1 : 0;
    }
  } else {
    fa = 1;
  }
  f_add[i] = fa;
  f_no[i] = fn;
}

__global__ void k_compact4(const float4* __restrict__ in, const uint32_t* __restrict__ flag,
                           const uint32_t* __restrict__ rank, int64_t n, float4* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) out[rank[i]] = in[i];
}

// stable radix sort of n (key, value) pairs of 32-bit words by the whole key,
// enqueued on st; tmp (kept by the caller) grows to what the sort needs
hipError_t sort_pairs32(MapDev::Buf& tmp, const uint32_t* k0, uint32_t* k1, const uint32_t* v0, uint32_t* v1,
                        int64_t n, hipStream_t st) {
  size_t tb = 0;
  hipError_t e;
  if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k0, k1, v0, v1, (int)n, 0, 32, st)) ||
      (e = MapDev::take(tmp, tb)))
    return e;
  return hipcub::DeviceRadixSort::SortPairs(tmp.p, tb, k0, k1, v0, v1, (int)n, 0, 32, st);
}

// exclusive scan of n flags into rank, enqueued on st (no readback)
int scan_launch(const uint32_t* flag, uint32_t* rank, int64_t n, hipStream_t st) {
  size_t tb = 0;
  // scan temporaries cached per host thread AND device (no hipMalloc /
  // hipFree per call; one thread may drive handles on several GPUs, and a
  // device must never be handed another device's buffer).  Scans reusing
  // the buffer are ordered on one stream, and a buffer is replaced only
  // after the device is idle (hipFree synchronises).
  constexpr int kMaxDev = 64;
  static thread_local void* tmps[kMaxDev] = {};
  static thread_local size_t tcaps[kMaxDev] = {};
  int dev = 0;
  hipError_t e;
  if ((e = hipGetDevice(&dev)) || dev < 0 || dev >= kMaxDev) {
    set_error("slio map: scan: no current device");
    return SLIO_EDEVICE;
  }
  void*& tmp = tmps[dev];
  size_t& tcap = tcaps[dev];
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, flag, rank, (int)n, st))) {
    set_error(std::string("slio map: scan: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  if (tb > tcap) {
    (void)hipFree(tmp);
    tmp = nullptr;
    tcap = 0;
    if ((e = hipMalloc(&tmp, tb + tb / 2))) {
      set_error(std::string("slio map: scan: ") + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
    tcap = tb + tb / 2;
  }
  if ((e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, flag, rank, (int)n, st))) {
    set_error(std::string("slio map: scan: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  return SLIO_OK;
}

// exclusive scans of k flag arrays (n each) into ranks; totals read back
// with one synchronisation
static int scan_flags_k(int k, const uint32_t* const* flag, uint32_t* const* rank, int64_t n, hipStream_t st,
                        uint32_t* total) {
  for (int j = 0; j < k; ++j) total[j] = 0;
  if (n == 0) return SLIO_OK;
  uint32_t last[4] = {0, 0, 0, 0};
  Rb rb[4];
  for (int j = 0; j < k; ++j) {
    if (int rc = scan_launch(flag[j], rank[j], n, st)) return rc;
    rb[2 * j] = Rb{&last[2 * j], rank[j] + n - 1, 4};
    rb[2 * j + 1] = Rb{&last[2 * j + 1], flag[j] + n - 1, 4};
  }
  const hipError_t e = readback(st, rb, 2 * k);
  if (e) {
    set_error(std::string("slio map: scan total: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  for (int j = 0; j < k; ++j) total[j] = last[2 * j] + last[2 * j + 1];
  return SLIO_OK;
}

// exclusive scan of n flags into rank; returns the total
static int scan_flags(const uint32_t* flag, uint32_t* rank, int64_t n, hipStream_t st, uint32_t* total) {
  return scan_flags_k(1, &flag, &rank, n, st, total);
}

// two exclusive flag scans on one stream, one readback of both totals
static int scan_flags2(const uint32_t* f1, uint32_t* r1, const uint32_t* f2, uint32_t* r2, int64_t n,
                       hipStream_t st, uint32_t* t1, uint32_t* t2) {
  const uint32_t* f[2] = {f1, f2};
  uint32_t* r[2] = {r1, r2};
  uint32_t t[2];
  const int rc = scan_flags_k(2, f, r, n, st, t);
  *t1 = t[0];
  *t2 = t[1];
  return rc;
}

static int add_reserve(MapDev& m, int64_t more, hipStream_t st) {
  if (m.nadd + more <= m.add_cap) return SLIO_OK;
  const int64_t cap = std::max<int64_t>(2 * m.add_cap, m.nadd + more + 4096);
  float4* a = nullptr;
  uint8_t* k = nullptr;
  hipError_t e;
  if ((e = hipMalloc(&a, 16 * cap)) || (e = hipMalloc(&k, cap))) {
    (void)hipFree(a);
    set_error(std::string("slio map: hipMalloc adds: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  if (m.nadd > 0 && ((e = hipMemcpyAsync(a, m.add4, 16 * m.nadd, hipMemcpyDeviceToDevice, st)) ||
                     (e = hipMemcpyAsync(k, m.akeep, m.nadd, hipMemcpyDeviceToDevice, st)) ||
                     (e = spin_sync(st)))) {
    (void)hipFree(a);
    (void)hipFree(k);
    set_error(std::string("slio map: grow adds: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  (void)hipFree(m.add4);
  (void)hipFree(m.akeep);
  m.add4 = a;
  m.akeep = k;
  m.add_cap = cap;
  return SLIO_OK;
}

static int map_refresh_locked(Ctx& c, bool adds_only);

static MapView map_view(const MapDev& m) {
  const CoarseView cv{m.cg, m.clo, m.chi};
  return MapView{m.g, m.n, m.pts, m.start, m.blk, m.bstart, m.nblk, m.ncells, cv};
}

// KD_TREE::Add_Points on the device map: n points at `in` (device float4,
// .w ignored); returns the downsample counter (tmp_counter).
// Add_Points(downsample) for exact boxes by hash grouping (k_ds_hash,
// k_ds_groups_hash); *fallback = a voxel key outside ds_key's range was seen
// and nothing was changed (the caller then sorts).
static int map_add_hashed(Ctx& c, const float4* in, int64_t n, float ds, int64_t* counter, bool* fallback) {
  MapDev& m = *c.map;
  hipStream_t st = c.stream;
  *fallback = false;
  int hb = 10;
  while (((int64_t)1 << hb) < 2 * n) ++hb;
  const int64_t H = (int64_t)1 << hb;
  auto& B = m.b_add;
  hipError_t e;
  // B[0]: hash keys, B[1]: member counts, B[2]: members, B[4]: survivor flags,
  // B[5]: their ranks, B[6]: counters (ops, -, out-of-range)
  if ((e = m.take(B[0], 8 * H)) || (e = m.take(B[1], 4 * H)) || (e = m.take(B[2], 4 * kDsInline * H)) ||
      (e = m.take(B[4], 4 * n)) || (e = m.take(B[5], 4 * n)) || (e = m.take(B[6], 64))) {
    set_error(std::string("slio map: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  uint64_t* hkey = (uint64_t*)B[0].p;
  uint32_t* hcnt = (uint32_t*)B[1].p;
  uint32_t* hmem = (uint32_t*)B[2].p;
  uint32_t* surv = (uint32_t*)B[4].p;
  uint32_t* rank = (uint32_t*)B[5].p;
  unsigned long long* dcount = (unsigned long long*)B[6].p;
  // room for every point up front: the survivors are appended (past m.nadd)
  // before the readback that counts them
  if (int rc = add_reserve(m, n, st)) return rc;
  k_ds_init<<<grid_blocks(std::max<int64_t>(H, n)), 256, 0, st>>>(hkey, hcnt, H, surv, n, dcount);
  k_ds_hash<<<grid_blocks(n), 256, 0, st>>>(in, n, ds, hb, hkey, hcnt, hmem, dcount + 2);
  k_ds_groups_hash<<<grid_blocks(H), 256, 0, st>>>(in, n, ds, hb, hkey, hcnt, hmem, map_view(m), m.keep, surv,
                                                   dcount);
  // the survivors' ranks and their append, then their total and the
  // counters in one readback (a key out of range: nothing was appended past
  // m.nadd that counts, and no flag changed)
  if (int rc = scan_launch(surv, rank, n, st)) return rc;
  k_append<<<grid_blocks(n), 256, 0, st>>>(in, surv, rank, n, m.add4, m.akeep, m.nadd, m.next_id);
  uint32_t last[2] = {0, 0};
  unsigned long long ops[3] = {0, 0, 0};
  const Rb rb[3] = {{&last[0], rank + n - 1, 4}, {&last[1], surv + n - 1, 4}, {ops, dcount, 24}};
  if ((e = readback(st, rb, 3))) {
    set_error(std::string("slio map: groups: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  const uint32_t total = last[0] + last[1];
  if (ops[2]) {
    *fallback = true;
    return SLIO_OK;
  }
  *counter = (int64_t)ops[0];
  if ((e = hipGetLastError())) {
    set_error(std::string("slio map: append: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  m.nadd += total;
  m.next_id += total;
  m.dirty = true;  // deletions (keep flags) and / or additions
  return SLIO_OK;
}

static int map_add(Ctx& c, const float4* in, int64_t n, bool downsample, float ds, int64_t* counter) {
  MapDev& m = *c.map;
  hipStream_t st = c.stream;
  *counter = 0;
  if (n == 0) return SLIO_OK;
  if ((int64_t)m.next_id + n >= (int64_t)0x7FFFFFFF) {
    set_error("slio map: point ids exhausted (2^31)");
    return SLIO_ECAPACITY;
  }
  if (!downsample) {
    if (int rc = add_reserve(m, n, st)) return rc;
    k_append<<<grid_blocks(n), 256, 0, st>>>(in, nullptr, nullptr, n, m.add4, m.akeep, m.nadd, m.next_id);
    SLIO_HIP(hipGetLastError());
    m.nadd += n;
    m.next_id += (uint32_t)n;
    m.dirty = true;
    return SLIO_OK;
  }
  // the box searches need every stored point in the index
  if (int rc = map_refresh_locked(c, true)) return rc;
  {
    // exact boxes (a power-of-two size <= 1, see below): groups by hashing
    // the voxel keys -- no key-range readback, no sort (SLIO_NO_DS_HASH=1:
    // the sorting path)
    int ds_exp0 = 0;
    const char* nh = std::getenv("SLIO_NO_DS_HASH");
    const bool no_hash = nh && nh[0] && nh[0] != '0';
    if (!no_hash && std::frexp(ds, &ds_exp0) == 0.5f && ds <= 1.0f) {
      bool fallback = false;
      if (int rc = map_add_hashed(c, in, n, ds, counter, &fallback)) return rc;
      if (!fallback) return SLIO_OK;
    }
  }
  uint64_t *k0 = nullptr, *k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr, *surv = nullptr, *rank = nullptr;
  unsigned long long* dcount = nullptr;
  void* tmp = nullptr;
  int rc = SLIO_OK;
  do {
    // temporaries kept on the map across calls (a live map adds every scan;
    // hipFree would also synchronise the device)
    hipError_t e;
    auto& B = m.b_add;
    if ((e = m.take(B[0], 8 * n)) || (e = m.take(B[1], 8 * n)) || (e = m.take(B[2], 4 * n)) ||
        (e = m.take(B[3], 4 * n)) || (e = m.take(B[4], 4 * n)) || (e = m.take(B[5], 4 * n)) ||
        (e = m.take(B[6], 64))) {
      set_error(std::string("slio map: hipMalloc: ") + hipGetErrorString(e));
      rc = SLIO_ENOMEM;
      break;
    }
    k0 = (uint64_t*)B[0].p;
    k1 = (uint64_t*)B[1].p;
    v0 = (uint32_t*)B[2].p;
    v1 = (uint32_t*)B[3].p;
    surv = (uint32_t*)B[4].p;
    rank = (uint32_t*)B[5].p;
    dcount = (unsigned long long*)B[6].p;
    size_t tb = 0;
    if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, k0, k1, v0, v1, (int)n, 0, 63, st)) ||
        (e = m.take(B[7], tb))) {
      set_error(std::string("slio map: sort: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
    tmp = B[7].p;
    tb = B[7].cap;
    const int nb = grid_blocks(n);
    // Boxes interact only through float rounding: for a power-of-two size
    // <= 1 (0.5, the reference default) p / ds, floor * ds and + ds are all
    // exact while |key| + 1 < 2^24 (checked below on the call's key range),
    // every box is exactly [k ds, (k + 1) ds), and no point can lie outside
    // its own box or in two -- nothing to detect
    int ds_exp = 0;
    bool exact_boxes = std::frexp(ds, &ds_exp) == 0.5f && ds <= 1.0f;
    // Then only key equality matters (k_ds_groups; k_ds_conflicts and
    // k_ds_sequential, which look keys up by value, do not run): the keys are
    // packed relative to the call's voxel range, so the radix sort covers a
    // few dozen bits instead of 63 (8 onesweep passes: ~100 us for ~20k keys)
    int sort_bits = 63;
    if (exact_boxes) {
      int32_t* rg = (int32_t*)((char*)B[6].p + 16);  // after dcount (B[6]: 64 bytes)
      const int32_t init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
      int32_t got[6];
      if ((e = hipMemcpyAsync(rg, init, 24, hipMemcpyHostToDevice, st))) {
        set_error(std::string("slio map: range: ") + hipGetErrorString(e));
        rc = SLIO_EDEVICE;
        break;
      }
      k_ds_range<<<std::min(nb, 256), 256, 0, st>>>(in, n, ds, rg);
      const Rb rb{got, rg, 24};
      if ((e = readback(st, &rb, 1))) {
        set_error(std::string("slio map: range: ") + hipGetErrorString(e));
        rc = SLIO_EDEVICE;
        break;
      }
      for (int a = 0; a < 6; ++a)
        if (std::llabs((long long)got[a]) >= (1ll << 24) - 1) exact_boxes = false;  // (k + 1) ds inexact
      int bits[3];
      for (int a = 0; a < 3; ++a) {
        const int64_t span = (int64_t)got[3 + a] - (int64_t)got[a] + 1;
        bits[a] = 0;
        while (bits[a] < 40 && ((int64_t)1 << bits[a]) < span) ++bits[a];
      }
      if (exact_boxes && bits[0] + bits[1] + bits[2] <= 48) {
        sort_bits = std::max(1, bits[0] + bits[1] + bits[2]);
        const DsPack pk{got[0], got[1], got[2], bits[1] + bits[2], bits[2]};
        k_ds_keys_packed<<<nb, 256, 0, st>>>(in, n, ds, pk, k0, v0);
      }
    }
    if (sort_bits == 63) k_ds_keys<<<nb, 256, 0, st>>>(in, n, ds, k0, v0);
    if ((e = hipcub::DeviceRadixSort::SortPairs(tmp, tb, k0, k1, v0, v1, (int)n, 0, sort_bits, st)) ||
        (e = hipMemsetAsync(surv, 0, 4 * n, st)) || (e = hipMemsetAsync(dcount, 0, 16, st))) {
      set_error(std::string("slio map: sort: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
    if (!exact_boxes)
      k_ds_conflicts<<<nb, 256, 0, st>>>(in, k1, v1, n, ds, map_view(m), m.keep, dcount + 1);
    k_ds_groups<<<nb, 256, 0, st>>>(in, k1, v1, n, ds, map_view(m), m.keep, surv, dcount);
    uint32_t total = 0;
    if ((rc = scan_flags(surv, rank, n, st, &total))) break;
    unsigned long long ops[2] = {0, 0};
    const Rb rbo{ops, dcount, 16};
    if ((e = readback(st, &rbo, 1))) {
      set_error(std::string("slio map: groups: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
    if (ops[1]) {
      // interacting groups (k_ds_conflicts): the exact sequential order
      k_ds_sequential<<<1, 1, 0, st>>>(in, k1, v1, n, ds, map_view(m), m.keep, surv, dcount);
      if ((rc = scan_flags(surv, rank, n, st, &total))) break;
      const Rb rbs{ops, dcount, 8};
      if ((e = readback(st, &rbs, 1))) {
        set_error(std::string("slio map: sequential Add_Points: ") + hipGetErrorString(e));
        rc = SLIO_EDEVICE;
        break;
      }
      ++m.sequential_calls;
    }
    *counter = (int64_t)ops[0];
    if ((rc = add_reserve(m, total, st))) break;
    k_append<<<nb, 256, 0, st>>>(in, surv, rank, n, m.add4, m.akeep, m.nadd, m.next_id);
    if ((e = hipGetLastError())) {
      set_error(std::string("slio map: append: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
    m.nadd += total;
    m.next_id += total;
    m.dirty = true;  // deletions (keep flags) and / or additions
  } while (0);
  return rc;
}

// ---------------------------------------------------------------- merge rebuild
// A rebuild that keeps the grid does not sort the map again: the survivors
// are already in (cell, id) order and every addition has a larger id than
// every stored point, so the new order is, cell by cell, the cell's survivors
// (old order) followed by its additions (id order).  With rank = the
// survivors' exclusive prefix count and lb(c) = the number of (live, sorted)
// additions in cells < c:
//   new_start[c]       = rank(old_start[c]) + lb(c)
//   survivor p, cell c -> new_start[c] + rank[p] - rank(old_start[c])
//   addition j, cell c -> new_start[c + 1] - (lb(c + 1) - j)
// (rank(n0) = the survivor count).  Bit-identical to the sort: same points,
// same order, same cell table.
constexpr int kMergeTile = 4096;
constexpr int64_t kCoarseRetighten = 16;  // cells per workgroup of k_merge_start (256 threads x 16)
__device__ __forceinline__ uint32_t lower_bound_u32(const uint32_t* __restrict__ a, uint32_t lo, uint32_t hi,
                                                    uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(256) void k_merge_start(const uint32_t* __restrict__ old_start,
                                                     const uint32_t* __restrict__ rank, int64_t n0,
                                                     const uint32_t* __restrict__ n0p_p,
                                                     const uint32_t* __restrict__ sk, const uint32_t* __restrict__ jt,
                                                     int64_t ncells1, uint32_t* __restrict__ new_start) {
  __shared__ uint32_t lk[kMergeTile];
  const int64_t c0 = (int64_t)blockIdx.x * kMergeTile;
  const int64_t c1 = min(c0 + (int64_t)kMergeTile, ncells1);
  const int t = threadIdx.x;
  const uint32_t j0 = jt[blockIdx.x], m = jt[blockIdx.x + 1] - j0;
  const bool inl = m <= (uint32_t)kMergeTile;
  if (inl)
    for (uint32_t k = t; k < m; k += blockDim.x) lk[k] = sk[j0 + k];
  // every load of the thread's 16 cells in flight before any use (one round
  // trip for the cell table, one for the ranks: a load-use chain per cell
  // made this kernel latency-bound)
  constexpr int kPer = kMergeTile / 256;
  uint32_t os[kPer], r[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int64_t c = c0 + t + 256 * u;
    os[u] = c < c1 ? old_start[c] : 0u;
  }
  const uint32_t n0p = *n0p_p;
#pragma unroll
  for (int u = 0; u < kPer; ++u) r[u] = (int64_t)os[u] < n0 ? rank[os[u]] : n0p;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int64_t c = c0 + t + 256 * u;
    if (c >= c1) continue;
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((inl ? lk[mid] : sk[j0 + mid]) < (uint32_t)c)
        lo = mid + 1;
      else
        hi = mid;
    }
    new_start[c] = r[u] + j0 + lo;
  }
}
__device__ __forceinline__ uint32_t map_cell(const float4& v, const GridGeom& g) {
  const int cx = min(max(cell_coord(v.x, g.ox, g.inv_h), 0), g.dx - 1);
  const int cy = min(max(cell_coord(v.y, g.oy, g.inv_h), 0), g.dy - 1);
  const int cz = min(max(cell_coord(v.z, g.oz, g.inv_h), 0), g.dz - 1);
  return ((uint32_t)cz * (uint32_t)g.dy + (uint32_t)cy) * (uint32_t)g.dx + (uint32_t)cx;
}
// jp[t] = lb(cell of point t * kRankTile), t < ntiles; jp[ntiles] = na.  The
// stored points are in cell order, so a point p of tile t in cell c has
// jp[t] <= lb(c) <= jp[t + 1]
// (and in the same launch jt[t] = lb(t * kMergeTile), t <= ctiles: every
// cell tile's first addition for k_merge_start, one thread per tile -- a
// per-workgroup search at the head of k_merge_start put ~15 dependent loads
// in front of every tile: 294 us for the 10M map's grid)
__global__ void k_merge_ptiles(const float4* __restrict__ pts, int64_t ntiles, GridGeom g,
                               const uint32_t* __restrict__ sk, uint32_t na, uint32_t* __restrict__ jp,
                               int64_t ctiles, int64_t ncells1, uint32_t* __restrict__ jt) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t <= ctiles) {
    jt[t] = lower_bound_u32(sk, 0, na, (uint32_t)min(t * (int64_t)kMergeTile, ncells1));
    return;
  }
  t -= ctiles + 1;
  if (t > ntiles) return;
  jp[t] = t == ntiles ? na : lower_bound_u32(sk, 0, na, map_cell(pts[t * kRankTile], g));
}
// survivor p of cell c goes to new_start[c] + rank[p] - rank(old_start[c])
// = rank[p] + lb(c): one tile of kRankTile points per workgroup, 16 per
// thread with every load in flight before any use, lb(c) from the tile's
// additions in LDS (no per-point cell-table gathers: the dependent
// pts -> old_start -> rank chain made the one-point-per-thread kernel
// latency-bound, ~104 us for the 10M map)
__global__ __launch_bounds__(256) void k_merge_pts(const float4* __restrict__ pts, const uint8_t* __restrict__ keep,
                                                   const uint32_t* __restrict__ rank, const uint32_t* __restrict__ sk,
                                                   const uint32_t* __restrict__ jp, int64_t n0, GridGeom g,
                                                   float4* __restrict__ out, uint8_t* __restrict__ okeep) {
  constexpr int kPer = kRankTile / 256, kLds = 1024;
  __shared__ uint32_t lk[kLds];
  const int64_t p0 = (int64_t)blockIdx.x * kRankTile + threadIdx.x;
  const uint32_t j0 = jp[blockIdx.x], m = jp[blockIdx.x + 1] - j0;
  const bool inl = m <= (uint32_t)kLds;
  if (inl)
    for (uint32_t k = threadIdx.x; k < m; k += 256) lk[k] = sk[j0 + k];
  float4 v[kPer];
  uint32_t r[kPer];
  uint8_t kp[kPer];
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    const int64_t p = p0 + 256 * u;
    kp[u] = p < n0 ? keep[p] : (uint8_t)0;
    v[u] = p < n0 ? pts[p] : make_float4(0.f, 0.f, 0.f, 0.f);
    r[u] = p < n0 ? rank[p] : 0u;
  }
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kPer; ++u) {
    if (!kp[u]) continue;
    const uint32_t c = map_cell(v[u], g);
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if ((inl ? lk[mid] : sk[j0 + mid]) < c)
        lo = mid + 1;
      else
        hi = mid;
    }
    out[r[u] + j0 + lo] = v[u];
    okeep[r[u] + j0 + lo] = 1;
  }
}
// the additions' fine cell keys, dead ones keyed kDeadKey (sorted after
// every live one, and above every cell a lower bound asks for); chk[0] += the
// live count, chk[1] = 1 when a live addition is not a cell inside the grid
// (or not finite): the merge is then void and the caller re-grids by sorting
constexpr uint32_t kDeadKey = 0xFFFFFFFFu;
struct MergeBox {
  float lo[3], hi[3];
};
__global__ __launch_bounds__(256) void k_merge_keys(const float4* __restrict__ adds, const uint8_t* __restrict__ akeep,
                                                    int64_t n1, GridGeom g, MergeBox bx, uint32_t* __restrict__ keys,
                                                    uint32_t* __restrict__ vals, uint32_t* __restrict__ chk) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool live = false, fits = true;
  if (i < n1) {
    live = akeep[i] != 0;
    const float4 v = adds[i];
    fits = v.x >= bx.lo[0] && v.x <= bx.hi[0] && v.y >= bx.lo[1] && v.y <= bx.hi[1] && v.z >= bx.lo[2] &&
           v.z <= bx.hi[2];
    keys[i] = live ? map_cell(v, g) : kDeadKey;
    vals[i] = (uint32_t)i;
  }
  const int cnt = __syncthreads_count(live);
  const int bad = __syncthreads_or(live && !fits);
  if (threadIdx.x == 0) {
    if (cnt) atomicAdd(chk, (uint32_t)cnt);
    if (bad) atomicOr(chk + 1, 1u);
  }
}
__global__ void k_merge_adds(const float4* __restrict__ adds, const uint32_t* __restrict__ sk,
                             const uint32_t* __restrict__ sv, uint32_t na, const uint32_t* __restrict__ new_start,
                             float4* __restrict__ out, uint8_t* __restrict__ okeep) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= na) return;
  const uint32_t c = sk[j];
  if (c == kDeadKey) return;
  const uint32_t e = lower_bound_u32(sk, j, na, c + 1);
  out[new_start[c + 1] - (e - j)] = adds[sv[j]];
  okeep[new_start[c + 1] - (e - j)] = 1;
}

// The merge rebuild (see k_merge_start) of m: *handled = false when the
// additions do not all lie at least one cell inside the grid (then the caller
// rebuilds by sorting, with a new grid).  Stream-ordered and speculative: the
// merge runs into temporaries while k_merge_keys checks the additions, and
// ONE readback (survivor count, live additions, the edge flag) decides
// whether the map takes the result (three synchronisations before: the
// counts, the additions' box, the end).
static int merge_rebuild(MapDev& m, hipStream_t st, bool* handled) {
  *handled = false;
  const int64_t n0 = m.n, n1 = m.nadd;
  const GridGeom g = m.g;
  hipError_t e;
  auto fail = [&](const char* what, hipError_t err) {
    set_error(std::string("slio map merge: ") + what + ": " + hipGetErrorString(err));
    return err == hipErrorOutOfMemory ? SLIO_ENOMEM : SLIO_EDEVICE;
  };
  const int64_t na_cap = std::max<int64_t>(n1, 1);
  const int64_t rtiles = (n0 + kRankTile - 1) / kRankTile;
  const int64_t nc1 = m.ncells + 1, ntiles = (nc1 + kMergeTile - 1) / kMergeTile;
  if ((e = m.take(m.b_ref[1], 4 * (rtiles + 3))) || (e = m.take(m.b_ref[2], 4 * n0)) ||
      (e = m.take(m.b_tmp[1], 4 * na_cap)) || (e = m.take(m.b_tmp[2], 4 * na_cap)) ||
      (e = m.take(m.b_tmp[3], 4 * na_cap)) || (e = m.take(m.b_tmp[4], 4 * na_cap)) ||
      (e = m.take(m.b_tmp[5], 4 * (ntiles + 1))) || (e = m.take(m.b_tmp[6], 4 * (rtiles + 1))) ||
      (e = m.take(m.b_ref[0], 16 * (n0 + n1))) || (e = m.take(m.b_start2, sizeof(uint32_t) * nc1)) ||
      (e = m.take(m.b_keep2, n0 + n1)))
    return fail("hipMalloc", e);
  uint32_t* tcnt = (uint32_t*)m.b_ref[1].p;  // [rtiles] tile bases, survivors, live additions, edge flag
  uint32_t* rank = (uint32_t*)m.b_ref[2].p;
  uint32_t* ak = (uint32_t*)m.b_tmp[1].p;
  uint32_t* sk = (uint32_t*)m.b_tmp[2].p;
  uint32_t* av = (uint32_t*)m.b_tmp[3].p;
  uint32_t* sv = (uint32_t*)m.b_tmp[4].p;
  uint32_t* jt = (uint32_t*)m.b_tmp[5].p;
  uint32_t* jp = (uint32_t*)m.b_tmp[6].p;
  float4* out = (float4*)m.b_ref[0].p;
  uint32_t* new_start = (uint32_t*)m.b_start2.p;
  k_keep_tiles<<<(unsigned)rtiles, 256, 0, st>>>(m.keep, n0, rtiles, tcnt);
  k_tile_scan<<<1, 256, 0, st>>>(tcnt, rtiles);
  k_keep_rank<<<(unsigned)rtiles, 256, 0, st>>>(m.keep, n0, tcnt, rank);
  if (n1) {
    // the live additions must lie a cell inside the kept grid
    MergeBox bx;
    const float o[3] = {g.ox, g.oy, g.oz};
    const int d[3] = {g.dx, g.dy, g.dz};
    for (int a = 0; a < 3; ++a) {
      bx.lo[a] = o[a] + g.h;
      bx.hi[a] = o[a] + (float)(d[a] - 1) * g.h;
    }
    k_merge_keys<<<grid_blocks(n1), 256, 0, st>>>(m.add4, m.akeep, n1, g, bx, ak, av, tcnt + rtiles + 1);
    // (stable: a cell's additions stay in id order; the dead ones sort last)
    size_t tb = 0;
    if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, ak, sk, av, sv, (int)n1, 0, 32, st)) ||
        (e = m.take(m.b_tmp[7], tb)))
      return fail("sort size", e);
    tb = m.b_tmp[7].cap;
    if ((e = hipcub::DeviceRadixSort::SortPairs(m.b_tmp[7].p, tb, ak, sk, av, sv, (int)n1, 0, 32, st)))
      return fail("sort", e);
  }
  uint8_t* okeep = (uint8_t*)m.b_keep2.p;
  k_merge_ptiles<<<grid_blocks(ntiles + rtiles + 2), 256, 0, st>>>(m.pts, rtiles, g, sk, (uint32_t)n1, jp, ntiles,
                                                                    nc1, jt);
  k_merge_start<<<(unsigned)ntiles, 256, 0, st>>>(m.start, rank, n0, tcnt + rtiles, sk, jt, nc1, new_start);
  k_merge_pts<<<(unsigned)rtiles, 256, 0, st>>>(m.pts, m.keep, rank, sk, jp, n0, g, out, okeep);
  if (n1) k_merge_adds<<<grid_blocks(n1), 256, 0, st>>>(m.add4, sk, sv, (uint32_t)n1, new_start, out, okeep);
  // coarse level: the boxes widened by the additions (deleted points leave
  // them conservative); the points themselves are the fine runs.  In place
  // before the readback: a declined merge re-grids by sorting, which builds
  // the coarse level anew
  if (n1) k_coarse_extend<<<grid_blocks(n1), 256, 0, st>>>(m.add4, m.akeep, n1, g, m.clo, m.chi, m.cg);
  if ((e = hipGetLastError())) return fail("merge kernels", e);
  uint32_t cnt[3] = {0, 0, 0};
  {
    const Rb rb{cnt, tcnt + rtiles, 12};
    if ((e = readback(st, &rb, 1))) return fail("counts", e);
  }
  if (cnt[2]) return SLIO_OK;  // an addition near or past the grid's edge (or non-finite): re-grid by sorting
  const uint32_t n0p = cnt[0], na = cnt[1];
  *handled = true;
  const int64_t n = (int64_t)n0p + na;
  // new views: points and cell table swap buffers with their temporaries
  std::swap(m.b_pts, m.b_ref[0]);
  std::swap(m.b_start, m.b_start2);
  m.pts = (float4*)m.b_pts.p;
  m.start = (uint32_t*)m.b_start.p;
  m.n = n;
  std::swap(m.b_keep, m.b_keep2);  // (set by k_merge_pts / k_merge_adds)
  m.keep = (uint8_t*)m.b_keep.p;
  // the boxes only widen through merges: once the deletions since they were
  // tight pass n / kCoarseRetighten, the coarse level is rebuilt from the new
  // cell table -- the boxes a sorting rebuild gives
  m.del_loose += n0 - (int64_t)n0p;
  if (m.del_loose * kCoarseRetighten > n) {
    if ((e = m.take(m.b_tmp[6], 4 * (m.nccells + 1)))) return fail("hipMalloc", e);
    uint32_t* ccnt = (uint32_t*)m.b_tmp[6].p;
    k_coarse_count<<<grid_blocks(m.nccells), 256, 0, st>>>(m.start, g, m.cg, m.nccells, ccnt);
    k_coarse_boxes<<<grid_blocks(m.nccells), 256, 0, st>>>(m.pts, m.start, g, m.cg, ccnt, m.nccells, m.clo, m.chi);
    if ((e = hipGetLastError())) return fail("coarse boxes", e);
    m.del_loose = 0;
  }
  m.blk = nullptr;
  m.bstart = nullptr;
  m.nblk = 0;
  m.blk_deferred = block_rows_wanted(m);
  m.stable_passes = 0;
#ifdef SLIO_BOUNDS_CHECK
  dbg_set_bounds(n, m.ncells);
#endif
  if (std::getenv("SLIO_DEBUG_REBUILD"))
    std::fprintf(stderr, "slio rebuild: merge n %lld (survivors %u of %lld, additions %u of %lld)\n", (long long)n,
                 n0p, (long long)n0, na, (long long)n1);
  return SLIO_OK;
}

// Rebuild the index from the surviving points and the pending additions
// (when the map changed since the last build).  adds_only: only when points
// were added (deletions alone are honoured through the keep flags).
int map_refresh(Ctx& c, bool adds_only) {
  if (!c.map || !c.map->dirty) return SLIO_OK;
  std::unique_lock<std::shared_mutex> lk(c.map->mu);
  if (!c.map->dirty) return SLIO_OK;  // another user rebuilt it meanwhile
  if (int rc = map_read_sync(c)) return rc;
  if (int rc = map_write_begin(c)) return rc;
  const int rc = map_refresh_locked(c, adds_only);
  const int rc2 = map_write_end(c);
  return rc ? rc : rc2;
}

// the rebuild itself: MapDev::mu held exclusively, the stream ordered after
// the other users (map_write_begin)
static int map_refresh_locked(Ctx& c, bool adds_only) {
  if (!c.map || !c.map->dirty) return SLIO_OK;
  MapDev& m = *c.map;
  if (adds_only && m.nadd == 0) return SLIO_OK;
  if (int rc = nbr_settle(c)) return rc;  // the rebuild moves the points
  hipStream_t st = c.stream;
  const int64_t n0 = m.n, n1 = m.nadd, nt = n0 + n1;
  {
    // a grid that still holds every point: merge instead of sorting
    // (SLIO_NO_MERGE=1: always sort)
    const char* nm = std::getenv("SLIO_NO_MERGE");
    if (n0 > 0 && m.start && m.clo && !(nm && nm[0] && nm[0] != '0')) {
      bool handled = false;
      const int rc = merge_rebuild(m, st, &handled);
      if (handled || rc) {
        if (rc) {
          m.broken = true;
          m.free_index();
        }
        m.nadd = 0;
        m.version++;
        m.dirty = false;
        return rc;
      }
    }
  }
  hipError_t e;
  // survivors: stored points (cell order) and additions (id order) compacted
  // into in4; the sort in build_index orders them by (cell, id) anyway
  if ((e = m.take(m.b_ref[0], 16 * nt)) || (e = m.take(m.b_ref[1], 4 * nt)) || (e = m.take(m.b_ref[2], 4 * nt)) ||
      (e = m.take(m.b_ref[3], 32))) {
    set_error(std::string("slio map rebuild: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  float4* in4 = (float4*)m.b_ref[0].p;
  uint32_t* flag = (uint32_t*)m.b_ref[1].p;
  uint32_t* rank = (uint32_t*)m.b_ref[2].p;
  int32_t* bb = (int32_t*)m.b_ref[3].p;
  if (n0) k_widen_flags<<<grid_blocks(n0), 256, 0, st>>>(m.keep, n0, flag);
  if (n1) k_widen_flags<<<grid_blocks(n1), 256, 0, st>>>(m.akeep, n1, flag + n0);
  uint32_t total = 0;
  if (int rc = scan_flags(flag, rank, nt, st, &total)) return rc;
  const int64_t n = total;
  if (n0) k_compact4<<<grid_blocks(n0), 256, 0, st>>>(m.pts, flag, rank, n0, in4);
  // (the ranks of the additions continue the stored points': one scan)
  if (n1) k_compact4<<<grid_blocks(n1), 256, 0, st>>>(m.add4, flag + n0, rank + n0, n1, in4);
  const int32_t init[8] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0};
  int32_t got[8];
  if ((e = hipMemcpyAsync(bb, init, 32, hipMemcpyHostToDevice, st))) {
    set_error(std::string("slio map rebuild: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  if (n) k_bbox4<<<std::min(grid_blocks(n), 512), 256, 0, st>>>(in4, n, bb);
  const Rb rbb{got, bb, 32};
  if ((e = readback(st, &rbb, 1))) {
    set_error(std::string("slio map rebuild: bbox: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  if (got[6]) {
    set_error("slio map rebuild: non-finite map coordinate");
    return SLIO_EINVAL;
  }
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  if (n)
    for (int a = 0; a < 3; ++a) {
      mn[a] = fkey_inv(got[a]);
      mx[a] = fkey_inv(got[3 + a]);
    }
  // in4 is b_ref[0]: build_index reads it while writing the b_* tables
  const bool had_points = n0 > 0;
  m.free_index();
  m.nadd = 0;
  const int rc = build_index(m, in4, n, mn, mx, st, "slio map rebuild", false, true, had_points);
  if (rc) {
    // part-way: the stored points are gone from the views; fail every later
    // use of the map instead of searching a partial index
    m.broken = true;
    m.free_index();
  }
  m.version++;
  m.dirty = false;
  return rc;
}

}  // namespace slio

using namespace slio;

extern "C" {

int slio_map_upload(slio_handle h, const float* x, const float* y, const float* z, int64_t n) {
  SLIO_CHECK_H(h);
  if (n < 0 || (n > 0 && (!x || !y || !z)) || n >= (int64_t)0xFFFFFFFFll) {
    set_error("slio_map_upload: bad arguments");
    return SLIO_EINVAL;
  }
  auto m = std::make_shared<MapDev>();
  m->device = h->c.prm.device;
  m->cell0 = h->c.prm.grid_cell;
  m->max_cells = h->c.prm.max_grid_cells;
  m->next_id = (uint32_t)n;
  hipStream_t st = h->c.stream;
  // bounding box on the host (the snapshot is host-resident anyway)
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  const float* xyz[3] = {x, y, z};
  for (int a = 0; a < 3; ++a) {
    if (n == 0) break;
    float lo = xyz[a][0], hi = xyz[a][0];
    for (int64_t i = 0; i < n; ++i) {
      const float v = xyz[a][i];
      if (!std::isfinite(v)) {
        set_error("slio_map_upload: non-finite map coordinate");
        return SLIO_EINVAL;
      }
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    mn[a] = lo;
    mx[a] = hi;
  }
  float *dx_ = nullptr, *dy_ = nullptr, *dz_ = nullptr;
  float4* in4 = nullptr;
  int rc = SLIO_OK;
  if (n > 0) {
    hipError_t e;
    if ((e = hipMalloc(&dx_, 4 * n)) || (e = hipMalloc(&dy_, 4 * n)) || (e = hipMalloc(&dz_, 4 * n)) ||
        (e = hipMalloc(&in4, 16 * n))) {
      set_error(std::string("slio_map_upload: hipMalloc: ") + hipGetErrorString(e));
      rc = SLIO_ENOMEM;
    } else if ((e = hipMemcpyAsync(dx_, x, 4 * n, hipMemcpyHostToDevice, st)) ||
               (e = hipMemcpyAsync(dy_, y, 4 * n, hipMemcpyHostToDevice, st)) ||
               (e = hipMemcpyAsync(dz_, z, 4 * n, hipMemcpyHostToDevice, st))) {
      set_error(std::string("slio_map_upload: H2D: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
    } else {
      k_pack_ids<<<grid_blocks(n), 256, 0, st>>>(dx_, dy_, dz_, n, 0u, in4);
    }
  }
  if (!rc) rc = build_index(*m, in4, n, mn, mx, st, "slio_map_upload");
  for (void* q : {(void*)dx_, (void*)dy_, (void*)dz_, (void*)in4})
    if (q) (void)hipFree(q);
  if (rc) return rc;
  {
    // sharers of this map order their streams after its build
    SLIO_HIP(hipEventCreateWithFlags(&m->ready, hipEventDisableTiming));
    SLIO_HIP(hipEventRecord(m->ready, st));
    m->epoch = 1;
  }
  if ((rc = nbr_settle_shared(h->c))) return rc;
  map_attach(h->c, m);
  h->c.seen_epoch = 1;
  h->c.searched = false;
  return SLIO_OK;
}

int slio_map_share(slio_handle h, slio_handle src) {
  SLIO_CHECK_H(h);
  if (!src || !src->c.map || src->c.prm.device != h->c.prm.device) {
    set_error("slio_map_share: source has no map on this device");
    return SLIO_EINVAL;
  }
  if (h == src) return SLIO_OK;
  if (int rc = nbr_settle_shared(h->c)) return rc;
  map_attach(h->c, src->c.map);
  h->c.searched = false;
  return SLIO_OK;
}

int slio_map_info(slio_handle h, int32_t dims[3], float* cell, int64_t* n) {
  SLIO_CHECK_H(h);
  if (!h->c.map) {
    set_error("slio_map_info: no map");
    return SLIO_ESTATE;
  }
  if (int rc = map_refresh(h->c)) return rc;
  std::shared_lock<std::shared_mutex> lk(h->c.map->mu);
  if (dims) {
    dims[0] = h->c.map->g.dx;
    dims[1] = h->c.map->g.dy;
    dims[2] = h->c.map->g.dz;
  }
  if (cell) *cell = h->c.map->g.h;
  if (n) *n = h->c.map->n;
  return SLIO_OK;
}

int slio_map_add_points(slio_handle h, const float* x, const float* y, const float* z, int64_t n,
                        int downsample, float downsample_size, int64_t* counter) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (!c.map) {
    set_error("slio_map_add_points: no map");
    return SLIO_ESTATE;
  }
  if (n < 0 || (n > 0 && (!x || !y || !z)) || (downsample && !(downsample_size > 0.0f))) {
    set_error("slio_map_add_points: bad arguments");
    return SLIO_EINVAL;
  }
  for (int64_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i]) || !std::isfinite(y[i]) || !std::isfinite(z[i])) {
      set_error("slio_map_add_points: non-finite coordinate");
      return SLIO_EINVAL;
    }
  int64_t cnt = 0;
  if (n > 0) {
    std::unique_lock<std::shared_mutex> lk(c.map->mu);
    if (int rc = map_read_sync(c)) return rc;
    if (int rc = map_write_begin(c)) return rc;
    float *dx_ = nullptr, *dy_ = nullptr, *dz_ = nullptr;
    float4* in4 = nullptr;
    int rc = SLIO_OK;
    hipError_t e;
    if ((e = hipMalloc(&dx_, 4 * n)) || (e = hipMalloc(&dy_, 4 * n)) || (e = hipMalloc(&dz_, 4 * n)) ||
        (e = hipMalloc(&in4, 16 * n))) {
      set_error(std::string("slio_map_add_points: hipMalloc: ") + hipGetErrorString(e));
      rc = SLIO_ENOMEM;
    } else if ((e = hipMemcpyAsync(dx_, x, 4 * n, hipMemcpyHostToDevice, c.stream)) ||
               (e = hipMemcpyAsync(dy_, y, 4 * n, hipMemcpyHostToDevice, c.stream)) ||
               (e = hipMemcpyAsync(dz_, z, 4 * n, hipMemcpyHostToDevice, c.stream))) {
      set_error(std::string("slio_map_add_points: H2D: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
    } else {
      k_pack_ids<<<grid_blocks(n), 256, 0, c.stream>>>(dx_, dy_, dz_, n, 0u, in4);
      rc = map_add(c, in4, n, downsample != 0, downsample_size, &cnt);
      if (!rc) (void)spin_sync(c.stream);
    }
    if (int rc2 = map_write_end(c); rc2 && !rc) rc = rc2;
    for (void* q : {(void*)dx_, (void*)dy_, (void*)dz_, (void*)in4})
      if (q) (void)hipFree(q);
    if (rc) return rc;
  }
  if (counter) *counter = cnt;
  return SLIO_OK;
}

int slio_map_delete_boxes(slio_handle h, const float* boxes, int64_t nboxes, int64_t* deleted) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (!c.map) {
    set_error("slio_map_delete_boxes: no map");
    return SLIO_ESTATE;
  }
  if (nboxes < 0 || (nboxes > 0 && !boxes)) {
    set_error("slio_map_delete_boxes: bad arguments");
    return SLIO_EINVAL;
  }
  MapDev& m = *c.map;
  std::unique_lock<std::shared_mutex> lk(m.mu);
  if (int rc = map_read_sync(c)) return rc;
  if (int rc = map_write_begin(c)) return rc;
  unsigned long long* dc = nullptr;
  SLIO_HIP(hipMalloc(&dc, 8));
  SLIO_HIP(hipMemsetAsync(dc, 0, 8, c.stream));
  for (int64_t b0 = 0; b0 < nboxes; b0 += 8) {
    Boxes8 bx{};
    bx.n = (int)std::min<int64_t>(8, nboxes - b0);
    for (int k = 0; k < bx.n; ++k)
      for (int j = 0; j < 6; ++j) bx.b[k][j] = boxes[6 * (b0 + k) + j];
    if (m.n) k_map_delete<<<grid_blocks(m.n), 256, 0, c.stream>>>(m.pts, m.keep, m.n, bx, dc);
    if (m.nadd) k_map_delete<<<grid_blocks(m.nadd), 256, 0, c.stream>>>(m.add4, m.akeep, m.nadd, bx, dc);
  }
  unsigned long long k = 0;
  hipError_t e = hipMemcpyAsync(&k, dc, 8, hipMemcpyDeviceToHost, c.stream);
  if (!e) e = hipStreamSynchronize(c.stream);
  (void)hipFree(dc);
  if (e) {
    set_error(std::string("slio_map_delete_boxes: ") + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  if (k) m.dirty = true;
  if (deleted) *deleted = (int64_t)k;
  return map_write_end(c);
}

// map_incremental's two Add_Points in one stream of launches with ONE
// readback (exact hash boxes, nothing pending in the index): the lists'
// counts, the survivors and the counters stay on the device until the end,
// where the classify counts used to be read back first and the appends
// launched after.  *fallback: a voxel key outside ds_key's range (nothing
// added, no flag changed): the caller takes the per-call path.
static int map_incremental_hashed(Ctx& c, const float4* w4, uint32_t* fa, uint32_t* fn, uint32_t* ra,
                                  uint32_t* rn, float4* l1, float4* l2, int64_t n, float ds, int64_t out[3],
                                  bool* fallback) {
  MapDev& m = *c.map;
  hipStream_t st = c.stream;
  *fallback = false;
  const int nb = grid_blocks(n);
  if (int rc = scan_launch(fa, ra, n, st)) return rc;
  if (int rc = scan_launch(fn, rn, n, st)) return rc;
  k_compact4<<<nb, 256, 0, st>>>(w4, fa, ra, n, l1);
  k_compact4<<<nb, 256, 0, st>>>(w4, fn, rn, n, l2);
  int hb = 10;
  while (((int64_t)1 << hb) < 2 * n) ++hb;
  const int64_t H = (int64_t)1 << hb;
  auto& B = m.b_add;
  hipError_t e;
  if ((e = m.take(B[0], 8 * H)) || (e = m.take(B[1], 4 * H)) || (e = m.take(B[2], 4 * kDsInline * H)) ||
      (e = m.take(B[4], 4 * n)) || (e = m.take(B[5], 4 * n)) || (e = m.take(B[6], 64))) {
    set_error(std::string("slio map: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  uint64_t* hkey = (uint64_t*)B[0].p;
  uint32_t* hcnt = (uint32_t*)B[1].p;
  uint32_t* hmem = (uint32_t*)B[2].p;
  uint32_t* surv = (uint32_t*)B[4].p;
  uint32_t* rank = (uint32_t*)B[5].p;
  unsigned long long* dcount = (unsigned long long*)B[6].p;  // [0, 24): ops, -, out of range; [24, 36): counts
  uint32_t* cnt = (uint32_t*)((char*)B[6].p + 24);
  if (int rc = add_reserve(m, 2 * n, st)) return rc;
  k_ds_init<<<grid_blocks(std::max<int64_t>(H, n)), 256, 0, st>>>(hkey, hcnt, H, surv, n, dcount);
  k_ds_hash<<<nb, 256, 0, st>>>(l1, n, ds, hb, hkey, hcnt, hmem, dcount + 2, ra + n - 1, fa + n - 1);
  k_ds_groups_hash<<<grid_blocks(H), 256, 0, st>>>(l1, n, ds, hb, hkey, hcnt, hmem, map_view(m), m.keep, surv,
                                                   dcount);
  if (int rc = scan_launch(surv, rank, n, st)) return rc;
  k_append<<<nb, 256, 0, st>>>(l1, surv, rank, n, m.add4, m.akeep, m.nadd, m.next_id);
  k_append_after<<<nb, 256, 0, st>>>(l2, n, rn + n - 1, fn + n - 1, rank + n - 1, surv + n - 1, m.add4, m.akeep,
                                     m.nadd, m.next_id);
  k_inc_counts<<<1, 64, 0, st>>>(ra + n - 1, fa + n - 1, rn + n - 1, fn + n - 1, rank + n - 1, surv + n - 1, cnt);
  unsigned long long got[5];  // ops, -, out of range, then the three counts as 32-bit words
  {
    const Rb rb{got, dcount, 36};
    if ((e = hipGetLastError()) || (e = readback(st, &rb, 1))) {
      set_error(std::string("slio_map_incremental: ") + hipGetErrorString(e));
      return SLIO_EDEVICE;
    }
  }
  if (got[2]) {
    *fallback = true;
    return SLIO_OK;
  }
  uint32_t k3[3];
  std::memcpy(k3, &got[3], 12);
  const uint32_t na = k3[0], nn = k3[1], total = k3[2];
  out[0] = na;
  out[1] = nn;
  out[2] = (int64_t)got[0];
  m.nadd += (int64_t)total + nn;
  m.next_id += total + nn;
  if (na || nn) m.dirty = true;  // deletions (keep flags) and / or additions (as the per-call path)
  return SLIO_OK;
}

int slio_map_incremental(slio_handle h, const slio_state* x, double filter_size_map_min, int ekf_inited,
                         int64_t counts[3]) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (!x || !(filter_size_map_min > 0.0)) {
    set_error("slio_map_incremental: bad arguments");
    return SLIO_EINVAL;
  }
  if (!c.map) {
    set_error("slio_map_incremental: no map");
    return SLIO_ESTATE;
  }
  std::unique_lock<std::shared_mutex> map_lock(c.map->mu);
  if (!c.searched || c.search_version != c.map->version) {
    set_error("slio_map_incremental: no search pass on the current map (Nearest_Points)");
    return SLIO_ESTATE;
  }
  if (int rc = map_read_sync(c)) return rc;
  if (int rc = map_write_begin(c)) return rc;
  if (c.prm.nranks != 1) {
    set_error("slio_map_incremental: needs the whole scan (nranks == 1)");
    return SLIO_EINVAL;
  }
  const int64_t n = c.n;
  WorldMat W;
  {
    // Eigen Quaternion::toRotationMatrix (Sophus SO3::matrix)
    auto mat = [](const double* q, double* R) {
      const double w = q[0], qx = q[1], qy = q[2], qz = q[3];
      const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
      const double twx = tx * w, twy = ty * w, twz = tz * w;
      const double txx = tx * qx, txy = ty * qx, txz = tz * qx;
      const double tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
      R[0] = 1.0 - (tyy + tzz);
      R[1] = txy - twz;
      R[2] = txz + twy;
      R[3] = txy + twz;
      R[4] = 1.0 - (txx + tzz);
      R[5] = tyz - twx;
      R[6] = txz - twy;
      R[7] = tyz + twx;
      R[8] = 1.0 - (txx + tyy);
    };
    mat(x->rot, W.R);
    mat(x->rli, W.RL);
    for (int k = 0; k < 3; ++k) {
      W.pos[k] = x->pos[k];
      W.tli[k] = x->tli[k];
    }
  }
  int64_t out[3] = {0, 0, 0};
  if (n > 0) {
    float4 *w4 = nullptr, *l1 = nullptr, *l2 = nullptr;
    uint32_t *fa = nullptr, *fn = nullptr, *ra = nullptr, *rn = nullptr;
    int rc = SLIO_OK;
    do {
      hipError_t e;
      auto& B = c.inc;  // kept across scans (hipFree would synchronise the device)
      if ((e = MapDev::take(B[0], 16 * n)) || (e = MapDev::take(B[1], 16 * n)) ||
          (e = MapDev::take(B[2], 16 * n)) || (e = MapDev::take(B[3], 4 * n)) ||
          (e = MapDev::take(B[4], 4 * n)) || (e = MapDev::take(B[5], 4 * n)) || (e = MapDev::take(B[6], 4 * n))) {
        set_error(std::string("slio_map_incremental: hipMalloc: ") + hipGetErrorString(e));
        rc = SLIO_ENOMEM;
        break;
      }
      w4 = (float4*)B[0].p;
      l1 = (float4*)B[1].p;
      l2 = (float4*)B[2].p;
      fa = (uint32_t*)B[3].p;
      fn = (uint32_t*)B[4].p;
      ra = (uint32_t*)B[5].p;
      rn = (uint32_t*)B[6].p;
      const int nb = grid_blocks(n);
      k_map_classify<<<nb, 256, 0, c.stream>>>(c.bx, c.by, c.bz, n, W, c.nbr_pos, c.map->pts,
                                               filter_size_map_min, ekf_inited, w4, fa, fn);
      {
        MapDev& m = *c.map;
        const float ds = (float)filter_size_map_min;
        int ds_exp = 0;
        const char* nh = std::getenv("SLIO_NO_DS_HASH");
        if (!(nh && nh[0] && nh[0] != '0') && std::frexp(ds, &ds_exp) == 0.5f && ds <= 1.0f &&
            !(m.dirty && m.nadd > 0) && (int64_t)m.next_id + 2 * n < (int64_t)0x7FFFFFFF) {
          bool fallback = false;
          if ((rc = map_incremental_hashed(c, w4, fa, fn, ra, rn, l1, l2, n, ds, out, &fallback))) break;
          if (!fallback) break;
        }
      }
      uint32_t na = 0, nn = 0;
      if ((rc = scan_flags2(fa, ra, fn, rn, n, c.stream, &na, &nn))) break;
      k_compact4<<<nb, 256, 0, c.stream>>>(w4, fa, ra, n, l1);
      k_compact4<<<nb, 256, 0, c.stream>>>(w4, fn, rn, n, l2);
      out[0] = na;
      out[1] = nn;
      int64_t cnt = 0, cnt2 = 0;
      if ((rc = map_add(c, l1, na, true, (float)filter_size_map_min, &cnt))) break;
      if ((rc = map_add(c, l2, nn, false, (float)filter_size_map_min, &cnt2))) break;
      out[2] = cnt;
      SLIO_HIP(spin_sync(c.stream));
    } while (0);
    if (int rc2 = map_write_end(c); rc2 && !rc) rc = rc2;
    if (rc) return rc;
  }
  if (counts)
    for (int k = 0; k < 3; ++k) counts[k] = out[k];
  return SLIO_OK;
}

int slio_map_download(slio_handle h, float* x, float* y, float* z, uint32_t* ids, int64_t cap, int64_t* n) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (!c.map) {
    set_error("slio_map_download: no map");
    return SLIO_ESTATE;
  }
  if (int rc = map_refresh(c)) return rc;
  std::shared_lock<std::shared_mutex> lk(c.map->mu);
  if (int rc = map_read_sync(c)) return rc;
  const MapDev& m = *c.map;
  if (n) *n = m.n;
  if (cap < m.n || (m.n > 0 && (!x || !y || !z || !ids))) {
    set_error("slio_map_download: buffer too small");
    return SLIO_ECAPACITY;
  }
  std::vector<float4> buf((size_t)m.n);
  if (m.n) {
    SLIO_HIP(hipMemcpyAsync(buf.data(), m.pts, 16 * m.n, hipMemcpyDeviceToHost, c.stream));
    SLIO_HIP(hipStreamSynchronize(c.stream));
  }
  std::vector<std::pair<uint32_t, uint32_t>> order((size_t)m.n);
  for (int64_t i = 0; i < m.n; ++i) {
    uint32_t id;
    std::memcpy(&id, &buf[i].w, 4);
    order[i] = {id, (uint32_t)i};
  }
  std::sort(order.begin(), order.end());
  for (int64_t k = 0; k < m.n; ++k) {
    const float4& p = buf[order[k].second];
    x[k] = p.x;
    y[k] = p.y;
    z[k] = p.z;
    ids[k] = order[k].first;
  }
  return SLIO_OK;
}

// test support (not in include/slio.h): the index's points in their stored
// (cell, id) order, x, y, z, bits(id) per point, after the pending rebuild
int slio_dbg_map_raw(slio_handle h, float* xyzw, int64_t cap, int64_t* n) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (!c.map || !n) return SLIO_ESTATE;
  if (int rc = map_refresh(c)) return rc;
  std::shared_lock<std::shared_mutex> lk(c.map->mu);
  if (int rc = map_read_sync(c)) return rc;
  *n = c.map->n;
  if (cap < c.map->n || (c.map->n > 0 && !xyzw)) return SLIO_ECAPACITY;
  if (c.map->n) {
    SLIO_HIP(hipMemcpyAsync(xyzw, c.map->pts, 16 * c.map->n, hipMemcpyDeviceToHost, c.stream));
    SLIO_HIP(hipStreamSynchronize(c.stream));
  }
  return SLIO_OK;
}

// test support (not in include/slio.h): the coarse level's boxes, lo then hi
// (nccells float4 each: x, y, z and the count word), after the pending rebuild
int slio_dbg_map_coarse(slio_handle h, float* lohi, int64_t cap, int64_t* nccells) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (!c.map || !nccells) return SLIO_ESTATE;
  if (int rc = map_refresh(c)) return rc;
  std::shared_lock<std::shared_mutex> lk(c.map->mu);
  if (int rc = map_read_sync(c)) return rc;
  const int64_t nc = c.map->nccells;
  *nccells = nc;
  if (cap < 2 * nc || (nc > 0 && !lohi)) return SLIO_ECAPACITY;
  if (nc) {
    SLIO_HIP(hipMemcpyAsync(lohi, c.map->clo, 16 * nc, hipMemcpyDeviceToHost, c.stream));
    SLIO_HIP(hipMemcpyAsync(lohi + 4 * nc, c.map->chi, 16 * nc, hipMemcpyDeviceToHost, c.stream));
    SLIO_HIP(hipStreamSynchronize(c.stream));
  }
  return SLIO_OK;
}

int slio_fov_segment(const double pos_lid[3], float box_min[3], float box_max[3], int* initialized,
                     double cube_len, float det_range, float boxes_out[18], int* nboxes) {
  if (!pos_lid || !box_min || !box_max || !initialized || !boxes_out || !nboxes) {
    set_error("slio_fov_segment: bad arguments");
    return SLIO_EINVAL;
  }
  // lasermap_fov_segment (laserMapping.cpp:309-365), MOV_THRESHOLD 1.5 (:40)
  const float kMov = 1.5f;
  *nboxes = 0;
  if (!*initialized) {
    for (int i = 0; i < 3; ++i) {
      box_min[i] = (float)(pos_lid[i] - cube_len / 2.0);
      box_max[i] = (float)(pos_lid[i] + cube_len / 2.0);
    }
    *initialized = 1;
    return SLIO_OK;
  }
  float dist[3][2];
  bool need_move = false;
  for (int i = 0; i < 3; ++i) {
    dist[i][0] = (float)std::fabs(pos_lid[i] - box_min[i]);
    dist[i][1] = (float)std::fabs(pos_lid[i] - box_max[i]);
    if (dist[i][0] <= kMov * det_range || dist[i][1] <= kMov * det_range) need_move = true;
  }
  if (!need_move) return SLIO_OK;
  float nmin[3], nmax[3];
  for (int i = 0; i < 3; ++i) {
    nmin[i] = box_min[i];
    nmax[i] = box_max[i];
  }
  const float mov = (float)std::max((cube_len - 2.0 * kMov * det_range) * 0.5 * 0.9,
                                    double(det_range * (kMov - 1)));
  int k = 0;
  for (int i = 0; i < 3; ++i) {
    float tmin[3] = {box_min[0], box_min[1], box_min[2]}, tmax[3] = {box_max[0], box_max[1], box_max[2]};
    if (dist[i][0] <= kMov * det_range) {
      nmax[i] -= mov;
      nmin[i] -= mov;
      tmin[i] = box_max[i] - mov;
    } else if (dist[i][1] <= kMov * det_range) {
      nmax[i] += mov;
      nmin[i] += mov;
      tmax[i] = box_min[i] + mov;
    } else {
      continue;
    }
    for (int j = 0; j < 3; ++j) {
      boxes_out[6 * k + j] = tmin[j];
      boxes_out[6 * k + 3 + j] = tmax[j];
    }
    ++k;
  }
  for (int i = 0; i < 3; ++i) {
    box_min[i] = nmin[i];
    box_max[i] = nmax[i];
  }
  *nboxes = k;
  return SLIO_OK;
}

}  // extern "C"
