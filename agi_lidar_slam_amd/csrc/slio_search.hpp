// slio_search.hpp -- the device search primitives the IKF runtime
// (slio_device.hip, slio_map.hip) and the mapping back-ends (slio_mapopt.hip) compile:
// the grid views a kernel receives, the sorted top-5 list, the exactness bound
// of a fine cube and the whole-wavefront search on the coarse level.  The
// library is built without relocatable device code, so every function here is
// __forceinline__ and the header holds no __device__ or __constant__ variable
// (each file would get its own), no diagnostic stamp and no bounds-check macro.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace slio {

constexpr uint64_t kInfKey = ~0ull;

struct GridGeom {
  float ox, oy, oz;   // origin = bbox min
  float h, inv_h;     // cell edge and its reciprocal
  float tol;          // conservative slack on cell-boundary coordinates
  int dx, dy, dz;     // dims
};

// Coarse level for the queries the fine grid cannot finish cheaply (5th
// neighbour beyond the 5x5x5 fine cube, query cells outside the grid): cells
// of edge 4h on the fine grid's origin -- coarse cell (cx, cy, cz) is the fine
// cells [4cx, 4cx + 4) x [4cy, 4cy + 4) x [4cz, 4cz + 4), so its points are 16
// runs of the fine cell-sorted pts (one per fine (y, z) row) -- and a bounding
// box of every coarse cell's points: exact pruning, since a float distance to
// a point is never below the float distance to a box that contains it, both
// rounded monotonically.  An upload or a sorting rebuild makes the boxes
// tight; a merge rebuild (the live map) only widens them by its additions
// (k_coarse_extend): a deleted point leaves a box merely conservative.  No
// coarse copy of the points, so a merge rebuild does not rewrite one.
struct CoarseView {
  GridGeom g;               // h = 4 x the fine cell edge
  const float4* lo;         // per coarse cell: min x, y, z, bits(points ever counted: 0 = empty)
  const float4* hi;         // per coarse cell: max x, y, z
};

// trivially-copyable kernel argument view of a MapDev
struct MapView {
  GridGeom g;
  int64_t n;
  const float4* pts;
  const uint32_t* start;
  const float4* blk;       // null: the 3x3x3 block is scanned as 9 runs of pts
  const uint32_t* bstart;
  int64_t nblk;
  int64_t ncells;
  CoarseView cl;
};

__device__ __host__ __forceinline__ int cell_coord(float p, float o, float inv_h) {
  float t = floorf((p - o) * inv_h);
  t = fminf(fmaxf(t, -1.0e8f), 1.0e8f);
  return (int)t;
}

// Sorted top-5 list of 64-bit keys (float bits(squared distance) << 32) |
// position in the cell-sorted map: one u64 compare orders by distance, then
// by map position (squared distances are >= +0, whose bit patterns sort like
// the values).  The map index is read back from the point (float4.w) only for
// the five winners.
struct Top5 {
  uint64_t k[5];
};

__device__ __forceinline__ void top5_clear(Top5& t) {
#pragma unroll
  for (int j = 0; j < 5; ++j) t.k[j] = kInfKey;
}

// Branch-free insertion: slot j takes k[j-1] if key < k[j-1], key if
// k[j-1] <= key < k[j], else keeps k[j]; a key >= k[4] changes nothing.  All
// five slots update in parallel (no serial compare-swap chain, no divergent
// branch: across a wavefront some lane nearly always inserts).
__device__ __forceinline__ void top5_insert(Top5& t, uint64_t key) {
  bool c[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) c[j] = key < t.k[j];
#pragma unroll
  for (int j = 4; j > 0; --j) t.k[j] = c[j - 1] ? t.k[j - 1] : (c[j] ? key : t.k[j]);
  t.k[0] = c[0] ? key : t.k[0];
}

// 64-bit lane exchange by DPP (a VALU operand modifier, no LDS round trip)
template <int CTRL>
__device__ __forceinline__ uint64_t dpp64(uint64_t v) {
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xF, 0xF, false);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xF, 0xF, false);
  return ((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo;
}

template <int CTRL>
__device__ __forceinline__ void merge_round_dpp(Top5& t) {
  uint64_t ok[5];
#pragma unroll
  for (int j = 0; j < 5; ++j) ok[j] = dpp64<CTRL>(t.k[j]);
#pragma unroll
  for (int j = 0; j < 5; ++j) top5_insert(t, ok[j]);
}

// butterfly merge of the LPQ per-lane lists of a query group (lanes of a
// group are consecutive and aligned, and all active or all inactive).  Up to
// 16 lanes by DPP: quad_perm [1,0,3,2] and [2,3,0,1] merge each quad, then
// row_half_mirror (lane i <-> 7 - i) pairs the two quads of 8 lanes and
// row_mirror (i <-> 15 - i) the two halves of 16; wider groups by ds_bpermute.
template <int LPQ>
__device__ __forceinline__ void group_merge(Top5& t) {
  if (LPQ >= 2) merge_round_dpp<0xB1>(t);
  if (LPQ >= 4) merge_round_dpp<0x4E>(t);
  if (LPQ >= 8) merge_round_dpp<0x141>(t);
  if (LPQ >= 16) merge_round_dpp<0x140>(t);
#pragma unroll
  for (int m = 16; m < LPQ; m <<= 1) {
    uint64_t ok[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) ok[j] = __shfl_xor(t.k[j], m);
#pragma unroll
    for (int j = 0; j < 5; ++j) top5_insert(t, ok[j]);
  }
}

// Exactness bound: every map point outside cube [c-r, c+r] lies at least this
// far from q (minus float slack); +inf when the cube covers the grid.
__device__ __forceinline__ float outside_bound(const GridGeom& g, int cx, int cy, int cz, int r,
                                               float qx, float qy, float qz, bool& covers) {
  const float INF = __int_as_float(0x7f800000);
  float b = INF;
  covers = true;
  auto axis = [&](int c, int d, float o, float q) {
    if (c - r > 0) {
      covers = false;
      const float face = o + (float)(c - r) * g.h + g.tol;
      b = fminf(b, q - face);
    }
    if (c + r < d - 1) {
      covers = false;
      const float face = o + (float)(c + r + 1) * g.h - g.tol;
      b = fminf(b, face - q);
    }
  };
  axis(cx, g.dx, g.ox, qx);
  axis(cy, g.dy, g.oy, qy);
  axis(cz, g.dz, g.oz, qz);
  return b;
}

__device__ __forceinline__ void wave_fence() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// exclusive prefix sum over the wavefront's 64 lanes; total to every lane
__device__ __forceinline__ uint32_t wave_excl_scan(uint32_t v, uint32_t& total) {
  const int lane = threadIdx.x & 63;
  uint32_t s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(s, d, 64);
    if (lane >= d) s += o;
  }
  total = __shfl(s, 63, 64);
  return s - v;
}

// The exact 5-NN of one query by a whole wavefront on the coarse level:
// Chebyshev rings R = 0, 1, ... of coarse cells around the query's (clamped)
// cell; a cell is scanned unless its tight box lies farther than the bound
// (the 5th distance found so far, or bound0: the 5th distance of 5 real map
// points, or +inf).  The candidate cells of a batch of 64 ring positions are
// expanded, four at a time, into their 16 runs of the fine pts (one per fine
// (y, z) row), flattened into one list (lane prefix sums in LDS, a 6-step
// binary search per candidate) and swept with U loads in flight per lane.  The search ends
// when every unscanned cell lies beyond the 5th distance: the bound over the
// six slabs outside the ring's cube is per-axis exact (face distance on the
// slab's axis, distance to the grid's range on the other two).  Keys carry
// the fine pts position, so results equal the fine grid's.  Returns the list
// in every lane.  KNN = 1 (the loop-closure ICP pass, k_icp_pass) bounds and
// ends the search by the nearest distance instead of the 5th: entry 0 is then
// the exact nearest key, the same one a KNN = 5 search puts there.
template <int U, int KNN = 5>
__device__ __forceinline__ void far_search(const MapView& map, float qx, float qy, float qz,
                                        float bound, uint32_t* __restrict__ pre,
                                        uint32_t* __restrict__ beg, Top5& t) {
  const int lane = threadIdx.x & 63;
  const CoarseView& cv = map.cl;
  const GridGeom g = cv.g, fg = map.g;
  const float INF = __int_as_float(0x7f800000);
  top5_clear(t);
  bool full = false;
  float d5 = INF;
  const int CX = min(max(cell_coord(qx, g.ox, g.inv_h), 0), g.dx - 1);
  const int CY = min(max(cell_coord(qy, g.oy, g.inv_h), 0), g.dy - 1);
  const int CZ = min(max(cell_coord(qz, g.oz, g.inv_h), 0), g.dz - 1);
  // distance of q to the grid's range on each axis (every map point lies in it)
  auto range_gap = [&](float q, float o, int d) {
    const float lo = o - g.tol, hi = o + (float)d * g.h + g.tol;
    return fmaxf(fmaxf(lo - q, q - hi), 0.0f);
  };
  const float ax = range_gap(qx, g.ox, g.dx), ay = range_gap(qy, g.oy, g.dy),
              az = range_gap(qz, g.oz, g.dz);
  // conservative squared gap from q to the cells [a0, a1] of one axis
  auto span_gap = [&](float q, float o, int a0, int a1) {
    const float lo = o + (float)a0 * g.h - g.tol, hi = o + (float)(a1 + 1) * g.h + g.tol;
    const float d = fmaxf(fmaxf(lo - q, q - hi), 0.0f);
    return d * d;
  };
  for (int R = 0;; ++R) {
    const int x0 = max(CX - R, 0), x1 = min(CX + R, g.dx - 1);
    const int y0 = max(CY - R, 0), y1 = min(CY + R, g.dy - 1);
    const int z0 = max(CZ - R, 0), z1 = min(CZ + R, g.dz - 1);
    // the ring's shell (cube R minus cube R-1, clipped to the grid) as up to
    // six face rectangles: x faces over the full (y, z) span, y faces over
    // the inner x span, z faces over the inner x and y spans.  A face whose
    // box lies beyond the bound is skipped whole (its cells would all fail
    // the per-cell test below).
    const int xi0 = max(CX - R + 1, 0), xi1 = min(CX + R - 1, g.dx - 1);
    const int yi0 = max(CY - R + 1, 0), yi1 = min(CY + R - 1, g.dy - 1);
    const float lim_f = fminf(bound, d5);
    int fa[6], fna[6], fb[6], fv[6], cum[7];
    cum[0] = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
      const int fax = f >> 1;                              // fixed axis
      const int C = fax == 0 ? CX : fax == 1 ? CY : CZ;
      const int D = fax == 0 ? g.dx : fax == 1 ? g.dy : g.dz;
      const int v = (f & 1) ? C + R : C - R;
      const bool ok = (f == 0 || R > 0) && v >= 0 && v < D;
      int a0, a1, b0, b1;
      float gsum;
      if (fax == 0) {
        a0 = y0; a1 = y1; b0 = z0; b1 = z1;
        gsum = (span_gap(qx, g.ox, v, v) + span_gap(qy, g.oy, a0, a1)) + span_gap(qz, g.oz, b0, b1);
      } else if (fax == 1) {
        a0 = xi0; a1 = xi1; b0 = z0; b1 = z1;
        gsum = (span_gap(qx, g.ox, a0, a1) + span_gap(qy, g.oy, v, v)) + span_gap(qz, g.oz, b0, b1);
      } else {
        a0 = xi0; a1 = xi1; b0 = yi0; b1 = yi1;
        gsum = (span_gap(qx, g.ox, a0, a1) + span_gap(qy, g.oy, b0, b1)) + span_gap(qz, g.oz, v, v);
      }
      const bool live_f = ok && a0 <= a1 && b0 <= b1 && !(gsum * 0.99999f > lim_f);
      fa[f] = a0;
      fb[f] = b0;
      fv[f] = v;
      fna[f] = live_f ? a1 - a0 + 1 : 0;
      cum[f + 1] = cum[f] + (live_f ? (a1 - a0 + 1) * (b1 - b0 + 1) : 0);
    }
    const int total = cum[6];
    for (int base = 0; base < total; base += 64) {
      const int p = base + lane;
      bool pass = false;
      int ccx = 0, ccy = 0, ccz = 0;
      if (p < total) {
        int f = 0;
#pragma unroll
        for (int j = 1; j < 6; ++j) f = p >= cum[j] ? j : f;
        int A = 0, B = 0, V = 0, NA = 1;
#pragma unroll
        for (int j = 0; j < 6; ++j)
          if (f == j) {
            A = fa[j];
            B = fb[j];
            V = fv[j];
            NA = fna[j];
          }
        const int l = p - (f == 0 ? 0 : f == 1 ? cum[1] : f == 2 ? cum[2] : f == 3 ? cum[3] : f == 4 ? cum[4] : cum[5]);
        const int ua = A + l % NA, ub = B + l / NA;
        const int fax = f >> 1;
        ccx = fax == 0 ? V : ua;
        ccy = fax == 0 ? ua : fax == 1 ? V : ub;
        ccz = fax == 2 ? V : ub;
        const uint32_t c = ((uint32_t)ccz * (uint32_t)g.dy + (uint32_t)ccy) * (uint32_t)g.dx + (uint32_t)ccx;
        const float4 lo = cv.lo[c];
        if (__float_as_uint(lo.w)) {
          const float4 hi = cv.hi[c];
          const float gx = fmaxf(fmaxf(lo.x - qx, qx - hi.x), 0.0f);
          const float gy = fmaxf(fmaxf(lo.y - qy, qy - hi.y), 0.0f);
          const float gz = fmaxf(fmaxf(lo.z - qz, qz - hi.z), 0.0f);
          const float gd = (gx * gx + gy * gy) + gz * gz;
          pass = !(gd > fminf(bound, d5));  // a point at exactly d5 may still win on position
        }
      }
      // the passing coarse cells, four at a time: lane l reads the bounds of
      // fine row (l & 15) of passing cell (l >> 4), one run of the fine pts
      uint64_t pm = __ballot(pass);
      const int gi = lane >> 4, sl = lane & 15;
      while (pm) {
        uint64_t bm = pm;
        for (int q = 0; q < gi && bm; ++q) bm &= bm - 1;  // the gi-th passing cell
        const bool act = bm != 0;
        const int src = act ? __ffsll((unsigned long long)bm) - 1 : 0;
        // (every lane shuffles: a cross-lane read inside a condition would
        // read lanes the condition turned off)
        const int x = __shfl(ccx, src, 64), y = __shfl(ccy, src, 64), z = __shfl(ccz, src, 64);
        for (int q = 0; q < 4 && pm; ++q) pm &= pm - 1;
        uint32_t s = 0, k = 0;
        const int fy = 4 * y + (sl & 3), fz = 4 * z + (sl >> 2);
        if (act && fy < fg.dy && fz < fg.dz) {
          const int64_t rb = ((int64_t)fz * fg.dy + fy) * fg.dx;
          s = map.start[rb + 4 * x];
          k = map.start[rb + min(4 * x + 4, fg.dx)] - s;
        }
        if (!__any(k != 0)) continue;
        uint32_t tot;
        const uint32_t ex = wave_excl_scan(k, tot);
        pre[lane] = ex;
        beg[lane] = s;
        wave_fence();
        for (uint32_t f0 = 0; f0 < tot; f0 += 64 * U) {
          uint32_t a[U];
          float4 c[U];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const uint32_t f = min(f0 + (uint32_t)(u * 64 + lane), tot - 1);
            int j = 0;
#pragma unroll
            for (int st = 32; st > 0; st >>= 1)
              if (pre[j + st] <= f) j += st;
            a[u] = beg[j] + (f - pre[j]);
          }
#pragma unroll
          for (int u = 0; u < U; ++u) c[u] = map.pts[a[u]];
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const float ddx = qx - c[u].x, ddy = qy - c[u].y, ddz = qz - c[u].z;
            const float d = (ddx * ddx + ddy * ddy) + ddz * ddz;  // calc_dist, ikd_Tree.cpp:1539-1544
            const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint64_t)a[u];
            top5_insert(t, (f0 + (uint32_t)(u * 64 + lane) < tot) ? key : kInfKey);
          }
        }
        group_merge<64>(t);  // every lane: the merged list
        full = t.k[KNN - 1] != kInfKey;
        if (full) d5 = __uint_as_float((uint32_t)(t.k[KNN - 1] >> 32));
        if (lane != 0) top5_clear(t);  // lane 0 keeps it
        wave_fence();                  // pre / beg are rewritten by the next batch
      }
    }
    // lower bound of the squared distance to every cell outside this cube
    float lb = INF;
    bool covers = true;
    auto slab = [&](bool open, float face_gap, float o1, float o2) {
      if (!open) return;
      covers = false;
      const float f = fmaxf(face_gap, 0.0f);
      lb = fminf(lb, (f * f + o1 * o1) + o2 * o2);
    };
    slab(x0 > 0, qx - (g.ox + (float)x0 * g.h + g.tol), ay, az);
    slab(x1 < g.dx - 1, (g.ox + (float)(x1 + 1) * g.h - g.tol) - qx, ay, az);
    slab(y0 > 0, qy - (g.oy + (float)y0 * g.h + g.tol), ax, az);
    slab(y1 < g.dy - 1, (g.oy + (float)(y1 + 1) * g.h - g.tol) - qy, ax, az);
    slab(z0 > 0, qz - (g.oz + (float)z0 * g.h + g.tol), ax, ay);
    slab(z1 < g.dz - 1, (g.oz + (float)(z1 + 1) * g.h - g.tol) - qz, ax, ay);
    if (covers || (full && d5 < lb * 0.99999f)) break;
    if (R > g.dx + g.dy + g.dz) break;  // unreachable: the cube covers the grid long before
  }
#pragma unroll
  for (int j = 0; j < 5; ++j) t.k[j] = __shfl(t.k[j], 0, 64);
}

}  // namespace slio
