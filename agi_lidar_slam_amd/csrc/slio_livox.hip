// slio_livox.hip -- livox_mapping's rolling cube map on the device
// (src/livox_mapping/src/laserMapping.cpp: laserCloudCornerArray /
// laserCloudSurfArray, 21 x 11 x 21 cubes of 50 m).
//
// Per class the map is ONE SoA of points sorted by cube index, inside a cube
// in the reference's order, with a 4852-entry offset table (device, and a host
// mirror refreshed by the one readback of every change).  Every change is one
// pass over the whole class:
//
//   append    k_lvx_append   the incoming points through pointAssociateToMap
//                            (:195-217) behind the stored ones, cube index in
//                            double (:1162-1168); out of range = dropped
//   shift     k_lvx_relabel  cube id -> shifted id, leaving cubes dropped
//   box       k_lvx_box      per valid cube, PCL's getMinMax3D
//   geometry  k_lvx_geom     per valid cube, VoxelGrid's inverse leaf, min_b,
//                            divb_mul, and the leaf-too-small pass-through
//   keys      k_lvx_keys     (cube id << 32) | voxel index; 0 in a cube that
//                            is not filtered
//   sort      hipcub radix   stable: `old ++ new` inside a cube, ascending
//                            input position inside a voxel
//   heads, ranks, centroids  one output point per voxel of a filtered cube,
//                            per point of any other cube
//   offsets   k_lvx_offsets  the new table; read back (19 KB) with the total
//
// Everything from "shift" to "offsets", the gather of listed cubes and the
// search grid are the cube store of slio_cube_store.hpp (slio::lvx::CubeStore,
// store_*), which A-LOAM's mapper (slio_aloam_map.hip) shares; slio_lvx derives
// from it.
//
// so the VoxelGrids of all valid cubes of a class (:1197-1216, up to 125) are
// one sequence of launches and one host wait.  Per cube the result is what
// slio_scan_upload_voxel gives for that cube's cloud alone: the geometry
// kernel is k_vg_geom's arithmetic (slio_device.hip) per cube.  A voxel index
// is below 2^31 by PCL's own overflow rule, so the 64-bit key cannot overflow
// for any leaf: a leaf too small for a cube passes that cube through, as PCL
// does.  A point that does not transform to finite coordinates is dropped at
// append (the reference's int() of it is undefined; x86-64 gives INT_MIN, out
// of range).
#include <hipcub/hipcub.hpp>

#include <cstring>
#include <vector>

#include "slio_cube_store.hpp"
#include "slio_device.hpp"
#include "slio_fkey.hpp"
#include "slio_frontend.h"
#include "slio_livox.hpp"
#include "slio_lreg.hpp"

using slio::fkey;
using slio::set_error;
using slio::MapDev;
using namespace slio::lvx;

namespace {

constexpr uint64_t kDropKey = ~0ull;
constexpr int kSortBits = 45;  // 32 voxel bits + 13 cube bits (kNum < 8191 = the dropped points' field)

__global__ void k_lvx_append(const float* __restrict__ in, int64_t n, slio::LegoRot T, int cenI, int cenJ, int cenK,
                             float* __restrict__ x, float* __restrict__ y, float* __restrict__ z,
                             uint32_t* __restrict__ id) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float ox, oy, oz;
  slio::lego_to_map(T, in[3 * i], in[3 * i + 1], in[3 * i + 2], ox, oy, oz);
  int ci, cj, ck;
  uint32_t c = kDrop;
  if (cube_of(ox, cenI, &ci) && cube_of(oy, cenJ, &cj) && cube_of(oz, cenK, &ck) && ci >= 0 && ci < kW && cj >= 0 &&
      cj < kH && ck >= 0 && ck < kD)
    c = (uint32_t)(ci + kW * cj + kW * kH * ck);
  x[i] = ox;
  y[i] = oy;
  z[i] = oz;
  id[i] = c;
}

// the six shift loops (:493-713) composed: every cube moves by (di, dj, dk);
// what leaves the array is dropped, what enters is empty
__global__ void k_lvx_relabel(uint32_t* __restrict__ id, int64_t n, int di, int dj, int dk, int kW, int kH, int kD) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = id[i];
  if (c == kDrop) return;
  const int ci = (int)(c % kW) + di, cj = (int)(c / kW % kH) + dj, ck = (int)(c / (kW * kH)) + dk;
  id[i] = (ci >= 0 && ci < kW && cj >= 0 && cj < kH && ck >= 0 && ck < kD) ? (uint32_t)(ci + kW * cj + kW * kH * ck)
                                                                            : kDrop;
}

__global__ void k_lvx_box_init(int32_t* __restrict__ bb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kNum * 8) return;
  const int f = i & 7;
  bb[i] = f < 3 ? INT32_MAX : f < 6 ? INT32_MIN : 0;
}

// bb[c] = {min keys, max keys, count, -} of the points of every cube to be
// filtered.  The stored points are sorted by cube, so a wavefront mostly holds
// one cube: it reduces by shuffles and issues one set of atomics; a mixed
// wavefront falls back to one set per lane.
__global__ void __launch_bounds__(256)
k_lvx_box(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
          const uint32_t* __restrict__ id, int64_t n, const uint8_t* __restrict__ filt, int32_t* __restrict__ bb) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = i < n ? id[i] : kDrop;
  if (c != kDrop && !filt[c]) c = kDrop;
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  if (c != kDrop) {
    lo[0] = hi[0] = fkey(x[i]);
    lo[1] = hi[1] = fkey(y[i]);
    lo[2] = hi[2] = fkey(z[i]);
  }
  const uint32_t c0 = __shfl(c, 0, 64);
  if (__all(c == c0)) {
    if (c0 == kDrop) return;  // (uniform)
#pragma unroll
    for (int a = 0; a < 3; ++a)
      for (int d = 32; d > 0; d >>= 1) {
        lo[a] = min(lo[a], __shfl_xor(lo[a], d, 64));
        hi[a] = max(hi[a], __shfl_xor(hi[a], d, 64));
      }
    if ((threadIdx.x & 63) == 0) {
      int32_t* b = bb + 8 * (int64_t)c0;
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(b + a, lo[a]);
        atomicMax(b + 3 + a, hi[a]);
      }
      atomicAdd(b + 6, 64);
    }
  } else if (c != kDrop) {
    int32_t* b = bb + 8 * (int64_t)c;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      atomicMin(b + a, lo[a]);
      atomicMax(b + 3 + a, hi[a]);
    }
    atomicAdd(b + 6, 1);
  }
}

// k_vg_geom (slio_device.hip) per cube: mode[c] = 1 where the cube's points go
// through the grid, 0 where they stay as they are (not a valid cube, no
// point, or PCL's "leaf size is too small": dx * dy * dz above INT32_MAX)
__global__ void k_lvx_geom(const int32_t* __restrict__ bb, const uint8_t* __restrict__ filt, float leaf,
                           CubeGeom* __restrict__ G, uint8_t* __restrict__ mode) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= kNum) return;
  const int32_t* b = bb + 8 * c;
  if (!filt[c] || b[6] == 0) {
    mode[c] = 0;
    return;
  }
  CubeGeom g;
  g.inv = 1.0f / leaf;
  float mn[3], mx[3];
  int64_t dd[3];
  for (int a = 0; a < 3; ++a) {
    const int32_t lo = b[a] >= 0 ? b[a] : b[a] ^ 0x7FFFFFFF, hi = b[3 + a] >= 0 ? b[3 + a] : b[3 + a] ^ 0x7FFFFFFF;
    mn[a] = __int_as_float(lo);
    mx[a] = __int_as_float(hi);
    const float span = (mx[a] - mn[a]) * g.inv;
    dd[a] = isfinite(span) && span < 9.2e18f ? (int64_t)span + 1 : INT64_MAX / 4;
  }
  bool pass = dd[0] > INT32_MAX || dd[1] > INT32_MAX || dd[2] > INT32_MAX;
  if (!pass) {
    const int64_t d01 = dd[0] * dd[1];
    pass = d01 > INT32_MAX || d01 * dd[2] > (int64_t)INT32_MAX;
  }
  if (pass) {
    mode[c] = 0;
    return;
  }
  int div[3];
  for (int a = 0; a < 3; ++a) {
    g.minb[a] = (int)floorf(mn[a] * g.inv);
    div[a] = (int)floorf(mx[a] * g.inv) - g.minb[a] + 1;
  }
  g.mul[0] = 1;
  g.mul[1] = div[0];
  g.mul[2] = div[0] * div[1];
  G[c] = g;
  mode[c] = 1;
}

__global__ void k_lvx_keys(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                           const uint32_t* __restrict__ id, int64_t n, const CubeGeom* __restrict__ G,
                           const uint8_t* __restrict__ mode, uint64_t* __restrict__ keys,
                           uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t c = id[i];
  uint64_t key = kDropKey;
  if (c != kDrop) {
    uint32_t v = 0;
    if (mode[c]) {
      const CubeGeom g = G[c];
      const int i0 = (int)(floorf(x[i] * g.inv) - (float)g.minb[0]);
      const int i1 = (int)(floorf(y[i] * g.inv) - (float)g.minb[1]);
      const int i2 = (int)(floorf(z[i] * g.inv) - (float)g.minb[2]);
      v = (uint32_t)(i0 * g.mul[0] + i1 * g.mul[1] + i2 * g.mul[2]);
    }
    key = ((uint64_t)c << 32) | v;
  }
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

__global__ void k_lvx_heads(const uint64_t* __restrict__ keys, int64_t n, const uint8_t* __restrict__ mode,
                            uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = keys[i];
  uint32_t h = 0;
  if (k != kDropKey) h = (!mode[k >> 32] || i == 0 || keys[i - 1] != k) ? 1u : 0u;
  head[i] = h;
}

// one thread per output point: the centroid of a voxel's run, summed in float
// in the sorted order and divided by the count (k_vg_centroids), or the point
// itself where its cube is not filtered
__global__ void k_lvx_centroids(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                                const uint64_t* __restrict__ keys, const uint32_t* __restrict__ order,
                                const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank, int64_t n,
                                const uint8_t* __restrict__ mode, float* __restrict__ ox, float* __restrict__ oy,
                                float* __restrict__ oz, uint32_t* __restrict__ oid) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 >= n || !head[i0]) return;
  const uint64_t k = keys[i0];
  const uint32_t c = (uint32_t)(k >> 32);
  const uint32_t r = rank[i0];
  oid[r] = c;
  if (!mode[c]) {
    const uint32_t o = order[i0];
    ox[r] = x[o];
    oy[r] = y[o];
    oz[r] = z[o];
    return;
  }
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  int64_t j = i0;
  for (; j < n && keys[j] == k; ++j) {
    const uint32_t o = order[j];
    sx = sx + x[o];
    sy = sy + y[o];
    sz = sz + z[o];
  }
  const float cnt = (float)(j - i0);
  ox[r] = sx / cnt;
  oy[r] = sy / cnt;
  oz[r] = sz / cnt;
}

// off[c] = output position of cube c's first point, c = 0 .. kNum (the total)
__global__ void k_lvx_offsets(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ head,
                              const uint32_t* __restrict__ rank, int64_t n, uint32_t* __restrict__ off) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c > kNum) return;
  const uint64_t want = (uint64_t)c << 32;
  int64_t lo = 0, hi = n;  // first position with keys >= want
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < want) lo = mid + 1;
    else hi = mid;
  }
  off[c] = lo < n ? rank[lo] : rank[n - 1] + head[n - 1];
}

// the concatenation of nseg cube ranges: seg[s] = {first stored position,
// first output position}, seg[nseg].y = total; out is n x {x, y, z}
__global__ void k_lvx_gather(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                             const uint2* __restrict__ seg, int nseg, int64_t total, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  int lo = 0, hi = nseg - 1;  // last segment whose output position is <= i
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((int64_t)seg[mid].y <= i) lo = mid;
    else hi = mid - 1;
  }
  const int64_t p = (int64_t)seg[lo].x + (i - (int64_t)seg[lo].y);
  out[3 * i] = x[p];
  out[3 * i + 1] = y[p];
  out[3 * i + 2] = z[p];
}

// ---- the search grid over a gathered map (GridView, slio_livox.hpp) ----------
__global__ void k_lvx_bbox3(const float* __restrict__ xyz, int64_t n, int32_t* __restrict__ bb) {
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int32_t k = fkey(xyz[3 * i + a]);
      lo[a] = min(lo[a], k);
      hi[a] = max(hi[a], k);
    }
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    for (int d = 32; d > 0; d >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], d, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], d, 64));
    }
    if ((threadIdx.x & 63) == 0) {
      atomicMin(bb + a, lo[a]);
      atomicMax(bb + 3 + a, hi[a]);
    }
  }
}

__device__ __forceinline__ int grid_cell(float v, float o, float inv_h) { return (int)floorf((v - o) * inv_h); }

__global__ void k_lvx_cellkeys(const float* __restrict__ xyz, int64_t n, GridView g, uint32_t* __restrict__ keys,
                               uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // (inside the grid by construction; clamped all the same, so that no key can
  // point past the start table)
  const int cx = min(max(grid_cell(xyz[3 * i], g.o[0], g.inv_h), 0), g.nx - 1);
  const int cy = min(max(grid_cell(xyz[3 * i + 1], g.o[1], g.inv_h), 0), g.ny - 1);
  const int cz = min(max(grid_cell(xyz[3 * i + 2], g.o[2], g.inv_h), 0), g.nz - 1);
  keys[i] = (uint32_t)(((int64_t)cz * g.ny + cy) * g.nx + cx);
  vals[i] = (uint32_t)i;
}

__global__ void k_lvx_grid_pts(const float* __restrict__ xyz, const uint32_t* __restrict__ order, int64_t n,
                               float4* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = order[i];
  pts[i] = make_float4(xyz[3 * o], xyz[3 * o + 1], xyz[3 * o + 2], __uint_as_float(o));
}

// start[c] = first sorted position whose cell is >= c, c = 0 .. ncells
__global__ void k_lvx_cellstart(const uint32_t* __restrict__ keys, int64_t n, int64_t ncells,
                                uint32_t* __restrict__ start) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c > ncells) return;
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)keys[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  start[c] = (uint32_t)lo;
}

// a host cloud (n x 3) into a class's SoA as ONE cube (id 0): the scan's own
// VoxelGrid is the per-cube grid of a one-cube map; non-finite points dropped
__global__ void k_lvx_scan_in(const float* __restrict__ in, int64_t n, float* __restrict__ x, float* __restrict__ y,
                              float* __restrict__ z, uint32_t* __restrict__ id) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float a = in[3 * i], b = in[3 * i + 1], c = in[3 * i + 2];
  x[i] = a;
  y[i] = b;
  z[i] = c;
  id[i] = (isfinite(a) && isfinite(b) && isfinite(c)) ? 0u : kDrop;
}

constexpr int64_t kMaxCells = (int64_t)1 << 24;

struct Scan {
  MapDev::Buf xyz, world, nbr_idx, nbr_sqd, coeff, sel, partial;
  int64_t n = 0;
  bool fed = false, passed = false;
};

}  // namespace

struct slio_lvx : slio::lvx::CubeStore {  // (the store's class 2 holds the surf scan for its VoxelGrid)
  slio_lvx_params prm{};
  bool dev_counted = false;
  Scan scan[2];
  float tobe[6] = {0}, aft[6] = {0}, last[6] = {0};  // transformTobeMapped / AftMapped / LastMapped
  // isDegenerate and matP are globals of the node: a call whose first turn has
  // fewer than 50 rows goes on with what the previous call left (:1105, :1128)
  int is_degenerate = 0;
  float matP[36] = {0};
  int32_t cen[3] = {10, 5, 10};  // laserCloudCenWidth / Height / Depth (:64-66)
  int32_t valid[125], surround[125];
  int32_t nvalid = 0, nsurround = 0;
  bool selected = false;
};

void slio::lvx::store_free(CubeStore* m) {
  for (StoreClass& c : m->cls)
    for (int b = 0; b < 2; ++b) {
      for (int a = 0; a < 3; ++a)
        if (c.xyz[b][a]) (void)hipFree(c.xyz[b][a]);
      if (c.id[b]) (void)hipFree(c.id[b]);
    }
  for (void* p : {(void*)m->k0, (void*)m->k1, (void*)m->v0, (void*)m->v1, (void*)m->head, (void*)m->rank,
                  (void*)m->off, (void*)m->bb, (void*)m->geom, (void*)m->filt, (void*)m->mode, (void*)m->seg})
    if (p) (void)hipFree(p);
  for (MapDev::Buf* b : {&m->tmp_sort, &m->tmp_scan, &m->in, &m->out})
    if (b->p) (void)hipFree(b->p);
  for (StoreGrid& g : m->grid)
    for (MapDev::Buf* b : {&g.xyz, &g.pts, &g.start})
      if (b->p) (void)hipFree(b->p);
  if (m->h_off) (void)hipHostFree(m->h_off);
  if (m->h_filt) (void)hipHostFree(m->h_filt);
  if (m->h_seg) (void)hipHostFree(m->h_seg);
  if (m->stream) (void)hipStreamDestroy(m->stream);
}

static void lvx_free(slio_lvx* m) {
  for (Scan& s : m->scan)
    for (MapDev::Buf* b : {&s.xyz, &s.world, &s.nbr_idx, &s.nbr_sqd, &s.coeff, &s.sel, &s.partial})
      if (b->p) (void)hipFree(b->p);
  slio::lvx::store_free(m);
}

int slio::lvx::store_rebuild(CubeStore* m, int k, int64_t N, bool with_filter, float leaf, const char* who) {
  StoreClass& c = m->cls[k];
  hipStream_t st = m->stream;
  if (N == 0) {
    c.n = 0;
    std::fill(c.off.begin(), c.off.end(), 0u);
    return SLIO_OK;
  }
  float** s = c.xyz[c.cur];
  float** d = c.xyz[c.cur ^ 1];
  uint32_t* sid = c.id[c.cur];
  hipError_t e;
  if (with_filter) {
    k_lvx_box_init<<<blocks(kNum * 8), 256, 0, st>>>(m->bb);
    k_lvx_box<<<blocks(N), 256, 0, st>>>(s[0], s[1], s[2], sid, N, m->filt, m->bb);
    k_lvx_geom<<<blocks(kNum), 256, 0, st>>>(m->bb, m->filt, leaf, m->geom, m->mode);
  } else {
    SLIO_HIP(hipMemsetAsync(m->mode, 0, kNum, st));
  }
  k_lvx_keys<<<blocks(N), 256, 0, st>>>(s[0], s[1], s[2], sid, N, m->geom, m->mode, m->k0, m->v0);
  size_t tb = 0;
  if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, m->k0, m->k1, m->v0, m->v1, (int)N, 0, kSortBits, st)) ||
      (e = MapDev::take(m->tmp_sort, tb)) ||
      (e = hipcub::DeviceRadixSort::SortPairs(m->tmp_sort.p, tb, m->k0, m->k1, m->v0, m->v1, (int)N, 0, kSortBits,
                                              st))) {
    set_error(std::string(who) + ": sort: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  k_lvx_heads<<<blocks(N), 256, 0, st>>>(m->k1, N, m->mode, m->head);
  tb = 0;
  if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, tb, m->head, m->rank, (int)N, st)) ||
      (e = MapDev::take(m->tmp_scan, tb)) ||
      (e = hipcub::DeviceScan::ExclusiveSum(m->tmp_scan.p, tb, m->head, m->rank, (int)N, st))) {
    set_error(std::string(who) + ": scan: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  k_lvx_centroids<<<blocks(N), 256, 0, st>>>(s[0], s[1], s[2], m->k1, m->v1, m->head, m->rank, N, m->mode, d[0], d[1],
                                             d[2], c.id[c.cur ^ 1]);
  k_lvx_offsets<<<blocks(kNum + 1), 256, 0, st>>>(m->k1, m->head, m->rank, N, m->off);
  SLIO_HIP(hipGetLastError());
  SLIO_HIP(hipMemcpyAsync(m->h_off, m->off, 4 * (kNum + 1), hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));
  std::memcpy(c.off.data(), m->h_off, 4 * (kNum + 1));
  c.n = c.off[kNum];
  c.cur ^= 1;
  return SLIO_OK;
}

int slio::lvx::store_upload_filter(CubeStore* m, const int32_t* list, int32_t n) {
  std::memset(m->h_filt, 0, kNum);
  for (int i = 0; i < n; ++i) m->h_filt[list[i]] = 1;
  SLIO_HIP(hipMemcpyAsync(m->filt, m->h_filt, kNum, hipMemcpyHostToDevice, m->stream));
  return SLIO_OK;
}

bool slio::lvx::store_list_ok(const int32_t* list, int32_t n) {
  if (n < 0 || (n > 0 && !list)) return false;
  for (int i = 0; i < n; ++i)
    if (list[i] < 0 || list[i] >= kNum) return false;
  return true;
}

int slio::lvx::store_gather(CubeStore* m, int k, const int32_t* list, int32_t n, int64_t* total,
                            MapDev::Buf* dst) {
  if (!dst) dst = &m->out;
  const StoreClass& c = m->cls[k];
  int nseg = 0;
  uint32_t pos = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t len = c.off[list[i] + 1] - c.off[list[i]];
    if (!len) continue;
    m->h_seg[nseg++] = make_uint2(c.off[list[i]], pos);
    pos += len;
  }
  *total = pos;
  if (!pos) return SLIO_OK;
  if (hipError_t e = MapDev::take(*dst, 12 * (size_t)pos)) {
    set_error(std::string("slio_lvx: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  SLIO_HIP(hipMemcpyAsync(m->seg, m->h_seg, sizeof(uint2) * nseg, hipMemcpyHostToDevice, m->stream));
  float* const* s = c.xyz[c.cur];
  k_lvx_gather<<<blocks(pos), 256, 0, m->stream>>>(s[0], s[1], s[2], m->seg, nseg, pos, (float*)dst->p);
  SLIO_HIP(hipGetLastError());
  return SLIO_OK;
}

int slio::lvx::store_download(CubeStore* m, int k, const int32_t* list, int32_t n, float* xyz, int64_t cap,
                              int64_t* npts, const char* who) {
  int64_t total = 0;
  for (int i = 0; i < n; ++i) total += m->cls[k].off[list[i] + 1] - m->cls[k].off[list[i]];
  if (npts) *npts = total;
  if (!xyz) return SLIO_OK;
  if (total > cap) {
    set_error(std::string(who) + ": the output holds fewer points than the cubes");
    return SLIO_ECAPACITY;
  }
  int rc = store_gather(m, k, list, n, &total);
  if (rc || !total) return rc;
  SLIO_HIP(hipMemcpyAsync(xyz, m->out.p, 12 * (size_t)total, hipMemcpyDeviceToHost, m->stream));
  SLIO_HIP(hipStreamSynchronize(m->stream));
  return SLIO_OK;
}

int slio::lvx::store_shift(CubeStore* m, const int32_t shift[3], const char* who) {
  for (int k = 0; k < 2; ++k) {
    StoreClass& c = m->cls[k];
    if (!c.n) continue;
    k_lvx_relabel<<<blocks(c.n), 256, 0, m->stream>>>(c.id[c.cur], c.n, shift[0], shift[1], shift[2], m->W, m->H, m->D);
    const int rc = store_rebuild(m, k, c.n, false, 0.0f, who);
    if (rc) return rc;
  }
  return SLIO_OK;
}

hipError_t slio::lvx::store_alloc(CubeStore* m, size_t cap) {
  hipError_t e = hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking);
  for (StoreClass& c : m->cls)
    for (int b = 0; b < 2 && !e; ++b) {
      for (int a = 0; a < 3 && !e; ++a) e = hipMalloc(&c.xyz[b][a], 4 * cap);
      if (!e) e = hipMalloc(&c.id[b], 4 * cap);
    }
  if (!e) e = hipMalloc(&m->k0, 8 * cap);
  if (!e) e = hipMalloc(&m->k1, 8 * cap);
  if (!e) e = hipMalloc(&m->v0, 4 * cap);
  if (!e) e = hipMalloc(&m->v1, 4 * cap);
  if (!e) e = hipMalloc(&m->head, 4 * cap);
  if (!e) e = hipMalloc(&m->rank, 4 * cap);
  if (!e) e = hipMalloc(&m->off, 4 * (kNum + 1));
  if (!e) e = hipMalloc(&m->bb, 4 * 8 * kNum);
  if (!e) e = hipMalloc(&m->geom, sizeof(CubeGeom) * kNum);
  if (!e) e = hipMalloc(&m->filt, kNum);
  if (!e) e = hipMalloc(&m->mode, kNum);
  if (!e) e = hipMalloc(&m->seg, sizeof(uint2) * (kMaxListed + 1));
  if (!e) e = hipHostMalloc(&m->h_off, 4 * (kNum + 1), hipHostMallocDefault);
  if (!e) e = hipHostMalloc(&m->h_filt, kNum, hipHostMallocDefault);
  if (!e) e = hipHostMalloc(&m->h_seg, sizeof(uint2) * (kMaxListed + 1), hipHostMallocDefault);
  return e;
}

void slio::lvx::store_clear(CubeStore* m) {
  for (StoreClass& c : m->cls) {
    c.n = 0;
    std::fill(c.off.begin(), c.off.end(), 0u);
  }
  for (StoreGrid& g : m->grid) g.built = false;
}

#define LVX_CHECK(m, who)                                \
  do {                                                   \
    if (!(m)) {                                          \
      set_error(who ": null handle");                    \
      return SLIO_EINVAL;                                \
    }                                                    \
  } while (0)

extern "C" {

int slio_lvx_params_default(slio_lvx_params* p) {
  if (!p) {
    set_error("slio_lvx_params_default: null");
    return SLIO_EINVAL;
  }
  std::memset(p, 0, sizeof(*p));
  p->device = 0;
  p->max_points = 1 << 21;
  p->leaf_corner = 0.2f;  // filter_parameter_corner (horizon / outdoor launch files)
  p->leaf_surf = 0.4f;    // filter_parameter_surf
  return SLIO_OK;
}

int slio_lvx_create(slio_lvx_handle* out, const slio_lvx_params* p) {
  if (!out || !p || p->max_points < 1 || !(p->leaf_corner > 0.0f) || !(p->leaf_surf > 0.0f) ||
      !std::isfinite(p->leaf_corner) || !std::isfinite(p->leaf_surf) || p->device < 0) {
    set_error("slio_lvx_create: bad arguments (max_points >= 1, finite leaves > 0, device >= 0)");
    return SLIO_EINVAL;
  }
  int ndev = 0;
  SLIO_HIP(hipGetDeviceCount(&ndev));
  if (p->device >= ndev) {
    set_error("slio_lvx_create: no such device");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(p->device));
  slio_lvx* m = new slio_lvx();
  m->prm = *p;
  const hipError_t e = store_alloc(m, (size_t)p->max_points);
  if (e) {
    set_error(std::string("slio_lvx_create: ") + hipGetErrorString(e));
    lvx_free(m);
    delete m;
    return SLIO_ENOMEM;
  }
  m->dev_counted = true;
  slio::dev_users(p->device, +1);
  *out = m;
  return SLIO_OK;
}

int slio_lvx_destroy(slio_lvx_handle m) {
  if (!m) return SLIO_OK;
  (void)hipSetDevice(m->prm.device);
  if (m->stream) (void)hipStreamSynchronize(m->stream);
  lvx_free(m);
  if (m->dev_counted) slio::dev_users(m->prm.device, -1);
  delete m;
  return SLIO_OK;
}

int slio_lvx_clear(slio_lvx_handle m) {
  LVX_CHECK(m, "slio_lvx_clear");
  store_clear(m);
  m->cen[0] = 10;
  m->cen[1] = 5;
  m->cen[2] = 10;
  m->nvalid = m->nsurround = 0;
  m->selected = false;
  for (int k = 0; k < 2; ++k) {
    m->scan[k].fed = m->scan[k].passed = false;
    m->scan[k].n = 0;
  }
  for (int a = 0; a < 6; ++a) m->tobe[a] = m->aft[a] = m->last[a] = 0.0f;
  m->is_degenerate = 0;
  std::memset(m->matP, 0, sizeof m->matP);
  return SLIO_OK;
}

int slio_lvx_select_cubes(slio_lvx_handle m, const float transform[6], int32_t center[3], int32_t* valid,
                          int32_t* nvalid, int32_t* surround, int32_t* nsurround) {
  LVX_CHECK(m, "slio_lvx_select_cubes");
  if (!transform) {
    set_error("slio_lvx_select_cubes: null transform");
    return SLIO_EINVAL;
  }
  for (int a = 0; a < 6; ++a)
    if (!std::isfinite(transform[a])) {
      set_error("slio_lvx_select_cubes: transform is not finite");
      return SLIO_EINVAL;
    }
  int32_t cen[3] = {m->cen[0], m->cen[1], m->cen[2]}, ctr[3], shift[3], v[125], s[125], nv = 0, ns = 0;
  if (select_host(transform, cen, ctr, shift, v, &nv, s, &ns)) {
    set_error("slio_lvx_select_cubes: position beyond 1e6 m");
    return SLIO_EINVAL;
  }
  if (shift[0] || shift[1] || shift[2]) {
    SLIO_HIP(hipSetDevice(m->prm.device));
    if (const int rc = store_shift(m, shift, "slio_lvx_select_cubes")) return rc;
  }
  m->grid[0].built = m->grid[1].built = false;  // (a new valid list: the maps are to be gathered again)
  std::memcpy(m->cen, cen, sizeof cen);
  std::memcpy(m->valid, v, sizeof v);
  std::memcpy(m->surround, s, sizeof s);
  m->nvalid = nv;
  m->nsurround = ns;
  m->selected = true;
  if (center) std::memcpy(center, ctr, sizeof ctr);
  if (valid) std::memcpy(valid, v, 4 * nv);
  if (nvalid) *nvalid = nv;
  if (surround) std::memcpy(surround, s, 4 * ns);
  if (nsurround) *nsurround = ns;
  return SLIO_OK;
}

}  // extern "C"

// slio_lvx_update_map; on_device: the two clouds are device buffers (the fed
// scans of slio_lvx_process), nothing crosses PCIe
static int update_impl(slio_lvx_handle m, const float transform[6], const float* corner_xyz, int64_t n_corner,
                       const float* surf_xyz, int64_t n_surf, const int32_t* valid, int32_t nvalid,
                       int64_t counts[2], bool on_device) {
  if (!transform || n_corner < 0 || n_surf < 0 || (n_corner && !corner_xyz) || (n_surf && !surf_xyz)) {
    set_error("slio_lvx_update_map: bad arguments");
    return SLIO_EINVAL;
  }
  for (int a = 0; a < 6; ++a)
    if (!std::isfinite(transform[a])) {
      set_error("slio_lvx_update_map: transform is not finite");
      return SLIO_EINVAL;
    }
  if (!valid) {
    if (nvalid != 0) {
      set_error("slio_lvx_update_map: nvalid without a list");
      return SLIO_EINVAL;
    }
    if (!m->selected) {
      set_error("slio_lvx_update_map: no cube list given and no slio_lvx_select_cubes before");
      return SLIO_ESTATE;
    }
    valid = m->valid;
    nvalid = m->nvalid;
  } else if (!store_list_ok(valid, nvalid)) {
    set_error("slio_lvx_update_map: cube index out of range");
    return SLIO_EINVAL;
  }
  const int64_t nn[2] = {n_corner, n_surf};
  for (int k = 0; k < 2; ++k)
    if (m->cls[k].n + nn[k] > m->prm.max_points) {
      set_error("slio_lvx_update_map: map and scan exceed max_points");
      return SLIO_ECAPACITY;
    }
  if (m->cls[0].n + nn[0] + m->cls[1].n + nn[1] == 0) {
    if (counts) counts[0] = counts[1] = 0;
    return SLIO_OK;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  int rc = store_upload_filter(m, valid, nvalid);
  if (rc) return rc;
  slio::LegoRot T;
  T.cr = slio::fcos(transform[0]);
  T.sr = slio::fsin(transform[0]);
  T.cp = slio::fcos(transform[1]);
  T.sp = slio::fsin(transform[1]);
  T.cy = slio::fcos(transform[2]);
  T.sy = slio::fsin(transform[2]);
  T.tx = transform[3];
  T.ty = transform[4];
  T.tz = transform[5];
  const float* src[2] = {corner_xyz, surf_xyz};
  const float leaf[2] = {m->prm.leaf_corner, m->prm.leaf_surf};
  for (int k = 0; k < 2; ++k) {
    StoreClass& c = m->cls[k];
    if (nn[k]) {
      const float* d_src = src[k];
      if (!on_device) {
        if (hipError_t e = MapDev::take(m->in, 12 * (size_t)nn[k])) {
          set_error(std::string("slio_lvx_update_map: hipMalloc: ") + hipGetErrorString(e));
          return SLIO_ENOMEM;
        }
        // (pageable source: the copy has read it when the call returns)
        SLIO_HIP(hipMemcpyAsync(m->in.p, src[k], 12 * (size_t)nn[k], hipMemcpyHostToDevice, m->stream));
        d_src = (const float*)m->in.p;
      }
      float** s = c.xyz[c.cur];
      k_lvx_append<<<blocks(nn[k]), 256, 0, m->stream>>>(d_src, nn[k], T, m->cen[0], m->cen[1],
                                                         m->cen[2], s[0] + c.n, s[1] + c.n, s[2] + c.n,
                                                         c.id[c.cur] + c.n);
    }
    if ((rc = store_rebuild(m, k, c.n + nn[k], true, leaf[k], "slio_lvx_update_map"))) return rc;
    if (counts) counts[k] = c.n;
    m->grid[k].built = false;  // the map the grid was built on has changed
  }
  return SLIO_OK;
}

extern "C" {

int slio_lvx_update_map(slio_lvx_handle m, const float transform[6], const float* corner_xyz, int64_t n_corner,
                        const float* surf_xyz, int64_t n_surf, const int32_t* valid, int32_t nvalid,
                        int64_t counts[2]) {
  LVX_CHECK(m, "slio_lvx_update_map");
  return update_impl(m, transform, corner_xyz, n_corner, surf_xyz, n_surf, valid, nvalid, counts, false);
}

int slio_lvx_cube_sizes(slio_lvx_handle m, int kind, int32_t* sizes) {
  LVX_CHECK(m, "slio_lvx_cube_sizes");
  if ((kind != 0 && kind != 1) || !sizes) {
    set_error("slio_lvx_cube_sizes: kind outside {0, 1} or null output");
    return SLIO_EINVAL;
  }
  const StoreClass& c = m->cls[kind];
  for (int i = 0; i < kNum; ++i) sizes[i] = (int32_t)(c.off[i + 1] - c.off[i]);
  return SLIO_OK;
}

int slio_lvx_get_cube(slio_lvx_handle m, int kind, int32_t cube, float* xyz, int64_t cap, int64_t* n) {
  LVX_CHECK(m, "slio_lvx_get_cube");
  if ((kind != 0 && kind != 1) || cube < 0 || cube >= kNum || cap < 0) {
    set_error("slio_lvx_get_cube: kind outside {0, 1}, cube outside the array or negative capacity");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  return store_download(m, kind, &cube, 1, xyz, cap, n, "slio_lvx_get_cube");
}

int slio_lvx_get_surround(slio_lvx_handle m, int kind, const int32_t* cubes, int32_t ncubes, float* xyz, int64_t cap,
                          int64_t* n) {
  LVX_CHECK(m, "slio_lvx_get_surround");
  if ((kind != 0 && kind != 1) || cap < 0 || (cubes && (ncubes > 125 || !store_list_ok(cubes, ncubes))) ||
      (!cubes && ncubes != 0)) {
    set_error("slio_lvx_get_surround: kind outside {0, 1}, a cube outside the array, more than 125 cubes or "
              "negative capacity");
    return SLIO_EINVAL;
  }
  if (!cubes) {
    if (!m->selected) {
      set_error("slio_lvx_get_surround: no cube list given and no slio_lvx_select_cubes before");
      return SLIO_ESTATE;
    }
    cubes = m->surround;
    ncubes = m->nsurround;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  return store_download(m, kind, cubes, ncubes, xyz, cap, n, "slio_lvx_get_surround");
}

int slio_lvx_get_centers(slio_lvx_handle m, int32_t cen[3]) {
  LVX_CHECK(m, "slio_lvx_get_centers");
  if (!cen) {
    set_error("slio_lvx_get_centers: null output");
    return SLIO_EINVAL;
  }
  std::memcpy(cen, m->cen, sizeof m->cen);
  return SLIO_OK;
}

}  // extern "C"

namespace {

int take_scan_outputs(slio_lvx* m, int k, int64_t n) {
  Scan& sc = m->scan[k];
  const int K = k == 0 ? 5 : 8;
  const size_t nb = (size_t)((n + 255) / 256);
  hipError_t e;
  if ((e = MapDev::take(sc.world, 12 * (size_t)n)) || (e = MapDev::take(sc.nbr_idx, 4 * (size_t)n * K)) ||
      (e = MapDev::take(sc.nbr_sqd, 4 * (size_t)n * K)) || (e = MapDev::take(sc.coeff, 16 * (size_t)n)) ||
      (e = MapDev::take(sc.sel, (size_t)n)) || (e = MapDev::take(sc.partial, 8 * 28 * nb))) {
    set_error(std::string("slio_lvx: hipMalloc: ") + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  return SLIO_OK;
}

}  // namespace

int slio::lvx::store_build_grid(CubeStore* m, int k, const int32_t* valid, int32_t nvalid, float h, const char* who) {
  StoreGrid& g = m->grid[k];
  hipStream_t st = m->stream;
  int64_t total = 0;
  int rc = store_gather(m, k, valid, nvalid, &total, &g.xyz);
  if (rc) return rc;
  g.n = total;
  g.view = GridView{};
  g.built = true;
  if (!total) return SLIO_OK;
  const int32_t init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
  std::memcpy(m->h_off, init, sizeof init);
  SLIO_HIP(hipMemcpyAsync(m->bb, m->h_off, sizeof init, hipMemcpyHostToDevice, st));
  k_lvx_bbox3<<<std::min(blocks(total), 256), 256, 0, st>>>((const float*)g.xyz.p, total, m->bb);
  SLIO_HIP(hipMemcpyAsync(m->h_off, m->bb, sizeof init, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));
  GridView v{};
  v.h = h;
  v.inv_h = 1.0f / v.h;
  int dim[3];
  for (int a = 0; a < 3; ++a) {
    int32_t lo = (int32_t)m->h_off[a], hi = (int32_t)m->h_off[3 + a];
    lo = lo >= 0 ? lo : lo ^ 0x7FFFFFFF;
    hi = hi >= 0 ? hi : hi ^ 0x7FFFFFFF;
    float flo, fhi;
    std::memcpy(&flo, &lo, 4);
    std::memcpy(&fhi, &hi, 4);
    v.o[a] = flo - 2.0f * v.h;
    // the cell function of the kernels, on the host: same float operations
    const double top = std::floor((double)((fhi - v.o[a]) * v.inv_h));
    if (!(top >= 0.0 && top < 1.0e6)) {
      set_error(std::string(who) + ": map extent out of range");
      return SLIO_ECAPACITY;
    }
    dim[a] = (int)top + 3;
  }
  v.nx = dim[0];
  v.ny = dim[1];
  v.nz = dim[2];
  const int64_t ncells = (int64_t)dim[0] * dim[1] * dim[2];
  if (ncells > kMaxCells) {
    set_error(std::string(who) + ": the valid cubes span more than 2^24 search cells");
    return SLIO_ECAPACITY;
  }
  hipError_t e;
  if ((e = MapDev::take(g.pts, 16 * (size_t)total)) || (e = MapDev::take(g.start, 4 * (size_t)(ncells + 1)))) {
    set_error(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  v.n = total;
  k_lvx_cellkeys<<<blocks(total), 256, 0, st>>>((const float*)g.xyz.p, total, v, m->v0, m->head);
  int bits = 1;
  while (((int64_t)1 << bits) < ncells) ++bits;
  size_t tb = 0;
  if ((e = hipcub::DeviceRadixSort::SortPairs(nullptr, tb, m->v0, m->v1, m->head, m->rank, (int)total, 0, bits, st)) ||
      (e = MapDev::take(m->tmp_sort, tb)) ||
      (e = hipcub::DeviceRadixSort::SortPairs(m->tmp_sort.p, tb, m->v0, m->v1, m->head, m->rank, (int)total, 0, bits,
                                              st))) {
    set_error(std::string(who) + ": sort: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  k_lvx_grid_pts<<<blocks(total), 256, 0, st>>>((const float*)g.xyz.p, m->rank, total, (float4*)g.pts.p);
  k_lvx_cellstart<<<blocks(ncells + 1), 256, 0, st>>>(m->v1, total, ncells, (uint32_t*)g.start.p);
  SLIO_HIP(hipGetLastError());
  v.pts = (const float4*)g.pts.p;
  v.start = (const uint32_t*)g.start.p;
  g.view = v;
  return SLIO_OK;
}

namespace {

int run_pass(slio_lvx* m, int k, const float tf[6]) {
  Scan& sc = m->scan[k];
  if (!sc.n) {
    sc.passed = true;
    return SLIO_OK;
  }
  const PassOut o{(float*)sc.world.p, (int32_t*)sc.nbr_idx.p, (float*)sc.nbr_sqd.p,
                  (float4*)sc.coeff.p, (uint8_t*)sc.sel.p,    (double*)sc.partial.p};
  const int rc = pass_launch(k, m->grid[k].view, (const float*)sc.xyz.p, sc.n, tf, o, m->stream);
  if (!rc) sc.passed = true;
  return rc;
}

// the partials of both classes, corners first, in workgroup order: ONE wait
int sum_partials(slio_lvx* m, float AtA[36], float AtB[6], int64_t* nsel) {
  double acc[28] = {0};
  std::vector<double> part[2];
  for (int k = 0; k < 2; ++k) {
    if (!m->scan[k].n) continue;
    part[k].resize((size_t)((m->scan[k].n + 255) / 256) * 28);
    SLIO_HIP(hipMemcpyAsync(part[k].data(), m->scan[k].partial.p, 8 * part[k].size(), hipMemcpyDeviceToHost,
                            m->stream));
  }
  SLIO_HIP(hipStreamSynchronize(m->stream));
  for (int k = 0; k < 2; ++k)
    for (size_t b = 0; b < part[k].size() / 28; ++b)
      for (int q = 0; q < 28; ++q) acc[q] = acc[q] + part[k][b * 28 + q];
  int q = 0;
  for (int r = 0; r < 6; ++r)
    for (int c = r; c < 6; ++c, ++q) AtA[6 * r + c] = AtA[6 * c + r] = (float)acc[q];
  for (int r = 0; r < 6; ++r) AtB[r] = (float)acc[21 + r];
  if (nsel) *nsel = (int64_t)llround(acc[27]);
  return SLIO_OK;
}

// n x {x, y, z, intensity} on the device -> n x {x, y, z}
__global__ void k_lvx_take_xyz(const float* __restrict__ in, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[3 * i] = in[4 * i];
  out[3 * i + 1] = in[4 * i + 1];
  out[3 * i + 2] = in[4 * i + 2];
}

}  // namespace

void slio::lvx::store_take_xyz(const float* d_xyzi, int64_t n, float* d_xyz, hipStream_t st) {
  if (n) k_lvx_take_xyz<<<blocks(n), 256, 0, st>>>(d_xyzi, n, d_xyz);
}

int slio::lvx::store_scan_voxel(CubeStore* m, const float* d_xyz, int64_t n, float leaf, MapDev::Buf* dst,
                                int64_t* n_out, const char* who) {
  StoreClass& tmp = m->cls[2];
  tmp.cur = 0;
  tmp.n = 0;
  k_lvx_scan_in<<<blocks(n), 256, 0, m->stream>>>(d_xyz, n, tmp.xyz[0][0], tmp.xyz[0][1], tmp.xyz[0][2], tmp.id[0]);
  const int32_t cube0 = 0;
  int rc = store_upload_filter(m, &cube0, 1);
  if (!rc) rc = store_rebuild(m, 2, n, true, leaf, who);
  if (rc) return rc;
  return store_gather(m, 2, &cube0, 1, n_out, dst);
}

namespace {

// A feed is feed_begin, then the caller's copies on the stream -- the corner
// cloud into scan[0].xyz, the surf cloud into m->in, both n x 3, from the host
// (slio_lvx_feed_host) or from the registration's clouds (slio_lvx_feed_device)
// -- then feed_finish, the part both share.
int feed_begin(slio_lvx* m, int64_t n_corner, int64_t n_surf, const char* who) {
  if (n_corner > m->prm.max_points || n_surf > m->prm.max_points) {
    set_error(std::string(who) + ": scan exceeds max_points");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  for (int k = 0; k < 2; ++k) m->scan[k].fed = m->scan[k].passed = false;
  hipError_t e = hipSuccess;
  if (n_corner) e = MapDev::take(m->scan[0].xyz, 12 * (size_t)n_corner);
  if (!e && n_surf) e = MapDev::take(m->in, 12 * (size_t)n_surf);
  if (e) {
    set_error(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  return SLIO_OK;
}

int feed_finish(slio_lvx* m, int64_t n_corner, int64_t n_surf, int64_t counts[2], const char* who) {
  hipStream_t st = m->stream;
  // corner: the raw laserCloudCornerLast (:825 runs over it, not over _down)
  Scan& c0 = m->scan[0];
  c0.n = n_corner;
  // surf: downSizeFilterSurf (:795-798) = the per-cube VoxelGrid of a one-cube map
  Scan& s1 = m->scan[1];
  if (n_surf) {
    int64_t total = 0;
    if (int rc = store_scan_voxel(m, (const float*)m->in.p, n_surf, m->prm.leaf_surf, &s1.xyz, &total, who)) return rc;
    s1.n = total;
  } else {
    s1.n = 0;
  }
  for (int k = 0; k < 2; ++k) {
    if (m->scan[k].n)
      if (int rc = take_scan_outputs(m, k, m->scan[k].n)) return rc;
    m->scan[k].fed = true;
  }
  SLIO_HIP(hipStreamSynchronize(st));  // the source clouds have been read
  if (counts) {
    counts[0] = c0.n;
    counts[1] = s1.n;
  }
  return SLIO_OK;
}

bool finite6(const float* t) {
  for (int a = 0; a < 6; ++a)
    if (!std::isfinite(t[a])) return false;
  return true;
}

}  // namespace

extern "C" {

int slio_lvx_feed_host(slio_lvx_handle m, const float* corner_xyz, int64_t n_corner, const float* surf_xyz,
                       int64_t n_surf, int64_t counts[2]) {
  LVX_CHECK(m, "slio_lvx_feed_host");
  if (n_corner < 0 || n_surf < 0 || (n_corner && !corner_xyz) || (n_surf && !surf_xyz)) {
    set_error("slio_lvx_feed_host: bad arguments");
    return SLIO_EINVAL;
  }
  if (int rc = feed_begin(m, n_corner, n_surf, "slio_lvx_feed_host")) return rc;
  // the upload part: the two host clouds into the buffers the device part reads
  if (n_corner)
    SLIO_HIP(hipMemcpyAsync(m->scan[0].xyz.p, corner_xyz, 12 * (size_t)n_corner, hipMemcpyHostToDevice, m->stream));
  if (n_surf) SLIO_HIP(hipMemcpyAsync(m->in.p, surf_xyz, 12 * (size_t)n_surf, hipMemcpyHostToDevice, m->stream));
  return feed_finish(m, n_corner, n_surf, counts, "slio_lvx_feed_host");
}

int slio_lvx_feed_device(slio_lvx_handle m, void* reg, int64_t counts[2]) {
  LVX_CHECK(m, "slio_lvx_feed_device");
  slio::lreg::View v{};
  if (int rc = slio::lreg::view(reg, &v, "slio_lvx_feed_device")) return rc;
  if (v.device != m->prm.device) {
    set_error("slio_lvx_feed_device: the registration and the mapper are on different devices");
    return SLIO_EINVAL;
  }
  const int64_t n_corner = v.n_corner, n_surf = v.n_surf;
  if (int rc = feed_begin(m, n_corner, n_surf, "slio_lvx_feed_device")) return rc;
  // (slio_lreg_run ended with a wait: the registration's clouds are complete)
  store_take_xyz(v.corner_xyzi, n_corner, (float*)m->scan[0].xyz.p, m->stream);
  store_take_xyz(v.surf_xyzi, n_surf, (float*)m->in.p, m->stream);
  SLIO_HIP(hipGetLastError());
  return feed_finish(m, n_corner, n_surf, counts, "slio_lvx_feed_device");
}

int slio_lvx_get_scan(slio_lvx_handle m, int kind, float* xyz, int64_t cap, int64_t* n) {
  LVX_CHECK(m, "slio_lvx_get_scan");
  if ((kind != 0 && kind != 1) || cap < 0) {
    set_error("slio_lvx_get_scan: kind outside {0, 1} or negative capacity");
    return SLIO_EINVAL;
  }
  if (!m->scan[kind].fed) {
    set_error("slio_lvx_get_scan: no scan fed");
    return SLIO_ESTATE;
  }
  if (n) *n = m->scan[kind].n;
  if (!xyz || !m->scan[kind].n) return SLIO_OK;
  if (cap < m->scan[kind].n) {
    set_error("slio_lvx_get_scan: the output holds fewer points than the scan");
    return SLIO_ECAPACITY;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  SLIO_HIP(hipMemcpyAsync(xyz, m->scan[kind].xyz.p, 12 * (size_t)m->scan[kind].n, hipMemcpyDeviceToHost, m->stream));
  SLIO_HIP(hipStreamSynchronize(m->stream));
  return SLIO_OK;
}

int slio_lvx_build_maps(slio_lvx_handle m, const int32_t* valid, int32_t nvalid, int64_t counts[2]) {
  LVX_CHECK(m, "slio_lvx_build_maps");
  if (!valid) {
    if (nvalid != 0) {
      set_error("slio_lvx_build_maps: nvalid without a list");
      return SLIO_EINVAL;
    }
    if (!m->selected) {
      set_error("slio_lvx_build_maps: no cube list given and no slio_lvx_select_cubes before");
      return SLIO_ESTATE;
    }
    valid = m->valid;
    nvalid = m->nvalid;
  } else if (nvalid > 125 || !store_list_ok(valid, nvalid)) {
    set_error("slio_lvx_build_maps: cube index out of range or more than 125 cubes");
    return SLIO_EINVAL;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  for (int k = 0; k < 2; ++k) {
    const float h = k == 0 ? kCellCorner : kCellSurf;
    if (int rc = store_build_grid(m, k, valid, nvalid, h, "slio_lvx_build_maps")) return rc;
    m->scan[k].passed = false;
    if (counts) counts[k] = m->grid[k].n;
  }
  return SLIO_OK;
}

int slio_lvx_pass(slio_lvx_handle m, int kind, const float transform[6], int64_t* nsel) {
  LVX_CHECK(m, "slio_lvx_pass");
  if ((kind != 0 && kind != 1) || !transform || !finite6(transform)) {
    set_error("slio_lvx_pass: kind outside {0, 1} or a transform that is null or not finite");
    return SLIO_EINVAL;
  }
  if (!m->grid[kind].built || !m->scan[kind].fed) {
    set_error("slio_lvx_pass: no map built (slio_lvx_build_maps) or no scan fed (slio_lvx_feed_host)");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  if (int rc = run_pass(m, kind, transform)) return rc;
  if (nsel) {
    const Scan& sc = m->scan[kind];
    std::vector<uint8_t> sl((size_t)sc.n);
    if (sc.n) {
      SLIO_HIP(hipMemcpyAsync(sl.data(), sc.sel.p, (size_t)sc.n, hipMemcpyDeviceToHost, m->stream));
      SLIO_HIP(hipStreamSynchronize(m->stream));
    }
    int64_t c = 0;
    for (uint8_t v : sl) c += v;
    *nsel = c;
  }
  return SLIO_OK;
}

int slio_lvx_get_pass(slio_lvx_handle m, int kind, float* world, int32_t* nbr_idx, float* nbr_sqd, float* coeff,
                      uint8_t* sel) {
  LVX_CHECK(m, "slio_lvx_get_pass");
  if (kind != 0 && kind != 1) {
    set_error("slio_lvx_get_pass: kind outside {0, 1}");
    return SLIO_EINVAL;
  }
  const Scan& sc = m->scan[kind];
  if (!sc.passed) {
    set_error("slio_lvx_get_pass: no slio_lvx_pass of that kind since the last feed or map build");
    return SLIO_ESTATE;
  }
  if (!sc.n) return SLIO_OK;
  SLIO_HIP(hipSetDevice(m->prm.device));
  const size_t n = (size_t)sc.n, K = kind == 0 ? 5 : 8;
  hipStream_t st = m->stream;
  if (world) SLIO_HIP(hipMemcpyAsync(world, sc.world.p, 12 * n, hipMemcpyDeviceToHost, st));
  if (nbr_idx) SLIO_HIP(hipMemcpyAsync(nbr_idx, sc.nbr_idx.p, 4 * n * K, hipMemcpyDeviceToHost, st));
  if (nbr_sqd) SLIO_HIP(hipMemcpyAsync(nbr_sqd, sc.nbr_sqd.p, 4 * n * K, hipMemcpyDeviceToHost, st));
  if (coeff) SLIO_HIP(hipMemcpyAsync(coeff, sc.coeff.p, 16 * n, hipMemcpyDeviceToHost, st));
  if (sel) SLIO_HIP(hipMemcpyAsync(sel, sc.sel.p, n, hipMemcpyDeviceToHost, st));
  SLIO_HIP(hipStreamSynchronize(st));
  return SLIO_OK;
}

int slio_lvx_normal_equations(slio_lvx_handle m, float AtA[36], float AtB[6], int64_t* nsel) {
  LVX_CHECK(m, "slio_lvx_normal_equations");
  if (!AtA || !AtB) {
    set_error("slio_lvx_normal_equations: null output");
    return SLIO_EINVAL;
  }
  if (!m->scan[0].passed || !m->scan[1].passed) {
    set_error("slio_lvx_normal_equations: slio_lvx_pass of both kinds first");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  return sum_partials(m, AtA, AtB, nsel);
}

int slio_lvx_optimize(slio_lvx_handle m, float transform[6], int32_t* iterations, int32_t* is_degenerate) {
  LVX_CHECK(m, "slio_lvx_optimize");
  if (!transform || !finite6(transform)) {
    set_error("slio_lvx_optimize: a transform that is null or not finite");
    return SLIO_EINVAL;
  }
  if (!m->grid[0].built || !m->grid[1].built || !m->scan[0].fed || !m->scan[1].fed) {
    set_error("slio_lvx_optimize: slio_lvx_build_maps and slio_lvx_feed_host first");
    return SLIO_ESTATE;
  }
  SLIO_HIP(hipSetDevice(m->prm.device));
  int iters = 0;
  int& deg = m->is_degenerate;
  float* P = m->matP;
  if (m->grid[0].n > 10 && m->grid[1].n > 100) {  // :814
    for (int it = 0; it < 20; ++it) {  // :821
      ++iters;
      int rc = run_pass(m, 0, transform);
      if (!rc) rc = run_pass(m, 1, transform);
      float AtA[36], AtB[6];
      int64_t nsel = 0;
      if (!rc) rc = sum_partials(m, AtA, AtB, &nsel);
      if (rc) return rc;
      int conv = 0;
      rc = slio_lvx_lm_step(AtA, AtB, nsel, it, transform, &deg, P, &conv);
      if (rc < 0) return rc;
      if (conv) break;
    }
  }
  if (iterations) *iterations = iters;
  if (is_degenerate) *is_degenerate = deg;
  return SLIO_OK;
}

}  // extern "C"

namespace {

// One call of the main loop (:475-1216) around the given feed
template <class Feed>
int process_with(slio_lvx* m, Feed feed, float transform_aft_mapped[6], int32_t* iterations) {
  int rc = slio_lvx_select_cubes(m, m->tobe, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (!rc) rc = slio_lvx_build_maps(m, nullptr, 0, nullptr);
  if (!rc) rc = feed();
  int32_t iters = 0;
  if (!rc) rc = slio_lvx_optimize(m, m->tobe, &iters, nullptr);
  if (rc) return rc;
  if (iters > 0)  // transformUpdate (:188-193) sits inside the `if` of :814
    for (int a = 0; a < 6; ++a) {
      m->last[a] = m->aft[a];
      m->aft[a] = m->tobe[a];
    }
  rc = update_impl(m, m->tobe, (const float*)m->scan[0].xyz.p, m->scan[0].n, (const float*)m->scan[1].xyz.p,
                   m->scan[1].n, nullptr, 0, nullptr, true);
  if (rc) return rc;
  if (transform_aft_mapped) std::memcpy(transform_aft_mapped, m->aft, sizeof m->aft);
  if (iterations) *iterations = iters;
  return SLIO_OK;
}

}  // namespace

extern "C" {

int slio_lvx_process(slio_lvx_handle m, const float* corner_xyz, int64_t n_corner, const float* surf_xyz,
                     int64_t n_surf, float transform_aft_mapped[6], int32_t* iterations) {
  LVX_CHECK(m, "slio_lvx_process");
  if (n_corner < 0 || n_surf < 0 || (n_corner && !corner_xyz) || (n_surf && !surf_xyz)) {
    set_error("slio_lvx_process: bad arguments");
    return SLIO_EINVAL;
  }
  return process_with(
      m, [&] { return slio_lvx_feed_host(m, corner_xyz, n_corner, surf_xyz, n_surf, nullptr); }, transform_aft_mapped,
      iterations);
}

int slio_lvx_process_cloud(slio_lvx_handle m, void* reg, const float* xyzi, int64_t n, float transform_aft_mapped[6],
                           int32_t* iterations, int32_t counts[3]) {
  LVX_CHECK(m, "slio_lvx_process_cloud");
  if (n < 0 || (n && !xyzi)) {
    set_error("slio_lvx_process_cloud: negative size or null cloud");
    return SLIO_EINVAL;
  }
  int32_t dev = -1;
  if (int rc = slio::lreg::device_of(reg, &dev, "slio_lvx_process_cloud")) return rc;
  if (dev != m->prm.device) {
    set_error("slio_lvx_process_cloud: the registration and the mapper are on different devices");
    return SLIO_EINVAL;
  }
  int32_t cnt[3] = {0, 0, 0};
  if (int rc = slio_lreg_run((slio_lreg_handle)reg, xyzi, n, cnt)) return rc;
  if (counts) std::memcpy(counts, cnt, sizeof cnt);
  return process_with(m, [&] { return slio_lvx_feed_device(m, reg, nullptr); }, transform_aft_mapped, iterations);
}

int slio_lvx_get_transforms(slio_lvx_handle m, float tobe_mapped[6], float aft_mapped[6], float last_mapped[6]) {
  LVX_CHECK(m, "slio_lvx_get_transforms");
  if (tobe_mapped) std::memcpy(tobe_mapped, m->tobe, sizeof m->tobe);
  if (aft_mapped) std::memcpy(aft_mapped, m->aft, sizeof m->aft);
  if (last_mapped) std::memcpy(last_mapped, m->last, sizeof m->last);
  return SLIO_OK;
}

int slio_lvx_set_transform(slio_lvx_handle m, const float tobe_mapped[6]) {
  LVX_CHECK(m, "slio_lvx_set_transform");
  if (!tobe_mapped || !finite6(tobe_mapped)) {
    set_error("slio_lvx_set_transform: a transform that is null or not finite");
    return SLIO_EINVAL;
  }
  std::memcpy(m->tobe, tobe_mapped, sizeof m->tobe);
  return SLIO_OK;
}

}  // extern "C"
