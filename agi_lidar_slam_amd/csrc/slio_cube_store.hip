// slio_cube_store.hip -- the rolling cube store of slio_cube_store.hpp
// (slio::lvx::CubeStore, store_*) on the device: the map that livox_mapping's
// mapper (slio_livox.hip) and A-LOAM's (slio_aloam_map.hip) both keep.
//
// Per class the map is ONE SoA of points sorted by cube index, inside a cube
// in the reference's order, with a 4852-entry offset table (device, and a host
// mirror refreshed by the one readback of every change).  A mapper appends the
// incoming points behind the stored ones with its own kernel (its pose
// arithmetic and its cube index; out of range = dropped); from there every
// change is one pass over the whole class:
//
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
// so the VoxelGrids of all valid cubes of a class (livox_mapping
// laserMapping.cpp:1197-1216, up to 125) are one sequence of launches and one
// host wait.  Per cube the result is what slio_scan_upload_voxel gives for
// that cube's cloud alone: k_lvx_geom and k_vg_geom (slio_scan.hip) call the
// same geometry function (slio_voxel.hpp).  A voxel index is below 2^31 by
// PCL's own overflow rule, so the 64-bit key cannot overflow for any leaf: a
// leaf too small for a cube passes that cube through, as PCL does.
//
// The gather of listed cubes and the search grid over a gathered map
// (GridView, slio_livox.hpp) are here too.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "slio_cube_store.hpp"
#include "slio_device.hpp"
#include "slio_fkey.hpp"
#include "slio_livox.hpp"
#include "slio_voxel.hpp"

using slio::fkey;
using slio::set_error;
using slio::MapDev;
using namespace slio::lvx;

namespace {

constexpr uint64_t kDropKey = ~0ull;
constexpr int kSortBits = 45;  // 32 voxel bits + 13 cube bits (kNum < 8191 = the dropped points' field)

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

// the VoxelGrid geometry (voxel_geometry, as k_vg_geom of slio_scan.hip) per
// cube: mode[c] = 1 where the cube's points go through the grid, 0 where they
// stay as they are (not a valid cube, no point, or PCL's "leaf size is too
// small": dx * dy * dz above INT32_MAX)
__global__ void k_lvx_geom(const int32_t* __restrict__ bb, const uint8_t* __restrict__ filt, float leaf,
                           CubeGeom* __restrict__ G, uint8_t* __restrict__ mode) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= kNum) return;
  slio::VoxelGeom v;
  if (!filt[c] || slio::voxel_geometry(bb + 8 * c, leaf, &v) != slio::kVoxelGrid) {
    mode[c] = 0;
    return;
  }
  CubeGeom g;
  g.inv = v.inv;
  for (int a = 0; a < 3; ++a) {
    g.minb[a] = v.minb[a];
    g.mul[a] = v.mul[a];
  }
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
      v = slio::voxel_index(x[i], y[i], z[i], g.inv, g.minb, g.mul);
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

// n x {x, y, z, intensity} on the device -> n x {x, y, z}
__global__ void k_lvx_take_xyz(const float* __restrict__ in, int64_t n, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[3 * i] = in[4 * i];
  out[3 * i + 1] = in[4 * i + 1];
  out[3 * i + 2] = in[4 * i + 2];
}

}  // namespace

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
