// slio_scan.hip -- scan preparation of the IKF runtime on the MI355X (gfx950):
// what turns a driver's sweep, or a set of stored keyframes, into the scan or
// the map a search pass (slio_device.hip) reads.
//
//   * the scan VoxelGrid: downSizeFilterSurf as pcl::VoxelGrid on the device
//     (k_vg_*, vg_begin / vg_enqueue, voxel_device), its geometry and voxel
//     index from slio_voxel.hpp;
//   * undistortion: UndistortPcl's step 5 (k_time_keys, k_undistort);
//   * the keyframe map assembly: every selected keyframe's cloud gathered and
//     transformed in one launch, then the VoxelGrid, into the handle's map or
//     scan (k_kf_gather, kf_assemble; its callers are in slio_mapopt.hip);
//   * the C entry points that only drive these: slio_undistort,
//     slio_scan_upload_voxel, slio_scan_upload_undistort_voxel.
//
// The scan buffers themselves (ensure_scan_buffers) belong to the pass and stay
// in slio_device.hip; sorts, scans and the index build are in slio_map.hip
// (sort_pairs32, scan_launch, build_index: no hipCUB here).  What the files
// use of one another is declared in slio_device.hpp.
// Built like slio_device.hip, with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <shared_mutex>
#include <string>
#include <vector>

#include "slio_common.hpp"
#include "slio_device.hpp"
#include "slio_fkey.hpp"
#include "slio_frontend.h"
#include "slio_so3.hpp"
#include "slio_voxel.hpp"

namespace slio {

// ---------------------------------------------------------------- scan VoxelGrid
// downSizeFilterSurf (laserMapping.cpp:683-686, 737-739): pcl::VoxelGrid
// (PCL 1.10 voxel_grid.hpp applyFilter + CentroidPoint) on the device.

// workgroup -> grid reduction of a box in fkey order (and a count): shuffles,
// then one set of atomics per workgroup.  Every thread of the workgroup must
// call it.
__device__ __forceinline__ void vg_box_reduce(int32_t lo[3], int32_t hi[3], int cnt, int32_t* __restrict__ out) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    for (int d = 32; d > 0; d >>= 1) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], d, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], d, 64));
    }
  for (int d = 32; d > 0; d >>= 1) cnt += __shfl_xor(cnt, d, 64);
  // one set of atomics per workgroup on a small grid (as k_bbox4): one per
  // wavefront of a 391-block grid serialised on the 7 counters' cache line,
  // 128 us for a 100k-point scan
  __shared__ int32_t wl[3][4], wh[3][4];
  __shared__ int wc[4];
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      wl[a][w] = lo[a];
      wh[a][w] = hi[a];
    }
    wc[w] = cnt;
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
    int c = 0;
    for (int q = 0; q < (int)(blockDim.x >> 6); ++q) c += wc[q];
    atomicAdd(out + 6, c);
  }
}

__global__ void k_vg_bbox(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                          int64_t n, int32_t* __restrict__ out) {
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  int cnt = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float c[3] = {x[i], y[i], z[i]};
    if (!(isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))) continue;  // getMinMax3D skips them
    ++cnt;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int32_t k = fkey(c[a]);
      lo[a] = min(lo[a], k);
      hi[a] = max(hi[a], k);
    }
  }
  vg_box_reduce(lo, hi, cnt, out);
}

struct VgGeom {
  float inv[3];
  int minb[3];
  int mul[3];
};

// PCL's geometry (voxel_geometry, slio_voxel.hpp) from the bounding box keys,
// on the device: flags[0] = 1 when no point is finite (empty output),
// flags[1] = 1 when the leaf is too small for the cloud (PCL passes the input
// through).  With either flag set the keys below are meaningless and the
// caller, reading the flags with the voxel count, ignores them.
__global__ void k_vg_geom(const int32_t* __restrict__ bb, float leaf, VgGeom* __restrict__ G,
                          uint32_t* __restrict__ flags) {
  if (threadIdx.x != 0) return;
  VoxelGeom v;
  const VoxelKind kind = voxel_geometry(bb, leaf, &v);
  VgGeom g;
  for (int a = 0; a < 3; ++a) {
    g.inv[a] = v.inv;
    g.minb[a] = v.minb[a];
    g.mul[a] = v.mul[a];
  }
  *G = g;
  flags[0] = kind == kVoxelNone ? 1u : 0u;
  flags[1] = kind == kVoxelPass ? 1u : 0u;
}

// the voxel index of every point (voxel_index, slio_voxel.hpp); non-finite
// points sort last (dropped)
__global__ void k_vg_keys(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                          int64_t n, const VgGeom* __restrict__ Gp, uint32_t* __restrict__ keys,
                          uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const VgGeom G = *Gp;
  const float c[3] = {x[i], y[i], z[i]};
  uint32_t key = 0xFFFFFFFFu;
  if (isfinite(c[0]) && isfinite(c[1]) && isfinite(c[2]))
    key = voxel_index(c[0], c[1], c[2], G.inv[0], G.minb, G.mul);  // (inv[0..2] are one value)
  keys[i] = key;
  vals[i] = (uint32_t)i;
}

__global__ void k_vg_heads(const uint32_t* __restrict__ keys, int64_t n, uint32_t* __restrict__ head) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  head[i] = keys[i] != 0xFFFFFFFFu && (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// one thread per voxel: the centroid, summed in float in the sorted order
// (ascending point index inside a voxel), divided by the count (CentroidPoint
// AccumulatorXYZ: xyz += p; get: xyz / n)
__global__ void k_vg_centroids(const float* __restrict__ x, const float* __restrict__ y,
                               const float* __restrict__ z, const uint32_t* __restrict__ keys,
                               const uint32_t* __restrict__ order, const uint32_t* __restrict__ head,
                               const uint32_t* __restrict__ rank, int64_t n, float* __restrict__ ox,
                               float* __restrict__ oy, float* __restrict__ oz) {
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i0 >= n || !head[i0]) return;
  float sx = 0.0f, sy = 0.0f, sz = 0.0f;
  int64_t j = i0;
  for (; j < n && keys[j] == keys[i0]; ++j) {
    const uint32_t o = order[j];
    sx = sx + x[o];
    sy = sy + y[o];
    sz = sz + z[o];
  }
  const float cnt = (float)(j - i0);
  const uint32_t r = rank[i0];
  ox[r] = sx / cnt;
  oy[r] = sy / cnt;
  oz[r] = sz / cnt;
}

// k_vg_centroids for the keyframe map assembly: the centroid goes out as
// {x, y, z, bits(id)}, id = its rank in the output order, straight into
// build_index's input, and the output's box is folded into obb (fkey order)
// so the map's grid needs no further pass.  With either geometry flag set
// (no finite point / pass-through) the keys are meaningless: nothing is done.
__global__ void __launch_bounds__(256)
k_vg_centroids4(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                const uint32_t* __restrict__ head, const uint32_t* __restrict__ rank, int64_t n,
                const uint32_t* __restrict__ flags, float4* __restrict__ out, int32_t* __restrict__ obb) {
  if (flags[0] | flags[1]) return;  // (uniform)
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  int cnt1 = 0;
  if (i0 < n && head[i0]) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    int64_t j = i0;
    for (; j < n && keys[j] == keys[i0]; ++j) {
      const uint32_t o = order[j];
      sx = sx + x[o];
      sy = sy + y[o];
      sz = sz + z[o];
    }
    const float cnt = (float)(j - i0);
    const uint32_t r = rank[i0];
    const float c[3] = {sx / cnt, sy / cnt, sz / cnt};
    out[r] = make_float4(c[0], c[1], c[2], __uint_as_float(r));
#pragma unroll
    for (int a = 0; a < 3; ++a) lo[a] = hi[a] = fkey(c[a]);
    cnt1 = 1;
  }
  vg_box_reduce(lo, hi, cnt1, obb);
}

// ---------------------------------------------------------------- keyframe map assembly
// LIO-SAM extractCloud (mapOptmization.cpp:1204-1251): every selected
// keyframe's cloud through transformPointCloud (:382-409) into one
// concatenation, in ONE launch.  The keyframes live in the handles' SoA
// arenas; seg[s] describes the s-th NON-EMPTY selected entry: its first
// position in the concatenation, its first point in its arena and the
// float affine of its pose (pcl::getTransformation, host).  (KfSeg, LegoRot
// and lego_to_map: slio_device.hpp; the table is made in slio_mapopt.hip.)
//
// Each workgroup takes tiles of kKfTile consecutive concatenation positions;
// the segments a tile touches (at most kKfTile: none is empty) are staged in
// LDS and each thread finds its own by bisection there.  World point =
// m0 x + m1 y + m2 z + m3, left to right (:400-405; the build has
// -ffp-contract=off).  The VoxelGrid box and finite count of the
// concatenation (k_vg_bbox's work) are folded in: one set of atomics per
// workgroup.  FORM 0: the affine above (LIO-SAM); FORM 1: m[0..8] is a
// LegoRot and the point goes through lego_to_map (LeGO-LOAM).
template <int FORM>
__global__ void __launch_bounds__(kKfTile)
k_kf_gather(const KfSeg* __restrict__ seg, int nseg, int64_t n, float* __restrict__ cx,
            float* __restrict__ cy, float* __restrict__ cz, int32_t* __restrict__ bb) {
  __shared__ KfSeg ls[kKfTile];
  int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
  int cnt = 0;
  const int64_t ntiles = (n + kKfTile - 1) / kKfTile;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i0 = t * kKfTile, i1 = min(i0 + (int64_t)kKfTile, n) - 1;
    // last segment starting at or before i0 / i1 (seg[0].off == 0)
    int s0, s1;
    {
      int a = 0, b = nseg - 1;
      while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if ((int64_t)seg[mid].off <= i0) a = mid; else b = mid - 1;
      }
      s0 = a;
      b = min(nseg - 1, s0 + kKfTile - 1);
      while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if ((int64_t)seg[mid].off <= i1) a = mid; else b = mid - 1;
      }
      s1 = a;
    }
    const int ns = s1 - s0 + 1;  // 1..kKfTile
    __syncthreads();             // the previous tile's readers are done
    if ((int)threadIdx.x < ns) ls[threadIdx.x] = seg[s0 + threadIdx.x];
    __syncthreads();
    const int64_t i = i0 + threadIdx.x;
    if (i <= i1) {
      int a = 0, b = ns - 1;
      while (a < b) {
        const int mid = (a + b + 1) >> 1;
        if ((int64_t)ls[mid].off <= i) a = mid; else b = mid - 1;
      }
      const KfSeg& S = ls[a];
      const int64_t j = i - (int64_t)S.off;
      const float x = S.x[j], y = S.y[j], z = S.z[j];
      float w[3];
      if (FORM == 0) {
        w[0] = ((S.m[0] * x + S.m[1] * y) + S.m[2] * z) + S.m[3];
        w[1] = ((S.m[4] * x + S.m[5] * y) + S.m[6] * z) + S.m[7];
        w[2] = ((S.m[8] * x + S.m[9] * y) + S.m[10] * z) + S.m[11];
      } else {
        const LegoRot R{S.m[0], S.m[1], S.m[2], S.m[3], S.m[4], S.m[5], S.m[6], S.m[7], S.m[8]};
        lego_to_map(R, x, y, z, w[0], w[1], w[2]);
      }
      cx[i] = w[0];
      cy[i] = w[1];
      cz[i] = w[2];
      if (isfinite(w[0]) && isfinite(w[1]) && isfinite(w[2])) {  // getMinMax3D skips the others
        ++cnt;
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const int32_t k = fkey(w[q]);
          lo[q] = min(lo[q], k);
          hi[q] = max(hi[q], k);
        }
      }
    }
  }
  vg_box_reduce(lo, hi, cnt, bb);
}

}  // namespace slio

using namespace slio;

// The VoxelGrid work the scan's downSizeFilterSurf and the keyframe map
// assembly (slio_s2m_map_from_keyframes) share: vg_begin takes the cached
// temporaries and resets the boxes, vg_enqueue runs box -> geometry -> voxel
// keys -> sort -> voxel heads -> ranks.  Everything is enqueued on the handle's
// stream; nothing is read back here.
struct VgWork {
  uint32_t *k0, *k1, *v0, *v1, *hd, *rk;
  int32_t* bb;       // input box keys [0..5], finite points [6]
  int32_t* obb;      // bb + 8: output box keys [0..5] (k_vg_centroids4)
  VgGeom* geom;
  uint32_t* vflags;  // [0] no finite point, [1] leaf too small (pass-through)
  MapDev::Buf* sort_tmp;
};

static int vg_begin(Ctx& c, int64_t n, const char* who, VgWork& w) {
  hipError_t e;
  // (pre[0..3] may hold the undistorted input: slio_scan_upload_undistort_voxel)
  MapDev::Buf* B = c.pre + 8;
  if ((e = MapDev::take(B[0], 4 * n)) || (e = MapDev::take(B[1], 4 * n)) || (e = MapDev::take(B[2], 4 * n)) ||
      (e = MapDev::take(B[3], 4 * n)) || (e = MapDev::take(B[4], 4 * n)) || (e = MapDev::take(B[5], 4 * n)) ||
      (e = MapDev::take(B[6], 64 + sizeof(VgGeom) + 8))) {
    set_error(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  w.k0 = (uint32_t*)B[0].p;
  w.k1 = (uint32_t*)B[1].p;
  w.v0 = (uint32_t*)B[2].p;
  w.v1 = (uint32_t*)B[3].p;
  w.hd = (uint32_t*)B[4].p;
  w.rk = (uint32_t*)B[5].p;
  w.bb = (int32_t*)B[6].p;
  w.obb = w.bb + 8;
  w.geom = reinterpret_cast<VgGeom*>((char*)B[6].p + 64);
  w.vflags = reinterpret_cast<uint32_t*>((char*)B[6].p + 64 + sizeof(VgGeom));
  w.sort_tmp = &B[7];
  // (both boxes in one copy: the scan path pays what it paid for one)
  const int32_t init[16] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0,
                            INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN, 0, 0};
  if ((e = hipMemcpyAsync(w.bb, init, 64, hipMemcpyHostToDevice, c.stream))) {
    set_error(std::string(who) + ": H2D: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  return SLIO_OK;
}

// box_done: the caller's kernel has already folded the box and the finite
// count into w.bb (k_kf_gather), so the cloud is not read for them again
static int vg_enqueue(Ctx& c, const VgWork& w, const float* dx_, const float* dy_, const float* dz_, int64_t n,
                      float leaf, bool box_done, const char* who) {
  hipStream_t st = c.stream;
  hipError_t e;
  // the box, the geometry and the voxel keys stay on the device: the caller
  // makes ONE readback (voxel count and the geometry's flags) where the box
  // used to come back first
  if (!box_done) k_vg_bbox<<<std::min(grid_blocks(n), 64), 256, 0, st>>>(dx_, dy_, dz_, n, w.bb);
  k_vg_geom<<<1, 64, 0, st>>>(w.bb, leaf, w.geom, w.vflags);
  const int nb = grid_blocks(n);
  k_vg_keys<<<nb, 256, 0, st>>>(dx_, dy_, dz_, n, w.geom, w.k0, w.v0);
  if ((e = sort_pairs32(*w.sort_tmp, w.k0, w.k1, w.v0, w.v1, n, st))) {
    set_error(std::string(who) + ": sort: " + hipGetErrorString(e));
    return SLIO_EDEVICE;
  }
  k_vg_heads<<<nb, 256, 0, st>>>(w.k1, n, w.hd);
  return scan_launch(w.hd, w.rk, n, st);
}

// downSizeFilterSurf of n device points (dx_, dy_, dz_) into the handle's scan
int slio::voxel_device(Ctx& c, const float* dx_, const float* dy_, const float* dz_, int64_t n, float leaf,
                       int64_t* n_down) {
  hipStream_t st = c.stream;
  int rc = nbr_settle_shared(c);  // the scan it was searched with is replaced
  if (rc) return rc;
  int64_t m = 0;
  bool passthrough = false;
  do {
    if (n == 0) break;
    hipError_t e;
    VgWork w{};
    if ((rc = vg_begin(c, n, "slio_scan_upload_voxel", w))) break;
    if ((rc = vg_enqueue(c, w, dx_, dy_, dz_, n, leaf, false, "slio_scan_upload_voxel"))) break;
    uint32_t got[4] = {0, 0, 0, 0};
    {
      const Rb rb[3] = {{&got[0], w.rk + n - 1, 4}, {&got[1], w.hd + n - 1, 4}, {&got[2], w.vflags, 8}};
      if ((e = readback(st, rb, 3))) {
        set_error(std::string("slio_scan_upload_voxel: counts: ") + hipGetErrorString(e));
        rc = SLIO_EDEVICE;
        break;
      }
    }
    if (got[2]) break;  // no finite point: empty scan
    if (got[3]) {
      passthrough = true;  // PCL: leaf too small for the cloud, output = input
      break;
    }
    m = (int64_t)got[0] + got[1];
    if (m > c.prm.max_points) {
      set_error("slio_scan_upload_voxel: downsampled scan exceeds max_points");
      rc = SLIO_ECAPACITY;
      break;
    }
    if ((rc = ensure_scan_buffers(c))) break;
    k_vg_centroids<<<grid_blocks(n), 256, 0, st>>>(dx_, dy_, dz_, w.k1, w.v1, w.hd, w.rk, n, c.bx, c.by, c.bz);
    if ((e = hipGetLastError())) {
      set_error(std::string("slio_scan_upload_voxel: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
  } while (0);
  if (!rc && passthrough) {
    if (n > c.prm.max_points) {
      set_error("slio_scan_upload_voxel: scan exceeds max_points");
      rc = SLIO_ECAPACITY;
    } else if (!(rc = ensure_scan_buffers(c))) {
      // non-finite points stay (PCL copies the input as is)
      (void)hipMemcpyAsync(c.bx, dx_, 4 * n, hipMemcpyDeviceToDevice, st);
      (void)hipMemcpyAsync(c.by, dy_, 4 * n, hipMemcpyDeviceToDevice, st);
      (void)hipMemcpyAsync(c.bz, dz_, 4 * n, hipMemcpyDeviceToDevice, st);
      m = n;
    }
  }
  if (!rc) {
    // (no synchronisation: every user of the scan buffers runs on this
    // stream, after the centroids)
    if (m > 0 && c.bx) (void)hipMemsetAsync(c.sel, 0, m, st);
    if (const hipError_t e = hipGetLastError()) {
      set_error(std::string("slio_scan_upload_voxel: ") + hipGetErrorString(e));
      return SLIO_EDEVICE;
    }
    c.n = m;
    c.searched = false;
    if (n_down) *n_down = m;
  }
  return rc;
}

// ---------------------------------------------------------------- scan undistortion
struct UndistEnd {
  double R[9], RL[9], TL[3], pos[3];
};

__global__ void k_time_keys(const float* __restrict__ t, int64_t n, uint32_t* __restrict__ keys,
                            uint32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  // float order as unsigned; t + 0.0f turns -0.0f into +0.0f, so the two
  // zeros tie as they do under the reference's t[a] < t[b]
  keys[i] = (uint32_t)fkey(t[i] + 0.0f) ^ 0x80000000u;
  vals[i] = (uint32_t)i;
}

// UndistortPcl step 5 (IMU_Processing.hpp:351-401): point i of the time
// order takes the IMU segment (head k, tail k + 1) with the largest k <=
// npose - 2 whose offset is below its time -- the segment the reference's
// backward double loop assigns it -- and is moved to the scan end:
//   R_i = R_head Exp(gyr_tail dt),  T_ei = pos + vel dt + 0.5 acc dt dt - pos_end,
//   P' = R_LI^T (R_end^T (R_i (R_LI P + T_LI) + T_ei) - T_LI)
__global__ void k_undistort(const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ z,
                            const float* __restrict__ t, const uint32_t* __restrict__ order, int64_t n,
                            const slio_imu_pose* __restrict__ poses, int np, UndistEnd E, float* __restrict__ ox,
                            float* __restrict__ oy, float* __restrict__ oz, float* __restrict__ ot) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t o = order[i];
  const float px = x[o], py = y[o], pz = z[o], pt = t[o];
  ot[i] = pt;
  const double tt = (double)pt / double(1000);
  // largest k in [0, np-2] with offset[k] < tt, by a scan down from the top:
  // the table has tens of entries and need not increase (an IMU sample
  // between the previous scan's end and this scan's start has a negative
  // offset after the leading 0), so no bisection
  int lo = np - 2;
  while (lo >= 0 && !(poses[lo].offset_time < tt)) --lo;
  if (lo < 0) {
    ox[i] = px;
    oy[i] = py;
    oz[i] = pz;
    return;
  }
  // The reference's backward loop leaves its point iterator on the first
  // point once that point is done ("if (it_pcl == begin) break"), so every
  // earlier segment whose offset is below that point's time compensates it
  // again (IMU_Processing.hpp:365-399): mirrored for i == 0.  A segment
  // whose offset is not below the time is passed over, as the reference's
  // loop condition does per segment; the ones before it are still tried.
  float cx = px, cy = py, cz = pz;
  const int k_end = (i == 0) ? 0 : lo;
  for (int k = lo; k >= k_end; --k) {
    const slio_imu_pose& hd = poses[k];
    const slio_imu_pose& tl = poses[k + 1];
    if (!(tt > hd.offset_time)) continue;
    const double dt = tt - hd.offset_time;
    const double w[3] = {tl.gyr[0] * dt, tl.gyr[1] * dt, tl.gyr[2] * dt};
    double Ex[9];
    qmatrix(so3_exp(w), Ex);
    double Ri[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        Ri[3 * r + cc] = (hd.rot[3 * r] * Ex[cc] + hd.rot[3 * r + 1] * Ex[3 + cc]) + hd.rot[3 * r + 2] * Ex[6 + cc];
    const double P[3] = {(double)cx, (double)cy, (double)cz};
    double Tei[3], a[3], b[3], cv[3], d[3];
#pragma unroll
    for (int q = 0; q < 3; ++q)
      Tei[q] = ((hd.pos[q] + hd.vel[q] * dt) + ((0.5 * tl.acc[q]) * dt) * dt) - E.pos[q];
#pragma unroll
    for (int r = 0; r < 3; ++r)
      a[r] = ((E.RL[3 * r] * P[0] + E.RL[3 * r + 1] * P[1]) + E.RL[3 * r + 2] * P[2]) + E.TL[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) b[r] = ((Ri[3 * r] * a[0] + Ri[3 * r + 1] * a[1]) + Ri[3 * r + 2] * a[2]) + Tei[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) cv[r] = ((E.R[r] * b[0] + E.R[3 + r] * b[1]) + E.R[6 + r] * b[2]) - E.TL[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = (E.RL[r] * cv[0] + E.RL[3 + r] * cv[1]) + E.RL[6 + r] * cv[2];
    cx = (float)d[0];
    cy = (float)d[1];
    cz = (float)d[2];
  }
  ox[i] = cx;
  oy[i] = cy;
  oz[i] = cz;
}

// whether the host's point times are already in k_time_keys' order (the
// same unsigned keys, non-decreasing): then the stable sort is the identity
// and is skipped (a driver's scan usually arrives in firing order)
static bool time_keys_sorted(const float* t, int64_t n) {
  uint32_t prev = 0, bad = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float f = t[i] + 0.0f;  // (-0.0f -> +0.0f, as k_time_keys)
    int32_t b;
    std::memcpy(&b, &f, 4);
    const uint32_t k = (uint32_t)(b >= 0 ? b : b ^ 0x7FFFFFFF) ^ 0x80000000u;
    bad |= (uint32_t)(k < prev);
    prev = k;
  }
  return bad == 0;
}

// undistorted scan in time order into device arrays ux, uy, uz, ut (n each)
static int undistort_device(Ctx& c, const float* x, const float* y, const float* z, const float* t, int64_t n,
                            const slio_imu_pose* poses, int np, const slio_state* xe, float* ux, float* uy, float* uz,
                            float* ut, bool sync_end = true) {
  hipStream_t st = c.stream;
  UndistEnd E;
  qmatrix(Quat{xe->rot[0], xe->rot[1], xe->rot[2], xe->rot[3]}, E.R);
  qmatrix(Quat{xe->rli[0], xe->rli[1], xe->rli[2], xe->rli[3]}, E.RL);
  for (int k = 0; k < 3; ++k) {
    E.TL[k] = xe->tli[k];
    E.pos[k] = xe->pos[k];
  }
  float *dx_ = nullptr, *dy_ = nullptr, *dz_ = nullptr, *dt_ = nullptr;
  uint32_t *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr;
  slio_imu_pose* dp = nullptr;
  int rc = SLIO_OK;
  do {
    hipError_t e;
    MapDev::Buf* B = c.pre + 4;  // pre[0..3]: the caller's output; pre[8..15]: voxel_device
    if ((e = MapDev::take(B[0], 16 * n)) || (e = MapDev::take(B[1], 16 * n)) ||
        (e = MapDev::take(B[2], sizeof(slio_imu_pose) * std::max(np, 1)))) {
      set_error(std::string("slio undistort: hipMalloc: ") + hipGetErrorString(e));
      rc = SLIO_ENOMEM;
      break;
    }
    dx_ = (float*)B[0].p;
    dy_ = dx_ + n;
    dz_ = dx_ + 2 * n;
    dt_ = dx_ + 3 * n;
    k0 = (uint32_t*)B[1].p;
    k1 = k0 + n;
    v0 = k0 + 2 * n;
    v1 = k0 + 3 * n;
    dp = (slio_imu_pose*)B[2].p;
    if ((e = hipMemcpyAsync(dx_, x, 4 * n, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(dy_, y, 4 * n, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(dz_, z, 4 * n, hipMemcpyHostToDevice, st)) ||
        (e = hipMemcpyAsync(dt_, t, 4 * n, hipMemcpyHostToDevice, st)) ||
        (np > 0 && (e = hipMemcpyAsync(dp, poses, sizeof(slio_imu_pose) * np, hipMemcpyHostToDevice, st)))) {
      set_error(std::string("slio undistort: H2D: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
    const int nb = grid_blocks(n);
    k_time_keys<<<nb, 256, 0, st>>>(dt_, n, k0, v0);
    const bool in_order = time_keys_sorted(t, n);  // (while the copies and keys run)
    if (!in_order && (e = sort_pairs32(B[3], k0, k1, v0, v1, n, st))) {
      set_error(std::string("slio undistort: sort: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
    k_undistort<<<nb, 256, 0, st>>>(dx_, dy_, dz_, dt_, in_order ? v0 : v1, n, dp, np, E, ux, uy, uz, ut);
    // (the combined entry's VoxelGrid step follows on the stream and reads back
    // itself: no synchronisation here)
    if ((e = hipGetLastError()) || (sync_end && (e = spin_sync(st)))) {
      set_error(std::string("slio undistort: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
      break;
    }
  } while (0);
  return rc;
}

extern "C" {

int slio_undistort(slio_handle h, const float* x, const float* y, const float* z, const float* t_ms, int64_t n,
                   const slio_imu_pose* poses, int npose, const slio_state* x_end, float* ox, float* oy, float* oz,
                   float* ot_ms) {
  SLIO_CHECK_H(h);
  if (n < 0 || (n > 0 && (!x || !y || !z || !t_ms || !ox || !oy || !oz || !ot_ms)) || npose < 0 ||
      (npose > 0 && !poses) || !x_end || n >= (int64_t)0xFFFFFFFFll) {
    set_error("slio_undistort: bad arguments");
    return SLIO_EINVAL;
  }
  if (n == 0) return SLIO_OK;
  Ctx& c = h->c;
  SLIO_HIP(MapDev::take(c.pre[0], 16 * n));
  float* u = (float*)c.pre[0].p;
  int rc = undistort_device(c, x, y, z, t_ms, n, poses, npose, x_end, u, u + n, u + 2 * n, u + 3 * n);
  if (!rc) {
    hipError_t e;
    if ((e = hipMemcpy(ox, u, 4 * n, hipMemcpyDeviceToHost)) || (e = hipMemcpy(oy, u + n, 4 * n, hipMemcpyDeviceToHost)) ||
        (e = hipMemcpy(oz, u + 2 * n, 4 * n, hipMemcpyDeviceToHost)) ||
        (e = hipMemcpy(ot_ms, u + 3 * n, 4 * n, hipMemcpyDeviceToHost))) {
      set_error(std::string("slio_undistort: D2H: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
    }
  }
  return rc;
}

int slio_scan_upload_undistort_voxel(slio_handle h, const float* x, const float* y, const float* z,
                                     const float* t_ms, int64_t n, const slio_imu_pose* poses, int npose,
                                     const slio_state* x_end, float leaf, int64_t* n_down) {
  SLIO_CHECK_H(h);
  if (n < 0 || (n > 0 && (!x || !y || !z || !t_ms)) || npose < 0 || (npose > 0 && !poses) || !x_end ||
      !(leaf > 0.0f) || n >= (int64_t)0xFFFFFFFFll) {
    set_error("slio_scan_upload_undistort_voxel: bad arguments");
    return SLIO_EINVAL;
  }
  Ctx& c = h->c;
  float* u = nullptr;
  if (n > 0) {
    SLIO_HIP(MapDev::take(c.pre[0], 16 * n));
    u = (float*)c.pre[0].p;
  }
  int rc = n > 0 ? undistort_device(c, x, y, z, t_ms, n, poses, npose, x_end, u, u + n, u + 2 * n, u + 3 * n,
                                    false)
                 : SLIO_OK;
  if (!rc) rc = voxel_device(c, u, u ? u + n : nullptr, u ? u + 2 * n : nullptr, n, leaf, n_down);
  return rc;
}

int slio_scan_upload_voxel(slio_handle h, const float* x, const float* y, const float* z, int64_t n,
                           float leaf, int64_t* n_down) {
  SLIO_CHECK_H(h);
  Ctx& c = h->c;
  if (n < 0 || (n > 0 && (!x || !y || !z)) || !(leaf > 0.0f) || n >= (int64_t)0xFFFFFFFFll) {
    set_error("slio_scan_upload_voxel: bad arguments");
    return SLIO_EINVAL;
  }
  float *dx_ = nullptr, *dy_ = nullptr, *dz_ = nullptr;
  int rc = SLIO_OK;
  if (n > 0) {
    hipError_t e;
    if ((e = MapDev::take(c.pre[0], 12 * n))) {
      set_error(std::string("slio_scan_upload_voxel: hipMalloc: ") + hipGetErrorString(e));
      return SLIO_ENOMEM;
    }
    dx_ = (float*)c.pre[0].p;
    dy_ = dx_ + n;
    dz_ = dx_ + 2 * n;
    if ((e = hipMemcpyAsync(dx_, x, 4 * n, hipMemcpyHostToDevice, c.stream)) ||
        (e = hipMemcpyAsync(dy_, y, 4 * n, hipMemcpyHostToDevice, c.stream)) ||
        (e = hipMemcpyAsync(dz_, z, 4 * n, hipMemcpyHostToDevice, c.stream))) {
      set_error(std::string("slio_scan_upload_voxel: H2D: ") + hipGetErrorString(e));
      rc = SLIO_EDEVICE;
    }
  }
  if (!rc) rc = voxel_device(c, dx_, dy_, dz_, n, leaf, n_down);
  return rc;
}

}  // extern "C"

// What the three branches of kf_assemble share, for n > 0: the buffers the
// branch needs -- the concatenation's SoA in kfb[0] unless it goes straight
// into the scan buffers (into_scan), the segment table in kfb[1], with_in4
// build_index's input in kfb[2] -- then vg_begin, the table's upload and
// k_kf_gather<form> into out[0..2], its box folded into w.bb.
static int kf_gather(Ctx& c, const std::vector<KfSeg>& seg, int64_t n, int form, bool into_scan, bool with_in4,
                     const char* who, VgWork& w, float* out[3]) {
  hipStream_t st = c.stream;
  hipError_t e = hipSuccess;
  if ((!into_scan && (e = MapDev::take(c.kfb[0], 12 * n))) ||
      (e = MapDev::take(c.kfb[1], sizeof(KfSeg) * seg.size())) || (with_in4 && (e = MapDev::take(c.kfb[2], 16 * n)))) {
    set_error(std::string(who) + ": hipMalloc: " + hipGetErrorString(e));
    return SLIO_ENOMEM;
  }
  out[0] = into_scan ? c.bx : (float*)c.kfb[0].p;
  out[1] = into_scan ? c.by : out[0] + n;
  out[2] = into_scan ? c.bz : out[0] + 2 * n;
  KfSeg* dseg = (KfSeg*)c.kfb[1].p;
  if (const int rc = vg_begin(c, n, who, w)) return rc;
  // (pageable source: the copy has left `seg` when the caller's host wait returns)
  SLIO_HIP(hipMemcpyAsync(dseg, seg.data(), sizeof(KfSeg) * seg.size(), hipMemcpyHostToDevice, st));
  const int nblk = (int)std::min<int64_t>((n + kKfTile - 1) / kKfTile, 1024);
  if (form == 0)
    k_kf_gather<0><<<nblk, kKfTile, 0, st>>>(dseg, (int)seg.size(), n, out[0], out[1], out[2], w.bb);
  else
    k_kf_gather<1><<<nblk, kKfTile, 0, st>>>(dseg, (int)seg.size(), n, out[0], out[1], out[2], w.bb);
  SLIO_HIP(hipGetLastError());
  return SLIO_OK;
}

// Gather-transform the n points of `seg` into one concatenation on c's
// stream, VoxelGrid it with edge `leaf`, and make the result c's map
// (slio_s2m_map_from_keyframes, slio_s2m_loop_cloud, slio_lmap_extract) or
// c's scan (slio_s2m_loop_cloud, as_scan).  The callers are in
// slio_mapopt.hip, the index build in slio_map.hip.
int slio::kf_assemble(Ctx& c, const std::vector<KfSeg>& seg, int64_t n, float leaf, bool as_scan,
                      int64_t counts[2], const char* who, int form, bool pass_through) {
  hipStream_t st = c.stream;
  int rc = nbr_settle_shared(c);  // the map (scan) it was searched on (with) is replaced
  if (rc) return rc;
  VgWork w{};
  float* cc[3] = {nullptr, nullptr, nullptr};  // the concatenation
  if (as_scan && pass_through) {
    // the concatenation itself becomes the scan (no VoxelGrid; non-finite
    // points stay): the gather writes the scan buffers, the end state is
    // slio_scan_upload's
    if (n > c.prm.max_points) {
      set_error(std::string(who) + ": the concatenation exceeds max_points");
      return SLIO_ECAPACITY;
    }
    if ((rc = ensure_scan_buffers(c))) return rc;
    if (n > 0) {
      // (w only for the box the gather folds)
      if ((rc = kf_gather(c, seg, n, form, true, false, who, w, cc))) return rc;
      SLIO_HIP(hipMemsetAsync(c.sel, 0, n, st));
      // the call's one host wait: `seg` has left the host, the stores' arenas have been read
      SLIO_HIP(hipStreamSynchronize(st));
    }
    c.n = n;
    c.searched = false;
    if (counts) counts[0] = counts[1] = n;
    return SLIO_OK;
  }
  if (as_scan) {
    // (the gather folds its box into w.bb; the scan's VoxelGrid makes its own)
    if (n > 0 && (rc = kf_gather(c, seg, n, form, false, false, who, w, cc))) return rc;
    // downSizeFilterICP into the scan, as slio_scan_upload_voxel ends (one
    // readback there: `seg` has left the host when it returns)
    int64_t m = 0;
    if ((rc = voxel_device(c, cc[0], cc[1], cc[2], n, leaf, &m))) return rc;
    if (counts) {
      counts[0] = n;
      counts[1] = m;
    }
    return SLIO_OK;
  }
  int64_t m = 0;
  float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  float4* in4 = nullptr;
  if (n > 0) {
    if ((rc = kf_gather(c, seg, n, form, false, true, who, w, cc))) return rc;
    float *cx = cc[0], *cy = cc[1], *cz = cc[2];
    in4 = (float4*)c.kfb[2].p;
    if ((rc = vg_enqueue(c, w, cx, cy, cz, n, leaf, true, who))) return rc;
    // the centroids go out before the count is known (the output has room for
    // n); then the call's ONE readback: voxel count, flags, both boxes
    k_vg_centroids4<<<grid_blocks(n), 256, 0, st>>>(cx, cy, cz, w.k1, w.v1, w.hd, w.rk, n, w.vflags, in4, w.obb);
    uint32_t got[4] = {0, 0, 0, 0};
    int32_t boxes[16];  // the input's, then the output's
    const int32_t *ibox = boxes, *obox = boxes + 8;
    const Rb rb[4] = {{&got[0], w.rk + n - 1, 4}, {&got[1], w.hd + n - 1, 4}, {&got[2], w.vflags, 8},
                      {boxes, w.bb, 64}};
    if (const hipError_t e = readback(st, rb, 4)) {
      set_error(std::string(who) + ": counts: " + hipGetErrorString(e));
      return SLIO_EDEVICE;
    }
    const int32_t* box = obox;
    if (got[2]) {
      m = 0;  // no finite point: empty map
    } else if (got[3]) {
      // PCL: leaf too small for the cloud, output = input (non-finite points
      // stay, as in the scan path; the index clamps them into the grid)
      m = n;
      box = ibox;
      pack_ids(cx, cy, cz, n, in4, st);
    } else {
      m = (int64_t)got[0] + got[1];
    }
    if (m > 0)
      for (int a = 0; a < 3; ++a) {
        mn[a] = fkey_inv(box[a]);
        mx[a] = fkey_inv(box[3 + a]);
      }
  }
  // The result becomes the handle's map as slio_map_upload's would.  A map
  // only this handle holds is rebuilt in place, so its tables and
  // build_index's temporaries are reused scan after scan; a shared one is
  // left to its other users and this handle gets a new map.
  const bool in_place = c.map && c.map.use_count() == 1 && c.map->users.size() == 1;
  if (in_place) {
    MapDev& M = *c.map;
    std::unique_lock<std::shared_mutex> lk(M.mu);
    if ((rc = map_write_begin(c))) return rc;
    M.free_index();
    M.nadd = 0;
    M.next_id = (uint32_t)m;
    M.cell0 = c.prm.grid_cell;
    M.max_cells = c.prm.max_grid_cells;
    rc = build_index(M, in4, m, mn, mx, st, who, false);
    M.broken = rc != 0;
    if (rc) M.free_index();
    M.version++;
    M.dirty = false;
    const int rc2 = map_write_end(c);
    if (rc || rc2) return rc ? rc : rc2;
  } else {
    auto M = std::make_shared<MapDev>();
    M->device = c.prm.device;
    M->cell0 = c.prm.grid_cell;
    M->max_cells = c.prm.max_grid_cells;
    M->next_id = (uint32_t)m;
    if ((rc = build_index(*M, in4, m, mn, mx, st, who, false))) return rc;
    // sharers of this map order their streams after its build
    SLIO_HIP(hipEventCreateWithFlags(&M->ready, hipEventDisableTiming));
    SLIO_HIP(hipEventRecord(M->ready, st));
    M->epoch = 1;
    map_attach(c, M);
    c.seen_epoch = 1;
  }
  c.searched = false;
  if (counts) {
    counts[0] = n;
    counts[1] = m;
  }
  return SLIO_OK;
}
