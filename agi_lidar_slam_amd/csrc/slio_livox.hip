// slio_livox.hip -- livox_mapping's rolling cube map on the device
// (src/livox_mapping/src/laserMapping.cpp: laserCloudCornerArray /
// laserCloudSurfArray, 21 x 11 x 21 cubes of 50 m).
//
// The map itself is the cube store of slio_cube_store.hpp (slio::lvx::CubeStore,
// store_*; slio_cube_store.hip says how a change runs), which A-LOAM's mapper
// (slio_aloam_map.hip) shares; slio_lvx derives from it.  What is
// livox_mapping's own is here:
//
//   append    k_lvx_append   the incoming points through pointAssociateToMap
//                            (:195-217) behind the stored ones, cube index in
//                            double (:1162-1168); out of range = dropped.  A
//                            point that does not transform to finite
//                            coordinates is dropped too (the reference's int()
//                            of it is undefined; x86-64 gives INT_MIN, out of
//                            range)
//
// and the mapper around the store: the cube selection and shift, the scan's
// feed (its VoxelGrid is the store's, of a one-cube map), the 5-NN / 8-NN
// passes over the store's search grids and the optimisation loop
// (slio_lvx_*).
#include <cstring>
#include <vector>

#include "slio_cube_store.hpp"
#include "slio_device.hpp"
#include "slio_frontend.h"
#include "slio_livox.hpp"
#include "slio_lreg.hpp"

using slio::set_error;
using slio::MapDev;
using namespace slio::lvx;

namespace {

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

static void lvx_free(slio_lvx* m) {
  for (Scan& s : m->scan)
    for (MapDev::Buf* b : {&s.xyz, &s.world, &s.nbr_idx, &s.nbr_sqd, &s.coeff, &s.sel, &s.partial})
      if (b->p) (void)hipFree(b->p);
  slio::lvx::store_free(m);
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
