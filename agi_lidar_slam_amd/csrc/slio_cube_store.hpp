// slio_cube_store.hpp -- the rolling cube store (slio_cube_store.hip) of the
// two translation units that keep a LOAM cube map on the device
// (slio_livox.hip, slio_aloam_map.hip).  Internal to the library; HIP only.
//
// Per class the store is ONE SoA of points sorted by cube index with a
// 4852-entry offset table; every change is one pass over the whole class and
// one host wait (the header comment of slio_cube_store.hip says how).  The array's
// three extents are members: livox_mapping's is 21 x 11 x 21, A-LOAM's
// 21 x 21 x 11, both kNum = 4851 cubes, index i + W j + W H k.  A mapper brings
// its own append kernel (its pose arithmetic and its cube index) and its own
// list of cubes to filter; everything between "append" and "offsets", the
// gather of listed cubes and the search grid are the store's.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "slio_device.hpp"
#include "slio_livox.hpp"

namespace slio {
namespace lvx {

constexpr uint32_t kDrop = 0xFFFFFFFFu;  // the cube id of a point that leaves the store
constexpr int kMaxListed = 125;          // the longest cube list gathered at once

// workgroups of 256 threads for n items; 0 for none (grid_blocks of
// slio_device.hpp launches at least one), so a caller launches only for n > 0
inline int blocks(int64_t n) { return (int)((n + 255) / 256); }

struct CubeGeom {
  float inv;
  int minb[3];
  int mul[3];
};

struct StoreGrid {
  MapDev::Buf xyz, pts, start;  // the gathered map (n x 3), GridView's arrays
  GridView view{};
  int64_t n = 0;
  bool built = false;
};

struct StoreClass {
  float* xyz[2][3] = {};
  uint32_t* id[2] = {};
  int cur = 0;
  int64_t n = 0;
  std::vector<uint32_t> off = std::vector<uint32_t>(kNum + 1, 0u);  // host mirror
};

struct CubeStore {
  int W = kW, H = kH, D = kD;  // W * H * D == kNum
  hipStream_t stream = nullptr;
  StoreClass cls[3];  // corner map, surf map, and a scan as a one-cube map (its VoxelGrid)
  StoreGrid grid[2];
  // work buffers, shared by the classes (one change runs at a time)
  uint64_t* k0 = nullptr;
  uint64_t* k1 = nullptr;
  uint32_t *v0 = nullptr, *v1 = nullptr, *head = nullptr, *rank = nullptr, *off = nullptr;
  int32_t* bb = nullptr;
  CubeGeom* geom = nullptr;
  uint8_t *filt = nullptr, *mode = nullptr;
  uint2* seg = nullptr;
  // pinned staging: the offset table coming back, the cube flags and the
  // gather's segment table going out.  Every call that fills one ends with a
  // wait on the stream, so the next call never overwrites a copy in flight.
  uint32_t* h_off = nullptr;
  uint8_t* h_filt = nullptr;
  uint2* h_seg = nullptr;
  MapDev::Buf tmp_sort, tmp_scan, in, out;
};

// the stream and every buffer for classes of up to max_points points (the
// device is set by the caller); on an error the caller calls store_free
hipError_t store_alloc(CubeStore* m, size_t max_points);
void store_free(CubeStore* m);
// every class empty, no grid built
void store_clear(CubeStore* m);
// the six shift loops composed: both map classes move by shift; one wait per
// non-empty class
int store_shift(CubeStore* m, const int32_t shift[3], const char* who);
// One change of class k: the N = stored + appended points (appended ones
// already behind the stored ones, ids set) are sorted by cube, the cubes of
// the uploaded flags (with_filter) are replaced by their VoxelGrid, dropped
// points leave, and the offset table comes back: the ONE host wait.
int store_rebuild(CubeStore* m, int k, int64_t N, bool with_filter, float leaf, const char* who);
// the flags of a cube list (every index inside the array) on the device; no wait
int store_upload_filter(CubeStore* m, const int32_t* list, int32_t n);
bool store_list_ok(const int32_t* list, int32_t n);
// the concatenation of the listed cubes (at most kMaxListed) of class k into
// dst (null: m->out) as n x 3, *total points; no wait
int store_gather(CubeStore* m, int k, const int32_t* list, int32_t n, int64_t* total, MapDev::Buf* dst = nullptr);
// the same to the host (xyz null: the size only); one wait
int store_download(CubeStore* m, int k, const int32_t* list, int32_t n, float* xyz, int64_t cap, int64_t* npts,
                   const char* who);
// the search grid of class k, cells of edge h, over the concatenation of the
// listed cubes; one host wait (the map's bounding box)
int store_build_grid(CubeStore* m, int k, const int32_t* list, int32_t n, float h, const char* who);
// the VoxelGrid of a device cloud (n x 3, n >= 1) alone, as the per-cube grid
// of a one-cube map (class 2): dst n_out x 3; non-finite points dropped; one wait
int store_scan_voxel(CubeStore* m, const float* d_xyz, int64_t n, float leaf, MapDev::Buf* dst, int64_t* n_out,
                     const char* who);
// n x {x, y, z, intensity} on the device -> n x {x, y, z}; no wait
void store_take_xyz(const float* d_xyzi, int64_t n, float* d_xyz, hipStream_t st);

}  // namespace lvx
}  // namespace slio
