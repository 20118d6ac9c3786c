// slio_device.hpp -- what the three files of the IKF runtime -- the core
// (slio_device.hip), the map (slio_map.hip) and scan preparation
// (slio_scan.hip) -- use of one another, and what the mapping back-ends
// (slio_mapopt.hip) and the cube store (slio_cube_store.hip) use of them: the
// handle's context and map, the error macros, the bounds-check macro of the
// diagnostic build and the host entry points that enqueue a search pass,
// build a map or a scan, or read a few values back.  Internal to the library; every file
// that includes it is a HIP translation unit.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <memory>
#include <shared_mutex>
#include <string>
#include <utility>
#include <vector>

#include "slio_common.hpp"
#include "slio_search.hpp"

#define SLIO_HIP(call)                                                          \
  do {                                                                          \
    hipError_t e_ = (call);                                                     \
    if (e_ != hipSuccess) {                                                     \
      set_error(std::string(#call) + ": " + hipGetErrorString(e_));             \
      return SLIO_EDEVICE;                                                      \
    }                                                                           \
  } while (0)

#ifdef SLIO_BOUNDS_CHECK
// diagnostic build only: report and neutralise an out-of-range index
#define SLIO_BCHK(idx, lim, what)                                                       \
  do {                                                                                  \
    if ((int64_t)(idx) < 0 || (int64_t)(idx) >= (int64_t)(lim)) {                       \
      printf("slio bounds: %s idx %lld lim %lld block %d thread %d\n", what,             \
             (long long)(idx), (long long)(lim), (int)blockIdx.x, (int)threadIdx.x);     \
      idx = 0;                                                                          \
    }                                                                                   \
  } while (0)
#else
#define SLIO_BCHK(idx, lim, what) \
  do {                            \
  } while (0)
#endif

namespace slio {

struct Ctx;

struct MapDev {
  GridGeom g;
  int64_t n = 0;
  int64_t ncells = 0;
  float4* pts = nullptr;          // sorted by cell: x, y, z, bits(map index)
  uint32_t* start = nullptr;      // ncells + 1 prefix offsets
  // coarse level (CoarseView)
  GridGeom cg;
  int64_t nccells = 0;
  float4* clo = nullptr;
  float4* chi = nullptr;
  // block rows (optional, ~9x the points): entry (x, y, z) holds the points
  // of the 9 cells (x, y + j, z + k), j, k in {-1, 0, 1}, with .w = their
  // position in pts; entries are laid out in cell order, so the 3x3x3 block
  // around a cell is ONE contiguous range [bstart[c - 1], bstart[c + 2])
  float4* blk = nullptr;
  uint32_t* bstart = nullptr;     // ncells + 1 prefix offsets into blk
  int64_t nblk = 0;
  int device = 0;
  // map maintenance (slio_map_add_points / slio_map_delete_boxes /
  // slio_map_incremental): deletions are flags on pts positions, additions
  // wait in add4 (id order) until the next rebuild of the index (map_refresh,
  // before the next search pass or download).  Point ids: 0..n-1 for the
  // upload, then the next ids for every surviving added point.
  uint8_t* keep = nullptr;        // n: 0 = deleted since the last build
  float4* add4 = nullptr;         // x, y, z, bits(id)
  uint8_t* akeep = nullptr;
  int64_t nadd = 0, add_cap = 0;
  uint32_t next_id = 0;
  // stored points deleted since the coarse boxes were last made tight (merge
  // rebuilds only widen them): past n / kCoarseRetighten they are rebuilt
  int64_t del_loose = 0;
  std::atomic<uint64_t> version{1};  // bumped by every rebuild (positions change)
  std::atomic<bool> dirty{false};
  // block rows of a rebuilt map are built once it has been searched
  // kBlkAfterPasses times unchanged (a map changed every scan goes without:
  // they cost ~1 ms per rebuild and save ~5 us per search pass)
  std::atomic<bool> blk_deferred{false};
  int stable_passes = 0;
  // Sharing (slio_map_share).  Changes -- edits, rebuilds, block rows --
  // hold mu exclusively; passes and reads hold it shared from reading the
  // views through their launches.  Streams: a change first orders its stream
  // after everything the other users have enqueued (they may still be
  // reading what it overwrites: map_write_begin), then records `ready` and
  // bumps `epoch`; a reader whose stream has not yet waited for the current
  // epoch waits for `ready` (map_read_sync).
  std::shared_mutex mu;
  std::vector<Ctx*> users;  // handles holding this map
  hipEvent_t ready = nullptr;
  uint64_t epoch = 0;
  bool broken = false;  // an index rebuild failed part-way: unusable until a new upload
  int64_t sequential_calls = 0;  // Add_Points calls that took k_ds_sequential (diagnostic)
  float cell0 = 1.0f;             // requested grid cell and cell budget (slio_params)
  int64_t max_cells = 0;
  // device allocations kept across index rebuilds (capacity in bytes): a
  // rebuild per scan must not pay hipMalloc / hipFree of ~GB tables
  struct Buf {
    void* p = nullptr;
    size_t cap = 0;
  };
  Buf b_pts, b_keep, b_start, b_clo, b_chi, b_bstart, b_blk, b_tmp[8], b_ref[6], b_add[8], b_start2, b_keep2;
  static hipError_t take(Buf& b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (bytes <= b.cap) return hipSuccess;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 4;  // headroom: the map grows scan by scan
    hipError_t e = hipMalloc(&b.p, want);
    if (e) {
      (void)hipGetLastError();
      want = bytes;
      e = hipMalloc(&b.p, want);
    }
    if (!e) b.cap = want;
    return e;
  }
  void free_index() {  // the views only; allocations stay for the next build
    pts = nullptr;
    start = nullptr;
    blk = nullptr;
    bstart = nullptr;
    clo = nullptr;
    chi = nullptr;
    keep = nullptr;
    n = ncells = nccells = nblk = 0;
  }
  ~MapDev() {
    if (ready) (void)hipEventDestroy(ready);
    for (Buf* b : {&b_pts, &b_keep, &b_start, &b_clo, &b_chi, &b_bstart, &b_blk, &b_start2, &b_keep2})
      if (b->p) (void)hipFree(b->p);
    for (Buf& b : b_tmp)
      if (b.p) (void)hipFree(b.p);
    for (Buf& b : b_ref)
      if (b.p) (void)hipFree(b.p);
    for (Buf& b : b_add)
      if (b.p) (void)hipFree(b.p);
    if (add4) (void)hipFree(add4);
    if (akeep) (void)hipFree(akeep);
  }
};

struct PoseDev {
  double rq[4], pos[3], lq[4], tli[3];  // quaternions (w, x, y, z)
  double R[9];                          // rot.matrix(), row-major
  double RL[9];                         // offset_R_L_I.matrix(), row-major
};

static_assert(sizeof(PoseDev) == 32 * sizeof(double), "PoseDev: 32 doubles (IkfCtl::pose)");
static_assert(sizeof(IkfCtl::pose[0]) == sizeof(PoseDev), "IkfCtl::pose slots hold a PoseDev");

struct ScanDev {
  const float* bx;
  const float* by;
  const float* bz;
  int64_t n;
};

struct Ctx {
  slio_params prm{};
  hipStream_t own_stream = nullptr;
  hipStream_t stream = nullptr;
  std::shared_ptr<MapDev> map;
  // scan
  int64_t n = 0;
  float* bx = nullptr;
  float* by = nullptr;
  float* bz = nullptr;
  int32_t* nbr_idx = nullptr;
  uint32_t* nbr_pos = nullptr;
  PoseDev* nbr_pose = nullptr;  // pose of the last search pass (device)
  bool nbr_lazy = false;        // nbr_idx / nbr_sqd not yet derived from nbr_pos
  bool nbr_stale = false;       // ... and no longer derivable: another handle rebuilt the shared map
  uint64_t search_version = 0;  // map version the last search pass ran on
  uint64_t seen_epoch = 0;      // the map's last change this handle's stream is ordered after
  hipEvent_t map_ev = nullptr;  // recorded on this stream by another user's map change
  float* wbx = nullptr;  // scan-to-map: the scan in the map frame
  float* wby = nullptr;
  float* wbz = nullptr;
  int s2m_kind = -1;
  float* nbr_sqd = nullptr;
  float4* plane = nullptr;
  uint8_t* sel = nullptr;
  float* resid = nullptr;
  double* chunk_part = nullptr;
  uint32_t* chunk_cost = nullptr;  // per chunk of the last search pass (chunk_order)
  // kNN certificates of the device-resident update (k_search_pass): per point
  // query + bound (the 5 positions are nbr_pos); per chunk the update epoch
  float4* kq = nullptr;
  uint32_t* k6 = nullptr;
  uint32_t* kepoch = nullptr;
  uint32_t kc_next = 0;       // last epoch handed out
  uint32_t kc_epoch = 0;      // the running update's (0: certificates off)
  uint64_t kc_version = 0;    // map version of the update's first pass
  bool kc_stats = false;      // count certified / searched queries (slio_debug_knn_cert): two
                              // same-address atomics per workgroup, off the product path
  uint32_t* chunk_perm = nullptr;  // search order for the next device-resident pass
  int cus_per_xcd = 0;             // CUs per XCD (0: chunk_order off)
  // far queue (deferred queries, see far_search)
  double* d_super = nullptr;
  double* d_super_own = nullptr;
  double* d_seg = nullptr;    // the pass's 64 segment rows (k_super_sums hand-off)
  void* comm = nullptr;        // RCCL communicator of the rank group (slio_comm_init / slio_create_group)
  int group_reduce = 0;        // slio_create_group: 1 RCCL communicator, 2 in-device reduce (k_group_reduce)
  hipEvent_t grp_ev = nullptr; // in-device reduce: end of this rank's pass / of the reduce (rank 0)
  double* gsup = nullptr;      // fused group pass (rank 0): the group's 8 super rows
  uint32_t* garrive = nullptr; // ... and the ranks' arrival counter
  int32_t group_seq = 0;       // fused group pass: the running update's sequence number (0: none)
  int32_t upd_seq = 0;         // (rank 0) last sequence number handed out
  uint32_t* count = nullptr;  // [0] k_super_sums arrival counter, [4..5] far-queue head / tail,
  MapDev::Buf inc[7];         // map_incremental temporaries, kept across scans
                              // (zero between launches)
  MapDev::Buf pre[16];        // undistortion / VoxelGrid temporaries, kept across scans
                              // (per-call hipMalloc + hipFree cost more than the kernels)
  // LIO-SAM keyframe store (slio_s2m_kf_*): one growing SoA arena, keyframe k
  // at [kf_off[k], kf_off[k] + kf_len[k])
  float* kfx = nullptr;
  float* kfy = nullptr;
  float* kfz = nullptr;
  int64_t kf_used = 0, kf_cap = 0;
  std::vector<int64_t> kf_off, kf_len;
  MapDev::Buf kfb[3];         // map assembly: the concatenation (SoA), the segment table,
                              // build_index's input; kept across scans
  hipEvent_t kf_ev = nullptr; // orders another handle's assembly after this store's pushes
                              // (slio_s2m_loop_cloud)
  // loop-closure ICP (slio_icp_correspond): the working cloud (SoA), the last
  // pass's map id and squared distance per working point, the workgroup
  // partials, the device-resident loop's state (slio_icp_align)
  MapDev::Buf icp[5];
  int64_t icp_n = -1;         // working points (-1: no pass yet)
  int64_t icp_far = 0;        // queries the last pass sent down the far path
  IkfCtl* ctl = nullptr;   // device-resident update state (HBM)
  IkfCtl* h_ctl = nullptr;  // mapped, coherent host block: update input and output
  IkfCtl* d_hctl = nullptr; // its device view
  hipEvent_t done_ev = nullptr;  // end of a device-resident update (polled)
  double* h_super = nullptr;  // pinned
  bool searched = false;
  // profiling: event pairs pending per kind, accumulated time
  bool prof = false;
  int prof_mask = 0;  // bit k: time kernel kind k
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending[3];
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  double prof_ms[3] = {0, 0, 0};
  int64_t prof_n[3] = {0, 0, 0};
  // diagnostic switches of the update path, read from the environment once
  // per handle (slio_create, slio_debug_reload_switches): no getenv on the
  // host turnaround between updates
  struct Switches {
    bool no_fuse = false;     // SLIO_NO_FUSE: two launches per pass
    bool no_fuse0 = false;    // SLIO_NO_FUSE0: two launches for the first pass
    bool no_mfma = false;     // SLIO_NO_MFMA: VALU chunk products
    bool event_wait = false;  // SLIO_EVENT_WAIT: wait on a completion event
    bool no_kc = false;       // SLIO_NO_KNN_CERT: every pass searches in full
    bool persist = false;     // SLIO_PERSIST: one persistent launch per update (k_update_persist)
    bool no_reducer = false;  // SLIO_NO_REDUCER: a fused pass's filter step on its last workgroup to arrive
  } sw;
  // persistent update (k_update_persist): the flag replicas, the CU count and
  // the workgroups the device holds at once (-1: not yet queried)
  uint64_t* goflag = nullptr;
  int ncu = 0;
  int64_t persist_cap = -1;
  int last_path = 0;  // the last device-resident update: 1 persistent launch, 0 a launch per pass
  bool dev_counted = false;  // counted in dev_users (slio_create succeeded)
  uint64_t wait_ticks = 0;  // device-side waits give up after this many 100 MHz ticks (0: 1 s;
                            // slio_debug_wait_limit)
  // host clock stamps (CLOCK_MONOTONIC ns) of the last device-resident update
  // (slio_debug_host_stamps)
  bool hstamp = false;
  int64_t hst[8] = {};
};

// readback(): small device -> host reads (scan totals, counters, boxes)
// through a pinned staging buffer of the calling thread, then one polled wait: a copy into
// pageable host memory waits inside the runtime, and a blocking stream
// synchronisation wakes ~10-20 us late.
struct Rb {
  void* dst;
  const void* src;
  size_t n;
};

// One entry of a keyframe assembly's segment table (kf_assemble,
// k_kf_gather): a non-empty keyframe cloud, its place in the concatenation
// and its pose -- a float affine, or a LegoRot in m[0..8]
struct KfSeg {
  const float *x, *y, *z;  // the keyframe's first point in its store's arena (the loop-closure
                           // cloud reads two stores in one launch: slio_s2m_loop_cloud)
  uint32_t off;            // concatenation position of the entry's first point
  uint32_t pad;
  float m[12];
};
constexpr int kKfTile = 256;

// LeGO-LOAM's pointAssociateToMap / transformPointCloud
// (LeGO-LOAM/src/mapOptmization.cpp:578-607, :624-652): not an affine but
// three successive float rotations -- yaw about z, roll about x, pitch about
// y -- then the translation, with the six cached float sines and cosines
// (:562-576, :609-622; the trig in double, rounded to float, on the host)
struct LegoRot {
  float cr, sr, cp, sp, cy, sy, tx, ty, tz;
};
__device__ __forceinline__ void lego_to_map(const LegoRot& T, float x, float y, float z, float& ox, float& oy,
                                            float& oz) {
  const float x1 = T.cy * x - T.sy * y;
  const float y1 = T.sy * x + T.cy * y;
  const float z1 = z;
  const float x2 = x1;
  const float y2 = T.cr * y1 - T.sr * z1;
  const float z2 = T.sr * y1 + T.cr * z1;
  ox = T.cp * x2 + T.sp * z2 + T.tx;
  oy = y2 + T.ty;
  oz = -T.sp * x2 + T.cp * z2 + T.tz;
}

// a rebuilt map gets its block rows once it has been searched this many times
// unchanged (MapDev::blk_deferred)
constexpr int kBlkAfterPasses = 8;

struct SolveArgs;  // slio_device.hip
struct FuseArgs;

// The host entry points the files call across one another (not exported from
// the library).
#pragma GCC visibility push(hidden)
// ---- slio_device.hip
PoseDev make_pose(const slio_pose* x);
hipError_t spin_sync(hipStream_t st);  // polled wait for a stream
hipError_t readback(hipStream_t st, const Rb* rb, int k);
int enqueue_pass(Ctx& c, const PoseDev* Parg, IkfCtl* ctl, int which, int extrinsic_est,
                 const SolveArgs* sa = nullptr, bool with_super = true, bool knn_only = false,
                 const ScanDev* sd = nullptr, const FuseArgs* fuse = nullptr, int persist = 0);
// the last search pass's ids and distances (k_nbr_derive), before its scan or
// map changes: MapDev::mu held by the caller / taken shared
int nbr_settle(Ctx& c);
int nbr_settle_shared(Ctx& c);
int ensure_scan_buffers(Ctx& c);  // the scan and the pass's per-point outputs, allocated once
#ifdef SLIO_BOUNDS_CHECK
void dbg_set_bounds(int64_t npts, int64_t ncells);  // the limits the search's index checks read
#endif
// ---- slio_map.hip
int map_write_begin(Ctx& c);  // MapDev::mu held exclusively by the caller
int map_write_end(Ctx& c);
int map_read_sync(Ctx& c);  // MapDev::mu held by the caller
void map_attach(Ctx& c, std::shared_ptr<MapDev> m);
int map_refresh(Ctx& c, bool adds_only = false);
int grid_blocks(int64_t n);
int build_blk(MapDev& m, hipStream_t st, const char* who);
int build_index(MapDev& m, const float4* in, int64_t n, const float mn[3], const float mx[3], hipStream_t st,
                const char* who, bool with_blk = true, bool in_id_order = false, bool had_points = false);
// out[i] = {x[i], y[i], z[i], bits(i)}: build_index's input from a SoA cloud (k_pack_ids)
void pack_ids(const float* x, const float* y, const float* z, int64_t n, float4* out, hipStream_t st);
// exclusive scan of n flags into rank, enqueued on st (no readback)
int scan_launch(const uint32_t* flag, uint32_t* rank, int64_t n, hipStream_t st);
// stable radix sort of n 32-bit (key, value) pairs by the whole key, enqueued on st
hipError_t sort_pairs32(MapDev::Buf& tmp, const uint32_t* k0, uint32_t* k1, const uint32_t* v0, uint32_t* v1,
                        int64_t n, hipStream_t st);
// ---- slio_scan.hip
// downSizeFilterSurf of n device points (dx_, dy_, dz_) into the handle's scan
int voxel_device(Ctx& c, const float* dx_, const float* dy_, const float* dz_, int64_t n, float leaf,
                 int64_t* n_down);
// Gather-transform the n points of `seg` (FORM `form` of k_kf_gather) into one
// concatenation on c's stream, VoxelGrid it with edge `leaf`, and make the
// result c's map or, as_scan, c's scan.  pass_through (with as_scan only): no
// VoxelGrid, the concatenation itself becomes the scan, `leaf` is not read.
// The one map-building entry of the back-ends: the VoxelGrid is in
// slio_scan.hip, the index build in slio_map.hip.
int kf_assemble(Ctx& c, const std::vector<KfSeg>& seg, int64_t n, float leaf, bool as_scan, int64_t counts[2],
                const char* who, int form = 0, bool pass_through = false);
#pragma GCC visibility pop

}  // namespace slio

struct slio_ctx {
  slio::Ctx c;
};

#define SLIO_CHECK_H(h)                                  \
  do {                                                   \
    if (!(h)) {                                          \
      set_error("null handle");                          \
      return SLIO_EINVAL;                                \
    }                                                    \
    SLIO_HIP(hipSetDevice((h)->c.prm.device));           \
  } while (0)
