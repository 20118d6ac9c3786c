/*
 * slio.h — C-ABI drop-in boundary of the MI355X IKF scan-matching core.
 *
 * The reference (zhan994/agi_lidar_slam, S-FAST_LIO) has no plugin API for this
 * path; its seam is the C++ call
 *
 *   kf.update_iterated_dyn_share_modified(R, feats_down_body, ikdtree,
 *                                         Nearest_Points, maximum_iter,
 *                                         extrinsic_est)
 *       src/S-FAST_LIO/include/esekfom.hpp:270-275
 *       called from src/S-FAST_LIO/src/laserMapping.cpp:772-774
 *       and        src/S-FAST_LIO/src/laserMapping_re.cpp:663-665
 *
 * and, inside it, one measurement pass
 *
 *   esekf::h_share_model(dyn_share_datastruct&, feats_down_body, ikdtree,
 *                        Nearest_Points, extrinsic_est)
 *       src/S-FAST_LIO/include/esekfom.hpp:106-227
 *
 * whose per-point work (body->world transform, ikd-Tree 5-NN
 * KD_TREE::Nearest_Search ikd_Tree.cpp:370-402, esti_plane common_lib.h:102-134,
 * residual + range gate, Jacobian row) and whose H^T H / H^T h products
 * (esekfom.hpp:306-319) run here as HIP kernels on gfx950.  The 24x24 filter
 * algebra stays on the host (slio_ikf_update below, host C++).
 *
 * Conventions: plain pointers and sizes, int status (0 ok, <0 error, never
 * throws), one opaque handle per filter; a handle is not thread-safe.  All
 * host buffers are caller-owned.  Errors: slio_last_error() returns a
 * thread-local message for the last failing call on this thread.
 */
#ifndef SLIO_H
#define SLIO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLIO_NUM_MATCH 5   /* NUM_MATCH_POINTS, common_lib.h:22 */
#define SLIO_NPROD 91      /* 78 (H^T H upper triangle) + 12 (H^T h) + 1 (m) */
#define SLIO_NHTH 78
#define SLIO_NSUPER 8      /* fixed summation tree: 8 super-chunks of the scan */
#define SLIO_CHUNK 128     /* scan points per reduction chunk (one workgroup) */

enum {
  SLIO_OK = 0,
  SLIO_EINVAL = -1,    /* bad argument */
  SLIO_ENOMEM = -2,    /* device or host allocation failed */
  SLIO_EDEVICE = -3,   /* HIP runtime error */
  SLIO_ECAPACITY = -4, /* scan larger than params.max_points */
  SLIO_ESTATE = -5,    /* call out of order (e.g. iterate before map upload) */
  SLIO_ETIMEOUT = -6   /* a device-side wait of the update gave up (the persistent
                          update's pass flag or a fused group's gate, > 1 s): the
                          result is not written; the handle's arrival counters
                          are reset, so the next update runs normally */
};

typedef struct slio_ctx* slio_handle;

typedef struct slio_params {
  int32_t device;          /* HIP device ordinal                              */
  int32_t max_points;      /* scan capacity; reference caps at 100000
                              (esekfom.hpp:23-29)                             */
  int32_t rank;            /* this handle's shard of the scan points          */
  int32_t nranks;          /* 1, 2, 4 or 8 (must divide SLIO_NSUPER)          */
  float grid_cell;         /* map grid cell edge in metres; 0 (default): auto,
                              1.0 m, or 1.25 m when the 1.0 m grid would have
                              more than 2^27 cells (speed only)               */
  float plane_threshold;   /* esti_plane threshold, 0.1f (esekfom.hpp:157)    */
  float max_match_sqd;     /* 5th-NN sq.-distance gate, 5 (esekfom.hpp:147)   */
  int32_t lanes_per_query; /* search lanes per scan point: 1, 2, 4, 8 (0 ->
                              tuned default)                                  */
  int64_t max_grid_cells;  /* dense cell-table budget (0 -> 1<<29)            */
  float search_radius;     /* first search sphere radius in metres (default 0:
                              scan the 3x3x3 cell block first); capped at 1.99
                              cells.
                              Any value gives the exact 5-NN; it only tunes
                              speed.                                           */
  float far_query_margin;  /* scan points farther than this (metres) outside
                              the map grid's bounding box get no neighbours
                              (index -1, never selected) instead of the exact
                              coarse-level far search.  They cannot pass the
                              max_match_sqd gate anyway, so only
                              Nearest_Points would differ from ikd-Tree.
                              Default 0: no cut, exact everywhere.            */
} slio_params;

/* Pose slice of state_ikfom used by the measurement model
 * (use-ikfom.hpp:18-27).  Rotations are Sophus::SO3 unit quaternions stored
 * (w, x, y, z); the kernel rotates points with the quaternion exactly as
 * SO3::operator*(Vector3d) does (esekfom.hpp:128-129). */
typedef struct slio_pose {
  double rot[4];  /* x_.rot          */
  double pos[3];  /* x_.pos          */
  double rli[4];  /* x_.offset_R_L_I */
  double tli[3];  /* x_.offset_T_L_I */
} slio_pose;

/* Full 24-D state_ikfom (use-ikfom.hpp:18-27); vector order of boxplus /
 * boxminus (esekfom.hpp:59-73, 236-258): pos, rot, R_LI, T_LI, vel, bg, ba,
 * grav. */
typedef struct slio_state {
  double pos[3];
  double rot[4];
  double rli[4];
  double tli[3];
  double vel[3];
  double bg[3];
  double ba[3];
  double grav[3];
} slio_state;

/* ---- handle lifecycle --------------------------------------------------- */
int slio_params_default(slio_params* p);
int slio_create(slio_handle* out, const slio_params* p);
int slio_destroy(slio_handle h);
/* Use an external hipStream_t (e.g. torch's current stream) instead of the
 * handle's own stream; NULL restores the handle's stream.  torch's DEFAULT
 * stream has the handle NULL: to share a stream with torch collectives, make a
 * torch.cuda.Stream current and pass that one. */
int slio_set_stream(slio_handle h, void* hip_stream);
const char* slio_last_error(void);
/* Fingerprint of the sources this library was compiled from (16 hex digits
 * of a SHA-256 over the csrc sources and these headers; build.py computes the
 * same digest), so a caller can tell a stale prebuilt library. */
const char* slio_build_id(void);

/* ---- map (replaces KD_TREE::Build, ikd_Tree.cpp:355-367, for a static map;
 *      the search side replaces KD_TREE::Nearest_Search ikd_Tree.cpp:370) -- */
/* Upload a map snapshot (host SoA float32, n points) and build the device
 * grid index.  Neighbour indices reported later refer to positions in these
 * arrays.  Device memory: 16 B per point + 4 B per grid cell for the cell-
 * sorted map, and (speed only) ~9x that for the block rows, which are skipped
 * when they do not fit, when n > 477M, or when SLIO_NO_BLOCK_ROWS=1 is set;
 * results are identical either way. */
int slio_map_upload(slio_handle h, const float* x, const float* y,
                    const float* z, int64_t n);
/* Share src's read-only device map with h (same device; batched replay).
 * The share holds the map src had at the time of the call (reference-
 * counted): a later slio_map_upload on src gives src a new map and leaves h
 * on the old one until h shares again (esekf.Esekf re-shares when its
 * KdTreeMap's generation changes). */
int slio_map_share(slio_handle h, slio_handle src);
/* Grid diagnostics: dims[3], cell edge, number of map points. */
int slio_map_info(slio_handle h, int32_t dims[3], float* cell, int64_t* n);

/* ---- map maintenance (the live laserMapping map, replaces the ikd-Tree
 *      calls of laserMapping.cpp:364, 430-431 and map_incremental :382-433) */
/* Map point ids: slio_map_upload gives 0..n-1; each add call gives the new
 * points that survive it the next ids, in list order.  Nearest_Points
 * indices (slio_get_neighbors) are these ids.  Changes are applied to the
 * device map at once (deletions) or queued (additions) and the search index
 * is rebuilt on the device before the next search pass -- no host copy of
 * the map, no re-upload.  A map shared by several handles changes for all of
 * them; do not change it while another handle's update is in flight. */
/* KD_TREE::Add_Points (ikd_Tree.cpp:419-512).  downsample = 1: for every
 * point (in order) the points already in its voxel box [floor(p/ds)*ds,
 * +ds) and the point itself keep only the one nearest the box centre
 * (ties: the stored point with the lower id wins only when strictly
 * nearer); *counter = Add_Points' return value.  downsample = 0: every
 * point is added. */
int slio_map_add_points(slio_handle h, const float* x, const float* y,
                        const float* z, int64_t n, int downsample,
                        float downsample_size, int64_t* counter);
/* KD_TREE::Delete_Point_Boxes (ikd_Tree.cpp:559-579): removes the points in
 * the half-open boxes [min, max) (boxes: nboxes x {min x, y, z, max x, y,
 * z}); *deleted = number of points removed. */
int slio_map_delete_boxes(slio_handle h, const float* boxes, int64_t nboxes,
                          int64_t* deleted);
/* map_incremental (laserMapping.cpp:382-433) on the device: the handle's
 * scan (feats_down_body) to world at state x with pointBodyToWorld's
 * rotation matrices (:276-287), classified against the Nearest_Points of
 * the handle's last search pass (which must have run on the current map),
 * then Add_Points(PointToAdd, downsample, filter_size_map_min) and
 * Add_Points(PointNoNeedDownsample, no downsample).  counts = {|PointToAdd|,
 * |PointNoNeedDownsample|, Add_Points' counter}.  nranks must be 1. */
int slio_map_incremental(slio_handle h, const slio_state* x,
                         double filter_size_map_min, int ekf_inited,
                         int64_t counts[3]);
/* The valid map points in ascending id (KD_TREE::flatten /
 * featsFromMap): cap is the buffers' length; *n = number of points
 * (ECAPACITY if cap is smaller). */
int slio_map_download(slio_handle h, float* x, float* y, float* z,
                      uint32_t* ids, int64_t cap, int64_t* n);
/* lasermap_fov_segment (laserMapping.cpp:309-365), host only: moves the
 * local map box [box_min, box_max] (in/out) with the LiDAR position and
 * returns up to 3 boxes to delete (for slio_map_delete_boxes). */
int slio_fov_segment(const double pos_lid[3], float box_min[3], float box_max[3],
                     int* initialized, double cube_len, float det_range,
                     float boxes_out[18], int* nboxes);

/* ---- scan (feats_down_body, laserMapping.cpp:737-739) -------------------- */
/* Upload the whole scan (host SoA float32, body frame).  With nranks > 1
 * every rank uploads the full scan and processes its own point shard. */
int slio_scan_upload(slio_handle h, const float* x, const float* y,
                     const float* z, int64_t n);
/* downSizeFilterSurf (laserMapping.cpp:683-686, 737-739) on the device: the
 * raw scan (feats_undistort, host SoA float32, n points) through
 * pcl::VoxelGrid with edge `leaf` (PCL 1.10 applyFilter + CentroidPoint:
 * voxel index over the cloud's bounding box, centroids in ascending voxel
 * index, float sums / count; non-finite points skipped; a leaf too small for
 * the cloud copies the input) becomes the handle's scan (feats_down_body),
 * *n_down points, ready for the passes below.  Inside a voxel the points are
 * summed in ascending input order (PCL's std::sort leaves that order
 * implementation-defined; a voxel of >= 3 points can differ from PCL's in
 * the last bits).  ECAPACITY if more than max_points voxels remain. */
int slio_scan_upload_voxel(slio_handle h, const float* x, const float* y,
                           const float* z, int64_t n, float leaf,
                           int64_t* n_down);
/* The handle's current scan (feats_down_body) back to the host. */
int slio_scan_download(slio_handle h, float* x, float* y, float* z);
/* Point range [begin, end) this handle processes for the uploaded scan. */
int slio_shard_range(slio_handle h, int64_t* begin, int64_t* end);

/* ---- one h_share_model pass (esekfom.hpp:106-227) + reduction ----------- */
/* Enqueue one measurement pass on the device.  do_search = ekfom_data.converge
 * (esekfom.hpp:138): 1 re-runs the 5-NN search and the gate, 0 reuses the
 * neighbours / plane / selection of the previous pass exactly like
 * point_selected_surf does.  The pass leaves SLIO_NSUPER x SLIO_NPROD fp64
 * super-chunk sums in the handle's device buffer (rows of super-chunks this
 * rank does not own are zero, so a SUM all-reduce over ranks is an exact
 * gather).  Returns the device pointer through d_super if non-NULL. */
int slio_iterate_async(slio_handle h, const slio_pose* x, int do_search,
                       int extrinsic_est, double** d_super);
/* Make the handle write its super-chunk sums into a caller-owned device
 * buffer of SLIO_NSUPER*SLIO_NPROD doubles (e.g. a torch tensor that an RCCL
 * all-reduce then operates on); NULL restores the handle's own buffer. */
int slio_set_super_buffer(slio_handle h, double* dev_buf);
/* Copy the super-chunk sums to host (synchronises the stream). */
int slio_super_download(slio_handle h, double super_out[SLIO_NSUPER * SLIO_NPROD]);
/* Fixed-order sum of the super-chunk rows: H^T H upper triangle (row-major,
 * i <= j), H^T h with h_i = -pd2 (esekfom.hpp:225), and m = effct_feat_num. */
int slio_reduce_super(const double super_in[SLIO_NSUPER * SLIO_NPROD],
                      double HTH[SLIO_NHTH], double HTh[12], int64_t* m);
/* Convenience: iterate_async + download + reduce (single rank). */
int slio_iterate(slio_handle h, const slio_pose* x, int do_search,
                 int extrinsic_est, double HTH[SLIO_NHTH], double HTh[12],
                 int64_t* m);

/* ---- per-point results (Nearest_Points / point_selected_surf / normvec) -- */
/* For the shard's points (n = end - begin): neighbour map indices (-1 if
 * fewer than 5 map points exist), f32 squared distances ascending (the
 * pointSearchSqDis of esekfom.hpp:135-141), final selection flag.  They are
 * the last SEARCH pass's results: the search pass stores only the neighbours'
 * map positions, and ids and distances are derived from them on this call
 * (or, automatically, before the handle's scan or map is replaced). */
int slio_get_neighbors(slio_handle h, int32_t* idx, float* sqd, uint8_t* sel);
/* Number of scan points of the last pass (of this handle's shard) whose
 * 5-NN search did not finish on the fine grid -- 5th neighbour beyond the
 * 5x5x5 fine-cell cube, or query cell more than 2 cells outside the grid --
 * and went to the coarse-level far search instead (diagnostic; synchronises
 * the stream). */
int slio_far_queries(slio_handle h, int64_t* n);
/* Plane (a, b, c, d) per point; (a,b,c) unit normal, d offset, or NaNs where
 * esti_plane failed or the point was gated out before the fit. */
int slio_get_planes(slio_handle h, float* abcd);
/* Residual pd2 (normvec->points[i].intensity, esekfom.hpp:159-171) of the last
 * pass for selected points, NaN otherwise. */
int slio_get_residuals(slio_handle h, float* pd2);

/* ---- kernel timing (HIP events on the handle's stream) ------------------- */
#define SLIO_KERNEL_SEARCH 0   /* fused search pass (kNN + plane + Jacobian + chunk sums) */
#define SLIO_KERNEL_REUSE 1    /* non-search pass                                          */
#define SLIO_KERNEL_SUPER 2    /* super-chunk sums (+ fused filter step)                   */
#define SLIO_PROFILE_KEEP 16   /* flag: keep the accumulated totals                         */
/* enable == 1 times every launch of every kind (start/stop hipEvents carried
 * in the dispatch packet) and accumulates elapsed device time per kind;
 * otherwise only the kinds whose bit 1 << (kind + 1) is set are timed (e.g.
 * 1 << (SLIO_KERNEL_SEARCH + 1) = 2 times the search pass alone).  Without
 * SLIO_PROFILE_KEEP any call resets the totals; with it, the call only
 * changes what is timed (SLIO_PROFILE_KEEP alone pauses), so timing can be
 * sampled over a subset of launches.  0 disables and resets. */
int slio_profile(slio_handle h, int enable);
/* Accumulated device milliseconds and launch count of a kernel kind
 * (synchronises the stream). */
int slio_profile_read(slio_handle h, int kind, double* ms, int64_t* launches);

/* ---- host IKF driver (update_iterated_dyn_share_modified, host C++) ------ */
/* Optional cross-rank reduction hook: must SUM-all-reduce `count` doubles at
 * device pointer dev_buf in place, ordered on `stream`. */
typedef int (*slio_allreduce_fn)(void* ctx, double* dev_buf, int64_t count,
                                 void* stream);

typedef struct slio_ikf_stats {
  int32_t passes;        /* h_share_model passes run                   */
  int32_t searches;      /* passes with the kNN search                 */
  int32_t valid_passes;  /* passes with effct_feat_num >= 1            */
  int32_t converged;     /* dyn_share.converge at exit                 */
  int64_t last_m;        /* effct_feat_num of the last pass            */
  double device_ms;      /* wall time inside device passes (host clock)*/
} slio_ikf_stats;

#define SLIO_MODE_REFERENCE 0  /* esekfom.hpp:292-345 control flow       */
#define SLIO_MODE_FIXED 1      /* exactly maximum_iter passes, kNN search
                                  every pass, P update at the end        */

/* Run the iterated update on state x (in/out) and covariance P (24x24
 * row-major, in/out) with measurement noise R (LASER_POINT_COV,
 * laserMapping.cpp:29).  reduce may be NULL for a single rank. */
int slio_ikf_update(slio_handle h, slio_state* x, double P[576], double R,
                    int maximum_iter, int extrinsic_est, int mode,
                    slio_allreduce_fn reduce, void* reduce_ctx,
                    slio_ikf_stats* stats);

/* Same update, device-resident: state, covariance and the control flags of
 * esekfom.hpp:292-345 live in HBM and the filter step runs on the device
 * after each pass, so the passes are enqueued back to back with no host round
 * trip; the host synchronises once at the end.  The device filter step is the
 * information form on the D columns H can have non-zero -- D = 6 without
 * extrinsic estimation (H's columns 6..11 are zero, esekfom.hpp:218-220), 12
 * with it -- while slio_ikf_update's host step always works on 12: the same
 * algebra, different operation order, so the two agree to rounding (not
 * bitwise).  In the single-rank configuration each pass after the first is
 * one launch (search or reuse pass, its sums and the filter step).  `reduce` (if any) is called once per pass at
 * enqueue time and must enqueue a stream-ordered SUM all-reduce; with NULL
 * and nranks > 1 the handle's communicator is used (slio_comm_init). */
int slio_ikf_update_device(slio_handle h, slio_state* x, double P[576], double R,
                           int maximum_iter, int extrinsic_est, int mode,
                           slio_allreduce_fn reduce, void* reduce_ctx,
                           slio_ikf_stats* stats);

/* ---- multi-GPU: the per-pass all-reduce inside the library (RCCL) --------
 * The scan's points shard across ranks (slio_params rank / nranks); each
 * pass's 8 x 91 fp64 super rows are SUM-all-reduced (one ncclAllReduce over
 * xGMI) and every rank runs the identical filter step, so all ranks hold the
 * same x and P, bit for bit, as one rank would.  Replaces the per-iteration
 * all-reduce the reference does not have (its laserMapping.cpp:772-774 update
 * runs on one CPU process). */
#define SLIO_COMM_ID_BYTES 128
/* One process, ndev GPUs (the reference's single-process laserMapping node):
 * out[r] = a handle of rank r on devices[r].  p gives the other parameters
 * (rank / nranks / device are set here); ndev divides 8.  Each handle then
 * takes the map (slio_map_upload: a replica per GPU, or slio_map_share between
 * ranks on one device) and the whole scan (slio_scan_upload), and
 * slio_group_ikf_update runs the update on all of them.  The group's reduce
 * backend (slio_group_reduce_kind):
 *   SLIO_GROUP_RCCL   (1) one communicator over all ranks (ncclCommInitAll),
 *                         when every rank has its own GPU;
 *   SLIO_GROUP_DEVICE (2) an in-device fixed-order sum of the ranks' super
 *                         rows by one kernel on rank 0's stream (ordered by
 *                         HIP events), when ranks share a device (RCCL
 *                         refuses that), or across peer-accessible GPUs when
 *                         the environment sets SLIO_GROUP_REDUCE=device.
 * SLIO_GROUP_REDUCE=rccl forces RCCL (an error when ranks share a device).
 * Both give the same bits as one rank. */
#define SLIO_GROUP_RCCL 1
#define SLIO_GROUP_DEVICE 2
int slio_create_group(slio_handle* out, int ndev, const int* devices, const slio_params* p);
/* The reduce backend of a group handle (SLIO_GROUP_*), 0 for a handle made by
 * slio_create, < 0 for a null handle. */
int slio_group_reduce_kind(slio_handle h);
/* slio_ikf_update_device on every rank of a group, enqueued from the calling
 * thread: per pass, each rank's search pass, the all-reduce of the ranks'
 * super rows (RCCL: one ncclGroup; in-device: k_group_reduce), each rank's
 * filter step -- no host round trip until the end.  x and P (in / out) and
 * stats come back from rank 0; the call fails (SLIO_EDEVICE) if any rank's x
 * or P differs from rank 0's.  On any error every rank's stream is drained
 * before the call returns, and the calling thread's current device is
 * restored in every case. */
int slio_group_ikf_update(slio_handle* hs, int n, slio_state* x, double P[576], double R,
                          int maximum_iter, int extrinsic_est, int mode, slio_ikf_stats* stats);
/* One process per GPU (e.g. torchrun): rank 0 makes an id (ncclGetUniqueId),
 * the caller hands it to every rank, each initialises its handle's
 * communicator (ncclCommInitRank with the handle's rank / nranks, a
 * collective call); slio_ikf_update_device with reduce == NULL then
 * all-reduces in the library on the handle's stream. */
int slio_comm_unique_id(uint8_t id[SLIO_COMM_ID_BYTES]);
int slio_comm_init(slio_handle h, const uint8_t id[SLIO_COMM_ID_BYTES]);

/* ---- IMU forward propagation and scan undistortion (ImuProcess::UndistortPcl,
 *      src/S-FAST_LIO/src/IMU_Processing.hpp:253-402) ------------------------ */
/* One IMU sample: stamp (s), linear acceleration, angular velocity. */
typedef struct slio_imu_sample {
  double t;
  double acc[3];
  double gyr[3];
} slio_imu_sample;
/* Pose6D (common_lib.h / set_pose6d): offset from the scan start (s), the
 * world-frame acceleration and bias-free angular velocity at that sample,
 * velocity, position, rotation matrix (row-major). */
typedef struct slio_imu_pose {
  double offset_time;
  double acc[3];
  double gyr[3];
  double vel[3];
  double pos[3];
  double rot[9];
} slio_imu_pose;
/* esekf::predict (esekfom.hpp:82-95) with the process model of
 * use-ikfom.hpp (get_f, df_dx, df_dw): x [+]= f dt, P = F P F^T + G Q G^T. */
int slio_ikf_predict(slio_state* x, double P[576], double dt, const double Q[144],
                     const double acc[3], const double gyr[3]);
/* UndistortPcl steps 1-4 (IMU_Processing.hpp:253-346), host: forward
 * propagation over imu[0..nimu) (imu[0] = the previous scan's last sample,
 * last_imu_, then meas.imu), predicting x / P in place; writes the IMUpose
 * table (*npose <= nimu entries).  acc_s_last / angvel_last /
 * last_lidar_end_time are the ImuProcess members carried between scans. */
int slio_imu_forward(const slio_imu_sample* imu, int nimu, double pcl_beg_time,
                     double pcl_end_time, double* last_lidar_end_time,
                     double mean_acc_norm, const double cov_gyr[3],
                     const double cov_acc[3], const double cov_bias_gyr[3],
                     const double cov_bias_acc[3], double acc_s_last[3],
                     double angvel_last[3], slio_state* x, double P[576],
                     slio_imu_pose* poses, int cap, int* npose);
/* UndistortPcl step 5 (IMU_Processing.hpp:351-401) on the device: the raw
 * scan (x, y, z float32, t = per-point time offset in ms, the `curvature`
 * field of preprocess) sorted by time, every point with t / 1000 > the first
 * pose's offset moved to the scan end state x_end by the IMU pose segment it
 * falls in.  Results (feats_undistort, time order) to the host arrays. */
int slio_undistort(slio_handle h, const float* x, const float* y, const float* z,
                   const float* t_ms, int64_t n, const slio_imu_pose* poses,
                   int npose, const slio_state* x_end, float* ox, float* oy,
                   float* oz, float* ot_ms);
/* The same undistortion, then downSizeFilterSurf (see slio_scan_upload_voxel)
 * without leaving the device: the result is the handle's scan. */
int slio_scan_upload_undistort_voxel(slio_handle h, const float* x, const float* y,
                                     const float* z, const float* t_ms, int64_t n,
                                     const slio_imu_pose* poses, int npose,
                                     const slio_state* x_end, float leaf,
                                     int64_t* n_down);

/* ---- LIO-SAM scan-to-map (src/LIO-SAM/src/mapOptmization.cpp) -------------
 * One handle per feature class: map = laserCloud{Corner,Surf}FromMapDS
 * (slio_map_upload), scan = laserCloud{Corner,Surf}LastDS (slio_scan_upload). */
/* cornerOptimization (kind 0, :1303-1432) / surfOptimization (kind 1,
 * :1438-1515) at transformTobeMapped = {roll, pitch, yaw, x, y, z}:
 * pointAssociateToMap, exact 5-NN in the handle's map, point-to-line (3x3
 * covariance, cv::eigen restated as OpenCV's Jacobi) or point-to-plane
 * (ColPivHouseholderQR) coefficients; kept on the device.  *nsel = number of
 * selected points (laserCloudOri{Corner,Surf}Flag). */
int slio_s2m_coeffs(slio_handle h, int kind, const float transform[6], int64_t* nsel);
/* The handle's coefficients (n x {x, y, z, intensity}) and flags to host. */
int slio_s2m_get_coeffs(slio_handle h, float* coeff, uint8_t* sel);
/* LMOptimization rows (:1578-1626; corners, then surfs) and the normal
 * equations A^T A (6x6) / A^T B (6) of the selected points, fp64 sums in a
 * fixed order rounded to float; *nsel = laserCloudSelNum.  Either handle may
 * be NULL. */
int slio_s2m_normal_equations(slio_handle h_corner, slio_handle h_surf,
                              const float transform[6], float AtA[36], float AtB[6],
                              int64_t* nsel);
/* LMOptimization's host step (:1627-1700): X = solve(AtA, AtB) (QR); on
 * iteration 0 the degeneracy projection matP (eigenvalues < 100) is formed,
 * later iterations reuse it; transform += X; *converged = deltaR < 0.05 deg
 * and deltaT < 0.05 cm.  Returns 1 (nothing done) with fewer than 50
 * correspondences, as the reference's `return false`.  A (numerically)
 * singular A^T A -- an R diagonal below 10 * FLT_EPSILON in the QR, where
 * cv::solve(DECOMP_QR) gives up and zeroes matX -- is a zero step (then
 * converged), not an error, as in the reference, which ignores cv::solve's
 * result. */
int slio_s2m_lm_step(const float AtA[36], const float AtB[6], int64_t nsel, int iter_count,
                     float transform[6], int* is_degenerate, float matP[36], int* converged);

/* -- keyframe store and local map (extractSurroundingKeyFrames, :1152-1270) --
 * Each handle keeps the keyframe clouds of its feature class
 * (cornerCloudKeyFrames / surfCloudKeyFrames, :2069-2077) in device memory,
 * in the LiDAR frame, numbered 0, 1, ... in push order.  Argument errors
 * (null handle, negative sizes, a key out of range) are reported before any
 * device call. */
/* cornerCloudKeyFrames.push_back (:2076-2077) of a host cloud (SoA float32,
 * n points; n == 0 is a valid keyframe); *key_index = its number. */
int slio_s2m_kf_push(slio_handle h, const float* x, const float* y, const float* z,
                     int64_t n, int32_t* key_index);
/* saveKeyFramesAndFactor's copy of laserCloud{Corner,Surf}LastDS (:2069-2077):
 * the handle's current scan becomes a keyframe by a device-to-device copy.
 * ESTATE when the handle has no scan. */
int slio_s2m_kf_push_scan(slio_handle h, int32_t* key_index);
/* Number of keyframes (cloudKeyPoses3D->size(), :1159) and of stored points. */
int slio_s2m_kf_info(slio_handle h, int32_t* nkeys, int64_t* npoints);
/* Points per keyframe, sizes[0..nkeys); ECAPACITY if cap < nkeys. */
int slio_s2m_kf_sizes(slio_handle h, int64_t* sizes, int64_t cap);
/* Forget every keyframe; numbering restarts at 0 (the reference never drops
 * a keyframe cloud: for a new session or a bounded store). */
int slio_s2m_kf_clear(slio_handle h);
/* Keyframe `key` back to the host (tests, saveMapService :486); cap is
 * the buffers' length, *n the keyframe's size (ECAPACITY if cap is smaller). */
int slio_s2m_kf_get(slio_handle h, int32_t key, float* x, float* y, float* z,
                    int64_t cap, int64_t* n);
/* extractCloud (:1204-1251) on the device.  For i in list order keyframe
 * key_ind[i] goes through transformPointCloud (:382-409) with the pose
 * poses6[6 i ..] = {roll, pitch, yaw, x, y, z} -- pcl::getTransformation in
 * float, then m0 x + m1 y + m2 z + m3 per row, left to right (:389-405) --
 * and the clouds are concatenated in list order (a key may repeat:
 * extractNearby :1186-1193 appends the recent keyframes without looking for
 * duplicates).  The concatenation is then downsampled with edge `leaf`
 * (downSizeFilterCorner / downSizeFilterSurf, :1242-1247) under the semantics
 * of slio_scan_upload_voxel: non-finite points dropped, inside a voxel the
 * points summed in ascending position of the concatenation, a leaf too small
 * for the cloud passes the concatenation through, no finite point gives an
 * empty map.  The result becomes the handle's map exactly as slio_map_upload
 * of those points would make it (ids 0..n-1 in output order, the kd-tree
 * rebuild of :1716-1717), without a point travelling to the host: the host
 * waits once, for the voxel count, the flags and the box the grid needs, and
 * then as slio_map_upload does for the index build.  counts = {points
 * concatenated, map points}.  EINVAL for a key out of range, ECAPACITY for
 * more than 2^31 - 1 selected points (the concatenation is not bounded by
 * max_points, which is the scan's capacity); nsel == 0 gives an empty map.
 * The reference's laserCloudMapContainer (:1219-1237, 1250), a cache of transformed
 * keyframes, is not mirrored: the same pose gives the same floats, and
 * transforming a keyframe again reads no more bytes than copying its cached
 * transform would. */
int slio_s2m_map_from_keyframes(slio_handle h, const int32_t* key_ind, const float* poses6,
                                int32_t nsel, float leaf, int64_t counts[2]);

/* -- loop closure (performLoopClosure, :725-826) ------------------------------
 * loopFindNearKeyframes (:945-972) and pcl::IterativeClosestPoint (:766-780)
 * on the device.  PCL is not part of the reference tree: what follows restates
 * PCL 1.10 (registration/impl/icp.hpp, correspondence_estimation.hpp,
 * transformation_estimation_svd.hpp, default_convergence_criteria.hpp,
 * common/impl/transforms.hpp) and IS the specification of these entries, as
 * slio_scan_upload_voxel's comment is for VoxelGrid.  Three stated departures
 * from PCL: (1) the rigid fit runs in double and is rounded to float once
 * (PCL: float throughout); (2) inside a voxel of downSizeFilterICP the points
 * are summed in ascending position of the concatenation (PCL: in the order
 * its index sort leaves them); (3) among map points at exactly equal float
 * distance the nearest is the one this project's search returns first (the
 * lower position in the map's cell-sorted order: entry 0 of
 * slio_get_neighbors), where FLANN's kd-tree order is not pinned by anything.
 * Argument errors are reported before any device call. */
/* loopFindNearKeyframes (:945-972): for i in list order keyframe key_ind[i]
 * of h_corner's store, then the same key of h_surf's store (:959-960), both
 * through transformPointCloud with poses6[6 i ..] -- the float arithmetic of
 * slio_s2m_map_from_keyframes -- concatenated, then downSizeFilterICP
 * (:966-969, mappingICPSize) with edge `leaf` under that entry's VoxelGrid
 * semantics (non-finite points dropped, in-voxel sums in ascending
 * concatenation position, a leaf too small passes the cloud through).
 * as_scan == 0: the result becomes h_dst's MAP, indexed as slio_map_upload
 * would (ids 0..n-1); as_scan == 1: it becomes h_dst's SCAN, the end state of
 * slio_scan_upload_voxel (ECAPACITY beyond max_points).  counts = {points
 * concatenated, points kept}.  No point travels to the host.  The three
 * handles must be live, single-rank and on one device, the two stores of equal
 * length (EINVAL); h_dst may be one of the stores' handles.  The assembly runs
 * on h_dst's stream, ordered by an event after what the stores' streams have
 * pending, and has read the arenas when the call returns.  The caller must not
 * push keyframes to either store concurrently (the reference holds `mtx`
 * around the same reads, :730-735). */
int slio_s2m_loop_cloud(slio_handle h_dst, slio_handle h_corner, slio_handle h_surf,
                        const int32_t* key_ind, const float* poses6, int32_t nsel, float leaf,
                        int as_scan, int64_t counts[2]);
/* One ICP iteration's device work (icp.hpp computeTransformation's loop body
 * up to the fit), one launch and one readback.  h's map is the target
 * (setInputTarget), its scan the source (setInputSource).  T: row-major 4x4,
 * top three rows used.  from_scan == 1: working cloud = T * scan (the initial
 * transformPointCloud with the guess; also getFitnessScore's).  from_scan ==
 * 0: working cloud = T * working cloud, in place -- PCL transforms
 * input_transformed by each iteration's increment, not the source by the
 * accumulated matrix.  Per coordinate ((m0 x + m1 y) + m2 z) + m3 in float.
 * Every working point gets its exact nearest map point: float squared
 * distance (dx dx + dy dy) + dz dz and tie rule of the search pass, so for the
 * same world point it equals entry 0 of slio_get_neighbors bit for bit, index
 * included.  The pair is a correspondence when (double)sqd <= max_dist *
 * max_dist (CorrespondenceEstimation: `distance > max_dist_sqr` skips;
 * INFINITY keeps every finite point); a non-finite working point has none.
 * Over the correspondences, 16 fp64 sums in an order fixed by the point index
 * alone (per workgroup of 256 a butterfly over each wavefront, the four
 * wavefronts in order; the workgroups' partials in order): sums[0..2] = sum
 * of p (working point), [3..5] = sum of q (its map point), [6 + 3 r + c] = sum
 * of q_r p_c, [15] = sum of sqd.  Every term is an exact double (a product of
 * two floats), only the additions round.  *ncorr = correspondences.
 * getFitnessScore() (:780) is slio_icp_correspond(h, final_T, 1, INFINITY)
 * and sums[15] / ncorr.  EINVAL: null handle or pointers, from_scan not 0 / 1,
 * max_dist negative or NaN, a multi-rank handle; ESTATE: no map, no scan, or
 * from_scan == 0 before any from_scan == 1. */
int slio_icp_correspond(slio_handle h, const float T[16], int from_scan, double max_dist,
                        double sums[16], int64_t* ncorr);
/* The last pass, for tests: per working point its correspondence's map id
 * (-1: none, gated out included) and the float squared distance to its
 * nearest map point (+inf: non-finite point or empty map). */
int slio_icp_get_correspondences(slio_handle h, int32_t* idx, float* sqd);
/* The working cloud, for tests; cap = the buffers' length, *n its size. */
int slio_icp_get_working(slio_handle h, float* x, float* y, float* z, int64_t cap, int64_t* n);
/* Working points of the last pass whose nearest the 3x3x3 fine cells around
 * them did not certify (answered exactly on the map's coarse level). */
int slio_icp_far_queries(slio_handle h, int64_t* n);
/* DefaultConvergenceCriteria::ConvergenceState */
enum {
  SLIO_ICP_NOT_CONVERGED = 0,
  SLIO_ICP_ITERATIONS = 1,
  SLIO_ICP_TRANSFORM = 2,
  SLIO_ICP_ABS_MSE = 3,
  SLIO_ICP_REL_MSE = 4,
  SLIO_ICP_NO_CORRESPONDENCES = 5
};
typedef struct slio_icp_params {
  int32_t max_iterations;            /* 100  (:768) */
  int32_t reserved;
  double transformation_epsilon;     /* 1e-6 (:769) */
  double euclidean_fitness_epsilon;  /* 1e-6 (:770) */
} slio_icp_params;
typedef struct slio_icp_state {
  float final_T[16];  /* final_transformation_, row-major (identity or the guess at start) */
  double prev_mse;    /* correspondences_prev_mse_ (DBL_MAX at start) */
  int32_t iterations; /* nr_iterations_ */
  int32_t similar;    /* iterations_similar_transforms_ (stays 0: its limit is 0) */
  int32_t convergence_state;
  int32_t converged;
} slio_icp_state;
int slio_icp_params_default(slio_icp_params* p);
/* guess == NULL: identity */
int slio_icp_state_init(slio_icp_state* s, const float guess[16]);
/* One turn of computeTransformation's loop after the correspondences, host
 * only.  (1) ncorr < 3 (min_number_correspondences_): NO_CORRESPONDENCES,
 * converged = 0, *done = 1.  (2) delta = TransformationEstimationSVD, i.e.
 * pcl::umeyama without scaling, in double from the sums: means sum p / n, sum
 * q / n; Sigma = (sum q p^T) / n - mu_q mu_p^T; 3x3 SVD, S = diag(1, 1,
 * sign(det U det V)), R = U S V^T, t = mu_q - R mu_p; rounded to float (PCL
 * computes this in float on demeaned points: departure (1) above).  (3)
 * final_T = delta * final_T as a float 4x4 product (terms added in index
 * order), ++iterations.  (4) DefaultConvergenceCriteria::hasConverged, in
 * this order: iterations >= max_iterations -> ITERATIONS; cos = 0.5 (trace
 * R_delta - 1) >= 0.99999 and |t_delta|^2 <= transformation_epsilon (the
 * epsilon is compared with the SQUARED translation, as PCL does) ->
 * TRANSFORM; mse = sums[15] / ncorr: |mse - prev_mse| <
 * euclidean_fitness_epsilon -> ABS_MSE; |mse - prev_mse| / prev_mse < 1e-5 ->
 * REL_MSE; each converges at once (max_iterations_similar_transforms_ is 0).
 * Otherwise prev_mse = mse, NOT_CONVERGED, *done = 0. */
int slio_icp_step(const double sums[16], int64_t ncorr, const slio_icp_params* params,
                  slio_icp_state* state, float delta[16], int* done);
/* The whole of icp.align plus getFitnessScore (LIO-SAM :766-780; LeGO-LOAM
 * mapOptmization.cpp:957-975) without a host wait per iteration.  The meaning
 * is that of the lockstep loop over the entries above: slio_icp_state_init
 * (guess); slio_icp_correspond(final_T, from_scan = 1, max_dist);
 * slio_icp_step; then slio_icp_correspond(delta, from_scan = 0, max_dist) and
 * slio_icp_step until *done; at last the fitness pass slio_icp_correspond(
 * final_T, 1, INFINITY).  Every float and double it produces equals that
 * loop's bit for bit: the pass is the same device function with its 3x4
 * transform read from the loop's state in device memory; the 18 entries (16
 * sums, correspondences, far queries) are added over the workgroups' partials
 * in ascending workgroup order starting from +0, one lane per entry, exactly
 * as slio_icp_correspond adds them on the host; one thread then runs
 * slio_icp_step's body (one function compiled for both sides, double division
 * and square root correctly rounded on either).
 * An iteration is two launches (pass, one-workgroup tail) ordered by the
 * stream alone; no kernel waits for another workgroup.  The host enqueues
 * `batch` iterations (batch <= 0: the library's default, 8), reads the state
 * back once, and enqueues another batch while the loop has not ended; launches
 * after the end return at their first instruction.  Then the fitness pass and
 * one last read: ceil(iterations / batch) + 1 host waits per call.
 * *out = the final state; *fitness = sums[15] / ncorr of the fitness pass
 * (DBL_MAX without a correspondence, as getFitnessScore); *far_first = the far
 * queries of the first pass; fitness and far_first may be NULL.  Afterwards
 * slio_icp_get_correspondences, slio_icp_get_working and slio_icp_far_queries
 * read the fitness pass, as they do after the lockstep loop's last call.
 * Errors are slio_icp_correspond's, plus EINVAL for a null prm or out, all
 * reported before any device call.  An empty scan gives NO_CORRESPONDENCES
 * (not converged, 0 iterations) without a launch. */
int slio_icp_align(slio_handle h, const slio_icp_params* prm, const float guess[16], double max_dist,
                   int32_t batch, slio_icp_state* out, double* fitness, int64_t* far_first);

/* ---- LeGO-LOAM mapping (src/LeGO-LOAM/LeGO-LOAM/src/mapOptmization.cpp and
 *      transformFusion.cpp; the loopClosureEnableFlag == true parts are the
 *      entries after slio_lmap_clear) ------------------------------------------
 * One opaque mapper owns four single-rank handles on one device and one
 * stream (and a fifth, SLIO_LMAP_LOOP, from the first loop-closure call on): SLIO_LMAP_CORNER (laserCloudCornerFromMapDS, laserCloudCornerLastDS,
 * cornerCloudKeyFrames), SLIO_LMAP_SURF_TOTAL (laserCloudSurfFromMapDS,
 * laserCloudSurfTotalLastDS), SLIO_LMAP_SURF (laserCloudSurfLastDS,
 * surfCloudKeyFrames) and SLIO_LMAP_OUTLIER (laserCloudOutlierLastDS,
 * outlierCloudKeyFrames).  Everything is in LeGO-LOAM's camera-like frame;
 * poses are {rx, ry, rz, tx, ty, tz} (transformTobeMapped's layout); no axis
 * swap appears anywhere.  Argument errors are reported before any device call.
 *
 * Stated departures from the reference:
 *  - the 5-NN is exact and ties at equal float distance go to the lower
 *    position in the map's cell-sorted order (slio_get_neighbors), where
 *    FLANN's order is not pinned by anything;
 *  - inside a voxel the points are summed in ascending position of the input
 *    (slio_scan_upload_voxel's VoxelGrid semantics);
 *  - sin / cos / atan2 / asin of a float are the double functions rounded to
 *    float;
 *  - the key pose is transformTobeMapped itself.  The reference passes it
 *    through an iSAM2 chain of one prior and successive between-factors
 *    (:1656-1749); without loop closures that chain's optimum is the composed
 *    odometry, so GTSAM returns the same pose up to its own rounding and
 *    :1737-1749 write that value back.  GTSAM is absent here;
 *  - the reference's cache of transformed keyframes (surrounding*CloudKeyFrames)
 *    is not mirrored: without loop closure a key's pose never changes, so
 *    transforming it again gives the same floats.  The cache's list order,
 *    which fixes the concatenation order, is kept (the caller's key list). */
typedef struct slio_lmap* slio_lmap_handle;
enum {
  SLIO_LMAP_CORNER = 0,
  SLIO_LMAP_SURF_TOTAL = 1,
  SLIO_LMAP_SURF = 2,
  SLIO_LMAP_OUTLIER = 3,
  SLIO_LMAP_LOOP = 4 /* map nearHistorySurfKeyFrameCloudDS, scan latestSurfKeyFrameCloud */
};
typedef struct slio_lmap_params {
  int32_t device;
  int32_t max_points;          /* capacity of every downsampled scan cloud               */
  float leaf_corner;           /* downSizeFilterCorner, 0.2 (:265)                       */
  float leaf_surf;             /* downSizeFilterSurf, 0.4 (:266)                         */
  float leaf_outlier;          /* downSizeFilterOutlier, 0.4 (:267)                      */
  float pose_leaf;             /* downSizeFilterSurroundingKeyPoses, 1.0 (:274)          */
  float search_radius;         /* surroundingKeyframeSearchRadius, 50 (utility.h:79)     */
  int32_t max_iterations;      /* the 10 of scan2MapOptimization (:1612)                 */
  float mapping_interval;      /* mappingProcessInterval, 0.3 (utility.h:31)             */
  float scan_period;           /* scanPeriod, 0.1 (utility.h:28)                         */
  float keyframe_distance;     /* the 0.3 m of saveKeyFramesAndFactor (:1639)            */
  float grid_cell;             /* slio_params.grid_cell of the two map handles (0: auto) */
  int32_t reserved[4];
} slio_lmap_params;
int slio_lmap_params_default(slio_lmap_params* p);
int slio_lmap_create(slio_lmap_handle* out, const slio_lmap_params* p);
int slio_lmap_destroy(slio_lmap_handle m);
/* One of the five handles (SLIO_LMAP_*), for the getters this library already
 * has -- slio_scan_download, slio_map_download, slio_map_info,
 * slio_get_neighbors, slio_far_queries, slio_s2m_kf_info / _sizes / _get --
 * and, for tests and users without the front-end, slio_map_upload /
 * slio_scan_upload in place of slio_lmap_extract / slio_lmap_feed_*.  The
 * mapper keeps ownership. */
int slio_lmap_get_handle(slio_lmap_handle m, int which, slio_handle* out);
/* downsampleCurrentScan (:1197-1220), device to device, from the front-end's
 * published last clouds (slio_lego_odom_last_view, slio_frontend.h):
 * cornerLastDS = VoxelGrid(corner, leaf_corner), surfLastDS = VoxelGrid(surf,
 * leaf_surf), outlierLastDS = VoxelGrid(outlier, leaf_outlier), surfTotalLastDS
 * = VoxelGrid(surfLastDS ++ outlierLastDS, leaf_surf), each under
 * slio_scan_upload_voxel's semantics.  No point crosses PCIe; the host waits
 * for each grid's voxel count.  The front-end's buffers have been read when
 * the call returns.  counts = the four clouds' sizes in SLIO_LMAP_* order.
 * `lego` is a slio_lego_handle.  ESTATE when its last odometry call did not
 * publish (or the odometry is not enabled); EINVAL for another device. */
int slio_lmap_feed_lego(slio_lmap_handle m, void* lego, int64_t counts[4]);
/* The same from three host clouds (n x {x, y, z, intensity}, the layout of
 * slio_lego_odom_get_last). */
int slio_lmap_feed_host(slio_lmap_handle m, const float* corner_xyzi, int64_t n_corner,
                        const float* surf_xyzi, int64_t n_surf, const float* outlier_xyzi,
                        int64_t n_outlier, int64_t counts[4]);
/* extractSurroundingKeyFrames' cloud work (:1166-1194): for i in list order
 * key key_ind[i] (surroundingExistingKeyPosesID; a key may repeat) goes
 * through transformPointCloud (:624-652: yaw about z, roll about x, pitch
 * about y in float, then the translation) with its pose from the mapper's own
 * key-pose table.  Corner map = the keys' corner clouds; surf map = each
 * key's surf cloud followed by its outlier cloud (:1179-1183).  Both are
 * downsampled (leaf_corner / leaf_surf) and indexed in place as
 * slio_s2m_map_from_keyframes does.  counts = {corner points concatenated,
 * corner map points, surf points concatenated, surf map points}.  EINVAL for
 * a key out of range. */
int slio_lmap_extract(slio_lmap_handle m, const int32_t* key_ind, int32_t nsel, int64_t counts[4]);
/* cornerOptimization (kind 0, :1222-1370) / surfOptimization (kind 1,
 * :1372-1450) at transformTobeMapped = transform, and LMOptimization's rows
 * (:1477-1537) of the selected points with their per-workgroup fp64 partial
 * sums, after the search in one launch.  The plane of kind 1 is
 * cv::solve(DECOMP_QR) on the 5 x 3 system (:1395) as slio_cvsolve.hpp
 * restates it; a failed solve leaves x = 0, the NaNs that follow unselect the
 * point.  nsel may be NULL (no wait then).  EINVAL: kind outside {0, 1};
 * ESTATE: no map or no scan of that kind. */
int slio_lmap_coeffs(slio_lmap_handle m, int kind, const float transform[6], int64_t* nsel);
/* The kind's coefficients (n x 4) and flags of the last slio_lmap_coeffs. */
int slio_lmap_get_coeffs(slio_lmap_handle m, int kind, float* coeff, uint8_t* sel);
/* A^T A / A^T B of the rows the last slio_lmap_coeffs of BOTH kinds left (at
 * the transform given there): fp64 sums in k_s2m_rows' fixed tree -- a
 * butterfly per wavefront, the four wavefronts in order, workgroups in order,
 * corners before surfs -- rounded to float.  ESTATE unless both kinds'
 * coefficients are current (an empty scan counts as current once computed). */
int slio_lmap_normal_equations(slio_lmap_handle m, float AtA[36], float AtB[6], int64_t* nsel);
/* scan2MapOptimization's loop (:1606-1621) on the same kernels: runs only when
 * the corner map holds more than 10 points and the surf map more than 100
 * (else *iterations = 0 and transform is untouched); at most max_iterations
 * turns of coeffs(0), coeffs(1), normal equations (one wait) and
 * slio_s2m_lm_step -- which, read beside LMOptimization :1539-1600, is the same
 * function (QR solve, eigenvalue threshold 100, the 50-row gate, 0.05 / 0.05).
 * *iterations = turns executed.  transformUpdate is the caller's
 * (slio_lmap_transform_update). */
int slio_lmap_optimize(slio_lmap_handle m, float transform[6], int32_t* iterations, int32_t* is_degenerate);
/* saveKeyFramesAndFactor's cloud copies (:1751-1766): cornerLastDS, surfLastDS
 * and outlierLastDS become keyframe *key of the three stores by
 * device-to-device copies, pose6 its entry of the key-pose table
 * (cloudKeyPoses6D; see the departure above).  Before any feed the three
 * clouds are empty, which is a valid keyframe. */
int slio_lmap_save_keyframe(slio_lmap_handle m, const float pose6[6], int32_t* key);
/* cloudKeyPoses6D: nkeys x 6; ECAPACITY if cap < nkeys.  poses6 may be NULL. */
int slio_lmap_get_key_poses(slio_lmap_handle m, float* poses6, int32_t cap, int32_t* nkeys);
/* Forget every keyframe and key pose (the stores' arenas stay allocated). */
int slio_lmap_clear(slio_lmap_handle m);
/* -- loop closure (loopClosureEnableFlag == true: :844-1023, :1042-1097,
 *    :1769-1798) ---------------------------------------------------------------
 * The ICP is slio_icp_align (or the lockstep loop over slio_icp_correspond /
 * slio_icp_step) on the SLIO_LMAP_LOOP handle with max_dist 100, 100
 * iterations, 1e-6, 1e-6 (:957-961); PCL's rules and the three departures
 * stated above slio_s2m_loop_cloud hold here too.  GTSAM is absent: the factor
 * graph is the caller's, and what it returns comes back through
 * slio_lmap_set_key_poses.
 *
 * The recent-keyframe branch of extractSurroundingKeyFrames (:1042-1097) is a
 * host key list handed to slio_lmap_extract, which may repeat keys.  The
 * reference caches the transformed clouds of that list
 * (recent*CloudKeyFrames) and clears the cache in correctPoses; poses change
 * nowhere else, so transforming a key from the store with the current table
 * gives the floats the cache holds.  The cache is not mirrored; its list
 * order, which fixes the concatenation order, is kept.
 *
 * Stated departures of the loop clouds:
 *  - transformPointCloud(cloud, pose*) (:654-687) writes cos(pose->yaw) * x;
 *    whether that multiplies in float or in double depends on which cos the
 *    translation unit's headers select, and nothing in the tree pins it.  The
 *    cached-sine form of :624-652 is used: float products, the double
 *    functions rounded to float (slio_lmap_extract's arithmetic);
 *  - the (int)intensity >= 0 filter (:901-911) keeps every point the stores
 *    can hold from the front-end (a VoxelGrid mean of row + col / 10000 is
 *    never negative); the stores keep no intensity and the filter is not
 *    applied;
 *  - ties of the nearest neighbour and the in-voxel summation order are as
 *    stated for slio_s2m_loop_cloud and at the head of this section. */
/* correctPoses' device side (:1775-1794): replaces the mapper's key-pose
 * table (cloudKeyPoses6D as {rx, ry, rz, tx, ty, tz} per key), which
 * slio_lmap_extract and slio_lmap_loop_clouds read.  EINVAL unless nkeys
 * equals the table's length. */
int slio_lmap_set_key_poses(slio_lmap_handle m, const float* poses6, int32_t nkeys);
/* detectLoopClosure's cloud work (:889-931).  Source: key `latest`'s corner
 * cloud, then its surf cloud, at its pose, concatenated and NOT downsampled,
 * becomes the loop handle's scan (ECAPACITY beyond max_points).  Target: keys
 * closest - search_num .. closest + search_num, skipping k < 0 and
 * k > latest (:916-918; a target that contains `latest` itself is reproduced),
 * for each key corner then surf, concatenated and passed through the
 * VoxelGrid with edge `leaf` (downSizeFilterHistoryKeyFrames, 0.4, :269)
 * under slio_scan_upload_voxel's semantics, becomes the loop handle's map,
 * indexed as slio_map_upload would.  No point travels to the host.  counts =
 * {source concatenated, source kept, target concatenated, target points}.
 * EINVAL for a key out of range, search_num < 0 or a leaf that is not
 * positive, before any device call. */
int slio_lmap_loop_clouds(slio_lmap_handle m, int32_t latest, int32_t closest, int32_t search_num,
                          float leaf, int64_t counts[4]);
/* -- host only, callable without a GPU -- */
/* transformAssociateToMap (mapOptmization.cpp:394-519; transformFusion.cpp
 * :91-215 is the same formula writing transformMapped): float arithmetic in
 * the reference's expression order. */
int slio_lmap_associate_to_map(const float transform_sum[6], const float transform_bef_mapped[6],
                               const float transform_aft_mapped[6], float transform_tobe_mapped[6]);
/* transformUpdate (:521-560): the IMU blend 0.998 / 0.002 on rx (pitch) and rz
 * (roll) from the ring (imu_time, imu_roll, imu_pitch)[imu_len] with
 * imuPointerLast = imu_last (< 0: no IMU) and *imu_front = imuPointerFront
 * (in/out), interpolated at time_odometry + scan_period; then bef = sum,
 * aft = tobe. */
int slio_lmap_transform_update(float transform_tobe_mapped[6], const float transform_sum[6],
                               double time_odometry, float scan_period, const double* imu_time,
                               const float* imu_roll, const float* imu_pitch, int32_t imu_len,
                               int32_t imu_last, int32_t* imu_front, float transform_bef_mapped[6],
                               float transform_aft_mapped[6]);
/* transformFusion.cpp's state: laserOdometryHandler (:217-254) = fuse with
 * aft == NULL: transformSum = sum, transformMapped from the triple;
 * odomAftMappedHandler (:256-277) = sum == NULL: stores aft / bef. */
typedef struct slio_lmap_fusion {
  float transform_sum[6], transform_bef_mapped[6], transform_aft_mapped[6], transform_mapped[6];
} slio_lmap_fusion;
int slio_lmap_fuse(slio_lmap_fusion* f, const float transform_sum[6], const float aft_mapped[6],
                   const float bef_mapped[6]);
/* saveKeyFramesAndFactor's decision (:1629-1645): *save = 1 for the first
 * frame (nkeys == 0) or when the float distance |cur - prev| is not below
 * `distance` (the reference's double 0.3). */
int slio_lmap_keyframe_decision(const float prev_pos[3], const float cur_pos[3], int32_t nkeys,
                                double distance, int* save);
/* detectLoopClosure's search (:863-887): among the keys (key_xyz nkeys x 3 =
 * cloudKeyPoses3D, key_time = cloudKeyPoses6D.time) whose float squared
 * distance (dx dx + dy dy) + dz dz to cur_pos (currentRobotPosPoint) is below
 * radius^2 (historyKeyframeSearchRadius, 5.0, utility.h:94), taken in
 * ascending distance, equal distances by lower key, the first with
 * |key_time - t| > time_diff (30.0, double) is *closest; -1 when there is
 * none. */
int slio_lmap_detect_loop(const float* key_xyz, const double* key_time, int32_t nkeys,
                          const float cur_pos[3], double t, float radius, double time_diff,
                          int32_t* closest);
/* performLoopClosure after the ICP (:992-1012), float affine arithmetic in
 * the reference's order.  final_T: the ICP's camera-frame result, row-major
 * 4x4.  (x, y, z, roll, pitch, yaw) = pcl::getTranslationAndEulerAngles of it
 * (roll = atan2(t21, t22), pitch = asin(-t20), yaw = atan2(t10, t00));
 * correctionLidarFrame = pcl::getTransformation(z, x, y, yaw, roll, pitch);
 * tWrong = getTransformation(tz, tx, ty, rz, rx, ry) of latest_pose6 = {rx,
 * ry, rz, tx, ty, tz} (:1032-1036); tCorrect = correctionLidarFrame * tWrong
 * as an affine product (linear part L1 L2, translation L1 t2 + t1, every sum
 * in index order).  pose_from = {x, y, z, roll, pitch, yaw} of tCorrect;
 * pose_to = closest_pose6 as {tz, tx, ty, rz, rx, ry} (:1025-1030); *noise =
 * (float)fitness (:1009).  poseFrom.between(poseTo) and the factor are the
 * caller's GTSAM. */
int slio_lmap_loop_correction(const float final_T[16], const float latest_pose6[6],
                              const float closest_pose6[6], double fitness, float pose_from[6],
                              float pose_to[6], float* noise);
/* The M x N QR of slio_cvsolve.hpp for tests: (m, n) in {(5, 3), (3, 3),
 * (6, 6)}; returns 1 where the solve gives up (x zeroed). */
int slio_lmap_qr_solve(int m, int n, const float* A, const float* b, float* x);

/* ---- livox_mapping laserMapping (src/livox_mapping/src/laserMapping.cpp): the
 *      rolling cube map, its host formulas and the Gauss-Newton step -----------
 * All path:line below are in that file.  laserCloudCornerArray /
 * laserCloudSurfArray are 21 x 11 x 21 cubes of 50 m (:64-72), cube index
 * i + 21 j + 231 k; kind 0 is the corner class, kind 1 the surf class.  One
 * opaque handle owns both classes on one device and one stream.  For every
 * class and cube the device holds exactly the ordered cloud the reference holds
 * in laserCloud*Array[ind] after the same calls; slio_lvx_get_cube and
 * slio_lvx_cube_sizes show it.  Poses are {rx, ry, rz, tx, ty, tz}
 * (transformTobeMapped's layout), clouds n x {x, y, z} float32; the intensity
 * is not stored (nothing up to :1246 reads it).
 *
 * Errors: SLIO_OK or a negative SLIO_E* with slio_last_error() set.  Argument
 * errors (null pointers, negative sizes, a kind outside {0, 1}, a cube outside
 * 0 .. 4850, a pose that is not finite) are reported before any device call.
 *
 * slio_lvx_process is one call of the node's main loop (:475-1216); the other
 * entries are its stages, for tests and for users who drive them themselves.
 *
 * Stated departures from the reference:
 *  - k-NN ties at equal float distance go to the lower position in the
 *    cell-sorted map, where FLANN's order is not pinned by anything;
 *  - neighbour lists of points the gate rejects are not produced;
 *  - inside a voxel the points are summed in ascending position of the input
 *    (slio_scan_upload_voxel's VoxelGrid semantics; the stored points of a cube
 *    come before the appended ones), where PCL's std::sort leaves it open;
 *  - sin / cos / sqrt of a float are the double functions (rounded to float
 *    where the reference assigns to one);
 *  - a point whose map-frame coordinates are not finite, or beyond 1e6 m, is
 *    dropped at append: the reference converts it with int(), which is
 *    undefined (x86-64 gives INT_MIN: out of range, dropped as well). */
typedef struct slio_lvx* slio_lvx_handle;
#define SLIO_LVX_CUBES 4851 /* laserCloudNum (:71-72) */
typedef struct slio_lvx_params {
  int32_t device;
  int32_t max_points; /* capacity of each class: stored plus incoming points */
  float leaf_corner;  /* filter_parameter_corner: 0.2 (horizon, outdoor), 0.1 (mid) */
  float leaf_surf;    /* filter_parameter_surf: 0.4 / 0.2                            */
  int32_t reserved[4];
} slio_lvx_params;
int slio_lvx_params_default(slio_lvx_params* p);
/* EINVAL: max_points < 1, a leaf that is not positive and finite, no such
 * device.  No leaf can overflow the VoxelGrid's sort key: a voxel index stays
 * below 2^31 by PCL's own rule, under which a leaf too small for a cube's
 * extent passes that cube through unfiltered. */
int slio_lvx_create(slio_lvx_handle* out, const slio_lvx_params* p);
int slio_lvx_destroy(slio_lvx_handle m);
/* Empty both classes; laserCloudCenWidth / Height / Depth back to 10 / 5 / 10. */
int slio_lvx_clear(slio_lvx_handle m);
/* :475-776 at transformTobeMapped = transform: pointOnYAxis, the centre cube,
 * the six shift loops (the handle mirrors laserCloudCen*; several shifts in
 * one call compose as the reference's do, and each class's points are
 * relabelled and re-sorted on the device in one pass with one host wait; no
 * shift, no device work), then the cubes centre +- 2 in i, j, k order: every
 * one inside the array is a surround cube (laserCloudSurroundInd), those with
 * a corner inside the field of view (:727-761) are valid (laserCloudValidInd).
 * The handle keeps both lists for slio_lvx_update_map / slio_lvx_get_surround.
 * center[3] = centerCubeI / J / K after the shifts; valid / surround hold up to
 * 125 entries; any output may be NULL. */
int slio_lvx_select_cubes(slio_lvx_handle m, const float transform[6], int32_t center[3],
                          int32_t* valid, int32_t* nvalid, int32_t* surround, int32_t* nsurround);
/* :1159-1216 at transformTobeMapped = transform: every point of corner_xyz (the
 * raw laserCloudCornerLast) and of surf_xyz (laserCloudSurfLast_down) goes
 * through pointAssociateToMap (:195-217: yaw about z, roll about x, pitch
 * about y in float, then the translation), its cube index comes from the
 * double arithmetic of :1162-1168, and it is appended to that cube if the cube
 * is inside the array, valid or not.  Then every listed cube of both classes is
 * replaced by its VoxelGrid (leaf_corner / leaf_surf), each under
 * slio_scan_upload_voxel's semantics applied to that cube's cloud alone: its
 * own bounding box, min_b and div_b, the leaf-too-small pass-through, sums in
 * ascending input position, output in voxel-index order.  Every listed cube
 * is filtered on every call, whether it received a point or not, as the
 * reference does.  valid == NULL (nvalid 0): the list of the last
 * slio_lvx_select_cubes (ESTATE without one).  The scans are the only points
 * that cross PCIe; the host waits once per class (the new total and the 4852
 * offsets).  counts = the classes' new totals (may be NULL).  ECAPACITY when
 * stored + incoming points of a class exceed max_points. */
int slio_lvx_update_map(slio_lvx_handle m, const float transform[6], const float* corner_xyz,
                        int64_t n_corner, const float* surf_xyz, int64_t n_surf,
                        const int32_t* valid, int32_t nvalid, int64_t counts[2]);
/* laserCloud{Corner,Surf}Array[ind]->size() for ind = 0 .. 4850 (host table). */
int slio_lvx_cube_sizes(slio_lvx_handle m, int kind, int32_t sizes[SLIO_LVX_CUBES]);
/* laserCloud{Corner,Surf}Array[cube] to the host: *n points (n may be NULL);
 * xyz may be NULL (size only); ECAPACITY when cap < *n. */
int slio_lvx_get_cube(slio_lvx_handle m, int kind, int32_t cube, float* xyz, int64_t cap, int64_t* n);
/* laserCloudSurround2_corner (kind 0) / laserCloudSurround2 (kind 1), :1218-1224:
 * the concatenation of the listed cubes (at most 125) in list order, gathered
 * on the device and downloaded.  cubes == NULL (ncubes 0): the surround list
 * of the last slio_lvx_select_cubes (ESTATE without one). */
int slio_lvx_get_surround(slio_lvx_handle m, int kind, const int32_t* cubes, int32_t ncubes,
                          float* xyz, int64_t cap, int64_t* n);
/* laserCloudCenWidth / Height / Depth. */
int slio_lvx_get_centers(slio_lvx_handle m, int32_t cen[3]);
/* The two scans of a call (:351-369 and :789-798): corner_xyz = the raw
 * laserCloudCornerLast, kept as it is (the corner branch runs over it, :825);
 * surf_xyz = laserCloudSurfLast, which goes through downSizeFilterSurf
 * (leaf_surf, slio_scan_upload_voxel's semantics) on the device into
 * laserCloudSurfLast_down.  counts = {corner points, surf points after the
 * grid}.  One host wait (the grid's count) and one at the end, after which the
 * host clouds have been read.  ECAPACITY: a scan larger than max_points. */
int slio_lvx_feed_host(slio_lvx_handle m, const float* corner_xyz, int64_t n_corner,
                       const float* surf_xyz, int64_t n_surf, int64_t counts[2]);
/* The same feed, device to device, from the clouds the last slio_lreg_run of
 * `reg` (a slio_lreg_handle, slio_frontend.h) left in HBM: cornerPointsSharp is
 * the raw corner scan, surfPointsFlat goes through downSizeFilterSurf exactly
 * as above.  x, y, z only (the mapper stores no intensity); no point crosses
 * PCIe.  The upload is the only part the two feeds do not share, so equal
 * clouds give equal scans.  EINVAL: a registration handle that is null or
 * destroyed, or on another device; ESTATE: no run on it yet. */
int slio_lvx_feed_device(slio_lvx_handle m, void* reg, int64_t counts[2]);
/* The fed scan of a kind (kind 1: laserCloudSurfLast_down); xyz may be NULL. */
int slio_lvx_get_scan(slio_lvx_handle m, int kind, float* xyz, int64_t cap, int64_t* n);
/* :778-787 and the two setInputCloud of :816-817: laserCloud*FromMap = the valid
 * cubes of the last slio_lvx_select_cubes in laserCloudValidInd order, and over
 * each a search grid (cells of 1.25 m corner / 2.25 m surf, cell-sorted points,
 * offsets).  counts = the two maps' sizes.  One host wait per class (the map's
 * bounding box).  valid == NULL (nvalid 0): the list of the last
 * slio_lvx_select_cubes (ESTATE without one); ECAPACITY when the valid cubes
 * span more than 2^24 cells.  A map update or a new selection invalidates it. */
int slio_lvx_build_maps(slio_lvx_handle m, const int32_t* valid, int32_t nvalid, int64_t counts[2]);
/* One class's turn of the loop (:825-950 corner, kind 0; :954-1028 surf, kind 1)
 * at transformTobeMapped = transform, with its rows (:1059-1095) and their fp64
 * sums per workgroup, in ONE launch: pointAssociateToMap, the exact 5-NN / 8-NN
 * in the map (gate sqd[4] < 1.5 / sqd[7] < 5.0), the line through +- 0.1 of the
 * first eigenvector with D[0] > 3 D[1] (cv::eigen as slio_cvsolve.hpp restates
 * it) or the plane of slio_lvx_plane_solve with all eight neighbours within
 * 0.2, s > 0.1.  A failed plane solve leaves x = 0, the NaNs that follow
 * unselect the point.  nsel may be NULL (no wait then).  ESTATE: no map built
 * or no scan fed.
 * Departures: ties of the K-NN at equal float distance go to the lower
 * position in the cell-sorted map; the neighbour lists of points the gate
 * rejects are not produced (index -1, distance +inf). */
int slio_lvx_pass(slio_lvx_handle m, int kind, const float transform[6], int64_t* nsel);
/* What the last slio_lvx_pass of a kind left, n = that scan's size: world n x 3
 * (pointSel), nbr_idx / nbr_sqd n x 5 (kind 0) or n x 8 (kind 1) with indices
 * into laserCloud*FromMap, coeff n x 4, sel n.  Any output may be NULL. */
int slio_lvx_get_pass(slio_lvx_handle m, int kind, float* world, int32_t* nbr_idx, float* nbr_sqd,
                      float* coeff, uint8_t* sel);
/* A^T A / A^T B (:1099-1101) of the rows the last slio_lvx_pass of BOTH kinds
 * left: fp64 sums in k_lmap_coeff's fixed tree (slio_lmap_normal_equations),
 * corners before surfs, rounded to float.  One host wait. */
int slio_lvx_normal_equations(slio_lvx_handle m, float AtA[36], float AtB[6], int64_t* nsel);
/* :814-1151: only with more than 10 corner and more than 100 surf map points
 * (else *iterations = 0, transform untouched); at most 20 turns of pass(0),
 * pass(1), the normal equations (the turn's one host wait) and
 * slio_lvx_lm_step.  isDegenerate and matP persist across calls in the handle
 * as the node's globals do.  *iterations = num_temp. */
int slio_lvx_optimize(slio_lvx_handle m, float transform[6], int32_t* iterations,
                      int32_t* is_degenerate);
/* One call of the main loop, :475-1216: select_cubes at the handle's
 * transformTobeMapped (what the previous call left: transformAssociateToMap is
 * commented out at :472), build_maps, feed_host, optimize, transformUpdate
 * (:188-193, only when the loop ran), and the map update from the fed scans on
 * the device.  Host waits: 2 (maps) + 2 (feed) + 1 per turn + 2 (update), + 2
 * when the map shifts.  transform_aft_mapped and iterations may be NULL. */
int slio_lvx_process(slio_lvx_handle m, const float* corner_xyz, int64_t n_corner,
                     const float* surf_xyz, int64_t n_surf, float transform_aft_mapped[6],
                     int32_t* iterations);
/* From the sensor's cloud to a pose: slio_lreg_run(reg, xyzi, n) (scanRegistration's
 * laserCloudHandler, slio_frontend.h), then slio_lvx_process's body with
 * slio_lvx_feed_device in place of the host feed.  Only the raw cloud crosses
 * PCIe; host waits are those of slio_lvx_process plus one, the registration's
 * counts.  counts = {laserCloud, cornerPointsSharp, surfPointsFlat} sizes (may
 * be NULL).  Both handles on one device (EINVAL otherwise, before any device
 * call). */
int slio_lvx_process_cloud(slio_lvx_handle m, void* reg, const float* xyzi, int64_t n,
                           float transform_aft_mapped[6], int32_t* iterations, int32_t counts[3]);
/* transformTobeMapped / transformAftMapped / transformLastMapped; any may be NULL. */
int slio_lvx_get_transforms(slio_lvx_handle m, float tobe_mapped[6], float aft_mapped[6],
                            float last_mapped[6]);
/* Set transformTobeMapped (an initial guess from outside the node). */
int slio_lvx_set_transform(slio_lvx_handle m, const float tobe_mapped[6]);
/* -- host only, callable without a GPU -- */
/* int((t + 25.0) / 50.0) + cen, one less when t + 25.0 < 0 (:482-491,
 * :1162-1168).  EINVAL for a t that is not finite or beyond 1e6 m. */
int slio_lvx_cube_index(float t, int32_t cen, int32_t* cube);
/* slio_lvx_select_cubes without a handle: cen[3] (laserCloudCen*) in and out,
 * shift[3] = how many cubes the contents move along i, j, k (+1 per turn of a
 * `while (centerCube < 3)` loop, -1 per turn of the opposite one). */
int slio_lvx_select_host(const float transform[6], int32_t cen[3], int32_t center[3],
                         int32_t shift[3], int32_t* valid, int32_t* nvalid, int32_t* surround,
                         int32_t* nsurround);
/* The plane system of the surf branch (:962-975): cv::solve(DECOMP_QR) of
 * matA0 x = matB0 as slio_cvsolve.hpp restates it, nb_xyz = the 8 neighbours.
 * m = 10 is the reference's system (10 x 3, rows 8 and 9 zero, against ten
 * times -1); m = 8 leaves the zero rows out and gives the same bits: a zero row
 * adds +0 to every column norm and dot product of the Householder steps and the
 * back-substitution reads the top three rows only.  Returns 1 where the solve
 * gives up (x zeroed). */
int slio_lvx_plane_solve(const float* nb_xyz, int m, float x[3]);
/* The step after the normal equations (:1102-1150): slio_s2m_lm_step's body
 * with eignThre = 1 (:1114) and deltaR from the file's own double rad2deg
 * (:139).  Returns 1 (nothing done, *converged = 0) with fewer than 50 rows:
 * the reference's `continue` (:1040-1042), a turn that still counts. */
int slio_lvx_lm_step(const float AtA[36], const float AtB[6], int64_t nsel, int iter_count,
                     float transform[6], int* is_degenerate, float matP[36], int* converged);

/* Manifold helpers exported for tests (esekfom.hpp:59-73, 236-258). */
int slio_state_boxplus(const slio_state* x, const double dx[24], slio_state* out);
int slio_state_boxminus(const slio_state* x1, const slio_state* x2, double dx[24]);

/* ---- diagnostics ----------------------------------------------------------- */
/* Re-read the SLIO_NO_FUSE / SLIO_NO_FUSE0 / SLIO_NO_REDUCER / SLIO_PERSIST /
 * SLIO_NO_MFMA / SLIO_EVENT_WAIT / SLIO_NO_KNN_CERT switches of the update path
 * (read once at slio_create). */
int slio_debug_reload_switches(slio_handle h);
/* How the last slio_ikf_update_device ran: 1 one persistent launch for all
 * its passes (SLIO_PERSIST=1, single rank, fused configuration, every chunk's
 * workgroup resident at once), 0 a launch (or two) per pass. */
int slio_debug_update_path(slio_handle h);
/* Host clock stamps (CLOCK_MONOTONIC ns) of the last slio_ikf_update_device:
 * [0] entry, [1] state set up, [2] control block + information-form constants
 * ready (fused path), [3] first launch enqueued, [4] every launch enqueued,
 * [5] result seen, [6] return.  After slio_group_ikf_update, rank 0's handle
 * holds the group's: [0] entry, [1] every pass enqueued, [2] every rank's
 * result seen, [3] return, [4] / [5] / [6] host ns spent enqueueing the
 * ranks' pass launches / the reduce (events + in-device reduce, or the RCCL
 * group) / the filter steps.  out may be NULL; enable 1 / 0 turns stamping
 * on / off, -1 leaves it. */
int slio_debug_host_stamps(slio_handle h, int enable, int64_t out[8]);
/* kNN certificate counters (wrapping 32-bit; counting starts with the first
 * call, which turns it on for the handle -- it costs two same-address atomics
 * per workgroup):
 * out[0] queries whose 5 nearest a later pass certified from its earlier
 * search's 5 nearest and bound, out[1] queries searched in full in passes that write
 * certificates (device-resident passes after the first). */
int slio_debug_knn_cert(slio_handle h, uint32_t out[2]);
/* The device-side waits of the next updates on this handle (a fused pass's
 * reducer workgroup waiting for the launch's segment rows; a persistent
 * update's workgroups waiting for the pass flag; on a group's rank 0, every
 * rank's gate between fused group passes) give up after `ticks` 100 MHz
 * clock ticks instead of 1 s (0 restores 1 s).  A test hook: 1 forces the
 * give-up path (SLIO_ETIMEOUT, counters reset). */
int slio_debug_wait_limit(slio_handle h, int64_t ticks);

#ifdef __cplusplus
}
#endif

#endif /* SLIO_H */
