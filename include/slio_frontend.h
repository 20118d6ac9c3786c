/* slio_frontend.h -- C-ABI of the MI355X front-end:
 * LIO-SAM ImageProjection::projectPointCloud + cloudExtraction and
 * FeatureExtraction::calculateSmoothness + markOccludedPoints +
 * extractFeatures (incl. the per-ring pcl::VoxelGrid) as HIP kernels on gfx950.
 *
 * Reference seams (class members operating on class-owned arrays):
 *   ImageProjection::cloudHandler      LIO-SAM/src/imageProjection.cpp:193-212
 *     projectPointCloud :610-650, deskewPoint :565-604, findRotation :492-529,
 *     cloudExtraction :656-678 -> cloud_info.msg (startRingIndex, endRingIndex,
 *     pointColInd, pointRange, cloud_deskewed)
 *   FeatureExtraction::laserCloudInfoHandler  LIO-SAM/src/featureExtraction.cpp:88-100
 *     calculateSmoothness :108-131, markOccludedPoints :137-177,
 *     extractFeatures :183-296 -> cloud_corner, cloud_surface
 * The IMU queue handling (imuDeskewInfo :345-392) stays on the host: it hands
 * the integrated rotation table to slio_lio_set_deskew.
 *
 * Conventions as in slio.h: opaque handle, plain host pointers, int status
 * (SLIO_OK = 0, negative on error, message via slio_last_error()); points are
 * SoA float32; xyzi outputs are interleaved float32 (x, y, z, intensity).
 */
#ifndef SLIO_FRONTEND_H
#define SLIO_FRONTEND_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct slio_lio* slio_lio_handle;

typedef struct slio_lio_params {
  int32_t device;          /* HIP device ordinal                                   */
  int32_t n_scan;          /* N_SCAN (params.yaml:27, default 16)                  */
  int32_t horizon_scan;    /* Horizon_SCAN (params.yaml:28, default 1800)          */
  int32_t downsample_rate; /* downsampleRate (params.yaml:29, default 1)           */
  float lidar_min_range;   /* lidarMinRange (params.yaml:30, default 1.0)          */
  float lidar_max_range;   /* lidarMaxRange (params.yaml:31, default 1000.0)       */
  float edge_threshold;    /* edgeThreshold (params.yaml:57, default 1.0)          */
  float surf_threshold;    /* surfThreshold (params.yaml:58, default 0.1)          */
  float surf_leaf_size;    /* odometrySurfLeafSize (params.yaml:63, default 0.4)   */
  int32_t max_points;      /* input capacity (0 -> n_scan * horizon_scan)          */
  int32_t reserved[4];
} slio_lio_params;

typedef struct slio_lio_counts {
  int64_t n_extracted; /* points in cloud_deskewed / pointColInd / pointRange       */
  int64_t n_corner;    /* cloud_corner                                             */
  int64_t n_surface;   /* cloud_surface (after the per-ring VoxelGrid)            */
} slio_lio_counts;

/* params.yaml defaults (VLP-16: 16 x 1800). */
int slio_lio_params_default(slio_lio_params* p);
int slio_lio_create(slio_lio_handle* out, const slio_lio_params* p);
int slio_lio_destroy(slio_lio_handle h);
/* Enqueue on a caller stream (hipStream_t); NULL -> the handle's own stream. */
int slio_lio_set_stream(slio_lio_handle h, void* stream);

/* Deskew table of imuDeskewInfo (imageProjection.cpp:345-392): n_imu =
 * imuPointerCur + 1 entries of imuTime / imuRotX / imuRotY / imuRotZ (n_imu <=
 * 2000 = queueLength) and timeScanCur.  enabled = (deskewFlag == 1 &&
 * cloudInfo.imuAvailable); 0 leaves points as they are (deskewPoint :566). */
int slio_lio_set_deskew(slio_lio_handle h, const double* imu_time, const double* rot_x,
                        const double* rot_y, const double* rot_z, int32_t n_imu,
                        double time_scan_cur, int32_t enabled);

/* laserCloudIn (VelodynePointXYZIRT, imageProjection.cpp:4-15): x, y, z,
 * intensity, ring, time (s after timeScanCur; Ouster: t * 1e-9f, :244-258). */
int slio_lio_upload(slio_lio_handle h, const float* x, const float* y, const float* z,
                    const float* intensity, const uint16_t* ring, const float* time, int64_t n);

/* The whole front-end for the uploaded scan, enqueued on the stream. */
int slio_lio_run_async(slio_lio_handle h);
/* slio_lio_run_async + wait; counts may be NULL. */
int slio_lio_run(slio_lio_handle h, slio_lio_counts* counts);
int slio_lio_get_counts(slio_lio_handle h, slio_lio_counts* counts);

/* Kernel timing: enable != 0 times every feature stage (k_fe_pick start to
 * k_fe_voxel end, the dominant part; start/stop hipEvents carried in the
 * dispatch packets) and
 * accumulates device milliseconds; 0 disables.  SLIO_LIO_PROFILE_KEEP keeps
 * the totals (pause / resume).  Read: accumulated ms and launch count
 * (synchronises the stream). */
#define SLIO_LIO_PROFILE_KEEP 16
/* enable | SLIO_LIO_PROFILE_SCAN: time every whole scan instead (the first
 * launch's start to the last launch's end: all the front-end's kernels). */
#define SLIO_LIO_PROFILE_SCAN 32
int slio_lio_profile(slio_lio_handle h, int enable);
int slio_lio_profile_read(slio_lio_handle h, double* ms, int64_t* launches);

/* rangeMat (n_scan * horizon_scan, FLT_MAX = empty, :146) and, per cell, the
 * index of the input point that filled it (-1 = empty). Either may be NULL. */
int slio_lio_get_range_image(slio_lio_handle h, float* range_mat, int32_t* cell_point);
/* cloud_info: startRingIndex / endRingIndex [n_scan], pointColInd /
 * pointRange [n_extracted], cloud_deskewed xyzi [n_extracted * 4].  Any may be NULL. */
int slio_lio_get_cloud_info(slio_lio_handle h, int32_t* start_ring, int32_t* end_ring,
                            int32_t* col_ind, float* point_range, float* xyzi);
/* Per extracted point: cloudCurvature, cloudNeighborPicked after
 * markOccludedPoints, final cloudLabel (1 corner, -1 flat, 0 other).  Any may be NULL. */
int slio_lio_get_features(slio_lio_handle h, float* curvature, uint8_t* picked, int32_t* label);
/* cloud_corner [n_corner * 4], cloud_surface [n_surface * 4].  Either may be NULL. */
int slio_lio_get_clouds(slio_lio_handle h, float* corner_xyzi, float* surface_xyzi);

/* ======================================================================
 * LeGO-LOAM
 *   ImageProjection::cloudHandler  LeGO-LOAM/src/imageProjection.cpp:151-158
 *     findStartEndAngle :160-175, projectPointCloud :177-213 (the LAST point
 *     wins a cell), groundRemoval :216-262, cloudSegmentation :268-330 +
 *     labelComponents :332-393 -> cloud_info.msg + segmented / outlier clouds
 *   FeatureAssociation::runFeatureAssociation (front half)
 *     featureAssociation.cpp: adjustDistortion :617-805, calculateSmoothness
 *     :807-834, markOccludedPoints :838-876, extractFeatures :883-1007
 * The IMU ring buffer (imuHandler / AccumulateIMUShiftAndRotation :430-588)
 * is host state handed over with slio_lego_set_imu.
 * ====================================================================== */
typedef struct slio_lego* slio_lego_handle;

typedef struct slio_lego_params {
  int32_t device;
  int32_t n_scan;                  /* N_SCAN (utility.h:20, 16)                */
  int32_t horizon_scan;            /* Horizon_SCAN (1800)                      */
  int32_t ground_scan_ind;         /* groundScanInd (7)                        */
  int32_t segment_valid_point_num; /* segmentValidPointNum (5)                 */
  int32_t segment_valid_line_num;  /* segmentValidLineNum (3)                  */
  float ang_res_x;                 /* 0.2 deg                                  */
  float ang_res_y;                 /* 2.0 deg                                  */
  float ang_bottom;                /* 15.0 + 0.1 deg                           */
  float sensor_mount_angle;        /* 0 deg                                    */
  float segment_theta;             /* 1.0472 rad (60 deg)                      */
  float edge_threshold;            /* 0.1                                      */
  float surf_threshold;            /* 0.1                                      */
  float leaf_size;                 /* less-flat VoxelGrid leaf (0.2, :222)     */
  float scan_period;               /* 0.1 s                                    */
  int32_t max_points;              /* input capacity (0 -> 4 * cells)          */
  int32_t reserved[4];
} slio_lego_params;

/* FeatureAssociation IMU state read by adjustDistortion: the que_len-entry
 * ring buffer (imuTime double, the rest float), imuPointerLast (-1: no IMU),
 * imuPointerLastIteration, timeScanCur and imuAngularRotation{X,Y,Z}Last. */
typedef struct slio_lego_imu {
  const double* time;
  const float *roll, *pitch, *yaw;
  const float *velo_x, *velo_y, *velo_z;
  const float *shift_x, *shift_y, *shift_z;
  const float *ang_x, *ang_y, *ang_z; /* imuAngularRotation{X,Y,Z} */
  int32_t pointer_last, pointer_last_iteration, que_len;
  double time_scan_cur;
  float ang_last[3];
} slio_lego_imu;

/* State adjustDistortion leaves for the back half (updateInitialGuess
 * :1999-2029): imu{Roll,Pitch,Yaw}Start, imu{Roll,Pitch,Yaw}Cur of the last
 * point, imuVeloFromStart{X,Y,Z}Cur of the last point, imuAngularFromStart,
 * the new imuAngularRotation*Last and imuPointerLastIteration. */
typedef struct slio_lego_imu_out {
  float rpy_start[3], rpy_cur[3], velo_from_start[3], angular_from_start[3], ang_last[3];
  int32_t pointer_last_iteration;
} slio_lego_imu_out;

typedef struct slio_lego_counts {
  int64_t n_segmented, n_outlier, n_sharp, n_less_sharp, n_flat, n_less_flat;
  float orientation[3]; /* startOrientation, endOrientation, orientationDiff */
} slio_lego_counts;

int slio_lego_params_default(slio_lego_params* p);
int slio_lego_create(slio_lego_handle* out, const slio_lego_params* p);
int slio_lego_destroy(slio_lego_handle h);
int slio_lego_set_stream(slio_lego_handle h, void* stream);
/* IMU state for the next run; NULL or pointer_last < 0 -> no IMU correction. */
int slio_lego_set_imu(slio_lego_handle h, const slio_lego_imu* imu);
/* laserCloudIn x, y, z (PointXYZI order of the driver); findStartEndAngle runs here. */
int slio_lego_upload(slio_lego_handle h, const float* x, const float* y, const float* z, int64_t n);
int slio_lego_run_async(slio_lego_handle h);
int slio_lego_run(slio_lego_handle h, slio_lego_counts* counts);
/* Waits for the sweep.  SLIO_ETIMEOUT: the row stage's wait for an earlier
 * ring gave up (~0.5 s; the sweep's outputs are void, the next sweep is not
 * affected). */
int slio_lego_get_counts(slio_lego_handle h, slio_lego_counts* counts);
/* rangeMat, the input index that filled each cell (-1 empty), groundMat, labelMat. */
int slio_lego_get_image(slio_lego_handle h, float* range_mat, int32_t* cell_point, int8_t* ground,
                        int32_t* label);
/* cloud_info (startRingIndex, endRingIndex, segmentedCloudGroundFlag,
 * segmentedCloudColInd, segmentedCloudRange), segmented cloud xyzi (as
 * imageProjection publishes it) and outlier cloud xyzi.  Any may be NULL. */
int slio_lego_get_seg_info(slio_lego_handle h, int32_t* start_ring, int32_t* end_ring,
                           uint8_t* ground_flag, int32_t* col_ind, float* range, float* seg_xyzi,
                           float* outlier_xyzi);
/* After adjustDistortion: the segmented cloud in the LOAM frame (x, y, z,
 * ring + scanPeriod * relTime), cloudCurvature, cloudNeighborPicked after
 * markOccludedPoints, cloudLabel (2 sharp, 1 less sharp, -1 flat, 0), IMU state. */
int slio_lego_get_features(slio_lego_handle h, float* deskewed, float* curvature, uint8_t* picked,
                           int32_t* label, slio_lego_imu_out* imu_out);
/* cornerPointsSharp, cornerPointsLessSharp, surfPointsFlat, surfPointsLessFlat. */
int slio_lego_get_clouds(slio_lego_handle h, float* sharp, float* less_sharp, float* flat,
                         float* less_flat);
/* Timing of the feature kernels (or, with SLIO_LIO_PROFILE_SCAN, of the
 * whole sweep), as slio_lio_profile. */
int slio_lego_profile(slio_lego_handle h, int enable);
int slio_lego_profile_read(slio_lego_handle h, double* ms, int64_t* launches);

/* ----------------------------------------------------------------------
 * LeGO-LOAM scan-to-scan odometry: the back half of
 * FeatureAssociation::runFeatureAssociation (featureAssociation.cpp
 * :2232-2248), which produces /laser_odom_to_init.  The Gauss-Newton loop of
 * updateTransformation runs in one launch, without a host round trip between
 * iterations; per sweep the host reads one slio_lego_odom_out.
 *
 * Stated departures from the reference:
 *  - the 1-NN (kdtree nearestKSearch, k = 1) is exact and ties go to the
 *    lower index; FLANN's order among equal distances is unpinned;
 *  - the forward neighbour scan is bounded by the CURRENT feature count
 *    (j < cornerPointsSharpNum / surfPointsFlatNum, :1316 / :1448) as the
 *    reference writes it, and additionally by the last cloud's size, where
 *    the reference would read past the cloud's end;
 *  - sin / cos / asin / atan2 / sqrt of a float are the double function
 *    rounded to float;
 *  - the searches always run on the new last clouds.  The reference re-seats
 *    its kd-trees only when the swapped clouds hold MORE than 10 / 100 points
 *    (:2169) while updateTransformation returns early only BELOW 10 / 100
 *    (:2037), so at exactly 10 corner or 100 surf points it searches the
 *    trees of the sweep before.
 * The neighbour scans are evaluated in parallel, which relies on
 * int(intensity) (the ring) not decreasing with the index in the last
 * clouds; every cloud the handle produces itself has that order.
 * When the IMU is absent adjustDistortion's outputs read as 0 (the handle
 * does not keep an earlier sweep's imu*Start as the reference's members do).
 * ---------------------------------------------------------------------- */
#define SLIO_LEGO_ODOM_SURF 0   /* findCorrespondingSurfFeatures + calculateTransformationSurf     */
#define SLIO_LEGO_ODOM_CORNER 1 /* findCorrespondingCornerFeatures + calculateTransformationCorner */

typedef struct slio_lego_odom_params {
  float nearest_feature_sq_dist; /* nearestFeatureSearchSqDist (utility.h:89, 25)          */
  int32_t max_iterations;        /* the 25 of updateTransformation :2039 / :2053 (<= 64)   */
  int32_t search_period;         /* the 5 of iterCount % 5 == 0 (:1303 / :1426)            */
  int32_t skip_frame_num;        /* skipFrameNum (:30, 1)                                  */
  float scan_period;             /* scanPeriod (utility.h:28, 0.1)                         */
  int32_t reserved[3];
} slio_lego_odom_params;

typedef struct slio_lego_odom_out {
  float transform_cur[6], transform_sum[6];
  int32_t inited;          /* 0: this call was checkSystemInitialization (:1964-1997)      */
  int32_t iters[2];        /* iterations executed (surf, corner); 0 on the early return    */
  int32_t rows[2];         /* rows selected at the last executed iteration                 */
  int32_t degenerate[2];   /* isDegenerate of each loop's iteration 0 (0 if no step there) */
  int32_t n_corner_last, n_surf_last; /* after the swap                                    */
  int32_t published;       /* the frameCount >= skipFrameNum + 1 gate (:2176)              */
  int32_t n_outlier_last;  /* points of the outlier cloud last published                   */
  int32_t reserved;
} slio_lego_odom_out;

/* Every member variable the back half carries between sweeps. */
typedef struct slio_lego_odom_state {
  float transform_cur[6], transform_sum[6];
  float imu_last[3];            /* imuRollLast, imuPitchLast, imuYawLast                    */
  float imu_shift_from_start[3]; /* stays 0: this reference never calls ShiftToStartIMU     */
  float imu_velo_from_start[3];
  float mat_p[9];
  int32_t system_inited, is_degenerate, frame_count, n_corner_last, n_surf_last;
  int32_t reserved[3];
} slio_lego_odom_state;

int slio_lego_odom_params_default(slio_lego_odom_params* p);
/* Allocates the odometry state (the "last" clouds double-buffered against
 * the less-sharp / less-flat clouds, transformCur / transformSum, the
 * correspondence indices).  Without it the handle behaves as before. */
int slio_lego_odom_enable(slio_lego_handle h, const slio_lego_odom_params* params);
/* Back to the constructor's state (:318-354: systemInitedLM = false,
 * transforms 0, frameCount = skipFrameNum, so that the first sweep after
 * checkSystemInitialization publishes). */
int slio_lego_odom_reset(slio_lego_handle h);
/* runFeatureAssociation :2232-2248 for the sweep last run, enqueued on the
 * stream: checkSystemInitialization on the first sweep; afterwards
 * updateInitialGuess, updateTransformation, integrateTransformation and
 * publishCloudsLast (TransformToEnd, the pointer swap, adjustOutlierCloud).
 * SLIO_ESTATE without a sweep (or slio_lego_odom_set_clouds) since the last
 * call.  After it the handle's less-sharp / less-flat buffers hold the
 * previous "last" clouds, as the reference's swapped Ptrs do. */
int slio_lego_odom_run_async(slio_lego_handle h);
/* slio_lego_odom_run_async + wait + the result; out may be NULL. */
int slio_lego_odom_run(slio_lego_handle h, slio_lego_odom_out* out);
/* What publishCloudsLast publishes: laserCloudCornerLast [n_corner_last * 4],
 * laserCloudSurfLast [n_surf_last * 4] (both current after every sweep) and
 * the axis-permuted outlier cloud of the last publishing sweep
 * [n_outlier_last * 4].  Any may be NULL. */
int slio_lego_odom_get_last(slio_lego_handle h, float* corner_xyzi, float* surf_xyzi, float* outlier_xyzi);

/* Device views of the same three clouds (float4 xyzi) for a consumer on the
 * device (slio_lmap_feed_lego, slio.h): waits for the handle's stream, so the
 * clouds are complete when it returns; they stay valid until the next sweep
 * or odometry call on this handle.  published = the last odometry call's gate
 * (the outlier cloud is current only then). */
typedef struct slio_lego_last_view {
  const float* corner_xyzi;
  const float* surf_xyzi;
  const float* outlier_xyzi;
  int32_t n_corner, n_surf, n_outlier;
  int32_t published;
  int32_t device;
  int32_t reserved;
} slio_lego_last_view;
int slio_lego_odom_last_view(slio_lego_handle h, slio_lego_last_view* view);

/* Lockstep / test entries: the same kernels and the same step code, one host
 * wait per call. */
/* Replaces cornerPointsSharp, surfPointsFlat and the two last clouds (xyzi)
 * and sets systemInitedLM; the less clouds become empty.  SLIO_EINVAL for a
 * last cloud whose int(intensity) decreases with the index. */
int slio_lego_odom_set_clouds(slio_lego_handle h, const float* sharp, int32_t n_sharp, const float* flat,
                              int32_t n_flat, const float* corner_last, int32_t n_corner_last,
                              const float* surf_last, int32_t n_surf_last);
int slio_lego_odom_set_state(slio_lego_handle h, const slio_lego_odom_state* s);
int slio_lego_odom_get_state(slio_lego_handle h, slio_lego_odom_state* s);
/* One findCorresponding{Surf,Corner}Features(iter_count) pass at
 * transform_cur plus the Jacobian rows and normal equations of
 * calculateTransformation{Surf,Corner} (:1593-1648 / :1726-1762).  n is the
 * kind's query count.  ind[3n] = pointSearch*Ind1 / Ind2 / Ind3 per query
 * (Ind3 = -1 for corners; refreshed when iter_count % search_period == 0,
 * else the ones cached by the kind's last refreshing pass -- each kind keeps
 * its own, -1 before the first), coeff[4n] = s * (a, b, c, d) (0 where not
 * selected), sel[n], AtA[9] / AtB[3]: fp64 sums rounded to float, in the
 * fixed order of DESIGN.md §3.12.  Any output may be NULL. */
int slio_lego_odom_pass(slio_lego_handle h, int kind, int iter_count, const float transform_cur[6],
                        int32_t* ind, float* coeff, uint8_t* sel, float AtA[9], float AtB[3], int32_t* nsel);
/* Host export of the in-kernel step (:1649-1695 / :1764-1814).  Returns 1
 * without a step when nsel < 10 (the loop's `continue`).  keep_going = the
 * reference function's bool (0: converged, the loop breaks).  A singular AtA
 * gives a zero step, which counts as converged (as slio_s2m_lm_step). */
int slio_lego_odom_step(int kind, const float AtA[9], const float AtB[3], int32_t nsel, int iter_count,
                        float transform_cur[6], int* is_degenerate, float matP[9], int* keep_going);

/* ======================================================================
 * livox_mapping scanRegistration (src/livox_mapping/src/scanRegistration.cpp;
 * every path:line below is in that file): laserCloudHandler :152-534 on the
 * device.  One opaque handle owns the buffers of one device and one stream.
 * Input: n x {x, y, z, intensity} float32 in the message's order.  A run is
 *   prepare   :157-194  the first min(n, 32000) points, the finite ones in
 *                       order, intensity = scanID + intensity / 10000
 *   loop 1    :212-325  the strided pass (i += 4 where right_curvature < 0.01,
 *                       else 1): flat points (1), surf-surf corners (150)
 *   loop 2    :327-483  per point: outliers (250), break points (100), the
 *                       break-point select (a point that fails goes to 0)
 *   collect   :486-508  flag 1 -> surfPointsFlat, 100 / 150 ->
 *                       cornerPointsSharp, in index order
 * as a fixed number of launches (six, whatever n) and ONE host wait, the copy
 * of the three counts.  The three clouds stay on the device
 * (slio_lvx_feed_device, slio.h) until the next run.
 *
 * Stated departures from the reference:
 *  - atan2 of two floats is the double function rounded to float (the
 *    library's convention); where the device's double atan2 differs from the
 *    host's in the last place AND the rounding to float does not hide it, the
 *    scan id of a point within that distance of a multiple of 9 degrees may
 *    differ.  The intensity is the only output it reaches;
 *  - dis, dis2 and theta2 (:172-176, :488-493) are dead and not computed; the
 *    scan id of a point that is dropped is not evaluated;
 *  - Eigen's normalize() is 3.3's, which leaves a zero vector as it is.
 * Errors as in slio.h; argument errors are reported before any device call.
 * ====================================================================== */
typedef struct slio_lreg* slio_lreg_handle;

typedef struct slio_lreg_params {
  int32_t device;
  int32_t max_points; /* input capacity, 1 .. 32000 = CloudFeatureFlag's size (:53) */
  int32_t reserved[6];
} slio_lreg_params;

/* device 0, max_points 32000 (:53, :158). */
int slio_lreg_params_default(slio_lreg_params* p);
/* EINVAL: max_points outside 1 .. 32000, no such device. */
int slio_lreg_create(slio_lreg_handle* out, const slio_lreg_params* p);
int slio_lreg_destroy(slio_lreg_handle h);
/* laserCloudHandler (:152-534) on xyzi[n * 4].  Points past max_points are
 * not read (:158).  counts = {laserCloud, cornerPointsSharp, surfPointsFlat}
 * sizes.  EINVAL: n < 0, null cloud with n > 0, null counts. */
int slio_lreg_run(slio_lreg_handle h, const float* xyzi, int64_t n, int32_t counts[3]);
/* laserCloud (:189-190, :518) of the last run: counts[0] x 4.  ESTATE without
 * a run; ECAPACITY when cap < counts[0]. */
int slio_lreg_get_cloud(slio_lreg_handle h, float* xyzi, int64_t cap);
/* kind 0: cornerPointsSharp (:505-507), kind 1: surfPointsFlat (:500-503). */
int slio_lreg_get_features(slio_lreg_handle h, int kind, float* xyzi, int64_t cap);
/* For tests: CloudFeatureFlag[0 .. counts[0]) after loop 2 and, per point, 1
 * where loop 1 (:212) visited it.  Either may be NULL. */
int slio_lreg_get_flags(slio_lreg_handle h, int32_t* flags, uint8_t* visited);
/* The shape of the kernel that resolves loop 1's chain: thread t owns the
 * loop positions [5 + t * per_thread, 5 + (t + 1) * per_thread), one workgroup
 * owns per_workgroup of them (all 32000: there is no seam between workgroups). */
int slio_lreg_chain_tile(int32_t* per_thread, int32_t* per_workgroup);
/* -- host only, callable without a GPU -- */
/* The whole handler as its literal serial loops.  Outputs sized for min(n,
 * 32000) points; any of flags, visited, cloud, corner, surf, stats may be
 * NULL.  stats[12] = visits with stride 1, with stride 4, flag[i-2] = 1
 * writes (:242), flag[i+2] = 1 writes (:272), 150 set (:322), outliers (:358),
 * break test entered left (:366) / right (:405), 100 set (:449), 100 kept
 * (:475), 100 reset (:478), resets that erased a flag of loop 1. */
int slio_lreg_classify_host(const float* xyzi, int64_t n, int32_t* flags, uint8_t* visited, float* cloud,
                            float* corner, float* surf, int32_t counts[3], int32_t* stats);
/* plane_judge (:64-120) on xyz[num * 3], 1 <= num <= 64. */
int slio_lreg_plane_judge(const float* xyz, int32_t num, int32_t threshold, int32_t* is_plane);

/* ======================================================================
 * A-LOAM scanRegistration (src/A-LOAM/src/scanRegistration.cpp; every
 * path:line below is in that file): laserCloudHandler :124-432 on the device
 * for the 16-, 32- and 64-line layouts.  One opaque handle owns the buffers of
 * one device and one stream.  Input: n x {x, y, z} float32 in the message's
 * order.  A run is
 *   filters    :145-148  non-finite points and points nearer than
 *                        minimum_range dropped, order kept
 *   scan id    :155-239  startOri / endOri from the first and last survivor,
 *                        the scan id from the elevation, the two orientation
 *                        branches, intensity = scanID + scanPeriod * relTime
 *   bucketing  :246-250  laserCloud = the scans concatenated, stable
 *   curvature  :254-278  the 11-tap stencil over the concatenated cloud
 *   picks      :289-422  per scan, six sectors: 2 sharp, up to 20 less sharp,
 *                        up to 4 flat, +-5 neighbour marks up to a 0.05 gap
 *   VoxelGrid  :424-431  one per scan over its less-flat points, leaf 0.2
 * as seven launches, whatever n, on one stream and ONE host wait, the copy of
 * the five counts.  The five clouds stay on the device (slio_aloam_get_view)
 * until the next run.  halfPassed (:166) is no serial dependency: until it is
 * set every kept point is evaluated in the first branch, so the switch point
 * is the first kept point whose first-branch `ori - startOri > M_PI`, a
 * min-reduction; points up to and including it use the first branch.
 *
 * Stated departures from the reference:
 *  - std::sort (:304) orders equal curvatures as introsort leaves them; here
 *    the sort is stable, ties by position;
 *  - atan2 of two floats is the double function rounded to float (the
 *    library's convention); atan(z / sqrt(..)) (:177) is the double function
 *    of the float quotient, `* 180 / M_PI` in double, rounded to float on
 *    assignment.  Which overload the reference's unqualified atan binds to
 *    depends on its headers; the scan id differs only for a point whose
 *    pre-truncation scan value lies within rounding of an integer;
 *  - an input with no survivor gives five empty clouds (the reference reads
 *    points[0] of an empty cloud, :155);
 *  - a NaN elevation (a point at the origin with minimum_range 0) is dropped;
 *    non-finite curvature (coordinates near float overflow) is outside the
 *    contract: it sorts by its bit pattern and faults nothing;
 *  - inside a voxel the points are summed in list order (as the LeGO
 *    front-end's per-ring VoxelGrid, slio_lio_*);
 *  - PUB_EACH_LINE (:469-477) and systemDelay (:61, 0) are not restated.
 * Errors as in slio.h; argument errors are reported before any device call.
 * ====================================================================== */
typedef struct slio_aloam* slio_aloam_handle;

typedef struct slio_aloam_params {
  int32_t device;
  int32_t n_scans;    /* 16, 32 or 64 (scan_line, :487) */
  int32_t max_points; /* input capacity, 1 .. 400000 = cloudCurvature's size (:65-68) */
  int32_t reserved0;
  double minimum_range; /* 0.1 (:82); compared as a float (:93, :148) */
  double scan_period;   /* 0.1 (:59) */
  int32_t reserved[4];
} slio_aloam_params;

/* The device-resident result of the last run: device pointers to the five
 * clouds (n x {x, y, z, intensity}) in the order laserCloud, cornerPointsSharp,
 * cornerPointsLessSharp, surfPointsFlat, surfPointsLessFlat (:437-465), valid
 * until the next run or destroy. */
typedef struct slio_aloam_view {
  const float* cloud[5];
  int32_t count[5];
  int32_t device;
} slio_aloam_view;

/* device 0, n_scans 16, max_points 400000, minimum_range 0.1, scan_period 0.1. */
int slio_aloam_params_default(slio_aloam_params* p);
/* EINVAL: n_scans not 16 / 32 / 64, max_points outside 1 .. 400000, negative
 * device (before any device call), no such device. */
int slio_aloam_create(slio_aloam_handle* out, const slio_aloam_params* p);
int slio_aloam_destroy(slio_aloam_handle h);
/* laserCloudHandler (:124-432) on xyz[n * 3].  counts = sizes of the five
 * clouds in the view's order.  EINVAL: n < 0, null cloud with n > 0, null
 * counts; ECAPACITY: n > max_points. */
int slio_aloam_run(slio_aloam_handle h, const float* xyz, int64_t n, int32_t counts[5]);
/* Cloud `kind` (0 .. 4, the view's order) of the last run: counts[kind] x 4.
 * ESTATE without a run; ECAPACITY when cap < counts[kind]. */
int slio_aloam_get_cloud(slio_aloam_handle h, int kind, float* xyzi, int64_t cap);
/* scanStartInd / scanEndInd (:246-250), n_scans entries each. */
int slio_aloam_get_scan_index(slio_aloam_handle h, int32_t* start, int32_t* end);
/* For tests: cloudCurvature, cloudLabel, cloudNeighborPicked over [0,
 * counts[0]) (:274-277; 0 where the reference's loop does not write).  Any
 * may be NULL. */
int slio_aloam_get_work(slio_aloam_handle h, float* curvature, int32_t* label, uint8_t* picked);
/* The device view of the last run; waits for the handle's stream. */
int slio_aloam_get_view(slio_aloam_handle h, slio_aloam_view* v);
/* The kernels' shape: points per workgroup of the per-point passes, and the
 * longest list (a sector, or a scan's less-flat list) the LDS sort takes in
 * one piece; a longer one is sorted in pieces and merged in global memory. */
int slio_aloam_tile(int32_t* block, int32_t* sort_cap);
/* -- host only, callable without a GPU -- */
/* The whole handler as its literal serial loops (p->device is not read).
 * Clouds sized for n points, scan_start / scan_end for n_scans entries,
 * curvature / label / picked for n; any output but counts may be NULL.
 * stats[18] = points dropped as non-finite, by range (:102), by scan id
 * (:184, :190, :201), of those by `scanID > 50` alone; endOri -= 2 pi (:160),
 * += 2 pi (:162); first branch += 2 pi (:216), -= 2 pi (:218); second branch
 * += 2 pi (:228), -= 2 pi (:230); halfPassed set (:222); scans skipped
 * (:291); 21st-candidate breaks (:332); flat points (:377); 4th-flat breaks
 * (:383); marks written outside the sector of their pick; candidates that
 * pass the curvature test but carry a mark of another sector; scans whose
 * VoxelGrid takes PCL's overflow branch. */
int slio_aloam_register_host(const slio_aloam_params* p, const float* xyz, int64_t n, float* laser_cloud,
                             float* corner_sharp, float* corner_less_sharp, float* surf_flat,
                             float* surf_less_flat, int32_t* scan_start, int32_t* scan_end, float* curvature,
                             int32_t* label, uint8_t* picked, int32_t counts[5], int32_t* stats);

/* ======================================================================
 * A-LOAM laserOdometry (src/A-LOAM/src/laserOdometry.cpp; every path:line
 * below is in that file unless said otherwise): the node's loop body :304-695
 * on the device, from the four feature clouds of one sweep to
 * /laser_odom_to_init.  DISTORTION is 0 as compiled (:52): s = 1, and
 * Identity.slerp(1, q) rotates as q.  A sweep is
 *   first sweep   :307-309  systemInited only
 *   two passes    :317-593  each one association at the current para_q /
 *                           para_t, then one solve:
 *     TransformToStart :105-126  q * p + t in double, rounded to float
 *     1-NN             :345, :457  exact, over the whole last cloud, gate < 25
 *     second / third   :361-418, :476-539  the ring-bounded scans, as index
 *                           ranges of the table ring_start[65]
 *     factors          lidarFactor.hpp:12-125 with analytic Jacobians in the
 *                           tangent [d theta (3), d t (3)], HuberLoss(0.1)
 *     solve            :586-591  this library's own Levenberg-Marquardt in
 *                           the shape of Ceres' trust-region defaults, at most
 *                           4 iterations
 *   integration   :600-601  t_w_curr += q_w_curr * t_last_curr, then q_w_curr
 *                           *= q_last_curr, unnormalised
 *   swap and gate :650-695  the two less clouds become the last clouds;
 *                           published = (frameCount % skipFrameNum == 0)
 * as at most six launches on the handle's stream and ONE host wait, for the
 * result.  Quaternions are (x, y, z, w), as para_q (:55).
 *
 * Stated departures from the reference:
 *  - the solve is not Ceres: parity with Ceres' own iterates is unpinned.
 *    Every constant of the solve is in csrc/slio_aloam_odom.hpp; the
 *    retraction is q' = normalize((d theta / 2, 1)) * q, so everything from
 *    the association to the pose is + - * / sqrt in IEEE double and the
 *    device, the host restatement and a numpy model agree to the bit;
 *  - the 1-NN is exact with ties to the lower index (FLANN's order among
 *    equal distances is unpinned);
 *  - scan ids (int(intensity)) of the two less clouds must be non-decreasing
 *    in the index and inside [0, 64): EINVAL otherwise, with no change of the
 *    handle's state.  It holds for the clouds of slio_aloam_*;
 *  - an empty last cloud gives no factor (the reference reads a stale
 *    pointSearchSqDis[0]);
 *  - a factor with coincident edge points or a non-finite plane normal is
 *    dropped and counted as degenerate (the reference divides by zero);
 *  - the sums run over factor slots in query order (sharp, then flat), 32
 *    strided partials per entry in ascending slot, then ascending lane;
 *  - the `if (0)` block (:630-648), the publishers and the path message are
 *    not restated.
 * ====================================================================== */
typedef struct slio_aloam_odom* slio_aloam_odom_handle;

typedef struct slio_aloam_odom_params {
  int32_t device;
  int32_t n_scans;        /* 1 .. 64: sharp <= 12 n_scans, flat <= 24 n_scans queries per sweep */
  int32_t max_points;     /* capacity of each less cloud, 1 .. 400000 */
  int32_t skip_frame_num; /* mapping_skip_frame (:199), >= 1; default 2, 1 in the launch files */
  int32_t reserved[4];
} slio_aloam_odom_params;

/* One opti pass (:317). stop: 0 max_num_iterations, 1 gradient, 2 function,
 * 3 parameter.  it_*[k]: the point, its cost and the radius mu after
 * iteration k (k < iterations).  few: corner + plane < 10 (:579). */
typedef struct slio_aloam_odom_pass {
  int32_t corner, plane, degenerate, iterations, accepted, outliers, stop, few;
  double cost_first, cost_last;
  double it_q[4][4], it_t[4][3], it_cost[4], it_mu[4];
} slio_aloam_odom_pass;

typedef struct slio_aloam_odom_result {
  double q_w_curr[4], t_w_curr[3];       /* /laser_odom_to_init (:607-619) */
  double q_last_curr[4], t_last_curr[3]; /* para_q, para_t */
  int32_t inited;    /* systemInited was set before this sweep: the passes ran */
  int32_t published; /* the skipFrameNum gate (:667) opened */
  int32_t frame_count, reserved;
  slio_aloam_odom_pass pass[2];
} slio_aloam_odom_result;

/* The host-side state of slio_aloam_odom_host_run: what the node keeps
 * between sweeps besides the last clouds. */
typedef struct slio_aloam_odom_state {
  double q_w_curr[4], t_w_curr[3], para_q[4], para_t[3];
  int32_t inited, frame_count;
} slio_aloam_odom_state;

/* The controller's state of one solve (slio_aloam_odom_lm_step). */
typedef struct slio_aloam_odom_lm {
  double mu, nu;
  double q[4], t[3];
  double A[21], g[6], cost;
  double delta[6], model, xnorm;
  double qn[4], tn[3];
  int32_t pivots_ok, iterations, accepted, stop, done, last_accepted;
} slio_aloam_odom_lm;

/* The last clouds on the device: n x {x, y, z, intensity}, valid until the
 * next run. */
typedef struct slio_aloam_odom_view {
  const float* corner_last;
  const float* surf_last;
  int32_t n_corner, n_surf, device, reserved;
} slio_aloam_odom_view;

/* device 0, n_scans 16, max_points 400000, skip_frame_num 2. */
int slio_aloam_odom_params_default(slio_aloam_odom_params* p);
/* EINVAL: n_scans outside 1 .. 64, max_points outside 1 .. 400000,
 * skip_frame_num < 1, negative device (before any device call), no such
 * device. */
int slio_aloam_odom_create(slio_aloam_odom_handle* out, const slio_aloam_odom_params* p);
int slio_aloam_odom_destroy(slio_aloam_odom_handle h);
/* Back to the state after create: identity poses, systemInited false,
 * frameCount 0 (:42-50, :55-59). */
int slio_aloam_odom_reset(slio_aloam_odom_handle h);
/* One sweep (:304-695) from four host clouds, n x {x, y, z, intensity} each.
 * EINVAL: a negative size, a null cloud with a size > 0, a null result, scan
 * ids of a less cloud decreasing or outside [0, 64); ECAPACITY: more sharp
 * points than 12 n_scans, flat than 24 n_scans, or less points than
 * max_points.  Returns after the handle's stream has finished. */
int slio_aloam_odom_run(slio_aloam_odom_handle h, const float* sharp, int64_t n_sharp, const float* less_sharp,
                        int64_t n_less_sharp, const float* flat, int64_t n_flat, const float* less_flat,
                        int64_t n_less_flat, slio_aloam_odom_result* res);
/* The same from the device-resident clouds of slio_aloam_get_view (which has
 * waited for the registration's stream); the clouds are copied device to
 * device, so the view may be overwritten afterwards.  EINVAL also for a view
 * of another device; the ids are checked by the kernel that copies. */
int slio_aloam_odom_run_view(slio_aloam_odom_handle h, const slio_aloam_view* v, slio_aloam_odom_result* res);
/* laserCloudCornerLast / laserCloudSurfLast (:650-659) to the host.  counts =
 * {corner, surf}.  ESTATE before a sweep; ECAPACITY where a cap is short. */
int slio_aloam_odom_get_last(slio_aloam_odom_handle h, float* corner_last, int64_t cap_corner, float* surf_last,
                             int64_t cap_surf, int32_t counts[2]);
int slio_aloam_odom_get_view(slio_aloam_odom_handle h, slio_aloam_odom_view* v);
/* (closest, second, third) per factor slot of the last association: the
 * sharp queries, then the flat ones; -1: none (a corner has no third).  n =
 * the slots.  ESTATE before an association; ECAPACITY: cap_slots < n. */
int slio_aloam_odom_get_correspondences(slio_aloam_odom_handle h, int32_t* corr, int64_t cap_slots, int32_t* n);
/* -- lockstep entries, for tests -- */
/* One association (:341-573) of the last sweep's sharp and flat points at
 * (q, t) against the last clouds, which after a first sweep are that sweep's
 * own less clouds.  ESTATE before a sweep. */
int slio_aloam_odom_associate(slio_aloam_odom_handle h, const double q[4], const double t[3]);
/* The factors of the last association at (q, t): A = sum w J^T J (upper
 * triangle, row-major), g = sum w J^T r, cost = 1/2 sum rho, counts =
 * {corner, plane, degenerate, outliers}.  ESTATE before an association. */
int slio_aloam_odom_evaluate(slio_aloam_odom_handle h, const double q[4], const double t[3], double A[21],
                             double g[6], double* cost, int32_t counts[4]);
/* -- host only, callable without a GPU -- */
/* The controller.  phase 0: start a solve at (lm->q, lm->t) with the
 * evaluation (lm->A, lm->g, lm->cost) there: mu 1e4, nu 2.  phase 1: the first
 * half of an iteration: the gradient stop, the damped LDL^T solve, the model
 * decrease, the proposed point (qn, tn); returns with lm->done set where the
 * solve has stopped.  phase 2: the second half, with the evaluation (A, g,
 * cost) at the proposed point: accept or reject, the radius, the function and
 * parameter stops. */
int slio_aloam_odom_lm_step(slio_aloam_odom_lm* lm, int phase, const double A[21], const double g[6], double cost);
/* The association as its literal serial loops.  corr: 3 ints per slot. */
int slio_aloam_odom_host_associate(const float* sharp, int64_t n_sharp, const float* flat, int64_t n_flat,
                                   const float* corner_last, int64_t n_corner, const float* surf_last,
                                   int64_t n_surf, const double q[4], const double t[3], int32_t* corr);
int slio_aloam_odom_host_evaluate(const float* sharp, int64_t n_sharp, const float* flat, int64_t n_flat,
                                  const float* corner_last, int64_t n_corner, const float* surf_last,
                                  int64_t n_surf, const int32_t* corr, const double q[4], const double t[3],
                                  double A[21], double g[6], double* cost, int32_t counts[4]);
/* state to identity poses, not inited, frame_count 0. */
int slio_aloam_odom_host_init(slio_aloam_odom_state* st);
/* One sweep on the host: the passes against (corner_last, surf_last), the
 * integration and the gate; the caller then makes its less clouds the last
 * ones.  p->device is not read. */
int slio_aloam_odom_host_run(const slio_aloam_odom_params* p, slio_aloam_odom_state* st, const float* sharp,
                             int64_t n_sharp, const float* flat, int64_t n_flat, const float* corner_last,
                             int64_t n_corner, const float* surf_last, int64_t n_surf,
                             slio_aloam_odom_result* res);

/* ======================================================================
 * A-LOAM laserMapping (src/A-LOAM/src/laserMapping.cpp; every path:line below
 * is in that file unless said otherwise): the loop body of process() :326-893
 * with the cloud outputs of :898-939 on the device, from the odometry's two
 * last clouds and /laser_odom_to_init to /aft_mapped_to_init and the rolling
 * map of 21 x 21 x 11 cubes of 50 m.  One sweep is
 *   initial guess   :148-152  transformAssociateToMap
 *   centre, shifts  :331-559  the centre cube from the DOUBLE t_w_curr, the
 *                             six shift loops composed
 *   selection       :566-583  i +- 2, j +- 2, k +- 1, k innermost: at most 75
 *                             cubes, each both valid and surround
 *   down-sampling   :597-607  VoxelGrid of both incoming clouds (leaf_corner,
 *                             leaf_surf; 0.4 / 0.8 at :993-997)
 *   gate            :613      more than 10 corner and more than 50 surf map
 *                             points in the valid cubes, or no optimisation
 *   two passes      :622-824  each one association at the current pose, then
 *                             one solve of at most 4 iterations (:811):
 *     pointAssociateToMap :160-168  q * p + t in double, rounded to float
 *     5-NN            :644, :722  exact, gate sqd[4] < 1.0
 *     line fit        :648-691  centre, covariance, 3 x 3 eigen-solve, the
 *                               test lambda2 > 3 lambda1, a / b = centre +- 0.1 d
 *     plane fit       :725-766  5 x 3 A x = -1, n = x / |x|, d = 1 / |x|, all
 *                               five neighbours within 0.2
 *     factors         lidarFactor.hpp:12-67 (double end points), :127-164,
 *                     analytic Jacobians in [d theta, d t], HuberLoss(0.1)
 *   transformUpdate :155-158  in every case
 *   map update      :835-892  both stacks at the solved pose into their cubes,
 *                             then the VoxelGrid of every valid cube
 * The cube store is livox_mapping's (slio_lvx_*: one SoA per class sorted by
 * cube, one pass and one host wait per change), its extents set to 21 x 21 x
 * 11.  The solve is enqueued whole -- per pass: associate (one launch per
 * class), evaluate, control, then 4 x (evaluate, control), the kernels of a
 * finished solve returning at once -- with no host wait in between: 24
 * launches for the two passes.  Host waits per sweep: 2 for the two
 * VoxelGrids of the incoming clouds, 0 to 2 for a shift (one per non-empty
 * class), 2 for the bounding boxes of the two search grids, 1 for the result,
 * 2 for the map update: 7, and up to 9 on a sweep that shifts.
 *
 * Stated departures from the reference:
 *  - the solve is not Ceres: this library's Levenberg-Marquardt of
 *    slio_aloam_odom_*, parity with Ceres' own iterates unpinned;
 *  - the eigen-solve (cyclic Jacobi, 8 sweeps) and the column-pivoting QR are
 *    this library's text (csrc/slio_aloam_map.hpp): parity with Eigen's
 *    SelfAdjointEigenSolver and with Eigen's summation order is unpinned; the
 *    sign of the line direction is free, it leaves J^T J and J^T r unchanged;
 *  - the 5-NN is exact with ties to the lower index in the concatenation of
 *    the valid cubes (FLANN's order among equal distances is unpinned);
 *  - a VoxelGrid sums a voxel's points in the stored order (slio_lvx_*'s);
 *  - the map stores x, y, z only: A-LOAM's intensity only reaches published
 *    clouds (slio_aloam_map_register_cloud keeps it);
 *  - a zero covariance, a rank-deficient plane system or a plane normal that
 *    is not finite gives no factor and is counted as degenerate (the
 *    reference would hand Ceres a NaN, or a plane through collinear points);
 *  - a point that does not transform to a finite coordinate is dropped at
 *    append;
 *  - the sums run over factor slots (corner stack, then surf stack) in a
 *    fixed order: per 256 slots 32 strided partials in ascending slot, added
 *    in ascending lane, then the same over the groups of 256;
 *  - publishers, path, TF and the message queue's dropping of old frames
 *    (:317-320) are not restated.
 * ====================================================================== */
typedef struct slio_aloam_map* slio_aloam_map_handle;
typedef struct slio_aloam_map_host* slio_aloam_map_host_handle;

typedef struct slio_aloam_map_params {
  int32_t device;
  int32_t max_points; /* capacity of each class of the map, >= 1 */
  int32_t max_scan;   /* capacity of each incoming cloud, 1 .. 400000 */
  float leaf_corner;  /* mapping_line_resolution (:993), 0.4 */
  float leaf_surf;    /* mapping_plane_resolution (:994), 0.8 */
  int32_t reserved[3];
} slio_aloam_map_params;

typedef struct slio_aloam_map_result {
  double q_w_curr[4], t_w_curr[3];         /* /aft_mapped_to_init */
  double q_wmap_wodom[4], t_wmap_wodom[3]; /* after transformUpdate */
  int32_t center[3], shift[3];             /* the centre cube after the shifts; turns of the `< 3` loops minus
                                              those of the `>= dim - 3` loops */
  int32_t map_size[2];                     /* laserCloudCornerFromMapNum, laserCloudSurfFromMapNum */
  int32_t stack_size[2];                   /* the two down-sampled clouds */
  int32_t optimized;                       /* the gate of :613 opened: pass[] is filled */
  int32_t nvalid;                          /* laserCloudValidNum */
  slio_aloam_odom_pass pass[2];            /* corner / plane: factors; few: always 0 */
} slio_aloam_map_result;

/* device 0, max_points 2^21, max_scan 400000, leaves 0.4 / 0.8. */
int slio_aloam_map_params_default(slio_aloam_map_params* p);
/* EINVAL: max_points < 1, max_scan outside 1 .. 400000, a leaf that is not
 * finite and positive, negative device (before any device call), no such device. */
int slio_aloam_map_create(slio_aloam_map_handle* out, const slio_aloam_map_params* p);
int slio_aloam_map_destroy(slio_aloam_map_handle h);
/* Back to the state after create: empty map, centres 10 / 10 / 5, identity poses. */
int slio_aloam_map_reset(slio_aloam_map_handle h);
/* One sweep from laserCloudCornerLast / laserCloudSurfLast on the host, n x
 * {x, y, z, intensity} each, and the odometry's pose.  EINVAL (before any
 * device call): a negative size, a null cloud with a size > 0, a null or
 * non-finite pose, a zero q_wodom_curr, a null result; ECAPACITY: a cloud
 * beyond max_scan, or stored + incoming points of a class beyond max_points.
 * The handle is unchanged after a refused call. */
int slio_aloam_map_run(slio_aloam_map_handle h, const float* corner_last, int64_t n_corner, const float* surf_last,
                       int64_t n_surf, const double q_wodom_curr[4], const double t_wodom_curr[3],
                       slio_aloam_map_result* res);
/* The same from the odometry's device-resident last clouds
 * (slio_aloam_odom_get_view), device to device.  EINVAL also for a view of
 * another device. */
int slio_aloam_map_run_view(slio_aloam_map_handle h, const slio_aloam_odom_view* v, const double q_wodom_curr[4],
                            const double t_wodom_curr[3], slio_aloam_map_result* res);
/* laserCloudFullRes into the map frame at the last sweep's pose (:929-933):
 * n x {x, y, z, intensity}, intensity kept.  on_device: xyzi is a device
 * pointer of the handle's device.  ESTATE before a sweep. */
int slio_aloam_map_register_cloud(slio_aloam_map_handle h, const float* xyzi, int64_t n, int on_device, float* out);
/* One cube (n x 3), the sizes of all 4851 cubes, the cubes of the last
 * selection concatenated (:899-905, one class), a whole class in cube order
 * (:916-921, one class), the down-sampled cloud of the last sweep.  kind 0
 * corner, 1 surf.  xyz null: the size only.  ESTATE before a sweep;
 * ECAPACITY: cap < n. */
int slio_aloam_map_get_cube(slio_aloam_map_handle h, int kind, int32_t cube, float* xyz, int64_t cap, int64_t* n);
int slio_aloam_map_cube_sizes(slio_aloam_map_handle h, int kind, int32_t* sizes);
int slio_aloam_map_get_surround(slio_aloam_map_handle h, int kind, float* xyz, int64_t cap, int64_t* n);
int slio_aloam_map_get_map(slio_aloam_map_handle h, int kind, float* xyz, int64_t cap, int64_t* n);
int slio_aloam_map_get_stack(slio_aloam_map_handle h, int kind, float* xyz, int64_t cap, int64_t* n);
/* -- lockstep entries, for tests -- */
/* One association of the last sweep's stacks at (q, t) against the map that
 * sweep was solved against.  ESTATE before a sweep, or where that sweep's
 * gate stayed shut (no search grid was built). */
int slio_aloam_map_associate(slio_aloam_map_handle h, const double q[4], const double t[3]);
/* Per slot (corner stack, then surf stack) of the last association: kind (0
 * none, 1 edge, 2 plane, 3 degenerate, 4 rejected by the fit), the record (6
 * doubles: a, b or n, d, 0, 0), the five neighbours' indices in the
 * concatenation of the valid cubes and their squared distances (-1 / +inf
 * where the gate stayed shut).  Any output may be null.  ESTATE before an
 * association; ECAPACITY: cap_slots < n. */
int slio_aloam_map_get_association(slio_aloam_map_handle h, uint8_t* kind, double* rec, int32_t* nbr_idx,
                                   float* nbr_sqd, int64_t cap_slots, int32_t* n);
/* The factors of the last association at (q, t): A, g, cost as
 * slio_aloam_odom_evaluate, counts = {edge, plane, degenerate, outliers}. */
int slio_aloam_map_evaluate(slio_aloam_map_handle h, const double q[4], const double t[3], double A[21], double g[6],
                            double* cost, int32_t counts[4]);
/* -- host only, callable without a GPU -- */
/* :222-223: the high-frequency pose from q / t_wmap_wodom and an odometry pose. */
int slio_aloam_map_predict(const double q_wmap_wodom[4], const double t_wmap_wodom[3], const double q_wodom_curr[4],
                           const double t_wodom_curr[3], double q_w_curr[4], double t_w_curr[3]);
/* :331-583 at t_w_curr: cen (laserCloudCenWidth / Height / Depth) is updated;
 * list holds up to 75 cube indices. */
int slio_aloam_map_host_select(const double t_w_curr[3], int32_t cen[3], int32_t center[3], int32_t shift[3],
                               int32_t* list, int32_t* n);
/* The fits on five neighbours (15 doubles, nearest first).  Return the kind
 * (1 edge / 2 plane, 3 degenerate, 4 rejected) or a negative error.  lam / vec
 * (3 / 9 doubles, vec row-major with the eigenvectors in its columns; either
 * may be null): the eigen-solve of the covariance.  x (3 doubles, may be
 * null): the solution of A x = -1 before normalisation. */
int slio_aloam_map_host_fit_line(const double* nb, double a[3], double b[3], double* lam, double* vec);
int slio_aloam_map_host_fit_plane(const double* nb, double normal[3], double* d, double* x);
/* The sums over n slots (points n x 3, kinds, records) at (q, t), in the stated order. */
int slio_aloam_map_host_evaluate(const float* xyz, const uint8_t* kind, const double* rec, int64_t n,
                                 const double q[4], const double t[3], double A[21], double g[6], double* cost,
                                 int32_t counts[4]);
/* The whole node on the host: the same entries on a host-resident map (p->device
 * is not read); the 5-NN is brute force over the valid cubes.  get_association
 * reports the last pass's. */
int slio_aloam_map_host_create(slio_aloam_map_host_handle* out, const slio_aloam_map_params* p);
int slio_aloam_map_host_destroy(slio_aloam_map_host_handle h);
int slio_aloam_map_host_run(slio_aloam_map_host_handle h, const float* corner_last, int64_t n_corner,
                            const float* surf_last, int64_t n_surf, const double q_wodom_curr[4],
                            const double t_wodom_curr[3], slio_aloam_map_result* res);
int slio_aloam_map_host_get_cube(slio_aloam_map_host_handle h, int kind, int32_t cube, float* xyz, int64_t cap,
                                 int64_t* n);
int slio_aloam_map_host_get_stack(slio_aloam_map_host_handle h, int kind, float* xyz, int64_t cap, int64_t* n);
int slio_aloam_map_host_get_association(slio_aloam_map_host_handle h, uint8_t* kind, double* rec, int32_t* nbr_idx,
                                        float* nbr_sqd, int64_t cap_slots, int32_t* n);

/* ======================================================================
 * LIO-Livox ScanRegistration for Use_seg = 0 (src/LIO-Livox/src/lio/
 * ScanRegistration.cpp, "SR" below, and LidarFeatureExtractor.cpp, every other
 * path:line below): lidarCallBackHorizon -> FeatureExtract :1218-1291 and
 * lidarCallBackPc2 (SR:61-93) -> FeatureExtract_Mid :1352-1401, with
 * detectFeaturePoint :93-614 once per line, on the device.  One opaque handle
 * owns the buffers of one device and one stream.  A run is
 *   ingest     :1237-1263  (SR:69-84 for Pc2) the line and x filters, normal_x,
 *                          the per-line lists in the message's order
 *   finite     :112-130    the finite points of each line, order kept
 *   per point  :151-203    depth, the two ray angles, K, curvature, diffR
 *   picking    :205-297    PartNum parts per line, each sorted twice (stable),
 *                          the flag loop (3 and the neighbour marks 1) and the
 *                          pick loop (2, and 300 by reflectivity)
 *   lines      :301-403    the strided pass (i += 4 after a flat right side):
 *                          150 where two flat sides meet at a sharp angle
 *   breaks     :407-578    100 by the depth-ordering rules, demoted to 101 by
 *                          the front / back fan test
 *   collect    :591-613    2 -> surf, 100 / 150 -> corner, the near points out
 *   write-back :1273-1290  the labels 1 (corner) and 2 (surf) on the cloud, the
 *                          two feature clouds in cloud order
 * as nine launches, whatever n, on one stream and ONE host wait, the copy of
 * the counts.  The three clouds stay on the device until the next run.
 *
 * A cloud point is 8 floats: {x, y, z, intensity, normal_x, normal_y, normal_z,
 * curvature = 0}.  normal_x is the time fraction; normal_y the line, as the
 * int's bits in the CustomMsg path (_int_as_float, :1254) and as a float value
 * in the Pc2 path (SR:82); normal_z the label 0 / 1 / 2.
 *
 * Kept as written: the label of a line's feature idx (an index into the
 * line's FINITE points) lands on vlines[line][idx], an index into ALL its
 * points (:1276, :1280), so a line with non-finite points labels other points
 * of that line; K in the picking loops is the K of the line's last loop
 * position, so NumCurvSize is accepted and never has an effect; temp_depth
 * reads i - k in both fan loops (:535, :554).
 *
 * Undefined in the reference, defined here: cloudAngle[] and CloudFeatureFlag[]
 * (:96, :102, never initialised) are zero before use; thNumCurvSize (raced on
 * by the per-line threads) is a per-line value; a line of more than 20000
 * points after ingest (:96) is SLIO_ECAPACITY, nothing is truncated; the Pc2
 * entries (line = i % 4) want n_scans >= 4, SLIO_EINVAL otherwise (:1372
 * indexes past vlines); an empty message (:1238 calls back()) gives zero
 * counts.  plane_judge (:473, :512) is dead and not built.  A diffR or a
 * curvature that is NaN (a NaN or infinite intensity in the Pc2 cloud, which
 * only x, y and z are tested for, reaches the diffR of up to seven points
 * around it; coordinates near FLT_MAX do it to the curvature) leaves the
 * reference's two sorts to the order of their swaps; here NaN sorts as one
 * class after every number, ties by position, on the host and on the device.
 * Errors as in slio.h; argument errors are reported before any device call.
 * ====================================================================== */
typedef struct slio_llreg* slio_llreg_handle;

typedef struct slio_llreg_params {
  int32_t device;
  int32_t max_points;            /* input capacity, 1 .. 120000 = 6 lines of 20000 (:96)      */
  int32_t n_scans;               /* Used_Line, 1 .. 6                                         */
  int32_t lidar_type;            /* Lidar_Type 0 / 1: x < 0.01 dropped; 2: fabs(x) < 0.01      */
  int32_t num_curv_size;         /* NumCurvSize: accepted, never has an effect (see above)    */
  int32_t num_flat;              /* NumFlat >= 0                                              */
  int32_t part_num;              /* PartNum, 1 .. 20000                                       */
  float distance_faraway;        /* DistanceFaraway                                           */
  float flat_threshold;          /* FlatThreshold                                             */
  float break_corner_dis;        /* BreakCornerDis                                            */
  float lidar_nearest_dis;       /* LidarNearestDis                                           */
  float kdtree_corner_outlier_dis; /* KdTreeCornerOutlierDis: read by no path built here      */
  int32_t reserved[4];
} slio_llreg_params;

/* What a consumer on the device reads (a later estimator): device pointers to
 * the three clouds of the last run, n x 8 floats each. */
typedef struct slio_llreg_view {
  const float* cloud;
  const float* corner;
  const float* surf;
  int32_t n_cloud, n_corner, n_surf, device;
} slio_llreg_view;

/* config/horizon_config.yaml: device 0, max_points 120000, 6 lines, type 0,
 * NumCurvSize 2, DistanceFaraway 100, NumFlat 3, PartNum 150, FlatThreshold
 * 0.02, BreakCornerDis 1, LidarNearestDis 1, KdTreeCornerOutlierDis 0.2. */
int slio_llreg_params_default(slio_llreg_params* p);
/* The LidarFeatureExtractor constructor (:3-23).  EINVAL: a field outside the
 * ranges above, a threshold that is not finite, no such device. */
int slio_llreg_create(slio_llreg_handle* out, const slio_llreg_params* p);
int slio_llreg_destroy(slio_llreg_handle h);
/* lidarCallBackHorizon's FeatureExtract (:1218-1291) on one CustomMsg as SoA
 * arrays: xyz[n * 3], reflectivity[n], line[n], offset_time[n].  counts =
 * {laserCloud, laserConerFeature, laserSurfFeature} sizes.  EINVAL: n < 0, a
 * null array with n > 0, null counts; ECAPACITY: n > max_points, or a line of
 * more than 20000 points after ingest (the handle then has no run). */
int slio_llreg_run(slio_llreg_handle h, const float* xyz, const uint8_t* reflectivity, const uint8_t* line,
                   const uint32_t* offset_time, int64_t n, int32_t counts[3]);
/* lidarCallBackPc2 (SR:61-93) with FeatureExtract_Mid (:1352-1401) on xyzi[n *
 * 4]: the x filter of lidar_type, normal_x = float(i) / float(n), line = i % 4
 * with i the index before the filter.  counts[0] is laser_cloud_custom's size.
 * EINVAL also when the handle's n_scans < 4. */
int slio_llreg_run_pc2(slio_llreg_handle h, const float* xyzi, int64_t n, int32_t counts[3]);
/* kind 0: the full cloud with its labels (:1285 reads it), 1: laserConerFeature
 * (:1286), 2: laserSurfFeature (:1289); counts[kind] x 8 floats.  ESTATE
 * without a run; ECAPACITY when cap (in points) is less. */
int slio_llreg_get_cloud(slio_llreg_handle h, int kind, float* points, int64_t cap);
/* vlines[l]->size() (:1261) and the number of finite points among them (:132)
 * for l < 6 (zero past n_scans).  Either may be NULL. */
int slio_llreg_get_lines(slio_llreg_handle h, int32_t line_size[6], int32_t finite_size[6]);
/* For tests: line l's CloudFeatureFlag[0 .. finite_size[l]) after the break-
 * point loop, 1 where the line-feature loop (:301) visited the position, and
 * the finite points themselves (x 4 floats).  Any may be NULL; cap in points. */
int slio_llreg_get_flags(slio_llreg_handle h, int32_t l, int32_t* flags, uint8_t* visited, float* xyzi, int64_t cap);
int slio_llreg_get_view(slio_llreg_handle h, slio_llreg_view* v);
/* The shapes of the kernels, for tests that put seams on them: the chain kernel
 * (one workgroup per line) gives thread t the loop positions [5 + t *
 * chain_per_thread, 5 + (t + 1) * chain_per_thread); the picking kernel
 * resolves a part of up to pick_fast points in registers and a longer one
 * serially on one lane; every other kernel works on block inputs per workgroup. */
int slio_llreg_tiles(int32_t* chain_per_thread, int32_t* chain_per_workgroup, int32_t* pick_fast, int32_t* block);
/* -- host only, callable without a GPU -- */
/* The same two paths as their literal serial loops (p->device and max_points
 * are not read).  cloud / corner / surf: n x 8 floats; flags / visited / lines
 * (x 4 floats): the lines' finite points concatenated in line order, n entries
 * at most; line_size / finite_size as slio_llreg_get_lines.  Every output but
 * counts may be NULL. */
int slio_llreg_extract_host(const slio_llreg_params* p, const float* xyz, const uint8_t* reflectivity,
                            const uint8_t* line, const uint32_t* offset_time, int64_t n, float* cloud, float* corner,
                            float* surf, int32_t counts[3], int32_t* line_size, int32_t* finite_size, int32_t* flags,
                            uint8_t* visited, float* lines);
int slio_llreg_extract_pc2_host(const slio_llreg_params* p, const float* xyzi, int64_t n, float* cloud, float* corner,
                                float* surf, int32_t counts[3], int32_t* line_size, int32_t* finite_size,
                                int32_t* flags, uint8_t* visited, float* lines);

#ifdef __cplusplus
}
#endif

#endif /* SLIO_FRONTEND_H */
