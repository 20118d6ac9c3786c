"""Host side of the LeGO-LOAM front-end, mirroring
ImageProjection (LeGO-LOAM/src/imageProjection.cpp) and the whole of
FeatureAssociation::runFeatureAssociation (featureAssociation.cpp): the front
half (adjustDistortion, calculateSmoothness, markOccludedPoints,
extractFeatures) and, after `enable_odometry`, the back half -- the
scan-to-scan odometry that produces /laser_odom_to_init
(checkSystemInitialization, updateInitialGuess, updateTransformation,
integrateTransformation, publishOdometry, publishCloudsLast).

The IMU ring buffer that adjustDistortion reads is host state filled message
by message (imuHandler + AccumulateIMUShiftAndRotation, :430-588); `LegoImu`
restates it.  The device side lives behind include/slio_frontend.h
(slio_lego_*, slio_lego_odom_*).
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib as L
from .lego_map import (LegoLoopClosure, LegoMapping, TransformFusion,  # noqa: F401  (the mapping back-end)
                       extract_surrounding)

IMU_QUE_LEN = 200  # imuQueLength (utility.h:42)


@dataclass
class LegoParams:
    """LeGO-LOAM/include/utility.h:20-49 (VLP-16) and the less-flat VoxelGrid
    leaf of featureAssociation.cpp:222."""
    N_SCAN: int = 16
    Horizon_SCAN: int = 1800
    ang_res_x: float = 0.2
    ang_res_y: float = 2.0
    ang_bottom: float = 15.0 + 0.1
    groundScanInd: int = 7
    sensorMountAngle: float = 0.0
    segmentTheta: float = 1.0472
    segmentValidPointNum: int = 5
    segmentValidLineNum: int = 3
    edgeThreshold: float = 0.1
    surfThreshold: float = 0.1
    leafSize: float = 0.2
    scanPeriod: float = 0.1

    def to_c(self, device: int = 0, max_points: int = 0) -> L.SlioLegoParams:
        p = L.SlioLegoParams()
        L.load().slio_lego_params_default(C.byref(p))
        p.device, p.max_points = device, max_points
        p.n_scan, p.horizon_scan, p.ground_scan_ind = self.N_SCAN, self.Horizon_SCAN, self.groundScanInd
        p.segment_valid_point_num = self.segmentValidPointNum
        p.segment_valid_line_num = self.segmentValidLineNum
        p.ang_res_x, p.ang_res_y, p.ang_bottom = self.ang_res_x, self.ang_res_y, self.ang_bottom
        p.sensor_mount_angle, p.segment_theta = self.sensorMountAngle, self.segmentTheta
        p.edge_threshold, p.surf_threshold = self.edgeThreshold, self.surfThreshold
        p.leaf_size, p.scan_period = self.leafSize, self.scanPeriod
        return p


class LegoImu:
    """FeatureAssociation's IMU ring buffer (featureAssociation.cpp:109-132):
    imuHandler (:559-587) + AccumulateIMUShiftAndRotation (:430-557), and the
    pointers / angular rotation adjustDistortion carries between scans."""

    def __init__(self, que_len: int = IMU_QUE_LEN, scan_period: float = 0.1):
        f = lambda: np.zeros(que_len, np.float32)  # noqa: E731
        self.Q = que_len
        self.scan_period = scan_period
        self.time = np.zeros(que_len, np.float64)
        self.roll, self.pitch, self.yaw = f(), f(), f()
        self.acc_x, self.acc_y, self.acc_z = f(), f(), f()
        self.velo_x, self.velo_y, self.velo_z = f(), f(), f()
        self.shift_x, self.shift_y, self.shift_z = f(), f(), f()
        self.angvel_x, self.angvel_y, self.angvel_z = f(), f(), f()
        self.ang_x, self.ang_y, self.ang_z = f(), f(), f()
        self.pointer_last = -1
        self.pointer_last_iteration = 0
        self.ang_last = np.zeros(3, np.float32)

    def imuHandler(self, stamp: float, roll: float, pitch: float, yaw: float, acc, gyro):
        f32 = np.float32
        ax = f32(acc[1] - math.sin(roll) * math.cos(pitch) * 9.81)
        ay = f32(acc[2] - math.cos(roll) * math.cos(pitch) * 9.81)
        az = f32(acc[0] + math.sin(pitch) * 9.81)
        p = self.pointer_last = (self.pointer_last + 1) % self.Q
        self.time[p] = stamp
        self.roll[p], self.pitch[p], self.yaw[p] = roll, pitch, yaw
        self.acc_x[p], self.acc_y[p], self.acc_z[p] = ax, ay, az
        self.angvel_x[p], self.angvel_y[p], self.angvel_z[p] = gyro
        self._accumulate()

    def _accumulate(self):
        f32 = np.float32
        p = self.pointer_last
        r, pi, yw = f32(self.roll[p]), f32(self.pitch[p]), f32(self.yaw[p])
        ax, ay, az = self.acc_x[p], self.acc_y[p], self.acc_z[p]
        c, s = f32(math.cos(r)), f32(math.sin(r))
        x1, y1, z1 = f32(c * ax - s * ay), f32(s * ax + c * ay), az
        c, s = f32(math.cos(pi)), f32(math.sin(pi))
        x2, y2, z2 = x1, f32(c * y1 - s * z1), f32(s * y1 + c * z1)
        c, s = f32(math.cos(yw)), f32(math.sin(yw))
        ax, ay, az = f32(c * x2 + s * z2), y2, f32(-s * x2 + c * z2)
        b = (p + self.Q - 1) % self.Q
        dt = self.time[p] - self.time[b]
        if dt < self.scan_period:
            for sh, ve, a in ((self.shift_x, self.velo_x, ax), (self.shift_y, self.velo_y, ay),
                              (self.shift_z, self.velo_z, az)):
                sh[p] = f32(sh[b] + ve[b] * dt + a * dt * dt / 2)
                ve[p] = f32(ve[b] + a * dt)
            for an, av in ((self.ang_x, self.angvel_x), (self.ang_y, self.angvel_y),
                           (self.ang_z, self.angvel_z)):
                an[p] = f32(an[b] + av[b] * dt)

    def feed(self, imu: dict, until: float):
        """imuHandler for every message of a synth stream up to `until`."""
        for k in range(imu["time"].size):
            if imu["time"][k] > until:
                break
            self.imuHandler(float(imu["time"][k]), float(imu["roll"][k]), float(imu["pitch"][k]),
                            float(imu["yaw"][k]), imu["acc"][k], imu["gyro"][k])


def odometry_step(kind: int, AtA, AtB, nsel: int, iter_count: int, transform_cur, is_degenerate: int, matP):
    """slio_lego_odom_step: calculateTransformation{Surf,Corner} from
    cv::solve on (featureAssociation.cpp:1649-1695 / :1764-1814), the same
    code the device loop runs in-kernel.  transform_cur [6] and matP [9]
    (contiguous float32 arrays) are updated in place.  Returns (rc,
    keep_going, is_degenerate); rc 1 means fewer than 10 rows and no step."""
    a = np.ascontiguousarray(AtA, np.float32)
    b = np.ascontiguousarray(AtB, np.float32)
    deg, keep = C.c_int(int(is_degenerate)), C.c_int(1)
    rc = L.load().slio_lego_odom_step(kind, L.fptr(a), L.fptr(b), int(nsel), iter_count, L.fptr(transform_cur),
                                      C.byref(deg), L.fptr(matP), C.byref(keep))
    if rc < 0:
        L.check(rc, "slio_lego_odom_step")
    return rc, keep.value, deg.value


class LegoFrontEnd:
    """ImageProjection::cloudHandler + FeatureAssociation::runFeatureAssociation
    as one device pipeline: the front half (adjustDistortion ..
    extractFeatures, slio_lego_run) and, once `enable_odometry` was called, the
    scan-to-scan odometry (slio_lego_odom_run).  The range image,
    segmentation, cloud_info and the feature clouds never leave HBM.  No CPU
    fallback: without libslio.so the constructor raises."""

    def __init__(self, params: LegoParams | None = None, device: int = 0, max_points: int = 0):
        self.params = params or LegoParams()
        self.lib = L.load()
        self.h = C.c_void_p()
        self._p = self.params.to_c(device, max_points)
        L.check(self.lib.slio_lego_create(C.byref(self.h), C.byref(self._p)), "slio_lego_create")
        self.counts = L.SlioLegoCounts()
        self._n_outlier_last = 0   # the device's count of published outlier points (odometry)

    def close(self):
        if self.h:
            self.lib.slio_lego_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_imu(self, imu: LegoImu | None, time_scan_cur: float = 0.0):
        """The IMU state adjustDistortion reads (None: imuPointerLast = -1)."""
        if imu is None:
            L.check(self.lib.slio_lego_set_imu(self.h, None), "set_imu")
            return
        keep = [np.ascontiguousarray(imu.time, np.float64)]
        arrs = []
        for n in ("roll", "pitch", "yaw", "velo_x", "velo_y", "velo_z", "shift_x", "shift_y",
                  "shift_z", "ang_x", "ang_y", "ang_z"):
            a = np.ascontiguousarray(getattr(imu, n), np.float32)
            keep.append(a)
            arrs.append(L.fptr(a))
        s = L.SlioLegoImu(L.dptr(keep[0]), *arrs, imu.pointer_last, imu.pointer_last_iteration,
                          imu.Q, float(time_scan_cur), (C.c_float * 3)(*imu.ang_last))
        L.check(self.lib.slio_lego_set_imu(self.h, C.byref(s)), "set_imu")

    def upload(self, x, y, z):
        f = [np.ascontiguousarray(v, dtype=np.float32) for v in (x, y, z)]
        self._keep = f
        L.check(self.lib.slio_lego_upload(self.h, *(L.fptr(v) for v in f), len(f[0])), "upload")

    def run(self) -> L.SlioLegoCounts:
        L.check(self.lib.slio_lego_run(self.h, C.byref(self.counts)), "slio_lego_run")
        return self.counts

    def cloudHandler(self, x, y, z, imu: LegoImu | None = None, time_scan_cur: float = 0.0):
        """One sweep through imageProjection + featureAssociation's front half;
        carries the IMU pointers / angular rotation into `imu` as the
        reference does between scans."""
        self.set_imu(imu, time_scan_cur)
        self.upload(x, y, z)
        self.run()
        f = self.features()
        if imu is not None:
            imu.pointer_last_iteration = f["imu_out"]["pointer_last_iteration"]
            imu.ang_last = np.asarray(f["imu_out"]["ang_last"], np.float32)
        return f

    # -------------------------------------------------------------- odometry
    def enable_odometry(self, nearest_feature_sq_dist: float = 25.0, max_iterations: int = 25,
                        search_period: int = 5, skip_frame_num: int = 1):
        """Allocate the back half's device state (slio_lego_odom_enable);
        calling it again resets it."""
        p = L.SlioLegoOdomParams()
        L.check(self.lib.slio_lego_odom_params_default(C.byref(p)), "odom_params_default")
        p.nearest_feature_sq_dist, p.max_iterations = nearest_feature_sq_dist, max_iterations
        p.search_period, p.skip_frame_num = search_period, skip_frame_num
        p.scan_period = self.params.scanPeriod
        L.check(self.lib.slio_lego_odom_enable(self.h, C.byref(p)), "odom_enable")
        self._n_outlier_last = 0

    def reset_odometry(self):
        L.check(self.lib.slio_lego_odom_reset(self.h), "odom_reset")
        self._n_outlier_last = 0

    @staticmethod
    def _odom_dict(o: L.SlioLegoOdomOut) -> dict:
        return dict(transform_cur=np.array(o.transform_cur, np.float32),
                    transform_sum=np.array(o.transform_sum, np.float32), inited=o.inited,
                    iters=list(o.iters), rows=list(o.rows), degenerate=list(o.degenerate),
                    n_corner_last=o.n_corner_last, n_surf_last=o.n_surf_last, published=o.published,
                    n_outlier_last=o.n_outlier_last)

    def odometry_run(self) -> dict:
        """The back half for the sweep last run (slio_lego_odom_run)."""
        o = L.SlioLegoOdomOut()
        L.check(self.lib.slio_lego_odom_run(self.h, C.byref(o)), "odom_run")
        self._n_outlier_last = o.n_outlier_last
        return self._odom_dict(o)

    def runFeatureAssociation(self, x, y, z, imu: LegoImu | None = None, time_scan_cur: float = 0.0):
        """cloudHandler followed by the odometry; returns the odometry result
        (`features` holds what cloudHandler returns)."""
        f = self.cloudHandler(x, y, z, imu, time_scan_cur)
        out = self.odometry_run()
        out["features"] = f
        return out

    def odometry_pose(self):
        """publishOdometry (:2106-2128): (quaternion xyzw, position) of
        /laser_odom_to_init from the last transformSum, on the host
        (tf::createQuaternionMsgFromRollPitchYaw(ts[2], -ts[0], -ts[1]))."""
        ts = self.odometry_state()["transform_sum"].astype(np.float64)
        hr, hp, hy = ts[2] * 0.5, -ts[0] * 0.5, -ts[1] * 0.5
        cy, sy, cp, sp, cr, sr = (math.cos(hy), math.sin(hy), math.cos(hp), math.sin(hp), math.cos(hr),
                                  math.sin(hr))
        qx, qy = sr * cp * cy - cr * sp * sy, cr * sp * cy + sr * cp * sy
        qz, qw = cr * cp * sy - sr * sp * cy, cr * cp * cy + sr * sp * sy
        return np.array([-qy, -qz, qx, qw]), ts[3:6].copy()

    def last_clouds(self) -> dict:
        """What publishCloudsLast publishes (slio_lego_odom_get_last)."""
        st = self.odometry_state()
        cl = np.empty((st["n_corner_last"], 4), np.float32)
        sl = np.empty((st["n_surf_last"], 4), np.float32)
        ol = np.empty((self._n_outlier_last, 4), np.float32)   # only enable / reset / a run change it
        L.check(self.lib.slio_lego_odom_get_last(self.h, L.fptr(cl), L.fptr(sl), L.fptr(ol)), "odom_get_last")
        return dict(laserCloudCornerLast=cl, laserCloudSurfLast=sl, outlierCloudLast=ol)

    # lockstep / test entries
    _STATE_VEC = ("transform_cur", "transform_sum", "imu_last", "imu_shift_from_start",
                  "imu_velo_from_start", "mat_p")
    _STATE_INT = ("system_inited", "is_degenerate", "frame_count", "n_corner_last", "n_surf_last")

    def odometry_state(self) -> dict:
        s = L.SlioLegoOdomState()
        L.check(self.lib.slio_lego_odom_get_state(self.h, C.byref(s)), "odom_get_state")
        d = {k: np.array(getattr(s, k), np.float32) for k in self._STATE_VEC}
        d.update({k: getattr(s, k) for k in self._STATE_INT})
        return d

    def set_odometry_state(self, **kw):
        """Overwrite the named members of the odometry state."""
        s = L.SlioLegoOdomState()
        L.check(self.lib.slio_lego_odom_get_state(self.h, C.byref(s)), "odom_get_state")
        for k, v in kw.items():
            if k in self._STATE_VEC:
                a = np.asarray(v, np.float32)
                setattr(s, k, (C.c_float * a.size)(*a))
            elif k in self._STATE_INT:
                setattr(s, k, int(v))
            else:
                raise KeyError(k)
        L.check(self.lib.slio_lego_odom_set_state(self.h, C.byref(s)), "odom_set_state")

    def odometry_set_clouds(self, sharp, flat, corner_last, surf_last) -> int:
        """Inject the four clouds (xyzi); returns the C status (SLIO_EINVAL
        for a last cloud whose ring order decreases)."""
        a = [np.ascontiguousarray(v, np.float32).reshape(-1, 4) for v in (sharp, flat, corner_last, surf_last)]
        args = []
        for v in a:
            args += [L.fptr(v), v.shape[0]]
        return self.lib.slio_lego_odom_set_clouds(self.h, *args)

    def odometry_pass(self, kind: int, iter_count: int, transform_cur, n: int) -> dict:
        """One correspondence + normal-equations pass (slio_lego_odom_pass);
        n is the kind's query count."""
        tc = np.ascontiguousarray(transform_cur, np.float32)
        ind = np.empty((3, n), np.int32)
        coeff, sel = np.empty((n, 4), np.float32), np.empty(n, np.uint8)
        AtA, AtB, nsel = np.empty(9, np.float32), np.empty(3, np.float32), C.c_int32()
        L.check(self.lib.slio_lego_odom_pass(self.h, kind, iter_count, L.fptr(tc), L.iptr(ind), L.fptr(coeff),
                                             L.u8ptr(sel), L.fptr(AtA), L.fptr(AtB), C.byref(nsel)), "odom_pass")
        return dict(ind=ind, coeff=coeff, sel=sel, AtA=AtA, AtB=AtB, nsel=nsel.value)

    def odometry_step(self, kind: int, AtA, AtB, nsel: int, iter_count: int, transform_cur, is_degenerate: int,
                      matP):
        """The host export of the in-kernel step; transform_cur and matP
        (float32 arrays) are updated in place.  Returns (rc, keep_going,
        is_degenerate); rc 1: fewer than 10 rows, no step."""
        return odometry_step(kind, AtA, AtB, nsel, iter_count, transform_cur, is_degenerate, matP)

    def odometry_lockstep(self, kind: int, n: int, transform_cur, is_degenerate: int, matP, max_iterations=25):
        """One loop of updateTransformation on the host: a pass and a step per
        iteration, with the loop's `continue` and `break`.  Returns
        (iterations, rows, degenerate of iteration 0, is_degenerate)."""
        iters = rows = deg0 = 0
        for it in range(max_iterations):
            p = self.odometry_pass(kind, it, transform_cur, n)
            iters, rows = it + 1, p["nsel"]
            rc, keep, is_degenerate = odometry_step(kind, p["AtA"], p["AtB"], p["nsel"], it, transform_cur,
                                                    is_degenerate, matP)
            if rc == 1:
                continue
            if it == 0:
                deg0 = is_degenerate
            if not keep:
                break
        return iters, rows, deg0, is_degenerate

    # --------------------------------------------------------------- outputs
    def image(self) -> dict:
        N, H = self.params.N_SCAN, self.params.Horizon_SCAN
        rm = np.empty((N, H), np.float32)
        own = np.empty((N, H), np.int32)
        gr = np.empty((N, H), np.int8)
        lb = np.empty((N, H), np.int32)
        L.check(self.lib.slio_lego_get_image(self.h, L.fptr(rm), L.iptr(own),
                                             gr.ctypes.data_as(C.POINTER(C.c_int8)), L.iptr(lb)),
                "image")
        return dict(range_mat=rm, cell_point=own, ground=gr, label=lb)

    def seg_info(self) -> dict:
        c, R = self.counts, self.params.N_SCAN
        n, no = c.n_segmented, c.n_outlier
        st, en = np.empty(R, np.int32), np.empty(R, np.int32)
        gf, ci, sr = np.empty(n, np.uint8), np.empty(n, np.int32), np.empty(n, np.float32)
        sx, ox = np.empty((n, 4), np.float32), np.empty((no, 4), np.float32)
        L.check(self.lib.slio_lego_get_seg_info(self.h, L.iptr(st), L.iptr(en), L.u8ptr(gf),
                                                L.iptr(ci), L.fptr(sr), L.fptr(sx), L.fptr(ox)),
                "seg_info")
        return dict(orientation=np.array(c.orientation, np.float32), startRingIndex=st,
                    endRingIndex=en, segmentedCloudGroundFlag=gf, segmentedCloudColInd=ci,
                    segmentedCloudRange=sr, segmented_cloud=sx, outlier_cloud=ox)

    def features(self) -> dict:
        c = self.counts
        n = c.n_segmented
        dk = np.empty((n, 4), np.float32)
        cv, pk, lb = np.empty(n, np.float32), np.empty(n, np.uint8), np.empty(n, np.int32)
        io = L.SlioLegoImuOut()
        L.check(self.lib.slio_lego_get_features(self.h, L.fptr(dk), L.fptr(cv), L.u8ptr(pk),
                                                L.iptr(lb), C.byref(io)), "features")
        out = [np.empty((k, 4), np.float32) for k in (c.n_sharp, c.n_less_sharp, c.n_flat,
                                                       c.n_less_flat)]
        L.check(self.lib.slio_lego_get_clouds(self.h, *(L.fptr(v) for v in out)), "clouds")
        return dict(deskewed=dk, cloudCurvature=cv, cloudNeighborPicked=pk, cloudLabel=lb,
                    cornerPointsSharp=out[0], cornerPointsLessSharp=out[1], surfPointsFlat=out[2],
                    surfPointsLessFlat=out[3],
                    imu_out=dict(rpy_start=np.array(io.rpy_start), rpy_cur=np.array(io.rpy_cur),
                                 velo_from_start=np.array(io.velo_from_start),
                                 angular_from_start=np.array(io.angular_from_start),
                                 ang_last=np.array(io.ang_last),
                                 pointer_last_iteration=io.pointer_last_iteration))
