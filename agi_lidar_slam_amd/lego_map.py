"""LeGO-LOAM's mapping back-end (mapOptmization.cpp, transformFusion.cpp) on
the device: the slio_lmap_* entries of include/slio.h behind the reference's
member names.  ``LegoMapping(loop_closure=True)`` is the reference with
loopClosureEnableFlag = true: the recent-keyframe local map, performLoopClosure
and correctPoses; the factor graph (GTSAM) stays with the caller, behind the
``graph`` object.

Everything is in LeGO-LOAM's camera-like frame; poses are float32
``{rx, ry, rz, tx, ty, tz}``.  The stated departures (tie rule of the 5-NN,
in-voxel summation order, trigonometry in double, the GTSAM-free key pose,
the uncached keyframe transforms) are listed in slio.h and DESIGN.md §3.13.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import numpy as np

from . import _lib as L
from .lio_sam import icp_align_device, icp_align_lockstep

CORNER, SURF_TOTAL, SURF, OUTLIER, LOOP = 0, 1, 2, 3, 4
IMU_QUE_LENGTH = 200   # imuQueLength (utility.h)
SURROUNDING_KEYFRAME_SEARCH_NUM = 50     # surroundingKeyframeSearchNum (utility.h:92)
HISTORY_KEYFRAME_SEARCH_RADIUS = 5.0     # historyKeyframeSearchRadius (utility.h:94)
HISTORY_KEYFRAME_SEARCH_NUM = 25         # historyKeyframeSearchNum (utility.h:95)
HISTORY_KEYFRAME_FITNESS_SCORE = 0.3     # historyKeyframeFitnessScore (utility.h:96)
# performLoopClosure's ICP path when the caller names none.  The device loop:
# on the 16 x 1800 sequence's sizes it measured faster than the lockstep loop
# by more than the spread between runs
LOOP_ICP_LOCKSTEP_DEFAULT = False


class LegoLoopClosure(NamedTuple):
    """A closure performLoopClosure found: the factor's keys (latest,
    closest), its poses as GTSAM takes them ({x, y, z, roll, pitch, yaw} of
    tCorrect; the closest key as {tz, tx, ty, rz, rx, ry}), the noise score,
    and the ICP's iteration count and convergence state."""
    latest: int
    closest: int
    pose_from: np.ndarray
    pose_to: np.ndarray
    noise: float
    iterations: int
    state: int


def recent_keyframes(recent: list, latest_frame_id: int, nkeys: int,
                     search_num: int = SURROUNDING_KEYFRAME_SEARCH_NUM):
    """The recent-keyframe list of extractSurroundingKeyFrames (:1044-1089) as
    key numbers: (list, latestFrameID) after the call.  While the list holds
    fewer than search_num entries it is refilled whole, from the newest key
    back, each pushed to the front (so ascending), and latestFrameID stays as
    it is; once it holds search_num, a call with latestFrameID != nkeys - 1
    pops the oldest entry and appends the latest key -- also when that key
    already is the last entry, as on the first call after the list filled up."""
    recent = list(recent)
    if len(recent) < search_num:
        recent = list(range(max(nkeys - search_num, 0), nkeys))
    elif latest_frame_id != nkeys - 1:
        recent.pop(0)
        latest_frame_id = nkeys - 1
        recent.append(latest_frame_id)
    return recent, latest_frame_id


def _pose_voxel_grid4(pts: np.ndarray, leaf: float) -> np.ndarray:
    """pcl::VoxelGrid of a few PointXYZI poses in float32 (PCL 1.10
    applyFilter with downsample_all_data_): the voxel comes from x, y, z; all
    FOUR fields are averaged, a voxel's points summed in input order;
    centroids in ascending voxel index.  A leaf too small for the cloud passes
    it through.  (lio_sam._pose_voxel_grid with the intensity carried.)"""
    f = np.float32
    pts = np.ascontiguousarray(pts, f).reshape(-1, 4)
    if pts.shape[0] == 0:
        return pts.copy()
    inv = f(1.0) / f(leaf)
    xyz = pts[:, :3]
    mn, mx = xyz.min(axis=0), xyz.max(axis=0)
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    d = ((mx - mn) * inv).astype(np.int64) + 1
    if int(d[0]) * int(d[1]) * int(d[2]) > np.iinfo(np.int32).max:
        return pts.copy()
    div = max_b - min_b + 1
    ijk = (np.floor(xyz * inv) - min_b.astype(f)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    out = []
    for v in np.unique(idx):
        s = np.zeros(4, f)
        members = np.nonzero(idx == v)[0]
        for i in members:
            s = s + pts[i]
        out.append(s / f(len(members)))
    return np.array(out, f).reshape(-1, 4)


def extract_surrounding(key_poses3d, current_pos, existing_ids, radius: float = 50.0, pose_leaf: float = 1.0):
    """The host selection of extractSurroundingKeyFrames (:1101-1177).

    key_poses3d (N, 4) = cloudKeyPoses3D (x, y, z, intensity = key index),
    current_pos = currentRobotPosPoint, existing_ids =
    surroundingExistingKeyPosesID.  Returns (the updated id list,
    surroundingKeyPosesDS).  The radius search returns ascending float
    distance (ties: lower index; the test is `<`).  The VoxelGrid over the
    poses averages all four fields, and a downsampled pose's key is int() of
    the MEAN intensity of the poses in its voxel (:1127, :1157, :1165) -- a
    reference quirk that can name a key outside the radius; reproduced.  The
    list keeps the reference's order: stale ids erased in place, new keys
    appended in surroundingKeyPosesDS order."""
    f = np.float32
    kp = np.ascontiguousarray(key_poses3d, f).reshape(-1, 4)
    cur = np.asarray(current_pos, f).reshape(3)
    existing = [int(v) for v in existing_ids]
    if kp.shape[0] == 0:
        return existing, kp.copy()
    d = kp[:, :3] - cur
    sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    order = np.argsort(sq, kind="stable")
    order = order[sq[order] < f(radius) * f(radius)]
    ds = _pose_voxel_grid4(kp[order], pose_leaf)
    ds_ids = [int(v) for v in ds[:, 3]]   # (int) truncates
    existing = [k for k in existing if k in ds_ids]
    for k in ds_ids:
        if k not in existing:
            existing.append(k)
    return existing, ds


class TransformFusion:
    """transformFusion.cpp: the same transformAssociateToMap on the triple
    (transformBefMapped, transformAftMapped, transformSum)."""

    def __init__(self):
        self.lib = L.load()
        self.s = L.SlioLmapFusion()

    def laserOdometryHandler(self, transform_sum) -> np.ndarray:
        ts = np.ascontiguousarray(transform_sum, np.float32)
        L.check(self.lib.slio_lmap_fuse(C.byref(self.s), L.fptr(ts), None, None), "lmap_fuse")
        return np.array(self.s.transform_mapped, np.float32)

    def odomAftMappedHandler(self, aft, bef) -> None:
        a, b = np.ascontiguousarray(aft, np.float32), np.ascontiguousarray(bef, np.float32)
        L.check(self.lib.slio_lmap_fuse(C.byref(self.s), None, L.fptr(a), L.fptr(b)), "lmap_fuse")

    @property
    def transformMapped(self) -> np.ndarray:
        return np.array(self.s.transform_mapped, np.float32)


class LegoMapping:
    """mapOptmization's members and run() (:1807-1845) without loop closure,
    GTSAM, ROS or publishing."""

    def __init__(self, device: int = 0, max_points: int = 100000, grid_cell: float = 0.0,
                 loop_closure: bool = False, **kw):
        self.lib = L.load()
        self.loop_closure = bool(loop_closure)     # loopClosureEnableFlag (utility.h:68)
        self.keyTimes: list[float] = []            # cloudKeyPoses6D.time
        self.recentKeyFrames: list[int] = []       # recent*CloudKeyFrames, as key numbers
        self.latestFrameID = 0
        self.aLoopIsClosed = False
        self._corrected = None                     # the table graph.add_loop returned
        self.graph = None
        p = L.SlioLmapParams()
        L.check(self.lib.slio_lmap_params_default(C.byref(p)), "lmap_params_default")
        p.device, p.max_points, p.grid_cell = device, max_points, grid_cell
        for k, v in kw.items():
            if not hasattr(p, k):
                raise KeyError(k)
            setattr(p, k, v)
        self.params = p
        self.m = C.c_void_p()
        L.check(self.lib.slio_lmap_create(C.byref(self.m), C.byref(p)), "lmap_create")
        f = np.float32
        self.transformSum = np.zeros(6, f)
        self._tobe = np.zeros(6, f)
        self._bef = np.zeros(6, f)
        self._aft = np.zeros(6, f)
        self.timeLaserOdometry = 0.0
        self.timeLastProcessing = -1.0
        self.imuTime = np.zeros(IMU_QUE_LENGTH, np.float64)
        self.imuRoll = np.zeros(IMU_QUE_LENGTH, f)
        self.imuPitch = np.zeros(IMU_QUE_LENGTH, f)
        self.imuPointerLast, self.imuPointerFront = -1, 0
        self.cloudKeyPoses3D = np.zeros((0, 4), f)
        self._poses6 = np.zeros((0, 6), f)
        self.surroundingExistingKeyPosesID: list[int] = []
        self.currentRobotPosPoint = np.zeros(3, f)
        self.previousRobotPosPoint = np.zeros(3, f)
        self.map_counts = np.zeros(4, np.int64)    # corner concatenated / map, surf concatenated / map
        self.scan_counts = np.zeros(4, np.int64)   # cornerLastDS, surfTotalLastDS, surfLastDS, outlierLastDS
        self._degenerate, self._iterations = 0, 0
        self.trace: list[np.ndarray] = []          # lockstep: transformTobeMapped after every iteration
        self.saved_last = False
        self.tobe_associated = np.zeros(6, f)
        self._last = np.zeros(6, f)                # transformLast
        self.loop_counts = np.zeros(4, np.int64)

    def close(self):
        if self.m:
            self.lib.slio_lmap_destroy(self.m)
            self.m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------ properties
    transformTobeMapped = property(lambda self: self._tobe.copy())
    transformAftMapped = property(lambda self: self._aft.copy())
    transformBefMapped = property(lambda self: self._bef.copy())
    cloudKeyPoses6D = property(lambda self: self._poses6.copy())
    isDegenerate = property(lambda self: bool(self._degenerate))
    iterations = property(lambda self: self._iterations)

    def handle(self, which: int) -> C.c_void_p:
        """One of the mapper's four slio handles (CORNER, SURF_TOTAL, SURF,
        OUTLIER) for the library's getters."""
        h = C.c_void_p()
        L.check(self.lib.slio_lmap_get_handle(self.m, which, C.byref(h)), "lmap_get_handle")
        return h

    def scan(self, which: int) -> np.ndarray:
        h, n = self.handle(which), int(self.scan_counts[which])
        out = np.empty((3, n), np.float32)
        L.check(self.lib.slio_scan_download(h, L.fptr(out[0]), L.fptr(out[1]), L.fptr(out[2])), "scan_download")
        return np.ascontiguousarray(out.T)

    def map_points(self, kind: int) -> np.ndarray:
        """laserCloud{Corner,Surf}FromMapDS in output (id) order."""
        h = self.handle(CORNER if kind == 0 else SURF_TOTAL)
        cap = int(self.map_counts[1 + 2 * kind])
        out, ids, n = np.empty((3, cap), np.float32), np.empty(cap, np.uint32), C.c_int64()
        if cap == 0:
            return np.zeros((0, 3), np.float32)
        L.check(self.lib.slio_map_download(h, L.fptr(out[0]), L.fptr(out[1]), L.fptr(out[2]),
                                           ids.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(n)),
                "map_download")
        return np.ascontiguousarray(out[:, :n.value].T)

    def keyframe(self, which: int, key: int) -> np.ndarray:
        """Keyframe `key` of the CORNER, SURF or OUTLIER store (n, 3)."""
        h, n = self.handle(which), C.c_int64()
        self.lib.slio_s2m_kf_get(h, key, None, None, None, 0, C.byref(n))   # its size (ECAPACITY unless empty)
        out = np.empty((3, max(n.value, 1)), np.float32)
        L.check(self.lib.slio_s2m_kf_get(h, key, L.fptr(out[0]), L.fptr(out[1]), L.fptr(out[2]), out.shape[1],
                                         C.byref(n)), "s2m_kf_get")
        return np.ascontiguousarray(out[:, :n.value].T)

    def far_queries(self, kind: int) -> int:
        n = C.c_int64()
        L.check(self.lib.slio_far_queries(self.handle(CORNER if kind == 0 else SURF_TOTAL), C.byref(n)),
                "far_queries")
        return n.value

    # -------------------------------------------------------------- handlers
    def laserOdometryHandler(self, transform_sum, t: float) -> None:
        """transformSum as the front-end holds it (the reference's round trip
        through a quaternion message is ROS plumbing)."""
        self.transformSum = np.array(transform_sum, np.float32).reshape(6)
        self.timeLaserOdometry = float(t)

    def imuHandler(self, t: float, roll: float, pitch: float) -> None:
        self.imuPointerLast = (self.imuPointerLast + 1) % IMU_QUE_LENGTH
        self.imuTime[self.imuPointerLast] = t
        self.imuRoll[self.imuPointerLast] = roll
        self.imuPitch[self.imuPointerLast] = pitch

    # ---------------------------------------------------------------- stages
    def transformAssociateToMap(self) -> np.ndarray:
        out = np.empty(6, np.float32)
        L.check(self.lib.slio_lmap_associate_to_map(L.fptr(self.transformSum), L.fptr(self._bef),
                                                    L.fptr(self._aft), L.fptr(out)), "lmap_associate_to_map")
        self._tobe = out
        self.tobe_associated = out.copy()   # transformTobeMapped before the optimisation
        return out.copy()

    def transformUpdate(self) -> None:
        front = C.c_int32(self.imuPointerFront)
        L.check(self.lib.slio_lmap_transform_update(
            L.fptr(self._tobe), L.fptr(self.transformSum), self.timeLaserOdometry, self.params.scan_period,
            L.dptr(self.imuTime), L.fptr(self.imuRoll), L.fptr(self.imuPitch), IMU_QUE_LENGTH,
            self.imuPointerLast, C.byref(front), L.fptr(self._bef), L.fptr(self._aft)), "lmap_transform_update")
        self.imuPointerFront = front.value

    def extractSurroundingKeyFrames(self) -> np.ndarray:
        """:1098-1194.  Without key poses the reference returns at once and
        the maps stay empty (clearCloud): an empty key list here."""
        nkeys = self.cloudKeyPoses3D.shape[0]
        if nkeys and self.loop_closure:      # :1042-1097
            self.recentKeyFrames, self.latestFrameID = recent_keyframes(self.recentKeyFrames, self.latestFrameID,
                                                                        nkeys)
            keys = np.array(self.recentKeyFrames, np.int32)
        else:
            if nkeys:
                self.surroundingExistingKeyPosesID, _ = extract_surrounding(
                    self.cloudKeyPoses3D, self.currentRobotPosPoint, self.surroundingExistingKeyPosesID,
                    self.params.search_radius, self.params.pose_leaf)
            keys = np.array(self.surroundingExistingKeyPosesID, np.int32)
        L.check(self.lib.slio_lmap_extract(self.m, L.iptr(keys), keys.size, L.i64ptr(self.map_counts)),
                "lmap_extract")
        return self.map_counts.copy()

    def downsampleCurrentScan(self, front_end=None, clouds=None) -> np.ndarray:
        """From the front-end's device clouds (front_end: a LegoFrontEnd), or
        from three host clouds (clouds = (corner, surf, outlier), each n x 4)."""
        if front_end is not None:
            L.check(self.lib.slio_lmap_feed_lego(self.m, front_end.h, L.i64ptr(self.scan_counts)), "lmap_feed_lego")
        else:
            a = [np.ascontiguousarray(v, np.float32).reshape(-1, 4) for v in clouds]
            args = []
            for v in a:
                args += [L.fptr(v), v.shape[0]]
            L.check(self.lib.slio_lmap_feed_host(self.m, *args, L.i64ptr(self.scan_counts)), "lmap_feed_host")
        return self.scan_counts.copy()

    def coeffs(self, kind: int, transform, want_nsel: bool = True):
        tf = np.ascontiguousarray(transform, np.float32)
        nsel = C.c_int64(-1)
        L.check(self.lib.slio_lmap_coeffs(self.m, kind, L.fptr(tf), C.byref(nsel) if want_nsel else None),
                "lmap_coeffs")
        return nsel.value

    def get_coeffs(self, kind: int, n: int):
        coeff, sel = np.empty((n, 4), np.float32), np.empty(n, np.uint8)
        L.check(self.lib.slio_lmap_get_coeffs(self.m, kind, L.fptr(coeff), L.u8ptr(sel)), "lmap_get_coeffs")
        return coeff, sel

    def normal_equations(self):
        AtA, AtB, nsel = np.empty(36, np.float32), np.empty(6, np.float32), C.c_int64()
        L.check(self.lib.slio_lmap_normal_equations(self.m, L.fptr(AtA), L.fptr(AtB), C.byref(nsel)),
                "lmap_normal_equations")
        return AtA, AtB, nsel.value

    def optimize(self, transform):
        """slio_lmap_optimize: (transform, iterations, isDegenerate)."""
        tf = np.array(transform, np.float32).reshape(6)
        it, deg = C.c_int32(), C.c_int32()
        L.check(self.lib.slio_lmap_optimize(self.m, L.fptr(tf), C.byref(it), C.byref(deg)), "lmap_optimize")
        return tf, it.value, deg.value

    def optimize_lockstep(self, transform):
        """The same loop through the single-stage entries and
        slio_s2m_lm_step; also returns the transform after every iteration."""
        tf = np.array(transform, np.float32).reshape(6)
        matP, deg, conv = np.zeros(36, np.float32), C.c_int(0), C.c_int(0)
        trace, iters = [], 0
        if not (self.map_counts[1] > 10 and self.map_counts[3] > 100):
            return tf, 0, 0, trace
        for it in range(self.params.max_iterations):
            self.coeffs(0, tf, want_nsel=False)
            self.coeffs(1, tf, want_nsel=False)
            AtA, AtB, nsel = self.normal_equations()
            rc = self.lib.slio_s2m_lm_step(L.fptr(AtA), L.fptr(AtB), nsel, it, L.fptr(tf), C.byref(deg),
                                           L.fptr(matP), C.byref(conv))
            if rc < 0:
                L.check(rc, "s2m_lm_step")
            iters = it + 1
            trace.append(tf.copy())
            if conv.value:
                break
        return tf, iters, deg.value, trace

    def scan2MapOptimization(self, lockstep: bool = False) -> None:
        """:1603-1626: the loop, then transformUpdate, only with more than 10
        corner and 100 surf map points."""
        self._iterations = 0
        self.trace = []
        if self.map_counts[1] > 10 and self.map_counts[3] > 100:
            if lockstep:
                self._tobe, self._iterations, self._degenerate, self.trace = self.optimize_lockstep(self._tobe)
            else:
                self._tobe, self._iterations, self._degenerate = self.optimize(self._tobe)
            self.transformUpdate()

    def saveKeyFramesAndFactor(self) -> bool:
        """:1628-1767.  The key pose is transformTobeMapped, or what
        graph.add_keyframe(key, pose_from6, pose_to6) returns: pose_from6 =
        transformLast and pose_to6 = transformAftMapped, both {rx, ry, rz, tx,
        ty, tz} (the reference hands GTSAM their {rz, rx, ry, tz, tx, ty},
        :1656-1693); for key 0 pose_from6 is None and pose_to6 is
        transformTobeMapped (the prior factor)."""
        self.currentRobotPosPoint = self._aft[3:6].copy()
        save = C.c_int()
        nkeys = self.cloudKeyPoses3D.shape[0]
        L.check(self.lib.slio_lmap_keyframe_decision(L.fptr(self.previousRobotPosPoint),
                                                     L.fptr(self.currentRobotPosPoint), nkeys, 0.3,
                                                     C.byref(save)), "lmap_keyframe_decision")
        self.saved_last = bool(save.value)
        if not save.value:
            return False
        self.previousRobotPosPoint = self.currentRobotPosPoint.copy()
        pose = self._tobe.copy()
        if self.graph is not None:
            est = self.graph.add_keyframe(nkeys, self._last.copy() if nkeys else None,
                                          self._aft.copy() if nkeys else self._tobe.copy())
            pose = np.array(est, np.float32).reshape(6)
        self._last = pose.copy() if nkeys else self._tobe.copy()    # transformLast (:1695-1696, :1745-1748)
        self.keyTimes.append(float(self.timeLaserOdometry))         # thisPose6D.time (:1734)
        p3 = np.array([pose[3], pose[4], pose[5], nkeys], np.float32)
        self.cloudKeyPoses3D = np.vstack([self.cloudKeyPoses3D, p3[None]])
        self._poses6 = np.vstack([self._poses6, pose[None]])
        if nkeys + 1 > 1:   # :1737-1749
            self._aft = pose.copy()
            if self.graph is not None:
                self._tobe = pose.copy()
        key = C.c_int32()
        L.check(self.lib.slio_lmap_save_keyframe(self.m, L.fptr(pose), C.byref(key)), "lmap_save_keyframe")
        assert key.value == nkeys
        return True

    def run(self, front_end, t: float, lockstep: bool = False) -> bool:
        """run() :1807-1845 after a sweep of `front_end` (a LegoFrontEnd with
        odometry) stamped t.  False when that sweep did not publish or the
        mappingProcessInterval gate holds the call back."""
        v = L.SlioLegoLastView()
        L.check(self.lib.slio_lego_odom_last_view(front_end.h, C.byref(v)), "odom_last_view")
        if not v.published:
            return False
        self.laserOdometryHandler(front_end.odometry_state()["transform_sum"], t)
        if not (self.timeLaserOdometry - self.timeLastProcessing >= float(np.float32(self.params.mapping_interval))):
            return False
        self.timeLastProcessing = self.timeLaserOdometry
        self.transformAssociateToMap()
        self.extractSurroundingKeyFrames()
        self.downsampleCurrentScan(front_end)
        self.scan2MapOptimization(lockstep=lockstep)
        self.saveKeyFramesAndFactor()
        self.correctPoses()
        return True

    # ------------------------------------------------------------ loop closure
    def set_key_poses(self, poses6) -> None:
        """slio_lmap_set_key_poses: the whole key-pose table ({rx, ry, rz, tx,
        ty, tz} per key); cloudKeyPoses3D / 6D follow."""
        t = np.ascontiguousarray(np.asarray(poses6, np.float32).reshape(-1, 6))
        L.check(self.lib.slio_lmap_set_key_poses(self.m, L.fptr(t), t.shape[0]), "lmap_set_key_poses")
        self._poses6 = t.copy()
        self.cloudKeyPoses3D[:, :3] = t[:, 3:6]

    def correctPoses(self) -> None:
        """:1769-1798: after a closed loop the recent list is cleared and every
        key pose takes the graph's estimate (the table graph.add_loop
        returned; the isamCurrentEstimate -> table mapping is INTEGRATION.md's)."""
        if not self.aLoopIsClosed:
            return
        self.recentKeyFrames = []
        if self._corrected is not None:
            self.set_key_poses(self._corrected)
            self._corrected = None
        self.aLoopIsClosed = False

    def detectLoopClosure(self) -> int:
        """:863-887: the closest history key, or -1."""
        xyz = np.ascontiguousarray(self.cloudKeyPoses3D[:, :3], np.float32)
        times = np.ascontiguousarray(self.keyTimes, np.float64)
        cur = np.ascontiguousarray(self.currentRobotPosPoint, np.float32)
        out = C.c_int32(-1)
        L.check(self.lib.slio_lmap_detect_loop(L.fptr(xyz), L.dptr(times), xyz.shape[0], L.fptr(cur),
                                               float(self.timeLaserOdometry), HISTORY_KEYFRAME_SEARCH_RADIUS, 30.0,
                                               C.byref(out)), "lmap_detect_loop")
        return out.value

    def loop_clouds(self, latest: int, closest: int, search_num: int = HISTORY_KEYFRAME_SEARCH_NUM,
                    leaf: float = 0.4) -> np.ndarray:
        """slio_lmap_loop_clouds: {source concatenated, source kept, target
        concatenated, target points}."""
        self.loop_counts = np.zeros(4, np.int64)
        L.check(self.lib.slio_lmap_loop_clouds(self.m, latest, closest, search_num, leaf,
                                               L.i64ptr(self.loop_counts)), "lmap_loop_clouds")
        return self.loop_counts.copy()

    def loop_correction(self, final_T, latest: int, closest: int, fitness: float):
        """slio_lmap_loop_correction: (pose_from, pose_to, noise)."""
        T = np.ascontiguousarray(np.asarray(final_T, np.float32).reshape(16))
        pf, pt, noise = np.empty(6, np.float32), np.empty(6, np.float32), C.c_float()
        a, b = np.ascontiguousarray(self._poses6[latest]), np.ascontiguousarray(self._poses6[closest])
        L.check(self.lib.slio_lmap_loop_correction(L.fptr(T), L.fptr(a), L.fptr(b), float(fitness), L.fptr(pf),
                                                   L.fptr(pt), C.byref(noise)), "lmap_loop_correction")
        return pf, pt, noise.value

    def performLoopClosure(self, graph=None, lockstep: Optional[bool] = None, batch: int = 0,
                           search_num: int = HISTORY_KEYFRAME_SEARCH_NUM) -> Optional[LegoLoopClosure]:
        """:944-1023, called between run() calls (the reference runs it in a
        1 Hz thread under `mtx`).  None where the reference returns early: no
        key yet, no candidate, ICP not converged or its fitness above
        historyKeyframeFitnessScore.  The ICP (:957-971, max distance 100, 100
        iterations, 1e-6, 1e-6) runs as slio_icp_align on the loop handle, or
        as the lockstep loop (lockstep=True; None: the module's default).
        With a `graph` (default: self.graph), graph.add_loop(closure) adds the
        factor and returns the corrected key-pose table, which the next run()'s
        correctPoses writes; without one the closure is only returned."""
        if self.cloudKeyPoses3D.shape[0] == 0:
            return None
        closest = self.detectLoopClosure()
        if closest < 0:
            return None
        latest = self.cloudKeyPoses3D.shape[0] - 1
        self.loop_clouds(latest, closest, search_num)
        if lockstep is None:
            lockstep = LOOP_ICP_LOCKSTEP_DEFAULT
        h = self.handle(LOOP)
        if lockstep:
            res = icp_align_lockstep(self.lib, h, 100.0, max_iterations=100, owner=self)
        else:
            res = icp_align_device(self.lib, h, 100.0, batch=batch, max_iterations=100, owner=self)
        conv, T, fitness, iters, state = res
        self.loop_final_T, self.loop_fitness = T, fitness
        if not conv or fitness > float(np.float32(HISTORY_KEYFRAME_FITNESS_SCORE)):
            return None
        pf, pt, noise = self.loop_correction(T, latest, closest, fitness)
        closure = LegoLoopClosure(latest, closest, pf, pt, noise, iters, state)
        graph = self.graph if graph is None else graph
        if graph is not None:
            table = graph.add_loop(closure)
            self._corrected = np.array(table, np.float32).reshape(-1, 6)
            self.aLoopIsClosed = True
        return closure
