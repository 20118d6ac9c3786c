"""LIO-SAM scan-to-map optimisation on the MI355X path.

Mirrors ``src/LIO-SAM/src/mapOptmization.cpp`` scan2MapOptimization
(:1706-1740) and the functions it calls: cornerOptimization (:1303-1432),
surfOptimization (:1438-1515), combineOptimizationCoeffs (:1517-1543) and
LMOptimization (:1552-1700).  The per-point work (pointAssociateToMap, exact
5-NN in the corner / surf local maps, line and plane fits, the LM rows and
the normal equations) runs on the device through libslio; the 6x6 step is
host C++ (slio_s2m_lm_step).  The local map the solve runs against is made
on the device too: the keyframe clouds (saveKeyFramesAndFactor :2069-2077)
live in the handles' keyframe stores, downsampleCurrentScan (:1276-1288) and
extractCloud (:1204-1251) run there, and extractNearby's key selection
(:1152-1193, a few hundred poses) is host numpy (extract_nearby).
transformUpdate's IMU blending (:1742-1781) and the factor graph are out of
scope (SURVEY.md §8f-4 names the scan-to-map core).

Loop closure (performLoopClosure :725-826) runs on the same keyframe stores:
detect_loop_closure_distance (:836-873, host numpy), loopFindNearKeyframes
(:945-972) and pcl::IterativeClosestPoint (:766-780) on the device
(slio_s2m_loop_cloud, slio_icp_correspond) with the rigid fit and PCL's
convergence rules on the host (slio_icp_step).  detectLoopClosureExternal
(:883-938, "not used yet" in the reference) and the GTSAM between-factor the
result feeds (:800-822) stay out of scope: perform_loop_closure returns what
the factor is made from.
"""
from __future__ import annotations

import ctypes as C
import math
import time
from typing import NamedTuple, Optional

import numpy as np

from . import _lib as L

EDGE_FEATURE_MIN_VALID_NUM = 10    # params.yaml edgeFeatureMinValidNum
SURF_FEATURE_MIN_VALID_NUM = 100   # params.yaml surfFeatureMinValidNum


def _pose_voxel_grid(pts: np.ndarray, leaf: float) -> np.ndarray:
    """pcl::VoxelGrid of a few poses in float32 (PCL 1.10 applyFilter):
    centroids in ascending voxel index, a voxel's points summed in input
    order.  A leaf too small for the cloud passes it through."""
    f = np.float32
    if pts.shape[0] == 0:
        return pts.copy()
    inv = f(1.0) / f(leaf)
    mn, mx = pts.min(axis=0), pts.max(axis=0)
    min_b = np.floor(mn * inv).astype(np.int64)
    max_b = np.floor(mx * inv).astype(np.int64)
    d = ((mx - mn) * inv).astype(np.int64) + 1
    if int(d[0]) * int(d[1]) * int(d[2]) > np.iinfo(np.int32).max:
        return pts.copy()
    div = max_b - min_b + 1
    ijk = (np.floor(pts * inv) - min_b.astype(f)).astype(np.int64)
    idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
    out = []
    for v in np.unique(idx):
        s = np.zeros(3, f)
        members = np.nonzero(idx == v)[0]
        for i in members:
            s = s + pts[i]
        out.append(s / f(len(members)))
    return np.array(out, f).reshape(-1, 3)


def extract_nearby(key_poses3d, key_times, t_cur: float, radius: float = 50.0, density: float = 2.0) -> np.ndarray:
    """The keyframes extractNearby (:1152-1193) hands to extractCloud, after
    extractCloud's own distance check (:1211), as a list of key indices for
    ScanToMap.extract_cloud.  Host numpy: a few hundred poses.

    key_poses3d (N, 3) = cloudKeyPoses3D, key_times (N,) = cloudKeyPoses6D's
    stamps, t_cur = timeLaserInfoCur, radius = surroundingKeyframeSearchRadius,
    density = surroundingKeyframeDensity.  Steps, in float32 as PCL:
    the poses within `radius` of the last one in ascending distance (:1164-1172);
    their VoxelGrid with leaf `density`, one centroid per voxel in ascending
    voxel index (:1175-1176); each centroid replaced by the index of the key
    pose nearest to it (:1179-1183); then the keys of the last 10 s, newest
    first, appended with duplicates kept (:1186-1193).  An entry whose point --
    the centroid, or the tail key's pose -- is farther than `radius` from the
    last pose is dropped (:1211).

    FLANN's order among poses at exactly equal distance (and whether a pose at
    exactly `radius` counts) is not pinned by anything here: ties go to the
    lower index, and the radius test is `<`.  Only the in-voxel summation
    order, hence the last bits of a centroid, depends on it."""
    f = np.float32
    P = np.ascontiguousarray(np.asarray(key_poses3d, dtype=f).reshape(-1, 3))
    T = np.asarray(key_times, dtype=np.float64).reshape(-1)
    n = P.shape[0]
    if n == 0:
        return np.zeros(0, np.int32)

    def sqd(a, b):
        d = a - b
        return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]

    back = P[-1]
    d2 = sqd(P, back)
    near = np.nonzero(d2 < f(radius) * f(radius))[0]
    near = near[np.argsort(d2[near], kind="stable")]
    cents = _pose_voxel_grid(P[near], density)
    keys, pts = [], []
    for c in cents:
        keys.append(int(np.argmin(sqd(P, c))))
        pts.append(c)
    for i in range(n - 1, -1, -1):
        if t_cur - T[i] < 10.0:
            keys.append(i)
            pts.append(P[i])
        else:
            break
    out = [k for k, p in zip(keys, pts) if not np.sqrt(sqd(np.asarray(p, f), back)) > f(radius)]
    return np.array(out, np.int32)


def detect_loop_closure_distance(key_poses3d, key_times, t_cur: float, loop_index_container,
                                 radius: float = 15.0, time_diff: float = 30.0):
    """detectLoopClosureDistance (:836-873): (loopKeyCur, loopKeyPre) or None.
    Host numpy, float32 distances as PCL.

    loopKeyCur is the newest key; None when it already is in
    loop_index_container (:842-843).  The poses within `radius`
    (historyKeyframeSearchRadius) of the newest one are taken in ascending
    distance, ties to the lower index and the radius test `<` as in
    extract_nearby; the first whose stamp differs from t_cur
    (timeLaserInfoCur) by more than `time_diff`
    (historyKeyframeSearchTimeDiff) is loopKeyPre (:856-864).  None when
    nothing qualifies or the match is the newest key itself (:867)."""
    f = np.float32
    P = np.ascontiguousarray(np.asarray(key_poses3d, dtype=f).reshape(-1, 3))
    T = np.asarray(key_times, dtype=np.float64).reshape(-1)
    n = P.shape[0]
    if n == 0:
        return None
    cur = n - 1
    if cur in loop_index_container:
        return None
    d = P - P[-1]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    near = np.nonzero(d2 < f(radius) * f(radius))[0]
    near = near[np.argsort(d2[near], kind="stable")]
    pre = -1
    for i in near:
        if abs(T[i] - t_cur) > time_diff:
            pre = int(i)
            break
    if pre == -1 or pre == cur:
        return None
    return cur, pre


def pose_affine(pose6) -> np.ndarray:
    """pcl::getTransformation(x, y, z, roll, pitch, yaw) of pose6 = (roll,
    pitch, yaw, x, y, z) as a float32 4x4 (pclPointToAffine3f :443-447), the
    arithmetic of the device path's assembly: float products of correctly
    rounded float sines and cosines."""
    f = np.float32
    roll, pitch, yaw, x, y, z = (f(v) for v in np.asarray(pose6, dtype=f).reshape(6))
    A, B = f(math.cos(float(yaw))), f(math.sin(float(yaw)))
    Cc, D = f(math.cos(float(pitch))), f(math.sin(float(pitch)))
    E, F = f(math.cos(float(roll))), f(math.sin(float(roll)))
    DE, DF = D * E, D * F
    return np.array([[A * Cc, A * DF - B * E, B * F + A * DE, x],
                     [B * Cc, A * E + B * DF, B * DE - A * F, y],
                     [-D, Cc * F, Cc * E, z],
                     [0, 0, 0, 1]], dtype=f)


class LoopClosure(NamedTuple):
    """What performLoopClosure (:796-825) makes its between-factor from."""
    pair: tuple            # (loopKeyCur, loopKeyPre)
    pose_from: np.ndarray  # tCorrect = icp result * pose(loopKeyCur): x, y, z, roll, pitch, yaw
    pose_to: np.ndarray    # pose(loopKeyPre): x, y, z, roll, pitch, yaw
    noise: float           # icp.getFitnessScore(), the factor's six variances
    iterations: int


def _handle(max_points: int, grid_cell: float, device: int = 0):
    lib = L.load()
    p = L.SlioParams()
    L.check(lib.slio_params_default(C.byref(p)), "params")
    p.device, p.max_points, p.grid_cell = device, max_points, grid_cell
    h = C.c_void_p()
    L.check(lib.slio_create(C.byref(h), C.byref(p)), "create")
    return h


def _upload(lib, fn, h, pts):
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
    x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    L.check(fn(h, L.fptr(x), L.fptr(y), L.fptr(z), pts.shape[0]), fn.__name__)
    return pts.shape[0]


DBL_MAX = float(np.finfo(np.float64).max)


def _icp_params(lib, max_iterations=None):
    prm = L.SlioIcpParams()
    L.check(lib.slio_icp_params_default(C.byref(prm)), "icp params")
    if max_iterations is not None:
        prm.max_iterations = int(max_iterations)
    return prm


def icp_align_device(lib, h, max_corr_dist: float, guess=None, batch: int = 0, max_iterations=None, owner=None):
    """slio_icp_align on handle h (map = target, scan = source): icp.align and
    getFitnessScore with the loop on the device.  Returns (converged, final_T
    4x4 float32, fitness, iterations, convergence_state); `owner` (optional)
    receives icp_far_first and icp_state."""
    prm, st = _icp_params(lib, max_iterations), L.SlioIcpState()
    g = None if guess is None else np.ascontiguousarray(np.asarray(guess, dtype=np.float32).reshape(16))
    fit, far = C.c_double(), C.c_int64()
    L.check(lib.slio_icp_align(h, C.byref(prm), None if g is None else L.fptr(g), float(max_corr_dist), int(batch),
                               C.byref(st), C.byref(fit), C.byref(far)), "icp align")
    if owner is not None:
        owner.icp_far_first, owner.icp_state = far.value, st
    final_T = np.array(st.final_T, dtype=np.float32).reshape(4, 4)
    return bool(st.converged), final_T, fit.value, int(st.iterations), int(st.convergence_state)


def icp_align_lockstep(lib, h, max_corr_dist: float, guess=None, max_iterations=None, owner=None):
    """The same alignment with one slio_icp_correspond launch, one readback
    and one host slio_icp_step per iteration (ScanToMap.icp_align's loop on any
    handle)."""
    prm, st = _icp_params(lib, max_iterations), L.SlioIcpState()
    g = None if guess is None else np.ascontiguousarray(np.asarray(guess, dtype=np.float32).reshape(16))
    L.check(lib.slio_icp_state_init(C.byref(st), None if g is None else L.fptr(g)), "icp state")
    T = np.array(st.final_T, dtype=np.float32)
    sums, nc = np.zeros(16, np.float64), C.c_int64()
    delta, done = np.zeros(16, np.float32), C.c_int(0)
    from_scan, far_first = 1, 0
    while True:
        L.check(lib.slio_icp_correspond(h, L.fptr(T), from_scan, float(max_corr_dist), L.dptr(sums), C.byref(nc)),
                "icp correspond")
        if from_scan:
            far = C.c_int64()
            L.check(lib.slio_icp_far_queries(h, C.byref(far)), "icp far queries")
            far_first = far.value
        L.check(lib.slio_icp_step(L.dptr(sums), nc.value, C.byref(prm), C.byref(st), L.fptr(delta), C.byref(done)),
                "icp step")
        if done.value:
            break
        T, from_scan = delta, 0
    final_T = np.array(st.final_T, dtype=np.float32).reshape(4, 4)
    L.check(lib.slio_icp_correspond(h, L.fptr(np.ascontiguousarray(final_T.reshape(16))), 1, math.inf, L.dptr(sums),
                                    C.byref(nc)), "icp fitness")
    fitness = float(sums[15]) / nc.value if nc.value > 0 else DBL_MAX
    if owner is not None:
        owner.icp_far_first, owner.icp_state = far_first, st
    return bool(st.converged), final_T, fitness, int(st.iterations), int(st.convergence_state)


class ScanToMap:
    """kdtreeCornerFromMap / kdtreeSurfFromMap and the scan-to-map solve."""

    def __init__(self, max_points: int = 200000, grid_cell: float = 1.0, device: int = 0):
        self.lib = L.load()
        self.hc = _handle(max_points, grid_cell, device)
        self.hs = _handle(max_points, grid_cell, device)
        self.hl = None   # loop closure: map = prevKeyframeCloud, scan = cureKeyframeCloud
        self._handle_args = (max_points, grid_cell, device)
        self.icp_far_first = 0
        self.icp_pass_ms = []
        self.n_corner = self.n_surf = 0
        self.isDegenerate = C.c_int(0)
        self.matP = np.zeros(36, np.float32)
        self.iterations = 0

    def close(self):
        for h in (self.hc, self.hs, getattr(self, "hl", None)):
            if h:
                self.lib.slio_destroy(h)
        self.hc = self.hs = self.hl = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_maps(self, corner_from_map_ds: np.ndarray, surf_from_map_ds: np.ndarray) -> None:
        """kdtree{Corner,Surf}FromMap->setInputCloud (:1716-1717)."""
        _upload(self.lib, self.lib.slio_map_upload, self.hc, corner_from_map_ds)
        _upload(self.lib, self.lib.slio_map_upload, self.hs, surf_from_map_ds)

    def set_scan(self, corner_last_ds: np.ndarray, surf_last_ds: np.ndarray) -> None:
        """laserCloud{Corner,Surf}LastDS of the current frame."""
        self.n_corner = _upload(self.lib, self.lib.slio_scan_upload, self.hc, corner_last_ds)
        self.n_surf = _upload(self.lib, self.lib.slio_scan_upload, self.hs, surf_last_ds)

    def downsample_current_scan(self, corner_last: np.ndarray, surf_last: np.ndarray,
                                corner_leaf: float = 0.2, surf_leaf: float = 0.4):
        """downsampleCurrentScan (:1276-1288): laserCloud{Corner,Surf}Last through
        downSizeFilterCorner / downSizeFilterSurf (mappingCornerLeafSize 0.2,
        mappingSurfLeafSize 0.4) on the device; the results are the handles'
        scans (laserCloud*LastDS).  Returns their sizes."""
        out = []
        for h, pts, leaf in ((self.hc, corner_last, corner_leaf), (self.hs, surf_last, surf_leaf)):
            pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
            x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
            n = C.c_int64()
            L.check(self.lib.slio_scan_upload_voxel(h, L.fptr(x), L.fptr(y), L.fptr(z), pts.shape[0], leaf,
                                                    C.byref(n)), "downsampleCurrentScan")
            out.append(n.value)
        self.n_corner, self.n_surf = out
        return self.n_corner, self.n_surf

    def save_keyframe(self) -> int:
        """saveKeyFramesAndFactor's cloud part (:2069-2077): the current
        laserCloud{Corner,Surf}LastDS become the next keyframe's clouds (device
        to device).  Returns the keyframe's index."""
        kc, ks = C.c_int32(), C.c_int32()
        L.check(self.lib.slio_s2m_kf_push_scan(self.hc, C.byref(kc)), "save_keyframe (corner)")
        L.check(self.lib.slio_s2m_kf_push_scan(self.hs, C.byref(ks)), "save_keyframe (surf)")
        if kc.value != ks.value:
            raise L.SlioError(f"save_keyframe: corner / surf stores out of step ({kc.value} / {ks.value})")
        return kc.value

    def push_keyframe(self, corner: np.ndarray, surf: np.ndarray) -> int:
        """A keyframe from host clouds in the LiDAR frame (e.g. a saved map)."""
        keys = []
        for h, pts in ((self.hc, corner), (self.hs, surf)):
            pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 3))
            x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
            k = C.c_int32()
            L.check(self.lib.slio_s2m_kf_push(h, L.fptr(x), L.fptr(y), L.fptr(z), pts.shape[0], C.byref(k)),
                    "push_keyframe")
            keys.append(k.value)
        if keys[0] != keys[1]:
            raise L.SlioError(f"push_keyframe: corner / surf stores out of step ({keys[0]} / {keys[1]})")
        return keys[0]

    def extract_cloud(self, key_ind, poses6, corner_leaf: float = 0.2, surf_leaf: float = 0.4):
        """extractCloud (:1204-1251): keyframes key_ind[i] at poses6[i] (roll,
        pitch, yaw, x, y, z) transformed, concatenated in list order and
        downsampled into laserCloud{Corner,Surf}FromMapDS, which become the
        handles' maps -- all on the device.  Returns ((corner points
        concatenated, corner map points), (surf ..., surf ...))."""
        key = np.ascontiguousarray(np.asarray(key_ind, dtype=np.int32).reshape(-1))
        poses = np.ascontiguousarray(np.asarray(poses6, dtype=np.float32).reshape(-1, 6))
        if poses.shape[0] != key.shape[0]:
            raise ValueError("extract_cloud: one pose per selected keyframe")
        out = []
        for h, leaf in ((self.hc, corner_leaf), (self.hs, surf_leaf)):
            cnt = np.zeros(2, np.int64)
            L.check(self.lib.slio_s2m_map_from_keyframes(h, L.iptr(key), L.fptr(poses), key.shape[0], leaf,
                                                         L.i64ptr(cnt)), "extractCloud")
            out.append((int(cnt[0]), int(cnt[1])))
        return tuple(out)

    def clear_keyframes(self) -> None:
        for h in (self.hc, self.hs):
            L.check(self.lib.slio_s2m_kf_clear(h), "clear_keyframes")

    def loop_handle(self):
        """The third handle (created on first use, freed in close): its map is
        the loop closure's target, its scan the source."""
        if self.hl is None:
            self.hl = _handle(*self._handle_args)
        return self.hl

    def loop_find_near_keyframes(self, key: int, search_num: int, poses6_all, as_scan: bool,
                                 leaf: float = 0.4) -> int:
        """loopFindNearKeyframes (:945-972): keyframes key - search_num ..
        key + search_num clipped to the store, corner then surf of each at its
        own pose poses6_all[k] (roll, pitch, yaw, x, y, z), through
        downSizeFilterICP (mappingICPSize) -- on the device, into the loop
        handle's scan (as_scan) or map.  Returns the cloud's size."""
        nk = C.c_int32()
        L.check(self.lib.slio_s2m_kf_info(self.hc, C.byref(nk), None), "loopFindNearKeyframes")
        poses_all = np.asarray(poses6_all, dtype=np.float32).reshape(-1, 6)
        n_keys = min(nk.value, poses_all.shape[0])
        keys = np.array([k for k in range(key - search_num, key + search_num + 1) if 0 <= k < n_keys], np.int32)
        poses = np.ascontiguousarray(poses_all[keys]) if keys.size else np.zeros((0, 6), np.float32)
        cnt = np.zeros(2, np.int64)
        L.check(self.lib.slio_s2m_loop_cloud(self.loop_handle(), self.hc, self.hs, L.iptr(keys), L.fptr(poses),
                                             keys.shape[0], leaf, 1 if as_scan else 0, L.i64ptr(cnt)),
                "loopFindNearKeyframes")
        return int(cnt[1])

    def icp_align(self, max_corr_dist: float, guess: Optional[np.ndarray] = None):
        """icp.align (:766-778) then getFitnessScore (:780) on the loop handle
        (map = target, scan = source): one slio_icp_correspond launch and one
        host slio_icp_step per iteration.  Returns (converged, final_T 4x4
        float32, fitness, iterations, convergence_state); icp_far_first keeps
        the first pass's far-query count, icp_pass_ms the host wall clock of
        every slio_icp_correspond call (scripts/bench_aux.py s2m_loop)."""
        lib, h = self.lib, self.loop_handle()
        prm, st = L.SlioIcpParams(), L.SlioIcpState()
        L.check(lib.slio_icp_params_default(C.byref(prm)), "icp params")
        g = None if guess is None else np.ascontiguousarray(np.asarray(guess, dtype=np.float32).reshape(16))
        L.check(lib.slio_icp_state_init(C.byref(st), None if g is None else L.fptr(g)), "icp state")
        T = np.array(st.final_T, dtype=np.float32)
        sums, nc = np.zeros(16, np.float64), C.c_int64()
        delta, done = np.zeros(16, np.float32), C.c_int(0)
        from_scan = 1
        self.icp_pass_ms = []
        while True:
            t0 = time.perf_counter()
            L.check(lib.slio_icp_correspond(h, L.fptr(T), from_scan, float(max_corr_dist), L.dptr(sums),
                                            C.byref(nc)), "icp correspond")
            self.icp_pass_ms.append((time.perf_counter() - t0) * 1e3)
            if from_scan:
                far = C.c_int64()
                L.check(lib.slio_icp_far_queries(h, C.byref(far)), "icp far queries")
                self.icp_far_first = far.value
            L.check(lib.slio_icp_step(L.dptr(sums), nc.value, C.byref(prm), C.byref(st), L.fptr(delta),
                                      C.byref(done)), "icp step")
            if done.value:
                break
            T, from_scan = delta, 0
        final_T = np.array(st.final_T, dtype=np.float32).reshape(4, 4)
        L.check(lib.slio_icp_correspond(h, L.fptr(np.ascontiguousarray(final_T.reshape(16))), 1, math.inf,
                                        L.dptr(sums), C.byref(nc)), "icp fitness")
        # (getFitnessScore: the mean squared distance; no point at all reads as DBL_MAX)
        fitness = float(sums[15]) / nc.value if nc.value > 0 else float(np.finfo(np.float64).max)
        return bool(st.converged), final_T, fitness, int(st.iterations), int(st.convergence_state)

    def icp_align_device(self, max_corr_dist: float, guess: Optional[np.ndarray] = None, batch: int = 0):
        """icp_align's result from the device-resident loop (slio_icp_align):
        the same bits with ceil(iterations / batch) + 1 host waits instead of
        iterations + 1 (batch <= 0: the library's default).  icp_far_first as
        icp_align; icp_state keeps the final slio_icp_state."""
        return icp_align_device(self.lib, self.loop_handle(), max_corr_dist, guess, batch, owner=self)

    def perform_loop_closure(self, key_poses6, key_times, t_cur: float, loop_index_container: dict,
                             radius: float = 15.0, time_diff: float = 30.0, search_num: int = 25,
                             fitness_score: float = 0.3, leaf: float = 0.4) -> Optional[LoopClosure]:
        """performLoopClosure (:725-826) up to the factor.  key_poses6 (N, 6) =
        cloudKeyPoses6D as (roll, pitch, yaw, x, y, z), key_times their stamps,
        t_cur = timeLaserInfoCur; radius / time_diff / search_num /
        fitness_score = historyKeyframeSearchRadius / SearchTimeDiff /
        SearchNum / FitnessScore.  Returns None where the reference returns
        early: no candidate, clouds below 300 / 1000 points (:756), ICP not
        converged or its fitness above fitness_score (:781-783).  Otherwise
        records the pair in loop_index_container (:825) and returns it with
        the corrected pose, loopKeyPre's pose and the noise score."""
        f = np.float32
        poses = np.ascontiguousarray(np.asarray(key_poses6, dtype=f).reshape(-1, 6))
        det = detect_loop_closure_distance(poses[:, 3:6], key_times, t_cur, loop_index_container, radius, time_diff)
        if det is None:
            return None
        cur, pre = det
        n_src = self.loop_find_near_keyframes(cur, 0, poses, True, leaf)
        n_tgt = self.loop_find_near_keyframes(pre, search_num, poses, False, leaf)
        if n_src < 300 or n_tgt < 1000:
            return None
        conv, T, fitness, iters, _ = self.icp_align(2.0 * radius)
        if not conv or fitness > fitness_score:
            return None
        t = np.matmul(T, pose_affine(poses[cur]))  # correctionLidarFrame * tWrong (float)
        # pcl::getTranslationAndEulerAngles
        roll = f(math.atan2(float(t[2, 1]), float(t[2, 2])))
        pitch = f(math.asin(float(-t[2, 0])))
        yaw = f(math.atan2(float(t[1, 0]), float(t[0, 0])))
        pose_from = np.array([t[0, 3], t[1, 3], t[2, 3], roll, pitch, yaw], f)
        p = poses[pre]
        pose_to = np.array([p[3], p[4], p[5], p[0], p[1], p[2]], f)
        loop_index_container[cur] = pre
        return LoopClosure((cur, pre), pose_from, pose_to, f(fitness).item(), iters)

    def corner_optimization(self, transform: np.ndarray, count: bool = True) -> int:
        """:1303-1432; count: return the selected points (a device -> host
        copy and a wait; the LM loop takes the count from the normal
        equations instead)."""
        k = C.c_int64()
        L.check(self.lib.slio_s2m_coeffs(self.hc, 0, L.fptr(transform), C.byref(k) if count else None),
                "cornerOptimization")
        return k.value

    def surf_optimization(self, transform: np.ndarray, count: bool = True) -> int:
        """:1438-1515 (see corner_optimization)."""
        k = C.c_int64()
        L.check(self.lib.slio_s2m_coeffs(self.hs, 1, L.fptr(transform), C.byref(k) if count else None),
                "surfOptimization")
        return k.value

    def normal_equations(self, transform: np.ndarray):
        AtA = np.zeros(36, np.float32)
        AtB = np.zeros(6, np.float32)
        n = C.c_int64()
        L.check(self.lib.slio_s2m_normal_equations(self.hc, self.hs, L.fptr(transform), L.fptr(AtA), L.fptr(AtB),
                                                   C.byref(n)), "normal_equations")
        return AtA, AtB, n.value

    def LMOptimization(self, transform: np.ndarray, iter_count: int) -> bool:
        AtA, AtB, nsel = self.normal_equations(transform)
        conv = C.c_int(0)
        rc = self.lib.slio_s2m_lm_step(L.fptr(AtA), L.fptr(AtB), nsel, iter_count, L.fptr(transform),
                                       C.byref(self.isDegenerate), L.fptr(self.matP), C.byref(conv))
        if rc < 0:
            L.check(rc, "LMOptimization")
        return bool(conv.value)

    def scan2MapOptimization(self, transformTobeMapped: np.ndarray) -> np.ndarray:
        """:1706-1740 -- returns the optimised transformTobeMapped (roll,
        pitch, yaw, x, y, z); unchanged when the frame has too few features."""
        tf = np.ascontiguousarray(transformTobeMapped, dtype=np.float32).copy()
        self.iterations = 0
        if not (self.n_corner > EDGE_FEATURE_MIN_VALID_NUM and self.n_surf > SURF_FEATURE_MIN_VALID_NUM):
            return tf
        for it in range(30):
            self.corner_optimization(tf, count=False)
            self.surf_optimization(tf, count=False)
            self.iterations = it + 1
            if self.LMOptimization(tf, it):
                break
        return tf
