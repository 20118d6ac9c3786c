"""A-LOAM's scanRegistration node (src/A-LOAM/src/scanRegistration.cpp) on the
device, behind the reference's names: the slio_aloam_* entries of
include/slio_frontend.h.

``AloamScanRegistration.laserCloudHandler`` is the node's one handler
(:124-432) for the 16-, 32- and 64-line layouts: the sensor's cloud in, the
five published clouds out (laserCloud, cornerPointsSharp,
cornerPointsLessSharp, surfPointsFlat, surfPointsLessFlat).  The clouds stay in
HBM behind ``view()`` until the next run.  ``register_host`` is the host
restatement (csrc/slio_aloam.cpp), callable without a GPU.  Input clouds are
(n, 3) float32 in the message's order, output clouds (n, 4) float32 {x, y, z,
intensity = scanID + scanPeriod * relTime}.

``AloamOdometry`` is the laserOdometry node's loop body
(src/A-LOAM/src/laserOdometry.cpp:304-695) on the device, the slio_aloam_odom_*
entries: the four feature clouds of a sweep in, /laser_odom_to_init out, from
host clouds (``process``) or from a registration's device view
(``process_view``).  ``AloamScanRegistration.enable_odometry`` puts one beside
a registration, and ``laserOdometry(xyz)`` is then the sensor's cloud in and
the pose out with only the raw cloud crossing PCIe.  ``AloamOdometryHost`` is
the host restatement (csrc/slio_aloam_odom.cpp), callable without a GPU.  The
association and the factors are the reference's; the solve is this library's
own Levenberg-Marquardt in the shape of Ceres' trust-region defaults, and
parity with Ceres' own iterates is unpinned.

``AloamMapping`` is the laserMapping node's loop body
(src/A-LOAM/src/laserMapping.cpp:326-893) on the device, the slio_aloam_map_*
entries: the odometry's two last clouds and its pose in, /aft_mapped_to_init
out, with the rolling 21 x 21 x 11 cube map in HBM.
``AloamScanRegistration.enable_mapping`` puts an odometry and a mapper beside a
registration, and ``laserMapping(xyz)`` is then the whole chain with only the
raw cloud crossing PCIe.  ``AloamMappingHost`` is the host restatement
(csrc/slio_aloam_map.cpp).  The stated departures are listed in slio_frontend.h
and DESIGN.md §3.17 - §3.19.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

CLOUDS = ("laserCloud", "cornerPointsSharp", "cornerPointsLessSharp", "surfPointsFlat", "surfPointsLessFlat")
MAX_POINTS = 400000       # cloudCurvature[400000] (:65-68)
STATS = ("drop_nonfinite", "drop_range", "drop_scan", "drop_over50", "end_minus", "end_plus", "first_plus",
         "first_minus", "second_plus", "second_minus", "half_passed", "scans_skipped", "break21", "flat", "break4",
         "seam_marks", "seam_suppressed", "vg_overflow")


def _xyz(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _params(n_scans, minimum_range, device, max_points, scan_period=0.1):
    p = L.SlioAloamParams()
    L.check(L.load().slio_aloam_params_default(C.byref(p)), "aloam_params_default")
    p.device, p.n_scans, p.max_points = device, n_scans, max_points
    p.minimum_range, p.scan_period = minimum_range, scan_period
    return p


def tile():
    """(points per workgroup of the per-point passes, the longest list the LDS
    sort takes in one piece)."""
    a, b = C.c_int32(), C.c_int32()
    L.check(L.load().slio_aloam_tile(C.byref(a), C.byref(b)), "aloam_tile")
    return a.value, b.value


def register_host(xyz, n_scans: int = 16, minimum_range: float = 0.1, max_points: int = MAX_POINTS):
    """The whole handler on the host, as its literal serial loops.  Returns a
    dict of the five clouds by the publishers' names plus scan_start, scan_end,
    curvature, label, picked, counts and stats."""
    c = _xyz(xyz)
    n = c.shape[0]
    p = _params(n_scans, minimum_range, 0, max_points)
    m = max(n, 1)
    clouds = [np.zeros((m, 4), np.float32) for _ in range(5)]
    start, end = np.zeros(64, np.int32), np.zeros(64, np.int32)
    curv, label, picked = np.zeros(m, np.float32), np.zeros(m, np.int32), np.zeros(m, np.uint8)
    counts, stats = np.zeros(5, np.int32), np.zeros(len(STATS), np.int32)
    L.check(L.load().slio_aloam_register_host(C.byref(p), L.fptr(c), n, *[L.fptr(a) for a in clouds], L.iptr(start),
                                              L.iptr(end), L.fptr(curv), L.iptr(label), L.u8ptr(picked),
                                              L.iptr(counts), L.iptr(stats)), "aloam_register_host")
    out = {name: clouds[k][:counts[k]].copy() for k, name in enumerate(CLOUDS)}
    N = int(counts[0])
    out.update(scan_start=start[:n_scans].copy(), scan_end=end[:n_scans].copy(), curvature=curv[:N].copy(),
               label=label[:N].copy(), picked=picked[:N].copy(), counts=counts,
               stats=dict(zip(STATS, (int(v) for v in stats))))
    return out


class AloamScanRegistration:
    """scanRegistration's laserCloudHandler on the device."""

    def __init__(self, n_scans: int = 16, minimum_range: float = 0.1, device: int = 0,
                 max_points: int = MAX_POINTS):
        self.lib = L.load()
        self.n_scans, self.device, self.max_points = n_scans, device, max_points
        p = _params(n_scans, minimum_range, device, max_points)
        self.h = C.c_void_p()
        L.check(self.lib.slio_aloam_create(C.byref(self.h), C.byref(p)), "aloam_create")
        self.counts = np.zeros(5, np.int32)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_aloam_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, xyz) -> np.ndarray:
        """The registration alone; the clouds stay on the device.  Returns the
        sizes of the five clouds in CLOUDS' order."""
        c = _xyz(xyz)
        counts = np.zeros(5, np.int32)
        L.check(self.lib.slio_aloam_run(self.h, L.fptr(c), c.shape[0], L.iptr(counts)), "aloam_run")
        self.counts = counts
        return counts

    def _get(self, kind: int) -> np.ndarray:
        n = int(self.counts[kind])
        out = np.zeros((max(n, 1), 4), np.float32)
        L.check(self.lib.slio_aloam_get_cloud(self.h, kind, L.fptr(out), n), "aloam_get_cloud")
        return out[:n]

    def laserCloud(self) -> np.ndarray:
        return self._get(0)

    def cornerPointsSharp(self) -> np.ndarray:
        return self._get(1)

    def cornerPointsLessSharp(self) -> np.ndarray:
        return self._get(2)

    def surfPointsFlat(self) -> np.ndarray:
        return self._get(3)

    def surfPointsLessFlat(self) -> np.ndarray:
        return self._get(4)

    def laserCloudHandler(self, xyz) -> dict:
        """:124-432.  Returns the five clouds by the publishers' names."""
        self.run(xyz)
        return {name: self._get(k) for k, name in enumerate(CLOUDS)}

    def scan_index(self):
        """(scanStartInd, scanEndInd) of the last run (:246-250)."""
        s, e = np.zeros(self.n_scans, np.int32), np.zeros(self.n_scans, np.int32)
        L.check(self.lib.slio_aloam_get_scan_index(self.h, L.iptr(s), L.iptr(e)), "aloam_get_scan_index")
        return s, e

    def work(self):
        """(cloudCurvature, cloudLabel, cloudNeighborPicked) of the last run."""
        n = int(self.counts[0])
        c, l, p = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        L.check(self.lib.slio_aloam_get_work(self.h, L.fptr(c), L.iptr(l), L.u8ptr(p)), "aloam_get_work")
        return c[:n], l[:n], p[:n]

    def view(self) -> L.SlioAloamView:
        """Device pointers and sizes of the five clouds, valid until the next run."""
        v = L.SlioAloamView()
        L.check(self.lib.slio_aloam_get_view(self.h, C.byref(v)), "aloam_get_view")
        return v

    def enable_odometry(self, skip_frame_num: int = 2) -> "AloamOdometry":
        """An AloamOdometry on this registration's device, fed by laserOdometry."""
        self.odometry = AloamOdometry(self.n_scans, skip_frame_num, self.device, self.max_points)
        return self.odometry

    def laserOdometry(self, xyz) -> dict:
        """scanRegistration's handler, then laserOdometry's loop body on its
        clouds, device to device.  Returns the odometry's result."""
        if getattr(self, "odometry", None) is None:
            raise L.SlioError("laserOdometry: no enable_odometry before")
        self.run(xyz)
        return self.odometry.process_view(self.view())

    def enable_mapping(self, skip_frame_num: int = 2, leaf_corner: float = 0.4, leaf_surf: float = 0.8,
                       max_map_points: int = 1 << 21) -> "AloamMapping":
        """An AloamOdometry (unless enable_odometry made one) and an
        AloamMapping on this registration's device, fed by laserMapping."""
        if getattr(self, "odometry", None) is None:
            self.enable_odometry(skip_frame_num)
        self.mapping = AloamMapping(leaf_corner, leaf_surf, self.device, max_map_points, self.max_points)
        return self.mapping

    def laserMapping(self, xyz) -> dict:
        """The three nodes on one sweep: scanRegistration's handler,
        laserOdometry's loop body and, on the sweeps the odometry publishes
        (laserOdometry.cpp:667), laserMapping's loop body on the odometry's
        last clouds, all device to device.  Returns dict(odometry=..,
        mapping=.. or None where the gate stayed shut)."""
        if getattr(self, "mapping", None) is None:
            raise L.SlioError("laserMapping: no enable_mapping before")
        od = self.laserOdometry(xyz)
        mp = None
        if od["published"]:
            mp = self.mapping.process_view(self.odometry.view(), od["q_w_curr"], od["t_w_curr"])
        return dict(odometry=od, mapping=mp)


STOPS = ("max_iter", "gradient", "function", "parameter")
PASS_FIELDS = ("corner", "plane", "degenerate", "iterations", "accepted", "outliers", "stop", "few", "cost_first",
               "cost_last")


def _xyzi(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).reshape(-1, 4)


def _odom_params(n_scans, skip_frame_num, device, max_points):
    p = L.SlioAloamOdomParams()
    L.check(L.load().slio_aloam_odom_params_default(C.byref(p)), "aloam_odom_params_default")
    p.device, p.n_scans, p.max_points, p.skip_frame_num = device, n_scans, max_points, skip_frame_num
    return p


def _result(r: L.SlioAloamOdomResult) -> dict:
    out = dict(q_w_curr=list(r.q_w_curr), t_w_curr=list(r.t_w_curr), q_last_curr=list(r.q_last_curr),
               t_last_curr=list(r.t_last_curr), inited=r.inited, published=r.published, frame_count=r.frame_count,
               passes=[])
    for k in range(2 if r.inited else 0):
        ps = r.passes[k]
        d = {f: getattr(ps, f) for f in PASS_FIELDS}
        d["iterates"] = [dict(q=list(ps.it_q[i]), t=list(ps.it_t[i]), cost=ps.it_cost[i], mu=ps.it_mu[i])
                         for i in range(ps.iterations)]
        out["passes"].append(d)
    return out


class AloamOdometry:
    """laserOdometry's loop body (:304-695) on the device."""

    def __init__(self, n_scans: int = 16, skip_frame_num: int = 2, device: int = 0, max_points: int = MAX_POINTS):
        self.lib = L.load()
        p = _odom_params(n_scans, skip_frame_num, device, max_points)
        self.h = C.c_void_p()
        L.check(self.lib.slio_aloam_odom_create(C.byref(self.h), C.byref(p)), "aloam_odom_create")
        self.result = None

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_aloam_odom_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def reset(self) -> None:
        L.check(self.lib.slio_aloam_odom_reset(self.h), "aloam_odom_reset")
        self.result = None

    def process(self, sharp, less_sharp, flat, less_flat) -> dict:
        """One sweep from cornerPointsSharp, cornerPointsLessSharp,
        surfPointsFlat and surfPointsLessFlat on the host."""
        a = [_xyzi(c) for c in (sharp, less_sharp, flat, less_flat)]
        r = L.SlioAloamOdomResult()
        args = [x for c in a for x in (L.fptr(c), c.shape[0])]
        L.check(self.lib.slio_aloam_odom_run(self.h, *args, C.byref(r)), "aloam_odom_run")
        self.result = _result(r)
        return self.result

    def process_view(self, view: L.SlioAloamView) -> dict:
        """One sweep from a registration's device view."""
        r = L.SlioAloamOdomResult()
        L.check(self.lib.slio_aloam_odom_run_view(self.h, C.byref(view), C.byref(r)), "aloam_odom_run_view")
        self.result = _result(r)
        return self.result

    @property
    def pose(self):
        """(q_w_curr (x, y, z, w), t_w_curr) after the last sweep."""
        if self.result is None:
            return [0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0]
        return self.result["q_w_curr"], self.result["t_w_curr"]

    def last_clouds(self):
        """(laserCloudCornerLast, laserCloudSurfLast) on the host."""
        n = np.zeros(2, np.int32)
        L.check(self.lib.slio_aloam_odom_get_last(self.h, None, 0, None, 0, L.iptr(n)), "aloam_odom_get_last")
        c, s = np.zeros((max(int(n[0]), 1), 4), np.float32), np.zeros((max(int(n[1]), 1), 4), np.float32)
        L.check(self.lib.slio_aloam_odom_get_last(self.h, L.fptr(c), int(n[0]), L.fptr(s), int(n[1]), L.iptr(n)),
                "aloam_odom_get_last")
        return c[:n[0]], s[:n[1]]

    def view(self) -> L.SlioAloamOdomView:
        v = L.SlioAloamOdomView()
        L.check(self.lib.slio_aloam_odom_get_view(self.h, C.byref(v)), "aloam_odom_get_view")
        return v

    # the lockstep entries, for tests
    def associate(self, q, t) -> None:
        q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
        L.check(self.lib.slio_aloam_odom_associate(self.h, L.dptr(q), L.dptr(t)), "aloam_odom_associate")

    def correspondences(self) -> np.ndarray:
        corr, n = np.zeros((2304, 3), np.int32), np.zeros(1, np.int32)
        L.check(self.lib.slio_aloam_odom_get_correspondences(self.h, L.iptr(corr), 2304, L.iptr(n)),
                "aloam_odom_get_correspondences")
        return corr[:n[0]]

    def evaluate(self, q, t):
        """(A[21], g[6], cost, counts {corner, plane, degenerate, outliers})."""
        q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
        A, g, cost, cnt = np.zeros(21), np.zeros(6), np.zeros(1), np.zeros(4, np.int32)
        L.check(self.lib.slio_aloam_odom_evaluate(self.h, L.dptr(q), L.dptr(t), L.dptr(A), L.dptr(g), L.dptr(cost),
                                                  L.iptr(cnt)), "aloam_odom_evaluate")
        return A, g, float(cost[0]), [int(v) for v in cnt]


def odom_host_associate(sharp, flat, corner_last, surf_last, q, t) -> np.ndarray:
    a = [_xyzi(c) for c in (sharp, flat, corner_last, surf_last)]
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    corr = np.zeros((a[0].shape[0] + a[1].shape[0] + 1, 3), np.int32)
    args = [x for c in a for x in (L.fptr(c), c.shape[0])]
    L.check(L.load().slio_aloam_odom_host_associate(*args, L.dptr(q), L.dptr(t), L.iptr(corr)),
            "aloam_odom_host_associate")
    return corr[:-1]


def odom_host_evaluate(sharp, flat, corner_last, surf_last, corr, q, t):
    a = [_xyzi(c) for c in (sharp, flat, corner_last, surf_last)]
    q, t = np.ascontiguousarray(q, np.float64), np.ascontiguousarray(t, np.float64)
    corr = np.ascontiguousarray(corr, np.int32)
    A, g, cost, cnt = np.zeros(21), np.zeros(6), np.zeros(1), np.zeros(4, np.int32)
    args = [x for c in a for x in (L.fptr(c), c.shape[0])]
    L.check(L.load().slio_aloam_odom_host_evaluate(*args, L.iptr(corr), L.dptr(q), L.dptr(t), L.dptr(A), L.dptr(g),
                                                   L.dptr(cost), L.iptr(cnt)), "aloam_odom_host_evaluate")
    return A, g, float(cost[0]), [int(v) for v in cnt]


class AloamOdometryHost:
    """The same loop body on the host (slio_aloam_odom_host_run), no GPU."""

    def __init__(self, n_scans: int = 16, skip_frame_num: int = 2, max_points: int = MAX_POINTS):
        self.lib = L.load()
        self.p = _odom_params(n_scans, skip_frame_num, 0, max_points)
        self.st = L.SlioAloamOdomState()
        self.reset()

    def reset(self) -> None:
        L.check(self.lib.slio_aloam_odom_host_init(C.byref(self.st)), "aloam_odom_host_init")
        self.corner_last = self.surf_last = np.zeros((0, 4), np.float32)
        self.result = None

    def process(self, sharp, less_sharp, flat, less_flat) -> dict:
        sharp, less_sharp, flat, less_flat = (_xyzi(c) for c in (sharp, less_sharp, flat, less_flat))
        for c in (less_sharp, less_flat):           # what becomes a last cloud is checked on the way in
            it = c[:, 3]
            if not (np.all((it >= 0) & (it < 64)) and np.all(np.diff(it.astype(np.int64)) >= 0)):
                raise L.SlioError("aloam_odom_host: EINVAL: scan ids of a less cloud decreasing or outside [0, 64)")
        r = L.SlioAloamOdomResult()
        a = (sharp, flat, self.corner_last, self.surf_last)
        args = [x for c in a for x in (L.fptr(c), c.shape[0])]
        L.check(self.lib.slio_aloam_odom_host_run(C.byref(self.p), C.byref(self.st), *args, C.byref(r)),
                "aloam_odom_host_run")
        self.corner_last, self.surf_last = less_sharp.copy(), less_flat.copy()
        self.result = _result(r)
        return self.result


# ---------------------------------------------------------------- laserMapping
KINDS = ("none", "edge", "plane", "degenerate", "rejected")
N_CUBES = 21 * 21 * 11


def _map_params(leaf_corner, leaf_surf, device, max_points, max_scan):
    p = L.SlioAloamMapParams()
    L.check(L.load().slio_aloam_map_params_default(C.byref(p)), "aloam_map_params_default")
    p.device, p.max_points, p.max_scan = device, max_points, max_scan
    p.leaf_corner, p.leaf_surf = leaf_corner, leaf_surf
    return p


def _pose(q, t):
    return np.ascontiguousarray(q, np.float64).reshape(4), np.ascontiguousarray(t, np.float64).reshape(3)


def _map_result(r: L.SlioAloamMapResult) -> dict:
    out = dict(q_w_curr=list(r.q_w_curr), t_w_curr=list(r.t_w_curr), q_wmap_wodom=list(r.q_wmap_wodom),
               t_wmap_wodom=list(r.t_wmap_wodom), center=list(r.center), shift=list(r.shift),
               map_size=list(r.map_size), stack_size=list(r.stack_size), optimized=r.optimized, nvalid=r.nvalid,
               passes=[])
    for k in range(2 if r.optimized else 0):
        ps = r.passes[k]
        d = {f: getattr(ps, f) for f in PASS_FIELDS}
        d["iterates"] = [dict(q=list(ps.it_q[i]), t=list(ps.it_t[i]), cost=ps.it_cost[i], mu=ps.it_mu[i])
                         for i in range(ps.iterations)]
        out["passes"].append(d)
    return out


def map_predict(q_wmap_wodom, t_wmap_wodom, q_wodom_curr, t_wodom_curr):
    """The high-frequency pose (laserMapping.cpp:222-223)."""
    a, b = _pose(q_wmap_wodom, t_wmap_wodom)
    c, d = _pose(q_wodom_curr, t_wodom_curr)
    q, t = np.zeros(4), np.zeros(3)
    L.check(L.load().slio_aloam_map_predict(L.dptr(a), L.dptr(b), L.dptr(c), L.dptr(d), L.dptr(q), L.dptr(t)),
            "aloam_map_predict")
    return list(q), list(t)


def map_host_select(t_w_curr, cen):
    """(centre cube, shift, cube list); cen (3 ints) is updated in place."""
    t = np.ascontiguousarray(t_w_curr, np.float64).reshape(3)
    c = np.array(cen, np.int32)
    center, shift, lst, n = np.zeros(3, np.int32), np.zeros(3, np.int32), np.zeros(75, np.int32), np.zeros(1, np.int32)
    L.check(L.load().slio_aloam_map_host_select(L.dptr(t), L.iptr(c), L.iptr(center), L.iptr(shift), L.iptr(lst),
                                                L.iptr(n)), "aloam_map_host_select")
    cen[:] = [int(v) for v in c]
    return [int(v) for v in center], [int(v) for v in shift], [int(v) for v in lst[:n[0]]]


def map_host_fit_line(nb):
    """(kind, a, b, eigenvalues, eigenvectors in columns) of five neighbours."""
    nb = np.ascontiguousarray(nb, np.float64).reshape(5, 3)
    a, b, lam, vec = np.zeros(3), np.zeros(3), np.zeros(3), np.zeros((3, 3))
    k = L.load().slio_aloam_map_host_fit_line(L.dptr(nb), L.dptr(a), L.dptr(b), L.dptr(lam), L.dptr(vec))
    if k < 0:
        L.check(k, "aloam_map_host_fit_line")
    return k, a, b, lam, vec


def map_host_fit_plane(nb):
    """(kind, unit normal, d, the solution x of A x = -1) of five neighbours."""
    nb = np.ascontiguousarray(nb, np.float64).reshape(5, 3)
    n, d, x = np.zeros(3), np.zeros(1), np.zeros(3)
    k = L.load().slio_aloam_map_host_fit_plane(L.dptr(nb), L.dptr(n), L.dptr(d), L.dptr(x))
    if k < 0:
        L.check(k, "aloam_map_host_fit_plane")
    return k, n, float(d[0]), x


def map_host_evaluate(xyz, kind, rec, q, t):
    """(A[21], g[6], cost, counts {edge, plane, degenerate, outliers}) over the slots."""
    xyz = _xyz(xyz)
    kind = np.ascontiguousarray(kind, np.uint8)
    rec = np.ascontiguousarray(rec, np.float64).reshape(-1, 6)
    q, t = _pose(q, t)
    A, g, cost, cnt = np.zeros(21), np.zeros(6), np.zeros(1), np.zeros(4, np.int32)
    L.check(L.load().slio_aloam_map_host_evaluate(L.fptr(xyz), L.u8ptr(kind), L.dptr(rec), xyz.shape[0], L.dptr(q),
                                                  L.dptr(t), L.dptr(A), L.dptr(g), L.dptr(cost), L.iptr(cnt)),
            "aloam_map_host_evaluate")
    return A, g, float(cost[0]), [int(v) for v in cnt]


class _MapCommon:
    """What AloamMapping and AloamMappingHost share: the getters by entry name."""

    def _cloud(self, fn, what, *args) -> np.ndarray:
        n = C.c_int64()
        L.check(fn(self.h, *args, None, 0, C.byref(n)), what)
        out = np.zeros((max(n.value, 1), 3), np.float32)
        L.check(fn(self.h, *args, L.fptr(out), n.value, C.byref(n)), what)
        return out[:n.value]

    def _association(self, fn, what):
        n = np.zeros(1, np.int32)
        rc = fn(self.h, None, None, None, None, 0, L.iptr(n))
        if rc not in (0, -4):
            L.check(rc, what)
        m = max(int(n[0]), 1)
        kind, rec = np.zeros(m, np.uint8), np.zeros((m, 6))
        idx, sqd = np.zeros((m, 5), np.int32), np.zeros((m, 5), np.float32)
        L.check(fn(self.h, L.u8ptr(kind), L.dptr(rec), L.iptr(idx), L.fptr(sqd), m, L.iptr(n)), what)
        k = int(n[0])
        return kind[:k], rec[:k], idx[:k], sqd[:k]


class AloamMapping(_MapCommon):
    """laserMapping's loop body (:326-893) on the device."""

    def __init__(self, leaf_corner: float = 0.4, leaf_surf: float = 0.8, device: int = 0,
                 max_points: int = 1 << 21, max_scan: int = MAX_POINTS):
        self.lib = L.load()
        p = _map_params(leaf_corner, leaf_surf, device, max_points, max_scan)
        self.h = C.c_void_p()
        L.check(self.lib.slio_aloam_map_create(C.byref(self.h), C.byref(p)), "aloam_map_create")
        self.result = None

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_aloam_map_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def reset(self) -> None:
        L.check(self.lib.slio_aloam_map_reset(self.h), "aloam_map_reset")
        self.result = None

    def process(self, corner_last, surf_last, q_wodom_curr, t_wodom_curr) -> dict:
        """One sweep from laserCloudCornerLast / laserCloudSurfLast on the host
        ((n, 4) float32) and /laser_odom_to_init."""
        c, s = _xyzi(corner_last), _xyzi(surf_last)
        q, t = _pose(q_wodom_curr, t_wodom_curr)
        r = L.SlioAloamMapResult()
        L.check(self.lib.slio_aloam_map_run(self.h, L.fptr(c), c.shape[0], L.fptr(s), s.shape[0], L.dptr(q), L.dptr(t),
                                            C.byref(r)), "aloam_map_run")
        self.result = _map_result(r)
        return self.result

    def process_view(self, view: L.SlioAloamOdomView, q_wodom_curr, t_wodom_curr) -> dict:
        """One sweep from an odometry's device view."""
        q, t = _pose(q_wodom_curr, t_wodom_curr)
        r = L.SlioAloamMapResult()
        L.check(self.lib.slio_aloam_map_run_view(self.h, C.byref(view), L.dptr(q), L.dptr(t), C.byref(r)),
                "aloam_map_run_view")
        self.result = _map_result(r)
        return self.result

    def register_cloud(self, xyzi) -> np.ndarray:
        """laserCloudFullRes in the map frame (:929-933), from the host."""
        c = _xyzi(xyzi)
        out = np.zeros((max(c.shape[0], 1), 4), np.float32)
        L.check(self.lib.slio_aloam_map_register_cloud(self.h, c.ctypes.data_as(C.c_void_p), c.shape[0], 0,
                                                       L.fptr(out)), "aloam_map_register_cloud")
        return out[:c.shape[0]]

    def register_device_cloud(self, ptr, n: int) -> np.ndarray:
        """The same from a device cloud (a registration's view)."""
        out = np.zeros((max(n, 1), 4), np.float32)
        L.check(self.lib.slio_aloam_map_register_cloud(self.h, C.c_void_p(ptr), n, 1, L.fptr(out)),
                "aloam_map_register_cloud")
        return out[:n]

    def cube(self, kind: int, ind: int) -> np.ndarray:
        return self._cloud(self.lib.slio_aloam_map_get_cube, "aloam_map_get_cube", kind, ind)

    def cube_sizes(self, kind: int) -> np.ndarray:
        out = np.zeros(N_CUBES, np.int32)
        L.check(self.lib.slio_aloam_map_cube_sizes(self.h, kind, L.iptr(out)), "aloam_map_cube_sizes")
        return out

    def surround(self, kind: int) -> np.ndarray:
        return self._cloud(self.lib.slio_aloam_map_get_surround, "aloam_map_get_surround", kind)

    def map(self, kind: int) -> np.ndarray:
        return self._cloud(self.lib.slio_aloam_map_get_map, "aloam_map_get_map", kind)

    def stack(self, kind: int) -> np.ndarray:
        return self._cloud(self.lib.slio_aloam_map_get_stack, "aloam_map_get_stack", kind)

    # the lockstep entries, for tests
    def associate(self, q, t) -> None:
        q, t = _pose(q, t)
        L.check(self.lib.slio_aloam_map_associate(self.h, L.dptr(q), L.dptr(t)), "aloam_map_associate")

    def association(self):
        """(kind, record, neighbour indices, squared distances) per slot."""
        return self._association(self.lib.slio_aloam_map_get_association, "aloam_map_get_association")

    def evaluate(self, q, t):
        q, t = _pose(q, t)
        A, g, cost, cnt = np.zeros(21), np.zeros(6), np.zeros(1), np.zeros(4, np.int32)
        L.check(self.lib.slio_aloam_map_evaluate(self.h, L.dptr(q), L.dptr(t), L.dptr(A), L.dptr(g), L.dptr(cost),
                                                 L.iptr(cnt)), "aloam_map_evaluate")
        return A, g, float(cost[0]), [int(v) for v in cnt]


class AloamMappingHost(_MapCommon):
    """The same loop body on the host (slio_aloam_map_host_run), no GPU."""

    def __init__(self, leaf_corner: float = 0.4, leaf_surf: float = 0.8, max_points: int = 1 << 21,
                 max_scan: int = MAX_POINTS):
        self.lib = L.load()
        self.p = _map_params(leaf_corner, leaf_surf, 0, max_points, max_scan)
        self.h = C.c_void_p()
        self.reset()

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_aloam_map_host_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def reset(self) -> None:
        self.close()
        self.h = C.c_void_p()
        L.check(self.lib.slio_aloam_map_host_create(C.byref(self.h), C.byref(self.p)), "aloam_map_host_create")
        self.result = None

    def process(self, corner_last, surf_last, q_wodom_curr, t_wodom_curr) -> dict:
        c, s = _xyzi(corner_last), _xyzi(surf_last)
        q, t = _pose(q_wodom_curr, t_wodom_curr)
        r = L.SlioAloamMapResult()
        L.check(self.lib.slio_aloam_map_host_run(self.h, L.fptr(c), c.shape[0], L.fptr(s), s.shape[0], L.dptr(q),
                                                 L.dptr(t), C.byref(r)), "aloam_map_host_run")
        self.result = _map_result(r)
        return self.result

    def cube(self, kind: int, ind: int) -> np.ndarray:
        return self._cloud(self.lib.slio_aloam_map_host_get_cube, "aloam_map_host_get_cube", kind, ind)

    def stack(self, kind: int) -> np.ndarray:
        return self._cloud(self.lib.slio_aloam_map_host_get_stack, "aloam_map_host_get_stack", kind)

    def association(self):
        return self._association(self.lib.slio_aloam_map_host_get_association, "aloam_map_host_get_association")
