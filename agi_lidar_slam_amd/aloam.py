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
intensity = scanID + scanPeriod * relTime}.  laserOdometry and laserMapping
solve through Ceres and are not part of this package.  The stated departures
are listed in slio_frontend.h and DESIGN.md §3.17.
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
        self.n_scans = n_scans
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
