"""livox_mapping's scanRegistration node (src/livox_mapping/src/scanRegistration.cpp)
on the device, behind the reference's names: the slio_lreg_* entries of
include/slio_frontend.h.

``LivoxScanRegistration.laserCloudHandler`` is the node's one handler
(:152-534): the sensor's cloud in, laserCloud / cornerPointsSharp /
surfPointsFlat out.  The three clouds stay in HBM, where
``LivoxMapping.feed_device`` / ``process_cloud`` (livox_map.py) read them, so a
frame goes from the sensor's cloud to a pose with only the raw cloud crossing
PCIe.  ``classify_host`` and ``plane_judge`` are the host restatement
(csrc/slio_lreg.cpp), callable without a GPU.  ``repub`` is livox_repub.cpp's
per-message formatting; it stays on the host, as message handling does
everywhere in this package.  Clouds are (n, 4) float32 {x, y, z, intensity}.
The stated departures are listed in slio_frontend.h and DESIGN.md §3.15.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

CORNER, SURF = 0, 1
MAX_POINTS = 32000        # CloudFeatureFlag[32000] (:53)
STATS = ("stride1", "stride4", "left_surf", "right_surf", "set150", "outlier", "break_left", "break_right",
         "set100", "kept100", "reset100", "reset_erased")


def _xyzi(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).reshape(-1, 4)


def chain_tile():
    """(positions per thread, positions per workgroup) of the chain kernel:
    thread t owns the loop positions [5 + t * per_thread, 5 + (t + 1) * per_thread)."""
    a, b = C.c_int32(), C.c_int32()
    L.check(L.load().slio_lreg_chain_tile(C.byref(a), C.byref(b)), "lreg_chain_tile")
    return a.value, b.value


def classify_host(cloud):
    """The whole handler on the host, as its literal serial loops.  Returns
    dict(flags, visited, cloud, corner, surf, counts, stats)."""
    c = _xyzi(cloud)
    cap = min(c.shape[0], MAX_POINTS)
    flags, vis = np.zeros(max(cap, 1), np.int32), np.zeros(max(cap, 1), np.uint8)
    full, corner, surf = (np.zeros((max(cap, 1), 4), np.float32) for _ in range(3))
    counts, stats = np.zeros(3, np.int32), np.zeros(len(STATS), np.int32)
    L.check(L.load().slio_lreg_classify_host(L.fptr(c), c.shape[0], L.iptr(flags), L.u8ptr(vis), L.fptr(full),
                                             L.fptr(corner), L.fptr(surf), L.iptr(counts), L.iptr(stats)),
            "lreg_classify_host")
    n, nc, ns = (int(v) for v in counts)
    return dict(flags=flags[:n].copy(), visited=vis[:n].copy(), cloud=full[:n].copy(), corner=corner[:nc].copy(),
                surf=surf[:ns].copy(), counts=counts, stats=dict(zip(STATS, (int(v) for v in stats))))


def plane_judge(points, threshold: int) -> bool:
    """plane_judge (:64-120) on a list of points (n, 3)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    out = C.c_int32()
    L.check(L.load().slio_lreg_plane_judge(L.fptr(p), p.shape[0], int(threshold), C.byref(out)), "lreg_plane_judge")
    return bool(out.value)


def repub(xyz, line, reflectivity, offset_time):
    """livox_repub.cpp:16-35 over a list of messages (each argument a list with
    one array per message): every point becomes {x, y, z, intensity = line +
    reflectivity / 10000.0, curvature = offset_time / float(the message's last
    offset_time) * 0.1}, the messages concatenated.  Returns (n, 5) float32.
    Per-message formatting: it runs on the host."""
    out = []
    for p, ln, rf, ot in zip(xyz, line, reflectivity, offset_time):
        p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
        ln, rf = np.asarray(ln, np.uint8).reshape(-1), np.asarray(rf, np.uint8).reshape(-1)
        ot = np.asarray(ot, np.uint32).reshape(-1)
        if p.shape[0] == 0:
            continue
        inten = (ln.astype(np.float64) + rf.astype(np.float64) / 10000.0).astype(np.float32)
        s = (ot.astype(np.float32) / np.float32(ot[-1])).astype(np.float32)     # uint / float: float
        curv = (s.astype(np.float64) * 0.1).astype(np.float32)
        out.append(np.concatenate([p, inten[:, None], curv[:, None]], 1))
    return np.concatenate(out, 0).astype(np.float32) if out else np.zeros((0, 5), np.float32)


class LivoxScanRegistration:
    """scanRegistration's laserCloudHandler on the device."""

    def __init__(self, device: int = 0, max_points: int = MAX_POINTS):
        self.lib = L.load()
        p = L.SlioLregParams()
        L.check(self.lib.slio_lreg_params_default(C.byref(p)), "lreg_params_default")
        p.device, p.max_points = device, max_points
        self.h = C.c_void_p()
        L.check(self.lib.slio_lreg_create(C.byref(self.h), C.byref(p)), "lreg_create")
        self.counts = np.zeros(3, np.int32)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_lreg_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, cloud) -> np.ndarray:
        """The registration alone; the clouds stay on the device.  Returns
        counts = sizes of {laserCloud, cornerPointsSharp, surfPointsFlat}."""
        c = _xyzi(cloud)
        counts = np.zeros(3, np.int32)
        L.check(self.lib.slio_lreg_run(self.h, L.fptr(c), c.shape[0], L.iptr(counts)), "lreg_run")
        self.counts = counts
        return counts

    def _get(self, kind) -> np.ndarray:
        n = int(self.counts[0] if kind is None else self.counts[1 + kind])
        out = np.zeros((max(n, 1), 4), np.float32)
        if kind is None:
            L.check(self.lib.slio_lreg_get_cloud(self.h, L.fptr(out), n), "lreg_get_cloud")
        else:
            L.check(self.lib.slio_lreg_get_features(self.h, kind, L.fptr(out), n), "lreg_get_features")
        return out[:n]

    def laserCloud(self) -> np.ndarray:
        return self._get(None)

    def cornerPointsSharp(self) -> np.ndarray:
        return self._get(CORNER)

    def surfPointsFlat(self) -> np.ndarray:
        return self._get(SURF)

    def laserCloudHandler(self, cloud):
        """:152-534.  Returns (laserCloud, cornerPointsSharp, surfPointsFlat)."""
        self.run(cloud)
        return self.laserCloud(), self.cornerPointsSharp(), self.surfPointsFlat()

    def flags(self):
        """(CloudFeatureFlag, loop 1's visited mask) of the last run."""
        n = int(self.counts[0])
        f, v = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint8)
        L.check(self.lib.slio_lreg_get_flags(self.h, L.iptr(f), L.u8ptr(v)), "lreg_get_flags")
        return f[:n], v[:n]
