"""LIO-Livox's ScanRegistration node for Use_seg = 0
(src/LIO-Livox/src/lio/ScanRegistration.cpp, LidarFeatureExtractor.cpp) on the
device, behind the reference's names: the slio_llreg_* entries of
include/slio_frontend.h.

``LioLivoxScanRegistration.FeatureExtract`` is lidarCallBackHorizon's path
(LidarFeatureExtractor.cpp:1218-1291) on a CustomMsg given as arrays;
``FeatureExtract_Mid`` is lidarCallBackPc2 with FeatureExtract_Mid
(ScanRegistration.cpp:61-93, :1352-1401) on an (n, 4) cloud.  Both return
(laserCloud, laserConerFeature, laserSurfFeature) and leave the three clouds in
HBM (``view``) for a later estimator.  ``extract_host`` is the host restatement
(csrc/slio_llreg.cpp), callable without a GPU.

A cloud point is 8 float32: {x, y, z, intensity, normal_x, normal_y, normal_z,
curvature = 0}; normal_x is the time fraction, normal_y the line (the int's bits
in the CustomMsg path, a float value in the Pc2 path, as in the reference) and
normal_z the label 0 / 1 (corner) / 2 (surf).  What is kept as written and what
is defined where the reference is undefined: slio_frontend.h and DESIGN.md
§3.20.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

FULL, CORNER, SURF = 0, 1, 2
MAX_LINE = 20000          # CloudFeatureFlag[20000] (LidarFeatureExtractor.cpp:96)
MAX_SCANS = 6
MAX_POINTS = MAX_SCANS * MAX_LINE
POINT_FLOATS = 8

# config/horizon_config.yaml and config/mid360_config.yaml
HORIZON = dict(n_scans=6, lidar_type=0, num_curv_size=2, distance_faraway=100.0, num_flat=3, part_num=150,
               flat_threshold=0.02, break_corner_dis=1.0, lidar_nearest_dis=1.0, kdtree_corner_outlier_dis=0.2)
MID360 = dict(n_scans=4, lidar_type=2, num_curv_size=2, distance_faraway=30.0, num_flat=3, part_num=100,
              flat_threshold=0.02, break_corner_dis=1.0, lidar_nearest_dis=1.0, kdtree_corner_outlier_dis=0.2)


def make_params(device: int = 0, max_points: int = MAX_POINTS, **config) -> L.SlioLlregParams:
    """The defaults (horizon_config.yaml) with the given fields replaced."""
    p = L.SlioLlregParams()
    L.check(L.load().slio_llreg_params_default(C.byref(p)), "llreg_params_default")
    p.device, p.max_points = device, max_points
    for k, v in config.items():
        if k not in dict(p._fields_):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def tiles():
    """(chain positions per thread, per workgroup, the longest part the picking
    kernel resolves in registers, inputs per workgroup of the other kernels)."""
    v = [C.c_int32() for _ in range(4)]
    L.check(L.load().slio_llreg_tiles(*[C.byref(x) for x in v]), "llreg_tiles")
    return tuple(x.value for x in v)


def _msg(xyz, reflectivity, line, offset_time):
    p = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    r = np.ascontiguousarray(reflectivity, np.uint8).reshape(-1)
    ln = np.ascontiguousarray(line, np.uint8).reshape(-1)
    ot = np.ascontiguousarray(offset_time, np.uint32).reshape(-1)
    if not (len(p) == len(r) == len(ln) == len(ot)):
        raise ValueError("the message's arrays differ in length")
    return p, r, ln, ot


def _split(flat, sizes):
    out, o = [], 0
    for m in sizes:
        out.append(flat[o:o + m].copy())
        o += m
    return out


def extract_host(params: L.SlioLlregParams, xyz=None, reflectivity=None, line=None, offset_time=None, cloud=None):
    """The node on the host, as its literal serial loops: the CustomMsg path
    from (xyz, reflectivity, line, offset_time), or the Pc2 path from cloud
    (n, 4).  Returns dict(cloud, corner, surf, counts, line_size, finite_size,
    flags, visited, lines), the last three as one array per line."""
    lib = L.load()
    n = len(np.asarray(cloud).reshape(-1, 4)) if cloud is not None else len(np.asarray(xyz).reshape(-1, 3))
    cap = max(n, 1)
    full, corner, surf = (np.zeros((cap, POINT_FLOATS), np.float32) for _ in range(3))
    counts, ls, fs = np.zeros(3, np.int32), np.zeros(MAX_SCANS, np.int32), np.zeros(MAX_SCANS, np.int32)
    flags, vis, lines = np.zeros(cap, np.int32), np.zeros(cap, np.uint8), np.zeros((cap, 4), np.float32)
    outs = (L.fptr(full), L.fptr(corner), L.fptr(surf), L.iptr(counts), L.iptr(ls), L.iptr(fs), L.iptr(flags),
            L.u8ptr(vis), L.fptr(lines))
    if cloud is not None:
        c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        L.check(lib.slio_llreg_extract_pc2_host(C.byref(params), L.fptr(c), n, *outs), "llreg_extract_pc2_host")
    else:
        p, r, ln, ot = _msg(xyz, reflectivity, line, offset_time)
        L.check(lib.slio_llreg_extract_host(C.byref(params), L.fptr(p), L.u8ptr(r), L.u8ptr(ln), L.u32ptr(ot), n,
                                            *outs), "llreg_extract_host")
    nn, nc, ns = (int(v) for v in counts)
    sizes = [int(v) for v in fs]
    return dict(cloud=full[:nn].copy(), corner=corner[:nc].copy(), surf=surf[:ns].copy(), counts=counts,
                line_size=ls, finite_size=fs, flags=_split(flags, sizes), visited=_split(vis, sizes),
                lines=_split(lines, sizes))


class LioLivoxScanRegistration:
    """ScanRegistration's two callbacks for Use_seg = 0 on the device."""

    def __init__(self, device: int = 0, max_points: int = MAX_POINTS, **config):
        self.lib = L.load()
        self.params = make_params(device, max_points, **config)
        self.h = C.c_void_p()
        L.check(self.lib.slio_llreg_create(C.byref(self.h), C.byref(self.params)), "llreg_create")
        self.counts = np.zeros(3, np.int32)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_llreg_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def run(self, xyz, reflectivity, line, offset_time) -> np.ndarray:
        """FeatureExtract alone; the clouds stay on the device.  Returns the
        sizes of {laserCloud, laserConerFeature, laserSurfFeature}."""
        p, r, ln, ot = _msg(xyz, reflectivity, line, offset_time)
        counts = np.zeros(3, np.int32)
        L.check(self.lib.slio_llreg_run(self.h, L.fptr(p), L.u8ptr(r), L.u8ptr(ln), L.u32ptr(ot), len(p),
                                        L.iptr(counts)), "llreg_run")
        self.counts = counts
        return counts

    def run_pc2(self, cloud) -> np.ndarray:
        """lidarCallBackPc2 alone; the clouds stay on the device."""
        c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        counts = np.zeros(3, np.int32)
        L.check(self.lib.slio_llreg_run_pc2(self.h, L.fptr(c), len(c), L.iptr(counts)), "llreg_run_pc2")
        self.counts = counts
        return counts

    def cloud(self, kind: int = FULL) -> np.ndarray:
        n = int(self.counts[kind])
        out = np.zeros((max(n, 1), POINT_FLOATS), np.float32)
        L.check(self.lib.slio_llreg_get_cloud(self.h, kind, L.fptr(out), n), "llreg_get_cloud")
        return out[:n]

    def _clouds(self):
        return self.cloud(FULL), self.cloud(CORNER), self.cloud(SURF)

    def FeatureExtract(self, xyz, reflectivity, line, offset_time):
        """LidarFeatureExtractor.cpp:1218-1291.  Returns (laserCloud,
        laserConerFeature, laserSurfFeature)."""
        self.run(xyz, reflectivity, line, offset_time)
        return self._clouds()

    def FeatureExtract_Mid(self, cloud):
        """ScanRegistration.cpp:61-93 with LidarFeatureExtractor.cpp:1352-1401.
        Returns (laser_cloud_custom, laserConerFeature, laserSurfFeature)."""
        self.run_pc2(cloud)
        return self._clouds()

    def lines(self):
        """(vlines[l]'s size, its finite points) for l < 6."""
        a, b = np.zeros(MAX_SCANS, np.int32), np.zeros(MAX_SCANS, np.int32)
        L.check(self.lib.slio_llreg_get_lines(self.h, L.iptr(a), L.iptr(b)), "llreg_get_lines")
        return a, b

    def flags(self, l: int):
        """(CloudFeatureFlag, the line-feature loop's visited mask, the finite
        points) of line l in the last run."""
        m = int(self.lines()[1][l])
        f, v, c = np.zeros(max(m, 1), np.int32), np.zeros(max(m, 1), np.uint8), np.zeros((max(m, 1), 4), np.float32)
        L.check(self.lib.slio_llreg_get_flags(self.h, l, L.iptr(f), L.u8ptr(v), L.fptr(c), m), "llreg_get_flags")
        return f[:m], v[:m], c[:m]

    def view(self) -> L.SlioLlregView:
        """Device pointers to the three clouds of the last run."""
        v = L.SlioLlregView()
        L.check(self.lib.slio_llreg_get_view(self.h, C.byref(v)), "llreg_get_view")
        return v
