"""livox_mapping's laserMapping node (src/livox_mapping/src/laserMapping.cpp)
on the device: the rolling cube map behind the reference's names, the
slio_lvx_* entries of include/slio.h.

``LivoxCubeMap`` is laserCloudCornerArray / laserCloudSurfArray with the steps
of the main loop that touch them: the cube selection with its shifts
(:475-776), the map update with the per-cube VoxelGrids (:1159-1216) and the
surround clouds (:1218-1224).  ``LivoxMapping`` adds the scans, the search
grids over the valid cubes, the fused 5-NN / 8-NN pass, the optimisation loop
(:814-1155) and ``process``, one call of the node's main loop.  Poses are
float32 ``{rx, ry, rz, tx, ty, tz}``, clouds (n, 3) float32.  The stated departures are listed in slio.h and DESIGN.md
§3.14.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib as L

CORNER, SURF = 0, 1
NUM_CUBES = 4851          # laserCloudNum
WIDTH, HEIGHT, DEPTH = 21, 11, 21


def _xyz(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).reshape(-1, 3)


def _pose(tf) -> np.ndarray:
    t = np.ascontiguousarray(tf, np.float32).reshape(-1)
    if t.size != 6:
        raise ValueError("a pose is {rx, ry, rz, tx, ty, tz}")
    return t


def _cubes(inds):
    if inds is None:
        return None, 0
    a = np.ascontiguousarray(inds, np.int32).reshape(-1)
    if a.size == 0:
        return np.zeros(1, np.int32), 0     # an empty list, not "the last list" (NULL)
    return a, a.size


def cube_index(t: float, cen: int) -> int:
    """int((t + 25.0) / 50.0) + cen, one less when t + 25.0 < 0 (:482-491)."""
    out = C.c_int32()
    L.check(L.load().slio_lvx_cube_index(float(np.float32(t)), int(cen), C.byref(out)), "lvx_cube_index")
    return out.value


def select_cubes_host(transform, cen):
    """:475-776 on the host alone.  Returns (cen after the shifts, centre cube,
    shift, laserCloudValidInd, laserCloudSurroundInd)."""
    tf = _pose(transform)
    cen = np.array(cen, np.int32)
    ctr, shift = np.zeros(3, np.int32), np.zeros(3, np.int32)
    v, s = np.zeros(125, np.int32), np.zeros(125, np.int32)
    nv, ns = C.c_int32(), C.c_int32()
    L.check(L.load().slio_lvx_select_host(L.fptr(tf), L.iptr(cen), L.iptr(ctr), L.iptr(shift), L.iptr(v),
                                          C.byref(nv), L.iptr(s), C.byref(ns)), "lvx_select_host")
    return cen, ctr, shift, v[:nv.value].copy(), s[:ns.value].copy()


def plane_solve(neighbours, m: int = 10):
    """The surf branch's plane system (:962-975): x of matA0 x = matB0, or
    None where cv::solve gives up."""
    nb = np.ascontiguousarray(neighbours, np.float32).reshape(-1)
    if nb.size != 24:
        raise ValueError("eight neighbours")
    x = np.zeros(3, np.float32)
    rc = L.load().slio_lvx_plane_solve(L.fptr(nb), m, L.fptr(x))
    if rc == 1:
        return None
    L.check(rc, "lvx_plane_solve")
    return x


def lm_step(AtA, AtB, nsel: int, iter_count: int, transform, is_degenerate: int, matP):
    """:1040-1150 after the normal equations.  Returns (stepped, converged,
    transform, is_degenerate, matP); stepped is False for the `continue` of
    fewer than 50 rows."""
    a = np.ascontiguousarray(AtA, np.float32).reshape(-1)
    b = np.ascontiguousarray(AtB, np.float32).reshape(-1)
    tf = _pose(transform).copy()
    P = np.zeros(36, np.float32) if matP is None else np.array(matP, np.float32).reshape(-1)
    deg, conv = C.c_int(int(is_degenerate)), C.c_int(0)
    rc = L.load().slio_lvx_lm_step(L.fptr(a), L.fptr(b), int(nsel), int(iter_count), L.fptr(tf), C.byref(deg),
                                   L.fptr(P), C.byref(conv))
    if rc not in (0, 1):
        L.check(rc, "lvx_lm_step")
    return rc == 0, bool(conv.value), tf, deg.value, P


class LivoxCubeMap:
    """laserCloudCornerArray / laserCloudSurfArray on the device."""

    def __init__(self, device: int = 0, leaf_corner: float = 0.2, leaf_surf: float = 0.4,
                 max_points: int = 1 << 21):
        self.lib = L.load()
        p = L.SlioLvxParams()
        L.check(self.lib.slio_lvx_params_default(C.byref(p)), "lvx_params_default")
        p.device, p.leaf_corner, p.leaf_surf, p.max_points = device, leaf_corner, leaf_surf, max_points
        self.h = C.c_void_p()
        L.check(self.lib.slio_lvx_create(C.byref(self.h), C.byref(p)), "lvx_create")
        self.laserCloudValidInd = np.zeros(0, np.int32)
        self.laserCloudSurroundInd = np.zeros(0, np.int32)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.slio_lvx_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    def clear(self) -> None:
        L.check(self.lib.slio_lvx_clear(self.h), "lvx_clear")

    @property
    def laserCloudCen(self) -> np.ndarray:
        """laserCloudCenWidth / Height / Depth."""
        c = np.zeros(3, np.int32)
        L.check(self.lib.slio_lvx_get_centers(self.h, L.iptr(c)), "lvx_get_centers")
        return c

    def select_cubes(self, transformTobeMapped):
        """:475-776.  Returns (centerCube I / J / K, laserCloudValidInd,
        laserCloudSurroundInd); the map is shifted when the centre is within 3
        cubes of an edge."""
        tf = _pose(transformTobeMapped)
        ctr = np.zeros(3, np.int32)
        v, s = np.zeros(125, np.int32), np.zeros(125, np.int32)
        nv, ns = C.c_int32(), C.c_int32()
        L.check(self.lib.slio_lvx_select_cubes(self.h, L.fptr(tf), L.iptr(ctr), L.iptr(v), C.byref(nv), L.iptr(s),
                                               C.byref(ns)), "lvx_select_cubes")
        self.laserCloudValidInd = v[:nv.value].copy()
        self.laserCloudSurroundInd = s[:ns.value].copy()
        return ctr, self.laserCloudValidInd, self.laserCloudSurroundInd

    def update_map(self, transformTobeMapped, corner_last, surf_last_down, valid=None):
        """:1159-1216: both scans appended at the pose, then every valid cube
        (default: the last select_cubes list) through its VoxelGrid.  Returns
        the classes' totals."""
        tf = _pose(transformTobeMapped)
        c, s = _xyz(corner_last), _xyz(surf_last_down)
        v, nv = _cubes(valid)
        counts = np.zeros(2, np.int64)
        L.check(self.lib.slio_lvx_update_map(self.h, L.fptr(tf), L.fptr(c), c.shape[0], L.fptr(s), s.shape[0],
                                             None if v is None else L.iptr(v), nv, L.i64ptr(counts)),
                "lvx_update_map")
        return counts

    def cube_sizes(self, kind: int) -> np.ndarray:
        out = np.zeros(NUM_CUBES, np.int32)
        L.check(self.lib.slio_lvx_cube_sizes(self.h, kind, L.iptr(out)), "lvx_cube_sizes")
        return out

    def get_cube(self, kind: int, ind: int) -> np.ndarray:
        n = C.c_int64()
        L.check(self.lib.slio_lvx_get_cube(self.h, kind, ind, None, 0, C.byref(n)), "lvx_get_cube")
        out = np.zeros((n.value, 3), np.float32)
        if n.value:
            L.check(self.lib.slio_lvx_get_cube(self.h, kind, ind, L.fptr(out), n.value, C.byref(n)), "lvx_get_cube")
        return out

    def _surround(self, kind: int, cubes=None) -> np.ndarray:
        v, nv = _cubes(cubes)
        ptr = None if v is None else L.iptr(v)
        n = C.c_int64()
        L.check(self.lib.slio_lvx_get_surround(self.h, kind, ptr, nv, None, 0, C.byref(n)), "lvx_get_surround")
        out = np.zeros((n.value, 3), np.float32)
        if n.value:
            L.check(self.lib.slio_lvx_get_surround(self.h, kind, ptr, nv, L.fptr(out), n.value, C.byref(n)),
                    "lvx_get_surround")
        return out

    def laserCloudSurround(self, cubes=None) -> np.ndarray:
        """laserCloudSurround2 (:1218-1224): the surf class of the surround cubes."""
        return self._surround(SURF, cubes)

    def laserCloudSurround_corner(self, cubes=None) -> np.ndarray:
        """laserCloudSurround2_corner."""
        return self._surround(CORNER, cubes)

    def laserCloudFromMap(self, kind: int, valid=None) -> np.ndarray:
        """laserCloudCornerFromMap (kind 0) / laserCloudSurfFromMap (kind 1),
        :778-785: the valid cubes' clouds in laserCloudValidInd order, unfiltered
        (default: the last select_cubes list)."""
        return self._surround(kind, self.laserCloudValidInd if valid is None else valid)


class LivoxMapping(LivoxCubeMap):
    """The node's main loop (:457-1246) without ROS: ``process`` per pair of
    feature clouds; the lockstep methods are its stages."""

    def process(self, corner_last, surf_last) -> np.ndarray:
        """One call of the main loop; returns transformAftMapped."""
        c, s = _xyz(corner_last), _xyz(surf_last)
        aft, it = np.zeros(6, np.float32), C.c_int32()
        L.check(self.lib.slio_lvx_process(self.h, L.fptr(c), c.shape[0], L.fptr(s), s.shape[0], L.fptr(aft),
                                          C.byref(it)), "lvx_process")
        self.iterations = it.value
        return aft

    def _transforms(self):
        t = [np.zeros(6, np.float32) for _ in range(3)]
        L.check(self.lib.slio_lvx_get_transforms(self.h, *(L.fptr(v) for v in t)), "lvx_get_transforms")
        return t

    @property
    def transformTobeMapped(self) -> np.ndarray:
        return self._transforms()[0]

    @transformTobeMapped.setter
    def transformTobeMapped(self, tf) -> None:
        L.check(self.lib.slio_lvx_set_transform(self.h, L.fptr(_pose(tf))), "lvx_set_transform")

    @property
    def transformAftMapped(self) -> np.ndarray:
        return self._transforms()[1]

    @property
    def transformLastMapped(self) -> np.ndarray:
        return self._transforms()[2]

    # -- lockstep
    def feed_host(self, corner_last, surf_last):
        """laserCloudCornerLast as it is, laserCloudSurfLast through
        downSizeFilterSurf; returns the two sizes."""
        c, s = _xyz(corner_last), _xyz(surf_last)
        counts = np.zeros(2, np.int64)
        L.check(self.lib.slio_lvx_feed_host(self.h, L.fptr(c), c.shape[0], L.fptr(s), s.shape[0], L.i64ptr(counts)),
                "lvx_feed_host")
        self.scan_counts = counts
        return counts

    def feed_device(self, reg):
        """feed_host from the clouds the last run of ``reg`` (a
        livox_reg.LivoxScanRegistration) left on the device: cornerPointsSharp
        as it is, surfPointsFlat through downSizeFilterSurf; nothing crosses
        PCIe.  Returns the two sizes."""
        counts = np.zeros(2, np.int64)
        L.check(self.lib.slio_lvx_feed_device(self.h, reg.h, L.i64ptr(counts)), "lvx_feed_device")
        self.scan_counts = counts
        return counts

    def process_cloud(self, reg, cloud) -> np.ndarray:
        """From the sensor's cloud (n, 4) to a pose: the registration on
        ``reg``, then ``process`` with the device feed.  Returns
        transformAftMapped; ``reg.counts`` holds the registration's sizes."""
        c = np.ascontiguousarray(cloud, np.float32).reshape(-1, 4)
        aft, it, counts = np.zeros(6, np.float32), C.c_int32(), np.zeros(3, np.int32)
        L.check(self.lib.slio_lvx_process_cloud(self.h, reg.h, L.fptr(c), c.shape[0], L.fptr(aft), C.byref(it),
                                                L.iptr(counts)), "lvx_process_cloud")
        self.iterations = it.value
        reg.counts = counts
        return aft

    def scan(self, kind: int) -> np.ndarray:
        n = C.c_int64()
        L.check(self.lib.slio_lvx_get_scan(self.h, kind, None, 0, C.byref(n)), "lvx_get_scan")
        out = np.zeros((n.value, 3), np.float32)
        if n.value:
            L.check(self.lib.slio_lvx_get_scan(self.h, kind, L.fptr(out), n.value, C.byref(n)), "lvx_get_scan")
        return out

    def build_maps(self, valid=None):
        v, nv = _cubes(valid)
        counts = np.zeros(2, np.int64)
        L.check(self.lib.slio_lvx_build_maps(self.h, None if v is None else L.iptr(v), nv, L.i64ptr(counts)),
                "lvx_build_maps")
        self.map_counts = counts
        return counts

    def pass_(self, kind: int, transform) -> int:
        n = C.c_int64()
        L.check(self.lib.slio_lvx_pass(self.h, kind, L.fptr(_pose(transform)), C.byref(n)), "lvx_pass")
        return n.value

    def get_pass(self, kind: int):
        """dict(world, nbr_idx, nbr_sqd, coeff, sel) of the kind's last pass."""
        n, K = int(self.scan_counts[kind]), 5 if kind == 0 else 8
        out = dict(world=np.zeros((n, 3), np.float32), nbr_idx=np.zeros((n, K), np.int32),
                   nbr_sqd=np.zeros((n, K), np.float32), coeff=np.zeros((n, 4), np.float32),
                   sel=np.zeros(n, np.uint8))
        L.check(self.lib.slio_lvx_get_pass(self.h, kind, L.fptr(out["world"]), L.iptr(out["nbr_idx"]),
                                           L.fptr(out["nbr_sqd"]), L.fptr(out["coeff"]), L.u8ptr(out["sel"])),
                "lvx_get_pass")
        return out

    def normal_equations(self):
        AtA, AtB, n = np.zeros(36, np.float32), np.zeros(6, np.float32), C.c_int64()
        L.check(self.lib.slio_lvx_normal_equations(self.h, L.fptr(AtA), L.fptr(AtB), C.byref(n)),
                "lvx_normal_equations")
        return AtA, AtB, n.value

    def optimize(self, transform):
        """:814-1151 from `transform`; returns (transform, iterations, is_degenerate)."""
        tf = _pose(transform).copy()
        it, deg = C.c_int32(), C.c_int32()
        L.check(self.lib.slio_lvx_optimize(self.h, L.fptr(tf), C.byref(it), C.byref(deg)), "lvx_optimize")
        return tf, it.value, deg.value

