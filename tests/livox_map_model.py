"""numpy restatement of the parts of livox_mapping's laserMapping node that the
library has on the device or as host formulas (slio_lvx_*, include/slio.h).
path:line below are in src/livox_mapping/src/laserMapping.cpp of the reference
workspace.  float32 where the reference computes in float, float64 where it
writes a double literal into the expression; sin / cos / sqrt of a float are the
double functions.

  to_map            pointAssociateToMap                              :195-217
  cube_index        int((t + 25.0) / 50.0) + cen, -- when negative   :482-491, :1162-1168
  select            pointOnYAxis, centre cube, shifts, FOV test      :475-776
  CubeMap           laserCloud{Corner,Surf}Array with the shifts,    :493-713, :1159-1224
                    the push_backs and the per-cube VoxelGrids
  plane_system      matA0 (10 x 3, two zero rows) x = matB0 (-1)     :423-425, :962-975
  lm_step           solve, degeneracy projection, update, deltas     :1102-1150
  coeffs            corner (5-NN, gate 1.5) / surf (8-NN, gate 5.0)  :825-1028
  optimize, Mapper  the loop and one call of the main loop           :814-1155, :475-1216

The VoxelGrid of a cube is oracle.voxel_grid of that cube's cloud; the OpenCV
solvers are the float32 restatements of tests/lego_map_model.py.
"""
import math

import numpy as np

import lego_map_model as LM
from lego_odom_model import fcos, fsin

F = np.float32
D = np.float64
W, H, DEPTH = 21, 11, 21          # laserCloudWidth / Height / Depth (:67-69)
NUM = W * H * DEPTH               # laserCloudNum (:71-72)


def to_map(tf, pts):
    """pointAssociateToMap (:195-217): yaw about z, roll about x, pitch about y,
    then the translation -- LeGO-LOAM's three float rotations."""
    return LM.to_map(tf, pts)


def cube_index(t, cen):
    """:482-491 / :1162-1168: the sum and the quotient in double, int()
    truncating, one less when the sum is negative."""
    v = D(F(t)) + 25.0
    c = int(v / 50.0) + cen
    if v < 0:
        c -= 1
    return c


def select(tf, cen):
    """:475-776.  cen = [laserCloudCenWidth, Height, Depth] is updated in place.
    Returns (centre cube [3], shift [3], valid list, surround list); shift[a]
    counts the turns of the `< 3` loop minus those of the `>= dim - 3` loop."""
    tf = np.asarray(tf, F)
    py = to_map(tf, np.array([[0.0, 10.0, 0.0]], F))[0]
    dim = (W, H, DEPTH)
    c, shift = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        c[a] = cube_index(tf[3 + a], cen[a])
        while c[a] < 3:
            c[a] += 1
            cen[a] += 1
            shift[a] += 1
        while c[a] >= dim[a] - 3:
            c[a] -= 1
            cen[a] -= 1
            shift[a] -= 1
    valid, surround = [], []
    k3 = 10.0 * math.sqrt(3.0)
    for i in range(c[0] - 2, c[0] + 3):
        for j in range(c[1] - 2, c[1] + 3):
            for k in range(c[2] - 2, c[2] + 3):
                if not (0 <= i < W and 0 <= j < H and 0 <= k < DEPTH):
                    continue
                ctr = [F(50.0 * (i - cen[0])), F(50.0 * (j - cen[1])), F(50.0 * (k - cen[2]))]
                in_fov = False
                for ii in (-1, 1):
                    for jj in (-1, 1):
                        for kk in (-1, 1):
                            cx = F(D(ctr[0]) + 25.0 * ii)
                            cy = F(D(ctr[1]) + 25.0 * jj)
                            cz = F(D(ctr[2]) + 25.0 * kk)
                            s1 = ((tf[3] - cx) * (tf[3] - cx) + (tf[4] - cy) * (tf[4] - cy)
                                  + (tf[5] - cz) * (tf[5] - cz))
                            s2 = ((py[0] - cx) * (py[0] - cx) + (py[1] - cy) * (py[1] - cy)
                                  + (py[2] - cz) * (py[2] - cz))
                            assert s1.dtype == F and s2.dtype == F
                            check1 = F(100.0 + D(s1) - D(s2) - k3 * math.sqrt(D(s1)))
                            check2 = F(100.0 + D(s1) - D(s2) + k3 * math.sqrt(D(s1)))
                            if check1 < 0 and check2 > 0:
                                in_fov = True
                ind = i + W * j + W * H * k
                if in_fov:
                    valid.append(ind)
                surround.append(ind)
    return c, shift, valid, surround


EMPTY = np.zeros((0, 3), F)


class CubeMap:
    """laserCloudCornerArray (kind 0) / laserCloudSurfArray (kind 1): a dict of
    cube index -> (n, 3) float32 cloud per class; absent = empty."""

    def __init__(self, voxel_grid, leaf_corner=0.2, leaf_surf=0.4):
        self.vg = voxel_grid
        self.leaf = (leaf_corner, leaf_surf)
        self.cubes = [{}, {}]
        self.cen = [10, 5, 10]
        self.valid, self.surround = [], []

    def shift(self, s):
        """The six while loops (:493-713), `s[a]` turns along each axis: every
        cube's cloud moves one index per turn, the clouds pushed out of the
        array come back cleared on the other side."""
        for kind in range(2):
            moved = {}
            for ind, cloud in self.cubes[kind].items():
                i, j, k = ind % W + s[0], ind // W % H + s[1], ind // (W * H) + s[2]
                if 0 <= i < W and 0 <= j < H and 0 <= k < DEPTH:
                    moved[i + W * j + W * H * k] = cloud
            self.cubes[kind] = moved

    def select(self, tf):
        c, s, self.valid, self.surround = select(tf, self.cen)
        if any(s):
            self.shift(s)
        return c, list(self.valid), list(self.surround)

    def update(self, tf, corner, surf, valid=None):
        """:1159-1216: push_back of both scans at the pose, then the VoxelGrid
        of every valid cube of both classes."""
        valid = self.valid if valid is None else valid
        for kind, scan in enumerate((corner, surf)):
            w = to_map(tf, scan)
            for p in w:
                ci, cj, ck = (cube_index(p[a], self.cen[a]) for a in range(3))
                if 0 <= ci < W and 0 <= cj < H and 0 <= ck < DEPTH:
                    ind = ci + W * cj + W * H * ck
                    old = self.cubes[kind].get(ind, EMPTY)
                    self.cubes[kind][ind] = np.concatenate([old, p[None, :]], 0)
            for ind in valid:
                cloud = self.cubes[kind].get(ind, EMPTY)
                if len(cloud):
                    self.cubes[kind][ind] = np.ascontiguousarray(self.vg(cloud, self.leaf[kind]), F)

    def cube(self, kind, ind):
        return self.cubes[kind].get(ind, EMPTY)

    def sizes(self, kind):
        out = np.zeros(NUM, np.int32)
        for ind, cloud in self.cubes[kind].items():
            out[ind] = len(cloud)
        return out

    def concat(self, kind, inds):
        return np.concatenate([EMPTY] + [self.cube(kind, i) for i in inds], 0)


def plane_system(nb, m=10):
    """:423-425, :962-975: matA0 is 10 x 3 of which only rows 0..7 are ever
    written, matB0 ten times -1; cv::solve(DECOMP_QR).  Returns x (float32[3])
    or None where the solve gives up."""
    A = np.zeros((m, 3), F)
    A[:8] = np.asarray(nb, F).reshape(8, 3)
    b = np.full(m, -1.0, F)
    x = LM.qr_solve(A.reshape(-1), b, m, 3)
    return None if x is None else np.array(x, F)


def lm_step(AtA, AtB, nsel, it, tf, state):
    """:1040-1150 after the normal equations; tf (float32[6]) updated in place,
    state = dict(is_degenerate, matP).  Returns (stepped, converged): stepped is
    False for the `continue` of :1040-1042."""
    if nsel < 50:
        return False, False
    X = LM.qr_solve(AtA, AtB, 6, 6)
    if X is None:
        X = [F(0)] * 6
    if it == 0:
        E, V = LM.jacobi(AtA, 6)
        V2 = list(V)
        state["is_degenerate"] = 0
        for i in range(5, -1, -1):
            if E[i] < F(1):                     # eignThre (:1114)
                for j in range(6):
                    V2[6 * i + j] = F(0)
                state["is_degenerate"] = 1
            else:
                break
        Vi = LM.inv_lu(V, 6)
        state["matP"] = [F(sum(D(Vi[6 * i + k]) * D(V2[6 * k + j]) for k in range(6))) for i in range(6)
                         for j in range(6)]
    if state["is_degenerate"]:
        P = state["matP"]
        X2 = []
        for i in range(6):
            s = D(0)
            for k in range(6):
                s = s + D(P[6 * i + k]) * D(X[k])
            X2.append(F(s))
        X = X2
    for k in range(6):
        tf[k] = tf[k] + X[k]
    # rad2deg (:139) is a double expression: radians * 180.0 / M_PI
    dR = F(math.sqrt(sum((D(X[k]) * 180.0 / math.pi) ** 2 for k in range(3))))
    dT = F(math.sqrt(sum(D(X[k] * F(100)) ** 2 for k in range(3, 6))))
    return True, bool(D(dR) < 0.05 and D(dT) < 0.05)


# ------------------------------------------------------------------ coefficients
GATE = (F(1.5), F(5.0))
KNN = (5, 8)


def surf_coeff8(nb, p):
    """:962-1026 on the eight neighbours nb and the map-frame point p.  Returns
    (coeff[4], selected, plane) -- plane False: the 0.2 check failed."""
    X = plane_system(nb, 10)
    if X is None:
        X = [F(0)] * 3        # cv::solve leaves matX zero
    pa, pb, pc, pd = X[0], X[1], X[2], F(1)
    with np.errstate(all="ignore"):
        ps = LM.fsqrt(pa * pa + pb * pb + pc * pc)
        pa, pb, pc, pd = pa / ps, pb / ps, pc / ps, pd / ps
        for j in range(8):
            if not D(abs(pa * nb[j][0] + pb * nb[j][1] + pc * nb[j][2] + pd)) <= 0.2:
                return np.zeros(4, F), 0, False
        x0, y0, z0 = p
        pd2 = pa * x0 + pb * y0 + pc * z0 + pd
        s = F(1.0 - 0.9 * D(abs(pd2)) / D(LM.fsqrt(LM.fsqrt(x0 * x0 + y0 * y0 + z0 * z0))))
        cf = np.array([s * pa, s * pb, s * pc, s * pd2], F)
    return cf, int(D(s) > 0.1), True


def coeffs(kind, world, map_xyz, idx, sqd):
    """Per point (coeff, sel, near) and the branch counts: gated (the K-th
    distance misses the gate, or fewer than K map points), rejected (eigenvalue
    ratio / plane check), weak (s <= 0.1), selected."""
    world = np.ascontiguousarray(world, F).reshape(-1, 3)
    n, K = world.shape[0], KNN[kind]
    coeff, sel, near = np.zeros((n, 4), F), np.zeros(n, np.uint8), np.zeros(n, bool)
    stats = dict(selected=0, gated=0, rejected=0, weak=0)
    for i in range(n):
        if not (idx.shape[1] >= K and sqd[i, K - 1] < GATE[kind]):
            stats["gated"] += 1
            continue
        near[i] = True
        nb = [[F(v) for v in map_xyz[idx[i, j]]] for j in range(K)]
        p = [F(v) for v in world[i]]
        cf, ok, shape_ok = (LM.corner_coeff if kind == 0 else surf_coeff8)(nb, p)
        coeff[i], sel[i] = cf, ok
        stats["selected"] += ok
        stats["rejected"] += 0 if shape_ok else 1
        stats["weak"] += 1 if (shape_ok and not ok) else 0
    return coeff, sel, near, stats


def tie_free(kind, sqd):
    """No query's K-th and (K+1)-th distances are equal, nor any two of its K
    nearest: the comparison never tests the tie rule."""
    K = KNN[kind]
    s = np.asarray(sqd)[:, :K + 1]
    return bool((np.diff(s, axis=1) > 0).all()) if s.shape[1] > 1 else True


def gate_clear(kind, sqd):
    """No K-th distance within 1 ulp of the gate."""
    K = KNN[kind]
    if np.asarray(sqd).shape[1] < K:
        return True
    d = np.asarray(sqd, F)[:, K - 1]
    g = GATE[kind]
    return bool(((d < np.nextafter(g, F(0))) | (d > np.nextafter(g, F(np.inf)))).all())


def optimize(tf, corner, surf_down, cmap, smap, knn, state):
    """:814-1151.  tf float32[6] in place; knn(kind, map, queries) -> (idx, sqd)
    with K columns; state = dict(is_degenerate, matP), the node's globals.
    Returns the number of turns (num_temp) and the per-turn trace."""
    trace = []
    if not (len(cmap) > 10 and len(smap) > 100):
        return 0, trace
    iters = 0
    for it in range(20):
        iters += 1
        clouds = []
        for kind, (scan, mp) in enumerate(((corner, cmap), (surf_down, smap))):
            world = to_map(tf, scan)
            idx, sqd = knn(kind, mp, world)
            cf, sel, _, _ = coeffs(kind, world, mp, idx, sqd)
            clouds.append((scan, cf, sel))
        AtA, AtB, nsel = LM.normal_equations(tf, clouds)
        stepped, conv = lm_step(AtA, AtB, nsel, it, tf, state)
        trace.append((nsel, tf.copy()))
        if stepped and conv:
            break
    return iters, trace


class Mapper(CubeMap):
    """One call of the main loop (:475-1216) on the cube map."""

    def __init__(self, voxel_grid, knn, leaf_corner=0.2, leaf_surf=0.4):
        super().__init__(voxel_grid, leaf_corner, leaf_surf)
        self.knn = knn
        self.tobe, self.aft, self.last = np.zeros(6, F), np.zeros(6, F), np.zeros(6, F)
        self.state = {"is_degenerate": 0, "matP": [F(0)] * 36}
        self.trace = []

    def process(self, corner, surf):
        corner = np.ascontiguousarray(corner, F).reshape(-1, 3)
        _, valid, _ = self.select(self.tobe)
        cmap, smap = self.concat(0, valid), self.concat(1, valid)
        surf_down = np.ascontiguousarray(self.vg(surf, self.leaf[1]), F).reshape(-1, 3)
        iters, self.trace = optimize(self.tobe, corner, surf_down, cmap, smap, self.knn, self.state)
        if iters:
            self.last[:] = self.aft
            self.aft[:] = self.tobe
        self.update(self.tobe, corner, surf_down)
        return iters

