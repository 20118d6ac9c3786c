"""numpy / plain-Python restatement of A-LOAM's laserMapping as the library
states it (include/slio_frontend.h, "A-LOAM laserMapping"; path:line below are
in src/A-LOAM/src/laserMapping.cpp of the reference workspace): the poses, the
cube indices, the shifts and the selection, the VoxelGrid as the cube store
states it, the exact 5-NN with ties to the lower index, the line fit on a
cyclic Jacobi eigen-solve, the plane fit on a column-pivoting Householder QR,
LidarEdgeFactor on double end points, LidarPlaneNormFactor, HuberLoss(0.1),
the sums in the stated order and the library's Levenberg-Marquardt.  It shares
no code with the library.  Doubles are Python floats (IEEE, never fused),
floats are numpy float32, so the library can be compared to it to the bit.
The controller, the weighting and the quaternion algebra are those of
tests/aloam_odom_model.py.  Quaternions are (x, y, z, w).
"""
import math

import numpy as np

import aloam_odom_model as OM

F = np.float32
W, H, D = 21, 21, 11
NUM = W * H * D
K, WG, LANES, SUMS = 5, 256, 32, 28
SWEEPS = 8
NONE, EDGE, PLANE, DEGENERATE, REJECTED = range(5)
EMPTY = np.zeros((0, 3), F)


# ---------------------------------------------------------------- poses
def associate_to_map(q_wmap, t_wmap, q_wodom, t_wodom):
    """:148-152 and :222-223."""
    r = OM.rotate(q_wmap, t_wodom)
    return OM.qmul(q_wmap, q_wodom), [r[a] + t_wmap[a] for a in range(3)]


def transform_update(q_w, t_w, q_wodom, t_wodom):
    """:155-158; inverse() = conjugate / squared norm."""
    n2 = ((q_wodom[0] * q_wodom[0] + q_wodom[1] * q_wodom[1]) + q_wodom[2] * q_wodom[2]) + q_wodom[3] * q_wodom[3]
    inv = [-q_wodom[0] / n2, -q_wodom[1] / n2, -q_wodom[2] / n2, q_wodom[3] / n2]
    q_wmap = OM.qmul(q_w, inv)
    r = OM.rotate(q_wmap, t_wodom)
    return q_wmap, [t_w[a] - r[a] for a in range(3)]


def to_map(q, t, pts):
    """pointAssociateToMap (:160-168) on (n, 3) float32: (n, 3) float32."""
    out = np.zeros((len(pts), 3), F)
    with np.errstate(all="ignore"):
        for i, p in enumerate(pts):
            out[i] = OM.to_start(q, t, p)
    return out


# ---------------------------------------------------------------- cubes
def cube_index(v, cen):
    """int((v + 25.0) / 50.0) + cen, one less when the sum is negative; v a
    Python float (the centre, :331-338) or the double of a float32 (:839-845).
    None where the library drops the coordinate."""
    s = float(v) + 25.0
    if not abs(s) < 1.0e6:
        return None
    c = int(s / 50.0) + cen
    return c - 1 if s < 0 else c


def select(t_w, cen):
    """:331-583.  cen is updated in place.  Returns (centre, shift, cube list)."""
    dim = (W, H, D)
    c, shift = [0, 0, 0], [0, 0, 0]
    for a in range(3):
        c[a] = cube_index(t_w[a], cen[a])
        while c[a] < 3:
            c[a] += 1
            cen[a] += 1
            shift[a] += 1
        while c[a] >= dim[a] - 3:
            c[a] -= 1
            cen[a] -= 1
            shift[a] -= 1
    lst = []
    for i in range(c[0] - 2, c[0] + 3):
        for j in range(c[1] - 2, c[1] + 3):
            for k in range(c[2] - 1, c[2] + 2):
                if 0 <= i < W and 0 <= j < H and 0 <= k < D:
                    lst.append(i + W * j + W * H * k)
    return c, shift, lst


def voxel_grid(pts, leaf):
    """The cube store's VoxelGrid of one (n, 3) float32 cloud: PCL's grid from
    the bounding box, a stable sort by voxel, float32 sums in the sorted order
    divided by the count; a leaf too small for the cloud passes it through;
    points that are not finite are dropped first."""
    pts = np.ascontiguousarray(pts, F).reshape(-1, 3)
    pts = pts[np.isfinite(pts).all(1)]
    if len(pts) == 0:
        return EMPTY
    mn, mx = pts.min(0), pts.max(0)
    inv = F(1) / F(leaf)
    dd = []
    for a in range(3):
        span = F(mx[a] - mn[a]) * inv
        dd.append(int(np.trunc(span)) + 1 if np.isfinite(span) and span < F(9.2e18) else 2 ** 61)
    if max(dd) > 2147483647 or dd[0] * dd[1] > 2147483647 or dd[0] * dd[1] * dd[2] > 2147483647:
        return pts.copy()
    minb = [int(np.floor(mn[a] * inv)) for a in range(3)]
    div = [int(np.floor(mx[a] * inv)) - minb[a] + 1 for a in range(3)]
    mul = (1, div[0], div[0] * div[1])
    idx = np.zeros(len(pts), np.int64)
    for a in range(3):
        idx += (np.floor(pts[:, a] * inv) - F(minb[a])).astype(np.int64) * mul[a]
    order = np.argsort(idx, kind="stable")
    si = idx[order]
    cuts = np.flatnonzero(np.r_[True, si[1:] != si[:-1], True])
    out = np.zeros((len(cuts) - 1, 3), F)
    for k in range(len(cuts) - 1):
        run = pts[order[cuts[k]:cuts[k + 1]]]
        out[k] = np.cumsum(run, axis=0, dtype=F)[-1] / F(len(run))
    return out


# ---------------------------------------------------------------- the fits
def jacobi3(m):
    """(eigenvalues[3], V with the eigenvectors in its columns) of the symmetric
    {xx, xy, xz, yy, yz, zz}: SWEEPS sweeps over (0,1), (0,2), (1,2)."""
    A = [[m[0], m[1], m[2]], [m[1], m[3], m[4]], [m[2], m[4], m[5]]]
    V = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]
    for _ in range(SWEEPS):
        for p, q, r in ((0, 1, 2), (0, 2, 1), (1, 2, 0)):
            apq = A[p][q]
            if apq == 0.0:
                continue
            with np.errstate(all="ignore"):
                theta = float(np.float64(A[q][q] - A[p][p]) / np.float64(2.0 * apq))
                t = float(np.float64(1.0) / (np.float64(abs(theta)) + np.sqrt(np.float64(theta) * np.float64(theta)
                                                                              + np.float64(1.0))))
            if theta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(t * t + 1.0)
            s = t * c
            A[p][p] = A[p][p] - t * apq
            A[q][q] = A[q][q] + t * apq
            A[p][q] = A[q][p] = 0.0
            arp, arq = A[r][p], A[r][q]
            A[r][p] = A[p][r] = c * arp - s * arq
            A[r][q] = A[q][r] = s * arp + c * arq
            for k in range(3):
                vp, vq = V[k][p], V[k][q]
                V[k][p] = c * vp - s * vq
                V[k][q] = s * vp + c * vq
    return [A[0][0], A[1][1], A[2][2]], V


def covariance(nb):
    c = [0.0, 0.0, 0.0]
    for p in nb:
        for k in range(3):
            c[k] = c[k] + p[k]
    c = [v / 5.0 for v in c]
    m = [0.0] * 6
    for p in nb:
        z = [p[k] - c[k] for k in range(3)]
        m[0] = m[0] + z[0] * z[0]
        m[1] = m[1] + z[0] * z[1]
        m[2] = m[2] + z[0] * z[2]
        m[3] = m[3] + z[1] * z[1]
        m[4] = m[4] + z[1] * z[2]
        m[5] = m[5] + z[2] * z[2]
    return c, m


def fit_line(nb):
    """(kind, record[6] = a, b) of five neighbours (lists of 3 Python floats)."""
    c, m = covariance(nb)
    lam, V = jacobi3(m)
    hi = (2 if lam[2] > lam[1] else 1) if lam[1] > lam[0] else (2 if lam[2] > lam[0] else 0)
    o1, o2 = (1 if hi == 0 else 0), (1 if hi == 2 else 2)
    mid = lam[o2] if lam[o2] > lam[o1] else lam[o1]
    if not lam[hi] > 0.0 or not math.isfinite(lam[hi]):
        return DEGENERATE, [0.0] * 6
    if not lam[hi] > 3.0 * mid:
        return REJECTED, [0.0] * 6
    d = [V[k][hi] for k in range(3)]
    return EDGE, [0.1 * d[k] + c[k] for k in range(3)] + [-0.1 * d[k] + c[k] for k in range(3)]


def qr_solve_m1(nb):
    """(rank, x) of A x = -1 by Eigen's ColPivHouseholderQR on doubles, every
    reduction summed left to right."""
    eps, tiny = 2.220446049250313e-16, 2.2250738585072014e-308
    a = [[nb[r][c] for r in range(K)] for c in range(3)]         # a[column][row]
    nd, nu = [0.0] * 3, [0.0] * 3
    for c in range(3):
        s = a[c][0] * a[c][0]
        for r in range(1, K):
            s = s + a[c][r] * a[c][r]
        nd[c] = nu[c] = math.sqrt(s)
    mx = nu[0]
    if nu[1] > mx:
        mx = nu[1]
    if nu[2] > mx:
        mx = nu[2]
    th = mx * eps
    helper = (th * th) / 5.0
    down = math.sqrt(eps)
    nzp, perm, hc = 3, [0, 1, 2], [0.0] * 3
    for k in range(3):
        big, bv = k, nu[k]
        for j in range(k + 1, 3):
            if nu[j] > bv:
                bv, big = nu[j], j
        if nzp == 3 and bv * bv < helper * float(K - k):
            nzp = k
        if big != k:
            a[k], a[big] = a[big], a[k]
            nu[k], nu[big] = nu[big], nu[k]
            nd[k], nd[big] = nd[big], nd[k]
            perm[k], perm[big] = perm[big], perm[k]
        tail = 0.0
        for r in range(k + 1, K):
            tail = a[k][r] * a[k][r] if r == k + 1 else tail + a[k][r] * a[k][r]
        c0 = a[k][k]
        if tail <= tiny:
            tau, beta = 0.0, c0
            for r in range(k + 1, K):
                a[k][r] = 0.0
        else:
            beta = math.sqrt(c0 * c0 + tail)
            if c0 >= 0.0:
                beta = -beta
            den = c0 - beta
            for r in range(k + 1, K):
                a[k][r] = a[k][r] / den
            tau = (beta - c0) / beta
        a[k][k] = beta
        hc[k] = tau
        if tau != 0.0:
            for j in range(k + 1, 3):
                t = 0.0
                for r in range(k + 1, K):
                    t = a[k][r] * a[j][r] if r == k + 1 else t + a[k][r] * a[j][r]
                t = t + a[j][k]
                a[j][k] = a[j][k] - tau * t
                for r in range(k + 1, K):
                    a[j][r] = a[j][r] - (tau * a[k][r]) * t
        for j in range(k + 1, 3):
            if nu[j] != 0.0:
                temp = abs(a[j][k]) / nu[j]
                temp = (1.0 + temp) * (1.0 - temp)
                temp = 0.0 if temp < 0.0 else temp
                q = nu[j] / nd[j]
                if temp * (q * q) <= down:
                    s = 0.0
                    for r in range(k + 1, K):
                        s = a[j][r] * a[j][r] if r == k + 1 else s + a[j][r] * a[j][r]
                    nd[j] = nu[j] = math.sqrt(s)
                else:
                    nu[j] = nu[j] * math.sqrt(temp)
    sol = [0.0] * 3
    if nzp > 0:
        c = [-1.0] * K
        for k in range(3):
            if k < nzp and hc[k] != 0.0:
                t = 0.0
                for r in range(k + 1, K):
                    t = a[k][r] * c[r] if r == k + 1 else t + a[k][r] * c[r]
                t = t + c[k]
                c[k] = c[k] - hc[k] * t
                for r in range(k + 1, K):
                    c[r] = c[r] - (hc[k] * a[k][r]) * t
        for i in range(2, -1, -1):
            if i < nzp and c[i] != 0.0:
                with np.errstate(all="ignore"):
                    c[i] = float(np.float64(c[i]) / np.float64(a[i][i]))    # (a zero pivot gives inf, as in C)
                for r in range(i):
                    c[r] = c[r] - c[i] * a[i][r]
        for i in range(nzp):
            sol[perm[i]] = c[i]
    return nzp, sol


def fit_plane(nb):
    """(kind, record[6] = n, d, 0, 0)."""
    rank, x = qr_solve_m1(nb)
    ln = math.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    if rank < 3 or ln == 0.0:
        return DEGENERATE, [0.0] * 6
    d = 1.0 / ln
    n = [v / ln for v in x]
    if not all(math.isfinite(v) for v in n + [d]):
        return DEGENERATE, [0.0] * 6
    for p in nb:
        if abs(((n[0] * p[0] + n[1] * p[1]) + n[2] * p[2]) + d) > 0.2:
            return REJECTED, [0.0] * 6
    return PLANE, n + [d, 0.0, 0.0]


# ---------------------------------------------------------------- association
def knn5(mp, w):
    """The five nearest of the (n, 3) float32 map to the float32 point w, ties
    to the lower index: (indices, float32 squared distances), or None where
    fewer than five points or a fifth distance not below 1.0."""
    if len(mp) < K or not np.isfinite(w).all():
        return None
    d = mp - w[None, :]
    d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)
    order = np.argsort(d2, kind="stable")[:K]
    if not d2[order[K - 1]] < F(1.0):
        return None
    return order, d2[order]


def associate(surf, stack, mp, q, t):
    """Per point of the (n, 3) stack: kind (uint8), record (n, 6), neighbour
    indices (n, 5; -1) and squared distances (n, 5; inf)."""
    n = len(stack)
    kind, rec = np.zeros(n, np.uint8), np.zeros((n, 6))
    idx, sqd = np.full((n, K), -1, np.int32), np.full((n, K), np.inf, F)
    world = to_map(q, t, stack)
    for i in range(n):
        nn = knn5(mp, world[i])
        if nn is None:
            continue
        idx[i], sqd[i] = nn
        nb = [[float(v) for v in mp[j]] for j in nn[0]]
        with np.errstate(all="ignore"):
            kind[i], rec[i] = (fit_plane if surf else fit_line)(nb)
    return kind, rec, idx, sqd


# ---------------------------------------------------------------- factors and sums
def plane_norm_factor(q, t, cp, n, d):
    """LidarPlaneNormFactor (lidarFactor.hpp:127-164)."""
    rc = OM.rotate(q, cp)
    lp = [rc[k] + t[k] for k in range(3)]
    return [((n[0] * lp[0] + n[1] * lp[1]) + n[2] * lp[2]) + d], [OM.cross(rc, n) + list(n)]


def slot_factor(q, t, cp, kind, rec):
    if kind == EDGE:
        return OM.edge_factor(q, t, cp, list(rec[:3]), list(rec[3:6]))
    if kind == PLANE:
        return plane_norm_factor(q, t, cp, list(rec[:3]), rec[3])
    return None


def _two_step(items, n):
    """items: index -> 28 values (absent: skipped); lane l adds the indices l,
    l + LANES, ... < n in ascending order, then the lanes in ascending order."""
    tot = [0.0] * SUMS
    parts = []
    for l in range(LANES):
        acc = [0.0] * SUMS
        for s in range(l, n, LANES):
            c = items.get(s)
            if c is not None:
                for k in range(SUMS):
                    acc[k] = acc[k] + c[k]
        parts.append(acc)
    for l in range(LANES):
        for k in range(SUMS):
            tot[k] = tot[k] + parts[l][k]
    return tot


def evaluate(xyz, kind, rec, q, t):
    """A (21), g (6), cost, counts {edge, plane, degenerate, outliers} over the
    slots, in the stated order: per WG slots, then over the groups."""
    q, t = [float(v) for v in q], [float(v) for v in t]
    n = len(xyz)
    counts = [int((kind == EDGE).sum()), int((kind == PLANE).sum()), int((kind == DEGENERATE).sum()), 0]
    groups = {}
    for w in range((n + WG - 1) // WG):
        items = {}
        m = min(WG, n - w * WG)
        for i in range(m):
            s = w * WG + i
            f = slot_factor(q, t, [float(v) for v in xyz[s]], int(kind[s]), [float(v) for v in rec[s]])
            if f is None:
                continue
            c, out = OM.contributions(*f)
            counts[3] += int(out)
            items[i] = c
        groups[w] = _two_step(items, m)
    sums = _two_step(groups, len(groups))
    return sums[:21], sums[21:27], 0.5 * sums[27], counts


# ---------------------------------------------------------------- the node
class Mapper:
    """The node's state and loop body (:326-893)."""

    def __init__(self, leaf_corner=0.4, leaf_surf=0.8):
        self.leaf = (leaf_corner, leaf_surf)
        self.reset()

    def reset(self):
        self.cubes = [{}, {}]
        self.cen = [10, 10, 5]
        self.q_wmap, self.t_wmap = list(OM.IDENT_Q), list(OM.ZERO_T)
        self.stack = [EMPTY, EMPTY]
        self.assoc = None

    def cube(self, kind, ind):
        return self.cubes[kind].get(ind, EMPTY)

    def sizes(self, kind):
        out = np.zeros(NUM, np.int32)
        for ind, c in self.cubes[kind].items():
            out[ind] = len(c)
        return out

    def concat(self, kind, inds):
        return np.concatenate([EMPTY] + [self.cube(kind, i) for i in inds], 0)

    def one_pass(self, maps, q, t):
        nc = len(self.stack[0])
        a = [associate(k, self.stack[k], maps[k], q, t) for k in range(2)]
        kind, rec, idx, sqd = (np.concatenate([a[0][j], a[1][j]], 0) for j in range(4))
        self.assoc = (kind, rec, idx, sqd)
        xyz = np.concatenate(self.stack, 0)
        A, g, cost, cnt = evaluate(xyz, kind, rec, q, t)
        s = OM.Lm(q, t, A, g, cost)
        info = dict(corner=cnt[0], plane=cnt[1], degenerate=cnt[2], outliers=cnt[3], few=0, cost_first=cost,
                    iterates=[], nc=nc)
        while s.propose():
            An, gn, costn, cn = evaluate(xyz, kind, rec, s.qn, s.tn)
            s.decide(An, gn, costn)
            if s.last_accepted:
                info["outliers"] = cn[3]
            info["iterates"].append(dict(q=list(s.q), t=list(s.t), cost=s.cost, mu=s.mu, accepted=s.last_accepted))
        info.update(iterations=s.iterations, accepted=s.accepted, stop=s.stop, cost_last=s.cost)
        return s.q, s.t, info

    def process(self, corner_last, surf_last, q_wodom, t_wodom):
        q_wodom, t_wodom = [float(v) for v in q_wodom], [float(v) for v in t_wodom]
        clouds = [np.ascontiguousarray(c, F).reshape(-1, 4)[:, :3] for c in (corner_last, surf_last)]
        q, t = associate_to_map(self.q_wmap, self.t_wmap, q_wodom, t_wodom)
        center, shift, lst = select(t, self.cen)
        if any(shift):
            for kind in range(2):
                moved = {}
                for ind, cloud in self.cubes[kind].items():
                    i, j, k = ind % W + shift[0], ind // W % H + shift[1], ind // (W * H) + shift[2]
                    if 0 <= i < W and 0 <= j < H and 0 <= k < D:
                        moved[i + W * j + W * H * k] = cloud
                self.cubes[kind] = moved
        maps = [self.concat(k, lst) for k in range(2)]
        self.stack = [voxel_grid(clouds[k], self.leaf[k]) for k in range(2)]
        res = dict(center=center, shift=shift, nvalid=len(lst), valid=lst, map_size=[len(m) for m in maps],
                   stack_size=[len(s) for s in self.stack], passes=[])
        res["optimized"] = int(len(maps[0]) > 10 and len(maps[1]) > 50)
        self.assoc = None
        if res["optimized"]:
            for _ in range(2):
                q, t, info = self.one_pass(maps, q, t)
                res["passes"].append(info)
        self.q_wmap, self.t_wmap = transform_update(q, t, q_wodom, t_wodom)
        touched = set()
        for kind in range(2):
            world = to_map(q, t, self.stack[kind])
            add = {}
            for p in world:
                if not np.isfinite(p).all():
                    continue
                c = [cube_index(p[a], self.cen[a]) for a in range(3)]
                if None not in c and 0 <= c[0] < W and 0 <= c[1] < H and 0 <= c[2] < D:
                    add.setdefault(c[0] + W * c[1] + W * H * c[2], []).append(p)
            for ind, pts in add.items():
                self.cubes[kind][ind] = np.concatenate([self.cube(kind, ind), np.array(pts, F)], 0)
                touched.add(ind)
            for ind in lst:
                if len(self.cube(kind, ind)):
                    self.cubes[kind][ind] = voxel_grid(self.cube(kind, ind), self.leaf[kind])
                    touched.add(ind)
        res.update(q_w_curr=list(q), t_w_curr=list(t), q_wmap_wodom=list(self.q_wmap),
                   t_wmap_wodom=list(self.t_wmap), touched=sorted(touched))
        return res
