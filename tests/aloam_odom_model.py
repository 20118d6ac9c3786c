"""numpy / plain-Python restatement of A-LOAM's laserOdometry as the library
states it (include/slio_frontend.h, "A-LOAM laserOdometry"): the reference's
serial neighbour loops (src/A-LOAM/src/laserOdometry.cpp:341-573), the two
factors of lidarFactor.hpp with analytic Jacobians, HuberLoss(0.1), the sums in
the stated order (32 strided partials per entry in ascending slot, then
ascending lane) and the library's Levenberg-Marquardt, integration and gate.
It shares no code with the library.  Doubles are Python floats (IEEE, never
fused), the distances are numpy float32, so the library can be compared to it
to the bit.  Quaternions are (x, y, z, w).
"""
import math

import numpy as np

F = np.float32
LANES, SUMS, MAX_ITER = 32, 28, 4
STOPS = ("max_iter", "gradient", "function", "parameter")
IDENT_Q, ZERO_T = (0.0, 0.0, 0.0, 1.0), (0.0, 0.0, 0.0)


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def rotate(q, v):
    """Eigen's _transformVector."""
    uv = cross(q, v)
    uv = [u + u for u in uv]
    c = cross(q, uv)
    return [(v[a] + q[3] * uv[a]) + c[a] for a in range(3)]


def qmul(a, b):
    return [a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
            a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
            a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
            a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]]


def to_start(q, t, p):
    """TransformToStart at s = 1 on one point (x, y, z, ..): float32[3]."""
    r = rotate(q, [float(p[0]), float(p[1]), float(p[2])])
    return np.array([r[0] + t[0], r[1] + t[1], r[2] + t[2]], np.float64).astype(F)


def dist2_all(last, sel):
    """float32 ((dx dx + dy dy) + dz dz) of every last point to sel."""
    d = last[:, :3] - sel[None, :]
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F)


def ids_ok(cloud):
    it = cloud[:, 3]
    if not np.all((it >= 0) & (it < 64)):
        return False
    return bool(np.all(np.diff(it.astype(np.int64)) >= 0))


def _assoc_one(sel, last, ids, surf):
    n = len(last)
    if n == 0:
        return -1, -1, -1
    with np.errstate(invalid="ignore", over="ignore"):
        d = dist2_all(last, sel)
    # exact 1-NN, ties to the lower index; a NaN distance is never nearest
    closest, bd = -1, math.inf
    dl = d.tolist()
    if not np.isnan(d).any():
        closest = int(np.argmin(d))
        bd = dl[closest]
        if not bd < math.inf:
            closest = -1
    else:
        for j in range(n):
            if dl[j] < bd:
                bd, closest = dl[j], j
    if closest < 0 or not bd < 25.0:
        return -1, -1, -1
    cs = ids[closest]
    ind2, ind3, min2, min3 = -1, -1, 25.0, 25.0
    if not surf:
        for j in range(closest + 1, n):
            if ids[j] <= cs:
                continue
            if ids[j] > cs + 2.5:
                break
            if dl[j] < min2:
                min2, ind2 = dl[j], j
        for j in range(closest - 1, -1, -1):
            if ids[j] >= cs:
                continue
            if ids[j] < cs - 2.5:
                break
            if dl[j] < min2:
                min2, ind2 = dl[j], j
        return closest, ind2, -1
    for j in range(closest + 1, n):
        if ids[j] > cs + 2.5:
            break
        if ids[j] <= cs and dl[j] < min2:
            min2, ind2 = dl[j], j
        elif ids[j] > cs and dl[j] < min3:
            min3, ind3 = dl[j], j
    for j in range(closest - 1, -1, -1):
        if ids[j] < cs - 2.5:
            break
        if ids[j] >= cs and dl[j] < min2:
            min2, ind2 = dl[j], j
        elif ids[j] < cs and dl[j] < min3:
            min3, ind3 = dl[j], j
    return closest, ind2, ind3


def associate(sharp, flat, corner_last, surf_last, q, t):
    """(n_sharp + n_flat, 3) int32: closest, second, third; -1: none."""
    assert ids_ok(corner_last) and ids_ok(surf_last)
    q, t = [float(v) for v in q], [float(v) for v in t]
    out = []
    for pts, last, surf in ((sharp, corner_last, False), (flat, surf_last, True)):
        ids = last[:, 3].astype(np.int64).tolist()
        for p in pts:
            out.append(_assoc_one(to_start(q, t, p), last, ids, surf))
    return np.array(out, np.int32).reshape(-1, 3)


def edge_factor(q, t, cp, a, b):
    """(residuals, Jacobian rows) or None where a == b."""
    rc = rotate(q, cp)
    lp = [rc[k] + t[k] for k in range(3)]
    d1 = [lp[k] - a[k] for k in range(3)]
    d2 = [lp[k] - b[k] for k in range(3)]
    de = [a[k] - b[k] for k in range(3)]
    n = math.sqrt((de[0] * de[0] + de[1] * de[1]) + de[2] * de[2])
    if n == 0.0:
        return None
    nu = cross(d1, d2)
    m = [(b[k] - a[k]) / n for k in range(3)]
    E = [[0.0, -m[2], m[1]], [m[2], 0.0, -m[0]], [-m[1], m[0], 0.0]]
    return [nu[i] / n for i in range(3)], [cross(rc, E[i]) + E[i] for i in range(3)]


def plane_factor(q, t, cp, j, l, m):
    jl = [j[k] - l[k] for k in range(3)]
    jm = [j[k] - m[k] for k in range(3)]
    nr = cross(jl, jm)
    ln = math.sqrt((nr[0] * nr[0] + nr[1] * nr[1]) + nr[2] * nr[2])
    if ln == 0.0:                       # (x / 0 is NaN or infinite: not a finite normal)
        return None
    n = [v / ln for v in nr]
    if not all(math.isfinite(v) for v in n):
        return None
    rc = rotate(q, cp)
    d = [(rc[k] + t[k]) - j[k] for k in range(3)]
    return [(d[0] * n[0] + d[1] * n[1]) + d[2] * n[2]], [cross(rc, n) + n]


def contributions(r, J):
    """28 contributions of one factor and whether it is a Huber outlier."""
    three = len(r) == 3
    s = r[0] * r[0]
    if three:
        s = (s + r[1] * r[1]) + r[2] * r[2]
    rho, w, out = s, 1.0, s > 0.01
    if out:
        sq = math.sqrt(s)
        rho, w = 0.2 * sq - 0.01, 0.1 / sq
    c = []
    for a in range(6):
        for b in range(a, 6):
            h = J[0][a] * J[0][b]
            if three:
                h = (h + J[1][a] * J[1][b]) + J[2][a] * J[2][b]
            c.append(w * h)
    for a in range(6):
        h = J[0][a] * r[0]
        if three:
            h = (h + J[1][a] * r[1]) + J[2][a] * r[2]
        c.append(w * h)
    c.append(rho)
    return c, out


def _xyz(cloud, i):
    return [float(cloud[i, 0]), float(cloud[i, 1]), float(cloud[i, 2])]


def slot_factor(s, sharp, flat, corner_last, surf_last, corr, q, t):
    """(matched, factor or None)."""
    i0, i1, i2 = (int(v) for v in corr[s])
    if s < len(sharp):
        if i1 < 0:
            return False, None
        return True, edge_factor(q, t, _xyz(sharp, s), _xyz(corner_last, i0), _xyz(corner_last, i1))
    if i1 < 0 or i2 < 0:
        return False, None
    return True, plane_factor(q, t, _xyz(flat, s - len(sharp)), _xyz(surf_last, i0), _xyz(surf_last, i1),
                              _xyz(surf_last, i2))


def evaluate(sharp, flat, corner_last, surf_last, corr, q, t):
    """A (21), g (6), cost, counts {corner, plane, degenerate, outliers}."""
    q, t = [float(v) for v in q], [float(v) for v in t]
    part = [[0.0] * SUMS for _ in range(LANES)]
    counts = [0, 0, 0, 0]
    for s in range(len(sharp) + len(flat)):
        matched, f = slot_factor(s, sharp, flat, corner_last, surf_last, corr, q, t)
        if matched:
            counts[0 if s < len(sharp) else 1] += 1
        if matched and f is None:
            counts[2] += 1
        if f is None:
            continue
        c, out = contributions(*f)
        counts[3] += int(out)
        p = part[s % LANES]
        for k in range(SUMS):
            p[k] = p[k] + c[k]
    sums = []
    for k in range(SUMS):
        tot = 0.0
        for l in range(LANES):
            tot = tot + part[l][k]
        sums.append(tot)
    return sums[:21], sums[21:27], 0.5 * sums[27], counts


def tri(a, b):
    lo, hi = min(a, b), max(a, b)
    return lo * 6 - lo * (lo - 1) // 2 + (hi - lo)


def ldlt_solve(A, g, mu):
    """delta of (A + D^2 / mu) delta = -g, and whether every pivot was positive."""
    M = [[A[tri(i, j)] for j in range(6)] for i in range(6)]
    for i in range(6):
        D2 = M[i][i]
        if not D2 >= 1e-6:
            D2 = 1e-6
        if D2 > 1e32:
            D2 = 1e32
        M[i][i] = M[i][i] + D2 / mu
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        v = M[j][j]
        for k in range(j):
            v = v - (L[j][k] * L[j][k]) * d[k]
        if not v > 0.0:
            return [0.0] * 6, False
        d[j] = v
        for i in range(j + 1, 6):
            s = M[i][j]
            for k in range(j):
                s = s - (L[i][k] * L[j][k]) * d[k]
            L[i][j] = s / v
    y = [0.0] * 6
    for i in range(6):
        s = -g[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = s
    x = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i] / d[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * x[k]
        x[i] = s
    return x, True


def retract(q, t, delta):
    dq = [delta[0] / 2.0, delta[1] / 2.0, delta[2] / 2.0, 1.0]
    n = math.sqrt(((dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2]) + dq[3] * dq[3])
    dq = [v / n for v in dq]
    return qmul(dq, q), [t[k] + delta[3 + k] for k in range(3)]


class Lm:
    """The controller of one solve."""

    def __init__(self, q, t, A, g, cost):
        self.mu, self.nu = 1e4, 2.0
        self.q, self.t = [float(v) for v in q], [float(v) for v in t]
        self.A, self.g, self.cost = list(A), list(g), cost
        self.delta, self.model, self.xnorm = [0.0] * 6, 0.0, 0.0
        self.qn, self.tn = list(self.q), list(self.t)
        self.pivots_ok = self.iterations = self.accepted = self.done = self.last_accepted = 0
        self.stop = 0

    def propose(self):
        if self.done:
            return False
        if self.iterations >= MAX_ITER:
            self.done, self.stop = 1, 0
            return False
        if max(abs(v) for v in self.g) <= 1e-10:
            self.done, self.stop = 1, 1
            return False
        self.delta, ok = ldlt_solve(self.A, self.g, self.mu)
        self.pivots_ok = int(ok)
        gd, dAd = 0.0, 0.0
        for i in range(6):
            gd = gd + self.g[i] * self.delta[i]
            Ad = 0.0
            for j in range(6):
                Ad = Ad + self.A[tri(i, j)] * self.delta[j]
            dAd = dAd + self.delta[i] * Ad
        self.model = -gd - 0.5 * dAd
        xn = 0.0
        for v in self.q + self.t:
            xn = xn + v * v
        self.xnorm = math.sqrt(xn)
        self.qn, self.tn = retract(self.q, self.t, self.delta)
        return True

    def decide(self, An, gn, costn):
        self.iterations += 1
        with np.errstate(all="ignore"):
            rho = float(np.float64(self.cost - costn) / np.float64(self.model))
        accept = bool(self.pivots_ok) and self.model > 0.0 and rho > 1e-3
        self.last_accepted = int(accept)
        if accept:
            tmp = 2.0 * rho - 1.0
            f = 1.0 - (tmp * tmp) * tmp
            if not f >= 1.0 / 3.0:
                f = 1.0 / 3.0
            self.mu = min(self.mu / f, 1e16)
            self.nu = 2.0
            old = self.cost
            self.q, self.t, self.A, self.g, self.cost = list(self.qn), list(self.tn), list(An), list(gn), costn
            self.accepted += 1
            if abs(old - costn) <= 1e-6 * old:
                self.done, self.stop = 1, 2
                return
        else:
            self.mu = self.mu / self.nu
            self.nu = 2.0 * self.nu
        dn = 0.0
        for v in self.delta:
            dn = dn + v * v
        if math.sqrt(dn) <= 1e-8 * (self.xnorm + 1e-8):
            self.done, self.stop = 1, 3
            return
        if self.iterations >= MAX_ITER:
            self.done, self.stop = 1, 0


def one_pass(sharp, flat, corner_last, surf_last, q, t):
    """One opti pass (:317): the association at (q, t), then the solve.
    Returns (q, t, info)."""
    corr = associate(sharp, flat, corner_last, surf_last, q, t)
    A, g, cost, cnt = evaluate(sharp, flat, corner_last, surf_last, corr, q, t)
    s = Lm(q, t, A, g, cost)
    info = dict(corner=cnt[0], plane=cnt[1], degenerate=cnt[2], outliers=cnt[3], few=int(cnt[0] + cnt[1] < 10),
                cost_first=cost, corr=corr, iterates=[])
    while s.propose():
        An, gn, costn, cn = evaluate(sharp, flat, corner_last, surf_last, corr, s.qn, s.tn)
        s.decide(An, gn, costn)
        if s.last_accepted:
            info["outliers"] = cn[3]
        info["iterates"].append(dict(q=list(s.q), t=list(s.t), cost=s.cost, mu=s.mu, accepted=s.last_accepted))
    info.update(iterations=s.iterations, accepted=s.accepted, stop=s.stop, cost_last=s.cost)
    return s.q, s.t, info


def integrate(q_w, t_w, q_lc, t_lc):
    r = rotate(q_w, t_lc)
    return qmul(q_w, q_lc), [t_w[k] + r[k] for k in range(3)]


class Odometry:
    """The node's state and loop body (:304-695)."""

    def __init__(self, skip_frame_num=2):
        self.skip = skip_frame_num
        self.reset()

    def reset(self):
        self.q_w, self.t_w = list(IDENT_Q), list(ZERO_T)
        self.para_q, self.para_t = list(IDENT_Q), list(ZERO_T)
        self.inited, self.frame_count = False, 0
        self.corner_last = self.surf_last = np.zeros((0, 4), F)

    def process(self, sharp, less_sharp, flat, less_flat):
        sharp, less_sharp, flat, less_flat = (np.ascontiguousarray(a, F).reshape(-1, 4)
                                              for a in (sharp, less_sharp, flat, less_flat))
        assert ids_ok(less_sharp) and ids_ok(less_flat)
        res = dict(inited=int(self.inited), passes=[])
        if not self.inited:
            self.inited = True
        else:
            for _ in range(2):
                self.para_q, self.para_t, info = one_pass(sharp, flat, self.corner_last, self.surf_last, self.para_q,
                                                          self.para_t)
                res["passes"].append(info)
            self.q_w, self.t_w = integrate(self.q_w, self.t_w, self.para_q, self.para_t)
        self.corner_last, self.surf_last = less_sharp.copy(), less_flat.copy()
        res["published"] = int(self.frame_count % self.skip == 0)
        if res["published"]:
            self.frame_count = 0
        self.frame_count += 1
        res.update(frame_count=self.frame_count, q_w_curr=list(self.q_w), t_w_curr=list(self.t_w),
                   q_last_curr=list(self.para_q), t_last_curr=list(self.para_t))
        return res
