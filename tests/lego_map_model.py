"""numpy float32 restatement of LeGO-LOAM's mapping back-end
(LeGO-LOAM/src/mapOptmization.cpp with loopClosureEnableFlag = false,
transformFusion.cpp), in the manner of tests/lego_odom_model.py:
pointAssociateToMap / transformPointCloud (:578-652), cornerOptimization
(:1222-1370), surfOptimization (:1372-1450) with cv::solve(DECOMP_QR) on the
5 x 3 system, LMOptimization (:1456-1601), scan2MapOptimization's loop
(:1603-1626), transformAssociateToMap (:394-519), transformUpdate (:521-560),
transformFusion's handlers and the keyframe decision (:1629-1645).

The yardstick of tests/test_lego_map_cpu.py and tests/test_gpu_lego_map.py;
it shares no code with the library.  Every float operation is one np.float32
operation in the reference's order, with the promotions the reference makes
(0.1 * v, 1 - 0.9 * fabs(d), > 0.2, 0.998 * a + 0.002 * b in double); sin /
cos / asin / atan2 / sqrt of a float are the double functions rounded to
float.  Neighbours come from the caller (oracle.Tree(...).knn), VoxelGrids
from oracle.voxel_grid.  A^T A / A^T B: fp64 products summed in the library's
stated tree -- per block of 256 points a butterfly over each 64-point group,
the four groups in order, blocks in order, corners before surfs -- and
rounded to float.
"""
import math

import numpy as np

from lego_odom_model import F, FLT_EPS, cv_hypot, fasin, fatan2, fcos, fsin, fsqrt

D = np.float64


# ------------------------------------------------------------------ transforms
def to_map(tf, pts):
    """pointAssociateToMap (:578-607) == transformPointCloud (:624-652)."""
    tf = np.asarray(tf, F)
    p = np.ascontiguousarray(pts, F).reshape(-1, 3)
    cr, sr, cp, sp, cy, sy = fcos(tf[0]), fsin(tf[0]), fcos(tf[1]), fsin(tf[1]), fcos(tf[2]), fsin(tf[2])
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    x1 = cy * x - sy * y
    y1 = sy * x + cy * y
    z1 = z
    x2 = x1
    y2 = cr * y1 - sr * z1
    z2 = sr * y1 + cr * z1
    ox = cp * x2 + sp * z2 + tf[3]
    oy = y2 + tf[4]
    oz = -sp * x2 + cp * z2 + tf[5]
    return np.stack([ox, oy, oz], 1).astype(F)


# ------------------------------------------------------------------ OpenCV's solvers, float32
def qr_solve(A_in, b_in, M, N):
    """cv::solve(DECOMP_QR) on an M x N system (row-major), None where
    hal::QR32f gives up (a diagonal of R below 10 * FLT_EPSILON)."""
    A = [F(v) for v in A_in]
    b = [F(v) for v in b_in]
    x = [F(0)] * N
    for k in range(N):
        nrm = F(0)
        for i in range(k, M):
            nrm = nrm + A[N * i + k] * A[N * i + k]
        nrm = fsqrt(nrm)
        if nrm == 0:
            return None
        alpha = -nrm if A[N * k + k] > 0 else nrm
        v = [F(0)] * M
        for i in range(k, M):
            v[i] = A[N * i + k]
        v[k] = v[k] - alpha
        vv = F(0)
        for i in range(k, M):
            vv = vv + v[i] * v[i]
        if vv == 0:
            continue
        for j in range(k, N):
            d = F(0)
            for i in range(k, M):
                d = d + v[i] * A[N * i + j]
            f = F(2) * d / vv
            for i in range(k, M):
                A[N * i + j] = A[N * i + j] - f * v[i]
        d = F(0)
        for i in range(k, M):
            d = d + v[i] * b[i]
        f = F(2) * d / vv
        for i in range(k, M):
            b[i] = b[i] - f * v[i]
    for i in range(N - 1, -1, -1):
        s = b[i]
        for j in range(i + 1, N):
            s = s - A[N * i + j] * x[j]
        if abs(A[N * i + i]) < F(10) * FLT_EPS:
            return None
        x[i] = s / A[N * i + i]
    return x


def jacobi(A_in, n):
    """hal::Jacobi on n x n: eigenvalues descending, eigenvectors the rows of V."""
    A = [F(v) for v in A_in]
    V = [F(1) if i // n == i % n else F(0) for i in range(n * n)]
    W = [F(0)] * n
    indR, indC = [0] * n, [0] * n

    def row_max(k):
        m = k + 1
        mv = abs(A[n * k + m])
        for i in range(k + 2, n):
            val = abs(A[n * k + i])
            if mv < val:
                mv, m = val, i
        return m

    def col_max(k):
        m = 0
        mv = abs(A[k])
        for i in range(1, k):
            val = abs(A[n * i + k])
            if mv < val:
                mv, m = val, i
        return m

    for k in range(n):
        W[k] = A[(n + 1) * k]
        if k < n - 1:
            indR[k] = row_max(k)
        if k > 0:
            indC[k] = col_max(k)
    for _ in range(n * n * 30):
        k = 0
        mv = abs(A[indR[0]])
        for i in range(1, n - 1):
            val = abs(A[n * i + indR[i]])
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[n * indC[i] + i])
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[n * k + l]
        if abs(p) <= FLT_EPS:
            break
        y = F(D(W[l] - W[k]) * 0.5)
        t = abs(y) + cv_hypot(p, y)
        s = cv_hypot(p, t)
        c = t / s
        s = p / s
        t = (p / t) * p
        if y < 0:
            s, t = -s, -t
        A[n * k + l] = F(0)
        W[k] = W[k] - t
        W[l] = W[l] + t

        def rot(Mx, i0, i1):
            a0, b0 = Mx[i0], Mx[i1]
            Mx[i0] = a0 * c - b0 * s
            Mx[i1] = a0 * s + b0 * c

        for i in range(k):
            rot(A, n * i + k, n * i + l)
        for i in range(k + 1, l):
            rot(A, n * k + i, n * i + l)
        for i in range(l + 1, n):
            rot(A, n * k + i, n * l + i)
        for i in range(n):
            rot(V, n * k + i, n * l + i)
        for idx in (k, l):
            if idx < n - 1:
                indR[idx] = row_max(idx)
            if idx > 0:
                indC[idx] = col_max(idx)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            for i in range(n):
                V[n * m + i], V[n * k + i] = V[n * k + i], V[n * m + i]
    return W, V


def inv_lu(Min, n):
    """cv::Mat::inv (DECOMP_LU, n > 3): LU with partial pivoting, float."""
    a = [F(v) for v in Min]
    b = [F(1) if i % (n + 1) == 0 else F(0) for i in range(n * n)]
    for k in range(n):
        p = k
        for i in range(k + 1, n):
            if abs(a[n * i + k]) > abs(a[n * p + k]):
                p = i
        if a[n * p + k] == 0:
            return None
        if p != k:
            for j in range(n):
                a[n * p + j], a[n * k + j] = a[n * k + j], a[n * p + j]
                b[n * p + j], b[n * k + j] = b[n * k + j], b[n * p + j]
        for i in range(k + 1, n):
            f = a[n * i + k] / a[n * k + k]
            for j in range(k, n):
                a[n * i + j] = a[n * i + j] - f * a[n * k + j]
            for j in range(n):
                b[n * i + j] = b[n * i + j] - f * b[n * k + j]
    out = [F(0)] * (n * n)
    for c in range(n):
        for i in range(n - 1, -1, -1):
            s = b[n * i + c]
            for j in range(i + 1, n):
                s = s - a[n * i + j] * out[n * j + c]
            out[n * i + c] = s / a[n * i + i]
    return out


# ------------------------------------------------------------------ coefficients
def corner_coeff(nb, p):
    """:1237-1365 on the five neighbours nb (5, 3) and the map-frame point p.
    Returns (coeff[4], selected, line) -- line False: the eigenvalue test failed."""
    cx = cy = cz = F(0)
    for j in range(5):
        cx, cy, cz = cx + nb[j][0], cy + nb[j][1], cz + nb[j][2]
    cx, cy, cz = cx / F(5), cy / F(5), cz / F(5)
    a11 = a12 = a13 = a22 = a23 = a33 = F(0)
    for j in range(5):
        ax, ay, az = nb[j][0] - cx, nb[j][1] - cy, nb[j][2] - cz
        a11, a12, a13 = a11 + ax * ax, a12 + ax * ay, a13 + ax * az
        a22, a23, a33 = a22 + ay * ay, a23 + ay * az, a33 + az * az
    a11, a12, a13, a22, a23, a33 = (v / F(5) for v in (a11, a12, a13, a22, a23, a33))
    W, V = jacobi([a11, a12, a13, a12, a22, a23, a13, a23, a33], 3)
    if not (W[0] > F(3) * W[1]):
        return np.zeros(4, F), 0, False
    x0, y0, z0 = p
    x1, y1, z1 = F(D(cx) + 0.1 * D(V[0])), F(D(cy) + 0.1 * D(V[1])), F(D(cz) + 0.1 * D(V[2]))
    x2, y2, z2 = F(D(cx) - 0.1 * D(V[0])), F(D(cy) - 0.1 * D(V[1])), F(D(cz) - 0.1 * D(V[2]))
    u = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)
    v = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)
    w = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)
    with np.errstate(all="ignore"):
        a012 = fsqrt(u * u + v * v + w * w)
        l12 = fsqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2))
        la = ((y1 - y2) * u + (z1 - z2) * v) / a012 / l12
        lb = -((x1 - x2) * u - (z1 - z2) * w) / a012 / l12
        lc = -((x1 - x2) * v + (y1 - y2) * w) / a012 / l12
        ld2 = a012 / l12
        s = F(1.0 - 0.9 * D(abs(ld2)))
        cf = np.array([s * la, s * lb, s * lc, s * ld2], F)
    return cf, int(D(s) > 0.1), True


def surf_coeff(nb, p):
    """:1381-1447.  Returns (coeff[4], selected, plane) -- plane False: the 0.2 check failed."""
    A = [nb[j][c] for j in range(5) for c in range(3)]
    X = qr_solve(A, [F(-1)] * 5, 5, 3)
    if X is None:
        X = [F(0)] * 3        # cv::solve leaves matX zero
    pa, pb, pc, pd = X[0], X[1], X[2], F(1)
    with np.errstate(all="ignore"):
        ps = fsqrt(pa * pa + pb * pb + pc * pc)
        pa, pb, pc, pd = pa / ps, pb / ps, pc / ps, pd / ps
        for j in range(5):
            if D(abs(pa * nb[j][0] + pb * nb[j][1] + pc * nb[j][2] + pd)) > 0.2:
                return np.zeros(4, F), 0, False
        x0, y0, z0 = p
        pd2 = pa * x0 + pb * y0 + pc * z0 + pd
        s = F(1.0 - 0.9 * D(abs(pd2)) / D(fsqrt(fsqrt(x0 * x0 + y0 * y0 + z0 * z0))))
        cf = np.array([s * pa, s * pb, s * pc, s * pd2], F)
    return cf, int(D(s) > 0.1), True


def coeffs(kind, world, map_xyz, idx, sqd):
    """Per point (coeff, sel) and the counts {selected, gated by 1 m, rejected
    by the eigenvalue ratio / the plane check}."""
    world = np.ascontiguousarray(world, F).reshape(-1, 3)
    n = world.shape[0]
    coeff, sel = np.zeros((n, 4), F), np.zeros(n, np.uint8)
    stats = dict(selected=0, gated=0, rejected=0)
    for i in range(n):
        if not (idx.shape[1] >= 5 and sqd[i, 4] < F(1.0)):
            stats["gated"] += 1
            continue
        nb = [[F(v) for v in map_xyz[idx[i, j]]] for j in range(5)]
        p = [F(v) for v in world[i]]
        cf, ok, shape_ok = (corner_coeff if kind == 0 else surf_coeff)(nb, p)
        coeff[i], sel[i] = cf, ok
        stats["selected"] += ok
        stats["rejected"] += 0 if shape_ok else 1
    return coeff, sel, stats


# ------------------------------------------------------------------ LMOptimization
def rows(tf, body, coeff):
    """:1477-1537: (n, 6) A and (n,) B, vectorised (elementwise float32)."""
    tf = np.asarray(tf, F)
    srx, crx, sry, cry, srz, crz = fsin(tf[0]), fcos(tf[0]), fsin(tf[1]), fcos(tf[1]), fsin(tf[2]), fcos(tf[2])
    b = np.ascontiguousarray(body, F).reshape(-1, 3)
    px, py, pz = b[:, 0], b[:, 1], b[:, 2]
    cx, cy, cz = coeff[:, 0], coeff[:, 1], coeff[:, 2]
    arx = (crx * sry * srz * px + crx * crz * sry * py - srx * sry * pz) * cx + \
          (-srx * srz * px - crz * srx * py - crx * pz) * cy + \
          (crx * cry * srz * px + crx * cry * crz * py - cry * srx * pz) * cz
    ary = ((cry * srx * srz - crz * sry) * px + (sry * srz + cry * crz * srx) * py + crx * cry * pz) * cx + \
          ((-cry * crz - srx * sry * srz) * px + (cry * srz - crz * srx * sry) * py - crx * sry * pz) * cz
    arz = ((crz * srx * sry - cry * srz) * px + (-cry * crz - srx * sry * srz) * py) * cx + \
          (crx * crz * px - crx * srz * py) * cy + \
          ((sry * srz + cry * crz * srx) * px + (crz * sry - cry * srx * srz) * py) * cz
    return np.stack([arx, ary, arz, cx, cy, cz], 1).astype(F), (-coeff[:, 3]).astype(F)


def tree_sum(terms):
    """(n, k) fp64 terms -> the list of per-block partials (k,): a butterfly
    over each group of 64, the four groups of a block of 256 in order."""
    n, k = terms.shape
    nb = (n + 255) // 256
    pad = np.zeros((nb * 256, k), D)
    pad[:n] = terms
    lane = np.arange(64)
    out = []
    for b in range(nb):
        w = []
        for g in range(4):
            v = pad[b * 256 + g * 64:b * 256 + g * 64 + 64].copy()
            for off in (32, 16, 8, 4, 2, 1):
                v = v + v[lane ^ off]
            w.append(v[0])
        out.append(((w[0] + w[1]) + w[2]) + w[3])
    return out


def normal_equations(tf, clouds):
    """clouds: [(body, coeff, sel)] corners first.  (AtA[36], AtB[6], nsel)."""
    acc = np.zeros(28, D)
    for body, coeff, sel in clouds:
        n = np.asarray(body).reshape(-1, 3).shape[0]
        if n == 0:
            continue
        A, B = rows(tf, body, coeff)
        t = np.zeros((n, 28), D)
        q = 0
        for r in range(6):
            for c in range(r, 6):
                t[:, q] = A[:, r].astype(D) * A[:, c].astype(D)
                q += 1
        for r in range(6):
            t[:, 21 + r] = A[:, r].astype(D) * B.astype(D)
        t[:, 27] = 1.0
        t[~np.asarray(sel, bool)] = 0.0
        for part in tree_sum(t):
            acc = acc + part
    AtA = np.zeros(36, F)
    q = 0
    for r in range(6):
        for c in range(r, 6):
            AtA[6 * r + c] = AtA[6 * c + r] = F(acc[q])
            q += 1
    return AtA, acc[21:27].astype(F), int(round(acc[27]))


def lm_step(AtA, AtB, nsel, it, tf, state):
    """:1464-1600 after the normal equations; tf (float32[6]) updated in place,
    state = dict(is_degenerate, matP).  Returns LMOptimization's bool."""
    if nsel < 50:
        return False
    X = qr_solve(AtA, AtB, 6, 6)
    if X is None:
        X = [F(0)] * 6
    if it == 0:
        E, V = jacobi(AtA, 6)
        V2 = list(V)
        state["is_degenerate"] = 0
        for i in range(5, -1, -1):
            if E[i] < F(100):
                for j in range(6):
                    V2[6 * i + j] = F(0)
                state["is_degenerate"] = 1
            else:
                break
        Vi = inv_lu(V, 6)
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
    r2d = F(180.0 / math.pi)
    dR = F(math.sqrt(sum(D(X[k] * r2d) ** 2 for k in range(3))))
    dT = F(math.sqrt(sum(D(X[k] * F(100)) ** 2 for k in range(3, 6))))
    return bool(D(dR) < 0.05 and D(dT) < 0.05)


def scan2map(tf0, corner_scan, surf_scan, corner_map, surf_map, knn, max_iter=10):
    """:1603-1621: (tf, iterations, is_degenerate, trace).  knn(map, queries)
    -> (idx, sqd) with five neighbours per query."""
    tf = np.array(tf0, F)
    state = dict(is_degenerate=0, matP=[F(0)] * 36)
    trace, iters = [], 0
    if not (corner_map.shape[0] > 10 and surf_map.shape[0] > 100):
        return tf, 0, 0, trace
    for it in range(max_iter):
        clouds = []
        for kind, scan, mp in ((0, corner_scan, corner_map), (1, surf_scan, surf_map)):
            w = to_map(tf, scan)
            idx, sqd = knn(mp, w)
            cf, sel, _ = coeffs(kind, w, mp, idx, sqd)
            clouds.append((scan, cf, sel))
        AtA, AtB, nsel = normal_equations(tf, clouds)
        done = lm_step(AtA, AtB, nsel, it, tf, state)
        iters = it + 1
        trace.append(tf.copy())
        if done:
            break
    return tf, iters, state["is_degenerate"], trace


# ------------------------------------------------------------------ host formulas
def associate_to_map(ts, tb, ta):
    """transformAssociateToMap (:394-519; transformFusion.cpp :91-215)."""
    ts, tb, ta = (np.asarray(v, F) for v in (ts, tb, ta))
    tm = np.zeros(6, F)
    x1 = fcos(ts[1]) * (tb[3] - ts[3]) - fsin(ts[1]) * (tb[5] - ts[5])
    y1 = tb[4] - ts[4]
    z1 = fsin(ts[1]) * (tb[3] - ts[3]) + fcos(ts[1]) * (tb[5] - ts[5])
    x2 = x1
    y2 = fcos(ts[0]) * y1 + fsin(ts[0]) * z1
    z2 = -fsin(ts[0]) * y1 + fcos(ts[0]) * z1
    ti3 = fcos(ts[2]) * x2 + fsin(ts[2]) * y2
    ti4 = -fsin(ts[2]) * x2 + fcos(ts[2]) * y2
    ti5 = z2
    sbcx, cbcx, sbcy, cbcy, sbcz, cbcz = fsin(ts[0]), fcos(ts[0]), fsin(ts[1]), fcos(ts[1]), fsin(ts[2]), fcos(ts[2])
    sblx, cblx, sbly, cbly, sblz, cblz = fsin(tb[0]), fcos(tb[0]), fsin(tb[1]), fcos(tb[1]), fsin(tb[2]), fcos(tb[2])
    salx, calx, saly, caly, salz, calz = fsin(ta[0]), fcos(ta[0]), fsin(ta[1]), fcos(ta[1]), fsin(ta[2]), fcos(ta[2])
    srx = -sbcx * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz) - \
        cbcx * sbcy * (calx * calz * (cbly * sblz - cblz * sblx * sbly) -
                       calx * salz * (cbly * cblz + sblx * sbly * sblz) + cblx * salx * sbly) - \
        cbcx * cbcy * (calx * salz * (cblz * sbly - cbly * sblx * sblz) -
                       calx * calz * (sbly * sblz + cbly * cblz * sblx) + cblx * cbly * salx)
    tm[0] = -fasin(srx)
    srycrx = sbcx * (cblx * cblz * (caly * salz - calz * salx * saly) -
                     cblx * sblz * (caly * calz + salx * saly * salz) + calx * saly * sblx) - \
        cbcx * cbcy * ((caly * calz + salx * saly * salz) * (cblz * sbly - cbly * sblx * sblz) +
                       (caly * salz - calz * salx * saly) * (sbly * sblz + cbly * cblz * sblx) -
                       calx * cblx * cbly * saly) + \
        cbcx * sbcy * ((caly * calz + salx * saly * salz) * (cbly * cblz + sblx * sbly * sblz) +
                       (caly * salz - calz * salx * saly) * (cbly * sblz - cblz * sblx * sbly) +
                       calx * cblx * saly * sbly)
    crycrx = sbcx * (cblx * sblz * (calz * saly - caly * salx * salz) -
                     cblx * cblz * (saly * salz + caly * calz * salx) + calx * caly * sblx) + \
        cbcx * cbcy * ((saly * salz + caly * calz * salx) * (sbly * sblz + cbly * cblz * sblx) +
                       (calz * saly - caly * salx * salz) * (cblz * sbly - cbly * sblx * sblz) +
                       calx * caly * cblx * cbly) - \
        cbcx * sbcy * ((saly * salz + caly * calz * salx) * (cbly * sblz - cblz * sblx * sbly) +
                       (calz * saly - caly * salx * salz) * (cbly * cblz + sblx * sbly * sblz) -
                       calx * caly * cblx * sbly)
    tm[1] = fatan2(srycrx / fcos(tm[0]), crycrx / fcos(tm[0]))
    srzcrx = (cbcz * sbcy - cbcy * sbcx * sbcz) * (calx * salz * (cblz * sbly - cbly * sblx * sblz) -
                                                   calx * calz * (sbly * sblz + cbly * cblz * sblx) +
                                                   cblx * cbly * salx) - \
        (cbcy * cbcz + sbcx * sbcy * sbcz) * (calx * calz * (cbly * sblz - cblz * sblx * sbly) -
                                              calx * salz * (cbly * cblz + sblx * sbly * sblz) +
                                              cblx * salx * sbly) + \
        cbcx * sbcz * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz)
    crzcrx = (cbcy * sbcz - cbcz * sbcx * sbcy) * (calx * calz * (cbly * sblz - cblz * sblx * sbly) -
                                                   calx * salz * (cbly * cblz + sblx * sbly * sblz) +
                                                   cblx * salx * sbly) - \
        (sbcy * sbcz + cbcy * cbcz * sbcx) * (calx * salz * (cblz * sbly - cbly * sblx * sblz) -
                                              calx * calz * (sbly * sblz + cbly * cblz * sblx) +
                                              cblx * cbly * salx) + \
        cbcx * cbcz * (salx * sblx + calx * cblx * salz * sblz + calx * calz * cblx * cblz)
    tm[2] = fatan2(srzcrx / fcos(tm[0]), crzcrx / fcos(tm[0]))
    x1 = fcos(tm[2]) * ti3 - fsin(tm[2]) * ti4
    y1 = fsin(tm[2]) * ti3 + fcos(tm[2]) * ti4
    z1 = ti5
    x2 = x1
    y2 = fcos(tm[0]) * y1 - fsin(tm[0]) * z1
    z2 = fsin(tm[0]) * y1 + fcos(tm[0]) * z1
    tm[3] = ta[3] - (fcos(tm[1]) * x2 + fsin(tm[1]) * z2)
    tm[4] = ta[4] - y2
    tm[5] = ta[5] - (-fsin(tm[1]) * x2 + fcos(tm[1]) * z2)
    return tm


def transform_update(tm, ts, t_odom, scan_period, imu_time, imu_roll, imu_pitch, imu_last, imu_front):
    """transformUpdate (:521-560): returns (tobe, bef, aft, imuPointerFront)."""
    tm = np.array(tm, F)
    n = len(imu_time)
    sp = D(F(scan_period))
    if imu_last >= 0:
        roll = pitch = F(0)
        while imu_front != imu_last:
            if t_odom + sp < imu_time[imu_front]:
                break
            imu_front = (imu_front + 1) % n
        if t_odom + sp > imu_time[imu_front]:
            roll, pitch = F(imu_roll[imu_front]), F(imu_pitch[imu_front])
        else:
            back = (imu_front + n - 1) % n
            rf = F((t_odom + sp - imu_time[back]) / (imu_time[imu_front] - imu_time[back]))
            rb = F((imu_time[imu_front] - t_odom - sp) / (imu_time[imu_front] - imu_time[back]))
            roll = F(imu_roll[imu_front]) * rf + F(imu_roll[back]) * rb
            pitch = F(imu_pitch[imu_front]) * rf + F(imu_pitch[back]) * rb
        tm[0] = F(0.998 * D(tm[0]) + 0.002 * D(pitch))
        tm[2] = F(0.998 * D(tm[2]) + 0.002 * D(roll))
    return tm, np.array(ts, F), tm.copy(), imu_front


def keyframe_decision(prev, cur, nkeys, distance=0.3):
    d = [F(prev[k]) - F(cur[k]) for k in range(3)]
    dist = fsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    return bool(not (D(dist) < distance) or nkeys == 0)


# ------------------------------------------------------------------ the frame convention
def cam_points(p_lidar):
    """(x, y, z)_cam = (y, z, x)_lidar."""
    p = np.ascontiguousarray(p_lidar, F).reshape(-1, 3)
    return np.ascontiguousarray(p[:, [1, 2, 0]])


def cam_pose(tf_lidar):
    """LIO-SAM {roll, pitch, yaw, x, y, z} -> {rx, ry, rz, tx, ty, tz} =
    {pitch, yaw, roll, y, z, x}."""
    t = np.asarray(tf_lidar, F)
    return np.array([t[1], t[2], t[0], t[4], t[5], t[3]], F)


def tie_free(idx6_sqd):
    """No two of a query's six nearest float distances are equal."""
    s = np.asarray(idx6_sqd)
    return bool((np.diff(np.sort(s, axis=1), axis=1) != 0).all())
