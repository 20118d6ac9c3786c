"""numpy float32 restatement of the back half of LeGO-LOAM's
FeatureAssociation::runFeatureAssociation (featureAssociation.cpp):
checkSystemInitialization :1964-1997, updateInitialGuess :1999-2030,
updateTransformation :2036-2065 (findCorresponding{Surf,Corner}Features,
calculateTransformation{Surf,Corner}), integrateTransformation :2068-2104
(AccumulateRotation, PluginIMURotation), publishOdometry :2106-2128 and
publishCloudsLast :2142-2199 (TransformToEnd, adjustOutlierCloud).

The yardstick of tests/test_lego_odom_cpu.py and tests/test_gpu_lego_odom.py.
It shares no code with the library.  Every float operation is one np.float32
operation in the reference's order; the promotions the reference makes are
kept (1 - 1.8 * fabs(ld2), closestScan + 2.5 and -0.05 * d2 in double; every
sin / cos / asin / atan2 / sqrt of a float is the double function rounded to
float).  The neighbour scans are the reference's sequential loops.  Stated
choices, the same as the library's header:
  - 1-NN: exact, ties to the lower index (FLANN's order is unpinned);
  - the forward scan is bounded by the current feature count as the reference
    writes it and, in addition, by the last cloud's size;
  - AtA / AtB: 32 interleaved partial sums per entry -- partial s adds the
    fp64 products of the selected queries q = s, s + 32, ... in ascending q --
    added in ascending s and rounded to float;
  - OpenCV's solvers restated: Householder QR (fails below 10 * FLT_EPSILON on
    R's diagonal -> zero step), hal::Jacobi, the 3 x 3 adjugate inverse in
    double; float matrix products accumulate in double; pow(x, 2) is x * x.
"""
import math

import numpy as np

F = np.float32
SURF, CORNER = 0, 1
FLT_EPS = F(1.1920928955078125e-07)


def fsin(a):
    return F(math.sin(float(a)))


def fcos(a):
    return F(math.cos(float(a)))


def fasin(a):
    a = float(a)
    return F(math.asin(a)) if -1.0 <= a <= 1.0 else F(np.nan)


def fatan2(y, x):
    return F(math.atan2(float(y), float(x)))


def fsqrt(a):
    a = float(a)
    if a != a or a < 0:
        return F(np.nan)
    return F(math.sqrt(a))


def trunc(w):
    return int(float(w))


def transform_to_start(p, tc):
    """:1041-1070; p = (x, y, z, intensity) float32."""
    x, y, z, w = (F(v) for v in p)
    s = F(10) * (w - F(trunc(w)))
    rx, ry, rz = s * tc[0], s * tc[1], s * tc[2]
    tx, ty, tz = s * tc[3], s * tc[4], s * tc[5]
    x1 = fcos(rz) * (x - tx) + fsin(rz) * (y - ty)
    y1 = -fsin(rz) * (x - tx) + fcos(rz) * (y - ty)
    z1 = z - tz
    x2 = x1
    y2 = fcos(rx) * y1 + fsin(rx) * z1
    z2 = -fsin(rx) * y1 + fcos(rx) * z1
    return np.array([fcos(ry) * x2 - fsin(ry) * z2, y2, fsin(ry) * x2 + fcos(ry) * z2, w], F)


def transform_to_end(p, tc, rpy_start, shift, imu_last):
    """:1073-1141; rpy_start = (imuRollStart, imuPitchStart, imuYawStart),
    imu_last = (imuRollLast, imuPitchLast, imuYawLast)."""
    x3, y3, z3, w = transform_to_start(p, tc)
    rx, ry, rz, tx, ty, tz = (F(v) for v in tc)
    x4 = fcos(ry) * x3 + fsin(ry) * z3
    y4 = y3
    z4 = -fsin(ry) * x3 + fcos(ry) * z3
    x5 = x4
    y5 = fcos(rx) * y4 - fsin(rx) * z4
    z5 = fsin(rx) * y4 + fcos(rx) * z4
    x6 = fcos(rz) * x5 - fsin(rz) * y5 + tx
    y6 = fsin(rz) * x5 + fcos(rz) * y5 + ty
    z6 = z5 + tz
    cR, sR = fcos(rpy_start[0]), fsin(rpy_start[0])
    cP, sP = fcos(rpy_start[1]), fsin(rpy_start[1])
    cY, sY = fcos(rpy_start[2]), fsin(rpy_start[2])
    sx, sy, sz = (F(v) for v in shift)
    x7 = cR * (x6 - sx) - sR * (y6 - sy)
    y7 = sR * (x6 - sx) + cR * (y6 - sy)
    z7 = z6 - sz
    x8 = x7
    y8 = cP * y7 - sP * z7
    z8 = sP * y7 + cP * z7
    x9 = cY * x8 + sY * z8
    y9 = y8
    z9 = -sY * x8 + cY * z8
    rl, pl, yl = (F(v) for v in imu_last)
    x10 = fcos(yl) * x9 - fsin(yl) * z9
    y10 = y9
    z10 = fsin(yl) * x9 + fcos(yl) * z9
    x11 = x10
    y11 = fcos(pl) * y10 + fsin(pl) * z10
    z11 = -fsin(pl) * y10 + fcos(pl) * z10
    return np.array([fcos(rl) * x11 + fsin(rl) * y11, -fsin(rl) * x11 + fcos(rl) * y11, z11,
                     F(trunc(w))], F)


def sq_dists(last, p):
    """pointSqDis against every point of `last`, float32, the reference's
    operation order."""
    dx, dy, dz = last[:, 0] - p[0], last[:, 1] - p[1], last[:, 2] - p[2]
    return (dx * dx + dy * dy + dz * dz).astype(F)


def nearest(d, gate):
    """Exact 1-NN under the gate: the lowest index of the minimum, or -1."""
    idx = np.flatnonzero(d < gate)          # NaN distances are never under the gate
    if idx.size == 0:
        return -1
    return int(idx[np.argmin(d[idx])])      # argmin: the first (lowest) index of the minimum


def search_corner(p, last, n_cur, gate):
    """:1305-1361.  Returns (closestPointInd, minPointInd2)."""
    d = sq_dists(last, p)
    ring = last[:, 3].astype(np.int64).tolist()     # int(intensity): truncation
    g = float(gate)
    c = nearest(d, F(gate))
    d = d.tolist()
    m2 = -1
    if c >= 0:
        sc = ring[c]
        md2 = g
        for j in range(c + 1, min(n_cur, len(ring))):
            if ring[j] > sc + 2.5:
                break
            if ring[j] > sc and d[j] < md2:
                md2, m2 = d[j], j
        for j in range(c - 1, -1, -1):
            if ring[j] < sc - 2.5:
                break
            if ring[j] < sc and d[j] < md2:
                md2, m2 = d[j], j
    return c, m2


def search_surf(p, last, n_cur, gate):
    """:1428-1509.  Returns (closestPointInd, minPointInd2, minPointInd3)."""
    d = sq_dists(last, p)
    ring = last[:, 3].astype(np.int64).tolist()     # int(intensity): truncation
    g = float(gate)
    c = nearest(d, F(gate))
    d = d.tolist()
    m2 = m3 = -1
    if c >= 0:
        sc = ring[c]
        md2 = md3 = g
        for j in range(c + 1, min(n_cur, len(ring))):
            if ring[j] > sc + 2.5:
                break
            if ring[j] <= sc:
                if d[j] < md2:
                    md2, m2 = d[j], j
            elif d[j] < md3:
                md3, m3 = d[j], j
        for j in range(c - 1, -1, -1):
            if ring[j] < sc - 2.5:
                break
            if ring[j] >= sc:
                if d[j] < md2:
                    md2, m2 = d[j], j
            elif d[j] < md3:
                md3, m3 = d[j], j
    return c, m2, m3


def corner_coeff(p, t1, t2, it):
    """:1369-1405 -> (coeff[4], selected)."""
    x0, y0, z0 = p[0], p[1], p[2]
    x1, y1, z1 = t1[0], t1[1], t1[2]
    x2, y2, z2 = t2[0], t2[1], t2[2]
    m11 = (x0 - x1) * (y0 - y2) - (x0 - x2) * (y0 - y1)
    m22 = (x0 - x1) * (z0 - z2) - (x0 - x2) * (z0 - z1)
    m33 = (y0 - y1) * (z0 - z2) - (y0 - y2) * (z0 - z1)
    a012 = fsqrt(m11 * m11 + m22 * m22 + m33 * m33)
    l12 = fsqrt((x1 - x2) * (x1 - x2) + (y1 - y2) * (y1 - y2) + (z1 - z2) * (z1 - z2))
    la = ((y1 - y2) * m11 + (z1 - z2) * m22) / a012 / l12
    lb = -((x1 - x2) * m11 - (z1 - z2) * m33) / a012 / l12
    lc = -((x1 - x2) * m22 + (y1 - y2) * m33) / a012 / l12
    ld2 = a012 / l12
    s = F(1)
    if it >= 5:
        s = F(1 - 1.8 * abs(float(ld2)))
    if float(s) > 0.1 and ld2 != 0:
        return np.array([s * la, s * lb, s * lc, s * ld2], F), True
    return np.zeros(4, F), False


def surf_coeff(p, t1, t2, t3, it):
    """:1521-1561 -> (coeff[4], selected)."""
    pa = (t2[1] - t1[1]) * (t3[2] - t1[2]) - (t3[1] - t1[1]) * (t2[2] - t1[2])
    pb = (t2[2] - t1[2]) * (t3[0] - t1[0]) - (t3[2] - t1[2]) * (t2[0] - t1[0])
    pc = (t2[0] - t1[0]) * (t3[1] - t1[1]) - (t3[0] - t1[0]) * (t2[1] - t1[1])
    pd = -(pa * t1[0] + pb * t1[1] + pc * t1[2])
    ps = fsqrt(pa * pa + pb * pb + pc * pc)
    pa = pa / ps
    pb = pb / ps
    pc = pc / ps
    pd = pd / ps
    pd2 = pa * p[0] + pb * p[1] + pc * p[2] + pd
    s = F(1)
    if it >= 5:
        r = fsqrt(fsqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]))
        with np.errstate(all="ignore"):
            s = F(np.float64(1) - np.float64(1.8) * np.float64(abs(float(pd2))) / np.float64(r))
    if float(s) > 0.1 and pd2 != 0:
        return np.array([s * pa, s * pb, s * pc, s * pd2], F), True
    return np.zeros(4, F), False


def correspond(kind, it, qry, last, tc, ind, gate=25.0, period=5):
    """findCorresponding{Surf,Corner}Features(it).  ind: int32 [3, n], the
    cached pointSearch*Ind arrays, refreshed in place on search iterations.
    Returns (coeff [n, 4], sel [n] uint8)."""
    n = qry.shape[0]
    coeff = np.zeros((n, 4), F)
    sel = np.zeros(n, np.uint8)
    gate = F(gate)
    with np.errstate(all="ignore"):
        for i in range(n):
            p = transform_to_start(qry[i], tc)
            if it % period == 0:
                if kind == CORNER:
                    c, m2 = search_corner(p, last, n, gate)
                    ind[:, i] = (c, m2, -1)
                else:
                    ind[:, i] = search_surf(p, last, n, gate)
            i1, i2, i3 = (int(v) for v in ind[:, i])
            if kind == CORNER:
                if i2 >= 0:
                    coeff[i], ok = corner_coeff(p, last[i1], last[i2], it)
                    sel[i] = ok
            elif i2 >= 0 and i3 >= 0:
                coeff[i], ok = surf_coeff(p, last[i1], last[i2], last[i3], it)
                sel[i] = ok
    return coeff, sel


def jacobian_rows(kind, qry, coeff, sel, tc):
    """:1583-1644 / :1716-1757 -> rows [n, 4] = (A0, A1, A2, B); zeros where not selected."""
    srx, crx = fsin(tc[0]), fcos(tc[0])
    sry, cry = fsin(tc[1]), fcos(tc[1])
    srz, crz = fsin(tc[2]), fcos(tc[2])
    tx, ty, tz = F(tc[3]), F(tc[4]), F(tc[5])
    b1 = -crz * sry - cry * srx * srz
    b2 = cry * crz * srx - sry * srz
    b5 = cry * crz - srx * sry * srz
    b6 = cry * srz + crz * srx * sry
    c5 = crx * srz
    rows = np.zeros((qry.shape[0], 4), F)
    with np.errstate(all="ignore"):
        if kind == CORNER:
            b3 = crx * cry
            b4 = tx * -b1 + ty * -b2 + tz * b3
            b7 = crx * sry
            b8 = tz * b7 - ty * b6 - tx * b5
            for i in np.nonzero(sel)[0]:
                x, y, z = qry[i, 0], qry[i, 1], qry[i, 2]
                cx, cy, cz, d2 = coeff[i]
                ary = (b1 * x + b2 * y - b3 * z + b4) * cx + (b5 * x + b6 * y - b7 * z + b8) * cz
                atx = -b5 * cx + c5 * cy + b1 * cz
                atz = b7 * cx - srx * cy - b3 * cz
                rows[i] = (ary, atx, atz, F(-0.05 * float(d2)))
        else:
            a1 = crx * sry * srz
            a2 = crx * crz * sry
            a3 = srx * sry
            a4 = tx * a1 - ty * a2 - tz * a3
            a5 = srx * srz
            a6 = crz * srx
            a7 = ty * a6 - tz * crx - tx * a5
            a8 = crx * cry * srz
            a9 = crx * cry * crz
            a10 = cry * srx
            a11 = tz * a10 + ty * a9 - tx * a8
            c1, c2 = -b6, b5
            c3 = tx * b6 - ty * b5
            c4 = -crx * crz
            c6 = ty * c5 + tx * -c4
            c7, c8 = b2, -b1
            c9 = tx * -b2 - ty * -b1
            for i in np.nonzero(sel)[0]:
                x, y, z = qry[i, 0], qry[i, 1], qry[i, 2]
                cx, cy, cz, d2 = coeff[i]
                arx = ((-a1 * x + a2 * y + a3 * z + a4) * cx + (a5 * x - a6 * y + crx * z + a7) * cy +
                       (a8 * x - a9 * y - a10 * z + a11) * cz)
                arz = ((c1 * x + c2 * y + c3) * cx + (c4 * x - c5 * y + c6) * cy +
                       (c7 * x + c8 * y + c9) * cz)
                aty = -b6 * cx + c4 * cy + b2 * cz
                rows[i] = (arx, arz, aty, F(-0.05 * float(d2)))
    return rows


def normal_equations(rows, sel):
    """AtA [9], AtB [3] float32 in the documented order, and the row count."""
    n = rows.shape[0]
    r64 = rows.astype(np.float64)
    out = np.zeros(12, F)
    with np.errstate(all="ignore"):
        for k in range(12):
            a, b = (k // 3, k % 3) if k < 9 else (k - 9, 3)
            prod = r64[:, a] * r64[:, b]
            total = np.float64(0.0)
            for s in range(32):
                acc = np.float64(0.0)
                for q in range(s, n, 32):
                    if sel[q]:
                        acc = acc + prod[q]
                total = total + acc
            out[k] = F(total)
    return out[:9].copy(), out[9:].copy(), int(np.count_nonzero(sel))


# ------------------------------------------------------------------ OpenCV's solvers, float32
def qr_solve3(A_in, b_in):
    N = 3
    A = [F(v) for v in A_in]
    b = [F(v) for v in b_in]
    x = [F(0)] * N
    for k in range(N):
        nrm = F(0)
        for i in range(k, N):
            nrm = nrm + A[N * i + k] * A[N * i + k]
        nrm = fsqrt(nrm)
        if nrm == 0:
            return None
        alpha = -nrm if A[N * k + k] > 0 else nrm
        v = [F(0)] * N
        for i in range(k, N):
            v[i] = A[N * i + k]
        v[k] = v[k] - alpha
        vv = F(0)
        for i in range(k, N):
            vv = vv + v[i] * v[i]
        if vv == 0:
            continue
        for j in range(k, N):
            d = F(0)
            for i in range(k, N):
                d = d + v[i] * A[N * i + j]
            f = F(2) * d / vv
            for i in range(k, N):
                A[N * i + j] = A[N * i + j] - f * v[i]
        d = F(0)
        for i in range(k, N):
            d = d + v[i] * b[i]
        f = F(2) * d / vv
        for i in range(k, N):
            b[i] = b[i] - f * v[i]
    for i in range(N - 1, -1, -1):
        s = b[i]
        for j in range(i + 1, N):
            s = s - A[N * i + j] * x[j]
        if abs(A[N * i + i]) < F(10) * FLT_EPS:
            return None
        x[i] = s / A[N * i + i]
    return x


def cv_hypot(a, b):
    a, b = abs(a), abs(b)
    if a > b:
        b = b / a
        return a * fsqrt(F(1) + b * b)
    if b > 0:
        a = a / b
        return b * fsqrt(F(1) + a * a)
    return F(0)


def jacobi3(A_in):
    """hal::Jacobi: eigenvalues descending, eigenvectors the rows of V."""
    n = 3
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
        y = (W[l] - W[k]) * F(0.5)
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

        def rot(M, i0, i1):
            a0, b0 = M[i0], M[i1]
            M[i0] = a0 * c - b0 * s
            M[i1] = a0 * s + b0 * c

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


def inv3(S):
    """cv::invert on 3 x 3 float: the adjugate over the determinant, in double."""
    s = [[float(S[3 * r + c]) for c in range(3)] for r in range(3)]
    d = (s[0][0] * (s[1][1] * s[2][2] - s[1][2] * s[2][1]) - s[0][1] * (s[1][0] * s[2][2] - s[1][2] * s[2][0]) +
         s[0][2] * (s[1][0] * s[2][1] - s[1][1] * s[2][0]))
    if d == 0.0:
        return [F(0)] * 9
    d = 1.0 / d
    return [F((s[1][1] * s[2][2] - s[1][2] * s[2][1]) * d), F((s[0][2] * s[2][1] - s[0][1] * s[2][2]) * d),
            F((s[0][1] * s[1][2] - s[0][2] * s[1][1]) * d), F((s[1][2] * s[2][0] - s[1][0] * s[2][2]) * d),
            F((s[0][0] * s[2][2] - s[0][2] * s[2][0]) * d), F((s[0][2] * s[1][0] - s[0][0] * s[1][2]) * d),
            F((s[1][0] * s[2][1] - s[1][1] * s[2][0]) * d), F((s[0][1] * s[2][0] - s[0][0] * s[2][1]) * d),
            F((s[0][0] * s[1][1] - s[0][1] * s[1][0]) * d)]


def step(kind, AtA, AtB, it, tc, is_degenerate, matP):
    """calculateTransformation{Surf,Corner} from cv::solve on (:1649-1695 /
    :1764-1814).  tc, matP: float32 arrays updated in place.  Returns
    (keep_going, is_degenerate)."""
    with np.errstate(all="ignore"):
        X = qr_solve3(AtA, AtB)
        if X is None:
            X = [F(0)] * 3
        if it == 0:
            E, V = jacobi3(AtA)
            V2 = list(V)
            is_degenerate = 0
            for i in (2, 1, 0):
                if E[i] < F(10):
                    for j in range(3):
                        V2[3 * i + j] = F(0)
                    is_degenerate = 1
                else:
                    break
            Vi = inv3(V)
            for i in range(3):
                for j in range(3):
                    s = 0.0
                    for k in range(3):
                        s = s + float(Vi[3 * i + k]) * float(V2[3 * k + j])
                    matP[3 * i + j] = F(s)
        if is_degenerate:
            X2 = []
            for i in range(3):
                s = 0.0
                for k in range(3):
                    s = s + float(matP[3 * i + k]) * float(X[k])
                X2.append(F(s))
            X = X2
        comp = (0, 2, 4) if kind == SURF else (1, 3, 5)
        for c, x in zip(comp, X):
            tc[c] = tc[c] + x
        for i in range(6):
            if np.isnan(tc[i]):
                tc[i] = 0
        r2d = lambda v: float(v) * 180.0 / math.pi  # noqa: E731
        cm = lambda v: float(v * F(100))  # noqa: E731
        if kind == SURF:
            dR = F(fsqrt64(r2d(X[0]) * r2d(X[0]) + r2d(X[1]) * r2d(X[1])))
            dT = F(fsqrt64(cm(X[2]) * cm(X[2])))
        else:
            dR = F(fsqrt64(r2d(X[0]) * r2d(X[0])))
            dT = F(fsqrt64(cm(X[1]) * cm(X[1]) + cm(X[2]) * cm(X[2])))
        keep = not (float(dR) < 0.1 and float(dT) < 0.1)
    return keep, is_degenerate


def fsqrt64(v):
    return math.sqrt(v) if v == v and v >= 0 else float("nan")


# ------------------------------------------------------------------ the transforms around the loop
def accumulate_rotation(cx, cy, cz, lx, ly, lz):
    """:1246-1285."""
    scx, ccx, scy, ccy, scz, ccz = fsin(cx), fcos(cx), fsin(cy), fcos(cy), fsin(cz), fcos(cz)
    slx, clx, sly, cly, slz, clz = fsin(lx), fcos(lx), fsin(ly), fcos(ly), fsin(lz), fcos(lz)
    srx = clx * ccx * sly * scz - ccx * ccz * slx - clx * cly * scx
    ox = -fasin(srx)
    srycrx = (slx * (ccy * scz - ccz * scx * scy) + clx * sly * (ccy * ccz + scx * scy * scz) +
              clx * cly * ccx * scy)
    crycrx = (clx * cly * ccx * ccy - clx * sly * (ccz * scy - ccy * scx * scz) -
              slx * (scy * scz + ccy * ccz * scx))
    oy = fatan2(srycrx / fcos(ox), crycrx / fcos(ox))
    srzcrx = (scx * (clz * sly - cly * slx * slz) + ccx * scz * (cly * clz + slx * sly * slz) +
              clx * ccx * ccz * slz)
    crzcrx = (clx * clz * ccx * ccz - ccx * scz * (cly * slz - clz * slx * sly) -
              scx * (sly * slz + cly * clz * slx))
    oz = fatan2(srzcrx / fcos(ox), crzcrx / fcos(ox))
    return ox, oy, oz


def plugin_imu_rotation(bcx, bcy, bcz, blx, bly, blz, alx, aly, alz):
    """:1145-1244, the repeated parenthesised factors named once."""
    sbcx, cbcx, sbcy, cbcy, sbcz, cbcz = fsin(bcx), fcos(bcx), fsin(bcy), fcos(bcy), fsin(bcz), fcos(bcz)
    sblx, cblx, sbly, cbly, sblz, cblz = fsin(blx), fcos(blx), fsin(bly), fcos(bly), fsin(blz), fcos(blz)
    salx, calx, saly, caly, salz, calz = fsin(alx), fcos(alx), fsin(aly), fcos(aly), fsin(alz), fcos(alz)
    u1 = cbly * sblz - cblz * sblx * sbly
    u2 = sbly * sblz + cbly * cblz * sblx
    u3 = cblz * sbly - cbly * sblx * sblz
    u4 = cbly * cblz + sblx * sbly * sblz
    T1 = calx * saly * u1 - calx * caly * u2 + cblx * cblz * salx
    T2 = calx * caly * u3 - calx * saly * u4 + cblx * salx * sblz
    T3 = salx * sblx + calx * caly * cblx * cbly + calx * cblx * saly * sbly
    srx = -sbcx * T3 - cbcx * cbcz * T1 - cbcx * sbcz * T2
    acx = -fasin(srx)
    srycrx = ((cbcy * sbcz - cbcz * sbcx * sbcy) * T1 - (cbcy * cbcz + sbcx * sbcy * sbcz) * T2 +
              cbcx * sbcy * T3)
    crycrx = ((cbcz * sbcy - cbcy * sbcx * sbcz) * T2 - (sbcy * sbcz + cbcy * cbcz * sbcx) * T1 +
              cbcx * cbcy * T3)
    acy = fatan2(srycrx / fcos(acx), crycrx / fcos(acx))
    v1 = caly * calz + salx * saly * salz
    v2 = calz * saly - caly * salx * salz
    v3 = saly * salz + caly * calz * salx
    v4 = caly * salz - calz * salx * saly
    srzcrx = (sbcx * (cblx * cbly * v2 - cblx * sbly * v1 + calx * salz * sblx) -
              cbcx * cbcz * (v1 * u1 + v2 * u2 - calx * cblx * cblz * salz) +
              cbcx * sbcz * (v1 * u4 + v2 * u3 + calx * cblx * salz * sblz))
    crzcrx = (sbcx * (cblx * sbly * v4 - cblx * cbly * v3 + calx * calz * sblx) +
              cbcx * cbcz * (v3 * u2 + v4 * u1 + calx * calz * cblx * cblz) -
              cbcx * sbcz * (v3 * u3 + v4 * u4 - calx * calz * cblx * sblz))
    acz = fatan2(srzcrx / fcos(acx), crzcrx / fcos(acx))
    return acx, acy, acz


def f3(v=None):
    return np.zeros(3, F) if v is None else np.asarray(v, F).copy()


class OdomModel:
    """FeatureAssociation's back-half members and runFeatureAssociation
    :2232-2248 on the four feature clouds, the outlier cloud and the IMU state
    adjustDistortion leaves (`imu_out`: rpy_start, rpy_cur, velo_from_start,
    angular_from_start; None = no IMU, all zero)."""

    def __init__(self, gate=25.0, max_iter=25, period=5, skip_frame_num=1, scan_period=0.1):
        self.gate, self.max_iter, self.period = gate, max_iter, period
        self.skip, self.scan_period = skip_frame_num, F(scan_period)
        self.reset()

    def reset(self):
        self.transformCur = np.zeros(6, F)
        self.transformSum = np.zeros(6, F)
        self.imu_last = f3()          # roll, pitch, yaw
        self.imu_shift = f3()         # stays 0
        self.imu_velo = f3()
        self.inited = False
        self.isDegenerate = 0
        self.matP = np.zeros(9, F)
        self.frameCount = self.skip       # the constructor's `frameCount = skipFrameNum` (:354)
        self.corner_last = np.zeros((0, 4), F)
        self.surf_last = np.zeros((0, 4), F)
        self.outlier_last = np.zeros((0, 4), F)

    # -- updateTransformation on given clouds; also used alone for injected cases
    def loop(self, kind, qry, last, tc, log=None):
        ind = np.full((3, qry.shape[0]), -1, np.int32)
        iters = rows_n = deg0 = 0
        for it in range(self.max_iter):
            coeff, sel = correspond(kind, it, qry, last, tc, ind, self.gate, self.period)
            rows = jacobian_rows(kind, qry, coeff, sel, tc)
            AtA, AtB, nsel = normal_equations(rows, sel)
            iters, rows_n = it + 1, nsel
            if log is not None:
                log.append(dict(kind=kind, it=it, nsel=nsel, AtA=AtA, AtB=AtB, ind=ind.copy(),
                                coeff=coeff, sel=sel, tc=tc.copy()))
            if nsel < 10:
                continue
            keep, self.isDegenerate = step(kind, AtA, AtB, it, tc, self.isDegenerate, self.matP)
            if it == 0:
                deg0 = self.isDegenerate
            if not keep:
                break
        return iters, rows_n, deg0

    def update_transformation(self, sharp, flat, log=None):
        out = dict(iters=[0, 0], rows=[0, 0], degenerate=[0, 0])
        if self.corner_last.shape[0] < 10 or self.surf_last.shape[0] < 100:
            return out
        for kind, qry, last in ((SURF, flat, self.surf_last), (CORNER, sharp, self.corner_last)):
            i, r, d = self.loop(kind, qry, last, self.transformCur, log)
            out["iters"][kind], out["rows"][kind], out["degenerate"][kind] = i, r, d
        return out

    def run(self, sharp, less_sharp, flat, less_flat, outlier, imu_out=None, log=None):
        io = imu_out or {}
        rpy_start, rpy_cur = f3(io.get("rpy_start")), f3(io.get("rpy_cur"))
        velo, ang = f3(io.get("velo_from_start")), f3(io.get("angular_from_start"))
        if not self.inited:
            # checkSystemInitialization
            self.corner_last, self.surf_last = less_sharp.copy(), less_flat.copy()
            self.transformSum[0] += rpy_start[1]
            self.transformSum[2] += rpy_start[0]
            self.inited = True
            return dict(inited=0, iters=[0, 0], rows=[0, 0], degenerate=[0, 0], published=0,
                        transform_cur=self.transformCur.copy(), transform_sum=self.transformSum.copy())
        # updateInitialGuess
        tc = self.transformCur
        self.imu_last = rpy_cur.copy()
        self.imu_velo = velo.copy()
        if ang[0] != 0 or ang[1] != 0 or ang[2] != 0:
            tc[0], tc[1], tc[2] = -ang[1], -ang[2], -ang[0]
        if velo[0] != 0 or velo[1] != 0 or velo[2] != 0:
            for k in range(3):
                tc[3 + k] = tc[3 + k] - velo[k] * self.scan_period
        self.guess = tc.copy()
        out = self.update_transformation(sharp, flat, log)
        out["inited"] = 1
        # integrateTransformation
        ts, sh = self.transformSum, self.imu_shift
        rx, ry, rz = accumulate_rotation(ts[0], ts[1], ts[2], -tc[0], -tc[1], -tc[2])
        x1 = fcos(rz) * (tc[3] - sh[0]) - fsin(rz) * (tc[4] - sh[1])
        y1 = fsin(rz) * (tc[3] - sh[0]) + fcos(rz) * (tc[4] - sh[1])
        z1 = tc[5] - sh[2]
        x2 = x1
        y2 = fcos(rx) * y1 - fsin(rx) * z1
        z2 = fsin(rx) * y1 + fcos(rx) * z1
        tx = ts[3] - (fcos(ry) * x2 + fsin(ry) * z2)
        ty = ts[4] - y2
        tz = ts[5] - (-fsin(ry) * x2 + fcos(ry) * z2)
        rx, ry, rz = plugin_imu_rotation(rx, ry, rz, rpy_start[1], rpy_start[2], rpy_start[0],
                                         self.imu_last[1], self.imu_last[2], self.imu_last[0])
        self.transformSum = np.array([rx, ry, rz, tx, ty, tz], F)
        # publishCloudsLast
        self.corner_last = np.array([transform_to_end(p, tc, rpy_start, sh, self.imu_last)
                                     for p in less_sharp], F).reshape(-1, 4)
        self.surf_last = np.array([transform_to_end(p, tc, rpy_start, sh, self.imu_last)
                                   for p in less_flat], F).reshape(-1, 4)
        self.frameCount += 1
        out["published"] = 0
        if self.frameCount >= self.skip + 1:
            self.frameCount = 0
            out["published"] = 1
            self.outlier_last = outlier[:, [1, 2, 0, 3]].astype(F)   # adjustOutlierCloud
        out["transform_cur"] = tc.copy()
        out["transform_sum"] = self.transformSum.copy()
        return out

    def odometry_pose(self):
        """publishOdometry: (quaternion xyzw, position)."""
        return odometry_pose(self.transformSum)


def odometry_pose(ts):
    """tf::createQuaternionMsgFromRollPitchYaw(ts[2], -ts[0], -ts[1]) (tf's
    setRPY, double) re-ordered as publishOdometry does."""
    roll, pitch, yaw = float(ts[2]), -float(ts[0]), -float(ts[1])
    hy, hp, hr = yaw * 0.5, pitch * 0.5, roll * 0.5
    cy, sy, cp, sp, cr, sr = math.cos(hy), math.sin(hy), math.cos(hp), math.sin(hp), math.cos(hr), math.sin(hr)
    qx = sr * cp * cy - cr * sp * sy
    qy = cr * sp * cy + sr * cp * sy
    qz = cr * cp * sy - sr * sp * cy
    qw = cr * cp * cy + sr * sp * sy
    return np.array([-qy, -qz, qx, qw]), np.array([float(ts[3]), float(ts[4]), float(ts[5])])
