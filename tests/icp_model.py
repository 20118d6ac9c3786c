"""numpy restatement of the loop-closure ICP (include/slio.h, slio_icp_*) and
the fixture the ICP tests share.  No device, no library."""
import math

import numpy as np

f32 = np.float32
NOT_CONVERGED, ITERATIONS, TRANSFORM, ABS_MSE, REL_MSE, NO_CORRESPONDENCES = range(6)
DBL_MAX = float(np.finfo(np.float64).max)


def scene(rng, n):
    """Ground, the wall y = 6 and the wall x = -5, float32; each patch draws
    its columns in x, y, z order."""
    n0, n1 = n // 2, n // 4
    n2 = n - n0 - n1
    g = np.stack([rng.uniform(-8, 8, n0), rng.uniform(-8, 8, n0), rng.normal(0, 0.02, n0)], axis=1)
    a = np.stack([rng.uniform(-8, 8, n1), 6 + rng.normal(0, 0.02, n1), rng.uniform(0, 3, n1)], axis=1)
    b = np.stack([-5 + rng.normal(0, 0.02, n2), rng.uniform(-8, 8, n2), rng.uniform(0, 3, n2)], axis=1)
    return np.concatenate([g, a, b]).astype(f32)


def rot_zyx(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = (math.cos(roll), math.sin(roll), math.cos(pitch), math.sin(pitch),
                              math.cos(yaw), math.sin(yaw))
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


FIX_R = rot_zyx(0.01, -0.015, 0.035)
FIX_T = np.array([0.3, -0.2, 0.05])


def fixture():
    """tgt = scene(1500), src = the rigid motion (R, t) undone on scene(400)."""
    rng = np.random.default_rng(20261020)
    tgt = scene(rng, 1500)
    src_w = scene(rng, 400)
    src = ((src_w - FIX_T.astype(f32)) @ FIX_R.astype(f32)).astype(f32)
    return tgt, src


def transform32(T, pts):
    """((m0 x + m1 y) + m2 z) + m3 per coordinate, float32."""
    T = np.asarray(T, f32).reshape(4, 4)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], axis=1).astype(f32)


def nearest32(work, tgt):
    """Brute-force 1-NN in float32: index (lowest index among ties), squared
    distance (dx dx + dy dy) + dz dz, and whether the nearest distance is
    shared by another target point.  Non-finite working points: index -1,
    distance +inf."""
    n = work.shape[0]
    idx = np.full(n, -1, np.int64)
    sqd = np.full(n, np.inf, f32)
    tie = np.zeros(n, bool)
    if tgt.shape[0] == 0:
        return idx, sqd, tie
    fin = np.isfinite(work).all(axis=1)
    w = work[fin]
    d = w[:, None, :] - tgt[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    assert d2.dtype == f32
    j = np.argmin(d2, axis=1)
    m = d2[np.arange(w.shape[0]), j]
    idx[fin] = j
    sqd[fin] = m
    tie[fin] = (d2 == m[:, None]).sum(axis=1) > 1
    return idx, sqd, tie


def sum_terms(work, tgt, idx, sqd, max_dist):
    """The correspondences' exact double terms, (16, ncorr): p (3), q (3),
    q_r p_c (9, row-major), sqd; and the correspondence mask."""
    ok = (idx >= 0) & (sqd.astype(np.float64) <= float(max_dist) * float(max_dist))
    p = work[ok].astype(np.float64)
    q = tgt[idx[ok]].astype(np.float64)
    rows = [p[:, a] for a in range(3)] + [q[:, a] for a in range(3)]
    rows += [q[:, r] * p[:, c] for r in range(3) for c in range(3)]
    rows.append(sqd[ok].astype(np.float64))
    return np.array(rows).reshape(16, p.shape[0]), ok


def fsums(terms):
    return np.array([math.fsum(r) for r in terms])


def sum_bounds(terms):
    """(n - 1) 2^-53 sum|term|: the bound any summation order satisfies."""
    n = terms.shape[1]
    return np.array([(max(n - 1, 0) * 2.0 ** -53) * math.fsum(np.abs(r)) for r in terms])


def umeyama(sums, n, dtype=np.float64):
    """TransformationEstimationSVD from the sums: float32 4x4 delta.  dtype =
    float32 runs the fit as PCL does, in float."""
    s = np.asarray(sums, np.float64)
    mp = (s[0:3] / n).astype(dtype)
    mq = (s[3:6] / n).astype(dtype)
    S = (s[6:15].reshape(3, 3) / n).astype(dtype) - np.outer(mq, mp).astype(dtype)
    U, _, Vt = np.linalg.svd(S)
    D = np.eye(3, dtype=dtype)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        D[2, 2] = -1
    R = (U @ D @ Vt).astype(dtype)
    t = (mq - R @ mp).astype(dtype)
    out = np.eye(4, dtype=f32)
    out[:3, :3] = R.astype(f32)
    out[:3, 3] = t.astype(f32)
    return out


def matmul32(A, B):
    """float32 4x4 product, terms added in index order."""
    A = np.asarray(A, f32).reshape(4, 4)
    B = np.asarray(B, f32).reshape(4, 4)
    C = np.zeros((4, 4), f32)
    for r in range(4):
        for c in range(4):
            s = A[r, 0] * B[0, c]
            for k in range(1, 4):
                s = f32(s + A[r, k] * B[k, c])
            C[r, c] = s
    return C


class State:
    def __init__(self, guess=None):
        self.final_T = np.eye(4, dtype=f32) if guess is None else np.asarray(guess, f32).reshape(4, 4).copy()
        self.prev_mse = DBL_MAX
        self.iterations = 0
        self.state = NOT_CONVERGED
        self.converged = False


def step(sums, ncorr, st, max_iterations=100, t_eps=1e-6, fit_eps=1e-6, dtype=np.float64):
    """One turn of computeTransformation's loop: (delta, done)."""
    st.state = NOT_CONVERGED
    if ncorr < 3:
        st.state, st.converged = NO_CORRESPONDENCES, False
        return np.eye(4, dtype=f32), True
    delta = umeyama(sums, ncorr, dtype)
    st.final_T = matmul32(delta, st.final_T)
    st.iterations += 1

    def conv(s):
        st.state, st.converged = s, True
        return delta, True

    if st.iterations >= max_iterations:
        return conv(ITERATIONS)
    d = delta.astype(np.float64)
    cos = 0.5 * ((d[0, 0] + d[1, 1] + d[2, 2]) - 1.0)
    t2 = (d[0, 3] * d[0, 3] + d[1, 3] * d[1, 3]) + d[2, 3] * d[2, 3]
    if cos >= 0.99999 and t2 <= t_eps:
        return conv(TRANSFORM)
    mse = sums[15] / ncorr
    if abs(mse - st.prev_mse) < fit_eps:
        return conv(ABS_MSE)
    if abs(mse - st.prev_mse) / st.prev_mse < 1e-5:
        return conv(REL_MSE)
    st.prev_mse = mse
    st.converged = False
    return delta, False


def icp_run(src, tgt, max_dist, dtype=np.float64, guess=None):
    """The whole alignment on the CPU.  Returns a dict: converged, final_T,
    fitness, iterations, state, ties (any exact nearest / second-nearest tie
    in any pass), gated_first (points without a correspondence in pass 1),
    fitness_terms."""
    st = State(guess)
    work = transform32(st.final_T, src)
    ties, gated_first = False, None
    while True:
        idx, sqd, tie = nearest32(work, tgt)
        ties |= bool(tie.any())
        terms, ok = sum_terms(work, tgt, idx, sqd, max_dist)
        if gated_first is None:
            gated_first = int((~ok).sum())
        delta, done = step(fsums(terms), int(ok.sum()), st, dtype=dtype)
        if done:
            break
        work = transform32(delta, work)
    fin = transform32(st.final_T, src)
    idx, sqd, tie = nearest32(fin, tgt)
    ties |= bool(tie.any())
    terms, ok = sum_terms(fin, tgt, idx, sqd, math.inf)
    n = int(ok.sum())
    return dict(converged=st.converged, final_T=st.final_T, fitness=math.fsum(terms[15]) / n if n else DBL_MAX,
                iterations=st.iterations, state=st.state, ties=ties, gated_first=gated_first,
                fitness_terms=terms[15])
