"""Crafted cases for step 5 of ImuProcess::UndistortPcl (IMU_Processing.hpp:
360-401, the per-point back-propagation: k_undistort on the device,
orc_undistort_points in the oracle) and an independent reference.

The reference evaluates

    P' = R_LI^T (R_end^T (R_head Exp(gyr_tail dt) (R_LI P + T_LI) + T_ei) - T_LI)

as a product of 4x4 homogeneous transforms in numpy.longdouble, with Exp by
Rodrigues' formula on libm sin and cos (no series, no branch on the angle), and rounds
to float32 once.  It shares no code with the oracle and no formula layout with
the kernel.  A point belongs to the segment with the largest k <= npose - 2
such that off[k] < t / 1000 (t / 1000 the fp64 quotient the reference program
forms), found by a plain linear scan.  The first point of the sorted order is
outside the reference: the program's `it_pcl == begin` quirk compensates it
once per earlier segment, rounding to float every time (checked against the
oracle only).

Every case has a non-identity R_LI (35 degrees about a skew axis), a non-zero
T_LI, and points at ranges of 2 to 80 m in shuffled time order.
check_cases() asserts on the model alone that each case reaches what it is
named for."""
import functools

import numpy as np

LD = np.longdouble
F = np.float32

# 64 fp64 roundings' worth of slack for the ~40-operation chain (see bound())
CHAIN_EPS = 64.0 * 2.0 ** -53


# ---------------------------------------------------------------- inputs (fp64, plain)
def _rot64(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    a = w / th
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def _quat64(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.deg2rad(deg) / 2
    return np.concatenate([[np.cos(h)], np.sin(h) * a])


RLI_Q = _quat64([1.0, 2.0, -1.5], 35.0)
TLI = np.array([0.12, -0.05, 0.30])


def make_table(off, seed, gyr=None):
    """An IMUpose table (npose, 22): offset, acc, gyr, vel, pos, rot row-major.
    gyr: {row: vector} overrides (row k is the tail of segment k - 1)."""
    rng = np.random.default_rng(1000 + seed)
    off = np.asarray(off, np.float64)
    tab = np.zeros((off.size, 22))
    R = _rot64(rng.normal(0, 0.3, 3))
    pos = rng.normal(0, 2.0, 3)
    vel = np.array([1.5, 0.2, -0.1]) + rng.normal(0, 0.1, 3)
    for k in range(off.size):
        tab[k, 0] = off[k]
        tab[k, 1:4] = np.array([0.3, 0.1, 0.2]) + rng.normal(0, 1.0, 3)
        tab[k, 4:7] = np.array([0.1, -0.2, 0.8]) + rng.normal(0, 0.01, 3)
        tab[k, 7:10] = vel
        tab[k, 10:13] = pos
        tab[k, 13:22] = R.reshape(-1)
        R = R @ _rot64(rng.normal(0, 0.004, 3))
        pos = pos + vel * 0.005
        vel = vel + rng.normal(0, 0.01, 3)
    for k, g in (gyr or {}).items():
        tab[k, 4:7] = g
    return tab


def end_state(tab, seed):
    """state26 at the scan end: pos 0, rot 3 (w x y z), rli 7, tli 11, rest unused."""
    rng = np.random.default_rng(2000 + seed)
    st = np.zeros(26)
    st[0:3] = (tab[-1, 10:13] if tab.shape[0] else np.zeros(3)) + rng.normal(0, 0.01, 3)
    q = _quat64(rng.normal(0, 1, 3), rng.uniform(10, 60))
    st[3:7] = q / np.linalg.norm(q)
    st[7:11] = RLI_Q
    st[11:14] = TLI
    st[23:26] = [0.0, 0.0, -9.81]
    return st


def make_points(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return (d * rng.uniform(2, 80, (n, 1))).astype(F)


def regular(m, step=0.005):
    return step * np.arange(m)


def negative(m, d):
    """[0, -d, 0.005 - d, 0.010 - d, ...]: an IMU sample d seconds before the
    scan start (after the previous scan's end), then the usual 5 ms grid."""
    return np.concatenate([[0.0, -d], 0.005 * np.arange(1, m - 1) - d])


def _axis(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# ---------------------------------------------------------------- the model
def tt_of(t):
    """curvature / double(1000), as the reference program forms it."""
    return np.asarray(t, F).astype(np.float64) / np.float64(1000)


def segment_linear(off, tt):
    """largest k <= npose - 2 with off[k] < tt, or -1 (ascending scan: the
    last hit stays)."""
    seg = -1
    for k in range(len(off) - 1):
        if off[k] < tt:
            seg = k
    return seg


def segment_bisect(off, tt):
    """The search k_undistort used to make: right on increasing tables only."""
    lo, a, b = -1, 0, len(off) - 2
    while a <= b:
        m = (a + b) >> 1
        if off[m] < tt:
            lo, a = m, m + 1
        else:
            b = m - 1
    return lo


def first_heads(off, tt, stop_at_miss=False):
    """Heads that compensate the first sorted point, in order: its own segment,
    then every earlier head whose offset is below its time.  stop_at_miss: the
    loop k_undistort used to run, which ended at the first head that is not."""
    out = []
    for k in range(segment_linear(off, tt), -1, -1):
        if off[k] < tt:
            out.append(k)
        elif stop_at_miss:
            break
    return out


def so3_branch(theta):
    """0: theta < 1e-10; 1: the Taylor series (theta / 2 < 0.125); 2: sincos."""
    return 0 if theta < 1e-10 else (1 if 0.5 * theta < 0.125 else 2)


def model(case):
    """Sorted order, fp64 times, segment, dt, theta and so3_exp branch of every
    point (segment -1: not touched), and the heads of the first point."""
    tab = case["tab"]
    order = np.argsort(case["t"], kind="stable")   # -0.0 == +0.0: a tie
    t = case["t"][order]
    tt = tt_of(t)
    off = tab[:, 0]
    seg = np.array([segment_linear(off, v) for v in tt], np.int64).reshape(-1)
    old = np.array([segment_bisect(off, v) for v in tt], np.int64).reshape(-1)
    dt, theta = np.zeros(t.size), np.zeros(t.size)
    hit = seg >= 0
    if hit.any():
        dt[hit] = tt[hit] - off[seg[hit]]
        theta[hit] = np.linalg.norm(tab[seg[hit] + 1, 4:7], axis=1) * dt[hit]
    branch = np.array([so3_branch(v) if s >= 0 else -1 for v, s in zip(theta, seg)], np.int64).reshape(-1)
    heads = first_heads(off, tt[0]) if t.size else []
    heads_old = first_heads(off, tt[0], stop_at_miss=True) if t.size else []
    return dict(order=order, t=t, tt=tt, seg=seg, seg_bisect=old, dt=dt, theta=theta, branch=branch,
                first_heads=heads, first_heads_old=heads_old)


# ---------------------------------------------------------------- the longdouble reference
def _rot_ld(q):
    q = np.asarray(q, LD)
    q = q / np.sqrt((q * q).sum())
    w, v = q[0], q[1:4]
    K = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], LD)
    return (w * w - (v * v).sum()) * np.eye(3, dtype=LD) + LD(2) * np.outer(v, v) + LD(2) * w * K


def _hom(R, t):
    T = np.zeros(R.shape[:-2] + (4, 4), LD)
    T[..., :3, :3] = R
    T[..., :3, 3] = t
    T[..., 3, 3] = 1
    return T


def _hom_inv(T):
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    return _hom(Rt, -(Rt @ T[..., :3, 3:4])[..., 0])


def _exp_ld(w):
    """Rodrigues: I + sin(th) K + (1 - cos(th)) K^2, K = hat(w / th)."""
    w = np.asarray(w, LD)
    th = np.sqrt((w * w).sum(axis=-1))
    a = np.where(th[:, None] > 0, w / np.where(th > 0, th, LD(1))[:, None], LD(0))
    K = np.zeros(w.shape[:-1] + (3, 3), LD)
    K[:, 0, 1], K[:, 0, 2] = -a[:, 2], a[:, 1]
    K[:, 1, 0], K[:, 1, 2] = a[:, 2], -a[:, 0]
    K[:, 2, 0], K[:, 2, 1] = -a[:, 1], a[:, 0]
    s, c = np.sin(th), np.cos(th)
    return np.eye(3, dtype=LD) + s[:, None, None] * K + (LD(1) - c)[:, None, None] * (K @ K)


def reference(case, mdl=None):
    """(ref (n, 3) longdouble in sorted order, scale (n,), checked (n,) bool):
    the exact value of every compensated point, the bound's scale ||P|| +
    ||T_LI|| + ||T_ei|| + 1, and which rows the reference covers (finite
    input, not the first point).  Untouched rows keep their input."""
    assert np.finfo(LD).eps < 1e-18, "numpy.longdouble is not wider than double here"
    mdl = mdl or model(case)
    tab, st = case["tab"], case["state"]
    P = case["pts"][mdl["order"]]
    n = P.shape[0]
    ref = P.astype(LD)
    scale = np.linalg.norm(P.astype(np.float64), axis=1) + np.linalg.norm(st[11:14]) + 1.0
    seg = mdl["seg"]
    hit = np.nonzero(seg >= 0)[0]
    if hit.size:
        k = seg[hit]
        dt = mdl["tt"][hit].astype(LD) - tab[k, 0].astype(LD)
        T_li = _hom(_rot_ld(st[7:11]), st[11:14].astype(LD))
        T_end = _hom(_rot_ld(st[3:7]), st[0:3].astype(LD))
        R_i = tab[k, 13:22].astype(LD).reshape(-1, 3, 3) @ _exp_ld(tab[k + 1, 4:7].astype(LD) * dt[:, None])
        p_i = (tab[k, 10:13].astype(LD) + tab[k, 7:10].astype(LD) * dt[:, None]
               + tab[k + 1, 1:4].astype(LD) * (dt * dt)[:, None] / LD(2))
        chain = _hom_inv(T_li) @ _hom_inv(T_end) @ _hom(R_i, p_i) @ T_li
        ph = np.concatenate([P[hit].astype(LD), np.ones((hit.size, 1), LD)], 1)
        with np.errstate(invalid="ignore"):
            ref[hit] = (chain @ ph[:, :, None])[:, :3, 0]
        scale[hit] += np.linalg.norm((p_i - st[0:3].astype(LD)).astype(np.float64), axis=1)
    checked = np.isfinite(P).all(axis=1)
    if n:
        checked[0] = False
    return ref, scale, checked


def ulp32(v):
    """The float32 spacing of the binade that holds |v| (v longdouble)."""
    _, e = np.frexp(np.abs(v))
    return np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 24, -149).astype(np.int32))


def bound(ref, scale):
    """|got - ref| <= 0.5 ulp32(ref) + 64 * 2^-53 * (||P|| + ||T_LI|| + ||T_ei||
    + 1): the final rounding to float, plus an fp64 chain of about 40
    operations on values no larger than the scale."""
    return LD(0.5) * ulp32(ref) + (LD(CHAIN_EPS) * scale.astype(LD))[:, None]


def worst_ratio(got, ref, scale, checked):
    """max over the checked rows of |got - ref| / bound."""
    if not checked.any():
        return 0.0
    err = np.abs(got[checked].astype(LD) - ref[checked])
    return float((err / bound(ref[checked], scale[checked])).max())


def worst_chain_ratio(got, ref, scale, checked):
    """For reading, not asserting: how much of the bound's second term is
    used, max over the checked rows of (|got - ref| - 0.5 ulp32(ref)) / (64 *
    2^-53 * scale), 0 where the float is the correctly rounded one."""
    if not checked.any():
        return 0.0
    r = ref[checked]
    over = np.abs(got[checked].astype(LD) - r) - LD(0.5) * ulp32(r)
    return float(np.maximum(over / (LD(CHAIN_EPS) * scale[checked].astype(LD))[:, None], 0).max())


def float_key(a):
    """float32 -> int64 in float order (adjacent floats differ by 1)."""
    i = np.ascontiguousarray(a, F).view(np.int32).astype(np.int64)
    return np.where(i >= 0, i, -(i & 0x7FFFFFFF))


# ---------------------------------------------------------------- the cases
def _case(name, tab, pts, t, seed, checks=()):
    pts, t = np.ascontiguousarray(pts, F).reshape(-1, 3), np.ascontiguousarray(t, F).reshape(-1)
    assert pts.shape[0] == t.shape[0]
    return dict(name=name, tab=tab, state=end_state(tab, seed), pts=pts, t=t, checks=list(checks))


def _shuffled(rng, pts, t):
    p = rng.permutation(t.shape[0])
    return pts[p], t[p]


def _reaches(*want, only=False):
    def chk(c, m):
        got = set(m["branch"][m["seg"] >= 0].tolist())
        assert set(want) <= got and (not only or got == set(want)), (c["name"], got, want)
    return chk


def _gyro_cases():
    out = []
    rng = np.random.default_rng(11)
    # exactly zero gyro in the tails of segments 1, 2 and 4
    tab = make_table(regular(8), 1, gyr={2: np.zeros(3), 3: np.zeros(3), 5: np.zeros(3)})
    n = 400

    def zero_theta(c, m):
        z = (m["seg"] >= 0) & (m["theta"] == 0.0)
        assert set(m["seg"][z].tolist()) == {1, 2, 4} and z.sum() > 50
    out.append(_case("gyro_zero", tab, make_points(rng, n), rng.uniform(0.1, 40, n), 1,
                     [_reaches(0, 1), zero_theta]))
    # |gyr| dt near 1e-12
    g = {k: 2e-10 * _axis([1, -2, 0.5]) for k in range(8)}

    def tiny(c, m):
        th = m["theta"][m["seg"] >= 0]
        assert (th > 0).all() and th.max() < 3e-12 and np.median(th) > 2e-13
    out.append(_case("gyro_tiny", make_table(regular(8), 2, gyr=g), make_points(rng, n), rng.uniform(0.1, 45, n), 2,
                     [_reaches(0, only=True), tiny]))
    # theta from 0.245 to 0.255 across half = 0.125: segment 2 is 10 ms long, its tail spins at 50 rad/s
    off = np.array([0, 0.005, 0.010, 0.020, 0.025, 0.030])
    tab = make_table(off, 3, gyr={3: 50.0 * _axis([0.3, -1, 2])})
    t = np.concatenate([np.linspace(14.9, 15.1, 300), rng.uniform(0.1, 35, 200)])

    def sweep(c, m):
        th = m["theta"][m["seg"] == 2]
        lo, hi = ((th >= 0.245) & (th < 0.25)).sum(), ((th >= 0.25) & (th <= 0.255)).sum()
        assert lo > 100 and hi > 100, (lo, hi)
        b = m["branch"][m["seg"] == 2]
        assert ((th < 0.25) == (b == 1)).all()
    out.append(_case("gyro_switch", tab, *_shuffled(rng, make_points(rng, 500), t), 3, [_reaches(1, 2), sweep]))
    # a 50 ms IMU dropout: about 0.9 rad at 18 rad/s, about 4 rad (past pi) at 80 rad/s
    off = np.array([0, 0.005, 0.010, 0.060, 0.065, 0.070])
    for name, rate, lo, hi, seed in (("gyro_dropout", 18.0, 0.85, 0.9, 4), ("gyro_past_pi", 80.0, np.pi, 4.0, 5)):
        tab = make_table(off, seed, gyr={3: rate * _axis([-1, 0.4, 0.8])})

        def big(c, m, lo=lo, hi=hi):
            th = m["theta"][m["seg"] == 2]
            assert ((th > lo) & (th <= hi)).sum() > 10 and th.max() <= hi, (th.max(), lo, hi)
        out.append(_case(name, tab, make_points(rng, n), rng.uniform(0.1, 75, n), seed, [_reaches(1, 2), big]))
    return out


def _edge_cases():
    out = []
    rng = np.random.default_rng(12)
    # offsets that are exactly double(t) / 1000 of float times
    m = 8
    tk = (4.7 * np.arange(m) + np.where(np.arange(m) > 0, 0.3, 0.0)).astype(F)
    off = tk.astype(np.float64) / np.float64(1000)
    ts, want = [], []
    for k in range(1, m):
        for v, s in ((tk[k], k - 1), (np.nextafter(tk[k], F(-np.inf)), k - 1),
                     (np.nextafter(tk[k], F(np.inf)), min(k, m - 2))):
            ts += [v] * 12
            want += [s] * 12
    # between the last two offsets, and past the last one
    mid = rng.uniform(tk[m - 2] + 0.5, tk[m - 1] - 0.5, 40).astype(F)
    past = rng.uniform(tk[m - 1] + 0.5, tk[m - 1] + 30, 40).astype(F)
    ts = np.concatenate([np.array(ts, F), mid, past])
    want = np.array(want + [m - 2] * 80)
    p = rng.permutation(ts.size)
    t, want = ts[p], want[p]

    def segs(c, mdl, want=want):
        np.testing.assert_array_equal(mdl["seg"], want[mdl["order"]])
        assert (mdl["tt"] == c["tab"][:, 0][:, None]).any(axis=1)[1:].all()   # t / 1000 hits every offset exactly
    out.append(_case("edge_exact_offsets", make_table(off, 6), make_points(rng, t.size), t, 6, [segs]))
    # two equal consecutive offsets: t = 5 ms stays in segment 0, just above it is segment 2
    off = np.array([0, 0.005, 0.005, 0.010, 0.015])
    five = F(5.0)
    t = np.concatenate([[five] * 20, [np.nextafter(five, F(10))] * 20, [np.nextafter(five, F(0))] * 20,
                        rng.uniform(0.1, 30, 240)]).astype(F)
    p = rng.permutation(t.size)
    t = t[p]

    def eq(c, mdl):
        s, tt = mdl["seg"], mdl["t"]
        assert (s[tt == five] == 0).all() and (s[tt == np.nextafter(five, F(10))] == 2).all()
        assert (s != 1).all() and (s[tt > 15.5] == 3).all()
    out.append(_case("equal_offsets", make_table(off, 7), make_points(rng, t.size), t, 7, [eq]))
    return out


def _untouched(c, m):
    assert (m["seg"] < 0).all()


def _table_cases():
    out = []
    rng = np.random.default_rng(13)
    n = 300
    for m in (0, 1, 2):
        t = rng.uniform(0.1, 100, n).astype(F)
        t[:20] = 0.0
        t[20:30] = rng.uniform(-3, -0.1, 10)
        pts, t = _shuffled(rng, make_points(rng, n), t)

        def one(c, mdl):
            assert ((mdl["seg"] == 0) == (mdl["t"] > 0)).all() and (mdl["seg"] <= 0).all()
            assert (mdl["t"] > 0).sum() > 200
        out.append(_case(f"npose_{m}", make_table(regular(m), 20 + m), pts, t, 20 + m, [_untouched if m < 2 else one]))
    # the second offset negative (an IMU sample in the gap before the scan start)
    for d, tag in ((2e-5, "20us"), (4e-3, "4ms")):
        for m in (3, 4, 5, 6, 7, 12):
            off = negative(m, d)
            t = rng.uniform(0.1, 5.0 * (m - 1) + 5, n).astype(F)
            t[:60] = 0.0
            t[60:70] = -0.0
            t[70:100] = rng.uniform(-0.999 * d * 1000, -0.001 * d * 1000, 30)   # in (-d, 0): moved from head 1
            t[100:110] = rng.uniform(-20, -d * 1000 - 0.01, 10)                # before every head: left alone
            pts, t = _shuffled(rng, make_points(rng, n), t)

            def neg(c, mdl, m=m, d=d):
                z = mdl["t"] == 0
                assert z.sum() == 70 and (mdl["seg"][z] == 1).all()
                np.testing.assert_allclose(mdl["dt"][z], d, rtol=0, atol=0)
                gap = (mdl["tt"] > -d) & (mdl["tt"] < 0)
                assert gap.sum() == 30 and (mdl["seg"][gap] == 1).all()
                assert (mdl["seg"][mdl["tt"] < -d] == -1).all() and (mdl["tt"] < -d).sum() == 10
                # the bisection k_undistort used misses the t = 0 points at these pose counts only
                missed = bool((mdl["seg_bisect"][z] != 1).any())
                assert missed == (m in (3, 6, 7, 12)), (m, missed)
                if missed:
                    assert (mdl["seg_bisect"][z] == -1).all()
            out.append(_case(f"neg_offset_{tag}_np{m}", make_table(off, 40 + m), pts, t, 40 + m, [neg]))
    return out


def _first_point_cases():
    out = []
    rng = np.random.default_rng(14)
    n = 300

    def comps(k, differs=False):
        def chk(c, mdl):
            assert len(mdl["first_heads"]) == k, mdl["first_heads"]
            assert (mdl["first_heads_old"] != mdl["first_heads"]) == differs
        return chk
    # the first sorted point is late: past four offsets, so four heads move it
    t = np.maximum(rng.uniform(0, 40, n), 17.0).astype(F)
    out.append(_case("first_late", make_table(regular(8), 60), make_points(rng, n), t, 60, [comps(4)]))
    out.append(_case("first_late_n1", make_table(regular(8), 61), make_points(rng, 1), np.array([17.0], F), 61,
                     [comps(4)]))
    out.append(_case("first_late_neg_offset", make_table(negative(8, 4e-3), 62), make_points(rng, n), t, 62,
                     [comps(6)]))
    # a table out of order: head 1 (7 ms) is not below the first point's 5 ms,
    # heads 2 (3 ms) and 0 are -- the reference tests every head on its own
    off = np.array([0, 0.007, 0.003, 0.012, 0.017])
    t = np.maximum(rng.uniform(0, 30, n), 5.0).astype(F)

    def heads(c, mdl):
        assert mdl["first_heads"] == [2, 0] and mdl["first_heads_old"] == [2]
    out.append(_case("first_skips_a_head", make_table(off, 63), make_points(rng, n), t, 63, [heads]))
    return out


def _time_cases():
    out = []
    rng = np.random.default_rng(15)
    n = 600
    t = rng.uniform(0, 100, n).astype(F)
    t[:400] = np.round(t[:400] / 4) * 4          # runs of ties
    t[400:410] = rng.uniform(-5, -0.5, 10)       # a few negative times
    t[410:420] = -2.0

    def ties(c, mdl):
        _, cnt = np.unique(mdl["t"], return_counts=True)
        assert cnt.max() >= 10 and (cnt > 1).sum() >= 20 and (mdl["t"] < 0).sum() == 20
    out.append(_case("time_ties", make_table(regular(21), 70), make_points(rng, n), t, 70, [ties]))
    # both zeros, in both input orders: a tie, so the input order stays
    for name, first in (("zeros_plus_first", 0.0), ("zeros_minus_first", -0.0)):
        t = rng.uniform(0.5, 100, 300).astype(F)
        z = np.where(np.arange(120) % 2 == 0, F(first), F(-first)).astype(F)
        t[np.sort(rng.choice(300, 120, replace=False))] = z

        def zeros(c, mdl, first=first):
            zt = mdl["t"][:120]
            assert (zt == 0).all() and (mdl["t"][120:] > 0).all()
            sign = np.signbit(zt)
            assert sign[0] == np.signbit(F(first)) and (sign[1:] != sign[:-1]).all()   # alternating: not bit-sorted
        out.append(_case(name, make_table(regular(21), 71), make_points(rng, 300), t, 71, [zeros]))
    return out


def _size_cases():
    rng = np.random.default_rng(16)
    out = []
    for n in (0, 1, 2, 255, 256, 257, 1000):
        t = rng.uniform(0.1, 100, n).astype(F)
        if n == 2:
            t = np.array([60.0, 20.0], F)
        out.append(_case(f"n_{n}", make_table(regular(21), 80), make_points(rng, n), t, 80 + n % 7))
    return out


def _nonfinite_case():
    rng = np.random.default_rng(17)
    n = 500
    pts = make_points(rng, n)
    t = np.round(rng.uniform(0.1, 100, n)).astype(F)    # ties between finite and non-finite rows
    bad = rng.choice(n, 60, replace=False)
    pts[bad[:15], 0] = np.nan
    pts[bad[15:30], 1] = np.inf
    pts[bad[30:45], 2] = -np.inf
    pts[bad[45:]] = np.nan

    def nf(c, mdl):
        assert (~np.isfinite(c["pts"]).all(axis=1)).sum() == 60
    return [_case("non_finite_rows", make_table(regular(21), 90), pts, t, 90, [nf])]


@functools.lru_cache(maxsize=None)
def cases():
    out = (_gyro_cases() + _edge_cases() + _table_cases() + _first_point_cases() + _time_cases() + _size_cases()
           + _nonfinite_case())
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return {c["name"]: c for c in out}


NAMES = tuple(cases())
# slio_scan_upload_undistort_voxel runs on these
PIPELINE_NAMES = ("n_0", "non_finite_rows", "neg_offset_4ms_np6")


@functools.lru_cache(maxsize=None)
def solved(name):
    """(case, model, (ref, scale, checked)) once per process; treat as read-only."""
    c = cases()[name]
    m = model(c)
    return c, m, reference(c, m)


def presorted(case):
    """The same points in stable time order: the device then skips its sort."""
    o = np.argsort(case["t"], kind="stable")
    return np.ascontiguousarray(case["pts"][o]), np.ascontiguousarray(case["t"][o])


def check_cases():
    """Each case reaches what it is named for (on the model alone)."""
    seen = set()
    for name in NAMES:
        c, m, _ = solved(name)
        n = c["t"].size
        assert n <= 1000 and c["tab"].shape[1] == 22
        if n:
            r = np.linalg.norm(c["pts"][np.isfinite(c["pts"]).all(axis=1)].astype(np.float64), axis=1)
            assert r.size == 0 or (r.min() >= 1.99 and r.max() <= 80.01)
        if n > 2:
            assert (np.diff(float_key(c["t"] + F(0))) < 0).any(), name   # unsorted input
        # R_LI is far from the identity, T_LI is not zero
        assert abs(c["state"][7]) < 0.96 and np.linalg.norm(c["state"][11:14]) > 0.1
        for chk in c["checks"]:
            chk(c, m)
        seen |= set(m["branch"].tolist())
    assert {0, 1, 2, -1} <= seen
    return len(NAMES)


def bisection_misses():
    """Names of the cases in which the bisection k_undistort used assigns some
    point another segment than the linear rule, or its first-point loop stops
    early (for the record of what the fix changes)."""
    out = []
    for name in NAMES:
        _, m, _ = solved(name)
        if (m["seg"] != m["seg_bisect"]).any() or m["first_heads"] != m["first_heads_old"]:
            out.append(name)
    return out
