"""The fixture of the A-LOAM laserOdometry tests (tests/test_aloam_odom_cpu.py,
tests/test_gpu_aloam_odom.py), the model's answers to it, computed once and
shared, the crafted single-pass cases, and the assertions made on the MODEL
alone, so that the reference restatement shows what a case is there for and not
only the code under test.

The fixture: the analytic room of test_lego_odom_cpu.moving_sweep (ground
1.7 m below the sensor, walls at x -13 / 15 and y -12 / 16 up to 3 m, three
0.5 m pillars, 16 beams), horizon 600, seed 11 + k, every ray of sweep k cast
from ONE pose (A-LOAM assumes deskewed sweeps): yaw 0.04 k rad, position
(0.25 k, 0.06 k, 0); sweeps k = 0 .. 3 through aloam_model.register.
"""
import functools
import math

import numpy as np

import aloam_model as RM
import aloam_odom_model as M

F = np.float32
WALLS = ((0, -13.0, 15.0), (1, -12.0, 16.0))
PILLARS = ((3.0, 2.0), (-4.0, 5.0), (6.0, -3.0))
N_SWEEPS = 4
IDENT = ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])


def pose_of(k):
    a = 0.04 * k
    R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return R, np.array([0.25 * k, 0.06 * k, 0.0])


@functools.lru_cache(maxsize=None)
def raw_sweep(k, horizon=600, n_scan=16):
    """(n, 3) float32 in firing order, in the sensor frame of pose k."""
    rng = np.random.default_rng(11 + k)
    cols = np.repeat(np.arange(horizon), n_scan)
    rings = np.tile(np.arange(n_scan), horizon)
    az = -(cols + rng.uniform(-0.3, 0.3, cols.size)) * (2 * np.pi / horizon) + np.pi
    el = np.deg2rad(-15.0 + 2.0 * rings + rng.normal(0, 0.02, cols.size))
    ds = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    R, o = pose_of(k)
    d = ds @ R.T
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[:, 2] < 0, (-1.7 - o[2]) / d[:, 2], np.inf)
        for ax, lo, hi in WALLS:
            tw = np.where(d[:, ax] > 0, (hi - o[ax]) / d[:, ax], (lo - o[ax]) / d[:, ax])
            tw = np.where(o[2] + tw * d[:, 2] < 3.0, tw, np.inf)
            t = np.minimum(t, tw)
        for cx, cy in PILLARS:
            ox, oy = o[0] - cx, o[1] - cy
            a = d[:, 0] ** 2 + d[:, 1] ** 2
            b = 2 * (d[:, 0] * ox + d[:, 1] * oy)
            c = ox * ox + oy * oy - 0.25
            disc = b * b - 4 * a * c
            tp = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            t = np.where((disc > 0) & (tp > 0), np.minimum(t, tp), t)
    ok = np.isfinite(t) & (rng.uniform(size=t.size) > 0.03)
    return (ds[ok] * (t[ok] + rng.normal(0, 0.005, ok.sum()))[:, None]).astype(F)


@functools.lru_cache(maxsize=None)
def features(k):
    """(sharp, less_sharp, flat, less_flat) of sweep k by the registration's model."""
    w = RM.register(raw_sweep(k))
    return tuple(np.ascontiguousarray(w[n]) for n in RM.CLOUDS[1:])


def true_motion(k):
    """(q, t) of T_last_curr for sweep k >= 1: p_last = q * p_curr + t."""
    R0, o0 = pose_of(k - 1)
    _, o1 = pose_of(k)
    return [0.0, 0.0, math.sin(0.02), math.cos(0.02)], list(R0.T @ (o1 - o0))


def errors(q, t, k):
    """(rotation error in rad, translation error in m) of (q, t) against sweep k's true motion."""
    qt, tt = true_motion(k)
    d = M.qmul([-q[0], -q[1], -q[2], q[3]], qt)
    n = math.sqrt(sum(v * v for v in d))
    ang = 2 * math.atan2(math.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2) / n, abs(d[3]) / n)
    return ang, math.sqrt(sum((t[a] - tt[a]) ** 2 for a in range(3)))


@functools.lru_cache(maxsize=None)
def model_run(skip=2):
    """The four sweeps through the model: the list of its results, and the
    last clouds after each sweep."""
    od = M.Odometry(skip)
    out = []
    for k in range(N_SWEEPS):
        r = od.process(*features(k))
        r["corner_last"], r["surf_last"] = od.corner_last.copy(), od.surf_last.copy()
        out.append(r)
    return out


def check_fixture():
    """The issue's assertions on the model; returns the figures."""
    run = model_run(2)
    fig = dict(queries=[(len(features(k)[0]), len(features(k)[2])) for k in range(N_SWEEPS)],
               last=[(len(features(k)[1]), len(features(k)[3])) for k in range(N_SWEEPS)])
    g = errors(*IDENT, 1)
    e1 = errors(run[1]["q_last_curr"], run[1]["t_last_curr"], 1)
    fig["guess"], fig["sweep1"] = g, e1
    assert e1[0] < g[0] / 4 and e1[1] < g[1] / 4, (g, e1)
    fig["later"] = []
    for k in (2, 3):
        e = errors(run[k]["q_last_curr"], run[k]["t_last_curr"], k)
        fig["later"].append(e)
        assert e[0] < 0.006 and e[1] < 0.04, (k, e)
    passes = [p for r in run[1:] for p in r["passes"]]
    assert len(passes) == 6
    for p in passes:
        assert p["corner"] >= 10 and p["plane"] >= 10 and not p["few"]
        assert p["outliers"] > 0 and p["corner"] + p["plane"] - p["degenerate"] - p["outliers"] > 0
    fig["outliers"] = [p["outliers"] for p in passes]
    fig["stops"] = [M.STOPS[p["stop"]] for p in passes]
    fig["iterations"] = [p["iterations"] for p in passes]
    fig["rejected"] = sum(p["iterations"] - p["accepted"] for p in passes)
    assert any(p["stop"] != 0 and p["iterations"] < M.MAX_ITER for p in passes), fig["stops"]
    assert [r["published"] for r in run] == [1, 0, 1, 0]
    assert [r["published"] for r in model_run(1)] == [1, 1, 1, 1]
    assert [r["inited"] for r in run] == [0, 1, 1, 1]
    return fig


# ---------------------------------------------------------------- crafted single passes
def P(x, y, z, ring, rel=0.0):
    return [x, y, z, ring + rel]


def cloud(rows):
    return np.array(rows, F).reshape(-1, 4)


def _below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


@functools.lru_cache(maxsize=None)
def crafted():
    """name -> (sharp, flat, corner_last, surf_last, q, t).  Every case is
    CRAFTED; check_crafted says on the model what each one reaches."""
    E = cloud([])
    c = {}
    # the lane-stride seam: last clouds of 0, 1, 63, 64 and 65 points on a line, two per ring
    for n in (0, 1, 63, 64, 65):
        rows = [P(0.3 * i, 0.0, 0.0, i // 2) for i in range(n)]
        q = cloud([P(0.3 * (n - 1) + 0.01, 0.0, 0.0, 0), P(0.02, 0.0, 0.0, 0)])
        c[f"last{n}"] = (q, q.copy(), cloud(rows), cloud(rows), *IDENT)
    base_c = cloud([P(x, 0.0, 0.4 * r, r) for r in range(6) for x in (0.0, 1.0, 2.0)])      # 3 points on rings 0 .. 5
    base_s = cloud([P(x, y, 0.0, r) for r in range(6) for y in (float(r),) for x in (0.0, 1.0, 2.0, 3.0)])
    one = cloud([P(1.1, 0.05, 0.85, 0)])
    c["one_query"] = (one, cloud([P(1.2, 2.1, 0.05, 0)]), base_c, base_s, *IDENT)
    c["no_sharp"] = (E, cloud([P(1.2, 2.1, 0.05, 0)]), base_c, base_s, *IDENT)
    c["no_flat"] = (one, E, base_c, base_s, *IDENT)
    c["no_queries"] = (E, E, base_c, base_s, *IDENT)
    # a 1-NN tie: two last points at the same distance, the lower index wins
    tie = cloud([P(-1.0, 0.0, 0.0, 0), P(1.0, 0.0, 0.0, 0), P(0.0, 2.0, 0.0, 1), P(0.0, 2.5, 0.0, 2)])
    c["nn_tie"] = (cloud([P(0.0, 0.0, 0.0, 0)]), E, tie, E, *IDENT)
    # second point: forward and backward candidates at the same distance: forward wins
    fb = cloud([P(0.0, 1.0, 0.0, 0), P(0.0, 0.0, 0.0, 1), P(0.0, -1.0, 0.0, 2)])
    c["fwd_bwd_tie"] = (cloud([P(0.0, 0.0, 0.1, 0)]), E, fb, E, *IDENT)
    # a tie inside the backward scan: the highest j wins
    bt = cloud([P(1.0, 0.0, 0.0, 0), P(-1.0, 0.0, 0.0, 0), P(0.0, 0.0, 0.0, 1)])
    c["bwd_tie"] = (cloud([P(0.0, 0.0, 0.1, 0)]), E, bt, E, *IDENT)
    # the closest point on scan 0 and on the top scan
    top = cloud([P(0.0, 0.0, 0.0, 0), P(0.0, 1.0, 0.0, 1), P(5.0, 0.0, 0.0, 62), P(5.0, 1.0, 0.0, 63)])
    c["scan0_and_top"] = (cloud([P(0.0, 0.1, 0.0, 0), P(5.0, 0.9, 0.0, 0)]), E, top, E, *IDENT)
    # a point on cs + 3 nearer than any allowed one
    c3 = cloud([P(0.0, 0.0, 0.0, 1), P(0.0, 3.0, 0.0, 3), P(0.0, 0.5, 0.0, 4)])
    c["cs_plus_3"] = (cloud([P(0.0, 0.1, 0.0, 0)]), E, c3, E, *IDENT)
    # ids 0 and 3 only: no second point
    c["missing_ids"] = (cloud([P(0.0, 0.1, 0.0, 0)]), E, cloud([P(0.0, 0.0, 0.0, 0), P(0.0, 0.5, 0.0, 3)]), E, *IDENT)
    # 1-NN distance^2 exactly 25 (no factor) and one float below (a factor)
    gate = cloud([P(0.0, 0.0, 0.0, 0), P(0.0, 0.0, 1.0, 1), P(0.0, 50.0, 0.0, 2), P(0.0, 50.0, 0.001, 3)])
    c["gate_25"] = (cloud([P(5.0, 0.0, 0.0, 0), P(_below(5.0), 50.0, 0.0, 0)]), E, gate, E, *IDENT)
    # a second point at exactly 25: refused by the strict <
    s25 = cloud([P(0.0, 0.0, 0.0, 0), P(3.0, 4.0, 0.0, 1)])
    c["second_25"] = (cloud([P(0.0, 0.0, 0.0, 0)]), E, s25, E, *IDENT)
    # surf: minPointInd2 only, minPointInd3 only, both
    s2 = cloud([P(0.0, 0.0, 0.0, 2), P(1.0, 0.0, 0.0, 2)])
    s3 = cloud([P(0.0, 0.0, 0.0, 2), P(0.0, 1.0, 0.0, 3)])
    sb = cloud([P(0.0, 0.0, 0.0, 2), P(1.0, 0.0, 0.0, 2), P(0.0, 1.0, 0.0, 3)])
    fq = cloud([P(0.1, 0.1, 0.05, 0)])
    c["surf_ind2_only"] = (E, fq, E, s2, *IDENT)
    c["surf_ind3_only"] = (E, fq, E, s3, *IDENT)
    c["surf_both"] = (E, fq, E, sb, *IDENT)
    # coincident edge points and a collinear plane triple: degenerate
    co = cloud([P(0.0, 0.0, 0.0, 0), P(0.0, 0.0, 0.0, 1)])
    col = cloud([P(0.0, 0.0, 0.0, 2), P(1.0, 0.0, 0.0, 2), P(2.0, 0.0, 0.0, 3)])
    c["degenerate"] = (cloud([P(0.1, 0.0, 0.0, 0)]), fq, co, col, *IDENT)
    # an edge residual with s exactly 0.01 and the next double above (huber_xy)
    hub = cloud([P(0.0, 0.0, 0.0, 0), P(0.0, 0.0, 1.0, 1)])
    for name, (x, y) in zip(("huber_at", "huber_above"), huber_xy()):
        c[name] = (cloud([P(0.0, 0.0, 0.0, 0)]), E, hub, E, IDENT[0], [x, y, 0.0])
    # all factors on one plane: the damped solve stays finite
    grid = cloud([P(float(x), float(r), 0.0, r) for r in range(5) for x in range(5)])
    fl = cloud([P(0.3 + 0.7 * i, 0.4 + 0.6 * i, 0.02 * (i + 1), 0) for i in range(5)])
    c["one_plane"] = (E, fl, E, grid, *IDENT)
    # a pose that moves the queries next to other points
    c["moved"] = (one, cloud([P(1.2, 2.1, 0.05, 0)]), base_c, base_s,
                  [0.0, 0.0, math.sin(0.1), math.cos(0.1)], [0.9, 1.1, 0.3])
    return c


@functools.lru_cache(maxsize=None)
def huber_xy():
    """Two translations (x, y, 0): with the edge a = (0, 0, 0), b = (0, 0, 1) and
    the query at the origin the residual at identity rotation is (-y, x, 0)
    exactly, so s = y y + x x: the first pair gives s == 0.01 to the bit, the
    second the next double above."""
    want = (0.01, float(np.nextafter(0.01, 1.0)))
    found = [None, None]
    x = 0.06
    for _ in range(64):
        y = math.sqrt(0.01 - x * x)
        for _ in range(64):
            y = float(np.nextafter(y, 0.0))
        for _ in range(128):
            sq = (y * y + x * x) + 0.0
            for k in range(2):
                if sq == want[k] and found[k] is None:
                    found[k] = (x, y)
            y = float(np.nextafter(y, 1.0))
        if all(found):
            return found
        x = float(np.nextafter(x, 1.0))
    raise AssertionError("no translation with s == 0.01")


def check_crafted():
    """Each crafted case reaches what it is there for, on the model."""
    c = crafted()
    A = lambda name: M.associate(*c[name][:4], c[name][4], c[name][5])
    assert (A("last0") == -1).all()
    assert (A("last1")[:, 1:] == -1).all() and A("last1")[1, 0] == 0
    for n in (63, 64, 65):
        a = A(f"last{n}")
        assert a[0, 0] == n - 1 and a[1, 0] == 0, (n, a)          # the last index: lane (n - 1) % 64
    assert len(A("no_sharp")) == 1 and len(A("no_flat")) == 1 and len(A("no_queries")) == 0
    assert list(A("nn_tie")[0]) == [0, 2, -1]
    assert list(A("fwd_bwd_tie")[0]) == [1, 2, -1]
    assert list(A("bwd_tie")[0]) == [2, 1, -1]
    assert [list(r) for r in A("scan0_and_top")] == [[0, 1, -1], [3, 2, -1]]
    assert list(A("cs_plus_3")[0]) == [0, 1, -1]
    assert list(A("missing_ids")[0]) == [0, -1, -1]
    assert [list(r) for r in A("gate_25")] == [[-1, -1, -1], [2, 3, -1]]
    assert list(A("second_25")[0]) == [0, -1, -1]
    assert list(A("surf_ind2_only")[0]) == [0, 1, -1]
    assert list(A("surf_ind3_only")[0]) == [0, -1, 1]
    assert list(A("surf_both")[0]) == [0, 1, 2]
    ev = lambda name: M.evaluate(*c[name][:4], A(name), c[name][4], c[name][5])
    assert ev("surf_ind2_only")[3][:2] == [0, 0] and ev("surf_both")[3][:2] == [0, 1]
    assert ev("degenerate")[3] == [1, 1, 2, 0]
    assert ev("huber_at")[3] == [1, 0, 0, 0] and ev("huber_above")[3] == [1, 0, 0, 1]
    assert ev("huber_at")[2] == 0.5 * 0.01                            # rho = s, cost = rho / 2
    Aq, g, cost, cnt = ev("one_plane")
    assert cnt[1] == 5
    s = M.Lm(*IDENT, Aq, g, cost)
    assert s.propose() and s.pivots_ok and all(math.isfinite(v) for v in s.delta)
    assert min(Aq[M.tri(k, k)] for k in range(6)) == 0.0            # rank-deficient: x, y and yaw are free
    a0 = M.associate(*c["moved"][:4], *IDENT)
    assert (a0 != A("moved")).any()
