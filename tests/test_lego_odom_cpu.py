"""CPU tests of the LeGO-LOAM scan-to-scan odometry (slio_lego_odom_*,
include/slio_frontend.h): the host export of the in-kernel step against the
numpy restatement (tests/lego_odom_model.py), the argument checks of every
new entry, and the three-sweep fixture the GPU tests share, checked on the
model alone.  No GPU.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lego_odom_model as M  # noqa: E402

from agi_lidar_slam_amd.lego import LegoParams  # noqa: E402

F = np.float32
SURF, CORNER = 0, 1


# ------------------------------------------------------------------ the fixture
SWEEP_T = 0.1                      # s per sweep
VEL = np.array([2.0, 0.5, 0.0])    # m/s, world
YAW_RATE = 0.5                     # rad/s
PARAMS = dict(Horizon_SCAN=360, ang_res_x=1.0)
# the room of small_sweep with the walls moved out by 4 m, so that the ground fills the four
# lowest rings: at 360 columns the ground is segmented every fifth column, and small_sweep's
# own walls leave fewer than 10 flat points
WALLS = ((0, -13.0, 15.0), (1, -12.0, 16.0))


def pose_at(t):
    """Constant-velocity trajectory: (rotation sensor -> world, position)."""
    a = YAW_RATE * t
    R = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    return R, VEL * t


def moving_sweep(k, seed=11, n_scan=16, horizon=360, res_y=2.0):
    """Sweep k (time [k, k + 1) * SWEEP_T) of the analytic room of
    test_lego_oracle.small_sweep (ground 1.7 m below the sensor, box walls up
    to 3 m, three pillars) in firing order, each ray cast from the pose at its
    own firing time; points in the sensor frame of that time."""
    rng = np.random.default_rng(seed + k)
    cols = np.repeat(np.arange(horizon), n_scan)
    rings = np.tile(np.arange(n_scan), horizon)
    az = -(cols + rng.uniform(-0.3, 0.3, cols.size)) * (2 * np.pi / horizon) + np.pi
    el = np.deg2rad(-15.0 + res_y * rings + rng.normal(0, 0.02, cols.size))
    ds = np.stack([np.cos(el) * np.cos(az), np.cos(el) * np.sin(az), np.sin(el)], 1)
    tt = (k + cols / horizon) * SWEEP_T
    ang = YAW_RATE * tt
    d = np.stack([np.cos(ang) * ds[:, 0] - np.sin(ang) * ds[:, 1],
                  np.sin(ang) * ds[:, 0] + np.cos(ang) * ds[:, 1], ds[:, 2]], 1)
    o = VEL[None, :] * tt[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[:, 2] < 0, (-1.7 - o[:, 2]) / d[:, 2], np.inf)
        for ax, lo, hi in WALLS:
            tw = np.where(d[:, ax] > 0, (hi - o[:, ax]) / d[:, ax], (lo - o[:, ax]) / d[:, ax])
            tw = np.where(o[:, 2] + tw * d[:, 2] < 3.0, tw, np.inf)
            t = np.minimum(t, tw)
        for cx, cy in ((3.0, 2.0), (-4.0, 5.0), (6.0, -3.0)):
            ox, oy = o[:, 0] - cx, o[:, 1] - cy
            a = d[:, 0] ** 2 + d[:, 1] ** 2
            b = 2 * (d[:, 0] * ox + d[:, 1] * oy)
            c = ox * ox + oy * oy - 0.25
            disc = b * b - 4 * a * c
            tp = (-b - np.sqrt(np.maximum(disc, 0))) / (2 * a)
            t = np.where((disc > 0) & (tp > 0), np.minimum(t, tp), t)
    ok = np.isfinite(t) & (rng.uniform(size=t.size) > 0.03)
    p = (ds[ok] * (t[ok] + rng.normal(0, 0.005, ok.sum()))[:, None]).astype(np.float32)
    return dict(x=p[:, 0].copy(), y=p[:, 1].copy(), z=p[:, 2].copy())


def true_motion(k):
    """(M, t) with p_end = M p_start + t over sweep k in the LOAM axes
    (x = sensor y, y = sensor z, z = sensor x): what transformCur encodes as
    M = Rz(rz) Rx(rx) Ry(ry), t = (tx, ty, tz)."""
    R0, o0 = pose_at(k * SWEEP_T)
    R1, o1 = pose_at((k + 1) * SWEEP_T)
    P = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    return P @ (R1.T @ R0) @ P.T, P @ (R1.T @ (o0 - o1))


def motion_of(tc):
    rx, ry, rz = (float(v) for v in tc[:3])
    Rx = np.array([[1, 0, 0], [0, math.cos(rx), -math.sin(rx)], [0, math.sin(rx), math.cos(rx)]])
    Ry = np.array([[math.cos(ry), 0, math.sin(ry)], [0, 1, 0], [-math.sin(ry), 0, math.cos(ry)]])
    Rz = np.array([[math.cos(rz), -math.sin(rz), 0], [math.sin(rz), math.cos(rz), 0], [0, 0, 1]])
    return Rz @ Rx @ Ry, np.array([float(v) for v in tc[3:]])


def motion_error(tc, k):
    Mt, tt = true_motion(k)
    Me, te = motion_of(tc)
    c = (np.trace(Me.T @ Mt) - 1.0) / 2.0
    return math.acos(max(-1.0, min(1.0, c))), float(np.linalg.norm(te - tt))


def oracle_features(oracle_mod, k, P):
    sc = moving_sweep(k)
    seg = oracle_mod.lego_project(sc["x"], sc["y"], sc["z"], P)
    f = oracle_mod.lego_features(seg, P)
    f["outlier_cloud"] = seg["outlier_cloud"]
    return f


@pytest.fixture(scope="module")
def model_sequence(oracle_mod):
    """The three sweeps through the oracle front-end and the model, once."""
    P = LegoParams(**PARAMS)
    m = M.OdomModel()
    seq = []
    for k in range(3):
        f = oracle_features(oracle_mod, k, P)
        n_last = (m.corner_last.shape[0], m.surf_last.shape[0])
        log = []
        out = m.run(f["cornerPointsSharp"], f["cornerPointsLessSharp"], f["surfPointsFlat"],
                    f["surfPointsLessFlat"], f["outlier_cloud"], None, log)
        seq.append(dict(out=out, log=log, n_last=n_last, guess=getattr(m, "guess", None)))
    return seq


def test_fixture_sanity_on_the_model(model_sequence):
    assert model_sequence[0]["out"]["inited"] == 0
    # frameCount starts at skipFrameNum = 1 (:354): the gate opens on sweeps 1, 3, 5, ...
    assert [s["out"]["published"] for s in model_sequence] == [0, 1, 0]
    for k in (1, 2):
        s = model_sequence[k]
        print(f"sweep {k}: last clouds {s['n_last']}, iters {s['out']['iters']}, rows {s['out']['rows']}")
        assert s["n_last"][0] >= 10 and s["n_last"][1] >= 100
        for kind in (SURF, CORNER):
            first = [e for e in s["log"] if e["kind"] == kind and e["it"] == 0][0]
            assert first["nsel"] >= 10, (k, kind, first["nsel"])
        r0, t0 = motion_error(s["guess"], k)
        r1, t1 = motion_error(s["out"]["transform_cur"], k)
        print(f"sweep {k}: rotation error {r0:.5f} -> {r1:.5f} rad, translation error {t0:.4f} -> {t1:.4f} m")
        assert r1 < r0 and t1 < t0


# ------------------------------------------------------------------ the step
@pytest.fixture(scope="module")
def lib():
    from agi_lidar_slam_amd import build, _lib
    build.build()
    return _lib.load()


def system(seed, scale=(1.0, 1.0, 1.0), n=300, b=0.01):
    """AtA / AtB of n random rows through the model's summation."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 4), F)
    rows[:, :3] = (rng.normal(size=(n, 3)) * np.asarray(scale)).astype(F)
    rows[:, 3] = (rng.normal(size=n) * b).astype(F)
    AtA, AtB, nsel = M.normal_equations(rows, np.ones(n, np.uint8))
    return AtA, AtB, nsel


def both_steps(kind, AtA, AtB, nsel, it, tc, deg, matP):
    """The library's step and the model's on copies; asserts they agree to
    the bit and returns the library's (tc, keep, deg, matP)."""
    from agi_lidar_slam_amd.lego import odometry_step
    tc_l, P_l = np.array(tc, F), np.array(matP, F)
    rc, keep_l, deg_l = odometry_step(kind, AtA, AtB, nsel, it, tc_l, deg, P_l)
    assert rc == 0
    tc_m, P_m = np.array(tc, F), np.array(matP, F)
    keep_m, deg_m = M.step(kind, AtA, AtB, it, tc_m, deg, P_m)
    np.testing.assert_array_equal(tc_l.view(np.uint32), tc_m.view(np.uint32))
    np.testing.assert_array_equal(P_l.view(np.uint32), P_m.view(np.uint32))
    assert (bool(keep_l), deg_l) == (bool(keep_m), deg_m)
    return tc_l, bool(keep_l), deg_l, P_l


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_step_well_conditioned(lib, kind):
    AtA, AtB, nsel = system(1 + kind, b=1.0)
    tc0 = np.array([0.01, -0.02, 0.005, 0.1, -0.05, 0.2], F)
    tc, keep, deg, P = both_steps(kind, AtA, AtB, nsel, 0, tc0, 1, np.zeros(9, F))
    assert deg == 0 and keep
    comp = (0, 2, 4) if kind == SURF else (1, 3, 5)
    other = [i for i in range(6) if i not in comp]
    assert all(tc[i] != tc0[i] for i in comp) and all(tc[i] == tc0[i] for i in other)
    np.testing.assert_allclose(P.reshape(3, 3), np.eye(3), atol=1e-5)


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_step_degenerate_projection_is_reused(lib, kind):
    AtA, AtB, nsel = system(5, scale=(1.0, 1.0, 0.01))     # one eigenvalue ~ 0.03 < 10
    tc, keep, deg, P = both_steps(kind, AtA, AtB, nsel, 0, np.zeros(6, F), 0, np.zeros(9, F))
    assert deg == 1
    # the weak direction (close to the third axis) is projected out
    assert abs(P[8]) < 1e-3 and abs(P[0] - 1) < 1e-3 and abs(P[4] - 1) < 1e-3
    AtA2, AtB2, _ = system(6, scale=(1.0, 1.0, 0.01))
    tc3, _, deg3, P3 = both_steps(kind, AtA2, AtB2, nsel, 3, tc, deg, P)
    assert deg3 == 1
    np.testing.assert_array_equal(P3, P)                    # not recomputed after iteration 0
    free, _, _, _ = both_steps(kind, AtA2, AtB2, nsel, 3, tc, 0, P)
    assert not np.array_equal(free, tc3)                    # ... and it was applied


@pytest.mark.parametrize("kind", [SURF, CORNER])
@pytest.mark.parametrize("it", [0, 3])
def test_step_singular_is_a_zero_step_and_converged(lib, kind, it):
    tc0 = np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.06], F)
    tc, keep, deg, P = both_steps(kind, np.zeros(9, F), np.array([1, 2, 3], F), 50, it, tc0, 0,
                                  np.eye(3, dtype=F).ravel())
    np.testing.assert_array_equal(tc, tc0)
    assert not keep
    # rank 1
    v = np.array([1.0, 2.0, -1.0], F)
    A1 = np.outer(v, v).astype(F).ravel() * F(40)
    both_steps(kind, A1, (v * F(3)).astype(F), 50, it, tc0, 0, np.eye(3, dtype=F).ravel())


@pytest.mark.parametrize("kind", [SURF, CORNER])
@pytest.mark.parametrize("it", [0, 3])
def test_step_nan_resets_to_zero(lib, kind, it):
    AtA, AtB, nsel = system(9)
    AtA = AtA.copy()
    AtA[4] = np.nan
    tc0 = np.array([0.01, 0.02, 0.03, 0.04, 0.05, 0.06], F)
    tc, _, _, _ = both_steps(kind, AtA, AtB, nsel, it, tc0, 0, np.eye(3, dtype=F).ravel())
    comp = (0, 2, 4) if kind == SURF else (1, 3, 5)
    for i in range(6):
        assert tc[i] == (0 if i in comp else tc0[i])
    # NaN already in transformCur (any component) is reset too
    tc0[(1, 0)[kind]] = np.nan
    tc, _, _, _ = both_steps(kind, *system(9), it, tc0, 0, np.eye(3, dtype=F).ravel())
    assert tc[(1, 0)[kind]] == 0 and not np.isnan(tc).any()


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_step_convergence_boundary(lib, kind):
    """deltaR < 0.1 deg && deltaT < 0.1 cm, both strict, on AtA = 100 I."""
    AtA = (np.eye(3) * 100).astype(F).ravel()
    r_in, r_out = 0.1 * math.pi / 180 * (1 - 1e-4), 0.1 * math.pi / 180 * (1 + 1e-4)
    t_in, t_out = 0.001 * (1 - 1e-4), 0.001 * (1 + 1e-4)
    if kind == SURF:       # X = (rx, rz, ty): deltaR over X0, X1; deltaT over X2
        cases = [((r_in / 2, r_in / 2, t_in), False), ((r_out, 0, t_in), True), ((0, r_out, 0), True),
                 ((r_in / 2, 0, t_out), True), ((0, 0, 0), False)]
    else:                  # X = (ry, tx, tz): deltaR over X0; deltaT over X1, X2
        cases = [((r_in, t_in / 2, t_in / 2), False), ((r_out, 0, 0), True), ((r_in, t_out, 0), True),
                 ((0, 0, t_out), True), ((0, 0.0008, 0.0008), True)]
    for X, want in cases:
        AtB = (np.asarray(X) * 100).astype(F)
        _, keep, _, _ = both_steps(kind, AtA, AtB, 50, 3, np.zeros(6, F), 0, np.zeros(9, F))
        assert keep == want, (X, keep)


def test_step_too_few_rows_and_bad_arguments(lib):
    from agi_lidar_slam_amd.lego import odometry_step
    AtA, AtB, _ = system(1)
    tc, P = np.full(6, 0.5, F), np.zeros(9, F)
    rc, keep, deg = odometry_step(SURF, AtA, AtB, 9, 0, tc, 0, P)
    assert (rc, keep, deg) == (1, 1, 0) and (tc == 0.5).all()
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    a, b = AtA.ctypes.data_as(fp), AtB.ctypes.data_as(fp)
    t, p = tc.ctypes.data_as(fp), P.ctypes.data_as(fp)
    d, k = C.c_int(0), C.c_int(0)
    ok = (SURF, a, b, 50, 0, t, C.byref(d), p, C.byref(k))
    for i in (1, 2, 5, 6, 7, 8):
        bad = list(ok)
        bad[i] = None
        assert lib.slio_lego_odom_step(*bad) == -1, i
    assert lib.slio_lego_odom_step(2, *ok[1:]) == -1
    assert lib.slio_lego_odom_step(SURF, a, b, 50, -1, t, C.byref(d), p, C.byref(k)) == -1
    assert b"slio_lego_odom_step" in lib.slio_last_error()
    del ip


def test_null_handle_and_argument_errors(lib):
    from agi_lidar_slam_amd import _lib as L
    p = L.SlioLegoOdomParams()
    assert lib.slio_lego_odom_params_default(None) == -1
    assert lib.slio_lego_odom_params_default(C.byref(p)) == 0
    assert (p.nearest_feature_sq_dist, p.max_iterations, p.search_period, p.skip_frame_num) == (25.0, 25, 5, 1)
    assert abs(p.scan_period - 0.1) < 1e-7
    assert lib.slio_lego_odom_enable(None, C.byref(p)) == -1
    assert lib.slio_lego_odom_reset(None) == -1
    assert lib.slio_lego_odom_run_async(None) == -1
    o, s = L.SlioLegoOdomOut(), L.SlioLegoOdomState()
    assert lib.slio_lego_odom_run(None, C.byref(o)) == -1
    assert lib.slio_lego_odom_get_last(None, None, None, None) == -1
    assert lib.slio_lego_odom_set_clouds(None, None, 0, None, 0, None, 0, None, 0) == -1
    assert lib.slio_lego_odom_set_state(None, C.byref(s)) == -1
    assert lib.slio_lego_odom_get_state(None, C.byref(s)) == -1
    assert lib.slio_lego_odom_pass(None, 0, 0, None, None, None, None, None, None, None) == -1
    assert b"null" in lib.slio_last_error()
