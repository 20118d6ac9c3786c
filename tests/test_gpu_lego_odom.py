"""GPU tests of the LeGO-LOAM scan-to-scan odometry (slio_lego_odom_*,
include/slio_frontend.h) against the numpy restatement
(tests/lego_odom_model.py): single correspondence / normal-equation passes on
injected clouds, the device-resident loop against the lockstep loop (one pass
and one host step per iteration) and the model, and the public path
(LegoFrontEnd.runFeatureAssociation) over the three-sweep fixture of
tests/test_lego_odom_cpu.py.  Everything is compared to the bit (NaN against
NaN by position).  Run on a MI355X: pytest -m gpu
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lego_odom_model as M  # noqa: E402
from test_lego_odom_cpu import PARAMS, SWEEP_T, YAW_RATE, moving_sweep  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
SURF, CORNER = 0, 1
ITERS = (0, 4, 5, 7)     # search, cached, search (weights on), cached after 5
WAVE = 64                # the search strides the last cloud by one wavefront


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.dtype.kind == "f":
        g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
        nan = np.isnan(w)
        np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
        np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan], err_msg=what)
    else:
        np.testing.assert_array_equal(got, want, err_msg=what)


@pytest.fixture(scope="module")
def fe():
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoParams
    h = LegoFrontEnd(LegoParams())       # 16 x 1800: ring caps 192 sharp / 384 flat
    h.enable_odometry()
    yield h
    h.close()


# ------------------------------------------------------------------ injected clouds
def last_cloud(rng, n, rings=tuple(range(16)), box=3.0):
    """n points in a box, ring numbers (with a sweep-time fraction) non-decreasing."""
    r = np.sort(rng.choice(np.asarray(rings), n))
    p = rng.uniform(-box, box, (n, 3))
    return np.column_stack([p, r + rng.uniform(0, 0.09, n)]).astype(F)


def queries_near(rng, last, n, noise=0.05, idx=None):
    if n == 0:
        return np.zeros((0, 4), F)
    idx = rng.integers(0, last.shape[0], n) if idx is None else np.resize(np.asarray(idx), n)
    q = last[idx].astype(np.float64)
    q[:, :3] += rng.normal(0, noise, (n, 3))
    q[:, 3] = np.floor(q[:, 3]) + rng.uniform(0, 0.0999, n)
    return q.astype(F)


def run_passes(fe, kind, qry, last, iters=ITERS):
    """The four passes on the device and in the model, caches in step."""
    other = np.zeros((0, 4), F)
    big = last_cloud(np.random.default_rng(0), 120)
    if kind == SURF:
        rc = fe.odometry_set_clouds(other, qry, big, last)
    else:
        rc = fe.odometry_set_clouds(qry, other, last, big)
    assert rc == 0
    n = qry.shape[0]
    ind = np.full((3, n), -1, np.int32)
    res = []
    for it in iters:
        tc = (np.array([0.004, -0.006, 0.005, 0.03, -0.02, 0.04]) * (1 + 0.5 * it)).astype(F)
        got = fe.odometry_pass(kind, it, tc, n)
        before = ind.copy()
        coeff, sel = M.correspond(kind, it, qry, last, tc, ind)
        rows = M.jacobian_rows(kind, qry, coeff, sel, tc)
        AtA, AtB, nsel = M.normal_equations(rows, sel)
        same_bits(got["ind"], ind, f"ind it={it}")
        same_bits(got["sel"], sel, f"sel it={it}")
        same_bits(got["coeff"], coeff, f"coeff it={it}")
        same_bits(got["AtA"], AtA, f"AtA it={it}")
        same_bits(got["AtB"], AtB, f"AtB it={it}")
        assert got["nsel"] == nsel
        if it % 5:
            np.testing.assert_array_equal(ind, before)   # cached, on both sides
        res.append(dict(it=it, ind=ind.copy(), sel=sel, nsel=nsel, coeff=coeff, AtA=AtA))
    return res


@pytest.mark.parametrize("kind", [SURF, CORNER])
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, "cap"])
def test_pass_query_counts(fe, kind, nq):
    rng = np.random.default_rng(100 + kind)
    nq = (384, 192)[kind] if nq == "cap" else nq
    last = last_cloud(rng, 200)                      # more than three wavefront tiles
    res = run_passes(fe, kind, queries_near(rng, last, nq), last)
    if nq >= 63:
        assert res[0]["nsel"] > 0


# the tile is the wavefront's stride of 64: one below, at and above it, more than three tiles,
# and clouds of a few thousand points (the corner cloud of a 16-ring handle holds 1920)
SIZES = [(k, n) for n in (100, 101, WAVE - 1, WAVE, WAVE + 1, 3 * WAVE + 9) for k in (SURF, CORNER)] + \
        [(SURF, 4200), (CORNER, 1920)]


@pytest.mark.parametrize("kind,nl", SIZES)
def test_pass_last_cloud_sizes(fe, kind, nl):
    rng = np.random.default_rng(200 + kind + nl)
    last = last_cloud(rng, nl, box=3.0 if nl < 1000 else 8.0)
    idx = rng.integers(0, nl, 65)
    edges = [i for i in (0, nl - 1, WAVE - 1, WAVE, 2 * WAVE - 1, 2 * WAVE) if i < nl]
    idx[:len(edges)] = edges                 # closest points on both sides of the stride boundaries
    res = run_passes(fe, kind, queries_near(rng, last, 65, noise=0.02, idx=idx), last)
    assert res[0]["nsel"] > 0 and (res[0]["ind"][0] >= 0).all()
    assert (res[0]["ind"][0][:len(edges)] == edges).all()


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_pass_empty_rings_and_gaps(fe, kind):
    """Rings {0, 1, 5, 9, 10}: both scans stop at a gap above 2 (the `break`s)."""
    rng = np.random.default_rng(300 + kind)
    last = last_cloud(rng, 150, rings=(0, 1, 5, 9, 10), box=1.5)
    res = run_passes(fe, kind, queries_near(rng, last, 80), last)
    ring = last[:, 3].astype(int)
    i1, i2 = res[0]["ind"][0], res[0]["ind"][1]
    assert (i1 >= 0).all()
    ok = i2 >= 0
    assert ok.any() and (np.abs(ring[i2[ok]] - ring[i1[ok]]) <= 2).all()
    if kind == CORNER:
        assert (ring[i1] == 5).any() and (~ok)[ring[i1] == 5].all()   # ring 5 has no ring within 2


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_pass_closest_at_the_ends_and_beyond_the_feature_count(fe, kind):
    rng = np.random.default_rng(400 + kind)
    last = last_cloud(rng, 180)
    idx = [0, 179, 0, 179, 150, 120, 90, 60, 30, 10, 11, 12]   # 12 queries: forward scans end at j < 12
    q = queries_near(rng, last, 12, noise=1e-3, idx=idx)
    res = run_passes(fe, kind, q, last)
    i1 = res[0]["ind"][0]
    np.testing.assert_array_equal(i1, idx)
    far = i1 >= 12                                               # forward scan empty: only lower indices
    assert (res[0]["ind"][1][far] < i1[far]).all() and (res[0]["ind"][2][far] < i1[far]).all()


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_pass_ties(fe, kind):
    """Exact duplicates: 1-NN ties (lower index), ties between the directions
    (forward wins), within a direction (forward: lowest j, backward: highest)."""
    rng = np.random.default_rng(500 + kind)
    last = last_cloud(rng, 160, box=2.0)
    ring = last[:, 3].astype(int)
    for r in (3, 6, 9):
        k = np.nonzero(ring == r)[0]
        c = k[len(k) // 2]
        last[c + 1, :3] = last[c, :3]                   # a 1-NN tie inside ring r
        lo, hi = np.nonzero(ring == r - 1)[0], np.nonzero(ring == r + 1)[0]
        p = last[c, :3] + F(0.25)
        last[lo[-1], :3] = last[lo[-2], :3] = p          # equal candidates below (backward: highest j)
        last[hi[0], :3] = last[hi[1], :3] = p            # ... and above (forward: lowest j; beats backward)
        k2 = k[k != c][:2]
        last[k2[0], :3] = last[k[-1], :3] = last[c, :3] - F(0.125)   # same-ring tie across directions
    idx = [k[len(k) // 2] for k in (np.nonzero(ring == r)[0] for r in (3, 6, 9))]
    q = last[np.resize(idx, 200)].copy()
    q[:, 3] = np.floor(q[:, 3])                          # s = 0: the query stays where it is
    q[3:, :3] += rng.normal(0, 0.3, (197, 3)).astype(F)
    res = run_passes(fe, kind, q, last)
    np.testing.assert_array_equal(res[0]["ind"][0][:3], idx)    # the lower index of each duplicate pair


@pytest.mark.parametrize("kind", [SURF, CORNER])
def test_pass_gate(fe, kind):
    """A query beyond 5 m of everything, and one at squared distance exactly
    25 (rejected: the test is `<`)."""
    rng = np.random.default_rng(600 + kind)
    last = last_cloud(rng, 130)
    last[40, :3] = (100.0, 100.0, 100.0)
    q = queries_near(rng, last, 70)
    q[0] = (103.0, 104.0, 100.0, 4.0)     # 9 + 16 + 0 == 25
    q[1] = (500.0, 500.0, 500.0, 2.0)
    q[2] = (102.5, 104.0, 100.0, 4.0)     # just inside
    res = run_passes(fe, kind, q, last, iters=(0, 5))
    for r in res:
        assert r["ind"][0][0] == -1 and r["ind"][0][1] == -1 and r["ind"][0][2] == 40
        assert not r["sel"][0] and not r["sel"][1]


def tripod_slots(last):
    """Indices (closest, same ring, ring below) that the BACKWARD scans reach
    from the closest point, whatever the query count: the second and the first
    point of ring 7 and the last point of ring 6."""
    ring = last[:, 3].astype(int)
    k7 = np.nonzero(ring == 7)[0]
    assert k7.size >= 2 and ring[k7[0] - 1] == 6
    return k7[1], k7[0], k7[0] - 1


def test_pass_zero_distance(fe):
    """A query on its plane / on its line: d == 0, not selected."""
    rng = np.random.default_rng(700)
    last = last_cloud(rng, 140)
    a, b, c = tripod_slots(last)
    last[a, :3], last[b, :3], last[c, :3] = (50.0, 50.0, 1.0), (51.0, 50.0, 1.0), (50.0, 51.0, 1.0)
    q = queries_near(rng, last, 66)
    q[5] = (50.125, 50.125, 1.0, 7.0)
    res = run_passes(fe, SURF, q, last, iters=(0, 5))
    assert tuple(res[0]["ind"][:, 5]) == (a, b, c) and not res[0]["sel"][5] and not res[1]["sel"][5]
    last[b, :3] = last[a, :3] + F(30.0)
    last[c, :3] = (52.0, 50.0, 1.0)
    q[5] = (50.5, 50.0, 1.0, 7.0)
    res = run_passes(fe, CORNER, q, last, iters=(0, 5))
    assert tuple(res[0]["ind"][:2, 5]) == (a, c) and not res[0]["sel"][5] and not res[1]["sel"][5]


def test_pass_collinear_tripod_nan(fe):
    """ps == 0: NaN coefficients, selected while s = 1 (iterations 0-4), NaN
    normal equations; from iteration 5 s is NaN and the row is dropped."""
    rng = np.random.default_rng(800)
    last = last_cloud(rng, 140)
    a, b, c = tripod_slots(last)
    last[a, :3], last[b, :3], last[c, :3] = (50.0, 50.0, 1.0), (51.0, 50.0, 1.0), (52.0, 50.0, 1.0)
    q = queries_near(rng, last, 66)
    q[5] = (50.125, 50.25, 1.0, 7.0)
    res = run_passes(fe, SURF, q, last)
    assert res[0]["sel"][5] and np.isnan(res[0]["coeff"][5]).all() and np.isnan(res[0]["AtA"]).all()
    assert res[1]["sel"][5] and not res[2]["sel"][5] and not res[3]["sel"][5]
    assert not np.isnan(res[2]["AtA"]).any()


def test_pass_cached_indices_survive_a_moved_query_and_the_other_kind(fe):
    """iter_count 7 after a pass at 5 reuses the indices of 5 although the
    transform at 7 moves most queries next to other points (a search at 7 would
    answer differently), and a pass of the other kind in between does not
    touch them: each kind keeps its own pointSearch*Ind arrays."""
    rng = np.random.default_rng(850)
    cl, sl = last_cloud(rng, 200), last_cloud(rng, 220)
    qc, qs = queries_near(rng, cl, 100, noise=0.01), queries_near(rng, sl, 120, noise=0.01)
    for q in (qc, qs):
        q[:, 3] = np.floor(q[:, 3]) + F(0.0995)          # s ~ 1: the whole transform applies
    assert fe.odometry_set_clouds(qc, qs, cl, sl) == 0
    tc5 = np.zeros(6, F)
    tc7 = np.array([0.0, 0.0, 0.0, 1.5, -1.0, 0.5], F)   # moves every query by ~1.9 m
    cache = {}
    for kind, q, last in ((SURF, qs, sl), (CORNER, qc, cl)):
        ind = np.full((3, q.shape[0]), -1, np.int32)
        M.correspond(kind, 5, q, last, tc5, ind)
        same_bits(fe.odometry_pass(kind, 5, tc5, q.shape[0])["ind"], ind, f"ind at 5, kind {kind}")
        cache[kind] = ind
    for kind, q, last in ((SURF, qs, sl), (CORNER, qc, cl)):
        searched = np.full((3, q.shape[0]), -1, np.int32)
        M.correspond(kind, 5, q, last, tc7, searched)                  # what a search at tc7 would find
        assert (searched[0] != cache[kind][0]).mean() > 0.5
        ind = cache[kind].copy()
        coeff, sel = M.correspond(kind, 7, q, last, tc7, ind)
        np.testing.assert_array_equal(ind, cache[kind])
        got = fe.odometry_pass(kind, 7, tc7, q.shape[0])
        same_bits(got["ind"], cache[kind], f"cached ind at 7, kind {kind}")
        same_bits(got["sel"], sel, f"sel at 7, kind {kind}")
        same_bits(got["coeff"], coeff, f"coeff at 7, kind {kind}")


def test_set_clouds_rejects_decreasing_rings_and_run_needs_a_sweep():
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoParams
    from agi_lidar_slam_amd import _lib as L
    import ctypes as C
    h = LegoFrontEnd(LegoParams(**PARAMS))
    try:
        assert h.lib.slio_lego_odom_run(h.h, None) == -5            # not enabled: SLIO_ESTATE
        h.enable_odometry()
        o = L.SlioLegoOdomOut()
        assert h.lib.slio_lego_odom_run(h.h, C.byref(o)) == -5      # no sweep: an error, not a wait
        rng = np.random.default_rng(1)
        last = last_cloud(rng, 120)
        bad = last.copy()
        bad[60, 3] = np.floor(bad[59, 3]) - 1 + F(0.05)      # one ring back in the middle
        e = np.zeros((0, 4), F)
        assert h.odometry_set_clouds(e, e, bad, last) == -1
        assert h.odometry_set_clouds(e, e, last, bad) == -1
        assert b"intensity" in h.lib.slio_last_error()
        assert h.odometry_set_clouds(e, e, last, last) == 0
        assert h.lib.slio_lego_odom_run(h.h, C.byref(o)) == 0
        assert h.lib.slio_lego_odom_run(h.h, C.byref(o)) == -5      # consumed
    finally:
        h.close()


# ------------------------------------------------------------------ the loop
def lockstep(fe, n_flat, n_sharp, st):
    """updateTransformation on the host from the device's current state."""
    tc, P, deg = st["transform_cur"].copy(), st["mat_p"].copy(), st["is_degenerate"]
    out = dict(iters=[0, 0], rows=[0, 0], degenerate=[0, 0])
    if st["n_corner_last"] < 10 or st["n_surf_last"] < 100:
        return tc, out
    for kind, n in ((SURF, n_flat), (CORNER, n_sharp)):
        i, r, d0, deg = fe.odometry_lockstep(kind, n, tc, deg, P)
        out["iters"][kind], out["rows"][kind], out["degenerate"][kind] = i, r, d0
    return tc, out


def check_out(got, want, what):
    for k in ("iters", "rows", "degenerate"):
        assert list(got[k]) == list(want[k]), (what, k, got[k], want[k])


def injected_loop(fe, sharp, flat, corner_last, surf_last, tc0):
    fe.reset_odometry()
    assert fe.odometry_set_clouds(sharp, flat, corner_last, surf_last) == 0
    fe.set_odometry_state(transform_cur=tc0, transform_sum=[0.01, -0.02, 0.03, 1.0, 2.0, 3.0])
    assert fe.odometry_state()["frame_count"] == 1          # the constructor's frameCount = skipFrameNum
    m = M.OdomModel()
    m.inited, m.corner_last, m.surf_last = True, corner_last, surf_last
    m.transformCur = np.array(tc0, F)
    m.transformSum = np.array([0.01, -0.02, 0.03, 1.0, 2.0, 3.0], F)
    e = np.zeros((0, 4), F)
    want = m.run(sharp, e, flat, e, e)
    tc_l, out_l = lockstep(fe, flat.shape[0], sharp.shape[0], fe.odometry_state())
    got = fe.odometry_run()
    check_out(got, want, "model")
    check_out(got, out_l, "lockstep")
    same_bits(got["transform_cur"], want["transform_cur"], "transformCur vs model")
    same_bits(got["transform_cur"], tc_l, "transformCur vs lockstep")
    same_bits(got["transform_sum"], want["transform_sum"], "transformSum")
    assert got["published"] == want["published"] == 1 and got["inited"] == 1
    assert (got["n_corner_last"], got["n_surf_last"]) == (0, 0)      # the (empty) less clouds swapped in
    return got


def test_loop_early_return_on_small_last_clouds(fe):
    rng = np.random.default_rng(900)
    cl, sl = last_cloud(rng, 200), last_cloud(rng, 200)
    tc0 = [0.001, 0.002, -0.001, 0.01, 0.02, -0.01]
    for c, s in ((cl[:9], sl), (cl, sl[:99])):
        got = injected_loop(fe, queries_near(rng, cl, 40), queries_near(rng, sl, 40), c, s, tc0)
        assert got["iters"] == [0, 0]
        same_bits(got["transform_cur"], np.array(tc0, F))


def test_loop_fewer_than_ten_rows_at_every_iteration(fe):
    rng = np.random.default_rng(901)
    cl, sl = last_cloud(rng, 150), last_cloud(rng, 150)
    sharp, flat = queries_near(rng, cl, 30), queries_near(rng, sl, 30)
    sharp[4:, :3] += F(40.0)          # all but four queries beyond the gate
    flat[4:, :3] += F(40.0)
    tc0 = [0.001, 0.002, -0.001, 0.01, 0.02, -0.01]
    got = injected_loop(fe, sharp, flat, cl, sl, tc0)
    assert got["iters"] == [25, 25] and max(got["rows"]) < 10
    same_bits(got["transform_cur"], np.array(tc0, F))


def test_loop_converges_at_iteration_zero(fe):
    rng = np.random.default_rng(902)
    cl, sl = last_cloud(rng, 400, box=4.0), last_cloud(rng, 400, box=4.0)
    sharp = queries_near(rng, cl, 192, noise=1e-4, idx=rng.permutation(400)[:192])
    flat = queries_near(rng, sl, 384, noise=1e-4, idx=rng.permutation(400)[:384])
    got = injected_loop(fe, sharp, flat, cl, sl, np.zeros(6))
    assert got["iters"] == [1, 1] and min(got["rows"]) >= 10


# ------------------------------------------------------------------ the public path
def imu_for_fixture():
    from agi_lidar_slam_amd.lego import LegoImu
    t = np.arange(-0.05, 3 * SWEEP_T + 0.1, 0.01)
    msgs = dict(time=t, roll=0.01 * np.sin(3 * t), pitch=0.015 * np.cos(2 * t), yaw=YAW_RATE * t,
                acc=np.column_stack([0.2 + 0 * t, 0.1 * np.cos(t), 9.81 + 0.05 * np.sin(t)]),
                gyro=np.column_stack([0.03 * np.cos(3 * t), -0.03 * np.sin(2 * t), YAW_RATE + 0 * t]))
    return LegoImu(), msgs


def feed(imu, msgs, lo, hi):
    for k in np.nonzero((msgs["time"] > lo) & (msgs["time"] <= hi))[0]:
        imu.imuHandler(float(msgs["time"][k]), float(msgs["roll"][k]), float(msgs["pitch"][k]),
                       float(msgs["yaw"][k]), msgs["acc"][k], msgs["gyro"][k])


def run_sequence(fe, with_imu, model=None, do_lockstep=False):
    """Three sweeps through runFeatureAssociation; with `model`, every sweep
    is checked against it (fed with the device's own feature clouds)."""
    imu, msgs = imu_for_fixture() if with_imu else (None, None)
    seen, t_fed = [], -1.0
    for k in range(3):
        sc = moving_sweep(k)
        t0 = k * SWEEP_T
        if imu is not None:
            feed(imu, msgs, t_fed, t0 + SWEEP_T + 0.03)
            t_fed = t0 + SWEEP_T + 0.03
        if do_lockstep and k > 0:
            f = fe.cloudHandler(sc["x"], sc["y"], sc["z"], imu, t0)
            st = fe.odometry_state()
            tc_l, out_l = lockstep(fe, f["surfPointsFlat"].shape[0], f["cornerPointsSharp"].shape[0], st)
            out = fe.odometry_run()
            out["features"] = f
            check_out(out, out_l, f"lockstep sweep {k}")
            same_bits(out["transform_cur"], tc_l, f"transformCur vs lockstep, sweep {k}")
        else:
            out = fe.runFeatureAssociation(sc["x"], sc["y"], sc["z"], imu, t0)
        f = out["features"]
        outlier = fe.seg_info()["outlier_cloud"]
        last = fe.last_clouds()
        if model is not None:
            want = model.run(f["cornerPointsSharp"], f["cornerPointsLessSharp"], f["surfPointsFlat"],
                             f["surfPointsLessFlat"], outlier, f["imu_out"] if with_imu else None)
            assert out["inited"] == want["inited"] == (1 if k else 0)
            check_out(out, want, f"model sweep {k}")
            same_bits(out["transform_cur"], want["transform_cur"], f"transformCur sweep {k}")
            same_bits(out["transform_sum"], want["transform_sum"], f"transformSum sweep {k}")
            # frameCount starts at skipFrameNum (1): sweep 1 publishes, sweep 2 does not
            assert out["published"] == want["published"] == (1 if k == 1 else 0)
            same_bits(last["laserCloudCornerLast"], model.corner_last, f"corner last sweep {k}")
            same_bits(last["laserCloudSurfLast"], model.surf_last, f"surf last sweep {k}")
            same_bits(last["outlierCloudLast"], model.outlier_last, f"outlier last sweep {k}")
            if k:
                assert min(want["rows"]) >= 10
        seen.append(dict(out={k_: v for k_, v in out.items() if k_ != "features"}, last=last, features=f))
    return seen


@pytest.fixture(scope="module")
def fe360():
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoParams
    h = LegoFrontEnd(LegoParams(**PARAMS))
    h.enable_odometry()
    yield h
    h.close()


def test_fixture_loop_against_lockstep_and_model(fe360):
    fe360.reset_odometry()
    run_sequence(fe360, False, M.OdomModel(), do_lockstep=True)


@pytest.mark.parametrize("with_imu", [False, True])
def test_sequence_through_the_public_path(fe360, with_imu):
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoParams
    fe360.reset_odometry()
    first = run_sequence(fe360, with_imu, M.OdomModel())
    assert first[0]["out"]["iters"] == [0, 0] and first[1]["out"]["iters"][1] > 0
    q, p = fe360.odometry_pose()
    qm, pm = M.odometry_pose(first[2]["out"]["transform_sum"])
    np.testing.assert_array_equal(q, qm)
    np.testing.assert_array_equal(p, pm)
    # after a reset the sequence repeats bit for bit (and nothing published is left)
    fe360.reset_odometry()
    assert all(v.shape == (0, 4) for v in fe360.last_clouds().values())
    assert fe360.odometry_state()["frame_count"] == 1
    again = run_sequence(fe360, with_imu)
    for a, b in zip(first, again):
        for k in ("transform_cur", "transform_sum"):
            same_bits(a["out"][k], b["out"][k], k)
        assert a["out"]["iters"] == b["out"]["iters"] and a["out"]["rows"] == b["out"]["rows"]
        for k in a["last"]:
            same_bits(a["last"][k], b["last"][k], k)
    # a handle without the odometry returns what cloudHandler returns, sweep after sweep
    plain = LegoFrontEnd(LegoParams(**PARAMS))
    try:
        imu, msgs = imu_for_fixture() if with_imu else (None, None)
        t_fed = -1.0
        for k in range(3):
            sc = moving_sweep(k)
            if imu is not None:
                feed(imu, msgs, t_fed, k * SWEEP_T + SWEEP_T + 0.03)
                t_fed = k * SWEEP_T + SWEEP_T + 0.03
            f = plain.cloudHandler(sc["x"], sc["y"], sc["z"], imu, k * SWEEP_T)
            for name, v in f.items():
                if name == "imu_out":
                    for n2, v2 in v.items():
                        np.testing.assert_array_equal(v2, first[k]["features"]["imu_out"][n2], err_msg=n2)
                else:
                    same_bits(v, first[k]["features"][name], name)
    finally:
        plain.close()
