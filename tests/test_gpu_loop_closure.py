"""GPU tests of the loop closure on the device (mapOptmization.cpp
performLoopClosure :725-826): slio_s2m_loop_cloud against the oracle's
transform and VoxelGrid bit for bit, slio_icp_correspond against a brute-force
float32 restatement (tests/icp_model.py) -- indices equal, distances and the
working cloud bit-equal, the fp64 sums within the bound any summation order
satisfies -- the lockstep and whole ICP runs, and perform_loop_closure end to
end."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

ULP1 = 2.0 ** -23
EINVAL, ECAPACITY = -1, -4


@pytest.fixture(scope="module")
def L():
    from agi_lidar_slam_amd import build, _lib
    build.build()
    return _lib


@pytest.fixture(scope="module")
def fix():
    """The fixture and what the CPU restatement makes of it, computed once and
    never modified.  The no-tie condition is asserted here: a redraw that
    breaks it fails loudly."""
    tgt, src = M.fixture()
    runs = {md: (M.icp_run(src, tgt, md), M.icp_run(src, tgt, md, dtype=np.float32)) for md in (30, 0.5)}
    for md, (r64, _) in runs.items():
        assert not r64["ties"], f"exact nearest / second-nearest tie in a pass at max_dist {md}"
    r = runs[30][0]
    assert (r["iterations"], r["state"]) == (12, M.TRANSFORM) and abs(r["fitness"] - 0.0746) < 5e-5
    r = runs[0.5][0]
    assert (r["iterations"], r["state"], r["gated_first"]) == (15, M.TRANSFORM, 61)
    return tgt, src, runs


def mk(L, max_points=4000, cell=1.0):
    lib = L.load()
    p = L.SlioParams()
    L.check(lib.slio_params_default(C.byref(p)), "params")
    p.device, p.max_points, p.grid_cell = 0, max_points, cell
    h = C.c_void_p()
    L.check(lib.slio_create(C.byref(h), C.byref(p)), "create")
    return h


def upload(L, fn, h, pts):
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    L.check(fn(h, L.fptr(x), L.fptr(y), L.fptr(z), pts.shape[0]), fn.__name__)


def correspond(L, h, T, from_scan, max_dist):
    T = np.ascontiguousarray(np.asarray(T, np.float32).reshape(16))
    sums, n = np.zeros(16), C.c_int64(-1)
    L.check(L.load().slio_icp_correspond(h, L.fptr(T), from_scan, float(max_dist), L.dptr(sums), C.byref(n)),
            "icp_correspond")
    return sums, n.value


def working(L, h):
    lib = L.load()
    n = C.c_int64()
    assert lib.slio_icp_get_working(h, None, None, None, 0, C.byref(n)) in (0, ECAPACITY)
    cap = max(n.value, 1)
    x, y, z = (np.zeros(cap, np.float32) for _ in range(3))
    L.check(lib.slio_icp_get_working(h, L.fptr(x), L.fptr(y), L.fptr(z), cap, C.byref(n)), "get_working")
    return np.stack([x, y, z], 1)[:n.value]


def correspondences(L, h, n):
    idx, sqd = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float32)
    L.check(L.load().slio_icp_get_correspondences(h, L.iptr(idx), L.fptr(sqd)), "get_correspondences")
    return idx[:n], sqd[:n]


def check_pass(L, h, tgt, base, T, from_scan, max_dist, tag=""):
    """One device pass against the restatement; base = the cloud T applies to
    (the scan, or the previous working cloud).  Returns the device's sums,
    count and working cloud."""
    want = M.transform32(T, base)
    idx_ref, sqd_ref, tie = M.nearest32(want, tgt)
    assert not tie.any(), "the reference has an exact nearest tie: indices are not comparable"
    terms, ok = M.sum_terms(want, tgt, idx_ref, sqd_ref, max_dist)
    sums, ncorr = correspond(L, h, T, from_scan, max_dist)
    work = working(L, h)
    assert work.shape == want.shape
    assert work.tobytes() == want.tobytes(), "working cloud differs"
    idx, sqd = correspondences(L, h, want.shape[0])
    assert sqd.tobytes() == sqd_ref.tobytes(), "squared distances differ"
    np.testing.assert_array_equal(idx, np.where(ok, idx_ref, -1))
    assert ncorr == int(ok.sum())
    exact, bound = M.fsums(terms), M.sum_bounds(terms)
    err = np.abs(sums - exact)
    print(f"{tag} n={want.shape[0]} ncorr={ncorr} max sum err / bound = "
          f"{(err / np.maximum(bound, 1e-300)).max() if ncorr else 0.0:.3f}")
    assert (err <= bound).all(), (err, bound)
    return sums, ncorr, work


T_STEP = np.eye(4, dtype=np.float32)
T_STEP[:3, :3] = M.rot_zyx(-0.02, 0.01, 0.03).astype(np.float32)
T_STEP[:3, 3] = [0.11, -0.07, 0.02]


def test_one_pass_exact(L, fix):
    tgt, src, _ = fix
    h = mk(L)
    try:
        lib = L.load()
        upload(L, lib.slio_map_upload, h, tgt)
        upload(L, lib.slio_scan_upload, h, src)
        for md in (30, 0.5):
            s1, n1, work = check_pass(L, h, tgt, src, np.eye(4), 1, md, f"identity max_dist {md}")
            if md == 0.5:
                assert src.shape[0] - n1 == 61
            s2, n2, _ = check_pass(L, h, tgt, src, np.eye(4), 1, md, "again")
            assert s1.tobytes() == s2.tobytes() and n1 == n2, "two identical calls differ"
        # the incremental transform: T applies to the working cloud, in place
        _, _, work2 = check_pass(L, h, tgt, work, T_STEP, 0, 30, "T, from_scan = 0")
        check_pass(L, h, tgt, work2, T_STEP, 0, 0.5, "T again")
        # a non-finite source point has no correspondence and leaves the sums alone
        bad = src.copy()
        bad[5, 1] = np.nan
        bad[77, 0] = np.inf
        upload(L, lib.slio_scan_upload, h, bad)
        sums, n = correspond(L, h, np.eye(4), 1, 30)
        idx, sqd = correspondences(L, h, bad.shape[0])
        assert n == bad.shape[0] - 2 and idx[5] == -1 and idx[77] == -1 and np.isinf(sqd[5]) and np.isinf(sqd[77])
        assert np.isfinite(sums).all()
        # argument and state errors on a live handle
        s = np.zeros(16)
        k = C.c_int64()
        T = np.eye(4, dtype=np.float32).reshape(16)
        assert lib.slio_icp_correspond(h, L.fptr(T), 2, 1.0, L.dptr(s), C.byref(k)) == EINVAL
        assert lib.slio_icp_correspond(h, L.fptr(T), 1, -1.0, L.dptr(s), C.byref(k)) == EINVAL
        assert lib.slio_icp_correspond(h, L.fptr(T), 1, math.nan, L.dptr(s), C.byref(k)) == EINVAL
        assert lib.slio_icp_correspond(h, None, 1, 1.0, L.dptr(s), C.byref(k)) == EINVAL
    finally:
        L.load().slio_destroy(h)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_reduction_edges(L, fix, n):
    tgt, src, _ = fix
    h = mk(L)
    try:
        lib = L.load()
        upload(L, lib.slio_map_upload, h, tgt)
        upload(L, lib.slio_scan_upload, h, src[:n])
        for md in (30, 0.5):
            sums, ncorr, _ = check_pass(L, h, tgt, src[:n], np.eye(4), 1, md, f"n {n} max_dist {md}")
            if n == 0:
                assert ncorr == 0 and not sums.any()
        if n:
            check_pass(L, h, tgt, M.transform32(np.eye(4), src[:n]), T_STEP, 0, 30, f"n {n} step")
    finally:
        L.load().slio_destroy(h)


def test_agrees_with_search_pass(L, fix):
    """Entry 0 of slio_get_neighbors for the same world points (a kNN pass at
    the identity pose: slio_s2m_coeffs with a zero transform) equals the ICP
    pass's index and distance -- also on a target with 40 duplicated points,
    where only the shared tie rule makes the index unique."""
    tgt, src, _ = fix
    rng = np.random.default_rng(5)
    dup = np.concatenate([tgt, tgt[rng.choice(tgt.shape[0], 40, replace=False)]])
    lib = L.load()
    for target in (tgt, dup):
        h, h2 = mk(L), mk(L)
        try:
            upload(L, lib.slio_map_upload, h, target)
            upload(L, lib.slio_scan_upload, h, src)
            correspond(L, h, np.eye(4), 1, 30)
            _, ncorr = correspond(L, h, T_STEP, 0, 30)
            work = working(L, h)
            idx, sqd = correspondences(L, h, work.shape[0])
            assert ncorr == work.shape[0]
            upload(L, lib.slio_map_upload, h2, target)
            upload(L, lib.slio_scan_upload, h2, work)
            L.check(lib.slio_s2m_coeffs(h2, 1, L.fptr(np.zeros(6, np.float32)), None), "kNN pass")
            nidx = np.zeros((work.shape[0], 5), np.int32)
            nsqd = np.zeros((work.shape[0], 5), np.float32)
            L.check(lib.slio_get_neighbors(h2, L.iptr(nidx), L.fptr(nsqd), None), "get_neighbors")
            np.testing.assert_array_equal(idx, nidx[:, 0])
            assert sqd.tobytes() == np.ascontiguousarray(nsqd[:, 0]).tobytes()
            if target is dup:
                # the duplicates are exercised: some query's nearest is a duplicated point
                _, sref, tie = M.nearest32(work, dup)
                assert tie.any() and sref.tobytes() == sqd.tobytes()
        finally:
            lib.slio_destroy(h)
            lib.slio_destroy(h2)


def test_far_start(L, fix):
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    tgt, src, _ = fix
    lib = L.load()
    h = mk(L)
    try:
        upload(L, lib.slio_map_upload, h, tgt)
        far_src = (src + np.float32([12, -9, 0])).astype(np.float32)
        upload(L, lib.slio_scan_upload, h, far_src)
        _, ncorr, work = check_pass(L, h, tgt, far_src, np.eye(4), 1, 30, "shifted (12, -9, 0)")
        assert ncorr == far_src.shape[0]
        nfar = C.c_int64()
        L.check(lib.slio_icp_far_queries(h, C.byref(nfar)), "far_queries")
        print("far queries", nfar.value, "of", far_src.shape[0])
        assert nfar.value > far_src.shape[0] // 2   # most of them start off the fine cells
        check_pass(L, h, tgt, work, T_STEP, 0, 30, "shifted, step")
    finally:
        lib.slio_destroy(h)
    s2m = ScanToMap(max_points=4000)
    try:
        hl = s2m.loop_handle()
        upload(L, lib.slio_map_upload, hl, tgt)
        upload(L, lib.slio_scan_upload, hl, (src + np.float32([100, 0, 0])).astype(np.float32))
        _, ncorr = correspond(L, hl, np.eye(4), 1, 5)
        assert ncorr == 0
        conv, T, _, iters, state = s2m.icp_align(5)
        assert (conv, iters, state) == (False, 0, M.NO_CORRESPONDENCES)
        np.testing.assert_array_equal(T, np.eye(4, dtype=np.float32))
    finally:
        s2m.close()


def device_step(L, sums, ncorr, prm, st):
    delta, done = np.zeros(16, np.float32), C.c_int(-1)
    L.check(L.load().slio_icp_step(L.dptr(sums), ncorr, C.byref(prm), C.byref(st), L.fptr(delta), C.byref(done)),
            "icp_step")
    return delta.reshape(4, 4).copy(), done.value


@pytest.mark.parametrize("max_dist", [30, 0.5])
def test_lockstep_run(L, fix, max_dist):
    """icp_align driven by hand: every pass verified as in test_one_pass_exact
    on the device's own working cloud, every step's delta against the numpy
    Umeyama of the device's own sums to the CPU test's bound -- by induction
    the whole run, with no tolerance beyond those two."""
    tgt, src, runs = fix
    lib = L.load()
    h = mk(L)
    try:
        upload(L, lib.slio_map_upload, h, tgt)
        upload(L, lib.slio_scan_upload, h, src)
        prm, st = L.SlioIcpParams(), L.SlioIcpState()
        lib.slio_icp_params_default(C.byref(prm))
        lib.slio_icp_state_init(C.byref(st), None)
        ms = M.State()
        T, base, from_scan = np.eye(4, dtype=np.float32), src, 1
        for it in range(101):
            sums, ncorr, work = check_pass(L, h, tgt, base, T, from_scan, max_dist, f"pass {it}")
            prev_T = np.array(st.final_T, np.float32).reshape(4, 4)
            delta, done = device_step(L, sums, ncorr, prm, st)
            want, done_ref = M.step(sums, ncorr, ms)
            assert np.abs(delta[:3, :3].astype(np.float64) - want[:3, :3]).max() <= ULP1
            for a in range(3):
                assert abs(float(delta[a, 3]) - float(want[a, 3])) <= ULP1 * abs(float(want[a, 3]))
            ms.final_T = np.array(st.final_T, np.float32).reshape(4, 4)  # follow the device from here
            assert np.array_equal(ms.final_T, M.matmul32(delta, prev_T))
            assert (bool(done), st.convergence_state, st.iterations) == (done_ref, ms.state, ms.iterations)
            if done:
                break
            T, base, from_scan = delta, work, 0
        ref = runs[max_dist][0]
        assert (st.iterations, st.convergence_state, st.converged) == (ref["iterations"], ref["state"], 1)
    finally:
        lib.slio_destroy(h)


@pytest.mark.parametrize("max_dist", [30, 0.5])
def test_whole_run(L, fix, max_dist):
    """icp_align against the float64 restatement: same iteration count and end
    state; final_T within 16x the algorithm's own noise scale (the largest
    elementwise difference between the restatement with the rigid fit in
    float64 and in float32); the fitness within the summation bound of the
    restatement's fitness pass at the device's final_T (and equal to the
    restatement's own within that bound when final_T is bit-equal)."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    tgt, src, runs = fix
    r64, r32 = runs[max_dist]
    noise = float(np.abs(r64["final_T"].astype(np.float64) - r32["final_T"]).max())
    lib = L.load()
    s2m = ScanToMap(max_points=4000)
    try:
        hl = s2m.loop_handle()
        upload(L, lib.slio_map_upload, hl, tgt)
        upload(L, lib.slio_scan_upload, hl, src)
        conv, T, fitness, iters, state = s2m.icp_align(max_dist)
        dev = float(np.abs(T.astype(np.float64) - r64["final_T"]).max())
        print(f"max_dist {max_dist}: noise scale {noise:.3g}, device - restatement {dev:.3g}, "
              f"fitness {fitness:.6g} / {r64['fitness']:.6g}")
        assert (conv, iters, state) == (True, r64["iterations"], r64["state"])
        assert noise > 0 and dev <= 16 * noise
        fin = M.transform32(T, src)
        idx, sqd, _ = M.nearest32(fin, tgt)
        terms, ok = M.sum_terms(fin, tgt, idx, sqd, math.inf)
        n = int(ok.sum())
        # the sums' bound, and the two quotients' own roundings
        bound = M.sum_bounds(terms)[15] / n + 2 * 2.0 ** -53 * fitness
        assert abs(fitness - math.fsum(terms[15]) / n) <= bound
        if np.array_equal(T, r64["final_T"]):
            assert abs(fitness - r64["fitness"]) <= bound
    finally:
        s2m.close()


# ---- assembly -----------------------------------------------------------------
SIZES = [0, 1, 63, 64, 65, 257, 1500, 300]   # empty; around the wavefront (64) and the block (256)


def key_pose(i):
    return np.array([0.02 * i, -0.03 * i, 0.4 * i, 1.5 * i, -0.7 * i, 0.05 * i], np.float32)


def pose_matrix(p):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw): R = Rz Ry Rx."""
    return M.rot_zyx(float(p[0]), float(p[1]), float(p[2])), np.asarray(p[3:], np.float64)


def draw_keyframes(seed):
    """A jittered 12 m x 12 m ground patch seen from eight poses: keyframe i
    holds SIZES[i] points in the LiDAR frame of key_pose(i); every 97th point
    of keyframe 6 is NaN."""
    rng = np.random.default_rng(seed)
    out = []
    for i, n in enumerate(SIZES):
        world = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.normal(0, 0.02, n)], 1)
        R, t = pose_matrix(key_pose(i))
        body = ((world - t) @ R).astype(np.float32)
        if i == 6:
            body[::97] = np.nan
        out.append(np.ascontiguousarray(body.reshape(-1, 3)))
    return out


def loop_concat(oracle_mod, corner, surf, keys):
    parts = [np.zeros((0, 3), np.float32)]
    for k in keys:
        for kf in (corner[k], surf[k]):
            if kf.shape[0]:
                parts.append(oracle_mod.s2m_transform(key_pose(k), kf))
    return np.concatenate(parts).astype(np.float32)


def map_download(L, h):
    lib = L.load()
    n = C.c_int64()
    dims, cell = np.zeros(3, np.int32), C.c_float()
    L.check(lib.slio_map_info(h, L.iptr(dims), C.byref(cell), C.byref(n)), "map_info")
    cap = max(n.value, 1)
    x, y, z = (np.zeros(cap, np.float32) for _ in range(3))
    ids = np.zeros(cap, np.uint32)
    got = C.c_int64()
    L.check(lib.slio_map_download(h, L.fptr(x), L.fptr(y), L.fptr(z), ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  cap, C.byref(got)), "map_download")
    np.testing.assert_array_equal(ids[:got.value], np.arange(got.value, dtype=np.uint32))
    return np.stack([x, y, z], 1)[:got.value]


def scan_download(L, h, n):
    x, y, z = (np.zeros(max(n, 1), np.float32) for _ in range(3))
    L.check(L.load().slio_scan_download(h, L.fptr(x), L.fptr(y), L.fptr(z)), "scan_download")
    return np.stack([x, y, z], 1)[:n]


def test_loop_cloud_assembly(L, oracle_mod):
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    corner, surf = draw_keyframes(20261020), draw_keyframes(20261021)
    poses_all = np.stack([key_pose(k) for k in range(len(SIZES))])
    cat = loop_concat(oracle_mod, corner, surf, range(8))
    assert cat.shape[0] == 2 * sum(SIZES) and np.isnan(cat).any()
    want = oracle_mod.voxel_grid(cat, 0.4)
    one = oracle_mod.voxel_grid(loop_concat(oracle_mod, corner, surf, [4]), 0.4)
    assert 0 < one.shape[0] < want.shape[0] < cat.shape[0]
    lib = L.load()
    s2m = ScanToMap(max_points=4000)
    try:
        for i in range(len(SIZES)):
            assert s2m.push_keyframe(corner[i], surf[i]) == i
        # key 4, search_num 25: clipped to keys 0..7, corner then surf of each
        n = s2m.loop_find_near_keyframes(4, 25, poses_all, as_scan=False)
        assert n == want.shape[0]
        np.testing.assert_array_equal(map_download(L, s2m.hl), want)
        n = s2m.loop_find_near_keyframes(4, 25, poses_all, as_scan=True)
        assert n == want.shape[0]
        assert scan_download(L, s2m.hl, n).tobytes() == want.tobytes()
        # search_num 0: one keyframe
        n = s2m.loop_find_near_keyframes(4, 0, poses_all, as_scan=True)
        assert n == one.shape[0]
        assert scan_download(L, s2m.hl, n).tobytes() == one.tobytes()
        n = s2m.loop_find_near_keyframes(4, 0, poses_all, as_scan=False)
        np.testing.assert_array_equal(map_download(L, s2m.hl), one)
        # the assembled clouds serve the ICP pass: map = keys 0..7, scan = key 4
        s2m.loop_find_near_keyframes(4, 25, poses_all, as_scan=False)
        _, ncorr = correspond(L, s2m.hl, np.eye(4), 1, math.inf)
        assert ncorr == one.shape[0]
        # EINVAL: a key out of range; stores of different length
        cnt = np.zeros(2, np.int64)
        key = np.array([8], np.int32)
        pose = np.ascontiguousarray(poses_all[:1])
        assert lib.slio_s2m_loop_cloud(s2m.hl, s2m.hc, s2m.hs, L.iptr(key), L.fptr(pose), 1, 0.4, 0,
                                       L.i64ptr(cnt)) == EINVAL
        assert b"out of range" in lib.slio_last_error()
        key[0] = -1
        assert lib.slio_s2m_loop_cloud(s2m.hl, s2m.hc, s2m.hs, L.iptr(key), L.fptr(pose), 1, 0.4, 0,
                                       L.i64ptr(cnt)) == EINVAL
        key[0] = 4
        assert lib.slio_s2m_loop_cloud(s2m.hl, s2m.hc, s2m.hs, L.iptr(key), L.fptr(pose), 1, 0.4, 2,
                                       L.i64ptr(cnt)) == EINVAL
        assert lib.slio_s2m_loop_cloud(s2m.hl, s2m.hc, s2m.hs, L.iptr(key), L.fptr(pose), 1, 0.0, 0,
                                       L.i64ptr(cnt)) == EINVAL
        x = np.zeros(1, np.float32)
        L.check(lib.slio_s2m_kf_push(s2m.hc, L.fptr(x), L.fptr(x), L.fptr(x), 1, None), "push")
        assert lib.slio_s2m_loop_cloud(s2m.hl, s2m.hc, s2m.hs, L.iptr(key), L.fptr(pose), 1, 0.4, 0,
                                       L.i64ptr(cnt)) == EINVAL
        assert b"different numbers" in lib.slio_last_error()
        L.check(lib.slio_s2m_kf_push(s2m.hs, L.fptr(x), L.fptr(x), L.fptr(x), 1, None), "push")
        # ECAPACITY: a destination whose max_points is smaller than the result, as a scan
        small = mk(L, max_points=want.shape[0] - 1)
        try:
            keys = np.arange(8, dtype=np.int32)
            poses = np.ascontiguousarray(poses_all)
            assert lib.slio_s2m_loop_cloud(small, s2m.hc, s2m.hs, L.iptr(keys), L.fptr(poses), 8, 0.4, 1,
                                           L.i64ptr(cnt)) == ECAPACITY
            # ... while the map is not bounded by max_points
            L.check(lib.slio_s2m_loop_cloud(small, s2m.hc, s2m.hs, L.iptr(keys), L.fptr(poses), 8, 0.4, 0,
                                            L.i64ptr(cnt)), "loop_cloud")
            assert cnt.tolist() == [cat.shape[0], want.shape[0]]
            np.testing.assert_array_equal(map_download(L, small), want)
        finally:
            lib.slio_destroy(small)
    finally:
        s2m.close()


def test_loop_cloud_as_scan_without_a_point(L):
    """The as_scan assembly with an empty segment table: key 0's clouds are
    empty (SIZES[0] == 0), so nothing is gathered and the destination's scan
    becomes empty, as it does for no key at all; an assembly afterwards gives
    what it gave before."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    corner, surf = draw_keyframes(20261020), draw_keyframes(20261021)
    poses_all = np.stack([key_pose(k) for k in range(len(SIZES))])
    lib = L.load()
    s2m = ScanToMap(max_points=4000)
    hl = s2m.loop_handle()

    def as_scan(keys):
        key = np.asarray(keys, np.int32)
        pose = np.ascontiguousarray(poses_all[key].reshape(-1, 6), np.float32)
        cnt = np.full(2, -1, np.int64)
        L.check(lib.slio_s2m_loop_cloud(hl, s2m.hc, s2m.hs, L.iptr(key) if len(keys) else None,
                                        L.fptr(pose) if len(keys) else None, len(keys), 0.4, 1, L.i64ptr(cnt)),
                "loop_cloud")
        b, e = C.c_int64(-1), C.c_int64(-1)
        L.check(lib.slio_shard_range(hl, C.byref(b), C.byref(e)), "shard_range")  # (one rank: the whole scan)
        assert (b.value, e.value) == (0, cnt[1])
        return cnt.tolist(), scan_download(L, hl, int(cnt[1]))

    try:
        for i in range(len(SIZES)):
            assert s2m.push_keyframe(corner[i], surf[i]) == i
        cnt4, scan4 = as_scan([4])
        assert cnt4[0] == 2 * SIZES[4] and 0 < cnt4[1] <= cnt4[0]
        for keys in ([0], [0, 0], []):
            assert as_scan(keys)[0] == [0, 0]
        cnt, scan = as_scan([4])
        assert cnt == cnt4 and scan.tobytes() == scan4.tobytes()
    finally:
        s2m.close()


# ---- perform_loop_closure -------------------------------------------------------
def loop_case(points_per_key, dt=4.0):
    """Twelve keyframes cut from the scene (each its own draw of the same
    surfaces, within 9 m of its pose) along a circle of radius 4 m that key 11
    all but closes; key 11's pose carries the drift (FIX_R, FIX_T).  (The
    tests pass search_num = 5: with the default 25 a store of twelve keyframes
    would put key 11's own drifted cloud into the target.)"""
    rng = np.random.default_rng(20261020)
    n = 12
    th = np.arange(n) * (2 * np.pi / 11.2)
    true = np.zeros((n, 6))
    true[:, 2] = (th + np.pi / 2 + np.pi) % (2 * np.pi) - np.pi
    true[:, 3], true[:, 4] = 4 * np.cos(th), 4 * np.sin(th)
    corner, surf = [], []
    for i in range(n):
        world = M.scene(rng, points_per_key).astype(np.float64)
        world = world[np.hypot(world[:, 0] - true[i, 3], world[:, 1] - true[i, 4]) < 9.0]
        R = M.rot_zyx(*true[i, :3])
        body = ((world - true[i, 3:]) @ R).astype(np.float32)
        k = body.shape[0] // 10
        corner.append(np.ascontiguousarray(body[:k]))
        surf.append(np.ascontiguousarray(body[k:]))
    poses = true.copy()
    # drifted pose of key 11: T_wrong = D^-1 T_true, so that ICP's correction is ~D = (FIX_R, FIX_T)
    Rt = M.rot_zyx(*true[11, :3])
    Rw = M.FIX_R.T @ Rt
    tw = M.FIX_R.T @ (true[11, 3:] - M.FIX_T)
    poses[11] = [math.atan2(Rw[2, 1], Rw[2, 2]), math.asin(-Rw[2, 0]), math.atan2(Rw[1, 0], Rw[0, 0]), *tw]
    times = np.arange(n) * dt
    return corner, surf, poses.astype(np.float32), true, times


def test_perform_loop_closure(L):
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    corner, surf, poses, true, times = loop_case(4000)
    s2m = ScanToMap(max_points=8000)
    try:
        for i in range(12):
            assert s2m.push_keyframe(corner[i], surf[i]) == i
        container = {}
        # every stamp within 30 s: no candidate
        assert s2m.perform_loop_closure(poses, np.arange(12) * 2.0, 22.0, container, search_num=5) is None
        assert not container
        res = s2m.perform_loop_closure(poses, times, float(times[-1]), container, search_num=5)
        assert res is not None
        print("loop closure:", res.pair, "fitness", res.noise, "iterations", res.iterations, "pose", res.pose_from)
        assert res.pair == (11, 0) and container == {11: 0}
        assert res.noise <= 0.3
        np.testing.assert_array_equal(res.pose_to, poses[0][[3, 4, 5, 0, 1, 2]])
        # sanity, not a tolerance: the corrected pose is nearer the true one than the drifted pose was
        before = np.linalg.norm(poses[11, 3:] - true[11, 3:])
        after = np.linalg.norm(res.pose_from[:3] - true[11, 3:])
        print("translation error before / after", before, after)
        assert after < before
        # the pair is in the container now
        assert s2m.perform_loop_closure(poses, times, float(times[-1]), container, search_num=5) is None
    finally:
        s2m.close()
    # keyframes too small for the 300 / 1000 thresholds
    corner, surf, poses, true, times = loop_case(150)
    s2m = ScanToMap(max_points=8000)
    try:
        for i in range(12):
            s2m.push_keyframe(corner[i], surf[i])
        container = {}
        assert s2m.perform_loop_closure(poses, times, float(times[-1]), container, search_num=5) is None
        assert not container
    finally:
        s2m.close()
