"""CPU tests of the loop-closure ICP's host side: slio_icp_step against the
numpy restatement (tests/icp_model.py), the convergence table, argument
checks of the device entries without a device, and
detect_loop_closure_distance.  No GPU."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_model as M  # noqa: E402

ULP1 = 2.0 ** -23  # one float ulp of 1.0


@pytest.fixture(scope="module")
def lib():
    from agi_lidar_slam_amd import build, _lib
    build.build()
    return _lib.load()


def call_step(lib, sums, ncorr, st=None, max_iterations=100, t_eps=1e-6, fit_eps=1e-6):
    from agi_lidar_slam_amd import _lib as L
    prm = L.SlioIcpParams()
    assert lib.slio_icp_params_default(C.byref(prm)) == 0
    assert (prm.max_iterations, prm.transformation_epsilon, prm.euclidean_fitness_epsilon) == (100, 1e-6, 1e-6)
    prm.max_iterations, prm.transformation_epsilon, prm.euclidean_fitness_epsilon = max_iterations, t_eps, fit_eps
    if st is None:
        st = L.SlioIcpState()
        assert lib.slio_icp_state_init(C.byref(st), None) == 0
        assert st.prev_mse == M.DBL_MAX and list(st.final_T) == list(np.eye(4).reshape(16))
    sums = np.ascontiguousarray(sums, np.float64)
    delta = np.zeros(16, np.float32)
    done = C.c_int(-1)
    assert lib.slio_icp_step(L.dptr(sums), ncorr, C.byref(prm), C.byref(st), L.fptr(delta), C.byref(done)) == 0
    return delta.reshape(4, 4), done.value, st


def sums_of(p, q):
    """The 16 sums of the pairs (p_i, q_i), float32 points, exact terms."""
    p = np.asarray(p, np.float32)
    q = np.asarray(q, np.float32)
    d = p - q
    sqd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    idx = np.arange(p.shape[0])
    terms, ok = M.sum_terms(p, q, idx, sqd, math.inf)
    assert ok.all()
    return M.fsums(terms)


def point_sets():
    rng = np.random.default_rng(7)
    R = M.rot_zyx(0.3, -0.2, 0.5)
    t = np.array([0.4, -1.0, 0.25])
    p = rng.uniform(-3, 3, (10, 3)).astype(np.float32)
    rigid = (p, (p.astype(np.float64) @ R.T + t).astype(np.float32))
    pl = rng.uniform(-3, 3, (12, 3)).astype(np.float32)
    pl[:, 2] = 0.0
    ql = (pl.astype(np.float64) @ R.T + t).astype(np.float32)
    planar = (pl, ql)
    pm = rng.uniform(-3, 3, (10, 3)).astype(np.float32)
    qm = (pm.astype(np.float64) * np.array([1.0, 1.0, -1.0]) @ R.T + t).astype(np.float32)
    mirrored = (pm, qm)  # the best orthogonal map is a reflection: det(U) det(V) < 0
    return {"rigid": rigid, "planar": planar, "mirrored": mirrored}


@pytest.mark.parametrize("name", ["rigid", "planar", "mirrored"])
def test_step_rigid_fit_matches_numpy(lib, name):
    p, q = point_sets()[name]
    s = sums_of(p, q)
    n = p.shape[0]
    if name == "mirrored":
        mp, mq = s[0:3] / n, s[3:6] / n
        S = s[6:15].reshape(3, 3) / n - np.outer(mq, mp)
        U, _, Vt = np.linalg.svd(S)
        assert np.linalg.det(U) * np.linalg.det(Vt) < 0
    want = M.umeyama(s, n)
    delta, _, _ = call_step(lib, s, n)
    print(name, "max |dR|", np.abs(delta[:3, :3] - want[:3, :3]).max(), "max |dt|",
          np.abs(delta[:3, 3] - want[:3, 3]).max())
    assert np.abs(delta[:3, :3].astype(np.float64) - want[:3, :3]).max() <= ULP1
    for a in range(3):
        assert abs(float(delta[a, 3]) - float(want[a, 3])) <= ULP1 * abs(float(want[a, 3]))
    assert list(delta[3]) == [0, 0, 0, 1]
    R = delta[:3, :3].astype(np.float64)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * ULP1
    assert np.linalg.det(R) > 0


def small_motion_sums(scale=1.0, sqd_sum=None, n=10):
    """Sums whose fit is a rotation of `scale` * 1e-4 rad about z and a
    translation of `scale` * 1e-4."""
    rng = np.random.default_rng(3)
    p = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    R = M.rot_zyx(0, 0, 1e-4 * scale)
    q = (p.astype(np.float64) @ R.T + np.array([1e-4 * scale, 0, 0])).astype(np.float32)
    s = sums_of(p, q)
    if sqd_sum is not None:
        s[15] = sqd_sum
    return s, n


def big_motion_sums(sqd_sum, n=10):
    rng = np.random.default_rng(4)
    p = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    q = (p.astype(np.float64) @ M.rot_zyx(0.1, 0.2, 0.3).T + np.array([1.0, 2.0, 3.0])).astype(np.float32)
    s = sums_of(p, q)
    s[15] = sqd_sum
    return s, n


def test_convergence_iterations(lib):
    s, n = big_motion_sums(40.0)
    _, done, st = call_step(lib, s, n, max_iterations=1)
    assert (done, st.converged, st.convergence_state, st.iterations) == (1, 1, M.ITERATIONS, 1)


def test_convergence_transform(lib):
    s, n = small_motion_sums()
    delta, done, st = call_step(lib, s, n)
    d = delta.astype(np.float64)
    assert 0.5 * (np.trace(d[:3, :3]) - 1) >= 0.99999 and (d[:3, 3] ** 2).sum() <= 1e-6
    assert (done, st.converged, st.convergence_state) == (1, 1, M.TRANSFORM)
    # the epsilon is compared with the SQUARED translation: |t| = 5e-4 > 1e-6 still converges
    s, n = small_motion_sums(5.0)
    delta, done, st = call_step(lib, s, n)
    assert (delta[:3, 3].astype(np.float64) ** 2).sum() ** 0.5 > 1e-6
    assert (done, st.convergence_state) == (1, M.TRANSFORM)


def test_convergence_abs_mse(lib):
    from agi_lidar_slam_amd import _lib as L
    s, n = big_motion_sums(40.0)
    st = L.SlioIcpState()
    lib.slio_icp_state_init(C.byref(st), None)
    st.prev_mse = 4.0 + 5e-7     # mse = 4.0: |diff| < 1e-6
    _, done, st = call_step(lib, s, n, st)
    assert (done, st.converged, st.convergence_state) == (1, 1, M.ABS_MSE)
    assert st.prev_mse == 4.0 + 5e-7   # a converging turn leaves prev_mse


def test_convergence_rel_mse(lib):
    from agi_lidar_slam_amd import _lib as L
    s, n = big_motion_sums(4.0e6)   # mse = 4e5
    st = L.SlioIcpState()
    lib.slio_icp_state_init(C.byref(st), None)
    st.prev_mse = 4.0e5 + 1.0      # |diff| = 1 >= 1e-6, / prev = 2.5e-6 < 1e-5
    _, done, st = call_step(lib, s, n, st)
    assert (done, st.converged, st.convergence_state) == (1, 1, M.REL_MSE)


def test_no_correspondences(lib):
    s, _ = big_motion_sums(1.0)
    delta, done, st = call_step(lib, s, 2)
    assert (done, st.converged, st.convergence_state, st.iterations) == (1, 0, M.NO_CORRESPONDENCES, 0)
    assert np.array_equal(delta, np.eye(4, dtype=np.float32))
    assert list(st.final_T) == list(np.eye(4).reshape(16))


def test_two_calls_update_state(lib):
    s1, n = big_motion_sums(40.0)
    d1, done, st = call_step(lib, s1, n)
    assert (done, st.converged, st.convergence_state, st.iterations) == (0, 0, M.NOT_CONVERGED, 1)
    assert st.prev_mse == 4.0
    assert np.array_equal(np.array(st.final_T, np.float32).reshape(4, 4), M.matmul32(d1, np.eye(4)))
    s2, _ = big_motion_sums(20.0)
    d2, done, st = call_step(lib, s2, n, st)
    assert (done, st.iterations, st.prev_mse) == (0, 2, 2.0)
    assert np.array_equal(np.array(st.final_T, np.float32).reshape(4, 4), M.matmul32(d2, M.matmul32(d1, np.eye(4))))
    # the same two turns in the restatement
    ms = M.State()
    M.step(s1, n, ms)
    M.step(s2, n, ms)
    assert (ms.iterations, ms.prev_mse) == (2, 2.0)
    assert np.abs(ms.final_T.astype(np.float64) - np.array(st.final_T).reshape(4, 4)).max() <= 8 * ULP1 * 4


def test_step_bad_arguments(lib):
    from agi_lidar_slam_amd import _lib as L
    prm, st = L.SlioIcpParams(), L.SlioIcpState()
    s = np.zeros(16)
    d = np.zeros(16, np.float32)
    done = C.c_int()
    assert lib.slio_icp_step(None, 5, C.byref(prm), C.byref(st), L.fptr(d), C.byref(done)) == -1
    assert lib.slio_icp_step(L.dptr(s), -1, C.byref(prm), C.byref(st), L.fptr(d), C.byref(done)) == -1
    assert lib.slio_icp_step(L.dptr(s), 5, None, C.byref(st), L.fptr(d), C.byref(done)) == -1
    assert b"slio_icp_step" in lib.slio_last_error()
    assert lib.slio_icp_params_default(None) == -1 and lib.slio_icp_state_init(None, None) == -1


def test_device_entries_reject_null_handles_without_a_device(lib):
    """No handle exists without a device: null handles and bad arguments are
    EINVAL (-1) before any device call (this test runs with no GPU)."""
    from agi_lidar_slam_amd import _lib as L
    T = np.eye(4, dtype=np.float32).reshape(16)
    s = np.zeros(16)
    n = C.c_int64()
    assert lib.slio_icp_correspond(None, L.fptr(T), 1, 1.0, L.dptr(s), C.byref(n)) == -1
    assert b"null handle" in lib.slio_last_error()
    assert lib.slio_icp_correspond(None, None, 7, -1.0, None, None) == -1
    assert lib.slio_icp_get_correspondences(None, None, None) == -1
    assert lib.slio_icp_get_working(None, None, None, None, 0, None) == -1
    assert lib.slio_icp_far_queries(None, C.byref(n)) == -1
    key = np.zeros(1, np.int32)
    pose = np.zeros(6, np.float32)
    cnt = np.zeros(2, np.int64)
    assert lib.slio_s2m_loop_cloud(None, None, None, L.iptr(key), L.fptr(pose), 1, 0.4, 0, L.i64ptr(cnt)) == -1
    assert b"null handle" in lib.slio_last_error()
    assert lib.slio_s2m_loop_cloud(None, None, None, None, None, -1, 0.0, 5, None) == -1


# six hand-placed poses: a drive out and back; key 5 ends 1 m from key 0
POSES = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0], [20, 10, 0], [4, 3, 0], [1, 0, 0]], np.float32)
TIMES = np.array([0.0, 10.0, 20.0, 30.0, 40.0, 50.0])


def test_detect_loop_closure_distance():
    from agi_lidar_slam_amd.lio_sam import detect_loop_closure_distance as det
    # within 15 m of key 5, in distance order: 5 (0 m), 0 (1 m), 4 (4.2 m), 1 (9 m)
    assert det(POSES, TIMES, 50.0, {}) == (5, 0)
    # |50 - 0| = 50 is not MORE than a 50 s gate: nothing qualifies
    assert det(POSES, TIMES, 50.0, {}, time_diff=50.0) is None
    # key 0 too young: of keys 4 and 1, both old enough, the nearer one wins, not the lower index
    assert det(POSES, np.array([45.0, 10.0, 20.0, 30.0, 5.0, 50.0]), 50.0, {}) == (5, 4)
    # key 0 at exactly the radius is outside (the test is `<`)
    assert det(POSES, TIMES, 50.0, {}, radius=1.0) is None
    # none old enough: every stamp within 30 s of t_cur
    assert det(POSES, np.linspace(30.0, 50.0, 6), 50.0, {}) is None
    # the newest key already in the container
    assert det(POSES, TIMES, 50.0, {5: 0}) is None
    # another key in the container does not matter
    assert det(POSES, TIMES, 50.0, {4: 1}) == (5, 0)
    # a single pose: the only match is the newest key itself
    assert det(POSES[:1], TIMES[:1], 100.0, {}) is None
    assert det(np.zeros((0, 3)), np.zeros(0), 0.0, {}) is None
