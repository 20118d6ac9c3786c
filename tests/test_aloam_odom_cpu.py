"""CPU tests of A-LOAM's laserOdometry on the host (slio_aloam_odom_host_*,
slio_aloam_odom_lm_step; the argument checks of every slio_aloam_odom_* entry
that need no device) against the plain-Python restatement
tests/aloam_odom_model.py, to the bit: correspondences, A, g, cost, each LM
iterate, both poses and every counter, over the four-sweep fixture and every
crafted case of tests/aloam_odom_case.py; the controller on injected values; a
finite-difference check of both Jacobians on the model; and a sanitizer run of
the host code in a stand-alone program (tests/aloam_odom_host_main.cpp).  The
host code shares its formulas with the kernels (csrc/slio_aloam_odom.hpp), so
this is also what checks them where there is no GPU.  No GPU.
"""
import ctypes as C
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aloam_odom_case as K  # noqa: E402
import aloam_odom_model as M  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import aloam as A  # noqa: E402

EINVAL, ECAPACITY, ESTATE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LM_FIELDS = ("mu", "nu", "cost", "model", "xnorm", "pivots_ok", "iterations", "accepted", "stop", "done",
             "last_accepted")
LM_VECTORS = ("q", "t", "A", "g", "delta", "qn", "tn")


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def same_result(got, want, what):
    for f in ("inited", "published", "frame_count"):
        assert got[f] == want[f], (what, f, got[f], want[f])
    for f in ("q_w_curr", "t_w_curr", "q_last_curr", "t_last_curr"):
        assert bits(got[f]) == bits(want[f]), (what, f, got[f], want[f])
    assert len(got["passes"]) == len(want["passes"]), what
    for k, (pg, pw) in enumerate(zip(got["passes"], want["passes"])):
        for f in A.PASS_FIELDS:
            assert pg[f] == pw[f], (what, k, f, pg[f], pw[f])
        assert len(pg["iterates"]) == len(pw["iterates"])
        for a, b in zip(pg["iterates"], pw["iterates"]):
            assert bits(a["q"]) == bits(b["q"]) and bits(a["t"]) == bits(b["t"]), (what, k)
            assert a["cost"] == b["cost"] and a["mu"] == b["mu"], (what, k)


# ------------------------------------------------------------------ the model alone
def test_model_on_the_fixture():
    fig = K.check_fixture()
    print("\nfixture figures:", fig)
    assert fig["rejected"] == 0                              # (so rejected steps are tested on injected values)


def test_crafted_cases_are_what_they_say():
    K.check_crafted()


def test_jacobians_against_finite_differences():
    """Central difference quotients of the residuals along the retraction, step
    1e-6, on the model.  Tolerance: 100 x the deviation the quotient alone
    shows between steps 1e-6 and 2e-6."""
    q = [0.02, -0.03, 0.05, math.sqrt(1 - 0.02 ** 2 - 0.03 ** 2 - 0.05 ** 2)]
    t = [0.3, -0.2, 0.1]
    cp, a, b, c = [1.0, 2.0, 0.5], [1.2, 1.9, 0.1], [1.1, 2.2, 1.3], [2.0, 2.5, 0.4]

    def quotient(fn, h):
        J = []
        for k in range(6):
            d = [0.0] * 6
            d[k] = h
            qp, tp = M.retract(q, t, d)
            d[k] = -h
            qm, tm = M.retract(q, t, d)
            rp, rm = fn(qp, tp)[0], fn(qm, tm)[0]
            J.append([(x - y) / (2 * h) for x, y in zip(rp, rm)])
        return np.array(J).T

    worst = {}
    for name, fn in (("edge", lambda q_, t_: M.edge_factor(q_, t_, cp, a, b)),
                     ("plane", lambda q_, t_: M.plane_factor(q_, t_, cp, a, b, c))):
        J = np.array(fn(q, t)[1])
        j1, j2 = quotient(fn, 1e-6), quotient(fn, 2e-6)
        dev, err = float(np.abs(j1 - j2).max()), float(np.abs(j1 - J).max())
        worst[name] = (err, dev)
        assert dev > 0 and err <= 100 * dev, (name, err, dev)
    print("\nJacobian against the quotient, quotient between the steps (edge, plane):", worst)


# ------------------------------------------------------------------ host against the model
@pytest.mark.parametrize("name", sorted(K.crafted()))
def test_crafted_pass(name):
    sharp, flat, corner_last, surf_last, q, t = K.crafted()[name]
    corr = M.associate(sharp, flat, corner_last, surf_last, q, t)
    got = A.odom_host_associate(sharp, flat, corner_last, surf_last, q, t)
    np.testing.assert_array_equal(got, corr, err_msg=name)
    Aw, gw, cw, nw = M.evaluate(sharp, flat, corner_last, surf_last, corr, q, t)
    Ag, gg, cg, ng = A.odom_host_evaluate(sharp, flat, corner_last, surf_last, corr, q, t)
    assert ng == nw and bits(Ag) == bits(Aw) and bits(gg) == bits(gw) and bits([cg]) == bits([cw]), name
    h, m = A.AloamOdometryHost(n_scans=64), M.Odometry()
    for k in range(2):
        same_result(h.process(sharp, corner_last, flat, surf_last), m.process(sharp, corner_last, flat, surf_last),
                    f"{name}, sweep {k}")


@pytest.mark.parametrize("skip", [2, 1])
def test_fixture(skip):
    want = K.model_run(skip)
    h = A.AloamOdometryHost(skip_frame_num=skip)
    for k in range(K.N_SWEEPS):
        same_result(h.process(*K.features(k)), want[k], f"sweep {k}")
    # each pass's correspondences and first evaluation through the single entries
    f0, f1 = K.features(0), K.features(1)
    corr = A.odom_host_associate(f1[0], f1[2], f0[1], f0[3], *K.IDENT)
    np.testing.assert_array_equal(corr, want[1]["passes"][0]["corr"])
    _, _, cost, cnt = A.odom_host_evaluate(f1[0], f1[2], f0[1], f0[3], corr, *K.IDENT)
    p0 = want[1]["passes"][0]
    assert cost == p0["cost_first"] and cnt[:3] == [p0["corner"], p0["plane"], p0["degenerate"]]
    h.reset()
    same_result(h.process(*K.features(0)), want[0], "after reset")


# ------------------------------------------------------------------ the controller on injected values
def lm_pair(A21, g, cost, q=(0.0, 0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0)):
    lm = L.SlioAloamOdomLm()
    lm.q[:], lm.t[:] = list(q), list(t)
    assert L.load().slio_aloam_odom_lm_step(C.byref(lm), 0, None, None, 0.0) == 0
    lm.A[:], lm.g[:], lm.cost = list(A21), list(g), cost
    return lm, M.Lm(q, t, A21, g, cost)


def same_lm(lm, m, what):
    for f in LM_FIELDS:
        a, b = getattr(lm, f), getattr(m, f)
        assert bits([a]) == bits([b]), (what, f, a, b)
    for f in LM_VECTORS:
        assert bits(list(getattr(lm, f))) == bits(getattr(m, f)), (what, f)


def propose(lm, m):
    assert L.load().slio_aloam_odom_lm_step(C.byref(lm), 1, None, None, 0.0) == 0
    go = m.propose()
    same_lm(lm, m, "propose")
    return go


def decide(lm, m, An, gn, cn):
    An, gn = np.ascontiguousarray(An, np.float64), np.ascontiguousarray(gn, np.float64)
    assert L.load().slio_aloam_odom_lm_step(C.byref(lm), 2, L.dptr(An), L.dptr(gn), cn) == 0
    m.decide(list(An), list(gn), cn)
    same_lm(lm, m, "decide")


def diag(d):
    Aq = [0.0] * 21
    for k in range(6):
        Aq[M.tri(k, k)] = d[k]
    return Aq


def test_controller_on_injected_values():
    rng = np.random.default_rng(3)
    B = rng.normal(size=(9, 6))
    H = B.T @ B
    A21 = [float(H[a, b]) for a in range(6) for b in range(a, 6)]
    g = [float(v) for v in rng.normal(size=6)]
    # two rejections: mu / 2 then mu / 4 of that; then an accepted step
    lm, m = lm_pair(A21, g, 1.0)
    assert propose(lm, m) and m.pivots_ok and m.model > 0
    decide(lm, m, A21, g, 2.0)                               # the cost rises: rejected
    assert (m.last_accepted, m.mu, m.nu) == (0, 1e4 / 2, 4.0)
    assert propose(lm, m)
    decide(lm, m, A21, g, 1.0)                               # rho = 0: rejected
    assert (m.last_accepted, m.mu, m.nu) == (0, 1e4 / 8, 8.0)
    assert propose(lm, m)
    mu0 = m.mu
    decide(lm, m, A21, g, 1.0 - m.model)                     # rho = 1: accepted, mu * 3, nu back to 2
    assert m.last_accepted == 1 and m.nu == 2.0 and m.mu == mu0 / (1.0 / 3.0) and not m.done
    assert bits(m.q) == bits(m.qn) and m.cost == lm.cost
    assert propose(lm, m)
    decide(lm, m, A21, g, m.cost)                            # the fourth: rejected, max_num_iterations
    assert m.done and m.stop == 0 and m.iterations == 4 and lm.done and lm.stop == 0
    assert not propose(lm, m)
    # rho just either side of 1e-3
    for rho, acc in ((1e-3 * (1 + 1e-9), 1), (1e-3 * (1 - 1e-9), 0), (1e-3, None)):
        lm, m = lm_pair(A21, g, 1.0)
        propose(lm, m)
        cn = 1.0 - rho * m.model
        decide(lm, m, A21, g, cn)
        if acc is not None:
            assert m.last_accepted == acc, rho
    # a non-positive model (with positive pivots it is delta^T (A / 2 + D^2 / mu) delta > 0, so only
    # rounding gives one: injected), with a cost that falls
    for model in (0.0, -1e-3):
        lm, m = lm_pair(A21, g, 1.0)
        assert propose(lm, m) and m.pivots_ok == 1
        lm.model = m.model = model
        decide(lm, m, A21, g, 0.5)
        assert m.last_accepted == 0 and m.nu == 4.0 and m.mu == 1e4 / 2
    # a non-positive pivot: delta is zero, the step is rejected and the parameter stop takes it
    lm, m = lm_pair(diag([1.0, 1.0, -1e9, 1.0, 1.0, 1.0]), g, 1.0)
    assert propose(lm, m) and m.pivots_ok == 0 and m.delta == [0.0] * 6
    decide(lm, m, lm.A, lm.g, 0.5)
    assert m.last_accepted == 0 and m.done and m.stop == 3
    # the 1e16 cap
    lm, m = lm_pair(A21, g, 1.0)
    lm.mu = m.mu = 0.9e16
    propose(lm, m)
    decide(lm, m, A21, g, 1.0 - m.model)
    assert m.last_accepted == 1 and m.mu == 1e16
    # the three stops
    lm, m = lm_pair(A21, [1e-10, -1e-11, 0.0, 0.0, 0.0, 0.0], 1.0)
    assert not propose(lm, m) and m.stop == 1 and m.iterations == 0
    lm, m = lm_pair(A21, g, 1.0)
    propose(lm, m)
    lm.cost = m.cost = 2e6 * m.model                         # rho = 1 and |cost - cost'| = model <= 1e-6 cost
    decide(lm, m, A21, g, m.cost - m.model)
    assert m.last_accepted == 1 and m.done and m.stop == 2 and m.iterations == 1
    lm, m = lm_pair(diag([1e8] * 6), [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1e-8)
    propose(lm, m)                                           # |delta| ~ 1e-8 <= 1e-8 (1 + 1e-8)
    assert math.sqrt(sum(v * v for v in m.delta)) <= 1e-8 * (m.xnorm + 1e-8)
    decide(lm, m, lm.A, lm.g, 1e-8 - 0.5 * m.model)
    assert m.last_accepted == 1 and m.done and m.stop == 3
    lm, m = lm_pair(diag([1e8] * 6), [1.0, 0.0, 0.0, 0.0, 0.0, 0.0], 1e-8)
    propose(lm, m)
    decide(lm, m, lm.A, lm.g, 1e-8)                          # the same step rejected: the parameter stop all the same
    assert m.last_accepted == 0 and m.done and m.stop == 3


# ------------------------------------------------------------------ argument errors, no device
def test_argument_errors_before_any_device_call():
    lib = L.load()
    p = L.SlioAloamOdomParams()
    assert lib.slio_aloam_odom_params_default(None) == EINVAL
    assert lib.slio_aloam_odom_params_default(C.byref(p)) == 0
    assert (p.device, p.n_scans, p.max_points, p.skip_frame_num) == (0, 16, 400000, 2)
    h = C.c_void_p()
    assert lib.slio_aloam_odom_create(None, C.byref(p)) == EINVAL
    assert lib.slio_aloam_odom_create(C.byref(h), None) == EINVAL
    for field, bad in (("n_scans", 0), ("n_scans", 65), ("max_points", 0), ("max_points", 400001),
                       ("skip_frame_num", 0), ("device", -1)):
        q = L.SlioAloamOdomParams()
        lib.slio_aloam_odom_params_default(C.byref(q))
        setattr(q, field, bad)
        assert lib.slio_aloam_odom_create(C.byref(h), C.byref(q)) == EINVAL, field
        assert not h.value
    one = K.cloud([K.P(1.0, 0.0, 0.0, 0)])
    r, v, ov = L.SlioAloamOdomResult(), L.SlioAloamView(), L.SlioAloamOdomView()
    d, i4 = np.zeros(28), np.zeros(4, np.int32)
    f1 = (L.fptr(one), 1)
    assert lib.slio_aloam_odom_destroy(None) == 0
    assert lib.slio_aloam_odom_reset(None) == EINVAL
    assert lib.slio_aloam_odom_run(None, *f1, *f1, *f1, *f1, C.byref(r)) == EINVAL
    assert lib.slio_aloam_odom_run_view(None, C.byref(v), C.byref(r)) == EINVAL
    assert lib.slio_aloam_odom_get_last(None, None, 0, None, 0, L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_odom_get_view(None, C.byref(ov)) == EINVAL
    assert lib.slio_aloam_odom_get_correspondences(None, None, 0, L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_odom_associate(None, L.dptr(d), L.dptr(d)) == EINVAL
    assert lib.slio_aloam_odom_evaluate(None, L.dptr(d), L.dptr(d), L.dptr(d), L.dptr(d), L.dptr(d),
                                        L.iptr(i4)) == EINVAL
    assert b"null or destroyed handle" in lib.slio_last_error()
    # the host entries
    lm = L.SlioAloamOdomLm()
    assert lib.slio_aloam_odom_lm_step(None, 0, None, None, 0.0) == EINVAL
    assert lib.slio_aloam_odom_lm_step(C.byref(lm), 3, None, None, 0.0) == EINVAL
    assert lib.slio_aloam_odom_lm_step(C.byref(lm), 2, None, None, 0.0) == EINVAL
    q, t = np.array([0, 0, 0, 1.0]), np.zeros(3)
    assert lib.slio_aloam_odom_host_associate(None, 1, *f1, *f1, *f1, L.dptr(q), L.dptr(t), L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_odom_host_associate(*f1, *f1, *f1, *f1, None, L.dptr(t), L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_odom_host_associate(*f1, *f1, *f1, *f1, L.dptr(q), L.dptr(t), None) == EINVAL
    assert lib.slio_aloam_odom_host_associate(L.fptr(one), 769, *f1, *f1, *f1, L.dptr(q), L.dptr(t),
                                              L.iptr(i4)) == ECAPACITY
    assert lib.slio_aloam_odom_host_evaluate(*f1, *f1, *f1, *f1, None, L.dptr(q), L.dptr(t), L.dptr(d), L.dptr(d),
                                             L.dptr(d), L.iptr(i4)) == EINVAL
    corr = np.array([[1, -1, -1], [0, 0, 0]], np.int32)      # an index past the one-point last cloud
    assert lib.slio_aloam_odom_host_evaluate(*f1, *f1, *f1, *f1, L.iptr(corr), L.dptr(q), L.dptr(t), L.dptr(d),
                                             L.dptr(d), L.dptr(d), L.iptr(i4)) == EINVAL
    st = L.SlioAloamOdomState()
    assert lib.slio_aloam_odom_host_init(None) == EINVAL and lib.slio_aloam_odom_host_init(C.byref(st)) == 0
    assert lib.slio_aloam_odom_host_run(None, C.byref(st), *f1, *f1, *f1, *f1, C.byref(r)) == EINVAL
    assert lib.slio_aloam_odom_host_run(C.byref(p), None, *f1, *f1, *f1, *f1, C.byref(r)) == EINVAL
    assert lib.slio_aloam_odom_host_run(C.byref(p), C.byref(st), *f1, *f1, *f1, *f1, None) == EINVAL
    p.n_scans = 1
    many = np.repeat(one, 13, 0)
    assert lib.slio_aloam_odom_host_run(C.byref(p), C.byref(st), L.fptr(many), 13, *f1, *f1, *f1,
                                        C.byref(r)) == ECAPACITY
    down = K.cloud([K.P(0.0, 0.0, 0.0, 2), K.P(1.0, 0.0, 0.0, 1)])
    assert lib.slio_aloam_odom_host_run(C.byref(p), C.byref(st), *f1, *f1, L.fptr(down), 2, *f1,
                                        C.byref(r)) == EINVAL
    assert b"scan ids" in lib.slio_last_error()
    with pytest.raises(L.SlioError, match="EINVAL"):
        A.AloamOdometryHost().process(one, down, one, one)


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_aloam_odom.cpp compiled with the host compiler and
    -fsanitize=address,undefined into a stand-alone program that drives the
    association, the evaluation, the sweep and the controller; run as a child
    process, nothing preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "aloam_odom_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "aloam_odom_host_main.cpp"), os.path.join(csrc, "slio_aloam_odom.cpp"),
           "-o", exe]
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
