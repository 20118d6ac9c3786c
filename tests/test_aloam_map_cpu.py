"""CPU tests of A-LOAM's laserMapping on the host (slio_aloam_map_host_*,
slio_aloam_map_predict; the argument checks of every slio_aloam_map_* entry
that need no device) against the plain-Python restatement
tests/aloam_map_model.py, to the bit: both poses, q / t_wmap_wodom, every LM
iterate, cost and mu, all counters, the stacks, the associations and every
touched cube, over the cases of tests/aloam_map_case.py; finite-difference
checks of both Jacobians on the model; the Jacobi eigen-solve against
numpy.linalg.eigh and the double QR against numpy.linalg.lstsq; and a
sanitizer run of the host code in a stand-alone program
(tests/aloam_map_host_main.cpp).  The host code shares its formulas with the
kernels (csrc/slio_aloam_map.hpp), so this is also what checks them where there
is no GPU.  No GPU.
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
import aloam_map_case as K  # noqa: E402
import aloam_map_model as M  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import aloam as A  # noqa: E402

EINVAL, ECAPACITY, ESTATE = -1, -4, -5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
# The largest relative deviations measured on the CPU by the two tests below
# (printed by them): eigenvalues of jacobi3 against numpy.linalg.eigh over the
# 400 random and the 60 two-equal matrices, relative to the largest eigenvalue,
# and the solution of qr_solve_m1 against numpy.linalg.lstsq over 400 random
# systems, relative to the largest |x_i|.  The assertions allow ten times that: the margin
# covers other libm and BLAS builds.
EIG_MEASURED = 1.14e-15   # measured 1.137e-15
QR_MEASURED = 6.6e-14    # measured 6.589e-14


def bits(a):
    return np.ascontiguousarray(a, np.float64).tobytes()


def same_result(got, want, what):
    """A library result (aloam._map_result) against the model's, to the bit."""
    for f in ("center", "shift", "map_size", "stack_size", "optimized", "nvalid"):
        assert got[f] == want[f], (what, f, got[f], want[f])
    for f in ("q_w_curr", "t_w_curr", "q_wmap_wodom", "t_wmap_wodom"):
        assert bits(got[f]) == bits(want[f]), (what, f, got[f], want[f])
    assert len(got["passes"]) == len(want["passes"]), what
    for k, (pg, pw) in enumerate(zip(got["passes"], want["passes"])):
        for f in A.PASS_FIELDS:
            assert pg[f] == pw[f], (what, k, f, pg[f], pw[f])
        assert len(pg["iterates"]) == len(pw["iterates"])
        for a, b in zip(pg["iterates"], pw["iterates"]):
            assert bits(a["q"]) == bits(b["q"]) and bits(a["t"]) == bits(b["t"]), (what, k)
            assert a["cost"] == b["cost"] and a["mu"] == b["mu"], (what, k)


def same_state(h, want, what):
    """The stacks and every touched cube of a mapper against the model's sweep."""
    for kind in range(2):
        np.testing.assert_array_equal(h.stack(kind), want["stack"][kind], err_msg=f"{what}, stack {kind}")
    for (kind, ind), cloud in want["cubes"].items():
        np.testing.assert_array_equal(h.cube(kind, ind), cloud, err_msg=f"{what}, cube {kind} {ind}")


def same_association(got, want, what):
    for g, w, name in zip(got, want, ("kind", "rec", "idx", "sqd")):
        assert g.tobytes() == np.ascontiguousarray(w, g.dtype).tobytes(), (what, name)


# ------------------------------------------------------------------ the model alone
def test_model_on_the_fixture():
    print("\nfixture figures:", K.check_fixture())


def test_crafted_cases_are_what_they_say():
    print("\ncrafted kinds:", K.check_crafted())
    print("shifts:", K.check_shifts())


def test_jacobians_against_finite_differences():
    """Central difference quotients of the residuals along the retraction, step
    1e-6, on the model: the step and the tolerance of test_aloam_odom_cpu.py's
    Jacobian test (100 x the deviation the quotient alone shows between steps
    1e-6 and 2e-6), the same arithmetic."""
    q = [0.02, -0.03, 0.05, math.sqrt(1 - 0.02 ** 2 - 0.03 ** 2 - 0.05 ** 2)]
    t = [0.3, -0.2, 0.1]
    cp, a, b = [1.0, 2.0, 0.5], [1.2, 1.9, 0.1], [1.21, 1.93, 0.29]
    n = [0.6, -0.48, 0.64]

    def quotient(fn, h):
        J = []
        for k in range(6):
            d = [0.0] * 6
            d[k] = h
            qp, tp = M.OM.retract(q, t, d)
            d[k] = -h
            qm, tm = M.OM.retract(q, t, d)
            rp, rm = fn(qp, tp)[0], fn(qm, tm)[0]
            J.append([(x - y) / (2 * h) for x, y in zip(rp, rm)])
        return np.array(J).T

    worst = {}
    for name, fn in (("edge", lambda q_, t_: M.slot_factor(q_, t_, cp, M.EDGE, a + b)),
                     ("plane", lambda q_, t_: M.slot_factor(q_, t_, cp, M.PLANE, n + [0.7, 0.0, 0.0]))):
        J = np.array(fn(q, t)[1])
        j1, j2 = quotient(fn, 1e-6), quotient(fn, 2e-6)
        dev, err = float(np.abs(j1 - j2).max()), float(np.abs(j1 - J).max())
        worst[name] = (err, dev)
        assert dev > 0 and err <= 100 * dev, (name, err, dev)
    print("\nJacobian against the quotient, quotient between the steps (edge, plane):", worst)


# ------------------------------------------------------------------ the two solvers
def spd_cases():
    rng = np.random.default_rng(5)
    out = []
    for k in range(400):
        B = rng.normal(size=(3, 5 if k % 2 else 3)) * 10.0 ** rng.uniform(-3, 2)
        out.append(B @ B.T)
    for k in range(60):                                          # two equal eigenvalues
        Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        a, b = rng.uniform(0.1, 5.0, 2)
        out.append(Q @ np.diag([a, a, b] if k % 2 else [b, a, a]) @ Q.T)
    out.append(np.zeros((3, 3)))
    out.append(np.diag([1.0, 1.0, 1.0]))
    return out


def test_jacobi_against_eigh():
    worst = 0.0
    for S in spd_cases():
        S = 0.5 * (S + S.T)
        lam, V = M.jacobi3([S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
        ref = np.linalg.eigh(S)[0]
        scale = max(abs(ref).max(), 1e-300)
        worst = max(worst, float(np.abs(np.sort(lam) - ref).max() / scale))
        V = np.array(V)
        assert np.abs(V.T @ V - np.eye(3)).max() < 1e-14
        assert np.abs(S @ V - V * np.array(lam)[None, :]).max() <= 1e-13 * scale + 1e-300
    print("\nlargest relative eigenvalue deviation:", worst)
    assert worst <= 10 * EIG_MEASURED


def test_qr_against_lstsq():
    rng = np.random.default_rng(6)
    worst = 0.0
    for k in range(400):
        Am = rng.normal(size=(5, 3)) * 10.0 ** rng.uniform(-1, 2) + rng.normal(size=3) * 5.0
        rank, x = M.qr_solve_m1([[float(v) for v in row] for row in Am])
        ref = np.linalg.lstsq(Am, -np.ones(5), rcond=None)[0]
        assert rank == 3
        worst = max(worst, float(np.abs(np.array(x) - ref).max() / np.abs(ref).max()))
    print("\nlargest relative deviation of x:", worst)
    assert worst <= 10 * QR_MEASURED
    # rank-deficient systems: Eigen's rank, and the fit counts them as degenerate
    assert M.qr_solve_m1([[0.1 * i, 1.0, 0.0] for i in range(5)])[0] == 2
    assert M.fit_plane([[0.0, 0.0, 0.0]] * 5)[0] == M.DEGENERATE


def test_host_fits_against_the_model():
    rng = np.random.default_rng(8)
    cases = [rng.normal(size=(5, 3)) * s + rng.normal(size=3) * 20 for s in (0.01, 0.1, 0.3, 1.0) for _ in range(25)]
    cases += [np.outer(np.arange(5) * 0.1, d) + 3.0 + rng.normal(size=(5, 3)) * 1e-3
              for d in rng.normal(size=(20, 3))]                 # near-lines
    cases += [np.c_[rng.uniform(-0.5, 0.5, (5, 2)), np.full(5, 2.0) + rng.normal(size=5) * e]
              for e in (0.0, 1e-3, 0.05, 0.2) for _ in range(10)]  # near-planes
    cases += [np.full((5, 3), 0.1), np.zeros((5, 3)), np.array([[0.1 * i, 1.0, 0.0] for i in range(5)])]
    kinds = set()
    for nb in cases:
        nb = np.ascontiguousarray(nb, F).astype(np.float64)       # neighbours are float32 map points
        lst = [[float(v) for v in row] for row in nb]
        k, a, b, lam, vec = A.map_host_fit_line(nb)
        wk, wrec = M.fit_line(lst)
        wl, wv = M.jacobi3(M.covariance(lst)[1])
        assert k == wk and bits(lam) == bits(wl) and bits(vec) == bits(wv)
        if k == M.EDGE:
            assert bits(np.r_[a, b]) == bits(wrec)
        k2, n, d, x = A.map_host_fit_plane(nb)
        with np.errstate(all="ignore"):
            wk2, wrec2 = M.fit_plane(lst)
        assert k2 == wk2 and bits(x) == bits(M.qr_solve_m1(lst)[1])
        if k2 == M.PLANE:
            assert bits(np.r_[n, d]) == bits(wrec2[:4])
        kinds |= {k, k2}
    assert kinds == {M.EDGE, M.PLANE, M.DEGENERATE, M.REJECTED}


def test_predict_and_select_against_the_model():
    q1, t1 = [0.01, -0.02, 0.3, 0.95], [1.5, -2.5, 0.25]          # (unnormalised on purpose)
    q2, t2 = [-0.05, 0.02, -0.1, 0.99], [30.0, -12.0, 1.0]
    q, t = A.map_predict(q1, t1, q2, t2)
    wq, wt = M.associate_to_map(q1, t1, q2, t2)
    assert bits(q) == bits(wq) and bits(t) == bits(wt)
    for tw in ([0.0, 0.0, 0.0], [-375.0, 375.0, -125.0], [-375.0000001, 374.9999999, 125.0], [-25.0, 25.0, -75.0],
               [999.0, -999.0, 400.0], [24.999, -25.001, 0.0]):
        cen, wcen = [10, 10, 5], [10, 10, 5]
        got = A.map_host_select(tw, cen)
        assert got == tuple(M.select(tw, wcen)) and cen == wcen, tw
        assert len(got[2]) <= 75
    c = np.array([10, 10, 5], np.int32)
    o = np.zeros(75, np.int32)
    bad = np.array([np.nan, 0.0, 0.0])
    assert L.load().slio_aloam_map_host_select(L.dptr(bad), L.iptr(c), L.iptr(o), L.iptr(o), L.iptr(o),
                                               L.iptr(o)) == EINVAL


# ------------------------------------------------------------------ host against the model
def run_pair(h, m, sweeps, what):
    for k, (c, s, q, t) in enumerate(sweeps):
        want = m.process(c, s, q, t)
        want["stack"] = [x.copy() for x in m.stack]
        want["cubes"] = K.snapshot(m, want["touched"])
        same_result(h.process(c, s, q, t), want, f"{what}, sweep {k}")
        same_state(h, want, f"{what}, sweep {k}")
        if want["optimized"]:
            same_association(h.association(), m.assoc, f"{what}, sweep {k}")


def test_fixture():
    want = K.model_run()
    h = A.AloamMappingHost()
    for k in range(K.N_SWEEPS):
        same_result(h.process(*K.last_clouds(k), *K.odom_pose(k)), want[k], f"sweep {k}")
        same_state(h, want[k], f"sweep {k}")
    h.reset()
    same_result(h.process(*K.last_clouds(0), *K.odom_pose(0)), want[0], "after reset")


def test_crafted_associations():
    cmap, smap, _ = K.crafted()
    m, r1, _ = K.crafted_model()
    h = A.AloamMappingHost(K.FINE, K.FINE)
    h.process(K.xyzi(cmap), K.xyzi(smap), *K.IDENT)
    cq, sq = K.crafted_scan()
    got = h.process(K.xyzi(cq), K.xyzi(sq), *K.IDENT)
    same_result(got, r1, "crafted")
    # (the host keeps the last pass's association; the first pass's, at the identity, through the evaluation)
    kind, rec, idx, sqd = K.M_assoc()
    xyz = np.concatenate([h.stack(0), h.stack(1)], 0)
    Aw, gw, cw, nw = M.evaluate(xyz, kind, rec, *K.IDENT)
    Ag, gg, cg, ng = A.map_host_evaluate(xyz, kind, rec, *K.IDENT)
    assert ng == nw and bits(Ag) == bits(Aw) and bits(gg) == bits(gw) and cg == cw
    assert cw == r1["passes"][0]["cost_first"]


@pytest.mark.parametrize("nc,ns,optimized", [(10, 50, 0), (11, 51, 1), (10, 51, 0), (11, 50, 0)])
def test_gate(nc, ns, optimized):
    c, s = (K.xyzi(x) for x in K.gate_clouds(nc, ns))
    h, m = A.AloamMappingHost(0.05, 0.05), M.Mapper(0.05, 0.05)
    run_pair(h, m, [(c, s, *K.IDENT), (c, s, *K.SIZE_POSE)], f"gate {nc} / {ns}")
    r = h.result
    assert r["map_size"] == [nc, ns] and r["optimized"] == optimized
    if not optimized:                                            # transformUpdate and the map update all the same
        assert bits(r["q_w_curr"]) == bits(K.SIZE_POSE[0]) and bits(r["t_w_curr"]) == bits(K.SIZE_POSE[1])
        assert sum(len(h.cube(0, i)) for i in m.cubes[0]) > nc


@pytest.mark.parametrize("nc,ns", K.SIZES)
def test_scan_sizes(nc, ns):
    want = K.size_model(nc, ns)
    h = A.AloamMappingHost(0.02, 0.02)
    h.process(*(K.xyzi(c) for c in K.size_map()), *K.IDENT)
    same_result(h.process(*(K.xyzi(c) for c in K.size_scan(nc, ns)), *K.SIZE_POSE), want, f"{nc} / {ns}")
    same_state(h, want, f"{nc} / {ns}")


def test_shift_sequence():
    want = K.shift_model()
    h = A.AloamMappingHost()
    c, s = (K.xyzi(x) for x in K.shift_clouds())
    for k, t in enumerate(K.SHIFT_STEPS):
        same_result(h.process(c, s, K.IDENT[0], [float(v) for v in t]), want[k], f"step {k}")
        for (kind, ind), cloud in want[k]["cubes"].items():
            np.testing.assert_array_equal(h.cube(kind, ind), cloud, err_msg=f"step {k}, cube {kind} {ind}")
        for kind in range(2):
            total = sum(len(h.cube(kind, i)) for i in range(M.NUM))
            assert total == int(want[k]["sizes"][kind].sum()), (k, kind)


# ------------------------------------------------------------------ argument errors, no device
def test_argument_errors_before_any_device_call():
    lib = L.load()
    p = L.SlioAloamMapParams()
    assert lib.slio_aloam_map_params_default(None) == EINVAL
    assert lib.slio_aloam_map_params_default(C.byref(p)) == 0
    assert (p.device, p.max_points, p.max_scan) == (0, 1 << 21, 400000)
    assert (p.leaf_corner, p.leaf_surf) == (F(0.4), F(0.8))
    h = C.c_void_p()
    assert lib.slio_aloam_map_create(None, C.byref(p)) == EINVAL
    assert lib.slio_aloam_map_create(C.byref(h), None) == EINVAL
    for field, bad in (("max_points", 0), ("max_scan", 0), ("max_scan", 400001), ("leaf_corner", 0.0),
                       ("leaf_surf", float("nan")), ("leaf_surf", float("inf")), ("device", -1)):
        for create in (lib.slio_aloam_map_create, lib.slio_aloam_map_host_create):
            if field == "device" and create is lib.slio_aloam_map_host_create:
                continue
            q = L.SlioAloamMapParams()
            lib.slio_aloam_map_params_default(C.byref(q))
            setattr(q, field, bad)
            assert create(C.byref(h), C.byref(q)) == EINVAL, field
            assert not h.value
    one = np.array([[1.0, 0.0, 0.0, 0.0]], F)
    q, t = np.array([0, 0, 0, 1.0]), np.zeros(3)
    r, ov = L.SlioAloamMapResult(), L.SlioAloamOdomView()
    d, i4, n64 = np.zeros(28), np.zeros(4, np.int32), C.c_int64()
    f1 = (L.fptr(one), 1)
    assert lib.slio_aloam_map_destroy(None) == 0
    assert lib.slio_aloam_map_reset(None) == EINVAL
    assert lib.slio_aloam_map_run(None, *f1, *f1, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
    assert lib.slio_aloam_map_run_view(None, C.byref(ov), L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
    assert lib.slio_aloam_map_register_cloud(None, None, 0, 0, None) == EINVAL
    assert lib.slio_aloam_map_get_cube(None, 0, 0, None, 0, C.byref(n64)) == EINVAL
    assert lib.slio_aloam_map_cube_sizes(None, 0, L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_map_get_surround(None, 0, None, 0, C.byref(n64)) == EINVAL
    assert lib.slio_aloam_map_get_map(None, 0, None, 0, C.byref(n64)) == EINVAL
    assert lib.slio_aloam_map_get_stack(None, 0, None, 0, C.byref(n64)) == EINVAL
    assert lib.slio_aloam_map_associate(None, L.dptr(q), L.dptr(t)) == EINVAL
    assert lib.slio_aloam_map_get_association(None, None, None, None, None, 0, L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_map_evaluate(None, L.dptr(q), L.dptr(t), L.dptr(d), L.dptr(d), L.dptr(d),
                                       L.iptr(i4)) == EINVAL
    assert b"null or destroyed handle" in lib.slio_last_error()
    # the host entries
    assert lib.slio_aloam_map_predict(None, L.dptr(t), L.dptr(q), L.dptr(t), L.dptr(d), L.dptr(d)) == EINVAL
    assert lib.slio_aloam_map_host_fit_line(None, L.dptr(d), L.dptr(d), None, None) == EINVAL
    assert lib.slio_aloam_map_host_fit_plane(L.dptr(d), None, L.dptr(d), None) == EINVAL
    assert lib.slio_aloam_map_host_evaluate(None, None, None, 1, L.dptr(q), L.dptr(t), L.dptr(d), L.dptr(d), L.dptr(d),
                                            L.iptr(i4)) == EINVAL
    assert lib.slio_aloam_map_host_run(None, *f1, *f1, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
    hh = A.AloamMappingHost(max_points=3, max_scan=2)
    with pytest.raises(L.SlioError, match="ESTATE"):
        hh.stack(0)
    run = lambda c, s, q_, t_: lib.slio_aloam_map_host_run(hh.h, L.fptr(c), len(c), L.fptr(s), len(s), L.dptr(q_),
                                                           L.dptr(t_), C.byref(r))
    two, three = np.repeat(one, 2, 0), np.repeat(one, 3, 0)
    assert run(one, one, np.array([0, 0, 0, np.nan]), t) == EINVAL
    assert run(one, one, np.zeros(4), t) == EINVAL                 # a zero quaternion has no inverse
    assert run(one, one, q, np.array([np.inf, 0, 0])) == EINVAL
    assert lib.slio_aloam_map_host_run(hh.h, None, 1, *f1, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
    assert lib.slio_aloam_map_host_run(hh.h, L.fptr(one), -1, *f1, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
    assert run(three, one, q, t) == ECAPACITY                     # beyond max_scan
    with pytest.raises(L.SlioError, match="ESTATE"):
        hh.stack(0)                                              # a refused call leaves the handle as it was
    spread = np.array([[0.0, 0, 0, 0], [5.0, 0, 0, 0]], F)
    assert run(spread, spread, q, t) == 0 and run(one, one, q, t) == 0
    assert [len(hh.cube(0, 2425)), len(hh.cube(1, 2425))] == [3, 3]   # the cube of the origin: 10 + 21 * 10 + 441 * 5
    assert run(one, one, q, t) == ECAPACITY                       # stored + incoming beyond max_points
    assert [len(hh.cube(0, 2425)), len(hh.cube(1, 2425))] == [3, 3]
    with pytest.raises(L.SlioError, match="EINVAL"):
        hh.cube(2, 0)
    with pytest.raises(L.SlioError, match="EINVAL"):
        hh.cube(0, M.NUM)


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_aloam_map.cpp compiled with the host compiler and
    -fsanitize=address,undefined into a stand-alone program that drives the
    fits, the evaluation and the sweeps; run as a child process, nothing
    preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "aloam_map_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "aloam_map_host_main.cpp"), os.path.join(csrc, "slio_aloam_map.cpp"),
           "-o", exe]
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
