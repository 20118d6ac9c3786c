"""GPU parity of the LIO-SAM scan-to-map core:
cornerOptimization / surfOptimization coefficients bit-exact vs the oracle
(oracle/lio_s2m_oracle.cpp) given the same transform, the LMOptimization
normal equations to fp32 rounding, and the whole scan2MapOptimization
converging to the ground-truth pose.  Parity unpinned: OpenCV / Eigen / PCL
are absent, their algorithms are restated (cv::eigen as OpenCV's Jacobi,
ColPivHouseholderQR, pcl::getTransformation).

Below those three cases: the same core on the fixtures of tests/s2m_case.py,
held to the oracle bit for bit (NaNs at the same places) and to the fp64
model tests/s2m_model.py, which is written from the geometry and shares no
expression with either.  Every branch of both coefficient functions runs
(the counts are asserted on the CPU first), the numerical edges by name
(clusters()), the transform through the neighbours it leads to, maps of four
and five points, the normal equations to the float ulp at the sizes where the
tail block, the butterfly and the per-workgroup partial could go wrong, and
the Jacobian against dR/d(angle) in fp64.  The tolerances against the model
are tests/test_s2m_model_cpu.py's (measured oracle against model, times 4);
the ulp bound is derived (s2m_case.ulp_bound)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2m_case as K  # noqa: E402
import s2m_model as M  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401
from test_s2m_model_cpu import NE_TOL, check_against_model, ne_deviation  # noqa: E402

pytestmark = pytest.mark.gpu


def lidar_pose(fr):
    from agi_lidar_slam_amd import synth
    return synth.s2m_lidar_pose(fr)


@pytest.fixture(scope="module")
def problem():
    from agi_lidar_slam_amd import synth
    return synth.make_s2m_problem()


@pytest.mark.parametrize("kind", [0, 1])
def test_coeffs_bitexact(L, oracle_mod, problem, kind):
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    s2m = ScanToMap(max_points=60000)
    try:
        s2m.set_maps(problem["corner_map"], problem["surf_map"])
        s2m.set_scan(problem["corner_scan"], problem["surf_scan"])
        rng = np.random.default_rng(kind)
        tf = problem["tf"] + np.concatenate([rng.uniform(-0.01, 0.01, 3), rng.uniform(-0.1, 0.1, 3)]).astype(np.float32)
        h = s2m.hc if kind == 0 else s2m.hs
        scan = problem["corner_scan"] if kind == 0 else problem["surf_scan"]
        mp = problem["corner_map"] if kind == 0 else problem["surf_map"]
        nsel = s2m.corner_optimization(tf) if kind == 0 else s2m.surf_optimization(tf)
        coeff = np.zeros((scan.shape[0], 4), np.float32)
        sel = np.zeros(scan.shape[0], np.uint8)
        L.check(L.load().slio_s2m_get_coeffs(h, L.fptr(coeff), L.u8ptr(sel)), "get")
        world = oracle_mod.s2m_transform(tf, scan)
        idx, sqd = oracle_mod.Tree(mp).knn(world, 5)
        rc, rs = oracle_mod.s2m_coeffs(kind, world, mp, idx, sqd)
        np.testing.assert_array_equal(sel, rs)
        np.testing.assert_array_equal(coeff, rc)
        assert nsel == int(rs.sum()) > (20 if kind == 0 else 1000)
    finally:
        s2m.close()


def test_normal_equations_and_convergence(L, oracle_mod, problem):
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    s2m = ScanToMap(max_points=60000)
    try:
        s2m.set_maps(problem["corner_map"], problem["surf_map"])
        s2m.set_scan(problem["corner_scan"], problem["surf_scan"])
        tf0 = problem["tf"] + np.array([0.005, -0.004, 0.01, 0.15, -0.1, 0.05], np.float32)
        s2m.corner_optimization(tf0)
        s2m.surf_optimization(tf0)
        AtA, AtB, n = s2m.normal_equations(tf0)
        clouds = []
        for kind, h, scan in ((0, s2m.hc, problem["corner_scan"]), (1, s2m.hs, problem["surf_scan"])):
            coeff = np.zeros((scan.shape[0], 4), np.float32)
            sel = np.zeros(scan.shape[0], np.uint8)
            L.check(L.load().slio_s2m_get_coeffs(h, L.fptr(coeff), L.u8ptr(sel)), "get")
            clouds.append((scan, coeff, sel))
        rA, rB, rn = oracle_mod.s2m_normal_equations(tf0, clouds)
        assert n == rn
        np.testing.assert_allclose(AtA.reshape(6, 6), rA, rtol=2e-6, atol=1e-6 * np.abs(rA).max())
        np.testing.assert_allclose(AtB, rB, rtol=2e-6, atol=1e-6 * np.abs(rB).max())
        tf = s2m.scan2MapOptimization(tf0)
        err_t = np.abs(tf[3:] - problem["tf"][3:]).max()
        err_r = np.abs(tf[:3] - problem["tf"][:3]).max()
        print(f"scan2MapOptimization: {s2m.iterations} iterations, |dt| {err_t:.4f} m, |dr| {err_r:.5f} rad, "
              f"degenerate {s2m.isDegenerate.value}")
        assert err_t < 0.05 and err_r < 0.003
    finally:
        s2m.close()


# ====================================================================== model, branches, edges
F = np.float32


def same_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan], err_msg=what)


@pytest.fixture(scope="module")
def s2m(L):
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    s = ScanToMap(max_points=8192)
    yield s
    s.close()


def handle(s2m, kind):
    return s2m.hc if kind == 0 else s2m.hs


def upload(L, s2m, kind, mp=None, scan=None):
    from agi_lidar_slam_amd.lio_sam import _upload
    lib = L.load()
    if mp is not None:
        _upload(lib, lib.slio_map_upload, handle(s2m, kind), mp)
    if scan is not None:
        _upload(lib, lib.slio_scan_upload, handle(s2m, kind), scan)


def device_coeffs(L, s2m, kind, tf, n):
    """slio_s2m_coeffs at tf, then what it left: (nsel, coeff, sel, idx, sqd)."""
    lib, h = L.load(), handle(s2m, kind)
    k = C.c_int64(-1)
    L.check(lib.slio_s2m_coeffs(h, kind, L.fptr(np.ascontiguousarray(tf, F)), C.byref(k)), "coeffs")
    coeff, sel = np.full((n, 4), 7.0, F), np.full(n, 7, np.uint8)
    L.check(lib.slio_s2m_get_coeffs(h, L.fptr(coeff), L.u8ptr(sel)), "get_coeffs")
    idx, sqd = np.full((n, 5), -7, np.int32), np.full((n, 5), -7.0, F)
    L.check(lib.slio_get_neighbors(h, L.iptr(idx), L.fptr(sqd), None), "get_neighbors")
    return k.value, coeff, sel, idx, sqd


def device_normal_equations(L, hc, hs, tf):
    AtA, AtB, n = np.full(36, 7.0, F), np.full(6, 7.0, F), C.c_int64(-1)
    L.check(L.load().slio_s2m_normal_equations(hc, hs, L.fptr(np.ascontiguousarray(tf, F)), L.fptr(AtA), L.fptr(AtB),
                                               C.byref(n)), "normal_equations")
    return AtA, AtB, n.value


def check_parity(L, s2m, kind, ref, what, tied=None):
    """Device against the oracle reference `ref` (bit for bit, neighbours
    included: k_s2m_transform is only reachable through them) and against the
    fp64 model."""
    n = ref["scan"].shape[0]
    upload(L, s2m, kind, ref["map"], ref["scan"])
    nsel, coeff, sel, idx, sqd = device_coeffs(L, s2m, kind, ref["tf"], n)
    same_bits(sqd, ref["sqd"], f"{what}: neighbour distances")
    free = np.ones(n, bool) if tied is None else ~tied
    np.testing.assert_array_equal(idx[free], ref["idx"][free], err_msg=f"{what}: neighbour ids")
    np.testing.assert_array_equal(np.sort(idx[~free], axis=1), np.sort(ref["idx"][~free], axis=1))
    np.testing.assert_array_equal(sel, ref["sel"], err_msg=f"{what}: sel")
    same_bits(coeff, ref["coeff"], f"{what}: coeff")
    assert nsel == int(sel.sum()) == int(ref["sel"].sum())
    check_against_model(coeff, sel, ref["model"], kind, f"device, {what}")
    return coeff, sel


@pytest.mark.parametrize("b", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cut_coeffs_oracle_and_model(L, oracle_mod, s2m, kind, b):
    ref = K.cut_reference(kind, b)
    # on the CPU, before anything runs on the device: the oracle alone reaches every branch
    n = {k: int(v.sum()) for k, v in ref["branches"].items()}
    assert n["selected"] >= 50 and n["gated"] >= 20 and n["shape"] >= 20 and (kind == 0 or n["weight"] >= 1), n
    assert K.tie_free(ref["sqd6"])
    check_parity(L, s2m, kind, ref, f"cut kind {kind} tf_b {b}")


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_clusters_coeffs_oracle_and_model(L, oracle_mod, s2m, kind, moved):
    ref = K.clusters_reference(kind, moved)
    names = K.clusters()[kind]["names"]
    identical = np.array([nm == "identical" for nm in names])
    assert K.tie_free(ref["sqd6"], exempt=identical)
    if not moved:
        assert ref["world"].tobytes() == ref["scan"].tobytes()
        br = ref["branches"]
        for nm, want in K.clusters()[kind]["expect"].items():
            if want is not None:
                assert br["selected" if want == "nan_selected" else want][names.index(nm)], nm
    coeff, sel = check_parity(L, s2m, kind, ref, f"clusters kind {kind} moved {moved}", tied=identical)
    if kind == 0 and not moved:
        i = names.index("line_z_on")
        assert sel[i] == 1 and np.isnan(coeff[i, :3]).all() and coeff[i, 3] == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_maps_of_four_and_five_points(L, oracle_mod, s2m, kind):
    cl = K.clusters()[kind]
    g = cl["names"].index("line_x_0" if kind == 0 else "plane_0")
    five, q = cl["map"][5 * g:5 * g + 5], np.ascontiguousarray(np.roll(cl["query"], -g, axis=0))
    zero = np.zeros(6, F)
    upload(L, s2m, kind, five[:4], q)
    nsel, coeff, sel, _, sqd = device_coeffs(L, s2m, kind, zero, q.shape[0])
    assert nsel == 0 and not sel.any() and not coeff.any()
    assert np.isinf(sqd[:, 4]).all()
    ref = K.reference(oracle_mod, kind, zero, q, five)
    assert ref["sel"][0] == 1 and ref["sel"].sum() == 1            # the group's own query, and only it
    upload(L, s2m, kind, five)
    nsel, coeff, sel, idx, sqd = device_coeffs(L, s2m, kind, zero, q.shape[0])
    np.testing.assert_array_equal(np.sort(idx, axis=1), np.tile(np.arange(5, dtype=np.int32), (q.shape[0], 1)))
    same_bits(sqd, ref["sqd"], "five-point map: distances")
    np.testing.assert_array_equal(sel, ref["sel"])
    same_bits(coeff, ref["coeff"], "five-point map: coeff")
    assert nsel == 1


def cut_clouds(nc, ns):
    c, rc, rs = K.cut(), K.cut_reference(0), K.cut_reference(1)
    return c, [(c["corner_scan"][:nc or 0], rc["coeff"][:nc or 0], rc["sel"][:nc or 0]),
               (c["surf_scan"][:ns or 0], rs["coeff"][:ns or 0], rs["sel"][:ns or 0])]


def check_ulp(AtA, AtB, n, tf, clouds, what):
    S, SB, T, TB, nsel = K.exact_sums(tf, clouds)
    assert n == nsel, what
    A = AtA.reshape(6, 6)
    errA, errB = np.abs(A.astype(np.float64) - S), np.abs(AtB.astype(np.float64) - SB)
    bA, bB = K.ulp_bound(S, T), K.ulp_bound(SB, TB)
    print(f"{what}: {n} rows, largest error / bound AtA {(errA / bA).max():.3f}, AtB {(errB / bB).max():.3f}")
    assert (errA <= bA).all() and (errB <= bB).all(), what
    assert A.tobytes() == np.ascontiguousarray(A.T).tobytes(), what


# None: that class through a NULL handle
@pytest.mark.parametrize("nc,ns", [(1, 1), (255, 257), (256, 256), (257, 255), (None, 513), (513, None)])
def test_normal_equations_to_the_ulp(L, oracle_mod, s2m, nc, ns):
    c, clouds = cut_clouds(nc, ns)
    for kind, m in ((0, nc), (1, ns)):
        if m is None:
            continue
        upload(L, s2m, kind, c["corner_map" if kind == 0 else "surf_map"], clouds[kind][0])
        _, coeff, sel, _, _ = device_coeffs(L, s2m, kind, c["tf"], m)
        np.testing.assert_array_equal(sel, clouds[kind][2])       # a prefix's points are the whole scan's
        same_bits(coeff, clouds[kind][1])
    hc, hs = (None if nc is None else s2m.hc), (None if ns is None else s2m.hs)
    AtA, AtB, n = device_normal_equations(L, hc, hs, c["tf"])
    assert n == int(clouds[0][2].sum()) + int(clouds[1][2].sum()) > 0
    check_ulp(AtA, AtB, n, c["tf"], clouds, f"nc {nc} ns {ns}")
    again = device_normal_equations(L, hc, hs, c["tf"])
    assert again[0].tobytes() == AtA.tobytes() and again[1].tobytes() == AtB.tobytes() and again[2] == n


def test_normal_equations_nothing_selected(L, oracle_mod, s2m):
    c = K.cut()
    for kind in (0, 1):
        ref = K.cut_reference(kind)
        scan = ref["scan"][ref["branches"]["gated"] | ref["branches"]["shape"]][:300]
        assert scan.shape[0] >= 40
        upload(L, s2m, kind, ref["map"], scan)
        nsel, coeff, sel, _, _ = device_coeffs(L, s2m, kind, c["tf"], scan.shape[0])
        assert nsel == 0 and not sel.any() and not coeff.any()
    AtA, AtB, n = device_normal_equations(L, s2m.hc, s2m.hs, c["tf"])
    assert n == 0 and not AtA.any() and not AtB.any()
    assert not np.signbit(AtA).any() and not np.signbit(AtB).any()


def test_normal_equations_with_the_nan_row(L, oracle_mod, s2m):
    """The query exactly on its line is selected with NaN coefficients: the
    sums are NaN exactly where the oracle's are; without it they are finite
    and within the ulp bound (rows of the hand-built clusters)."""
    zero = np.zeros(6, F)
    refs = [K.clusters_reference(0), K.clusters_reference(1)]
    on = K.clusters()[0]["names"].index("line_z_on")
    for drop in (False, True):
        clouds = []
        for kind, ref in enumerate(refs):
            keep = np.ones(ref["scan"].shape[0], bool)
            keep[on] = not (drop and kind == 0)
            upload(L, s2m, kind, ref["map"], ref["scan"][keep])
            _, coeff, sel, _, _ = device_coeffs(L, s2m, kind, zero, int(keep.sum()))
            same_bits(coeff, ref["coeff"][keep])
            clouds.append((ref["scan"][keep], coeff, sel))
        AtA, AtB, n = device_normal_equations(L, s2m.hc, s2m.hs, zero)
        rA, rB, rn = oracle_mod.s2m_normal_equations(zero, clouds)
        assert n == rn == sum(int(cl[2].sum()) for cl in clouds)
        np.testing.assert_array_equal(np.isnan(AtA.reshape(6, 6)), np.isnan(rA))
        np.testing.assert_array_equal(np.isnan(AtB), np.isnan(rB))
        if drop:
            assert np.isfinite(AtA).all() and np.isfinite(AtB).all()
            check_ulp(AtA, AtB, n, zero, clouds, "clusters without the NaN row")
        else:
            assert np.isnan(AtA).any() and np.isnan(AtB).any()


@pytest.mark.parametrize("b", [False, True])
def test_jacobian_against_fp64(L, oracle_mod, s2m, b):
    """A^T A / A^T B of the device against J^T J / -J^T d with J from the three
    dR/d(angle) matrices in fp64, at tf and at tf_b (every angle far from 0):
    the Jacobian's thirty terms and the camera / lidar axis swap, checked
    against something that is not a copy of them."""
    c = K.cut()
    tf = c["tf_b" if b else "tf"]
    clouds = []
    for kind in (0, 1):
        ref = K.cut_reference(kind, b)
        upload(L, s2m, kind, ref["map"], ref["scan"])
        nsel, coeff, sel, _, _ = device_coeffs(L, s2m, kind, tf, ref["scan"].shape[0])
        assert nsel >= 50
        clouds.append((ref["scan"], coeff, sel))
    AtA, AtB, n = device_normal_equations(L, s2m.hc, s2m.hs, tf)
    mA, mB, mn = M.normal_equations(tf, clouds)
    dA, dB = ne_deviation(AtA, AtB, mA, mB)
    print(f"device against fp64 at {'tf_b' if b else 'tf'}: {n} rows, deviation / largest entry AtA {dA:.2e}, AtB {dB:.2e}")
    assert n == mn
    assert dA <= NE_TOL and dB <= NE_TOL
