"""CPU tests of the livox_mapping back-end's host code (slio_lvx_*,
include/slio.h) against the numpy restatement (tests/livox_map_model.py), to
the bit: the cube index, the cube selection with its field-of-view test and
shift bookkeeping, the plane system, the Gauss-Newton step, the argument
checks that need no device, and a sanitizer run of the same host code in a
stand-alone program (tests/livox_host_main.cpp).  No GPU.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import livox_map_model as M  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import livox_map as LV  # noqa: E402

F = np.float32
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


def same_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=what)


# ------------------------------------------------------------------ cube index
def test_cube_index_edges(lib):
    """Negative coordinates, exact multiples of 50 - 25 and the floats on
    either side of them, for three centres."""
    ts = []
    for k in range(-14, 15):
        e = F(50.0 * k - 25.0)
        ts += [np.nextafter(e, F(-np.inf)), e, np.nextafter(e, F(np.inf))]
    ts += list(np.random.default_rng(3).uniform(-700, 700, 200).astype(F)) + [F(0.0), F(-0.0)]
    for cen in (10, 5, -3):
        for t in ts:
            assert LV.cube_index(t, cen) == M.cube_index(t, cen), (t, cen)
    # the reference's quirk, stated: truncation then `--` is the floor except
    # on an exact negative multiple of 50 (t + 25 = -50 -> cube cen - 2)
    assert LV.cube_index(-75.0, 10) == 8
    assert LV.cube_index(np.nextafter(F(-75.0), F(0)), 10) == 9
    assert LV.cube_index(-25.0, 10) == 10      # t + 25 = 0 is not negative
    assert LV.cube_index(np.nextafter(F(-25.0), F(-np.inf)), 10) == 9
    assert LV.cube_index(25.0, 10) == 11
    out = C.c_int32()
    for bad in (float("nan"), float("inf"), 3e9):
        assert lib.slio_lvx_cube_index(bad, 10, C.byref(out)) == EINVAL
    assert lib.slio_lvx_cube_index(1.0, 10, None) == EINVAL


# ------------------------------------------------------------------ selection
POSES = [
    [0, 0, 0, 0, 0, 0],
    [0.3, -0.2, 1.1, 12.0, -30.0, 24.9],
    [-0.7, 0.4, -2.0, -80.0, 49.0, 130.0],
]


@pytest.mark.parametrize("k", range(len(POSES)))
def test_fov_all_125_cubes(k):
    """The FOV test over all 125 cubes at three poses: the valid and the
    surround lists in the reference's i, j, k order."""
    tf = np.array(POSES[k], F)
    cen_m = [10, 5, 10]
    c, s, valid, surround = M.select(tf, cen_m)
    cen, ctr, shift, v, su = LV.select_cubes_host(tf, [10, 5, 10])
    assert len(surround) == 125 and list(su) == surround
    assert list(v) == valid
    assert 0 < len(valid) < 125          # the test separates the cubes at this pose
    assert list(ctr) == c and list(shift) == s == [0, 0, 0] and list(cen) == cen_m


def test_fov_clipped_at_the_array_edge():
    """Surround cubes outside the array are left out (:721-722): a centre that
    starts off-centre in j keeps fewer than 125."""
    tf = np.array([0.1, 0.2, 0.3, 0.0, 20.0, 0.0], F)
    for cen0 in ([10, 1, 10], [1, 5, 19]):
        cen_m = list(cen0)
        c, s, valid, surround = M.select(tf, cen_m)
        cen, ctr, shift, v, su = LV.select_cubes_host(tf, cen0)
        assert (list(cen), list(ctr), list(shift), list(v), list(su)) == (cen_m, c, s, valid, surround)


SHIFTS = [
    ("+i", [0, 0, 0, -400.0, 0, 0], [1, 0, 0]),      # centerCubeI = 2 < 3
    ("-i", [0, 0, 0, 400.0, 0, 0], [-1, 0, 0]),      # centerCubeI = 18 >= 18
    ("+j", [0, 0, 0, 0, -160.0, 0], [0, 1, 0]),
    ("-j", [0, 0, 0, 0, 160.0, 0], [0, -1, 0]),
    ("+k", [0, 0, 0, 0, 0, -400.0], [0, 0, 1]),
    ("-k", [0, 0, 0, 0, 0, 400.0], [0, 0, -1]),
    ("twice", [0, 0, 0, -460.0, 0, 0], [2, 0, 0]),
    ("two axes", [0.2, 0.1, -0.4, 455.0, -210.0, 30.0], [-2, 2, 0]),
]


@pytest.mark.parametrize("name,tf,want", SHIFTS, ids=[s[0] for s in SHIFTS])
def test_shift_bookkeeping(name, tf, want):
    tf = np.array(tf, F)
    cen_m = [10, 5, 10]
    c, s, valid, surround = M.select(tf, cen_m)
    assert s == want                      # the model itself, against the loops read by hand
    cen, ctr, shift, v, su = LV.select_cubes_host(tf, [10, 5, 10])
    assert (list(cen), list(ctr), list(shift), list(v), list(su)) == (cen_m, c, s, valid, surround)
    assert list(cen) == [10 + want[0], 5 + want[1], 10 + want[2]]
    # the next call at the same pose finds the centre in range: no further shift
    cen2, ctr2, shift2, _, _ = LV.select_cubes_host(tf, cen)
    assert list(shift2) == [0, 0, 0] and list(cen2) == list(cen) and list(ctr2) == list(ctr)


def test_select_host_argument_errors(lib):
    tf = np.zeros(6, F)
    i3, i125, n = np.zeros(3, np.int32), np.zeros(125, np.int32), C.c_int32()
    good = [L.fptr(tf), L.iptr(i3), L.iptr(i3.copy()), L.iptr(i3.copy()), L.iptr(i125), C.byref(n),
            L.iptr(i125.copy()), C.byref(n)]
    for k in range(8):
        a = list(good)
        a[k] = None
        assert lib.slio_lvx_select_host(*a) == EINVAL, k
    bad = np.array([0, 0, np.nan, 0, 0, 0], F)
    assert lib.slio_lvx_select_host(L.fptr(bad), *good[1:]) == EINVAL
    far = np.array([0, 0, 0, 2e6, 0, 0], F)
    assert lib.slio_lvx_select_host(L.fptr(far), *good[1:]) == EINVAL
    assert b"1e6" in lib.slio_last_error()


# ------------------------------------------------------------------ plane system
def plane_sets():
    rng = np.random.default_rng(11)
    out = []
    for k in range(40):
        n = rng.normal(size=3)
        n /= np.linalg.norm(n)
        d = rng.uniform(1, 30)
        p = rng.uniform(-2, 2, (8, 3)) + n * d
        p -= np.outer(p @ n - d, n)                     # on the plane n . p = d
        p += rng.normal(scale=[0.0, 0.01, 0.3][k % 3], size=(8, 3))
        out.append(p.astype(F))
    out.append(np.zeros((8, 3), F))                     # the solve gives up
    out.append(np.tile(np.array([[1.0, 2.0, 3.0]], F), (8, 1)))   # rank 1
    return out


def test_plane_system_10x3_equals_8x3_and_the_model():
    """The library may run the 8 x 3 system because the reference's 10 x 3
    (two zero rows against -1) gives the same bits: asserted on both, and both
    against the model's 10 x 3."""
    gave_up = 0
    for k, nb in enumerate(plane_sets()):
        x10, x8, want = LV.plane_solve(nb, 10), LV.plane_solve(nb, 8), M.plane_system(nb, 10)
        if want is None:
            assert x10 is None and x8 is None, k
            gave_up += 1
            continue
        same_bits(x10, want, f"set {k}: m = 10")
        same_bits(x8, want, f"set {k}: m = 8")
        same_bits(M.plane_system(nb, 8), want, f"set {k}: model m = 8")
    assert gave_up >= 1


def test_plane_solve_argument_errors(lib):
    nb, x = np.zeros(24, F), np.zeros(3, F)
    assert lib.slio_lvx_plane_solve(None, 10, L.fptr(x)) == EINVAL
    assert lib.slio_lvx_plane_solve(L.fptr(nb), 10, None) == EINVAL
    for m in (0, 5, 9, 11):
        assert lib.slio_lvx_plane_solve(L.fptr(nb), m, L.fptr(x)) == EINVAL


# ------------------------------------------------------------------ the step
def spd(eigs, seed):
    """A^T A with the given eigenvalues (float32, symmetric)."""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.normal(size=(6, 6)))
    A = (Q * np.array(eigs, float)) @ Q.T
    A = ((A + A.T) / 2).astype(F)
    return np.ascontiguousarray(A)


STEP_CASES = [
    ("all above 1", [900, 400, 250, 90, 30, 4.0]),           # degenerate for LIO-SAM's 100, not here
    ("one below 1", [900, 400, 250, 90, 30, 0.3]),
    ("three below 1", [900, 400, 250, 0.8, 0.5, 0.2]),
    ("just above 1", [900, 400, 250, 90, 30, 1.5]),
]


@pytest.mark.parametrize("name,eigs", STEP_CASES, ids=[c[0] for c in STEP_CASES])
def test_lm_step_against_the_model(name, eigs):
    AtA = spd(eigs, 5)
    ev = np.linalg.eigvalsh(AtA.astype(float))
    below = int((ev < 1).sum())
    assert below == sum(e < 1 for e in eigs)     # the case is what its name says
    rng = np.random.default_rng(8)
    tf_c = np.array([0.01, -0.02, 0.3, 1.0, -2.0, 0.5], F)
    tf_m = tf_c.copy()
    state = {"is_degenerate": 0, "matP": [F(0)] * 36}
    deg, P = 0, None
    for it in range(4):
        # shrinking right-hand sides: the last turns converge
        AtB = (rng.normal(size=6) * [1e-1, 1e-2, 1e-4, 1e-6][it]).astype(F)
        stepped_m, conv_m = M.lm_step(AtA.reshape(-1), AtB, 400, it, tf_m, state)
        stepped, conv, tf_c, deg, P = LV.lm_step(AtA, AtB, 400, it, tf_c, deg, P)
        assert (stepped, conv) == (stepped_m, conv_m), it
        same_bits(tf_c, tf_m, f"{name}: transform after turn {it}")
        assert deg == state["is_degenerate"] == (1 if below else 0)
        same_bits(P, state["matP"], f"{name}: matP")
    assert conv_m                                 # the sequence did reach the 0.05 / 0.05 test


def test_lm_step_fewer_than_50_rows_is_a_continue():
    AtA = spd([900, 400, 250, 90, 30, 4.0], 5)
    AtB = np.full(6, 0.1, F)
    tf0 = np.arange(6, dtype=F)
    for nsel, want in ((0, False), (49, False), (50, True)):
        stepped, conv, tf, deg, P = LV.lm_step(AtA, AtB, nsel, 0, tf0, 7, None)
        tf_m, state = tf0.copy(), {"is_degenerate": 7, "matP": [F(0)] * 36}
        stepped_m, conv_m = M.lm_step(AtA.reshape(-1), AtB, nsel, 0, tf_m, state)
        assert stepped == stepped_m == want and conv == conv_m
        same_bits(tf, tf_m)
        if not want:                        # nothing moved, nothing decided
            same_bits(tf, tf0)
            assert deg == 7 and not conv and not P.any()


def test_lm_step_threshold_is_the_only_difference_to_lio_sam(lib):
    """slio_s2m_lm_step (threshold 100) and slio_lvx_lm_step (threshold 1) on an
    A^T A whose smallest eigenvalue lies between: degenerate there, not here;
    with every eigenvalue above 100 the transforms agree to the bit."""
    def both(AtA, AtB):
        out = []
        for fn in (lib.slio_s2m_lm_step, lib.slio_lvx_lm_step):
            tf, P, deg, conv = np.zeros(6, F), np.zeros(36, F), C.c_int(0), C.c_int(0)
            assert fn(L.fptr(AtA), L.fptr(AtB), 400, 0, L.fptr(tf), C.byref(deg), L.fptr(P), C.byref(conv)) == 0
            out.append((tf, deg.value))
        return out
    AtB = np.array([0.3, -0.2, 0.1, 0.5, 0.4, -0.6], F)
    (t_s, d_s), (t_l, d_l) = both(spd([900, 400, 250, 190, 130, 40.0], 2), AtB)
    assert (d_s, d_l) == (1, 0)
    (t_s, d_s), (t_l, d_l) = both(spd([900, 400, 250, 190, 130, 104.0], 2), AtB)
    assert (d_s, d_l) == (0, 0)
    same_bits(t_s, t_l)


def test_lm_step_argument_errors(lib):
    a36, a6, deg, conv = np.zeros(36, F), np.zeros(6, F), C.c_int(0), C.c_int(0)
    good = [L.fptr(a36), L.fptr(a6), 400, 0, L.fptr(a6.copy()), C.byref(deg), L.fptr(a36.copy()), C.byref(conv)]
    for k in (0, 1, 4, 5, 6, 7):
        a = list(good)
        a[k] = None
        assert lib.slio_lvx_lm_step(*a) == EINVAL, k
    assert b"slio_lvx_lm_step" in lib.slio_last_error()


# ------------------------------------------------------------------ handle entries, no device
def test_handle_entries_report_argument_errors_before_any_device_call(lib):
    p = L.SlioLvxParams()
    assert lib.slio_lvx_params_default(None) == EINVAL
    assert lib.slio_lvx_params_default(C.byref(p)) == 0
    assert (p.device, p.max_points) == (0, 1 << 21)
    assert (F(p.leaf_corner), F(p.leaf_surf)) == (F(0.2), F(0.4))
    h = C.c_void_p()
    assert lib.slio_lvx_create(None, C.byref(p)) == EINVAL
    assert lib.slio_lvx_create(C.byref(h), None) == EINVAL
    for field, bad in (("max_points", 0), ("leaf_corner", 0.0), ("leaf_surf", -0.4), ("leaf_corner", float("nan")),
                       ("leaf_surf", float("inf")), ("device", -1)):
        q = L.SlioLvxParams()
        lib.slio_lvx_params_default(C.byref(q))
        setattr(q, field, bad)
        assert lib.slio_lvx_create(C.byref(h), C.byref(q)) == EINVAL, field
        assert not h.value
    tf, i3, i125 = np.zeros(6, F), np.zeros(3, np.int32), np.zeros(125, np.int32)
    n32, n64, xyz = C.c_int32(), C.c_int64(), np.zeros(3, F)
    sizes = np.zeros(LV.NUM_CUBES, np.int32)
    assert lib.slio_lvx_destroy(None) == 0
    assert lib.slio_lvx_clear(None) == EINVAL
    assert lib.slio_lvx_select_cubes(None, L.fptr(tf), L.iptr(i3), L.iptr(i125), C.byref(n32), L.iptr(i125),
                                     C.byref(n32)) == EINVAL
    assert lib.slio_lvx_update_map(None, L.fptr(tf), L.fptr(xyz), 1, L.fptr(xyz), 1, None, 0, None) == EINVAL
    assert lib.slio_lvx_cube_sizes(None, 0, L.iptr(sizes)) == EINVAL
    assert lib.slio_lvx_get_cube(None, 0, 0, L.fptr(xyz), 1, C.byref(n64)) == EINVAL
    assert lib.slio_lvx_get_surround(None, 0, None, 0, L.fptr(xyz), 1, C.byref(n64)) == EINVAL
    assert lib.slio_lvx_get_centers(None, L.iptr(i3)) == EINVAL
    assert b"null handle" in lib.slio_last_error()


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_livox.cpp and slio_s2m.cpp compiled with the host compiler and
    -fsanitize=address,undefined into a stand-alone program that drives the
    same cases; run as a child process, nothing preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "livox_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "livox_host_main.cpp"), os.path.join(csrc, "slio_livox.cpp"),
           os.path.join(csrc, "slio_s2m.cpp"), "-o", exe]
    # the runtimes linked into the program itself (GCC's default is the shared
    # libasan, which insists on being first in the process's library list)
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
