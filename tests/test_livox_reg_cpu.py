"""CPU tests of livox_mapping's scanRegistration on the host
(slio_lreg_classify_host, slio_lreg_plane_judge, livox_reg.repub; the argument
checks of every slio_lreg_* entry that need no device) against the numpy
restatement tests/livox_reg_model.py, to the bit, and a sanitizer run of the
same host code in a stand-alone program (tests/livox_reg_host_main.cpp).  The
host code shares its per-point formulas with the kernels (csrc/slio_lreg.hpp),
so this is also what checks the formulas where there is no GPU.  No GPU.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import livox_reg_case as K  # noqa: E402
import livox_reg_model as M  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import livox_reg as R  # noqa: E402

F = np.float32
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check(cloud, want, what):
    got = R.classify_host(cloud)
    assert list(got["counts"]) == list(want["counts"]), what
    np.testing.assert_array_equal(got["visited"], want["visited"], err_msg=f"{what}: visited")
    np.testing.assert_array_equal(got["flags"], want["flags"], err_msg=f"{what}: flags")
    for name in ("cloud", "corner", "surf"):
        assert got[name].shape == want[name].shape, (what, name)
        np.testing.assert_array_equal(bits(got[name]), bits(want[name]), err_msg=f"{what}: {name}")
    assert got["stats"] == want["stats"], what
    return got


# ------------------------------------------------------------------ the fixtures
def test_dense_frame_takes_every_branch():
    st = K.check_dense_is_fit()
    assert st["reset_erased"] >= 1           # from the crafted spot (livox_reg_case.dense says so)


def test_no_fixture_point_on_a_scan_id_boundary():
    for name in ("dense", "duplicates", "nan_runs", "all_stride1", "all_stride4", "stress0", "kink+0"):
        K.check_no_scan_id_boundary(K.cut(name))


def test_stress_clouds_enter_the_runs_at_all_four_offsets():
    per_thread, per_wg = R.chain_tile()
    assert per_wg >= M.MAX_POINTS and per_thread >= 4
    seen = set()
    for s in K.STRESS_SEEDS:
        seen |= K.entry_offsets(K.model(f"stress{s}")["visited"], per_thread)
    assert seen == {0, 1, 2, 3}
    st1, st4 = K.model("all_stride1")["stats"], K.model("all_stride4")["stats"]
    assert st1["stride4"] == 0 and st1["stride1"] > 0 and st4["stride1"] == 0 and st4["stride4"] > 0


# ------------------------------------------------------------------ the handler
def test_dense_frame():
    check(K.cut("dense"), K.model("dense"), "dense")


@pytest.mark.parametrize("n", K.SMALL_SIZES + K.EDGE_SIZES)
def test_dense_frame_cut(n):
    got = check(K.cut("dense", n), K.model("dense", n), f"dense[:{n}]")
    if n <= 10:
        assert not got["visited"].any() and not got["flags"].any()      # no loop body runs
    if n == 11:
        assert list(np.nonzero(got["visited"])[0]) == [5]


def test_small_sizes_after_dropping_nonfinite_points():
    d = K.dense()
    for n in K.SMALL_SIZES:
        c = np.repeat(d[:n], 2, axis=0).copy()
        c[1::2, 2] = np.nan
        c = np.concatenate([np.full((3, 4), np.inf, F), c])
        want = M.register(c)
        assert want["counts"][0] == n
        check(c, want, f"{n} finite of {len(c)}")


@pytest.mark.parametrize("name", ["only_nonfinite", "nan_start", "nan_end", "nan_runs", "nan_blocks"])
def test_nonfinite_points(name):
    want = K.model(name)
    assert want["counts"][0] < len(K.cut(name))
    check(K.cut(name), want, name)


@pytest.mark.parametrize("n", K.TRUNC_SIZES)
def test_truncation_at_32000(n):
    want = K.model("big", n)
    assert list(want["counts"]) == list(K.model("big", 32000)["counts"])    # nothing past 32000 is read
    check(K.cut("big", n), want, f"big[:{n}]")


def test_duplicated_points_leave_zero_vectors_unnormalised():
    want = K.model("duplicates")
    assert not np.isnan(want["cloud"]).any()
    check(K.cut("duplicates"), want, "duplicates")


def test_points_on_the_axes():
    c = K.cut("axes")
    got = check(c, K.model("axes"), "axes")
    ids = [int(got["cloud"][i, 3]) for i in (7, 13, 21, 29)]       # +y, -y, +z, -z
    # -y: the reference's std::atan2 of two floats is the float -1.5707964, a
    # hair beyond -pi / 2: 89.9999975 degrees, scan id 9 (a double atan2 would give 10)
    assert ids == [30, 9, 20, 40]
    assert [M.scan_id(F(y), F(z)) for y, z in ((2, 0), (-2, 0), (0, 3), (0, -3))] == ids


def test_chain_clouds():
    for name in ("all_stride1", "all_stride4", "stress3", "kink-1", "kink+2"):
        check(K.cut(name), K.model(name), name)


# ------------------------------------------------------------------ plane_judge
def test_plane_judge():
    rng = np.random.default_rng(4)
    t = np.linspace(0, 1, 4)[:, None]
    line = np.array([3.0, 1.0, 0.5]) + t * np.array([0.3, -0.2, 0.1])
    plane = np.array([[0, 0, 2.0], [1, 0, 2.0], [0, 1, 2.0], [1, 1, 2.0], [0.5, 0.2, 2.0]])
    ball = rng.normal(size=(12, 3))
    lists = [line, line + rng.normal(0, 1e-3, line.shape), plane, ball, ball[:4], line[:1], np.zeros((4, 3))]
    seen = set()
    for k, p in enumerate(lists):
        p = p.astype(F)
        for thr in (100, 1000, 3):
            want = M.plane_judge([tuple(q) for q in p], thr)
            assert R.plane_judge(p, thr) == want, (k, thr)
            seen.add(want)
    assert seen == {True, False}
    assert R.plane_judge(line.astype(F), 100) and not R.plane_judge(ball.astype(F), 100)
    assert not R.plane_judge(plane.astype(F), 100)          # two equal large eigenvalues: no line


# ------------------------------------------------------------------ repub
def test_repub_two_messages():
    rng = np.random.default_rng(6)
    msgs = []
    for n in (5, 3):
        msgs.append((rng.normal(size=(n, 3)).astype(F), rng.integers(0, 6, n).astype(np.uint8),
                     rng.integers(0, 255, n).astype(np.uint8), np.sort(rng.integers(1, 10**8, n)).astype(np.uint32)))
    out = R.repub(*[[m[k] for m in msgs] for k in range(4)])
    assert out.shape == (8, 5) and out.dtype == F
    row = 0
    for xyz, line, refl, off in msgs:
        for i in range(len(xyz)):
            s = F(off[i]) / F(off[-1])                                  # uint32 / (float): float
            want = [xyz[i, 0], xyz[i, 1], xyz[i, 2], F(float(line[i]) + float(refl[i]) / 10000.0),
                    F(float(s) * 0.1)]
            np.testing.assert_array_equal(bits(out[row]), bits(np.array(want, F)))
            row += 1
    np.testing.assert_array_equal(out[[4, 7], 4], F(0.1))              # each message ends at curvature 0.1
    assert R.repub([], [], [], []).shape == (0, 5)


# ------------------------------------------------------------------ argument errors, no device
def test_argument_errors_before_any_device_call(lib):
    p = L.SlioLregParams()
    assert lib.slio_lreg_params_default(None) == EINVAL
    assert lib.slio_lreg_params_default(C.byref(p)) == 0
    assert (p.device, p.max_points) == (0, 32000)
    h = C.c_void_p()
    assert lib.slio_lreg_create(None, C.byref(p)) == EINVAL
    assert lib.slio_lreg_create(C.byref(h), None) == EINVAL
    for field, bad in (("max_points", 0), ("max_points", 32001), ("device", -1)):
        q = L.SlioLregParams()
        lib.slio_lreg_params_default(C.byref(q))
        setattr(q, field, bad)
        assert lib.slio_lreg_create(C.byref(h), C.byref(q)) == EINVAL, field
        assert not h.value
    xyzi, c3, i32 = np.zeros((4, 4), F), np.zeros(3, np.int32), np.zeros(4, np.int32)
    u8, aft, it, c2 = np.zeros(4, np.uint8), np.zeros(6, F), C.c_int32(), np.zeros(2, np.int64)
    assert lib.slio_lreg_destroy(None) == 0
    assert lib.slio_lreg_run(None, L.fptr(xyzi), 4, L.iptr(c3)) == EINVAL
    assert lib.slio_lreg_get_cloud(None, L.fptr(xyzi), 4) == EINVAL
    assert lib.slio_lreg_get_features(None, 0, L.fptr(xyzi), 4) == EINVAL
    assert lib.slio_lreg_get_flags(None, L.iptr(i32), L.u8ptr(u8)) == EINVAL
    assert b"null or destroyed handle" in lib.slio_last_error()
    assert lib.slio_lreg_chain_tile(None, L.iptr(i32)) == EINVAL
    assert lib.slio_lreg_chain_tile(L.iptr(i32), None) == EINVAL
    assert lib.slio_lvx_feed_device(None, None, L.i64ptr(c2)) == EINVAL
    assert lib.slio_lvx_process_cloud(None, None, L.fptr(xyzi), 4, L.fptr(aft), C.byref(it), L.iptr(c3)) == EINVAL
    # the host entries
    assert lib.slio_lreg_classify_host(None, 4, None, None, None, None, None, L.iptr(c3), None) == EINVAL
    assert lib.slio_lreg_classify_host(L.fptr(xyzi), -1, None, None, None, None, None, L.iptr(c3), None) == EINVAL
    assert lib.slio_lreg_classify_host(L.fptr(xyzi), 4, None, None, None, None, None, None, None) == EINVAL
    assert lib.slio_lreg_classify_host(None, 0, None, None, None, None, None, L.iptr(c3), None) == 0
    assert lib.slio_lreg_classify_host(L.fptr(xyzi), 4, None, None, None, None, None, L.iptr(c3), None) == 0
    assert list(c3) == [4, 0, 0]
    one = C.c_int32()
    xyz = np.zeros((4, 3), F)
    assert lib.slio_lreg_plane_judge(None, 4, 100, C.byref(one)) == EINVAL
    assert lib.slio_lreg_plane_judge(L.fptr(xyz), 0, 100, C.byref(one)) == EINVAL
    assert lib.slio_lreg_plane_judge(L.fptr(xyz), 65, 100, C.byref(one)) == EINVAL
    assert lib.slio_lreg_plane_judge(L.fptr(xyz), 4, 100, None) == EINVAL
    assert b"slio_lreg_plane_judge" in lib.slio_last_error()


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_lreg.cpp compiled with the host compiler and
    -fsanitize=address,undefined into a stand-alone program that drives the
    handler over the sizes and shapes above; run as a child process, nothing
    preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "livox_reg_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "livox_reg_host_main.cpp"), os.path.join(csrc, "slio_lreg.cpp"), "-o", exe]
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
