"""CPU tests of LIO-Livox's ScanRegistration on the host (slio_llreg_extract_host,
slio_llreg_extract_pc2_host; the argument checks of every slio_llreg_* entry
that need no device) against the numpy restatement
tests/lio_livox_reg_model.py, to the bit, and a sanitizer run of the same host
code in a stand-alone program (tests/lio_livox_reg_host_main.cpp).  The host
code shares its formulas, and the serial form of a part's picking, with the
kernels (csrc/slio_llreg.hpp), so this is also what checks them where there is
no GPU.  No GPU.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_livox_reg_case as K  # noqa: E402
import lio_livox_reg_model as M  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import lio_livox as R  # noqa: E402

F = np.float32
EINVAL, ECAPACITY = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return L.load()


def same_points(got, want, what):
    """Bit for bit.  The one exception is normal_x (column 4 of a cloud point),
    where a NaN matches a NaN: the 0 / 0 of a zero time span carries the sign
    the machine gives it."""
    got, want = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    differ = got.view(np.uint32) != want.view(np.uint32)
    if got.shape[1] == 8:
        differ[:, 4] &= ~(np.isnan(got[:, 4]) & np.isnan(want[:, 4]))
    assert not differ.any(), (what, np.argwhere(differ)[:5])


def same_answer(got, want, what):
    assert [int(v) for v in got["counts"]] == list(want["counts"]), what
    assert [int(v) for v in got["line_size"]] == list(want["line_size"]), what
    assert [int(v) for v in got["finite_size"]] == list(want["finite_size"]), what
    for l in range(M.MAX_SCANS):
        np.testing.assert_array_equal(got["visited"][l], want["visited"][l], err_msg=f"{what}: visited of line {l}")
        np.testing.assert_array_equal(got["flags"][l], want["flags"][l], err_msg=f"{what}: flags of line {l}")
        same_points(got["lines"][l], want["lines"][l], f"{what}: line {l}")
    for name in ("cloud", "corner", "surf"):
        same_points(got[name], want[name], f"{what}: {name}")


def host(prm, kind, data):
    p = R.make_params(**prm)
    return R.extract_host(p, cloud=data) if kind == "pc2" else R.extract_host(p, **data)


# ------------------------------------------------------------------ the fixtures
def test_fixtures_reach_every_branch():
    st = K.check_fit()
    assert st["set101_nan"] >= 1 and st["set101_cc"] >= 1      # from the crafted spots (the case file says so)


def test_synth_frame_is_a_custom_msg():
    d = K.dense()
    n = len(d["xyz"])
    assert d["xyz"].dtype == F and d["reflectivity"].dtype == np.uint8 and d["line"].dtype == np.uint8
    assert d["offset_time"].dtype == np.uint32 and (np.diff(d["offset_time"].astype(np.int64)) > 0).all()
    assert all(len(v) == n for v in d.values()) and set(d["line"]) == set(range(6))


# ------------------------------------------------------------------ the node
@pytest.mark.parametrize("name", K.CPU_CASES)
def test_host_matches_model(name):
    same_answer(host(*K.case(name)), K.model(name), name)


def test_a_line_of_20001_is_an_error(lib):
    msg = K.one_line(M.MAX_LINE + 1)
    with pytest.raises(M.LineTooLong):
        M.feature_extract(K.P(n_scans=1), **msg)
    with pytest.raises(L.SlioError, match="20000"):
        host(K.P(n_scans=1), "msg", msg)
    # the same points on two lines are no error: nothing is truncated, nothing refused early
    msg["line"][1::2] = 1
    got = host(K.P(n_scans=2), "msg", msg)
    assert list(got["line_size"][:2]) == [10001, 10000]
    same_answer(got, M.feature_extract(K.P(n_scans=2), **msg), "20001 on two lines")


def test_pc2_wants_four_lines(lib):
    c3 = np.zeros(3, np.int32)
    xyzi = np.ones((8, 4), F)
    for n_scans in (1, 3):
        p = R.make_params(**K.P(n_scans=n_scans))
        assert lib.slio_llreg_extract_pc2_host(C.byref(p), L.fptr(xyzi), 8, None, None, None, L.iptr(c3), None, None,
                                               None, None, None) == EINVAL
        assert b"n_scans >= 4" in lib.slio_last_error()
        with pytest.raises(ValueError):
            M.feature_extract_mid(K.P(n_scans=n_scans), xyzi)


def test_num_curv_size_has_no_effect():
    prm, kind, data = K.case("dense")
    want = K.model("dense")
    for ncs in (0, 3, 7):
        same_answer(host(dict(prm, num_curv_size=ncs), kind, data), want, f"NumCurvSize {ncs}")


# ------------------------------------------------------------------ argument errors, no device
def test_argument_errors_before_any_device_call(lib):
    p = L.SlioLlregParams()
    assert lib.slio_llreg_params_default(None) == EINVAL
    assert lib.slio_llreg_params_default(C.byref(p)) == 0
    assert (p.device, p.max_points, p.n_scans, p.lidar_type, p.num_curv_size, p.num_flat, p.part_num) == \
        (0, 120000, 6, 0, 2, 3, 150)
    assert (p.distance_faraway, p.flat_threshold, p.break_corner_dis, p.lidar_nearest_dis,
            p.kdtree_corner_outlier_dis) == (100.0, F(0.02), 1.0, 1.0, F(0.2))
    h = C.c_void_p()
    assert lib.slio_llreg_create(None, C.byref(p)) == EINVAL
    assert lib.slio_llreg_create(C.byref(h), None) == EINVAL
    bad = (("max_points", 0), ("max_points", 120001), ("device", -1), ("n_scans", 0), ("n_scans", 7),
           ("lidar_type", -1), ("lidar_type", 3), ("num_flat", -1), ("part_num", 0), ("part_num", 20001),
           ("distance_faraway", float("nan")), ("flat_threshold", float("inf")),
           ("break_corner_dis", float("nan")), ("lidar_nearest_dis", float("-inf")))
    xyz, u8, u32 = np.ones((4, 3), F), np.zeros(4, np.uint8), np.arange(1, 5, dtype=np.uint32)
    xyzi, c3, i32 = np.ones((4, 4), F), np.zeros(3, np.int32), np.zeros(6, np.int32)
    nothing = (None,) * 3
    tail = (None,) * 5
    for field, value in bad:
        q = L.SlioLlregParams()
        lib.slio_llreg_params_default(C.byref(q))
        setattr(q, field, value)
        assert lib.slio_llreg_create(C.byref(h), C.byref(q)) == EINVAL, field
        assert not h.value
        if field in ("max_points", "device"):
            continue                                  # (the host entries read neither)
        assert lib.slio_llreg_extract_host(C.byref(q), L.fptr(xyz), L.u8ptr(u8), L.u8ptr(u8), L.u32ptr(u32), 4,
                                           *nothing, L.iptr(c3), *tail) == EINVAL, field
        assert lib.slio_llreg_extract_pc2_host(C.byref(q), L.fptr(xyzi), 4, *nothing, L.iptr(c3), *tail) == EINVAL
    assert lib.slio_llreg_destroy(None) == 0
    assert lib.slio_llreg_run(None, L.fptr(xyz), L.u8ptr(u8), L.u8ptr(u8), L.u32ptr(u32), 4, L.iptr(c3)) == EINVAL
    assert lib.slio_llreg_run_pc2(None, L.fptr(xyzi), 4, L.iptr(c3)) == EINVAL
    assert lib.slio_llreg_get_cloud(None, 0, L.fptr(xyzi), 4) == EINVAL
    assert lib.slio_llreg_get_lines(None, L.iptr(i32), L.iptr(i32)) == EINVAL
    assert lib.slio_llreg_get_flags(None, 0, L.iptr(i32), L.u8ptr(u8), L.fptr(xyzi), 4) == EINVAL
    assert lib.slio_llreg_get_view(None, C.byref(L.SlioLlregView())) == EINVAL
    assert b"null or destroyed" in lib.slio_last_error()
    for k in range(4):
        args = [L.iptr(i32)] * 4
        args[k] = None
        assert lib.slio_llreg_tiles(*args) == EINVAL
    per_thread, per_wg, fast, block = R.tiles()
    assert per_wg >= M.MAX_LINE and per_wg % per_thread == 0 and per_thread >= 4 and 1 <= fast <= 58 and block >= 64
    # the host entries
    ok = lambda: R.make_params()  # noqa: E731
    msg = (L.fptr(xyz), L.u8ptr(u8), L.u8ptr(u8), L.u32ptr(u32))
    assert lib.slio_llreg_extract_host(None, *msg, 4, *nothing, L.iptr(c3), *tail) == EINVAL
    assert lib.slio_llreg_extract_host(C.byref(ok()), *msg, -1, *nothing, L.iptr(c3), *tail) == EINVAL
    assert lib.slio_llreg_extract_host(C.byref(ok()), *msg, 4, *nothing, None, *tail) == EINVAL
    assert lib.slio_llreg_extract_host(C.byref(ok()), *msg, 120001, *nothing, L.iptr(c3), *tail) == ECAPACITY
    for k in range(4):
        holed = list(msg)
        holed[k] = None
        assert lib.slio_llreg_extract_host(C.byref(ok()), *holed, 4, *nothing, L.iptr(c3), *tail) == EINVAL, k
    assert lib.slio_llreg_extract_host(C.byref(ok()), None, None, None, None, 0, *nothing, L.iptr(c3), *tail) == 0
    assert list(c3) == [0, 0, 0]
    assert lib.slio_llreg_extract_host(C.byref(ok()), *msg, 4, *nothing, L.iptr(c3), *tail) == 0
    assert list(c3) == [4, 0, 0]
    assert lib.slio_llreg_extract_pc2_host(None, L.fptr(xyzi), 4, *nothing, L.iptr(c3), *tail) == EINVAL
    assert lib.slio_llreg_extract_pc2_host(C.byref(ok()), None, 4, *nothing, L.iptr(c3), *tail) == EINVAL
    assert lib.slio_llreg_extract_pc2_host(C.byref(ok()), L.fptr(xyzi), -1, *nothing, L.iptr(c3), *tail) == EINVAL
    assert lib.slio_llreg_extract_pc2_host(C.byref(ok()), L.fptr(xyzi), 4, *nothing, None, *tail) == EINVAL
    assert b"slio_llreg_extract_pc2_host" in lib.slio_last_error()
    assert lib.slio_llreg_extract_pc2_host(C.byref(ok()), L.fptr(xyzi), 4, *nothing, L.iptr(c3), *tail) == 0
    assert list(c3) == [4, 0, 0]


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_llreg.cpp compiled with the host compiler and
    -fsanitize=address,undefined into a stand-alone program that drives both
    paths over the sizes and shapes above; run as a child process, nothing
    preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "lio_livox_reg_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "lio_livox_reg_host_main.cpp"), os.path.join(csrc, "slio_llreg.cpp"), "-o", exe]
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
