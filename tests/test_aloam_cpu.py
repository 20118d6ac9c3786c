"""CPU tests of A-LOAM's scanRegistration on the host
(slio_aloam_register_host; the argument checks of every slio_aloam_* entry that
need no device) against the numpy restatement tests/aloam_model.py, to the bit:
the five clouds, the scan index arrays, curvature, labels, picked, counts and
every branch counter; and a sanitizer run of the same host code in a
stand-alone program (tests/aloam_host_main.cpp).  The host code shares its
per-point formulas with the kernels (csrc/slio_aloam.hpp), so this is also
what checks the formulas where there is no GPU.  No GPU.
"""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aloam_case as K  # noqa: E402
import aloam_model as M  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import aloam as A  # noqa: E402
from agi_lidar_slam_amd import synth  # noqa: E402

F = np.float32
EINVAL, ECAPACITY = -1, -4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = M.CLOUDS + ("scan_start", "scan_end", "curvature", "label", "picked")


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=what)


def check(cloud, want, what, n_scans=16):
    got = A.register_host(cloud, n_scans=n_scans)
    assert list(got["counts"]) == list(want["counts"]), what
    for name in FIELDS:
        same_bits(got[name], want[name], f"{what}: {name}")
    assert got["stats"] == want["stats"], what
    return got


# ------------------------------------------------------------------ the fixtures
def test_stats_names_agree():
    assert A.STATS == M.STATS and A.CLOUDS == M.CLOUDS


def test_dense_sweep_takes_every_pick_branch():
    K.check_dense_is_fit()


def test_cases_reach_every_orientation_branch():
    K.check_orientation_branches()


def test_crafted_cases_are_what_they_say():
    K.check_crafted_cases()


def test_no_fixture_point_near_a_scan_id_boundary():
    K.check_margins()
    assert K.scan_margin("dense") > 0.4 and K.scan_margin("hdl32") > 0.4 and K.scan_margin("hdl64") > 0.25


def test_spinning_sweep_generalises_the_vlp16_sweep():
    a = synth.make_vlp16_sweep(horizon=120)
    b = synth.make_spinning_sweep(K.VLP16, horizon=120)
    for k in "xyz":
        np.testing.assert_array_equal(a[k], b[k])
    c = synth.make_spinning_sweep(K.HDL32, horizon=50)
    assert set(np.unique(c["ring"])) == set(range(32)) and (np.diff(c["col"]) >= 0).all()


# ------------------------------------------------------------------ the handler
@pytest.mark.parametrize("name", K.CPU_CASES)
def test_case(name):
    got = check(K.cut(name), K.model(name), name, K.layout(name))
    if name in ("empty", "all_range", "all_scan_id", "survivors_all_dropped"):
        assert list(got["counts"]) == [0] * 5


def test_minimum_range_is_compared_as_a_float():
    d = K.cut("dense")
    r2 = (d.astype(np.float64) ** 2).sum(1)
    thr = float(np.sqrt(np.median(r2)))
    want = M.register(d, minimum_range=thr)
    assert 0 < want["stats"]["drop_range"] < len(d)
    got = A.register_host(d, minimum_range=thr)
    assert got["stats"] == want["stats"]
    same_bits(got["laserCloud"], want["laserCloud"], "range")
    same_bits(got["surfPointsLessFlat"], want["surfPointsLessFlat"], "range")


def test_tile():
    blk, cap = A.tile()
    assert blk >= 64 and blk % 64 == 0 and cap >= blk


# ------------------------------------------------------------------ argument errors, no device
def test_argument_errors_before_any_device_call():
    lib = L.load()
    p = L.SlioAloamParams()
    assert lib.slio_aloam_params_default(None) == EINVAL
    assert lib.slio_aloam_params_default(C.byref(p)) == 0
    assert (p.device, p.n_scans, p.max_points, p.minimum_range, p.scan_period) == (0, 16, 400000, 0.1, 0.1)
    h = C.c_void_p()
    assert lib.slio_aloam_create(None, C.byref(p)) == EINVAL
    assert lib.slio_aloam_create(C.byref(h), None) == EINVAL
    for field, bad in (("n_scans", 0), ("n_scans", 17), ("n_scans", 128), ("max_points", 0), ("max_points", 400001),
                       ("device", -1)):
        q = L.SlioAloamParams()
        lib.slio_aloam_params_default(C.byref(q))
        setattr(q, field, bad)
        assert lib.slio_aloam_create(C.byref(h), C.byref(q)) == EINVAL, field
        assert not h.value
        if field != "device":
            c5 = np.zeros(5, np.int32)
            assert lib.slio_aloam_register_host(C.byref(q), None, 0, *[None] * 10, L.iptr(c5), None) == EINVAL, field
    xyz, c5, i32, u8 = np.zeros((4, 3), F), np.zeros(5, np.int32), np.zeros(64, np.int32), np.zeros(4, np.uint8)
    out, v = np.zeros((4, 4), F), L.SlioAloamView()
    assert lib.slio_aloam_destroy(None) == 0
    assert lib.slio_aloam_run(None, L.fptr(xyz), 4, L.iptr(c5)) == EINVAL
    assert lib.slio_aloam_get_cloud(None, 0, L.fptr(out), 4) == EINVAL
    assert lib.slio_aloam_get_scan_index(None, L.iptr(i32), L.iptr(i32)) == EINVAL
    assert lib.slio_aloam_get_work(None, L.fptr(out), L.iptr(i32), L.u8ptr(u8)) == EINVAL
    assert lib.slio_aloam_get_view(None, C.byref(v)) == EINVAL
    assert b"null or destroyed handle" in lib.slio_last_error()
    assert lib.slio_aloam_tile(None, L.iptr(i32)) == EINVAL
    assert lib.slio_aloam_tile(L.iptr(i32), None) == EINVAL
    # the host entry
    none10 = [None] * 10
    assert lib.slio_aloam_register_host(None, L.fptr(xyz), 4, *none10, L.iptr(c5), None) == EINVAL
    assert lib.slio_aloam_register_host(C.byref(p), None, 4, *none10, L.iptr(c5), None) == EINVAL
    assert lib.slio_aloam_register_host(C.byref(p), L.fptr(xyz), -1, *none10, L.iptr(c5), None) == EINVAL
    assert lib.slio_aloam_register_host(C.byref(p), L.fptr(xyz), 4, *none10, None, None) == EINVAL
    p.max_points = 3
    assert lib.slio_aloam_register_host(C.byref(p), L.fptr(xyz), 4, *none10, L.iptr(c5), None) == ECAPACITY
    assert b"max_points" in lib.slio_last_error()
    p.max_points = 4
    assert lib.slio_aloam_register_host(C.byref(p), L.fptr(xyz), 4, *none10, L.iptr(c5), None) == 0
    assert list(c5) == [0] * 5                                    # four points at the origin: too close
    assert lib.slio_aloam_register_host(C.byref(p), None, 0, *none10, L.iptr(c5), None) == 0


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_aloam.cpp compiled with the host compiler and
    -fsanitize=address,undefined into a stand-alone program that drives the
    handler over sizes and shapes as above; run as a child process, nothing
    preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "aloam_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "aloam_host_main.cpp"), os.path.join(csrc, "slio_aloam.cpp"), "-o", exe]
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
