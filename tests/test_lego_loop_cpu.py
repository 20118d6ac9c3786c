"""CPU tests of LeGO-LOAM's loop closure host code (slio_lmap_detect_loop,
slio_lmap_loop_correction, the recent-keyframe list of lego_map.py) against
the numpy restatement (tests/lego_loop_model.py), and a sanitizer run of the
same host code with the shared ICP step in a stand-alone program
(tests/lego_loop_host_main.cpp).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import icp_model  # noqa: E402
import lego_loop_model as LM  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd import lego_map  # noqa: E402

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    from agi_lidar_slam_amd import build
    build.build()
    return L.load()


def detect(lib, xyz, times, cur, t, radius=5.0, time_diff=30.0):
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    times = np.ascontiguousarray(times, np.float64)
    cur = np.ascontiguousarray(cur, F)
    out = C.c_int32(-7)
    L.check(lib.slio_lmap_detect_loop(L.fptr(xyz), L.dptr(times), xyz.shape[0], L.fptr(cur), float(t), radius,
                                      time_diff, C.byref(out)), "detect_loop")
    return out.value


# ------------------------------------------------------------------ detection
def test_detection_ascending_distance_and_30s_rule(lib):
    rng = np.random.default_rng(5)
    hits = set()
    for trial in range(200):
        n = int(rng.integers(1, 40))
        xyz = rng.uniform(-6, 6, (n, 3)).astype(F)
        times = np.sort(rng.uniform(0, 100, n))
        cur = rng.uniform(-3, 3, 3).astype(F)
        t = float(rng.uniform(0, 130))
        want = LM.detect_loop(xyz, times, cur, t)
        assert detect(lib, xyz, times, cur, t) == want
        hits.add(want >= 0)
    assert hits == {True, False}
    # the nearest key is too recent, the second nearest is not: the second wins
    xyz = np.array([[0.1, 0, 0], [1, 0, 0], [2, 0, 0], [9, 0, 0]], F)
    assert detect(lib, xyz, [99.0, 10.0, 0.0, 0.0], [0, 0, 0], 100.0) == 1
    # exactly 30 s is not enough (the test is `>`), and the radius test is `<`
    assert detect(lib, xyz, [99.0, 70.0, 69.0, 0.0], [0, 0, 0], 100.0) == 2
    assert detect(lib, [[5.0, 0, 0]], [0.0], [0, 0, 0], 100.0) == -1
    assert detect(lib, [[np.nextafter(F(5.0), F(0)), 0, 0]], [0.0], [0, 0, 0], 100.0) == 0


def test_detection_no_candidate_and_equal_distances(lib):
    assert detect(lib, np.zeros((0, 3)), [], [0, 0, 0], 50.0) == -1
    assert LM.detect_loop(np.zeros((0, 3)), [], [0, 0, 0], 50.0) == -1
    xyz = np.array([[3, 0, 0], [0, 3, 0], [0, 0, -3], [-3, 0, 0]], F)   # four keys at exactly 3 m
    for times, want in (([0, 0, 0, 0], 0), ([40, 0, 0, 0], 1), ([40, 45, 29, 0], 2), ([40, 45, 45, 45], -1)):
        assert LM.detect_loop(xyz, times, [0, 0, 0], 60.0) == want
        assert detect(lib, xyz, times, [0, 0, 0], 60.0) == want


# ------------------------------------------------------------------ the recent list
def drive(calls, search_num=50):
    """calls: the number of keys at each extractSurroundingKeyFrames call, or
    "correct" for a correctPoses in between.  Returns the lists of the library's
    function and of the model after every call."""
    model = LM.RecentList(search_num)
    recent, latest = [], 0
    out = []
    for c in calls:
        if c == "correct":
            model.correct_poses()
            recent = []
            continue
        recent, latest = lego_map.recent_keyframes(recent, latest, c, search_num)
        want = model.update(c)
        assert recent == want and latest == model.latest_frame_id, (c, recent, want)
        out.append(list(recent))
    return out


def test_recent_list_to_52_keys():
    # a new key before every call
    lists = drive(range(1, 53))
    assert lists[48] == list(range(49)) and lists[49] == list(range(50))
    # the first call after the list reached 50 entries: latestFrameID is still 0,
    # so the oldest entry goes and key 50 is appended
    assert lists[50] == list(range(1, 51))
    assert lists[51] == list(range(2, 52))
    # no new key between two calls once the list is full: the pop-and-duplicate case
    lists = drive([49, 50, 50, 50, 51, 51, 52])
    assert lists[1] == list(range(50))
    assert lists[2] == list(range(1, 50)) + [49]        # key 49 is already the last entry
    assert lists[3] == lists[2]                         # latestFrameID caught up: nothing moves
    assert lists[4] == list(range(2, 50)) + [49, 50]
    assert lists[5] == lists[4]
    assert lists[6] == list(range(3, 50)) + [49, 50, 51]
    # below 50 the whole list is rebuilt at every call, new key or not
    assert drive([3, 3, 5]) == [[0, 1, 2], [0, 1, 2], [0, 1, 2, 3, 4]]


def test_recent_list_across_correct_poses():
    lists = drive([50, 51, 52, "correct", 52, 53, 53])
    assert lists[2] == list(range(2, 52))
    # cleared: refilled from the newest 50; latestFrameID (51) is not touched by the refill
    assert lists[3] == list(range(2, 52))
    assert lists[4] == list(range(3, 53))
    assert lists[5] == lists[4]
    lists = drive([10, "correct", 10, 11])
    assert lists == [list(range(10)), list(range(10)), list(range(11))]
    # a small search_num shows the same steps
    assert drive([1, 2, 3, 4, 4, 5], 3) == [[0], [0, 1], [0, 1, 2], [1, 2, 3], [1, 2, 3], [2, 3, 4]]


# ------------------------------------------------------------------ the correction
def correction(lib, T, latest, closest, fitness):
    T = np.ascontiguousarray(np.asarray(T, F).reshape(16))
    a, b = np.ascontiguousarray(latest, F), np.ascontiguousarray(closest, F)
    pf, pt, noise = np.empty(6, F), np.empty(6, F), C.c_float()
    L.check(lib.slio_lmap_loop_correction(L.fptr(T), L.fptr(a), L.fptr(b), float(fitness), L.fptr(pf), L.fptr(pt),
                                          C.byref(noise)), "loop_correction")
    return pf, pt, F(noise.value)


def test_correction_bit_exact(lib):
    rng = np.random.default_rng(11)
    cases = [(np.eye(4, dtype=F), np.array([0.01, 0.7, -0.02, 1.5, -0.2, 2.5], F), np.zeros(6, F), 0.125)]
    for _ in range(50):
        T = np.eye(4, dtype=F)
        T[:3, :3] = icp_model.rot_zyx(*rng.uniform(-0.2, 0.2, 3)).astype(F)
        T[:3, 3] = rng.uniform(-1, 1, 3)
        cases.append((T, np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-20, 20, 3)]).astype(F),
                      np.concatenate([rng.uniform(-3, 3, 3), rng.uniform(-20, 20, 3)]).astype(F),
                      float(rng.uniform(0, 0.3))))
    for T, latest, closest, fit in cases:
        pf, pt, noise = correction(lib, T, latest, closest, fit)
        wf, wt, wn = LM.loop_correction(T, latest, closest, fit)
        assert pf.tobytes() == wf.tobytes(), (pf, wf)
        assert pt.tobytes() == wt.tobytes()
        assert noise.tobytes() == wn.tobytes()
    # the identity: the latest key's own pose in GTSAM's order, up to the trigonometry's rounding
    pf, pt, _ = correction(lib, *cases[0][:3], 0.0)
    np.testing.assert_allclose(LM.table_pose(pf), cases[0][1], atol=1e-6)
    assert pt.tobytes() == np.zeros(6, F).tobytes()


# ------------------------------------------------------------------ errors
def test_argument_errors(lib):
    xyz, tm, cur, out = np.zeros((2, 3), F), np.zeros(2), np.zeros(3, F), C.c_int32()
    assert lib.slio_lmap_detect_loop(None, L.dptr(tm), 2, L.fptr(cur), 0.0, 5.0, 30.0, C.byref(out)) == EINVAL
    assert lib.slio_lmap_detect_loop(L.fptr(xyz), None, 2, L.fptr(cur), 0.0, 5.0, 30.0, C.byref(out)) == EINVAL
    assert lib.slio_lmap_detect_loop(L.fptr(xyz), L.dptr(tm), -1, L.fptr(cur), 0.0, 5.0, 30.0, C.byref(out)) == EINVAL
    assert lib.slio_lmap_detect_loop(L.fptr(xyz), L.dptr(tm), 2, None, 0.0, 5.0, 30.0, C.byref(out)) == EINVAL
    assert lib.slio_lmap_detect_loop(L.fptr(xyz), L.dptr(tm), 2, L.fptr(cur), 0.0, -1.0, 30.0, C.byref(out)) == EINVAL
    assert lib.slio_lmap_detect_loop(L.fptr(xyz), L.dptr(tm), 2, L.fptr(cur), 0.0, 5.0, 30.0, None) == EINVAL
    assert b"slio_lmap_detect_loop" in lib.slio_last_error()
    T, p, o, n = np.eye(4, dtype=F).reshape(16), np.zeros(6, F), np.empty(6, F), C.c_float()
    assert lib.slio_lmap_loop_correction(None, L.fptr(p), L.fptr(p), 0.0, L.fptr(o), L.fptr(o), C.byref(n)) == EINVAL
    assert lib.slio_lmap_loop_correction(L.fptr(T), None, L.fptr(p), 0.0, L.fptr(o), L.fptr(o), C.byref(n)) == EINVAL
    assert lib.slio_lmap_loop_correction(L.fptr(T), L.fptr(p), L.fptr(p), 0.0, None, L.fptr(o), C.byref(n)) == EINVAL
    assert lib.slio_lmap_loop_correction(L.fptr(T), L.fptr(p), L.fptr(p), 0.0, L.fptr(o), L.fptr(o), None) == EINVAL
    # entries that take a mapper or a handle check it before any device call
    assert lib.slio_lmap_set_key_poses(None, L.fptr(p), 1) == EINVAL
    assert lib.slio_lmap_loop_clouds(None, 0, 0, 1, 0.4, None) == EINVAL
    prm, st = L.SlioIcpParams(), L.SlioIcpState()
    assert lib.slio_icp_align(None, C.byref(prm), None, 1.0, 0, C.byref(st), None, None) == EINVAL


# ------------------------------------------------------------------ sanitizers
def test_host_code_under_asan_and_ubsan(tmp_path):
    """slio_lmap.cpp and slio_s2m.cpp (with slio_icp.hpp) compiled with the
    host compiler and -fsanitize=address,undefined into a stand-alone program;
    run as a child process, nothing preloaded."""
    cxx = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    csrc = os.path.join(ROOT, "agi_lidar_slam_amd", "csrc")
    exe = str(tmp_path / "lego_loop_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-I", csrc,
           os.path.join(ROOT, "tests", "lego_loop_host_main.cpp"), os.path.join(csrc, "slio_lmap.cpp"),
           os.path.join(csrc, "slio_s2m.cpp"), "-o", exe]
    b = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if b.returncode != 0:
        b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert r.stdout.strip().endswith("ok")
