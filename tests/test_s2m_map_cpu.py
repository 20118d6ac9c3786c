"""CPU tests of the LIO-SAM keyframe store / local-map entries
(include/slio.h, s2m section) and of lio_sam.extract_nearby
(mapOptmization.cpp extractNearby :1152-1193 with extractCloud's distance
check :1211).  No GPU: without a device no handle exists, so the argument
checks reachable here are the ones made before the handle is touched; the
others (a key out of range on a live handle, ...) are in
test_gpu_s2m_map.py::test_argument_errors_on_a_live_handle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NEW = ["slio_s2m_kf_push", "slio_s2m_kf_push_scan", "slio_s2m_kf_info", "slio_s2m_kf_sizes",
       "slio_s2m_kf_clear", "slio_s2m_kf_get", "slio_s2m_map_from_keyframes"]


@pytest.fixture(scope="module")
def lib():
    from agi_lidar_slam_amd import build, _lib
    build.build()
    return _lib.load()


def test_new_symbols_are_bound(lib):
    from agi_lidar_slam_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "slio.h")).read()
    for name in NEW:
        assert name + "(" in hdr
        assert name in _lib.SIGNATURES
        fn = getattr(lib, name)
        assert fn.argtypes == _lib.SIGNATURES[name][1]


def test_argument_errors_before_any_device_call(lib):
    """A null handle (with otherwise valid or invalid arguments: negative n,
    a key out of range, nsel < 0) is EINVAL with a message, and nothing
    touches the device -- this machine has none."""
    from agi_lidar_slam_amd import _lib as L
    x = np.zeros(4, np.float32)
    k, n, nk = C.c_int32(), C.c_int64(), C.c_int32()
    key = np.array([0, 5], np.int32)
    pose = np.zeros((2, 6), np.float32)
    cnt = np.zeros(2, np.int64)
    calls = [
        lambda: lib.slio_s2m_kf_push(None, L.fptr(x), L.fptr(x), L.fptr(x), 4, C.byref(k)),
        lambda: lib.slio_s2m_kf_push(None, L.fptr(x), L.fptr(x), L.fptr(x), -1, C.byref(k)),
        lambda: lib.slio_s2m_kf_push_scan(None, C.byref(k)),
        lambda: lib.slio_s2m_kf_info(None, C.byref(nk), C.byref(n)),
        lambda: lib.slio_s2m_kf_sizes(None, L.i64ptr(cnt), 2),
        lambda: lib.slio_s2m_kf_clear(None),
        lambda: lib.slio_s2m_kf_get(None, 5, L.fptr(x), L.fptr(x), L.fptr(x), 4, C.byref(n)),
        lambda: lib.slio_s2m_map_from_keyframes(None, L.iptr(key), L.fptr(pose), 2, 0.4, L.i64ptr(cnt)),
        lambda: lib.slio_s2m_map_from_keyframes(None, L.iptr(key), L.fptr(pose), -1, 0.4, L.i64ptr(cnt)),
    ]
    for call in calls:
        lib.slio_iterate_async(None, None, 1, 0, None)   # leaves another message behind
        assert call() == -1
        assert b"null handle" in lib.slio_last_error()


def brute_extract_nearby(P, T, t_cur, radius, density):
    """extractNearby + extractCloud's check restated with plain loops."""
    f = np.float32
    P = np.asarray(P, f)
    n = len(P)
    back = P[-1]

    def d2(a, b):
        return f(f(f(a[0] - b[0]) * f(a[0] - b[0]) + f(a[1] - b[1]) * f(a[1] - b[1])) + f(a[2] - b[2]) * f(a[2] - b[2]))

    near = sorted((i for i in range(n) if d2(P[i], back) < f(radius) * f(radius)), key=lambda i: (d2(P[i], back), i))
    inv = f(1.0) / f(density)
    mn = [min(P[i][a] for i in near) for a in range(3)]
    mx = [max(P[i][a] for i in near) for a in range(3)]
    minb = [int(np.floor(f(mn[a] * inv))) for a in range(3)]
    div = [int(np.floor(f(mx[a] * inv))) - minb[a] + 1 for a in range(3)]
    vox = {}
    for i in near:
        ijk = [int(f(np.floor(f(P[i][a] * inv))) - f(minb[a])) for a in range(3)]
        vox.setdefault(ijk[0] + ijk[1] * div[0] + ijk[2] * div[0] * div[1], []).append(i)
    entries = []
    for v in sorted(vox):
        s = np.zeros(3, f)
        for i in vox[v]:
            s = s + P[i]
        c = s / f(len(vox[v]))
        best = min(range(n), key=lambda i: (d2(P[i], c), i))
        entries.append((best, c))
    for i in range(n - 1, -1, -1):
        if t_cur - T[i] < 10.0:
            entries.append((i, P[i]))
        else:
            break
    return [k for k, p in entries if not np.sqrt(d2(p, back)) > f(radius)]


def test_extract_nearby():
    """A 40-pose trajectory along +x, 2.5 m apart (so one pose per 2 m voxel),
    stamps 4 s apart, every coordinate a dyadic fraction so that no distance
    below is rounded.  Pose 1 lies far beyond the radius; poses 20 and 21 are
    0.5 m apart, closer than `density`, in one voxel; the last three poses are
    inside the 10 s window."""
    from agi_lidar_slam_amd.lio_sam import extract_nearby
    P = np.zeros((40, 3), np.float32)
    P[:, 0] = 2.5 * np.arange(40) + 0.25
    P[:, 1] = 0.25
    P[:, 2] = 0.125
    P[1] = [-400.0, 30.0, 0.0]
    P[21] = P[20] + np.array([0.5, 0.0, 0.0], np.float32)
    assert np.floor(P[20, 0] / 2.0) == np.floor(P[21, 0] / 2.0)
    T = 4.0 * np.arange(40, dtype=np.float64)
    t_cur = T[-1] + 1.0                  # 1, 5, 9 s after the last three poses
    got = extract_nearby(P, T, t_cur, radius=49.0, density=2.0)
    assert got.dtype == np.int32
    # within 49 m of pose 39 (x 97.75): poses 20..39 (pose 19, x 47.75, is 50 m
    # away).  Voxels in ascending x: {20, 21} share one, and their centroid (x
    # 50.5) is exactly as far from pose 20 as from pose 21 -- the lower index
    # (the documented tie rule) -- then 22..39, one voxel each; then the 10 s
    # tail, newest first, duplicates kept.  :1211 drops nothing.
    literal = [20, 22, 23, 24, 25, 26, 27, 28, 29, 30, 31, 32, 33, 34, 35, 36, 37, 38, 39, 39, 38, 37]
    assert got.tolist() == literal
    assert brute_extract_nearby(P, T, t_cur, 49.0, 2.0) == literal
    # smaller radii: the radius search and the :1211 check against the brute force
    for r in (10.0, 26.0, 4.0):
        assert extract_nearby(P, T, t_cur, radius=r, density=2.0).tolist() == brute_extract_nearby(P, T, t_cur, r, 2.0)
    # radius 4 m: only poses 38, 39 are near; the tail's pose 37 (5 m away) is dropped by :1211
    assert extract_nearby(P, T, t_cur, radius=4.0, density=2.0).tolist() == [38, 39, 39, 38]
    assert extract_nearby(np.zeros((0, 3)), np.zeros(0), 0.0).size == 0
    assert extract_nearby(np.zeros((1, 3)), np.zeros(1), 1.0).tolist() == [0, 0]
