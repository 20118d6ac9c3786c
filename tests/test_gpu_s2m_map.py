"""GPU tests of the LIO-SAM keyframe store and local-map assembly
(mapOptmization.cpp extractCloud :1204-1251, saveKeyFramesAndFactor
:2069-2077, downsampleCurrentScan :1276-1288) against the oracle:
oracle.s2m_transform is pcl::getTransformation applied to a cloud, i.e.
transformPointCloud (:382-409), and oracle.voxel_grid(pcl_order=False) is the
device's VoxelGrid order, so the assembled map is compared bit for bit."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 63, 64, 65, 257, 1500, 300]   # empty; around the wavefront (64) and the block (256)
SELECTION = [6, 2, 0, 3, 6, 4, 1, 7]         # 5 unselected, 6 twice, 0 empty
LEAVES = (0.4, 0.2)                          # mappingSurfLeafSize, mappingCornerLeafSize


def key_pose(i):
    return np.array([0.02 * i, -0.03 * i, 0.4 * i, 1.5 * i, -0.7 * i, 0.05 * i], np.float32)


def pose_matrix(p):
    """pcl::getTransformation(x, y, z, roll, pitch, yaw): R = Rz Ry Rx."""
    r, pt, yw = (float(v) for v in p[:3])
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(pt), np.sin(pt), np.cos(yw), np.sin(yw)
    R = np.array([[cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr],
                  [sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr],
                  [-sp, cp * sr, cp * cr]])
    return R, np.asarray(p[3:], np.float64)


@pytest.fixture(scope="module")
def keyframes():
    """A jittered 12 m x 12 m ground patch seen from eight poses: keyframe i
    holds SIZES[i] points of it in the LiDAR frame of key_pose(i); every 97th
    point of keyframe 6 is NaN."""
    rng = np.random.default_rng(20261019)
    out = []
    for i, n in enumerate(SIZES):
        world = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.normal(0, 0.02, n)], 1)
        R, t = pose_matrix(key_pose(i))
        body = ((world - t) @ R).astype(np.float32)
        if i == 6:
            body[::97] = np.nan
        out.append(np.ascontiguousarray(body.reshape(-1, 3)))
    return out


def concatenation(oracle_mod, keyframes, selection, poses=None):
    parts, src = [np.zeros((0, 3), np.float32)], [np.zeros(0, np.int64)]
    for j, k in enumerate(selection):
        pose = key_pose(k) if poses is None else poses[j]
        if keyframes[k].shape[0]:
            parts.append(oracle_mod.s2m_transform(pose, keyframes[k]))
            src.append(np.full(keyframes[k].shape[0], k))
    return np.concatenate(parts).astype(np.float32), np.concatenate(src)


@pytest.fixture(scope="module")
def expected(oracle_mod, keyframes):
    """The concatenation over SELECTION and its VoxelGrid per leaf, computed
    once on the CPU and shared (never modified)."""
    cat, src = concatenation(oracle_mod, keyframes, SELECTION)
    assert cat.shape[0] == 3493
    maps = {leaf: oracle_mod.voxel_grid(cat, leaf) for leaf in LEAVES}
    # the in-voxel order is exercised: some voxel holds >= 3 points from >= 2 keyframes
    fin = np.isfinite(cat).all(axis=1)
    c, s = cat[fin], src[fin]
    inv = np.float32(1.0) / np.float32(0.4)
    ijk = np.floor(c * inv).astype(np.int64)
    ijk -= ijk.min(axis=0)
    vox = (ijk[:, 2] * (ijk[:, 1].max() + 1) + ijk[:, 1]) * (ijk[:, 0].max() + 1) + ijk[:, 0]
    mixed = 0
    for v in np.unique(vox):
        members = s[vox == v]
        mixed += members.size >= 3 and np.unique(members).size >= 2
    assert mixed >= 1
    assert 0 < maps[0.4].shape[0] < maps[0.2].shape[0] < cat.shape[0]
    return cat, maps


def push_all(s2m, keyframes):
    for i, kf in enumerate(keyframes):
        assert s2m.push_keyframe(kf, kf) == i


def sel_poses(selection):
    return np.stack([key_pose(k) for k in selection]) if len(selection) else np.zeros((0, 6), np.float32)


def map_download(L, h):
    lib = L.load()
    n = C.c_int64()
    dims = np.zeros(3, np.int32)
    cell = C.c_float()
    L.check(lib.slio_map_info(h, L.iptr(dims), C.byref(cell), C.byref(n)), "map_info")
    cap = max(n.value, 1)
    x, y, z = (np.zeros(cap, np.float32) for _ in range(3))
    ids = np.zeros(cap, np.uint32)
    got = C.c_int64()
    L.check(lib.slio_map_download(h, L.fptr(x), L.fptr(y), L.fptr(z), ids.ctypes.data_as(C.POINTER(C.c_uint32)),
                                  cap, C.byref(got)), "map_download")
    assert got.value == n.value
    np.testing.assert_array_equal(ids[:got.value], np.arange(got.value, dtype=np.uint32))
    return np.stack([x, y, z], 1)[:got.value]


def kf_download(L, h, key):
    lib = L.load()
    n = C.c_int64()
    assert lib.slio_s2m_kf_get(h, key, None, None, None, 0, C.byref(n)) in (0, -4)
    cap = max(n.value, 1)
    x, y, z = (np.zeros(cap, np.float32) for _ in range(3))
    L.check(lib.slio_s2m_kf_get(h, key, L.fptr(x), L.fptr(y), L.fptr(z), cap, C.byref(n)), "kf_get")
    return np.stack([x, y, z], 1)[:n.value]


def test_assembly_matches_oracle(L, oracle_mod, keyframes, expected):
    """extractCloud on the device == concatenation of oracle.s2m_transform over
    the selection through oracle.voxel_grid, bit for bit, for both leaves;
    the concatenation (3,493 points) is larger than max_points, which bounds
    the scan only."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    cat, maps = expected
    s2m = ScanToMap(max_points=2000)
    try:
        lib = L.load()
        push_all(s2m, keyframes)
        nk, npts = C.c_int32(), C.c_int64()
        L.check(lib.slio_s2m_kf_info(s2m.hs, C.byref(nk), C.byref(npts)), "kf_info")
        assert (nk.value, npts.value) == (len(SIZES), sum(SIZES))
        sizes = np.zeros(len(SIZES), np.int64)
        L.check(lib.slio_s2m_kf_sizes(s2m.hs, L.i64ptr(sizes), sizes.size), "kf_sizes")
        assert sizes.tolist() == SIZES
        np.testing.assert_array_equal(kf_download(L, s2m.hs, 6), keyframes[6])
        cc, cs = s2m.extract_cloud(SELECTION, sel_poses(SELECTION), corner_leaf=0.2, surf_leaf=0.4)
        assert cc == (cat.shape[0], maps[0.2].shape[0])
        assert cs == (cat.shape[0], maps[0.4].shape[0])
        np.testing.assert_array_equal(map_download(L, s2m.hc), maps[0.2])
        np.testing.assert_array_equal(map_download(L, s2m.hs), maps[0.4])
    finally:
        s2m.close()


def test_assembled_index_is_valid(L, keyframes, expected):
    """The index of the assembled map answers like the index slio_map_upload
    builds from the same points: cornerOptimization / surfOptimization of a
    small scan are bit-equal in sel and coeff (device against device, so ties
    cannot make it ambiguous; the upload path is pinned to the oracle by
    test_gpu_lio_s2m.py)."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    _, maps = expected
    rng = np.random.default_rng(3)
    scan = (maps[0.4][rng.choice(maps[0.4].shape[0], 500)] + rng.normal(0, 0.03, (500, 3))).astype(np.float32)
    tf = np.array([0.004, -0.003, 0.01, 0.05, -0.04, 0.02], np.float32)
    a, b = ScanToMap(max_points=2000), ScanToMap(max_points=2000)
    try:
        push_all(a, keyframes)
        a.extract_cloud(SELECTION, sel_poses(SELECTION), corner_leaf=0.2, surf_leaf=0.4)
        b.set_maps(maps[0.2], maps[0.4])
        res = []
        for s in (a, b):
            s.set_scan(scan, scan)
            nsel = (s.corner_optimization(tf), s.surf_optimization(tf))
            out = []
            for h in (s.hc, s.hs):
                coeff = np.zeros((scan.shape[0], 4), np.float32)
                sel = np.zeros(scan.shape[0], np.uint8)
                L.check(L.load().slio_s2m_get_coeffs(h, L.fptr(coeff), L.u8ptr(sel)), "get")
                out.append((coeff, sel))
            res.append((nsel, out))
        assert res[0][0] == res[1][0]
        assert res[0][0][1] > 100   # the ground patch is a plane: surf points are selected
        for k in range(2):
            np.testing.assert_array_equal(res[0][1][k][1], res[1][1][k][1])
            np.testing.assert_array_equal(res[0][1][k][0], res[1][1][k][0])
    finally:
        a.close()
        b.close()


def test_pass_through_and_empty(L, keyframes, expected):
    """Leaf 1e-5 is too small for the cloud: the concatenation passes through
    exactly as the scan path passes a scan through at that leaf (non-finite
    points included).  The empty keyframe alone, and an all-NaN keyframe, give
    an empty map; a normal assembly afterwards is unaffected."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    cat, maps = expected
    s2m = ScanToMap(max_points=4000)
    try:
        lib = L.load()
        push_all(s2m, keyframes)
        cc, cs = s2m.extract_cloud(SELECTION, sel_poses(SELECTION), corner_leaf=1e-5, surf_leaf=1e-5)
        assert cc == cs == (cat.shape[0], cat.shape[0])
        got = map_download(L, s2m.hs)
        n_down = s2m.downsample_current_scan(cat, cat, corner_leaf=1e-5, surf_leaf=1e-5)
        assert n_down == (cat.shape[0], cat.shape[0])
        x, y, z = (np.zeros(cat.shape[0], np.float32) for _ in range(3))
        L.check(lib.slio_scan_download(s2m.hs, L.fptr(x), L.fptr(y), L.fptr(z)), "scan_download")
        np.testing.assert_array_equal(got, np.stack([x, y, z], 1))
        np.testing.assert_array_equal(got, cat)
        assert np.isnan(got).any()
        # only the empty keyframe; no keyframe at all
        for sel in ([0], [0, 0], []):
            assert s2m.extract_cloud(sel, sel_poses(sel)) == ((0, 0), (0, 0))
            assert map_download(L, s2m.hs).shape == (0, 3)
        # a keyframe without a finite point
        bad = np.full((50, 3), np.nan, np.float32)
        bad[::7, 0] = np.inf
        k = s2m.push_keyframe(bad, bad)
        assert k == len(SIZES)
        assert s2m.extract_cloud([k], key_pose(1)[None]) == ((50, 0), (50, 0))
        assert map_download(L, s2m.hc).shape == (0, 3)
        s2m.extract_cloud(SELECTION, sel_poses(SELECTION), corner_leaf=0.2, surf_leaf=0.4)
        np.testing.assert_array_equal(map_download(L, s2m.hc), maps[0.2])
        np.testing.assert_array_equal(map_download(L, s2m.hs), maps[0.4])
    finally:
        s2m.close()


def test_argument_errors_on_a_live_handle(L, keyframes):
    """EINVAL / ESTATE with a message, and the store unchanged."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    s2m = ScanToMap(max_points=2000)
    try:
        lib = L.load()
        h = s2m.hs
        k = C.c_int32(-7)
        assert lib.slio_s2m_kf_push_scan(h, C.byref(k)) == -5 and b"no scan" in lib.slio_last_error()
        x = np.zeros(4, np.float32)
        assert lib.slio_s2m_kf_push(h, L.fptr(x), L.fptr(x), L.fptr(x), -1, C.byref(k)) == -1
        assert b"slio_s2m_kf_push" in lib.slio_last_error()
        assert lib.slio_s2m_kf_push(h, None, L.fptr(x), L.fptr(x), 4, C.byref(k)) == -1
        push_all(s2m, keyframes[:3])
        cnt = np.zeros(2, np.int64)
        pose = sel_poses([0, 1, 2])
        for bad in ([0, 3, 1], [0, -1, 1]):
            key = np.array(bad, np.int32)
            assert lib.slio_s2m_map_from_keyframes(h, L.iptr(key), L.fptr(pose), 3, 0.4, L.i64ptr(cnt)) == -1
            assert b"out of range" in lib.slio_last_error()
        key = np.array([0, 1, 2], np.int32)
        assert lib.slio_s2m_map_from_keyframes(h, L.iptr(key), L.fptr(pose), -1, 0.4, L.i64ptr(cnt)) == -1
        assert lib.slio_s2m_map_from_keyframes(h, L.iptr(key), L.fptr(pose), 3, 0.0, L.i64ptr(cnt)) == -1
        assert lib.slio_s2m_map_from_keyframes(h, None, L.fptr(pose), 3, 0.4, L.i64ptr(cnt)) == -1
        n = C.c_int64()
        assert lib.slio_s2m_kf_get(h, 3, None, None, None, 0, C.byref(n)) == -1
        assert lib.slio_s2m_kf_get(h, 2, None, None, None, 0, C.byref(n)) == -4 and n.value == SIZES[2]
        assert lib.slio_s2m_kf_sizes(h, None, 0) == -4
        nk = C.c_int32()
        L.check(lib.slio_s2m_kf_info(h, C.byref(nk), None), "kf_info")
        assert nk.value == 3
        s2m.clear_keyframes()
        L.check(lib.slio_s2m_kf_info(h, C.byref(nk), C.byref(n)), "kf_info")
        assert (nk.value, n.value) == (0, 0)
        assert s2m.push_keyframe(keyframes[4], keyframes[4]) == 0
    finally:
        s2m.close()


def test_kf_push_scan(L, oracle_mod, keyframes):
    """saveKeyFramesAndFactor: keyframes pushed from the handle's scan after
    downsampleCurrentScan download bit-equal to oracle.voxel_grid of the raw
    cloud; assembling the same selection twice gives the same bits (the second
    call rebuilds the handle's map in place, on cached buffers); a store
    holding the same keyframes in another arena order gives the same map."""
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    rng = np.random.default_rng(11)
    raws = []
    for i, n in enumerate((1500, 700, 2300)):
        raw = np.stack([rng.uniform(-6, 6, n), rng.uniform(-6, 6, n), rng.normal(0, 0.02, n)], 1).astype(np.float32)
        raw[5::211] = np.nan
        raws.append(raw)
    poses = np.stack([key_pose(i + 1) for i in range(3)])
    a, b = ScanToMap(max_points=4000), ScanToMap(max_points=4000)
    try:
        ds = []
        for i, raw in enumerate(raws):
            nc, ns = a.downsample_current_scan(raw, raw)
            assert a.save_keyframe() == i
            ds.append((oracle_mod.voxel_grid(raw, 0.2), oracle_mod.voxel_grid(raw, 0.4)))
            assert (nc, ns) == (ds[i][0].shape[0], ds[i][1].shape[0])
        for i in range(3):
            np.testing.assert_array_equal(kf_download(L, a.hc, i), ds[i][0])
            np.testing.assert_array_equal(kf_download(L, a.hs, i), ds[i][1])
        sel = [2, 0, 1, 0]
        first = a.extract_cloud(sel, poses[sel])
        m1 = (map_download(L, a.hc), map_download(L, a.hs))
        for kind, leaf in ((0, 0.2), (1, 0.4)):
            cat, _ = concatenation(oracle_mod, [d[kind] for d in ds], sel, poses[sel])
            np.testing.assert_array_equal(m1[kind], oracle_mod.voxel_grid(cat, leaf))
        assert a.extract_cloud(sel, poses[sel]) == first
        m2 = (map_download(L, a.hc), map_download(L, a.hs))
        # the other store: arena order 1, 2, 0
        order = [1, 2, 0]
        for k in order:
            b.push_keyframe(ds[k][0], ds[k][1])
        sel_b = [order.index(k) for k in sel]
        assert b.extract_cloud(sel_b, poses[sel]) == first
        m3 = (map_download(L, b.hc), map_download(L, b.hs))
        for k in range(2):
            np.testing.assert_array_equal(m2[k], m1[k])
            np.testing.assert_array_equal(m3[k], m1[k])
    finally:
        a.close()
        b.close()


def test_three_scan_sequence(L):
    """mapOptmization's per-scan order: downsampleCurrentScan,
    extractSurroundingKeyFrames' cloud assembly, scan2MapOptimization,
    saveKeyFramesAndFactor -- three times, the map coming from the keyframe
    store alone (first the bootstrap keyframes cut from the synthetic map, <=
    20k points each, then also the scans saved on the way).  Each solved pose
    stays within the tolerances test_normal_equations_and_convergence uses:
    0.05 m and 0.003 rad."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    p = synth.make_s2m_problem()
    tf_gt = p["tf"]
    t = tf_gt[3:].astype(np.float64)
    surf = p["surf_map"][np.linalg.norm(p["surf_map"][:, :2] - t[:2], axis=1) < 45.0]
    corner = p["corner_map"][np.linalg.norm(p["corner_map"][:, :2] - t[:2], axis=1) < 45.0]
    nkf = max(2, -(-surf.shape[0] // 20000))
    s2m = ScanToMap(max_points=60000)
    try:
        keys, poses = [], []
        for k in range(nkf):
            pose = np.array([0.01 * k, -0.02 * k, 0.3 * k, 2.0 * k, -1.0 * k, 0.1 * k], np.float32)
            R, tr = pose_matrix(pose)
            sk, ck = surf[k::nkf], corner[k::nkf]
            assert sk.shape[0] <= 20000 and ck.shape[0] <= 20000
            keys.append(s2m.push_keyframe(((ck - tr) @ R).astype(np.float32), ((sk - tr) @ R).astype(np.float32)))
            poses.append(pose)
        guesses = ([0.005, -0.004, 0.01, 0.15, -0.1, 0.05], [-0.004, 0.003, -0.008, -0.1, 0.12, -0.04],
                   [0.003, 0.005, -0.01, 0.08, 0.1, 0.06])
        for it, d in enumerate(guesses):
            nc, ns = s2m.downsample_current_scan(p["corner_scan"], p["surf_scan"][:20000])
            (_, mc), (_, ms) = s2m.extract_cloud(keys, np.stack(poses))
            tf = s2m.scan2MapOptimization(tf_gt + np.array(d, np.float32))
            err_t = np.abs(tf[3:] - tf_gt[3:]).max()
            err_r = np.abs(tf[:3] - tf_gt[:3]).max()
            print(f"scan {it}: scan {nc} / {ns} points, map {mc} / {ms} points from {len(keys)} keyframes, "
                  f"{s2m.iterations} iterations, |dt| {err_t:.4f} m, |dr| {err_r:.5f} rad")
            assert s2m.iterations >= 1
            assert err_t < 0.05 and err_r < 0.003
            keys.append(s2m.save_keyframe())
            poses.append(tf)
        assert keys == list(range(nkf + 3))
    finally:
        s2m.close()
