"""GPU tests of LeGO-LOAM's loop closure on the device (include/slio.h:
slio_lmap_loop_clouds, slio_lmap_set_key_poses, LegoMapping(loop_closure=True)
and performLoopClosure) against tests/lego_loop_model.py: the loop clouds and
the recent-list local maps bit for bit, the device ICP loop against the
lockstep loop bit for bit and against the float64 restatement, the correction
to the bit, and correctPoses through a stub graph.  The scenario is built
without the front-end: ten keyframes cut from one synthetic room in the camera
frame, on a circle, the last one beside the first with its stored pose off by
0.3 m and 2 degrees."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_model  # noqa: E402
import lego_loop_model as LM  # noqa: E402
import lego_map_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ECAPACITY = -1, -4
CORNER, SURF_TOTAL, SURF, OUTLIER, LOOP = 0, 1, 2, 3, 4
NKEYS = 10


@pytest.fixture(scope="module")
def L():
    from agi_lidar_slam_amd import build, _lib
    build.build()
    return _lib


# ------------------------------------------------------------------ the scenario (CPU only)
def room(rng):
    """World points in the camera frame (y up): the floor y = -1.5, four walls
    and two boxes (surf pool); the vertical edges of the room and the boxes
    (corner pool); scattered points (outlier pool)."""
    def rect(n, lo, hi, axis, at):
        p = rng.uniform(lo, hi, (n, 3))
        p[:, axis] = at + rng.normal(0, 0.01, n)
        return p

    lo, hi = np.array([-7.0, -1.5, -9.0]), np.array([7.0, 1.5, 9.0])
    surf = [rect(2500, lo, hi, 1, -1.5), rect(900, lo, hi, 0, -7.0), rect(900, lo, hi, 0, 7.0),
            rect(700, lo, hi, 2, -9.0), rect(700, lo, hi, 2, 9.0)]
    boxes = [(np.array([2.0, -1.5, 4.0]), np.array([3.0, 0.5, 5.2])),
             (np.array([-4.0, -1.5, -5.0]), np.array([-3.2, 1.0, -3.5]))]
    edges = [(x, z) for x in (-7.0, 7.0) for z in (-9.0, 9.0)]
    for b0, b1 in boxes:
        for axis in (0, 2):
            for at in (b0[axis], b1[axis]):
                surf.append(rect(150, b0, b1, axis, at))
        edges += [(x, z) for x in (b0[0], b1[0]) for z in (b0[2], b1[2])]
    corner = []
    for x, z in edges:
        n = 60
        corner.append(np.column_stack([x + rng.normal(0, 0.01, n), rng.uniform(-1.5, 1.0, n),
                                       z + rng.normal(0, 0.01, n)]))
    outlier = rng.uniform(lo, hi, (400, 3))
    return np.concatenate(corner), np.concatenate(surf), outlier


def to_sensor(pose, pw):
    """The inverse of lego_map_model.to_map in float64, rounded to float32."""
    rx, ry, rz, tx, ty, tz = (float(v) for v in pose)
    q = np.asarray(pw, np.float64) - np.array([tx, ty, tz])
    cr, sr, cp, sp, cy, sy = math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz), math.sin(rz)
    x2 = cp * q[:, 0] - sp * q[:, 2]
    z2 = sp * q[:, 0] + cp * q[:, 2]
    y2 = q[:, 1]
    y1 = cr * y2 + sr * z2
    z1 = -sr * y2 + cr * z2
    x = cy * x2 + sy * y1
    y = -sy * x2 + cy * y1
    return np.column_stack([x, y, z1]).astype(F)


def scenario():
    """True and stored poses, stamps and the raw clouds per key (corner, surf,
    outlier; a few hundred points each, within 12 m of the key)."""
    rng = np.random.default_rng(20261021)
    pools = room(rng)
    true, stored, stamps, clouds = [], [], [], []
    for k in range(NKEYS):
        th = 2.0 * math.pi * k / NKEYS
        pose = np.array([0.01 * math.sin(3 * th), 0.5 * math.pi - th, -0.008 * math.cos(2 * th),
                         3.0 * math.cos(th), 0.02 * k, 3.0 * math.sin(th)], F)
        true.append(pose)
        s = pose.copy()
        if k == NKEYS - 1:
            s = (s + np.array([0.0, math.radians(2.0), 0.0, 0.22, 0.03, -0.2], F)).astype(F)
        stored.append(s)
        stamps.append(5.0 * k)
        cl = []
        for pool, n in zip(pools, (150, 600, 60)):
            near = pool[np.linalg.norm(pool - pose[3:6].astype(np.float64), axis=1) < 12.0]
            cl.append(to_sensor(pose, near[rng.choice(near.shape[0], n, replace=False)]))
        clouds.append(cl)
    return true, stored, stamps, clouds


@pytest.fixture(scope="module")
def case(oracle_mod):
    """The scenario, the keyframes the stores will hold (the feed's VoxelGrids,
    from the oracle) and the model's loop closure on them, computed once.  The
    conditions the bit comparisons rest on are asserted here, on the CPU."""
    vg = oracle_mod.voxel_grid
    true, stored, stamps, clouds = scenario()
    kfs = [(vg(c, 0.2), vg(s, 0.4), vg(o, 0.4)) for c, s, o in clouds]
    for kf in kfs:
        assert 300 < sum(a.shape[0] for a in kf) < 1200   # a few hundred points per key
    latest = NKEYS - 1
    xyz = np.array([p[3:6] for p in stored], F)
    closest = LM.detect_loop(xyz, stamps, stored[latest][3:6], stamps[latest])
    assert closest == 0
    d = np.linalg.norm(xyz[latest] - xyz[0])
    assert d < 5.0
    off = stored[latest].astype(np.float64) - true[latest]
    assert 0.25 < np.linalg.norm(off[3:6]) < 0.35 and abs(math.degrees(off[1]) - 2.0) < 0.01
    src, cat, tgt = LM.loop_clouds(vg, kfs, stored, latest, closest, 2)
    r64 = icp_model.icp_run(src, tgt, 100.0)
    r32 = icp_model.icp_run(src, tgt, 100.0, dtype=np.float32)
    # no exact nearest tie in any pass of the model's run
    assert not r64["ties"]
    assert r64["converged"] and r64["fitness"] <= 0.3, (r64["iterations"], r64["state"], r64["fitness"])
    # the VoxelGrid's output as a search target: no two of a source point's six
    # nearest at the same float distance (lego_map_model.tie_free), at the start
    # and at the end of the run
    tree = oracle_mod.Tree(tgt)
    for T in (np.eye(4, dtype=F), r64["final_T"]):
        _, sqd6 = tree.knn(icp_model.transform32(T, src), 6)
        assert M.tie_free(sqd6)
    return dict(true=true, stored=stored, stamps=stamps, clouds=clouds, kfs=kfs, latest=latest, closest=closest,
                src=src, tgt=tgt, r64=r64, r32=r32)


# ------------------------------------------------------------------ device helpers
def same_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    np.testing.assert_array_equal(g.view(np.uint32), w.view(np.uint32), err_msg=what)


def build_mapper(L, case, graph=None, **kw):
    """A LegoMapping(loop_closure=True) whose stores hold the scenario's keys:
    slio_lmap_feed_host, then saveKeyFramesAndFactor at the stored pose."""
    from agi_lidar_slam_amd.lego_map import LegoMapping
    mp = LegoMapping(max_points=4096, loop_closure=True, **kw)
    mp.graph = graph
    for k in range(NKEYS):
        xyzi = [np.column_stack([c, np.zeros(c.shape[0], F)]).astype(F) for c in case["clouds"][k]]
        mp.downsampleCurrentScan(clouds=xyzi)
        mp._tobe = case["stored"][k].copy()
        mp._aft = case["stored"][k].copy()
        mp.timeLaserOdometry = case["stamps"][k]
        assert mp.saveKeyFramesAndFactor()
    return mp


def loop_scan(L, mp):
    h, n = mp.handle(LOOP), int(mp.loop_counts[1])
    out = np.empty((3, max(n, 1)), F)
    L.check(L.load().slio_scan_download(h, L.fptr(out[0]), L.fptr(out[1]), L.fptr(out[2])), "scan_download")
    return np.ascontiguousarray(out[:, :n].T)


def loop_map(L, mp):
    h, cap = mp.handle(LOOP), max(int(mp.loop_counts[3]), 1)
    out, ids, n = np.empty((3, cap), F), np.empty(cap, np.uint32), C.c_int64()
    L.check(L.load().slio_map_download(h, L.fptr(out[0]), L.fptr(out[1]), L.fptr(out[2]),
                                       ids.ctypes.data_as(C.POINTER(C.c_uint32)), cap, C.byref(n)), "map_download")
    order = np.argsort(ids[:n.value], kind="stable")
    return np.ascontiguousarray(out[:, :n.value].T[order])


@pytest.fixture(scope="module")
def mapper(L, case):
    mp = build_mapper(L, case)
    yield mp
    mp.close()


# ------------------------------------------------------------------ tests
def test_stores_hold_the_models_keyframes(L, case, mapper):
    for k in (0, 4, NKEYS - 1):
        for which, want in zip((CORNER, SURF, OUTLIER), case["kfs"][k]):
            same_bits(mapper.keyframe(which, k), want, f"key {k} store {which}")
    assert mapper.keyTimes == case["stamps"]
    same_bits(mapper.cloudKeyPoses6D, np.array(case["stored"]))


@pytest.mark.parametrize("closest,search_num", [(0, 2), (0, 25), (1, 1), (7, 3)])
def test_loop_clouds_bit_exact(L, oracle_mod, case, mapper, closest, search_num):
    """search_num 2 around key 0: clipped at key 0, without the latest key; 25:
    every key, the latest included; (7, 3): clipped at the latest key."""
    latest = case["latest"]
    src, cat, tgt = LM.loop_clouds(oracle_mod.voxel_grid, case["kfs"], case["stored"], latest, closest, search_num)
    cnt = mapper.loop_clouds(latest, closest, search_num)
    assert list(cnt) == [src.shape[0], src.shape[0], cat.shape[0], tgt.shape[0]]
    same_bits(loop_scan(L, mapper), src, "source")
    same_bits(loop_map(L, mapper), tgt, "target")
    keys = [k for k in range(closest - search_num, closest + search_num + 1) if 0 <= k <= latest]
    assert (latest in keys) == (search_num == 25 or closest == 7)


def test_loop_clouds_errors(L, case, mapper):
    lib, cnt = L.load(), np.zeros(4, np.int64)
    for latest, closest, sn, leaf in ((NKEYS, 0, 2, 0.4), (-1, 0, 2, 0.4), (9, NKEYS, 2, 0.4), (9, -1, 2, 0.4),
                                      (9, 0, -1, 0.4), (9, 0, 2, 0.0)):
        assert lib.slio_lmap_loop_clouds(mapper.m, latest, closest, sn, leaf, L.i64ptr(cnt)) == EINVAL
    from agi_lidar_slam_amd.lego_map import LegoMapping
    small = LegoMapping(max_points=200)
    try:
        # corner and surf clouds that each fit the scan capacity, but not together
        g = np.stack(np.meshgrid(np.arange(12), np.arange(12), [0.0]), -1).reshape(-1, 3).astype(F)
        xyzi = np.column_stack([g, np.zeros(g.shape[0], F)]).astype(F)
        cnts = small.downsampleCurrentScan(clouds=(xyzi, xyzi[:100], xyzi[:0]))
        assert cnts[CORNER] == 144 and cnts[SURF] == 100
        key = C.c_int32()
        L.check(lib.slio_lmap_save_keyframe(small.m, L.fptr(np.zeros(6, F)), C.byref(key)), "save_keyframe")
        assert lib.slio_lmap_loop_clouds(small.m, 0, 0, 0, 0.4, L.i64ptr(cnt)) == ECAPACITY
    finally:
        small.close()


def test_set_key_poses(L, case):
    mp = build_mapper(L, case)
    try:
        lib = L.load()
        t = np.ascontiguousarray(np.array(case["stored"], F))
        assert lib.slio_lmap_set_key_poses(mp.m, L.fptr(t), NKEYS - 1) == EINVAL
        assert lib.slio_lmap_set_key_poses(mp.m, L.fptr(np.zeros((NKEYS + 1, 6), F)), NKEYS + 1) == EINVAL
        assert lib.slio_lmap_set_key_poses(mp.m, None, NKEYS) == EINVAL
        t2 = (t + F(0.125)).astype(F)
        mp.set_key_poses(t2)
        got, nk = np.empty((NKEYS, 6), F), C.c_int32()
        L.check(lib.slio_lmap_get_key_poses(mp.m, L.fptr(got), NKEYS, C.byref(nk)), "get_key_poses")
        same_bits(got, t2)
        same_bits(mp.cloudKeyPoses3D[:, :3], t2[:, 3:6])
    finally:
        mp.close()


def local_maps_of(L, mp):
    return mp.map_points(0), mp.map_points(1)


def test_recent_list_assembly_differs_from_radius_search(L, oracle_mod, case, mapper):
    """loop_closure=True with fewer than 50 keys: the local maps are the
    recent list's (every key, ascending), bit for bit -- not those of the
    radius-search branch, whose key order is another on this scenario."""
    from agi_lidar_slam_amd.lego_map import extract_surrounding
    mapper.currentRobotPosPoint = case["stored"][-1][3:6].copy()
    cnt = mapper.extractSurroundingKeyFrames()
    assert mapper.recentKeyFrames == list(range(NKEYS))
    cc, sc, cmap, smap = LM.local_maps(oracle_mod.voxel_grid, case["kfs"], case["stored"], range(NKEYS))
    assert list(cnt) == [cc.shape[0], cmap.shape[0], sc.shape[0], smap.shape[0]]
    got_c, got_s = local_maps_of(L, mapper)
    same_bits(got_c, cmap, "corner map")
    same_bits(got_s, smap, "surf map")
    old_keys, _ = extract_surrounding(mapper.cloudKeyPoses3D, mapper.currentRobotPosPoint, [])
    assert old_keys != list(range(NKEYS))
    _, _, ocmap, osmap = LM.local_maps(oracle_mod.voxel_grid, case["kfs"], case["stored"], old_keys)
    assert ocmap.shape != cmap.shape or not np.array_equal(ocmap, cmap)
    assert osmap.shape != smap.shape or not np.array_equal(osmap, smap)


class StubGraph:
    """The seam where GTSAM binds: the key pose is the odometry's, and a loop
    moves the latest key to pose_from and leaves the others."""

    def __init__(self):
        self.table, self.loops = [], []

    def add_keyframe(self, key, pose_from6, pose_to6):
        assert key == len(self.table) and (pose_from6 is None) == (key == 0)
        self.table.append(np.array(pose_to6, F))
        return self.table[-1]

    def add_loop(self, closure):
        self.loops.append(closure)
        self.table[closure.latest] = LM.table_pose(closure.pose_from)
        return np.array(self.table, F)


def test_perform_loop_closure_end_to_end(L, oracle_mod, case):
    """historyKeyframeSearchNum = 2, so that the target leaves the latest key
    out and the ICP has the 0.3 m / 2 degrees to find."""
    r64, r32 = case["r64"], case["r32"]
    latest, closest = case["latest"], case["closest"]
    graph = StubGraph()
    mp = build_mapper(L, case, graph=graph)
    try:
        same_bits(np.array(graph.table), np.array(case["stored"]))
        mp.currentRobotPosPoint = case["stored"][latest][3:6].copy()
        mp.extractSurroundingKeyFrames()
        old_maps = local_maps_of(L, mp)
        # the lockstep loop first (no graph: the closure is only returned)
        mp.graph = None
        lock = mp.performLoopClosure(lockstep=True, search_num=2)
        mp.graph = graph
        lock_T, lock_fit, lock_far = mp.loop_final_T.copy(), mp.loop_fitness, mp.icp_far_first
        assert not mp.aLoopIsClosed and lock is not None
        dev = mp.performLoopClosure(lockstep=False, search_num=2)
        assert dev is not None and mp.aLoopIsClosed and len(graph.loops) == 1 and graph.loops[0] is dev
        # device loop == lockstep loop, to the bit
        assert mp.loop_final_T.tobytes() == lock_T.tobytes()
        assert (mp.loop_fitness, mp.icp_far_first) == (lock_fit, lock_far)
        assert (dev.latest, dev.closest, dev.iterations, dev.state) == (lock.latest, lock.closest, lock.iterations,
                                                                        lock.state)
        assert dev.pose_from.tobytes() == lock.pose_from.tobytes() and dev.noise == lock.noise
        # the model's float64 ICP: iterations and end state; final_T within 16x its own noise scale
        assert (dev.latest, dev.closest) == (latest, closest)
        assert (dev.iterations, dev.state) == (r64["iterations"], r64["state"])
        noise = float(np.abs(r64["final_T"].astype(np.float64) - r32["final_T"]).max())
        err = float(np.abs(mp.loop_final_T.astype(np.float64) - r64["final_T"]).max())
        print(f"iterations {dev.iterations} state {dev.state} fitness {mp.loop_fitness:.6g} / {r64['fitness']:.6g}; "
              f"noise scale {noise:.3g}, device - model {err:.3g}; far_first {mp.icp_far_first}")
        assert noise > 0 and err <= 16 * noise
        assert mp.loop_fitness <= 0.3
        # the correction: the model's, applied to the device's final_T, to the bit
        wf, wt, wn = LM.loop_correction(mp.loop_final_T, case["stored"][latest], case["stored"][closest],
                                        mp.loop_fitness)
        assert dev.pose_from.tobytes() == wf.tobytes() and dev.pose_to.tobytes() == wt.tobytes()
        assert F(dev.noise).tobytes() == wn.tobytes()
        # the corrected pose lies closer to the true one than the stored pose did
        new_pose = LM.table_pose(dev.pose_from)
        e_old = np.linalg.norm(case["stored"][latest][3:6] - case["true"][latest][3:6])
        e_new = np.linalg.norm(new_pose[3:6] - case["true"][latest][3:6])
        assert e_new < e_old, (e_old, e_new)
        # correctPoses at the next run(): the table moves key 9, the recent list
        # is rebuilt, and both local maps are the model's at the new table
        mp.correctPoses()
        assert not mp.aLoopIsClosed and mp.recentKeyFrames == []
        table = [p.copy() for p in case["stored"]]
        table[latest] = new_pose
        same_bits(mp.cloudKeyPoses6D, np.array(table))
        cnt = mp.extractSurroundingKeyFrames()
        cc, sc, cmap, smap = LM.local_maps(oracle_mod.voxel_grid, case["kfs"], table, range(NKEYS))
        assert list(cnt) == [cc.shape[0], cmap.shape[0], sc.shape[0], smap.shape[0]]
        new_maps = local_maps_of(L, mp)
        same_bits(new_maps[0], cmap, "corner map after correctPoses")
        same_bits(new_maps[1], smap, "surf map after correctPoses")
        for a, b in zip(old_maps, new_maps):
            assert a.shape != b.shape or not np.array_equal(a, b)
    finally:
        mp.close()


def test_reference_search_num_and_no_candidate(L, case, mapper):
    """historyKeyframeSearchNum = 25: the target holds the latest key itself
    (reproduced); both ICP paths still agree to the bit.  No candidate: None."""
    mapper.currentRobotPosPoint = case["stored"][-1][3:6].copy()
    mapper.timeLaserOdometry = case["stamps"][-1]
    a = mapper.performLoopClosure(lockstep=True)
    Ta, fa = mapper.loop_final_T.copy(), mapper.loop_fitness
    b = mapper.performLoopClosure(lockstep=False)
    assert mapper.loop_final_T.tobytes() == Ta.tobytes() and mapper.loop_fitness == fa
    assert (a is None) == (b is None)
    if a is not None:
        assert a.pose_from.tobytes() == b.pose_from.tobytes() and (a.iterations, a.state) == (b.iterations, b.state)
    mapper.timeLaserOdometry = 20.0     # no key is 30 s away
    assert mapper.performLoopClosure() is None
    mapper.timeLaserOdometry = case["stamps"][-1]
    from agi_lidar_slam_amd.lego_map import LegoMapping
    empty = LegoMapping(max_points=256, loop_closure=True)
    try:
        assert empty.performLoopClosure() is None
    finally:
        empty.close()
