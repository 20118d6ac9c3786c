"""GPU tests of the LeGO-LOAM mapping back-end (slio_lmap_*, include/slio.h;
agi_lidar_slam_amd/lego_map.py) against the numpy restatement
tests/lego_map_model.py, to the bit: coefficients, normal equations, map
assembly from three keyframe stores, the device-to-device feed from the
front-end, the scan-to-map solve and LegoMapping.run.  Neighbours of the
model come from oracle.Tree(...).knn, VoxelGrids from oracle.voxel_grid;
every fixture is checked to be tie-free (no two of a query's six nearest
float distances equal), so that the comparison never tests this project's
tie rule against the oracle's.
"""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lego_map_case as K  # noqa: E402
import lego_map_model as M  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401
from test_lego_odom_cpu import SWEEP_T, moving_sweep, pose_at  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
ESTATE, EINVAL = -5, -1
CORNER, SURF_TOTAL, SURF, OUTLIER = 0, 1, 2, 3


def same_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan], err_msg=what)


def soa(p):
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    return [np.ascontiguousarray(p[:, k]) for k in range(3)]


def upload_map(L, mp, kind, pts):
    x, y, z = soa(pts)
    L.check(L.load().slio_map_upload(mp.handle(CORNER if kind == 0 else SURF_TOTAL), L.fptr(x), L.fptr(y), L.fptr(z),
                                     x.size), "map_upload")
    mp.map_counts[1 + 2 * kind] = x.size


def upload_scan(L, mp, which, pts):
    x, y, z = soa(pts)
    L.check(L.load().slio_scan_upload(mp.handle(which), L.fptr(x), L.fptr(y), L.fptr(z), x.size), "scan_upload")
    mp.scan_counts[which] = x.size


@pytest.fixture(scope="module")
def mapper(L):
    from agi_lidar_slam_amd.lego import LegoMapping
    m = LegoMapping(max_points=4096)
    yield m
    m.close()


@pytest.fixture(scope="module")
def knn(oracle_mod):
    def f(mp, q):
        """Five neighbours from the oracle's tree; the six nearest must be tie-free."""
        k = min(6, mp.shape[0])
        if q.shape[0] == 0 or k < 5:
            return np.zeros((q.shape[0], k), np.int32), np.full((q.shape[0], k), np.inf, F)
        idx, sqd = oracle_mod.Tree(mp).knn(q, k)
        assert M.tie_free(sqd)
        return idx[:, :5], sqd[:, :5]
    return f


# ------------------------------------------------------------------ coefficients
@pytest.mark.parametrize("kind", [0, 1])
def test_coefficients_bit_exact(L, oracle_mod, mapper, kind):
    c, ref = K.cut(), K.cut_reference(kind)
    # checked on the CPU before anything runs on the device: the model alone covers every branch
    st = ref["stats"]
    assert st["selected"] >= 1 and st["gated"] >= 1 and st["rejected"] >= 1, st
    assert M.tie_free(ref["sqd6"])
    scan = c["corner_scan"] if kind == 0 else c["surf_scan"]
    upload_map(L, mapper, kind, c["corner_map"] if kind == 0 else c["surf_map"])
    for n in K.SIZES:
        upload_scan(L, mapper, CORNER if kind == 0 else SURF_TOTAL, scan[:n])
        nsel = mapper.coeffs(kind, c["tf_eval"])
        coeff, sel = mapper.get_coeffs(kind, n)
        np.testing.assert_array_equal(sel, ref["sel"][:n], err_msg=f"sel n={n}")
        same_bits(coeff, ref["coeff"][:n], f"coeff n={n}")
        assert nsel == int(ref["sel"][:n].sum())
    assert mapper.far_queries(kind) >= 0


@pytest.mark.parametrize("kind", [0, 1])
def test_coefficients_tiny_map_and_empty_scan(L, mapper, kind):
    c = K.cut()
    scan = (c["corner_scan"] if kind == 0 else c["surf_scan"])[:65]
    mp = (c["corner_map"] if kind == 0 else c["surf_map"])
    which = CORNER if kind == 0 else SURF_TOTAL
    upload_map(L, mapper, kind, mp[:4])                 # fewer than five map points: nothing selected
    upload_scan(L, mapper, which, scan)
    assert mapper.coeffs(kind, c["tf_eval"]) == 0
    coeff, sel = mapper.get_coeffs(kind, 65)
    assert not sel.any() and not coeff.any()
    upload_map(L, mapper, kind, mp)
    upload_scan(L, mapper, which, scan[:0])             # a scan of 0 points
    assert mapper.coeffs(kind, c["tf_eval"]) == 0
    lib = L.load()
    n = C.c_int64()
    assert lib.slio_lmap_coeffs(mapper.m, 2, L.fptr(c["tf_eval"]), C.byref(n)) == EINVAL
    assert lib.slio_lmap_coeffs(mapper.m, -1, L.fptr(c["tf_eval"]), C.byref(n)) == EINVAL
    assert lib.slio_lmap_get_coeffs(mapper.m, 2, None, None) == EINVAL
    assert lib.slio_lmap_coeffs(mapper.m, kind, None, C.byref(n)) == EINVAL


# ------------------------------------------------------------------ normal equations
@pytest.mark.parametrize("nc,ns", [(255, 255), (256, 256), (257, 257), (1500, 1500), (0, 257), (257, 0)])
def test_normal_equations_bit_exact(L, mapper, nc, ns):
    c = K.cut()
    rc, rs = K.cut_reference(0), K.cut_reference(1)
    upload_map(L, mapper, 0, c["corner_map"])
    upload_map(L, mapper, 1, c["surf_map"])
    upload_scan(L, mapper, CORNER, c["corner_scan"][:nc])
    upload_scan(L, mapper, SURF_TOTAL, c["surf_scan"][:ns])
    lib = L.load()
    AtA, AtB, n = np.empty(36, F), np.empty(6, F), C.c_int64()
    assert lib.slio_lmap_normal_equations(mapper.m, L.fptr(AtA), L.fptr(AtB), C.byref(n)) == ESTATE
    mapper.coeffs(0, c["tf_eval"], want_nsel=False)
    assert lib.slio_lmap_normal_equations(mapper.m, L.fptr(AtA), L.fptr(AtB), C.byref(n)) == ESTATE
    mapper.coeffs(1, c["tf_eval"], want_nsel=False)
    AtA, AtB, nsel = mapper.normal_equations()
    wA, wB, wn = M.normal_equations(c["tf_eval"], [(c["corner_scan"][:nc], rc["coeff"][:nc], rc["sel"][:nc]),
                                                   (c["surf_scan"][:ns], rs["coeff"][:ns], rs["sel"][:ns])])
    assert nsel == wn == int(rc["sel"][:nc].sum()) + int(rs["sel"][:ns].sum())
    same_bits(AtA, wA, "AtA")
    same_bits(AtB, wB, "AtB")
    assert nsel > 0 and np.abs(AtA).max() > 0


# ------------------------------------------------------------------ map assembly
KF_SIZES = (0, 1, 63, 64, 65, 257)


@pytest.fixture(scope="module")
def stores(L):
    """A mapper whose three stores hold keyframes of 0, 1, 63, 64, 65 and 257
    points (a different size per store and key; key 3's outlier cloud empty)."""
    from agi_lidar_slam_amd.lego import LegoMapping
    m = LegoMapping(max_points=4096)
    rng = np.random.default_rng(17)
    kfs, poses = [], []
    for k in range(len(KF_SIZES)):
        sizes = [KF_SIZES[k], KF_SIZES[(k + 2) % 6], KF_SIZES[(k + 4) % 6]]
        if k == 3:
            sizes[2] = 0
        # points on a few planes near the sensor, so that voxels hold several points
        clouds = [np.column_stack([rng.uniform(-1.5, 1.5, n), rng.choice([-1.7, 0.0, 1.3], n) + rng.normal(0, 0.02, n),
                                   rng.uniform(-1.5, 1.5, n)]).astype(F) for n in sizes]
        pose = np.concatenate([rng.uniform(-0.2, 0.2, 3), rng.uniform(-2, 2, 3)]).astype(F)
        for which, cl in zip((CORNER, SURF, OUTLIER), clouds):
            upload_scan(L, m, which, cl)
        key = C.c_int32()
        L.check(L.load().slio_lmap_save_keyframe(m.m, L.fptr(pose), C.byref(key)), "save_keyframe")
        assert key.value == k
        kfs.append(clouds)
        poses.append(pose)
    yield m, kfs, poses
    m.close()


def assembled(oracle_mod, kfs, poses, keys, swap=False):
    cc = [M.to_map(poses[k], kfs[k][0]) for k in keys]
    sc = []
    for k in keys:
        pair = [M.to_map(poses[k], kfs[k][1]), M.to_map(poses[k], kfs[k][2])]
        sc += pair[::-1] if swap else pair
    cc, sc = np.concatenate(cc), np.concatenate(sc)
    return cc, sc, oracle_mod.voxel_grid(cc, 0.2), oracle_mod.voxel_grid(sc, 0.4)


@pytest.mark.parametrize("keys", [(0, 1, 2, 3, 4, 5), (5, 2, 5, 3), (0,), (3, 1)])
def test_map_assembly_bit_exact(L, oracle_mod, stores, keys):
    m, kfs, poses = stores
    got_poses = np.empty((6, 6), F)
    nk = C.c_int32()
    L.check(L.load().slio_lmap_get_key_poses(m.m, L.fptr(got_poses), 6, C.byref(nk)), "get_key_poses")
    assert nk.value == 6
    same_bits(got_poses, np.array(poses))
    ka = np.array(keys, np.int32)
    L.check(L.load().slio_lmap_extract(m.m, L.iptr(ka), ka.size, L.i64ptr(m.map_counts)), "extract")
    cc, sc, cmap, smap = assembled(oracle_mod, kfs, poses, keys)
    assert list(m.map_counts) == [cc.shape[0], cmap.shape[0], sc.shape[0], smap.shape[0]]
    same_bits(m.map_points(0), cmap, "corner map")
    same_bits(m.map_points(1), smap, "surf map")
    if any(min(kfs[k][1].shape[0], kfs[k][2].shape[0]) >= 60 for k in keys):
        # surf-then-outlier order per key is really checked: where a key has both clouds well filled
        # (voxels of three and more points from both), the other order gives other bits
        _, _, _, swapped = assembled(oracle_mod, kfs, poses, keys, swap=True)
        assert swapped.shape != smap.shape or not np.array_equal(swapped, smap)


def test_assembled_index_answers_like_the_host_path(L, oracle_mod, stores):
    from agi_lidar_slam_amd.lego import LegoMapping
    m, kfs, poses = stores
    keys = np.array([0, 1, 2, 3, 4, 5], np.int32)
    L.check(L.load().slio_lmap_extract(m.m, L.iptr(keys), keys.size, L.i64ptr(m.map_counts)), "extract")
    maps = [m.map_points(0), m.map_points(1)]
    rng = np.random.default_rng(23)
    tf = np.array([0.01, -0.02, 0.015, 0.1, -0.05, 0.08], F)
    host = LegoMapping(max_points=4096)
    try:
        for kind in (0, 1):
            q = (maps[kind][rng.integers(0, maps[kind].shape[0], 300)] + rng.normal(0, 0.05, (300, 3))).astype(F)
            res = []
            for mp, via_host in ((m, False), (host, True)):
                if via_host:
                    upload_map(L, mp, kind, maps[kind])
                upload_scan(L, mp, CORNER if kind == 0 else SURF_TOTAL, q)
                nsel = mp.coeffs(kind, tf)
                res.append((nsel,) + mp.get_coeffs(kind, 300))
            assert res[0][0] == res[1][0]
            same_bits(res[0][1], res[1][1], f"coeff kind {kind}")
            np.testing.assert_array_equal(res[0][2], res[1][2])
            assert kind == 0 or res[0][0] > 0
    finally:
        host.close()
    bad = np.array([0, 6], np.int32)
    assert L.load().slio_lmap_extract(m.m, L.iptr(bad), 2, L.i64ptr(np.zeros(4, np.int64))) == EINVAL
    assert L.load().slio_lmap_extract(m.m, None, 1, L.i64ptr(np.zeros(4, np.int64))) == EINVAL


# ------------------------------------------------------------------ feed
def test_feed_from_the_front_end(L, oracle_mod):
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoMapping, LegoParams
    from test_lego_odom_cpu import PARAMS
    fe = LegoFrontEnd(LegoParams(**PARAMS))
    fe.enable_odometry()
    a, b = LegoMapping(max_points=8192), LegoMapping(max_points=8192)
    try:
        cnt = np.zeros(4, np.int64)
        assert L.load().slio_lmap_feed_lego(a.m, fe.h, L.i64ptr(cnt)) == ESTATE     # before any sweep
        for k in range(3):
            sc = moving_sweep(k)
            out = fe.runFeatureAssociation(sc["x"], sc["y"], sc["z"], None, k * SWEEP_T)
            if not out["published"]:
                assert L.load().slio_lmap_feed_lego(a.m, fe.h, L.i64ptr(cnt)) == ESTATE   # a non-publishing sweep
                continue
            last = fe.last_clouds()
            cl, sl, ol = (last[n] for n in ("laserCloudCornerLast", "laserCloudSurfLast", "outlierCloudLast"))
            assert min(cl.shape[0], sl.shape[0], ol.shape[0]) > 0
            cds, sds, ods = (oracle_mod.voxel_grid(cl[:, :3], 0.2), oracle_mod.voxel_grid(sl[:, :3], 0.4),
                             oracle_mod.voxel_grid(ol[:, :3], 0.4))
            tds = oracle_mod.voxel_grid(np.concatenate([sds, ods]), 0.4)            # the second grid, in that order
            want = {CORNER: cds, SURF_TOTAL: tds, SURF: sds, OUTLIER: ods}
            a.downsampleCurrentScan(fe)
            b.downsampleCurrentScan(clouds=(cl, sl, ol))
            for mp in (a, b):
                assert list(mp.scan_counts) == [want[w].shape[0] for w in range(4)]
                for w in range(4):
                    same_bits(mp.scan(w), want[w], f"cloud {w}")
    finally:
        a.close()
        b.close()
        fe.close()


# ------------------------------------------------------------------ solve
def test_solve_on_the_converted_problem(L, oracle_mod):
    """The solver class, problem, start and bounds of test_gpu_lio_s2m.py's
    convergence test, in this frame: start 0.005, -0.004, 0.01 rad and 0.15,
    -0.1, 0.05 m off the truth, end within 0.05 m and 0.003 rad."""
    from agi_lidar_slam_amd.lego import LegoMapping
    pb = K.problem()
    mp = LegoMapping(max_points=60000)
    try:
        upload_map(L, mp, 0, pb["corner_map"])
        upload_map(L, mp, 1, pb["surf_map"])
        upload_scan(L, mp, CORNER, pb["corner_scan"])
        upload_scan(L, mp, SURF_TOTAL, pb["surf_scan"])
        tf0 = pb["tf"] + M.cam_pose(np.array([0.005, -0.004, 0.01, 0.15, -0.1, 0.05], F))
        tf, iters, deg = mp.optimize(tf0)
        far = [mp.far_queries(0), mp.far_queries(1)]
        err_t = np.abs(tf[3:] - pb["tf"][3:]).max()
        err_r = np.abs(tf[:3] - pb["tf"][:3]).max()
        print(f"slio_lmap_optimize: {iters} iterations, |dt| {err_t:.4f} m, |dr| {err_r:.5f} rad, degenerate {deg}, "
              f"far queries of the last pass (corner, surf) {far}")
        assert 1 <= iters <= 10
        assert err_t < 0.05 and err_r < 0.003
        # the same loop through the single-stage entries and slio_s2m_lm_step, to the bit
        tl, il, dl, trace = mp.optimize_lockstep(tf0)
        assert (il, dl) == (iters, deg)
        same_bits(tl, tf, "optimize vs lockstep")
        # ... and after every iteration, on the cut (small maps): slio_lmap_optimize capped at k
        # iterations ends where the lockstep trace is after k
        c = K.cut()
        start = (c["tf"] + M.cam_pose(np.array([0.005, -0.004, 0.01, 0.15, -0.1, 0.05], F))).astype(F)
        trace, il = None, 10
        for k in (10, 1, 2, 3):
            if k > il:
                continue
            short = LegoMapping(max_points=4096, max_iterations=k)
            try:
                upload_map(L, short, 0, c["corner_map"])
                upload_map(L, short, 1, c["surf_map"])
                upload_scan(L, short, CORNER, c["corner_scan"])
                upload_scan(L, short, SURF_TOTAL, c["surf_scan"])
                tk, ik, dk = short.optimize(start)
                if trace is None:
                    tl, il, dl, trace = short.optimize_lockstep(start)
                    assert (ik, dk) == (il, dl) and il >= 2
                    same_bits(tk, tl, "cut: optimize vs lockstep")
                assert ik == min(k, il)
                same_bits(tk, trace[ik - 1], f"cut: after iteration {ik}")
            finally:
                short.close()
    finally:
        mp.close()


# ------------------------------------------------------------------ the public path
def gt_pose_cam(t):
    """Ground truth of the sensor at time t relative to t = 0, as a camera-frame position."""
    _, p = pose_at(t)
    return np.array([p[1], p[2], p[0]])


def test_public_path_four_mapping_calls(L, oracle_mod, knn):
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoMapping, LegoParams, TransformFusion
    fe = LegoFrontEnd(LegoParams())                       # 16 x 1800
    fe.enable_odometry()
    a, b = LegoMapping(max_points=20000), LegoMapping(max_points=20000)
    fusion = TransformFusion()
    calls, k, model_checked = 0, 0, False
    try:
        while calls < 4 and k < 20:
            sc = moving_sweep(k, horizon=1800)
            t = (k + 1) * SWEEP_T                         # the sweep's end stamps its odometry
            out = fe.runFeatureAssociation(sc["x"], sc["y"], sc["z"], None, k * SWEEP_T)
            k += 1
            keys_before = a.cloudKeyPoses3D.shape[0]
            ran = a.run(fe, t)
            if not ran:
                continue
            calls += 1
            assert out["published"]
            # the same call stage by stage through the lockstep entries
            b.laserOdometryHandler(out["transform_sum"], t)
            b.timeLastProcessing = t
            tobe0 = b.transformAssociateToMap()
            same_bits(a.tobe_associated, tobe0, "transformAssociateToMap")
            # transformFusion: the same formula on the same triple
            same_bits(fusion.laserOdometryHandler(out["transform_sum"]), tobe0, "TransformFusion")
            b.extractSurroundingKeyFrames()
            b.downsampleCurrentScan(fe)
            assert list(a.map_counts) == list(b.map_counts) and list(a.scan_counts) == list(b.scan_counts)
            b.scan2MapOptimization(lockstep=True)
            same_bits(a.transformTobeMapped, b.transformTobeMapped, f"call {calls}: optimize vs lockstep")
            assert (a.iterations, a.isDegenerate) == (b.iterations, b.isDegenerate)
            if keys_before and not model_checked:
                # the first call with a non-empty map, against the model end to end
                assert keys_before == 1 and a.map_counts[1] > 10 and a.map_counts[3] > 100
                kf = []
                for which in (CORNER, SURF, OUTLIER):
                    h = b.handle(which)
                    n = C.c_int64()
                    cap = 20000
                    xyz = np.empty((3, cap), F)
                    L.check(L.load().slio_s2m_kf_get(h, 0, L.fptr(xyz[0]), L.fptr(xyz[1]), L.fptr(xyz[2]), cap,
                                                     C.byref(n)), "kf_get")
                    kf.append(np.ascontiguousarray(xyz[:, :n.value].T))
                pose0 = b.cloudKeyPoses6D[0]
                cmap = oracle_mod.voxel_grid(M.to_map(pose0, kf[0]), 0.2)
                smap = oracle_mod.voxel_grid(np.concatenate([M.to_map(pose0, kf[1]), M.to_map(pose0, kf[2])]), 0.4)
                same_bits(b.map_points(0), cmap, "corner map")
                same_bits(b.map_points(1), smap, "surf map")
                want0 = M.associate_to_map(out["transform_sum"], a_prev["bef"], a_prev["aft"])
                same_bits(tobe0, want0, "model transformAssociateToMap")
                tm, im, dm, trace = M.scan2map(want0, b.scan(CORNER), b.scan(SURF_TOTAL), cmap, smap, knn)
                assert im == b.iterations and len(trace) == len(b.trace) and bool(dm) == b.isDegenerate
                for i, (g, w) in enumerate(zip(b.trace, trace)):
                    same_bits(g, w, f"transformTobeMapped after iteration {i}")
                model_checked = True
            same_bits(a.transformAftMapped, b.transformAftMapped, "transformAftMapped (after transformUpdate)")
            cur_before = b.transformAftMapped[3:6]
            saved = b.saveKeyFramesAndFactor()
            assert saved == a.saved_last == M.keyframe_decision(prev_pos if calls > 1 else np.zeros(3, F), cur_before,
                                                                keys_before)
            if saved:
                prev_pos = cur_before.copy()
            same_bits(a.transformAftMapped, b.transformAftMapped, "transformAftMapped")
            same_bits(a.cloudKeyPoses6D, b.cloudKeyPoses6D, "cloudKeyPoses6D")
            assert np.isfinite(a.transformAftMapped).all()
            a_prev = dict(bef=a.transformBefMapped, aft=a.transformAftMapped)
            fusion.odomAftMappedHandler(a.transformAftMapped, a.transformBefMapped)
        assert calls == 4 and model_checked
        assert a.cloudKeyPoses6D.shape[0] >= 2                      # keyframes are saved
        # distance to the ground truth at the last mapping call (printed, not asserted: nobody has measured a bound)
        gt = gt_pose_cam(t) - gt_pose_cam(SWEEP_T)                  # transformSum is 0 at the first sweep's end
        d_odom = float(np.linalg.norm(out["transform_sum"][3:6].astype(np.float64) - gt))
        d_map = float(np.linalg.norm(a.transformAftMapped[3:6].astype(np.float64) - gt))
        print(f"after {k} sweeps ({calls} mapping calls, {a.cloudKeyPoses6D.shape[0]} keyframes): distance to ground "
              f"truth /laser_odom_to_init {d_odom:.4f} m, /aft_mapped_to_init {d_map:.4f} m; map sizes "
              f"{list(a.map_counts)}, scan sizes {list(a.scan_counts)}, iterations {a.iterations}")
        assert math.isfinite(d_odom) and math.isfinite(d_map)
    finally:
        a.close()
        b.close()
        fe.close()
