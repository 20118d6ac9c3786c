#!/usr/bin/env python3
"""Timings of the rows around the hot path on one GPU.

  mapping   live laserMapping per scan on the C2-size map: lasermap_fov_segment +
            Delete_Point_Boxes, the 4-iteration device IKF update, map_incremental,
            and the device index rebuild the next search needs (forced here)
  preproc   UndistortPcl back-propagation + downSizeFilterSurf of a raw scan
  s2m       one LIO-SAM scan-to-map iteration (corner + surf coefficients, normal
            equations, LM step)
  s2m_map   one LIO-SAM local-map assembly (extractCloud) of 50 keyframes from the
            device keyframe store, against the host path it replaces (only when
            named: it also runs the CPU oracle)
  s2m_loop  one LIO-SAM loop closure (loopFindNearKeyframes twice + ICP + fitness)
            on the device: 51 keyframes in the store, the source keyframe's pose
            off by 1 m and 3 deg, against a host restatement (scipy cKDTree +
            numpy) over the same clouds, and the same ICP through the
            device-resident loop (icp_align_device) (only when named)
  lego_loop one LeGO-LOAM loop closure (LegoMapping(loop_closure=True)): 60 keyframes
            of the 16 x 1800 sequence's sizes in the stores, the newest key's pose
            off by 1 m and 3 deg; both assemblies, the ICP through slio_icp_align
            (per batch size) and through the lockstep loop on the same clouds, the
            fitness pass, the host restatement beside them (only when named)
  lego_odom LeGO-LOAM front-end + scan-to-scan odometry on a 16 x 1800 sequence:
            sweeps per second, the odometry call alone, the lockstep loop and
            the numpy restatement (only when named)
  lego_map  LeGO-LOAM mapping back-end (LegoMapping) behind the front-end and
            odometry on the same sequence: ms per mapping call and its split,
            iterations, map sizes, the host restatement beside it (only when
            named)
  livox_map livox_mapping's laserMapping (LivoxMapping: slio_lvx_*) on a synthetic
            Avia-pattern trajectory with crude feature clouds: ms per mapping
            call and its split (select + gather, downsample, optimise, update),
            iterations, map and cube sizes, host waits, the last call once more
            through the host restatement (only when named)
  aloam_reg A-LOAM's scanRegistration (AloamScanRegistration: slio_aloam_*) on a VLP-16
            sweep (horizon 1800) and a 64-line sweep (horizon 2083): ms per registration,
            the five counts, the host restatement beside it (only when named)
  aloam_odom A-LOAM's laserOdometry (AloamOdometry: slio_aloam_odom_*) on the same two inputs
            as two consecutive sweeps of a moving sensor: ms per odometry call and its split
            into association and solve, correspondences, iterations, launches and waits,
            registration plus odometry per sweep, the host restatement beside it (only
            when named)
  aloam_map A-LOAM's laserMapping (AloamMapping: slio_aloam_map_*) on the same two inputs as
            two alternating sweeps of a moving sensor with a drifting odometry pose: ms per
            mapping call, map and stack sizes, factors, iterations, launches and waits, the
            host restatement beside it (only when named)
  livox_reg livox_mapping's scanRegistration (LivoxScanRegistration: slio_lreg_*) on a
            dense continuous-curve frame of about 24,000 returns: ms per registration,
            the counts, the host restatement beside it; then process_cloud (sensor's
            cloud to pose) over a short drive: ms per call, of which the registration
            (only when named)
  lio_livox_reg LIO-Livox's ScanRegistration (LioLivoxScanRegistration: slio_llreg_*) on a
            24,000-point 6-line frame with the Horizon parameters and a 20,000-point 4-line
            frame with the Mid-360 parameters: ms per FeatureExtract, the counts, the host
            restatement beside each (only when named)
One JSON line per measurement (host wall clock around synchronous calls)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def t_ms(f, reps=1):
    t0 = time.perf_counter()
    for _ in range(reps):
        r = f()
    return (time.perf_counter() - t0) * 1e3 / reps, r


def mapping(n_map, n_scan, frames_n=6):
    from agi_lidar_slam_amd import _lib as L, synth
    from agi_lidar_slam_amd.esekf import StateIkfom
    from agi_lidar_slam_amd.mapping import LaserMapping
    seed = 20261015
    mp, _ = synth.make_problem(n_map, n_scan, cache_dir="/tmp/slio_cache")
    frames = synth.make_trajectory(seed, n_map, frames_n, n_scan, step=0.5)
    lm = LaserMapping(max_points=n_scan, cube_len=1000.0)
    lm.ikdtree.set_downsample_param(0.5)
    lm.ikdtree.Build(mp)
    lm.built = True
    lm.first_lidar_time = 0.0
    x = StateIkfom(pos=frames[0].gt_pos.copy(), rot=frames[0].gt_rot.copy(), offset_T_L_I=synth.AVIA_T_LI.copy())
    lm.kf.change_x(x)
    lib = L.load()
    rows = []
    steps, search = [], []
    for k, fr in enumerate(frames):
        x = lm.kf.get_x()
        if k:
            x.pos = x.pos + (fr.gt_pos - frames[k - 1].gt_pos)
            if os.environ.get("MAPPING_PRIOR") == "gtrot":
                # diagnostic: the ground-truth rotation as well (the default
                # prior carries the previous scan's rotation)
                x.rot = fr.gt_rot.copy()
        lm.kf.change_x(x)
        lm.kf.change_P(np.eye(24) * 1e-2)
        body = np.ascontiguousarray(fr.body[synth.voxel_order(fr.body)])
        # HIP events on this scan's search launches (diagnostic: ~5 us per launch)
        lib.slio_profile(lm.kf.h, 1 << (L.SLIO_KERNEL_SEARCH + 1))
        t0 = time.perf_counter()
        lm.process(body, lidar_beg_time=0.1 * (k + 1))
        t_total = (time.perf_counter() - t0) * 1e3
        ms, nl = C.c_double(), C.c_int64()
        lib.slio_profile_read(lm.kf.h, L.SLIO_KERNEL_SEARCH, C.byref(ms), C.byref(nl))
        lib.slio_profile(lm.kf.h, 0)
        nfar = C.c_int64()
        lib.slio_far_queries(lm.kf.h, C.byref(nfar))
        n = C.c_int64()
        t_rebuild, _ = t_ms(lambda: lib.slio_map_info(lm.ikdtree.h, None, None, C.byref(n)))
        rows.append((t_total, t_rebuild, int(n.value), [int(v) for v in lm.last["map_incremental"]]))
        steps.append([round(v, 3) for v in lm.last.get("t_ms", (0, 0, 0))])
        search.append((round(ms.value, 3), int(nl.value), int(nfar.value)))
    # first scan pays one-time allocations; report the median of the rest
    tt = np.median([r[0] for r in rows[1:]])
    tr = np.median([r[1] for r in rows[1:]])
    print(json.dumps({"bench": "live_mapping_per_scan", "map_points": n_map, "scan_points": n_scan,
                      "ms_fov_ikf4_map_incremental": tt, "ms_index_rebuild": tr,
                      "ms_per_scan": tt + tr, "ms_index_rebuild_each": [round(r[1], 3) for r in rows],
                      "map_size_after": rows[-1][2],
                      "map_incremental_counts_last": rows[-1][3],
                      "ms_fov_update_mapinc_each": steps,
                      "search_ms_launches_farq_each": search}), flush=True)


def chain(n_map, n_raw, frames_n=8):
    """Live laserMapping with a realistic prior: the C2-size map, raw scans
    rendered along a street with per-point time (100 ms sweep), 200 Hz IMU;
    per scan ImuProcess forward propagation (P carried, no reset) +
    undistortion + downSizeFilterSurf on the device, lasermap_fov_segment,
    the reference-flow update (maximum_iter 4), map_incremental; the index
    rebuild runs inside the next scan's first search (timed inside the
    update).  Host wall clock per stage (each stage synchronises), HIP events
    on the search launches, medians over scans 2.."""
    from agi_lidar_slam_amd import _lib as L, synth
    from agi_lidar_slam_amd.esekf import StateIkfom
    from agi_lidar_slam_amd.imu import ImuProcess, MeasureGroup
    from agi_lidar_slam_amd.mapping import LaserMapping
    import test_gpu_chain as TC
    seed = 20261015
    mp, _ = synth.make_problem(n_map, 100000, cache_dir="/tmp/slio_cache")
    seq = TC.make_sequence(seed, n_map, frames_n, n_raw, 0.5)
    lib = L.load()
    lm = LaserMapping(filter_size_map_min=0.5, cube_len=1000.0, maximum_iter=4, max_points=n_raw)
    lm.ikdtree.set_downsample_param(0.5)
    lm.ikdtree.Build(mp)
    lm.built = True
    ip = ImuProcess(mean_acc=np.array([0.0, 0.0, 1.0]), cov_gyr=TC.COV12[0:3], cov_acc=TC.COV12[3:6],
                    cov_bias_gyr=TC.COV12[6:9], cov_bias_acc=TC.COV12[9:12])
    fr0 = seq[0]["frame"]
    lm.kf.change_x(StateIkfom(pos=fr0.gt_pos.copy(), rot=fr0.gt_rot.copy(), offset_T_L_I=synth.AVIA_T_LI.copy(),
                              vel=seq[1]["v"].copy(), grav=np.array([0.0, 0.0, -9.81])))
    lm.kf.change_P(np.eye(24) * 1e-3)
    ip.last_imu_ = np.array([seq[0]["end"], 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])
    ip.last_lidar_end_time_ = seq[0]["end"]
    rows = []
    for k, s in enumerate(seq[1:], start=1):
        t0 = time.perf_counter()
        meas = MeasureGroup(lidar_beg_time=s["beg"], lidar_end_time=s["end"], points=s["raw"],
                            t_ms=s["t_ms"], imu=s["imu"])
        nd = ip.undistort_downsample(meas, lm.kf, 0.5)
        t1 = time.perf_counter()
        xp = lm.kf.get_x().to_array()
        pos_lid = xp[0:3] + synth.quat_matrix(xp[3:7]) @ xp[11:14]
        lm.lasermap_fov_segment(pos_lid)
        t2 = time.perf_counter()
        lib.slio_profile(lm.kf.h, 1 << (L.SLIO_KERNEL_SEARCH + 1))
        # Nearest_Points stay on the device (map_incremental reads them there)
        lm.kf.update_iterated_dyn_share_modified(0.001, None, lm.ikdtree, None, 4, False)
        t3 = time.perf_counter()
        ms, nl = C.c_double(), C.c_int64()
        lib.slio_profile_read(lm.kf.h, L.SLIO_KERNEL_SEARCH, C.byref(ms), C.byref(nl))
        lib.slio_profile(lm.kf.h, 0)
        nfar = C.c_int64()
        lib.slio_far_queries(lm.kf.h, C.byref(nfar))
        t4 = time.perf_counter()
        cnt = lm.kf.map_incremental(lm.ikdtree, 0.5, True)
        t5 = time.perf_counter()
        st = lm.kf.last_stats
        xg = lm.kf.get_x().to_array()
        rows.append(dict(scan=k, down=int(nd), ms_imu_undistort_voxel=(t1 - t0) * 1e3,
                         ms_fov=(t2 - t1) * 1e3, ms_update_incl_rebuild=(t3 - t2) * 1e3,
                         ms_map_incremental=(t5 - t4) * 1e3, passes=int(st.passes), searches=int(st.searches),
                         launch_ms=[round(ms.value, 3), int(nl.value)], far=int(nfar.value),
                         err_m=float(np.abs(xg[0:3] - s["frame"].gt_pos).max()),
                         added=[int(v) for v in cnt]))
    keys = ["ms_imu_undistort_voxel", "ms_fov", "ms_update_incl_rebuild", "ms_map_incremental"]
    med = {k_: float(np.median([r[k_] for r in rows[1:]])) for k_ in keys}
    print(json.dumps({"bench": "live_chain_per_scan", "map_points": n_map, "raw_points": n_raw,
                      "median": med, "ms_per_scan_mapping": med["ms_fov"] + med["ms_update_incl_rebuild"]
                      + med["ms_map_incremental"], "ms_per_scan_all": sum(med.values()), "scans": rows}),
          flush=True)
    lm.kf.close()
    lm.ikdtree.close()


def preproc(n_raw):
    from agi_lidar_slam_amd.esekf import Esekf, StateIkfom
    from agi_lidar_slam_amd.imu import ImuProcess, MeasureGroup
    from imu_case import make_case
    cs = make_case(0, False, n=n_raw)
    kf = Esekf(max_points=n_raw)

    def one():
        kf.change_x(StateIkfom.from_array(cs["state"]))
        kf.change_P(cs["P"])
        ip = ImuProcess(mean_acc=np.array([0.3, 0.1, 1.02]), last_imu_=cs["imu"][0],
                        acc_s_last=cs["acc_s_last"].copy(), angvel_last=cs["angvel_last"].copy(),
                        last_lidar_end_time_=cs["last_end"])
        meas = MeasureGroup(cs["beg"], cs["end"], cs["pts"], cs["t"], cs["imu"][1:])
        return ip.undistort_downsample(meas, kf, 0.5)
    one()
    ms, nd = t_ms(one, 10)
    print(json.dumps({"bench": "undistort_voxel_per_scan", "raw_points": n_raw, "down_points": int(nd),
                      "ms_per_scan_incl_h2d": ms}), flush=True)
    kf.close()


def s2m():
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    pr = synth.make_s2m_problem()
    s = ScanToMap(max_points=60000)
    s.set_maps(pr["corner_map"], pr["surf_map"])
    s.set_scan(pr["corner_scan"], pr["surf_scan"])
    tf = pr["tf"].copy()

    def it():
        s.corner_optimization(tf)
        s.surf_optimization(tf)
        return s.normal_equations(tf)
    it()
    ms, r = t_ms(it, 20)
    print(json.dumps({"bench": "lio_sam_s2m_iteration", "corner_points": int(pr["corner_scan"].shape[0]),
                      "surf_points": int(pr["surf_scan"].shape[0]), "ms_per_iteration": ms}), flush=True)
    s.close()


def s2m_map(n_kf=50, n_surf=20000, n_corner=1000, reps=200):
    """One local-map assembly per scan (extractCloud): n_kf keyframes of
    n_surf surf and n_corner corner points (drawn from the synthetic scene
    with 5 cm noise, each in the LiDAR frame of its own pose), leaves 0.4 /
    0.2, on the device from the keyframe store -- against the host path
    set_maps replaces: the oracle's transformPointCloud + VoxelGrid on the CPU
    (single thread), then slio_map_upload of both maps."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    from oracle import oracle as O
    O.build()
    pr = synth.make_s2m_problem()
    rng = np.random.default_rng(7)
    s = ScanToMap(max_points=60000)
    kfs, poses = [], []
    for k in range(n_kf):
        pose = np.array([0.002 * k, -0.003 * k, 0.02 * k, 0.5 * k, -0.1 * k, 0.01 * k], np.float32)
        cr, sr, cp, sp, cy, sy = (f(float(a)) for a in pose[:3] for f in (np.cos, np.sin))
        R = np.array([[cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr],
                      [sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr], [-sp, cp * sr, cp * cr]])
        out = []
        for mp, n in ((pr["corner_map"], n_corner), (pr["surf_map"], n_surf)):
            w = mp[rng.choice(mp.shape[0], n)] + rng.normal(0, 0.05, (n, 3))
            out.append(((w - pose[3:].astype(np.float64)) @ R).astype(np.float32))
        kfs.append(out)
        poses.append(pose)
        s.push_keyframe(out[0], out[1])
    poses = np.stack(poses)
    keys = np.arange(n_kf, dtype=np.int32)

    def device():
        return s.extract_cloud(keys, poses)   # (each call waits for its index build)
    first, _ = t_ms(device)
    ms_dev, cnt = t_ms(device, reps)
    host = {}

    def host_path():
        t0 = time.perf_counter()
        cats = [np.concatenate([O.s2m_transform(poses[k], kfs[k][j]) for k in range(n_kf)]) for j in range(2)]
        t1 = time.perf_counter()
        maps = [O.voxel_grid(cats[0], 0.2), O.voxel_grid(cats[1], 0.4)]
        t2 = time.perf_counter()
        s.set_maps(maps[0], maps[1])
        t3 = time.perf_counter()
        host.update(ms_transform=(t1 - t0) * 1e3, ms_voxel_grid=(t2 - t1) * 1e3, ms_map_upload=(t3 - t2) * 1e3,
                    map_points=[int(m.shape[0]) for m in maps])
    host_path()
    ms_host, _ = t_ms(host_path, 3)
    print(json.dumps({"bench": "lio_sam_s2m_map_assembly", "keyframes": n_kf, "surf_points_per_keyframe": n_surf,
                      "corner_points_per_keyframe": n_corner, "concatenated_corner_surf": [cnt[0][0], cnt[1][0]],
                      "map_points_corner_surf": [cnt[0][1], cnt[1][1]], "ms_device_first_call": first,
                      "ms_device_per_scan": ms_dev, "ms_host_path_per_scan": ms_host,
                      "host_path_last": host}), flush=True)
    s.close()


def host_icp(src, tgt, max_dist):
    """The ICP restated on the host over the two clouds: scipy cKDTree (built
    once, one query per pass, all cores) + numpy sums + the numpy Umeyama of
    tests/icp_model.py."""
    import icp_model as M
    from scipy.spatial import cKDTree
    med = lambda v: float(np.median(v))  # noqa: E731
    t0 = time.perf_counter()
    tree = cKDTree(tgt.astype(np.float64))
    t_build = (time.perf_counter() - t0) * 1e3
    st = M.State()
    work, pass_ms = src.copy(), []

    def one_pass(w, md):
        d, j = tree.query(w.astype(np.float64), k=1, workers=-1)
        ok = d <= md
        p, q = w[ok].astype(np.float64), tgt[j[ok]].astype(np.float64)
        sums = np.concatenate([p.sum(0), q.sum(0), (q.T @ p).reshape(9), [(d[ok] * d[ok]).sum()]])
        return sums, int(ok.sum())
    while True:
        t1 = time.perf_counter()
        sums, n = one_pass(work, max_dist)
        pass_ms.append((time.perf_counter() - t1) * 1e3)
        delta, done = M.step(sums, n, st)
        if done:
            break
        work = M.transform32(delta, work)
    sums, n = one_pass(M.transform32(st.final_T, src), np.inf)
    return dict(ms_total=(time.perf_counter() - t0) * 1e3, ms_tree_build=t_build, ms_per_pass=med(pass_ms),
                iterations=st.iterations, fitness=sums[15] / max(n, 1))


def s2m_loop(n_kf=51, n_surf=20000, n_corner=1000, reps=5):
    """performLoopClosure's device work: the store holds n_kf keyframes (as
    s2m_map's) plus the newest one, a fresh draw at keyframe 25's place whose
    stored pose is off by 1 m and 3 deg of yaw; the target is keyframes 0..50
    (loopKeyPre 25, historyKeyframeSearchNum 25) and the source the newest
    keyframe alone, both through downSizeFilterICP (0.4); ICP with
    max_corr_dist 30 and the fitness pass.  The host figure restates the ICP
    (not the assemblies) on the same two clouds: scipy cKDTree (built once,
    one query per pass, all cores) + numpy sums + the numpy Umeyama of
    tests/icp_model.py.  far_start: one more first pass with the source 12 m
    off, where most queries take the far path."""
    import icp_model as M
    from agi_lidar_slam_amd import _lib as L, synth
    from agi_lidar_slam_amd.lio_sam import ScanToMap
    pr = synth.make_s2m_problem()
    rng = np.random.default_rng(11)
    s = ScanToMap(max_points=60000)
    lib = s.lib

    def pose_of(k):
        return np.array([0.002 * k, -0.003 * k, 0.02 * k, 0.5 * k, -0.1 * k, 0.01 * k], np.float64)

    def keyframe(pose):
        R = M.rot_zyx(*pose[:3])
        out = []
        for mp, n in ((pr["corner_map"], n_corner), (pr["surf_map"], n_surf)):
            w = mp[rng.choice(mp.shape[0], n)] + rng.normal(0, 0.05, (n, 3))
            out.append(((w - pose[3:]) @ R).astype(np.float32))
        return out

    poses = [pose_of(k) for k in range(n_kf)]
    for k in range(n_kf):
        s.push_keyframe(*keyframe(poses[k]))
    s.push_keyframe(*keyframe(poses[n_kf // 2]))
    wrong = poses[n_kf // 2].copy()
    wrong[2] += np.deg2rad(3.0)
    wrong[3:] += [0.8, -0.6, 0.0]
    poses = np.array(poses + [wrong], np.float32)
    cur, pre = n_kf, n_kf // 2

    def assemble():
        return (s.loop_find_near_keyframes(cur, 0, poses, True), s.loop_find_near_keyframes(pre, 25, poses, False))

    def run():
        t0 = time.perf_counter()
        sizes = assemble()
        t1 = time.perf_counter()
        res = s.icp_align(30.0)
        t2 = time.perf_counter()
        return sizes, res, (t1 - t0) * 1e3, (t2 - t1) * 1e3, list(s.icp_pass_ms), s.icp_far_first

    run()
    rows = [run() for _ in range(reps)]
    sizes, res = rows[-1][0], rows[-1][1]
    med = lambda v: float(np.median(v))  # noqa: E731
    # the two clouds, for the host restatement
    n_src, n_tgt = sizes
    xs = [np.zeros(n_src, np.float32) for _ in range(3)]
    L.check(lib.slio_scan_download(s.hl, *(L.fptr(a) for a in xs)), "scan_download")
    src = np.stack(xs, 1)
    xt = [np.zeros(n_tgt, np.float32) for _ in range(3)]
    ids = np.zeros(n_tgt, np.uint32)
    got = C.c_int64()
    L.check(lib.slio_map_download(s.hl, *(L.fptr(a) for a in xt), ids.ctypes.data_as(C.POINTER(C.c_uint32)), n_tgt,
                                  C.byref(got)), "map_download")
    tgt = np.stack(xt, 1)

    host_icp(src, tgt, 30.0)
    host = host_icp(src, tgt, 30.0)
    # the same ICP through the device-resident loop (slio_icp_align), per batch size
    dev_loop = {}
    for batch in (0, 1, 4, 8, 16, 32):
        s.icp_align_device(30.0, batch=batch)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            rd = s.icp_align_device(30.0, batch=batch)
            ts.append((time.perf_counter() - t0) * 1e3)
        dev_loop["default" if batch == 0 else str(batch)] = med(ts)
    same = bool(rd[0] == res[0] and np.array_equal(rd[1], res[1]) and rd[2:] == res[2:])
    # a far start: the source 12 m off (the first pass only)
    shift = np.eye(4, dtype=np.float32)
    shift[:3, 3] = [12.0, -9.0, 0.0]
    sums, nc, far = np.zeros(16), C.c_int64(), C.c_int64()
    tf = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        L.check(lib.slio_icp_correspond(s.hl, L.fptr(shift.reshape(16)), 1, 30.0, L.dptr(sums), C.byref(nc)), "icp")
        tf.append((time.perf_counter() - t0) * 1e3)
    L.check(lib.slio_icp_far_queries(s.hl, C.byref(far)), "far")
    print(json.dumps({
        "bench": "lio_sam_s2m_loop_closure", "keyframes": n_kf, "surf_points_per_keyframe": n_surf,
        "corner_points_per_keyframe": n_corner, "source_points": n_src, "target_points": n_tgt,
        "ms_two_assemblies": med([r[2] for r in rows]), "ms_per_icp_pass": med(rows[-1][4]),
        "iterations": res[3], "convergence_state": res[4], "converged": res[0], "fitness": res[2],
        "ms_icp_incl_fitness": med([r[3] for r in rows]), "ms_total": med([r[2] + r[3] for r in rows]),
        "far_share_first_pass": rows[-1][5] / max(n_src, 1),
        "far_start": {"shift_m": 15.0, "far_share": far.value / max(n_src, 1), "ms_pass": med(tf[1:])},
        "host_ckdtree_numpy": host}), flush=True)
    print(json.dumps({
        "bench": "lio_sam_s2m_loop_closure_icp_align_device", "iterations": rd[3], "convergence_state": rd[4],
        "ms_icp_incl_fitness_by_batch": dev_loop, "ms_lockstep_icp_incl_fitness": med([r[3] for r in rows]),
        "host_waits_lockstep": res[3] + 1, "same_bits_as_lockstep": same}), flush=True)
    s.close()


def lego_loop(n_kf=60, n_corner=246, n_surf=2000, n_outlier=1000, reps=5):
    """performLoopClosure on LegoMapping(loop_closure=True).  The stores hold
    n_kf keyframes of about the sizes the 16 x 1800 sequence leaves (lego_map:
    246 corner, ~3,000 surf + outlier per key), drawn from make_s2m_problem's
    maps in the camera frame, on a circle of 0.5 m steps, 1 s apart; the newest
    key lies beside key 0 and its stored pose is off by 1 m and 3 deg of yaw.
    detectLoopClosure picks key 0; the target is keys 0..25
    (historyKeyframeSearchNum 25, clipped at 0), the source the newest key,
    not downsampled.  The ICP (100 m, 100 iterations) runs through
    slio_icp_align at several batch sizes and through the lockstep loop on the
    same clouds; the host figure restates the ICP as s2m_loop's does."""
    import math
    import lego_map_model as M
    from agi_lidar_slam_amd import _lib as L, synth
    from agi_lidar_slam_amd.lego_map import CORNER, LOOP, OUTLIER, SURF, LegoMapping
    from agi_lidar_slam_amd.lio_sam import icp_align_device, icp_align_lockstep
    pr = synth.make_s2m_problem()
    pools = [M.cam_points(pr["corner_map"]), M.cam_points(pr["surf_map"]), M.cam_points(pr["surf_map"])]
    rng = np.random.default_rng(12)
    mp = LegoMapping(max_points=20000, loop_closure=True)
    lib = mp.lib
    radius = 0.5 * n_kf / (2.0 * math.pi)

    def pose_of(k):
        th = 2.0 * math.pi * k / n_kf
        return np.array([0.004 * math.sin(th), 0.5 * math.pi - th, -0.003 * math.cos(th), radius * math.cos(th),
                         0.01 * k, radius * math.sin(th)], np.float32)

    def to_sensor(pose, pw):   # the inverse of M.to_map, in double
        rx, ry, rz, tx, ty, tz = (float(v) for v in pose)
        q = pw.astype(np.float64) - np.array([tx, ty, tz])
        cr, sr, cp, sp, cy, sy = (math.cos(rx), math.sin(rx), math.cos(ry), math.sin(ry), math.cos(rz),
                                  math.sin(rz))
        x2, z2, y2 = cp * q[:, 0] - sp * q[:, 2], sp * q[:, 0] + cp * q[:, 2], q[:, 1]
        y1, z1 = cr * y2 + sr * z2, -sr * y2 + cr * z2
        return np.column_stack([cy * x2 + sy * y1, -sy * x2 + cy * y1, z1]).astype(np.float32)

    for k in range(n_kf):
        true = pose_of(k)
        stored = true.copy()
        if k == n_kf - 1:
            stored = (stored + np.array([0, np.deg2rad(3.0), 0, 0.8, 0.0, -0.6], np.float32)).astype(np.float32)
        for which, pool, n in zip((CORNER, SURF, OUTLIER), pools, (n_corner, n_surf, n_outlier)):
            w = pool[rng.choice(pool.shape[0], n)] + rng.normal(0, 0.05, (n, 3))
            c = to_sensor(true, w)
            x, y, z = (np.ascontiguousarray(c[:, a]) for a in range(3))
            L.check(lib.slio_scan_upload(mp.handle(which), L.fptr(x), L.fptr(y), L.fptr(z), n), "scan_upload")
        mp._tobe, mp._aft, mp.timeLaserOdometry = stored.copy(), stored.copy(), float(k)
        assert mp.saveKeyFramesAndFactor()
    latest = n_kf - 1
    closest = mp.detectLoopClosure()
    med = lambda v: float(np.median(v))  # noqa: E731
    mp.loop_clouds(latest, closest)
    t_asm = []
    for _ in range(reps):
        t0 = time.perf_counter()
        cnt = mp.loop_clouds(latest, closest)
        t_asm.append((time.perf_counter() - t0) * 1e3)
    h = mp.handle(LOOP)

    class Own:
        pass
    own = Own()
    icp_align_lockstep(lib, h, 100.0, max_iterations=100, owner=own)
    t_lock = []
    for _ in range(reps):
        t0 = time.perf_counter()
        rl = icp_align_lockstep(lib, h, 100.0, max_iterations=100, owner=own)
        t_lock.append((time.perf_counter() - t0) * 1e3)
    far_first = own.icp_far_first
    dev_loop, waits = {}, {}
    for batch in (0, 1, 2, 4, 8, 16, 32, 100):
        icp_align_device(lib, h, 100.0, batch=batch, max_iterations=100)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            rd = icp_align_device(lib, h, 100.0, batch=batch, max_iterations=100, owner=own)
            ts.append((time.perf_counter() - t0) * 1e3)
        name = "default" if batch == 0 else str(batch)
        dev_loop[name] = med(ts)
        if batch:
            waits[name] = -(-rd[3] // batch) + 1
    same = bool(rd[0] == rl[0] and np.array_equal(rd[1], rl[1]) and rd[2:] == rl[2:] and
                own.icp_far_first == far_first)
    # the fitness pass alone
    sums, nc = np.zeros(16), C.c_int64()
    T = np.ascontiguousarray(rl[1].reshape(16))
    t_fit = []
    for _ in range(reps + 1):
        t0 = time.perf_counter()
        L.check(lib.slio_icp_correspond(h, L.fptr(T), 1, np.inf, L.dptr(sums), C.byref(nc)), "icp fitness")
        t_fit.append((time.perf_counter() - t0) * 1e3)
    # the whole call, both ICP paths
    mp.currentRobotPosPoint = mp.cloudKeyPoses3D[latest, :3].copy()
    t_call = {}
    for name, lockstep in (("device", False), ("lockstep", True)):
        mp.performLoopClosure(lockstep=lockstep)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            cl = mp.performLoopClosure(lockstep=lockstep)
            ts.append((time.perf_counter() - t0) * 1e3)
        t_call[name] = med(ts)
    n_src, n_tgt = int(cnt[1]), int(cnt[3])
    xs = [np.zeros(n_src, np.float32) for _ in range(3)]
    L.check(lib.slio_scan_download(h, *(L.fptr(a) for a in xs)), "scan_download")
    xt = [np.zeros(n_tgt, np.float32) for _ in range(3)]
    ids, got = np.zeros(n_tgt, np.uint32), C.c_int64()
    L.check(lib.slio_map_download(h, *(L.fptr(a) for a in xt), ids.ctypes.data_as(C.POINTER(C.c_uint32)), n_tgt,
                                  C.byref(got)), "map_download")
    src, tgt = np.stack(xs, 1), np.stack(xt, 1)
    host_icp(src, tgt, 100.0)
    host = host_icp(src, tgt, 100.0)
    print(json.dumps({
        "bench": "lego_loop_closure", "keyframes": n_kf, "points_per_keyframe": [n_corner, n_surf, n_outlier],
        "latest": latest, "closest": int(closest), "source_points": n_src, "target_concatenated": int(cnt[2]),
        "target_points": n_tgt, "ms_two_assemblies": med(t_asm),
        "iterations": rl[3], "convergence_state": rl[4], "converged": rl[0], "fitness": rl[2],
        "far_queries_first_pass": far_first, "ms_fitness_pass": med(t_fit[1:]),
        "ms_icp_lockstep_incl_fitness": med(t_lock), "host_waits_lockstep": rl[3] + 1,
        "ms_icp_align_by_batch": dev_loop, "host_waits_by_batch": waits, "same_bits_as_lockstep": same,
        "ms_perform_loop_closure": t_call, "closure_found": cl is not None,
        "host_ckdtree_numpy": host, "kernel_times": "not measured"}), flush=True)
    mp.close()


def lego_odom(sweeps=12, restate=True):
    """LeGO-LOAM front-end + scan-to-scan odometry on a VLP-16 16 x 1800
    sequence (the moving analytic room of tests/test_lego_odom_cpu.py): sweeps
    per second of upload + front-end + odometry, the front-end and the
    odometry call alone, the lockstep loop (one pass and one host step per
    iteration) and the numpy restatement (tests/lego_odom_model.py) on one
    sweep's clouds, with the iteration counts."""
    import lego_odom_model as M
    from test_lego_odom_cpu import moving_sweep
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoParams
    med = lambda v: float(np.median(v))  # noqa: E731
    scans = [moving_sweep(k, horizon=1800) for k in range(sweeps)]
    fe = LegoFrontEnd(LegoParams())
    fe.enable_odometry()
    fe.set_imu(None)
    t_all, t_fe, t_od, iters, rows = [], [], [], [], []
    lock = model = None
    for rep in range(2):                     # the first round warms up
        fe.reset_odometry()
        for k, sc in enumerate(scans):
            t0 = time.perf_counter()
            fe.upload(sc["x"], sc["y"], sc["z"])
            fe.run()
            t1 = time.perf_counter()
            if rep == 1 and k == sweeps - 1:
                # the last sweep once more on the host: lockstep, then the restatement
                f, st = fe.features(), fe.odometry_state()
                last = fe.last_clouds()
                tc, P = st["transform_cur"].copy(), st["mat_p"].copy()
                tl = time.perf_counter()
                li = [fe.odometry_lockstep(kind, f[name].shape[0], tc, st["is_degenerate"], P)[0]
                      for kind, name in ((0, "surfPointsFlat"), (1, "cornerPointsSharp"))]
                lock = dict(ms=(time.perf_counter() - tl) * 1e3, iters=li)
                if restate:
                    m = M.OdomModel()
                    m.inited, m.transformCur = True, st["transform_cur"].copy()
                    m.corner_last, m.surf_last = last["laserCloudCornerLast"], last["laserCloudSurfLast"]
                    tm = time.perf_counter()
                    mo = m.update_transformation(f["cornerPointsSharp"], f["surfPointsFlat"])
                    model = dict(ms=(time.perf_counter() - tm) * 1e3, iters=mo["iters"])
                t1 = time.perf_counter()
            o = fe.odometry_run()
            t2 = time.perf_counter()
            if rep == 1 and k > 0:
                t_fe.append((t1 - t0) * 1e3)
                t_od.append((t2 - t1) * 1e3)
                t_all.append((t2 - t0) * 1e3)
                iters.append(o["iters"])
                rows.append(o["rows"])
    c = fe.counts
    print(json.dumps({
        "bench": "lego_odom", "n_scan": 16, "horizon_scan": 1800, "sweeps": len(t_all),
        "points_per_sweep": int(scans[0]["x"].size), "n_sharp": int(c.n_sharp), "n_flat": int(c.n_flat),
        "n_corner_last": o["n_corner_last"], "n_surf_last": o["n_surf_last"],
        "sweeps_per_s_frontend_plus_odometry": 1e3 / med(t_all[:-1]), "ms_upload_frontend": med(t_fe[:-1]),
        "ms_odometry_call": med(t_od), "iterations_surf_corner": [int(np.median([i[0] for i in iters])),
                                                                  int(np.median([i[1] for i in iters]))],
        "rows_surf_corner": [int(np.median([r[0] for r in rows])), int(np.median([r[1] for r in rows]))],
        "lockstep_loop": lock, "numpy_restatement_loop": model}), flush=True)
    fe.close()


def lego_map(calls=8, restate=True):
    """LeGO-LOAM mapping (LegoMapping: slio_lmap_*) behind the front-end and
    odometry on the 16 x 1800 sequence of lego_odom: ms per mapping call and
    its split (downsampleCurrentScan from the device clouds,
    extractSurroundingKeyFrames, scan2MapOptimization, saveKeyFramesAndFactor),
    iterations, map and scan sizes, whether the searches took the far path;
    the first call apart (it allocates); and the last call once more through
    the host restatement (tests/lego_map_model.py: numpy, the oracle's kd-tree
    and VoxelGrid) on the same data."""
    import lego_map_model as M
    from oracle import oracle as O
    from test_lego_odom_cpu import SWEEP_T, moving_sweep
    from agi_lidar_slam_amd.lego import LegoFrontEnd, LegoMapping, LegoParams
    from agi_lidar_slam_amd.lego_map import CORNER, OUTLIER, SURF, SURF_TOTAL
    O.build()
    fe = LegoFrontEnd(LegoParams())
    fe.enable_odometry()
    mp = LegoMapping(max_points=20000)
    rows, host, k = [], None, 0
    while len(rows) < calls and k < 10 * calls:
        sc = moving_sweep(k, horizon=1800)
        out = fe.runFeatureAssociation(sc["x"], sc["y"], sc["z"], None, k * SWEEP_T)
        t = (k + 1) * SWEEP_T
        k += 1
        if not out["published"]:
            continue
        mp.laserOdometryHandler(out["transform_sum"], t)
        if not (t - mp.timeLastProcessing >= float(np.float32(mp.params.mapping_interval))):
            continue
        mp.timeLastProcessing = t
        t0 = time.perf_counter()
        tobe0 = mp.transformAssociateToMap()
        t1 = time.perf_counter()
        mp.extractSurroundingKeyFrames()
        t2 = time.perf_counter()
        mp.downsampleCurrentScan(fe)
        t3 = time.perf_counter()
        mp.scan2MapOptimization()
        t4 = time.perf_counter()
        far = [mp.far_queries(0), mp.far_queries(1)] if mp.iterations else [0, 0]
        if restate and len(rows) == calls - 1:
            # the same call on the host, before the keyframe is saved
            last = fe.last_clouds()
            cl, sl, ol = (last[n][:, :3] for n in ("laserCloudCornerLast", "laserCloudSurfLast", "outlierCloudLast"))
            keys = list(mp.surroundingExistingKeyPosesID)
            kf = {kk: [mp.keyframe(w, kk) for w in (CORNER, SURF, OUTLIER)] for kk in set(keys)}
            poses = mp.cloudKeyPoses6D
            h0 = time.perf_counter()
            cds, sds, ods = O.voxel_grid(cl, 0.2), O.voxel_grid(sl, 0.4), O.voxel_grid(ol, 0.4)
            tds = O.voxel_grid(np.concatenate([sds, ods]), 0.4)
            h1 = time.perf_counter()
            cmap = O.voxel_grid(np.concatenate([M.to_map(poses[kk], kf[kk][0]) for kk in keys]), 0.2)
            smap = O.voxel_grid(np.concatenate([M.to_map(poses[kk], kf[kk][j]) for kk in keys for j in (1, 2)]), 0.4)
            h2 = time.perf_counter()
            tm, im, _, _ = M.scan2map(tobe0, cds, tds, cmap, smap, lambda m_, q: O.Tree(m_).knn(q, 5))
            h3 = time.perf_counter()
            host = dict(ms_feed=(h1 - h0) * 1e3, ms_extract=(h2 - h1) * 1e3, ms_optimise=(h3 - h2) * 1e3,
                        ms_call=(h3 - h0) * 1e3, iterations=im,
                        same_bits_as_device=bool(np.array_equal(tm, mp.transformTobeMapped) or mp.imuPointerLast >= 0),
                        same_clouds=bool(np.array_equal(cds, mp.scan(CORNER)) and np.array_equal(tds, mp.scan(SURF_TOTAL))
                                         and np.array_equal(cmap, mp.map_points(0))
                                         and np.array_equal(smap, mp.map_points(1))))
        t5 = time.perf_counter()
        mp.saveKeyFramesAndFactor()
        t6 = time.perf_counter()
        rows.append(dict(ms_call=(t4 - t0 + t6 - t5) * 1e3, ms_associate=(t1 - t0) * 1e3, ms_extract=(t2 - t1) * 1e3,
                         ms_feed=(t3 - t2) * 1e3, ms_optimise=(t4 - t3) * 1e3, ms_save=(t6 - t5) * 1e3,
                         iterations=mp.iterations, far_queries_last_pass=far, keys=len(mp.surroundingExistingKeyPosesID),
                         map_counts=[int(v) for v in mp.map_counts], scan_counts=[int(v) for v in mp.scan_counts],
                         saved=mp.saved_last))
    later = rows[1:]
    mean = lambda key: float(np.mean([r[key] for r in later]))  # noqa: E731
    print(json.dumps({
        "bench": "lego_map", "n_scan": 16, "horizon_scan": 1800, "sweeps": k, "mapping_calls": len(rows),
        "first_call": rows[0],
        "mean_after_first": {key: mean(key) for key in ("ms_call", "ms_associate", "ms_extract", "ms_feed",
                                                        "ms_optimise", "ms_save", "iterations")},
        "last_call": rows[-1], "keyframes": int(mp.cloudKeyPoses6D.shape[0]),
        "far_path_used": bool(any(sum(r["far_queries_last_pass"]) for r in rows)),
        "host_restatement_last_call": host, "kernel_times": "not measured"}), flush=True)
    mp.close()
    fe.close()


def livox_map(calls=12, n_scan=20000):
    """livox_mapping's laserMapping (LivoxMapping: slio_lvx_*) on
    synth.make_trajectory's Avia frames, 0.3 m apart.  Feature clouds, crude,
    from what the scene knows (as make_s2m_problem makes them): corner = points
    on the buildings' vertical edges within 40 m of the sensor, surf = the whole
    frame.  One mapper runs `process` per frame (ms per mapping call); a second
    one runs the same calls stage by stage for the split (select + gather and
    index, downsample, optimise, update -- its update re-uploads the scans, so
    the split's sum is above the one-call figure).  The map frame is the first
    frame's.  The first call apart (no map yet, and it allocates); the last
    call once more through tests/livox_map_model.py (numpy, the oracle's
    kd-tree and VoxelGrid) from a copy of the map as it stood."""
    import livox_map_model as M
    from oracle import oracle as O
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    O.build()
    seed, n_map = 20261015, 200000
    frames = synth.make_trajectory(seed, n_map, calls, n_scan, step=0.3)
    scene = synth.make_scene(seed, n_map)
    rng = np.random.default_rng(4)
    lines = []
    for bx in scene.boxes:
        for (cx, cy) in ((bx[0], bx[1]), (bx[2], bx[1]), (bx[0], bx[3]), (bx[2], bx[3])):
            z = np.arange(0.0, bx[5], 0.1)
            lines.append(np.stack([cx + rng.normal(0, 0.005, z.size), cy + rng.normal(0, 0.005, z.size), z], 1))
    edges = np.concatenate(lines)

    def knn(kind, mp, world):
        k = M.KNN[kind]
        if len(mp) < k or len(world) == 0:
            return np.zeros((len(world), 0), np.int32), np.zeros((len(world), 0), np.float32)
        return O.Tree(mp).knn(world, k)

    dev, lock = LivoxMapping(), LivoxMapping()
    model = M.Mapper(O.voxel_grid, knn)
    rows, host = [], None
    tobe = np.zeros(6, np.float32)
    for k, fr in enumerate(frames):
        R = synth.quat_matrix(fr.gt_rot)
        t = fr.gt_pos + R @ synth.AVIA_T_LI
        near = edges[np.linalg.norm(edges[:, :2] - t[:2], axis=1) < 40][::3]
        corner = ((near + rng.normal(0, 0.01, near.shape) - t) @ R).astype(np.float32)
        surf = np.ascontiguousarray(fr.body, np.float32)
        last = k == len(frames) - 1
        if last:
            # the model catches up with the device map and pose as they stand (untimed)
            for kind in range(2):
                sz = dev.cube_sizes(kind)
                model.cubes[kind] = {int(i): dev.get_cube(kind, int(i)) for i in np.nonzero(sz)[0]}
            model.cen = [int(v) for v in dev.laserCloudCen]
            model.tobe[:], model.aft[:], model.last[:] = dev._transforms()
        t0 = time.perf_counter()
        dev.process(corner, surf)
        t1 = time.perf_counter()
        # the same call in stages
        _, valid, _ = lock.select_cubes(tobe)
        maps = lock.build_maps()
        s1 = time.perf_counter()
        scans = lock.feed_host(corner, surf)
        s2 = time.perf_counter()
        tobe, iters, _ = lock.optimize(tobe)
        s3 = time.perf_counter()
        totals = lock.update_map(tobe, lock.scan(0), lock.scan(1))
        s4 = time.perf_counter()
        sizes = [dev.cube_sizes(kind) for kind in range(2)]
        rows.append(dict(ms_call=(t1 - t0) * 1e3, ms_select_gather=(s1 - t1) * 1e3, ms_downsample=(s2 - s1) * 1e3,
                         ms_optimise=(s3 - s2) * 1e3, ms_update_staged=(s4 - s3) * 1e3, iterations=dev.iterations,
                         same_pose_staged=bool(np.array_equal(tobe, dev.transformTobeMapped)),
                         scan_corner_surf_down=[int(v) for v in scans], map_searched=[int(v) for v in maps],
                         map_total=[int(v) for v in totals], valid_cubes=len(valid),
                         nonempty_cubes=[int((sz > 0).sum()) for sz in sizes],
                         largest_cube=[int(sz.max()) for sz in sizes]))
        if last:
            h0 = time.perf_counter()
            it_m = model.process(corner, surf)
            h1 = time.perf_counter()
            host = dict(ms_call=(h1 - h0) * 1e3, iterations=it_m,
                        same_bits_as_device=bool(np.array_equal(model.tobe, dev.transformTobeMapped)
                                                 and all(np.array_equal(model.sizes(kd), dev.cube_sizes(kd))
                                                         for kd in range(2))))
    later = rows[1:]
    mean = lambda key: float(np.mean([r[key] for r in later]))  # noqa: E731
    R = synth.quat_matrix(frames[0].gt_rot)
    t_first = frames[0].gt_pos + R @ synth.AVIA_T_LI
    t_last = frames[-1].gt_pos + synth.quat_matrix(frames[-1].gt_rot) @ synth.AVIA_T_LI
    moved = float(np.linalg.norm(t_last - t_first))
    print(json.dumps({
        "bench": "livox_map", "pattern": "avia", "n_scan": n_scan, "calls": len(rows), "first_call": rows[0],
        "mean_after_first": {key: mean(key) for key in ("ms_call", "ms_select_gather", "ms_downsample",
                                                        "ms_optimise", "ms_update_staged", "iterations")},
        "last_call": rows[-1], "host_restatement_last_call": host,
        "true_distance_moved": moved, "estimated_distance_moved": float(np.linalg.norm(dev.transformTobeMapped[3:])),
        "host_waits_per_call": "2 maps + 2 feed + 1 per iteration + 2 update (+ 2 when the map shifts)",
        "kernel_times": "not measured"}), flush=True)
    dev.close()
    lock.close()


def livox_reg(n_rays=31000, frames_n=8, reps=20):
    """livox_mapping's scanRegistration (LivoxScanRegistration: slio_lreg_*) on
    synth.make_scan_curve's dense frame (one continuous curve, about 24,000
    returns): ms per registration (the upload, six launches and the wait for
    the counts), the counts, the host restatement (slio_lreg_classify_host)
    beside it; then `process_cloud` over a short drive, 0.25 m per frame: ms
    per call, of which the registration, and the same frames through
    laserCloudHandler + process (clouds down and up again)."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    from agi_lidar_slam_amd.livox_reg import LivoxScanRegistration, classify_host
    seed = 20261015
    scene = synth.make_scene(seed, 1000)
    anchor = np.array([synth.SENSOR_STREET[0] - 3.0, synth.SENSOR_STREET[1] + 0.2, 1.6])
    sc = synth.with_street_furniture(scene, anchor, 0.0)
    frames = [synth.make_scan_curve(sc, anchor + [0.25 * k, 0.0, 0.0], 0.0, n_rays, k0=137 * k, seed=seed + k,
                                    furniture=False) for k in range(frames_n)]
    reg = LivoxScanRegistration()
    reg.run(frames[0])                                   # warm-up
    ms_reg, counts = t_ms(lambda: reg.run(frames[0]), reps)
    ms_host, host = t_ms(lambda: classify_host(frames[0]), 3)
    full, corner, surf = reg.laserCloudHandler(frames[0])
    same = bool(np.array_equal(host["flags"], reg.flags()[0]) and np.array_equal(host["corner"], corner)
                and np.array_equal(host["surf"], surf) and np.array_equal(host["cloud"], full))
    dev, via_host = LivoxMapping(), LivoxMapping()
    reg2 = LivoxScanRegistration()
    rows = []
    for fr in frames:
        t0 = time.perf_counter()
        dev.process_cloud(reg, fr)
        t1 = time.perf_counter()
        reg2.run(fr)
        t2 = time.perf_counter()
        _, c, s = reg2.laserCloudHandler(fr)
        via_host.process(c[:, :3], s[:, :3])
        t3 = time.perf_counter()
        rows.append(dict(ms_process_cloud=(t1 - t0) * 1e3, ms_registration=(t2 - t1) * 1e3,
                         ms_handler_plus_process=(t3 - t2) * 1e3, iterations=dev.iterations,
                         counts=[int(v) for v in reg.counts],
                         same_pose=bool(np.array_equal(dev.transformTobeMapped, via_host.transformTobeMapped))))
    later = rows[1:]
    mean = lambda key: float(np.mean([r[key] for r in later]))  # noqa: E731
    print(json.dumps({
        "bench": "livox_reg", "returns": int(len(frames[0])), "ms_per_registration": ms_reg,
        "counts_cloud_corner_surf": [int(v) for v in counts], "ms_host_restatement": ms_host,
        "host_same_bits_as_device": same, "frames": len(rows), "first_call": rows[0],
        "mean_after_first": {key: mean(key) for key in ("ms_process_cloud", "ms_registration",
                                                        "ms_handler_plus_process", "iterations")},
        "estimated_distance_moved": float(np.linalg.norm(dev.transformTobeMapped[3:])),
        "true_distance_moved": 0.25 * (len(rows) - 1),
        "launches_per_registration": 6, "host_waits_per_registration": 1,
        "host_waits_per_process_cloud": "those of process (2 maps + 2 feed + 1 per iteration + 2 update) + 1",
        "kernel_times": "not measured"}), flush=True)
    for h in (dev, via_host, reg, reg2):
        h.close()


def lio_livox_reg(reps=50):
    """LIO-Livox's ScanRegistration (LioLivoxScanRegistration: slio_llreg_*) on
    synth.make_livox_lines frames: 6 lines of 4000 returns with
    horizon_config.yaml's parameters and 4 lines of 5000 with
    mid360_config.yaml's, and the first again with PartNum 1, where every part
    takes the picking kernel's serial path.  ms per FeatureExtract (the staging copy, the upload,
    nine launches and the wait for the counts; host wall clock around the
    synchronous call, mean of `reps` after a warm-up), the counts, and the same
    message through the host restatement (slio_llreg_extract_host, one
    thread) beside it."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.lio_livox import HORIZON, MID360, LioLivoxScanRegistration, extract_host, tiles
    seed = 20261020
    scene = synth.make_scene(seed, 1000)
    pos = np.array([synth.SENSOR_STREET[0] - 3.0, synth.SENSOR_STREET[1] + 0.2, 1.6])
    rows = []
    # the third row reaches the picking kernel's serial path: one part per line
    for name, cfg, per_line in (("horizon_6x4000", HORIZON, 4000), ("mid360_4x5000", MID360, 5000),
                                ("horizon_6x4000_partnum_1", dict(HORIZON, part_num=1), 4000)):
        n_lines = cfg["n_scans"]
        msg = synth.make_livox_lines(scene, pos, 0.0, n_lines, int(per_line * 1.4), seed=seed + 5)
        keep = np.zeros(len(msg["line"]), bool)
        for l in range(n_lines):
            keep[np.nonzero(msg["line"] == l)[0][:per_line]] = True
        msg = {k: np.ascontiguousarray(v[keep]) for k, v in msg.items()}
        reg = LioLivoxScanRegistration(**cfg)
        reg.run(**msg)                                      # warm-up
        long_parts = cfg["part_num"] == 1
        ms_dev, counts = t_ms(lambda: reg.run(**msg), 10 if long_parts else reps)
        ms_host, host = t_ms(lambda: extract_host(reg.params, **msg), 2 if long_parts else 5)
        full, corner, surf = reg.FeatureExtract(**msg)
        same = all(np.array_equal(a.view(np.uint32), b.view(np.uint32))
                   for a, b in ((full, host["cloud"]), (corner, host["corner"]), (surf, host["surf"])))
        same = bool(same and all(np.array_equal(reg.flags(l)[0], host["flags"][l]) for l in range(n_lines)))
        rows.append({"input": name, "points": int(len(msg["xyz"])), "ms_per_feature_extract": ms_dev,
                     "counts_cloud_corner_surf": [int(v) for v in counts], "ms_host_restatement": ms_host,
                     "host_same_bits_as_device": same})
        reg.close()
    print(json.dumps({"bench": "lio_livox_reg", "inputs": rows, "launches_per_message": 9,
                      "host_waits_per_message": 1, "picking": "one wavefront per line, parts in order",
                      "tiles_chain_per_thread_workgroup_pick_fast_block": list(tiles()),
                      "kernel_times": "not measured"}), flush=True)


def aloam_reg(reps=20):
    """A-LOAM's scanRegistration (AloamScanRegistration: slio_aloam_*) on a
    VLP-16 sweep at horizon 1800 and a 64-line sweep at horizon 2083
    (synth.make_spinning_sweep): ms per registration (the upload, seven
    launches and the wait for the counts; host wall clock around the
    synchronous call, mean of `reps` after a warm-up), the five counts, and
    the same input through the host restatement (slio_aloam_register_host, one
    thread) beside it."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.aloam import CLOUDS, AloamScanRegistration, register_host
    upper, lower = 2.0 - np.arange(33) / 3.0, -8.83 - np.arange(1, 32) / 2.0
    inputs = (("vlp16_h1800", 16, -15.0 + 2.0 * np.arange(16), 1800),
              ("hdl64_h2083", 64, np.concatenate([upper, lower]), 2083))
    rows = []
    for name, n_scans, beams, horizon in inputs:
        sw = synth.make_spinning_sweep(beams, horizon=horizon)
        xyz = np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"]], 1), np.float32)
        reg = AloamScanRegistration(n_scans=n_scans)
        reg.run(xyz)                                     # warm-up
        ms_reg, counts = t_ms(lambda: reg.run(xyz), reps)
        ms_host, host = t_ms(lambda: register_host(xyz, n_scans=n_scans), 3)
        got = reg.laserCloudHandler(xyz)
        same = all(np.array_equal(got[k].view(np.uint32), host[k].view(np.uint32)) for k in CLOUDS)
        rows.append({"input": name, "points": int(len(xyz)), "ms_per_registration": ms_reg,
                     "counts": [int(v) for v in counts], "ms_host_restatement": ms_host,
                     "host_same_bits_as_device": bool(same)})
        reg.close()
    print(json.dumps({"bench": "aloam_reg", "inputs": rows, "launches_per_registration": 7,
                      "host_waits_per_registration": 1, "kernel_times": "not measured"}), flush=True)


def aloam_odom(reps=20):
    """A-LOAM's laserOdometry (AloamOdometry: slio_aloam_odom_*) on aloam_reg's
    two inputs.  The second sweep is the first one's returns seen from a
    sensor that has moved by 0.02 rad of yaw and (0.15, 0.04, 0) m; the two
    alternate, so every call is a full odometry call (two associations, two
    solves) between different sweeps.  Host wall clock around synchronous
    calls, mean of `reps` after a warm-up: ms per odometry call from host
    feature clouds; ms of one association launch and its wait (the lockstep
    entry), from which the split is estimated as 2 associations + the rest; ms
    per sweep of registration plus odometry, device to device; the same calls
    through the host restatement (one thread) beside it."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.aloam import (CLOUDS, AloamOdometry, AloamOdometryHost, AloamScanRegistration,
                                          register_host)
    upper, lower = 2.0 - np.arange(33) / 3.0, -8.83 - np.arange(1, 32) / 2.0
    inputs = (("vlp16_h1800", 16, -15.0 + 2.0 * np.arange(16), 1800),
              ("hdl64_h2083", 64, np.concatenate([upper, lower]), 2083))
    rows = []
    for name, n_scans, beams, horizon in inputs:
        sw = synth.make_spinning_sweep(beams, horizon=horizon)
        a = np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"]], 1), np.float32)
        c, s_ = np.cos(0.02), np.sin(0.02)
        d = a.astype(np.float64) - np.array([0.15, 0.04, 0.0])
        b = np.ascontiguousarray(np.stack([c * d[:, 0] + s_ * d[:, 1], -s_ * d[:, 0] + c * d[:, 1], d[:, 2]], 1),
                                 np.float32)
        raw = (a, b)
        feats = [tuple(register_host(x, n_scans=n_scans)[k] for k in CLOUDS[1:]) for x in raw]
        od = AloamOdometry(n_scans=n_scans, skip_frame_num=1)
        host = AloamOdometryHost(n_scans=n_scans, skip_frame_num=1)
        for k in range(3):                               # warm-up; both now hold sweep 0 as the last clouds
            r_dev, r_host = od.process(*feats[k % 2]), host.process(*feats[k % 2])
        same = r_dev == r_host
        t0, k0 = time.perf_counter(), 3
        for k in range(k0, k0 + reps):
            r_dev = od.process(*feats[k % 2])
        ms_odom = (time.perf_counter() - t0) * 1e3 / reps
        t0 = time.perf_counter()
        for k in range(k0, k0 + 4):
            r_host = host.process(*feats[k % 2])
        ms_host = (time.perf_counter() - t0) * 1e3 / 4
        ms_assoc, _ = t_ms(lambda: od.associate(r_dev["q_last_curr"], r_dev["t_last_curr"]), reps)
        reg = AloamScanRegistration(n_scans=n_scans)
        reg.enable_odometry(skip_frame_num=1)
        for k in range(3):
            reg.laserOdometry(raw[k % 2])
        t0 = time.perf_counter()
        for k in range(3, 3 + reps):
            r_view = reg.laserOdometry(raw[k % 2])
        ms_sweep = (time.perf_counter() - t0) * 1e3 / reps
        ps = r_dev["passes"]
        rows.append({"input": name, "points": int(len(a)), "queries": [int(len(feats[1][0])), int(len(feats[1][2]))],
                     "last_points": [int(len(feats[0][1])), int(len(feats[0][3]))],
                     "ms_per_odometry_call": ms_odom, "ms_one_association_and_wait": ms_assoc,
                     "ms_two_solves_and_rest_est": ms_odom - 2 * ms_assoc,
                     "correspondences": [[p["corner"], p["plane"]] for p in ps],
                     "iterations": [p["iterations"] for p in ps], "stops": [p["stop"] for p in ps],
                     "ms_registration_plus_odometry": ms_sweep,
                     "view_pose_same_bits_as_host_clouds": bool(r_view["q_last_curr"] == r_dev["q_last_curr"]),
                     "ms_host_restatement": ms_host, "host_same_bits_as_device": bool(same)})
        for h in (od, reg.odometry, reg):
            h.close()
    print(json.dumps({"bench": "aloam_odom", "inputs": rows,
                      "launches_per_odometry_call": "1 memset + 5 kernels (store_last, 2 x assoc, 2 x solve)",
                      "host_waits_per_odometry_call": 1, "kernel_times": "not measured"}), flush=True)


def aloam_map(reps=20):
    """A-LOAM's laserMapping (AloamMapping: slio_aloam_map_*) on aloam_odom's
    two inputs and two sweeps.  The mapper takes each sweep's
    cornerPointsLessSharp and surfPointsLessFlat (the odometry's last clouds)
    and the sweep's true pose with an offset of 2 mrad and (3, -2, 1) cm as the
    odometry pose; the two sweeps alternate, so after the first two calls every
    call is a full mapping call (two associations, two solves, the map update)
    on a map that has stopped growing.  Host wall clock around synchronous
    calls, mean of `reps` after a warm-up of four; the same calls through the
    host restatement (one thread, brute-force 5-NN) beside it, mean of 2."""
    from agi_lidar_slam_amd import synth
    from agi_lidar_slam_amd.aloam import AloamMapping, AloamMappingHost, register_host
    upper, lower = 2.0 - np.arange(33) / 3.0, -8.83 - np.arange(1, 32) / 2.0
    inputs = (("vlp16_h1800", 16, -15.0 + 2.0 * np.arange(16), 1800),
              ("hdl64_h2083", 64, np.concatenate([upper, lower]), 2083))
    rows = []
    for name, n_scans, beams, horizon in inputs:
        sw = synth.make_spinning_sweep(beams, horizon=horizon)
        a = np.ascontiguousarray(np.stack([sw["x"], sw["y"], sw["z"]], 1), np.float32)
        c, s_ = np.cos(0.02), np.sin(0.02)
        d = a.astype(np.float64) - np.array([0.15, 0.04, 0.0])
        b = np.ascontiguousarray(np.stack([c * d[:, 0] + s_ * d[:, 1], -s_ * d[:, 0] + c * d[:, 1], d[:, 2]], 1),
                                 np.float32)
        clouds = []
        for x in (a, b):
            w = register_host(x, n_scans=n_scans)
            clouds.append((w["cornerPointsLessSharp"], w["surfPointsLessFlat"]))
        poses = (([0.0, 0.0, np.sin(0.001), np.cos(0.001)], [0.03, -0.02, 0.01]),
                 ([0.0, 0.0, np.sin(0.011), np.cos(0.011)], [0.18, 0.02, 0.01]))
        dev, host = AloamMapping(), AloamMappingHost()
        for k in range(4):
            r_dev, r_host = dev.process(*clouds[k % 2], *poses[k % 2]), host.process(*clouds[k % 2], *poses[k % 2])
        same = r_dev == r_host
        t0 = time.perf_counter()
        for k in range(4, 4 + reps):
            r_dev = dev.process(*clouds[k % 2], *poses[k % 2])
        ms_dev = (time.perf_counter() - t0) * 1e3 / reps
        t0 = time.perf_counter()
        for k in range(4, 6):
            r_host = host.process(*clouds[k % 2], *poses[k % 2])
        ms_host = (time.perf_counter() - t0) * 1e3 / 2
        ps = r_dev["passes"]
        rows.append({"input": name, "last_points": [int(len(clouds[1][0])), int(len(clouds[1][1]))],
                     "stack": r_dev["stack_size"], "map": r_dev["map_size"], "ms_per_mapping_call": ms_dev,
                     "factors": [[p["corner"], p["plane"]] for p in ps], "iterations": [p["iterations"] for p in ps],
                     "stops": [p["stop"] for p in ps], "ms_host_restatement": ms_host,
                     "host_same_bits_as_device": bool(same)})
        dev.close()
        host.close()
    print(json.dumps({"bench": "aloam_map", "inputs": rows,
                      "launches_of_the_solve": "24 (per pass 2 x associate, 5 x evaluate, 5 x control)",
                      "host_waits_per_mapping_call": "7 (2 scan VoxelGrids, 2 grid boxes, 1 result, 2 map updates)",
                      "kernel_times": "not measured"}), flush=True)


if __name__ == "__main__":
    what = sys.argv[1:] or ["mapping", "preproc", "s2m"]
    if "aloam_map" in what:
        aloam_map()
    if "aloam_odom" in what:
        aloam_odom()
    if "aloam_reg" in what:
        aloam_reg()
    if "lio_livox_reg" in what:
        lio_livox_reg()
    if "livox_reg" in what:
        livox_reg()
    if "livox_map" in what:
        livox_map()
    if "lego_map" in what:
        lego_map()
    if "lego_odom" in what:
        lego_odom()
    if "lego_loop" in what:
        lego_loop()
    if "s2m_loop" in what:
        s2m_loop()
    if "s2m_map" in what:
        s2m_map()
    if "mapping" in what:
        mapping(10_000_000, 100_000)
    if "chain" in what:
        chain(10_000_000, int(os.environ.get("CHAIN_RAW", "100000")))
    if "preproc" in what:
        preproc(200_000)
    if "s2m" in what:
        s2m()
