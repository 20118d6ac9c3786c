"""CPU tests of the LeGO-LOAM mapping back-end (slio_lmap_*, include/slio.h):
the host formulas against the numpy restatement (tests/lego_map_model.py) to
the bit, the M x N QR, the host key selection against a plain-loop
restatement, the frame convention of the converted scan-to-map problem, and
the argument checks that need no device.  No GPU.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lego_map_model as M  # noqa: E402
import lego_odom_model as MO  # noqa: E402

from agi_lidar_slam_amd import _lib as L  # noqa: E402
from agi_lidar_slam_amd.lego import TransformFusion, extract_surrounding  # noqa: E402

F = np.float32
EINVAL = -1


@pytest.fixture(scope="module")
def lib():
    return L.load()


def same_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan], err_msg=what)


def triples(n=24):
    """(transformSum, transformBefMapped, transformAftMapped): zero rotations,
    |rx| near 1.2 rad, and random ones."""
    rng = np.random.default_rng(7)
    out = []
    for k in range(n):
        t = np.concatenate([rng.uniform(-0.6, 0.6, (3, 3)), rng.uniform(-30, 30, (3, 3))], 1).astype(F)
        if k == 0:
            t[:] = 0
        elif k == 1:
            t[:, :3] = 0                      # zero rotations, translations only
        elif k == 2:
            t[0, :3] = 0
        elif k in (3, 4, 5):
            t[:, 0] = (1.2 if k != 4 else -1.2) + rng.uniform(-0.02, 0.02, 3)   # |rx| near 1.2
        out.append(t)
    return out


def c_associate(lib, ts, tb, ta):
    out = np.empty(6, F)
    assert lib.slio_lmap_associate_to_map(L.fptr(ts), L.fptr(tb), L.fptr(ta), L.fptr(out)) == 0
    return out


def test_associate_to_map_bits(lib):
    for k, t in enumerate(triples()):
        ts, tb, ta = (np.ascontiguousarray(v) for v in t)
        same_bits(c_associate(lib, ts, tb, ta), M.associate_to_map(ts, tb, ta), f"triple {k}")
    z = np.zeros(6, F)
    same_bits(c_associate(lib, z, z, z), z, "identity")


def c_update(lib, tm, ts, t_odom, imu, last, front):
    tm = np.array(tm, F)
    bef, aft, fr = np.empty(6, F), np.empty(6, F), C.c_int32(front)
    it, ir, ip = imu
    assert lib.slio_lmap_transform_update(L.fptr(tm), L.fptr(ts), t_odom, F(0.1), L.dptr(it), L.fptr(ir), L.fptr(ip),
                                          it.size, last, C.byref(fr), L.fptr(bef), L.fptr(aft)) == 0
    return tm, bef, aft, fr.value


@pytest.mark.parametrize("case", ["no_imu", "latest", "interpolate", "wrapped"])
def test_transform_update_bits(lib, case):
    rng = np.random.default_rng(3)
    n = 200
    it = np.zeros(n, np.float64)
    ir, ip = np.zeros(n, F), np.zeros(n, F)
    last, front = -1, 0
    t_odom = 10.0034                                   # between two IMU samples
    if case != "no_imu":
        m = 40
        off = 190 if case == "wrapped" else 0          # the ring wraps past its end
        for k in range(m):
            j = (off + k) % n
            it[j] = 9.9 + 0.01 * k                     # 9.90 .. 10.29
            ir[j], ip[j] = rng.uniform(-0.1, 0.1, 2)
        last, front = (off + m - 1) % n, off
        if case == "latest":
            t_odom = 10.5                              # every sample older: the newest one is taken
    for k, t in enumerate(triples(20)):
        tm, ts = np.ascontiguousarray(t[0]), np.ascontiguousarray(t[1])
        got = c_update(lib, tm, ts, t_odom, (it, ir, ip), last, front)
        want = M.transform_update(tm, ts, t_odom, 0.1, it, ir, ip, last, front)
        for g, w, name in zip(got[:3], want[:3], ("tobe", "bef", "aft")):
            same_bits(g, w, f"{case} {name} {k}")
        assert got[3] == want[3]
        if case == "no_imu":
            same_bits(got[0], tm)
        elif k > 2:
            assert not np.array_equal(got[0], tm)       # the blend did something
    if case == "interpolate":
        assert it[want[3]] > t_odom + float(F(0.1)) > it[(want[3] - 1) % n]   # the interpolation branch ran
    if case == "latest":
        assert want[3] == last


def test_fuse_is_the_same_formula_on_the_same_triple(lib):
    tf = TransformFusion()
    same_bits(tf.laserOdometryHandler(np.zeros(6, F)), np.zeros(6, F))
    for k, t in enumerate(triples()):
        ts, tb, ta = (np.ascontiguousarray(v) for v in t)
        tf.odomAftMappedHandler(ta, tb)
        got = tf.laserOdometryHandler(ts)
        same_bits(got, M.associate_to_map(ts, tb, ta), f"fuse {k}")
        same_bits(got, c_associate(lib, ts, tb, ta), f"fuse vs mapper {k}")
        same_bits(tf.transformMapped, got)
    s = L.SlioLmapFusion()
    z = np.zeros(6, F)
    assert lib.slio_lmap_fuse(None, L.fptr(z), None, None) == EINVAL
    assert lib.slio_lmap_fuse(C.byref(s), None, None, None) == EINVAL
    assert lib.slio_lmap_fuse(C.byref(s), L.fptr(z), L.fptr(z), L.fptr(z)) == EINVAL
    assert lib.slio_lmap_fuse(C.byref(s), None, L.fptr(z), None) == EINVAL


def c_qr(lib, m, n, A, b):
    A, b, x = np.ascontiguousarray(A, F), np.ascontiguousarray(b, F), np.full(n, 7, F)
    rc = lib.slio_lmap_qr_solve(m, n, L.fptr(A), L.fptr(b), L.fptr(x))
    assert rc in (0, 1)
    return rc, x


def test_qr_m_by_n(lib):
    rng = np.random.default_rng(5)
    for k in range(40):
        # five points near a plane a metre or so away: surfOptimization's system
        nrm = rng.normal(size=3)
        nrm /= np.linalg.norm(nrm)
        p = rng.uniform(-20, 20, (5, 3))
        p += np.outer(rng.uniform(1, 30) - p @ nrm + rng.normal(0, 0.02, 5), nrm)
        A = p.astype(F).reshape(-1)
        rc, x = c_qr(lib, 5, 3, A, np.full(5, -1, F))
        want = M.qr_solve(A, [F(-1)] * 5, 5, 3)
        assert rc == 0 and want is not None
        same_bits(x, want, f"5x3 {k}")
        np.testing.assert_allclose(x, np.linalg.lstsq(p.astype(F).astype(np.float64), -np.ones(5), rcond=None)[0],
                                   rtol=0, atol=2e-3 * np.abs(x).max())
    # the give-up cases return zero: a zero column (norm 0) and collinear points (R's diagonal below eps)
    A = rng.uniform(-5, 5, (5, 3)).astype(F)
    A[:, 1] = 0
    rc, x = c_qr(lib, 5, 3, A, np.full(5, -1, F))
    assert rc == 1 and M.qr_solve(A.reshape(-1), [F(-1)] * 5, 5, 3) is None
    same_bits(x, np.zeros(3, F))
    A = np.outer(np.arange(1, 6), [1.0, 2.0, 4.0]).astype(F)    # exact in float: rank 1
    rc, x = c_qr(lib, 5, 3, A, np.full(5, -1, F))
    assert rc == 1 and M.qr_solve(A.reshape(-1), [F(-1)] * 5, 5, 3) is None
    same_bits(x, np.zeros(3, F))
    # M = N: the same bits as the square solver's two restatements
    for k in range(30):
        for n in (3, 6):
            B = rng.normal(size=(n + 4, n))
            A = (B.T @ B * 50).astype(F).reshape(-1)              # normal-equation-like
            b = rng.normal(size=n).astype(F)
            rc, x = c_qr(lib, n, n, A, b)
            assert rc == 0
            same_bits(x, M.qr_solve(A, b, n, n), f"{n}x{n} {k}")
            if n == 3:
                same_bits(x, MO.qr_solve3(A, b), f"3x3 vs the odometry model {k}")
    assert lib.slio_lmap_qr_solve(4, 3, L.fptr(A), L.fptr(b), L.fptr(x)) == EINVAL


def test_lm_step_is_the_mapping_step(lib):
    """slio_s2m_lm_step, which slio_lmap_optimize uses, equals the model of
    LeGO-LOAM's LMOptimization :1539-1600 -- degenerate and regular systems,
    the 50-row gate, a singular system."""
    rng = np.random.default_rng(9)
    for k in range(12):
        J = rng.normal(size=(200, 6)) * np.array([3, 3, 3, 1, 1, 1])
        if k % 3 == 1:
            J[:, 4] *= 0.01                                      # one weak direction: eigenvalue < 100
        if k % 3 == 2:
            J[:, 2] = 0                                          # singular
        AtA = (J.T @ J).astype(F).reshape(-1)
        AtB = (J.T @ rng.normal(0, 0.01, 200)).astype(F)
        tf_c, tf_m = np.zeros(6, F) + F(0.1), np.zeros(6, F) + F(0.1)
        state = dict(is_degenerate=0, matP=[F(0)] * 36)
        matP, deg, conv = np.zeros(36, F), C.c_int(0), C.c_int(0)
        for it in range(2):
            rc = lib.slio_s2m_lm_step(L.fptr(AtA), L.fptr(AtB), 200, it, L.fptr(tf_c), C.byref(deg), L.fptr(matP),
                                      C.byref(conv))
            done = M.lm_step(AtA, AtB, 200, it, tf_m, state)
            assert rc == 0 and bool(conv.value) == done
            same_bits(tf_c, tf_m, f"system {k} iteration {it}")
            assert deg.value == state["is_degenerate"] == (1 if k % 3 else 0)
        assert lib.slio_s2m_lm_step(L.fptr(AtA), L.fptr(AtB), 49, 0, L.fptr(tf_c), C.byref(deg), L.fptr(matP),
                                    C.byref(conv)) == 1
        assert M.lm_step(AtA, AtB, 49, 0, tf_m, state) is False
        same_bits(tf_c, tf_m)


def test_keyframe_decision(lib):
    rng = np.random.default_rng(2)
    for k in range(40):
        prev = rng.uniform(-5, 5, 3).astype(F)
        d = rng.normal(size=3)
        cur = (prev + d / np.linalg.norm(d) * (0.3 + rng.choice([-1e-3, -1e-6, 0, 1e-6, 1e-3, 0.5]))).astype(F)
        for nkeys in (0, 3):
            save = C.c_int(-1)
            assert lib.slio_lmap_keyframe_decision(L.fptr(prev), L.fptr(cur), nkeys, 0.3, C.byref(save)) == 0
            assert bool(save.value) == M.keyframe_decision(prev, cur, nkeys)
            if nkeys == 0:
                assert save.value == 1
    z = np.zeros(3, F)
    save = C.c_int()
    assert lib.slio_lmap_keyframe_decision(L.fptr(z), L.fptr(z), 1, 0.3, C.byref(save)) == 0 and save.value == 0
    assert lib.slio_lmap_keyframe_decision(None, L.fptr(z), 1, 0.3, C.byref(save)) == EINVAL


# ------------------------------------------------------------------ the key selection
def plain_extract(kp, cur, existing, radius, leaf):
    """extractSurroundingKeyFrames :1101-1177 as the reference's loops."""
    kp = np.asarray(kp, F)
    cur = np.asarray(cur, F)
    cand = []
    for i in range(kp.shape[0]):
        dx, dy, dz = kp[i, 0] - cur[0], kp[i, 1] - cur[1], kp[i, 2] - cur[2]
        sq = (dx * dx + dy * dy) + dz * dz
        if sq < F(radius) * F(radius):
            cand.append((sq, i))
    cand.sort()
    sel = np.array([kp[i] for _, i in cand], F).reshape(-1, 4)
    # VoxelGrid: all four fields averaged, voxels in ascending index, members in input order
    inv = F(1.0) / F(leaf)
    mn = sel[:, :3].min(axis=0)
    mx = sel[:, :3].max(axis=0)
    lo = np.floor(mn * inv).astype(np.int64)
    div = np.floor(mx * inv).astype(np.int64) - lo + 1
    vox = {}
    for p in sel:
        ijk = (np.floor(p[:3] * inv) - lo.astype(F)).astype(np.int64)
        vox.setdefault(int(ijk[0] + ijk[1] * div[0] + ijk[2] * div[0] * div[1]), []).append(p)
    ds = []
    for v in sorted(vox):
        s = np.zeros(4, F)
        for p in vox[v]:
            s = s + p
        ds.append(s / F(len(vox[v])))
    ids = [int(float(p[3])) for p in ds]
    existing = list(existing)
    i = 0
    while i < len(existing):                  # erase in place
        if existing[i] not in ids:
            del existing[i]
            i -= 1
        i += 1
    for k in ids:                             # append the new keys in surroundingKeyPosesDS order
        if k not in existing:
            existing.append(k)
    return existing, np.array(ds, F).reshape(-1, 4)


def test_extract_surrounding_keys_enter_and_leave():
    # a track along x, a pose every 2.5 m, so each pose has a 1 m voxel of its own
    n = 60
    kp = np.column_stack([2.5 * np.arange(n) + 0.3, 0.2 * np.sin(np.arange(n)), np.zeros(n), np.arange(n)]).astype(F)
    existing, seen = [], []
    for cur in ([10.0, 0, 0], [60.0, 0, 0], [140.0, 0, 0]):       # three successive positions
        want, want_ds = plain_extract(kp, cur, existing, 50.0, 1.0)
        got, got_ds = extract_surrounding(kp, cur, existing, 50.0, 1.0)
        assert got == want
        same_bits(got_ds, want_ds)
        seen.append(set(got))
        # order: survivors keep their places, new keys follow
        survivors = [k for k in existing if k in got]
        assert got[:len(survivors)] == survivors
        existing = got
    assert seen[1] - seen[0] and seen[0] - seen[1]                  # keys entered and keys left
    assert seen[2] - seen[1] and seen[1] - seen[2]
    assert not (seen[0] & seen[2])
    assert extract_surrounding(np.zeros((0, 4), F), [0, 0, 0], [3], 50.0, 1.0)[0] == [3]


def test_extract_surrounding_mean_intensity_quirk():
    # keys 1 and 5 share one 1 m voxel: the downsampled pose's key is int((1 + 5) / 2) = 3,
    # a third key, which lies far outside the radius
    kp = np.zeros((6, 4), F)
    kp[:, 3] = np.arange(6)
    kp[0, :3] = [3.5, 0.5, 0.5]
    kp[1, :3] = [0.2, 0.2, 0.2]
    kp[5, :3] = [0.7, 0.6, 0.4]
    for k in (2, 3, 4):
        kp[k, :3] = [500.0 + k, 0, 0]
    got, ds = extract_surrounding(kp, [0, 0, 0], [1, 0], 50.0, 1.0)
    want, _ = plain_extract(kp, [0, 0, 0], [1, 0], 50.0, 1.0)
    assert got == want == [0, 3]                                    # 1 erased, 0 kept, 3 appended
    assert sorted(int(v) for v in ds[:, 3]) == [0, 3]


# ------------------------------------------------------------------ the frame convention
def test_camera_frame_conversion_of_the_s2m_problem(oracle_mod):
    from agi_lidar_slam_amd import synth
    pb = synth.make_s2m_problem(n_map=20000, n_surf=3000)
    rng = np.random.default_rng(1)
    for scan in (pb["surf_scan"], pb["corner_scan"]):
        for tf in (pb["tf"], pb["tf"] + rng.uniform(-0.3, 0.3, 6).astype(F)):
            want = M.cam_points(oracle_mod.s2m_transform(tf, scan))
            got = M.to_map(M.cam_pose(tf), M.cam_points(scan))
            # either side: nine products and six sums of magnitudes <= |p| + |t|, each within
            # half an ulp -> 8 ulps of that magnitude per side
            mag = np.abs(scan).sum(axis=1).max() + np.abs(tf[3:]).sum()
            assert np.abs(got - want).max() <= 16 * np.finfo(F).eps * mag
            assert np.abs(got - want).max() > 0 or scan.shape[0] == 0   # (not the same arithmetic)


@pytest.mark.parametrize("kind", [0, 1])
def test_cut_fixture_covers_every_branch_and_is_tie_free(oracle_mod, kind):
    """The cut tests/test_gpu_lego_map.py compares coefficients on: the model
    alone selects points, gates points out at 1 m and rejects points by the
    eigenvalue ratio (corner) / the 0.2 plane check (surf) -- otherwise a
    comparison could pass on all-zero outputs -- and no two of a query's six
    nearest float distances are equal."""
    import lego_map_case as K
    ref = K.cut_reference(kind)
    st = ref["stats"]
    assert st["selected"] >= 1 and st["gated"] >= 1 and st["rejected"] >= 1, st
    assert st["selected"] + st["gated"] <= 1500
    assert M.tie_free(ref["sqd6"])
    assert ref["sel"][:65].any() and not ref["sel"][:65].all()        # the small sizes are mixed too
    c = K.cut()
    assert 2000 < c["surf_map"].shape[0] < 10000 and c["corner_scan"].shape == c["surf_scan"].shape == (1500, 3)


# ------------------------------------------------------------------ argument checks
def test_argument_errors_without_a_device(lib):
    z6, i64 = np.zeros(6, F), np.zeros(4, np.int64)
    h = C.c_void_p()
    it, dg, key, nk = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    n = C.c_int64()
    p = L.SlioLmapParams()
    assert lib.slio_lmap_params_default(None) == EINVAL
    assert lib.slio_lmap_params_default(C.byref(p)) == 0
    assert (round(p.leaf_corner, 6), round(p.leaf_surf, 6), round(p.leaf_outlier, 6)) == (0.2, 0.4, 0.4)
    assert (p.pose_leaf, p.search_radius, p.max_iterations) == (1.0, 50.0, 10)
    assert (round(p.mapping_interval, 6), round(p.scan_period, 6), round(p.keyframe_distance, 6)) == (0.3, 0.1, 0.3)
    assert lib.slio_lmap_create(None, C.byref(p)) == EINVAL
    assert lib.slio_lmap_create(C.byref(h), None) == EINVAL
    p.leaf_surf = 0.0
    assert lib.slio_lmap_create(C.byref(h), C.byref(p)) == EINVAL and not h.value   # before any device call
    assert lib.slio_lmap_destroy(None) == 0
    assert lib.slio_lmap_get_handle(None, 0, C.byref(h)) == EINVAL
    assert lib.slio_lmap_feed_lego(None, None, L.i64ptr(i64)) == EINVAL
    assert lib.slio_lmap_feed_host(None, None, 0, None, 0, None, 0, L.i64ptr(i64)) == EINVAL
    assert lib.slio_lmap_extract(None, None, 0, L.i64ptr(i64)) == EINVAL
    for kind in (0, 1, 2, -1):
        assert lib.slio_lmap_coeffs(None, kind, L.fptr(z6), C.byref(n)) == EINVAL
        assert lib.slio_lmap_get_coeffs(None, kind, None, None) == EINVAL
    assert lib.slio_lmap_normal_equations(None, L.fptr(np.zeros(36, F)), L.fptr(z6), C.byref(n)) == EINVAL
    assert lib.slio_lmap_optimize(None, L.fptr(z6), C.byref(it), C.byref(dg)) == EINVAL
    assert lib.slio_lmap_save_keyframe(None, L.fptr(z6), C.byref(key)) == EINVAL
    assert lib.slio_lmap_get_key_poses(None, None, 0, C.byref(nk)) == EINVAL
    assert lib.slio_lmap_clear(None) == EINVAL
    assert lib.slio_lego_odom_last_view(None, C.byref(L.SlioLegoLastView())) == EINVAL
    assert lib.slio_lmap_associate_to_map(None, L.fptr(z6), L.fptr(z6), L.fptr(z6)) == EINVAL
    fr = C.c_int32(0)
    t, r = np.zeros(4), np.zeros(4, F)
    args = (L.fptr(z6), L.fptr(z6), 0.0, F(0.1), L.dptr(t), L.fptr(r), L.fptr(r), 4)
    assert lib.slio_lmap_transform_update(*args, 4, C.byref(fr), L.fptr(z6), L.fptr(z6)) == EINVAL   # last >= len
    assert lib.slio_lmap_transform_update(*args, 2, None, L.fptr(z6), L.fptr(z6)) == EINVAL
    assert lib.slio_lmap_transform_update(*args, -1, None, L.fptr(z6), L.fptr(z6)) == 0             # no IMU: fine
    assert b"slio_lmap" in lib.slio_last_error()
