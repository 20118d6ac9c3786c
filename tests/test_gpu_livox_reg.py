"""GPU tests of livox_mapping's scanRegistration on the device (slio_lreg_*,
include/slio_frontend.h; slio_lvx_feed_device / slio_lvx_process_cloud,
include/slio.h) against the numpy restatement tests/livox_reg_model.py, to the
bit: flags, loop 1's visited mask, counts and the three clouds.  The inputs and
the model's answers come from tests/livox_reg_case.py, which asserts them fit
for purpose.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import livox_map_model as MM  # noqa: E402
import livox_reg_case as K  # noqa: E402
import livox_reg_model as M  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ESTATE = -1, -5


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def check(reg, cloud, want, what):
    """One registration against the model's answer."""
    full, corner, surf = reg.laserCloudHandler(cloud)
    assert list(reg.counts) == list(want["counts"]), what
    flags, visited = reg.flags()
    np.testing.assert_array_equal(visited, want["visited"], err_msg=f"{what}: visited")
    np.testing.assert_array_equal(flags, want["flags"], err_msg=f"{what}: flags")
    for got, name in ((full, "cloud"), (corner, "corner"), (surf, "surf")):
        assert got.shape == want[name].shape, (what, name)
        np.testing.assert_array_equal(bits(got), bits(want[name]), err_msg=f"{what}: {name}")


@pytest.fixture(scope="module")
def reg(L):
    from agi_lidar_slam_amd.livox_reg import LivoxScanRegistration
    r = LivoxScanRegistration()
    yield r
    r.close()


@pytest.fixture(scope="module")
def tile(L):
    from agi_lidar_slam_amd.livox_reg import chain_tile
    per_thread, per_wg = chain_tile()
    assert per_wg >= M.MAX_POINTS      # no seam between workgroups: one sees the whole chain
    return per_thread


def test_fixtures_are_fit():
    K.check_dense_is_fit()
    K.check_no_scan_id_boundary(K.dense())


def test_full_dense_frame(reg):
    check(reg, K.cut("dense"), K.model("dense"), "dense")


@pytest.mark.parametrize("n", K.SMALL_SIZES + K.EDGE_SIZES)
def test_dense_frame_cut(reg, n):
    check(reg, K.cut("dense", n), K.model("dense", n), f"dense[:{n}]")


def test_cut_at_every_chain_seam(reg, tile):
    """N - 5, the loop's end, one and two positions either side of (and on)
    every seam between two threads' runs inside the dense frame."""
    seams = K.seam_sizes(tile, len(K.dense()))
    assert len(seams) >= 10
    for sizes in seams:
        for n in sizes:
            check(reg, K.cut("dense", n), K.model("dense", n), f"dense[:{n}]")


@pytest.mark.parametrize("n", K.TRUNC_SIZES)
def test_truncation_at_32000(reg, n):
    want = K.model("big", n)
    assert want["counts"][0] < 32000 <= n          # non-finite points before the cut, none counted after it
    check(reg, K.cut("big", n), want, f"big[:{n}]")


@pytest.mark.parametrize("name", ["axes", "duplicates", "only_nonfinite", "nan_start", "nan_end", "nan_runs",
                                  "nan_blocks", "all_stride1", "all_stride4"])
def test_special_clouds(reg, name):
    check(reg, K.cut(name), K.model(name), name)


def test_nonfinite_after_dropping_leaves_small_sizes(reg):
    """The small sizes again, reached by dropping non-finite points."""
    d = K.dense()
    for n in K.SMALL_SIZES:
        c = np.repeat(d[:n], 2, axis=0).copy()
        c[1::2, 2] = np.nan                        # every second point goes
        c = np.concatenate([np.full((3, 4), np.inf, F), c])
        want = M.register(c)
        assert want["counts"][0] == n
        check(reg, c, want, f"{n} finite of {len(c)}")


def test_chain_stress(reg, tile):
    """Lines (stride 4) with random kinks (stride 1 locally), 20 seeds: the
    chain enters the threads' runs at all four offsets."""
    seen = set()
    for s in K.STRESS_SEEDS:
        want = K.model(f"stress{s}")
        seen |= K.entry_offsets(want["visited"], tile)
        check(reg, K.cut(f"stress{s}"), want, f"stress {s}")
    assert seen == {0, 1, 2, 3}


@pytest.mark.parametrize("d", range(-4, 5))
def test_single_kink_across_a_seam(reg, tile, d):
    assert tile == 128                             # the case places the kink at 5 + 128 + d
    name = f"kink{d:+d}"
    check(reg, K.cut(name), K.model(name), name)


def test_reuse_large_then_small(reg):
    """No flag, visited bit or count of the large run survives in the small one."""
    check(reg, K.cut("big", 32000), K.model("big", 32000), "large")
    check(reg, K.cut("dense", 70), K.model("dense", 70), "small after large")
    check(reg, K.cut("dense", 0), K.model("dense", 0), "empty after small")
    check(reg, K.cut("dense"), K.model("dense"), "dense after empty")


# ------------------------------------------------------------------ the mapper's device feed
def test_feed_device_equals_feed_host(L, reg):
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    a, b = LivoxMapping(max_points=1 << 15), LivoxMapping(max_points=1 << 15)
    try:
        for name, n in (("dense", None), ("big", 32000), ("all_stride1", None), ("dense", 0)):
            _, corner, surf = reg.laserCloudHandler(K.cut(name, n))
            ca = a.feed_device(reg)
            cb = b.feed_host(corner[:, :3], surf[:, :3])
            assert list(ca) == list(cb), name
            assert ca[0] == len(corner) and ca[1] <= len(surf)
            for kind in (0, 1):
                np.testing.assert_array_equal(bits(a.scan(kind)), bits(b.scan(kind)), err_msg=f"{name}: scan {kind}")
    finally:
        a.close()
        b.close()


def oracle_knn(oracle_mod):
    def f(kind, mp, world):
        Kn = MM.KNN[kind]
        if len(mp) < Kn or len(world) == 0:
            return np.zeros((len(world), 0), np.int32), np.zeros((len(world), 0), F)
        return oracle_mod.Tree(mp).knn(world, Kn)
    return f


def test_process_cloud_six_frames(L, oracle_mod):
    """From the sensor's cloud to the pose, six frames of a short drive:
    process_cloud against the model registration followed by the model mapper,
    and against laserCloudHandler + process (the host feed), after every call."""
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    from agi_lidar_slam_amd.livox_reg import LivoxScanRegistration
    from test_gpu_livox_map import check_maps
    model = MM.Mapper(oracle_mod.voxel_grid, oracle_knn(oracle_mod))
    dev, host = LivoxMapping(max_points=1 << 16), LivoxMapping(max_points=1 << 16)
    r1, r2 = LivoxScanRegistration(), LivoxScanRegistration()
    try:
        iters = []
        for k in range(6):
            cloud = K.frame_at(k)
            want = M.register(cloud)
            it_m = model.process(want["corner"][:, :3], want["surf"][:, :3])
            aft = dev.process_cloud(r1, cloud)
            assert list(r1.counts) == list(want["counts"]), k
            assert dev.iterations == it_m, f"frame {k}: iterations"
            _, corner, surf = r2.laserCloudHandler(cloud)
            aft_h = host.process(corner[:, :3], surf[:, :3])
            assert host.iterations == it_m
            for m, a, what in ((dev, aft, "device feed"), (host, aft_h, "host feed")):
                np.testing.assert_array_equal(bits(m.transformTobeMapped), bits(model.tobe), err_msg=f"{k}: {what}")
                np.testing.assert_array_equal(bits(a), bits(model.aft), err_msg=f"{k}: {what}: Aft")
                np.testing.assert_array_equal(bits(m.transformLastMapped), bits(model.last), err_msg=f"{k}: {what}")
                check_maps(m, model, f"frame {k}: {what}")
            iters.append(it_m)
        assert iters[0] == 0 and any(i > 0 for i in iters[1:]), iters      # the optimisation did run
    finally:
        for h in (dev, host, r1, r2):
            h.close()


def test_errors(L, reg):
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    from agi_lidar_slam_amd.livox_reg import LivoxScanRegistration
    lib = L.load()
    m = LivoxMapping(max_points=1 << 12)
    fresh = LivoxScanRegistration()
    counts, c3 = np.zeros(2, np.int64), np.zeros(3, np.int32)
    xyzi, aft, it = np.zeros((4, 4), F), np.zeros(6, F), C.c_int32()
    try:
        # a feed before any run
        assert lib.slio_lvx_feed_device(m.h, fresh.h, L.i64ptr(counts)) == ESTATE
        assert lib.slio_lreg_get_cloud(fresh.h, L.fptr(xyzi), 4) == ESTATE
        assert lib.slio_lreg_get_flags(fresh.h, None, None) == ESTATE
        # argument errors on a live handle
        assert lib.slio_lreg_run(fresh.h, None, 4, L.iptr(c3)) == EINVAL
        assert lib.slio_lreg_run(fresh.h, L.fptr(xyzi), -1, L.iptr(c3)) == EINVAL
        assert lib.slio_lreg_run(fresh.h, L.fptr(xyzi), 4, None) == EINVAL
        assert lib.slio_lreg_get_features(reg.h, 2, L.fptr(xyzi), 4) == EINVAL
        assert lib.slio_lvx_feed_device(m.h, None, L.i64ptr(counts)) == EINVAL
        assert lib.slio_lvx_feed_device(None, fresh.h, L.i64ptr(counts)) == EINVAL
        assert lib.slio_lvx_process_cloud(m.h, fresh.h, None, 4, L.fptr(aft), C.byref(it), L.iptr(c3)) == EINVAL
        # a destroyed registration
        gone = C.c_void_p(fresh.h.value)
        fresh.close()
        assert lib.slio_lvx_feed_device(m.h, gone, L.i64ptr(counts)) == EINVAL
        assert lib.slio_lvx_process_cloud(m.h, gone, L.fptr(xyzi), 4, L.fptr(aft), C.byref(it), L.iptr(c3)) == EINVAL
        assert lib.slio_lreg_run(gone, L.fptr(xyzi), 4, L.iptr(c3)) == EINVAL
        assert b"destroyed" in lib.slio_last_error()
        assert lib.slio_lreg_destroy(gone) == EINVAL
    finally:
        m.close()
        fresh.close()


def test_handles_on_different_devices(L, reg):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device: nothing to mix")
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    lib = L.load()
    reg.run(K.cut("dense", 70))
    m = LivoxMapping(device=1, max_points=1 << 12)
    try:
        counts, c3 = np.zeros(2, np.int64), np.zeros(3, np.int32)
        xyzi, aft, it = np.zeros((4, 4), F), np.zeros(6, F), C.c_int32()
        assert lib.slio_lvx_feed_device(m.h, reg.h, L.i64ptr(counts)) == EINVAL
        assert b"different devices" in lib.slio_last_error()
        assert lib.slio_lvx_process_cloud(m.h, reg.h, L.fptr(xyzi), 4, L.fptr(aft), C.byref(it), L.iptr(c3)) == EINVAL
    finally:
        m.close()
