"""GPU tests of A-LOAM's scanRegistration on the device (slio_aloam_*,
include/slio_frontend.h) against the numpy restatement tests/aloam_model.py, to
the bit: the five clouds, the scan index arrays, curvature, labels, picked and
counts.  The inputs and the model's answers come from tests/aloam_case.py,
which asserts them fit for purpose; the clouds built here place the first
survivor, the last survivor and the switch point on the seams of the per-point
passes, and a sector on either side of the LDS sort's capacity
(slio_aloam_tile).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aloam_case as K  # noqa: E402
import aloam_model as M  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ECAPACITY, ESTATE = -1, -4, -5
NAN = np.full((1, 3), np.nan, F)
_models = {}


def model_of(key, build, n_scans=16):
    if key not in _models:
        cloud = build()
        _models[key] = (cloud, M.register(cloud, n_scans=n_scans))
    return _models[key]


def same_bits(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    np.testing.assert_array_equal(got.view(np.uint8), want.view(np.uint8), err_msg=what)


def check(reg, cloud, want, what):
    """One registration against the model's answer."""
    got = reg.laserCloudHandler(cloud)
    assert list(reg.counts) == list(want["counts"]), what
    for name in M.CLOUDS:
        same_bits(got[name], want[name], f"{what}: {name}")
    s, e = reg.scan_index()
    same_bits(s, want["scan_start"], f"{what}: scan_start")
    same_bits(e, want["scan_end"], f"{what}: scan_end")
    curv, label, picked = reg.work()
    same_bits(curv, want["curvature"], f"{what}: curvature")
    same_bits(label, want["label"], f"{what}: label")
    same_bits(picked, want["picked"], f"{what}: picked")


@pytest.fixture(scope="module")
def regs(L):
    """One handle per layout, alive together."""
    from agi_lidar_slam_amd.aloam import AloamScanRegistration
    r = {n: AloamScanRegistration(n_scans=n, max_points=40000) for n in (16, 32, 64)}
    yield r
    for v in r.values():
        v.close()


@pytest.fixture(scope="module")
def tile(L):
    from agi_lidar_slam_amd.aloam import tile
    return tile()


def test_getters_before_a_run(L):
    from agi_lidar_slam_amd.aloam import AloamScanRegistration
    r = AloamScanRegistration(max_points=64)
    out, i32, v = np.zeros((4, 4), F), np.zeros(64, np.int32), L.SlioAloamView()
    assert r.lib.slio_aloam_get_cloud(r.h, 0, L.fptr(out), 4) == ESTATE
    assert r.lib.slio_aloam_get_scan_index(r.h, L.iptr(i32), L.iptr(i32)) == ESTATE
    assert r.lib.slio_aloam_get_work(r.h, None, None, None) == ESTATE
    assert r.lib.slio_aloam_get_view(r.h, C.byref(v)) == ESTATE
    assert r.lib.slio_aloam_get_cloud(r.h, 5, L.fptr(out), 4) == EINVAL
    r.close()


def test_no_such_device(L):
    lib = L.load()
    p, h = L.SlioAloamParams(), C.c_void_p()
    lib.slio_aloam_params_default(C.byref(p))
    p.device = 4096
    assert lib.slio_aloam_create(C.byref(h), C.byref(p)) == EINVAL and not h.value
    assert b"no such device" in lib.slio_last_error()


@pytest.mark.parametrize("name", K.CPU_CASES)
def test_case(regs, name):
    check(regs[K.layout(name)], K.cut(name), K.model(name), name)


# ------------------------------------------------------------------ seams of the per-point passes
def test_first_survivor_on_a_block_seam(regs, tile):
    blk = tile[0]
    for lead in (blk - 1, blk, blk + 1):
        cloud, want = model_of(("first", lead), lambda: np.concatenate([np.repeat(NAN, lead, 0), K.dense()[:3000]]))
        assert want["stats"]["drop_nonfinite"] == lead
        check(regs[16], cloud, want, f"first survivor at {lead}")


def test_last_survivor_on_a_block_seam_then_a_block_of_dropped_points(regs, tile):
    blk = tile[0]
    for last in (8 * blk - 1, 8 * blk, 8 * blk + 1):
        cloud, want = model_of(("last", last),
                               lambda: np.concatenate([K.dense()[:last + 1], np.repeat(NAN, blk + 44, 0)]))
        assert want["counts"][0] == last + 1
        check(regs[16], cloud, want, f"last survivor at {last}")


def test_switch_point_on_a_block_seam(regs, tile):
    blk = tile[0]
    sw = K.model("dense")["info"]["switch_kept"]          # (nothing of the dense sweep is dropped: the input index)
    assert K.model("dense")["stats"]["drop_scan"] == 0 and sw > blk
    for target in (blk - 1, 0, 1):
        lead = (target - sw) % blk
        cloud, want = model_of(("switch", target), lambda: np.concatenate([np.repeat(NAN, lead, 0), K.dense()]))
        assert (want["info"]["switch_kept"] + lead) % blk == target
        check(regs[16], cloud, want, f"switch point at {target} of its block")


def test_a_block_of_dropped_points_inside_the_cloud(regs, tile):
    blk = tile[0]
    cloud, want = model_of("hole", lambda: np.concatenate([K.dense()[:1000], np.repeat(NAN, 2 * blk + 30, 0),
                                                           K.dense()[1000:]]))
    assert not np.isfinite(cloud[blk * 4:blk * 5]).any()  # block 4 holds dropped points only
    check(regs[16], cloud, want, "hole")


# ------------------------------------------------------------------ seams of the bucketing
def test_a_scan_fed_by_every_block_and_a_scan_fed_by_none(regs, tile):
    blk = tile[0]
    d = K.dense()
    sid, _ = M.scan_ids(16, M.elevation_deg(d))
    nblk = (len(d) + blk - 1) // blk
    for s in (0, 7):
        assert all((sid[b * blk:(b + 1) * blk] == s).any() for b in range(nblk)), s
    cloud, want = model_of("no5", lambda: d[sid != 5])
    assert want["scan_end"][5] - want["scan_start"][5] == -11 and want["stats"]["scans_skipped"] == 1
    check(regs[16], cloud, want, "no scan 5")


# ------------------------------------------------------------------ the sort paths
@pytest.mark.parametrize("over", [0, 1])
def test_sector_at_the_lds_sort_capacity(regs, tile, over):
    """One scan holds the whole cloud: six sectors of exactly the capacity of
    the LDS sort (one piece), then of one more (two pieces merged in global
    memory; the scan's VoxelGrid list takes several pieces either way)."""
    cap = tile[1]
    n = 6 * (cap + over) + 11
    cloud, want = model_of(("cap", over), lambda: K.one_scan(n))
    assert want["info"]["max_sector"] == cap + over and want["counts"][0] == n
    assert want["scan_end"][8] - want["scan_start"][8] == 6 * (cap + over)
    assert want["counts"][4] > 100 and want["stats"]["flat"] > 0 and want["stats"]["break21"] > 0
    check(regs[16], cloud, want, f"sectors of {cap + over}")


# ------------------------------------------------------------------ capacity, reuse, the view
def test_capacity(L):
    from agi_lidar_slam_amd.aloam import AloamScanRegistration
    r = AloamScanRegistration(max_points=4096)
    cloud, want = model_of("n4096", lambda: K.dense()[:4096])
    check(r, cloud, want, "n = max_points")
    c5 = np.zeros(5, np.int32)
    more = np.ascontiguousarray(K.dense()[:4097])
    assert r.lib.slio_aloam_run(r.h, L.fptr(more), 4097, L.iptr(c5)) == ECAPACITY
    assert r.lib.slio_aloam_run(r.h, L.fptr(more), -1, L.iptr(c5)) == EINVAL
    assert r.lib.slio_aloam_run(r.h, None, 3, L.iptr(c5)) == EINVAL
    r.close()


def test_large_then_small_then_empty_on_one_handle(regs):
    r = regs[16]
    check(r, K.cut("dense"), K.model("dense"), "dense")
    check(r, K.cut("small_scans"), K.model("small_scans"), "small after large")
    check(r, K.cut("empty"), K.model("empty"), "empty after small")
    assert all(len(c) == 0 for c in r.laserCloudHandler(K.cut("empty")).values())
    check(r, K.cut("one_scan"), K.model("one_scan"), "one scan after empty")


def test_view_points_at_the_clouds(regs):
    r = regs[16]
    got = r.laserCloudHandler(K.cut("dense"))
    v = r.view()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert list(v.count) == list(r.counts) and v.device == 0
    for k, name in enumerate(M.CLOUDS):
        host = np.zeros((v.count[k], 4), F)
        assert hip.hipMemcpy(host.ctypes.data, v.cloud[k], host.nbytes, 2) == 0      # device -> host
        same_bits(host, got[name], name)
