"""GPU: k_time_keys, the time sort and k_undistort on the crafted cases of
tests/undistort_case.py, through slio_undistort with the crafted IMUpose
table: a non-identity R_LI, every branch of so3_exp, points on and one ulp
either side of an offset, tables of 0, 1 and 2 poses, tables whose second
offset is negative, the first point's repeated compensation, both zeros as
times, non-finite rows.  Per case:

  order      the returned times are bit-equal to the oracle's stable order;
  reference  |got - ref| <= 0.5 ulp32(ref) + 64 * 2^-53 * (||P|| + ||T_LI|| +
             ||T_ei|| + 1) against the longdouble reference (the final
             rounding to float; an fp64 chain of about 40 operations);
  oracle     every coordinate within 1 float ulp of the oracle's (both are
             fp64 chains a few 1e-13 from the exact value before one rounding,
             so they part only where it sits on a rounding boundary), and at
             most 1 % of the points not bit-equal;
  untouched  points without a segment (npose < 2, t / 1000 <= every head's
             offset) come back bit-equal to the sorted input;
  presorted  the same points in time order (the sort is skipped) give the
             same bits.

One small handle serves the module."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_case as UC  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def kf(L):
    from agi_lidar_slam_amd.esekf import Esekf
    k = Esekf(max_points=1024)
    yield k
    k.close()


def _args(L, case, pts, t):
    from agi_lidar_slam_amd.esekf import StateIkfom
    tab = case["tab"]
    poses = (L.SlioImuPose * max(tab.shape[0], 1))()
    for k, r in enumerate(tab):
        poses[k].offset_time = r[0]
        poses[k].acc[:] = list(r[1:4])
        poses[k].gyr[:] = list(r[4:7])
        poses[k].vel[:] = list(r[7:10])
        poses[k].pos[:] = list(r[10:13])
        poses[k].rot[:] = list(r[13:22])
    xs = StateIkfom.from_array(case["state"]).to_c()
    n = t.shape[0]
    # (n = 0: one unused element, so that the pointers are valid)
    cols = [np.ascontiguousarray(pts[:, k] if n else np.zeros(1), np.float32) for k in range(3)]
    tm = np.ascontiguousarray(t if n else np.zeros(1), np.float32)
    return poses, tab.shape[0], xs, cols, tm, n


def undistort(L, kf, case, pts, t):
    poses, npose, xs, (x, y, z), tm, n = _args(L, case, pts, t)
    ox, oy, oz, ot = (np.zeros(max(n, 1), np.float32) for _ in range(4))
    L.check(L.load().slio_undistort(kf.h, L.fptr(x), L.fptr(y), L.fptr(z), L.fptr(tm), n, poses, npose,
                                    C.byref(xs), L.fptr(ox), L.fptr(oy), L.fptr(oz), L.fptr(ot)), "slio_undistort")
    return np.stack([ox[:n], oy[:n], oz[:n]], 1), ot[:n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", UC.NAMES)
def test_undistort_case(L, oracle_mod, kf, name):
    c, m, (ref, scale, checked) = UC.solved(name)
    want, want_t = oracle_mod.undistort_points(c["tab"], c["state"], c["pts"], c["t"])
    got, got_t = undistort(L, kf, c, c["pts"], c["t"])
    n = c["t"].shape[0]
    assert got.shape == (n, 3) and got_t.shape == (n,)
    # order: the stable time order, the times' own bits (-0.0 stays -0.0)
    np.testing.assert_array_equal(_bits(got_t), _bits(want_t))
    src = c["pts"][m["order"]]
    finite = np.isfinite(src).all(axis=1)
    ratio = UC.worst_ratio(got, ref, scale, checked)
    chain = UC.worst_chain_ratio(got, ref, scale, checked)
    dk = np.abs(UC.float_key(got[finite]) - UC.float_key(want[finite]))
    differ = float((dk > 0).any(axis=1).mean()) if finite.any() else 0.0
    print(f"{name}: n {n}, worst |err| / bound {ratio:.4f}, (|err| - half an ulp) / chain term {chain:.4f}, "
          f"worst distance to the oracle {int(dk.max()) if dk.size else 0} ulp, points not bit-equal {differ:.4f}")
    # against the longdouble reference
    assert ratio <= 1.0
    # against the oracle: 1 ulp, 1 % of the points; non-finite rows in place, NaN == NaN
    assert dk.size == 0 or dk.max() <= 1
    assert differ <= 0.01
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(got[~finite], want[~finite])
    # no so3_exp evaluated: the sorted input, bit for bit
    still = m["seg"] < 0
    np.testing.assert_array_equal(_bits(got[still]), _bits(src[still]))
    if c["tab"].shape[0] < 2:
        assert still.all()
    # presorted input: the same bits
    got2, got2_t = undistort(L, kf, c, *UC.presorted(c))
    np.testing.assert_array_equal(_bits(got2_t), _bits(got_t))
    np.testing.assert_array_equal(_bits(got2), _bits(got))


@pytest.mark.parametrize("name", UC.PIPELINE_NAMES)
def test_undistort_voxel_pipeline(L, oracle_mod, kf, name):
    """slio_scan_upload_undistort_voxel at leaf 0.5 leaves oracle.voxel_grid of
    the slio_undistort output in the handle's scan (n = 0 included)."""
    c, _, _ = UC.solved(name)
    und, _ = undistort(L, kf, c, c["pts"], c["t"])
    poses, npose, xs, (x, y, z), tm, n = _args(L, c, c["pts"], c["t"])
    nd = C.c_int64(-1)
    L.check(L.load().slio_scan_upload_undistort_voxel(kf.h, L.fptr(x), L.fptr(y), L.fptr(z), L.fptr(tm), n, poses,
                                                      npose, C.byref(xs), 0.5, C.byref(nd)), "undistort_voxel")
    kf._scan_ref = None
    kf._n_scan = int(nd.value)
    down = kf.feats_down_body()
    want = oracle_mod.voxel_grid(und, 0.5) if n else np.zeros((0, 3), np.float32)
    assert nd.value == want.shape[0] and (n == 0 or nd.value > 0)
    np.testing.assert_array_equal(down, want)
