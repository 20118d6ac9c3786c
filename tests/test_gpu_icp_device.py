"""GPU tests of the device-resident ICP loop (slio_icp_align, include/slio.h):
bit equality with the lockstep loop over slio_icp_correspond / slio_icp_step on
a second handle -- final state, fitness, working cloud, correspondences and far
counts -- for every batch boundary, source size and end state, and the float64
restatement's iteration count and end state (tests/icp_model.py)."""
import ctypes as C
import math
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import icp_model as M  # noqa: E402

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -5


@pytest.fixture(scope="module")
def L():
    from agi_lidar_slam_amd import build, _lib
    build.build()
    return _lib


@pytest.fixture(scope="module")
def fix():
    """icp_model's fixture with its two runs, computed once; the no-tie
    condition is asserted here."""
    tgt, src = M.fixture()
    runs = {md: M.icp_run(src, tgt, md) for md in (30, 0.5)}
    for md, r in runs.items():
        assert not r["ties"], f"exact nearest tie in a pass at max_dist {md}"
    assert (runs[30]["iterations"], runs[30]["state"]) == (12, M.TRANSFORM)
    assert (runs[0.5]["iterations"], runs[0.5]["state"]) == (15, M.TRANSFORM)
    return tgt, src, runs


def mk(L, max_points=4000, cell=1.0):
    lib = L.load()
    p = L.SlioParams()
    L.check(lib.slio_params_default(C.byref(p)), "params")
    p.device, p.max_points, p.grid_cell = 0, max_points, cell
    h = C.c_void_p()
    L.check(lib.slio_create(C.byref(h), C.byref(p)), "create")
    return h


def upload(L, fn, h, pts):
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    x, y, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    L.check(fn(h, L.fptr(x), L.fptr(y), L.fptr(z), pts.shape[0]), fn.__name__)


def left_behind(L, h):
    """What the last pass left on the handle, as bytes: working cloud,
    correspondence ids and squared distances, far queries."""
    lib = L.load()
    n = C.c_int64()
    assert lib.slio_icp_get_working(h, None, None, None, 0, C.byref(n)) in (0, ECAPACITY)
    cap = max(n.value, 1)
    x, y, z = (np.zeros(cap, np.float32) for _ in range(3))
    L.check(lib.slio_icp_get_working(h, L.fptr(x), L.fptr(y), L.fptr(z), cap, C.byref(n)), "get_working")
    idx, sqd = np.zeros(cap, np.int32), np.zeros(cap, np.float32)
    L.check(lib.slio_icp_get_correspondences(h, L.iptr(idx), L.fptr(sqd)), "get_correspondences")
    far = C.c_int64()
    L.check(lib.slio_icp_far_queries(h, C.byref(far)), "far_queries")
    k = n.value
    return (k, x[:k].tobytes(), y[:k].tobytes(), z[:k].tobytes(), idx[:k].tobytes(), sqd[:k].tobytes(), far.value)


class Owner:
    icp_far_first = None
    icp_state = None


def result_bits(res, own):
    conv, T, fitness, iters, state = res
    st = own.icp_state
    return (conv, T.tobytes(), struct.pack("<d", fitness), iters, state, struct.pack("<d", st.prev_mse),
            int(st.similar), int(st.converged), own.icp_far_first)


def both(L, hd, hl, max_dist, guess=None, batch=0, max_iterations=None):
    """The device loop on hd and the lockstep loop on hl; asserts they agree
    to the bit in everything they return and leave behind.  Returns the
    device's (result, owner)."""
    from agi_lidar_slam_amd import lio_sam
    lib = L.load()
    od, ol = Owner(), Owner()
    rd = lio_sam.icp_align_device(lib, hd, max_dist, guess, batch, max_iterations, owner=od)
    rl = lio_sam.icp_align_lockstep(lib, hl, max_dist, guess, max_iterations, owner=ol)
    assert result_bits(rd, od) == result_bits(rl, ol)
    assert left_behind(L, hd) == left_behind(L, hl)
    return rd, od


@pytest.fixture(scope="module")
def pair(L, fix):
    """Two handles holding the fixture's target; each test uploads its scan."""
    tgt, _, _ = fix
    lib = L.load()
    hd, hl = mk(L), mk(L)
    for h in (hd, hl):
        upload(L, lib.slio_map_upload, h, tgt)
    yield hd, hl
    lib.slio_destroy(hd)
    lib.slio_destroy(hl)


def set_scan(L, pair, pts):
    for h in pair:
        upload(L, L.load().slio_scan_upload, h, pts)


@pytest.mark.parametrize("max_dist", [30, 0.5])
def test_equals_lockstep_and_model(L, fix, pair, max_dist):
    _, src, runs = fix
    set_scan(L, pair, src)
    (conv, _, fitness, iters, state), own = both(L, *pair, max_dist)
    r = runs[max_dist]
    print(f"max_dist {max_dist}: {iters} iterations, state {state}, fitness {fitness:.6g}, "
          f"far_first {own.icp_far_first}")
    assert (conv, iters, state) == (True, r["iterations"], r["state"])


def test_batch_boundaries(L, fix, pair):
    """12 iterations: `done` lands mid-batch (100, 13), on the last launch of
    a batch (1, 4, 12) and -- with 13 -- one launch before the batch's end."""
    _, src, _ = fix
    set_scan(L, pair, src)
    seen = set()
    for batch in (1, 4, 12, 13, 100, 0, 5):
        rd, od = both(L, *pair, 30, batch=batch)
        assert rd[3] == 12
        seen.add(result_bits(rd, od) + left_behind(L, pair[0]))
    assert len(seen) == 1


def test_max_iterations(L, fix, pair):
    _, src, _ = fix
    set_scan(L, pair, src)
    for batch in (0, 2, 3):
        (conv, _, _, iters, state), _ = both(L, *pair, 30, batch=batch, max_iterations=3)
        assert (conv, iters, state) == (True, 3, M.ITERATIONS)
    (conv, _, _, iters, state), _ = both(L, *pair, 30, max_iterations=0)
    assert (conv, iters, state) == (True, 1, M.ITERATIONS)


@pytest.mark.parametrize("n", [0, 1, 2])
def test_too_few_points(L, fix, pair, n):
    _, src, _ = fix
    set_scan(L, pair, src[:n])
    (conv, T, fitness, iters, state), own = both(L, *pair, 30)
    assert (conv, iters, state) == (False, 0, M.NO_CORRESPONDENCES)
    np.testing.assert_array_equal(T, np.eye(4, dtype=np.float32))
    if n == 0:
        assert fitness == M.DBL_MAX and own.icp_far_first == 0


@pytest.mark.parametrize("n", [255, 256, 257])
def test_workgroup_edges(L, fix, pair, n):
    """One workgroup, exactly one, and two; the source tiled from the fixture."""
    _, src, _ = fix
    set_scan(L, pair, src[np.arange(n) % (src.shape[0] - 150)])
    (conv, _, _, iters, _), _ = both(L, *pair, 30)
    assert conv and iters > 1


def test_repeat_calls_rearm(L, fix, pair):
    """Two calls in a row on the same handles with different guesses, then the
    first again: the counters and the done flag start afresh."""
    _, src, _ = fix
    set_scan(L, pair, src)
    g = np.eye(4, dtype=np.float32)
    g[:3, :3] = M.rot_zyx(0.0, 0.0, 0.02).astype(np.float32)
    g[:3, 3] = [0.2, -0.1, 0.0]
    ra, oa = both(L, *pair, 30)
    rb, ob = both(L, *pair, 30, guess=g, batch=3)
    rc, oc = both(L, *pair, 30)
    assert result_bits(ra, oa) == result_bits(rc, oc)
    assert result_bits(ra, oa) != result_bits(rb, ob)


def test_far_start(L, fix, pair):
    _, src, _ = fix
    far_src = (src + np.float32([15, 0, 0])).astype(np.float32)
    set_scan(L, pair, far_src)
    _, own = both(L, *pair, 30)
    print("far queries of the first pass", own.icp_far_first, "of", far_src.shape[0])
    assert own.icp_far_first > far_src.shape[0] // 2


def test_argument_and_state_errors(L, fix):
    lib = L.load()
    prm, st = L.SlioIcpParams(), L.SlioIcpState()
    lib.slio_icp_params_default(C.byref(prm))
    assert lib.slio_icp_align(None, C.byref(prm), None, 30.0, 0, C.byref(st), None, None) == EINVAL
    h = mk(L)
    try:
        assert lib.slio_icp_align(h, None, None, 30.0, 0, C.byref(st), None, None) == EINVAL
        assert lib.slio_icp_align(h, C.byref(prm), None, 30.0, 0, None, None, None) == EINVAL
        assert lib.slio_icp_align(h, C.byref(prm), None, -1.0, 0, C.byref(st), None, None) == EINVAL
        assert lib.slio_icp_align(h, C.byref(prm), None, math.nan, 0, C.byref(st), None, None) == EINVAL
        assert lib.slio_icp_align(h, C.byref(prm), None, 30.0, 0, C.byref(st), None, None) == ESTATE  # no map
    finally:
        lib.slio_destroy(h)


def test_lockstep_pass_unchanged(L, fix, pair):
    """slio_icp_correspond, whose kernel now shares its body with the device
    loop's pass, against the brute-force restatement: working cloud, indices
    and distances to the bit, the sums within the bound any order satisfies."""
    tgt, src, _ = fix
    lib = L.load()
    hd, _ = pair
    upload(L, lib.slio_scan_upload, hd, src)
    for max_dist in (30, 0.5):
        T = np.eye(4, dtype=np.float32)
        want = M.transform32(T, src)
        idx_ref, sqd_ref, tie = M.nearest32(want, tgt)
        assert not tie.any()
        terms, ok = M.sum_terms(want, tgt, idx_ref, sqd_ref, max_dist)
        sums, n = np.zeros(16), C.c_int64(-1)
        L.check(lib.slio_icp_correspond(hd, L.fptr(np.ascontiguousarray(T.reshape(16))), 1, float(max_dist),
                                        L.dptr(sums), C.byref(n)), "icp_correspond")
        k, x, y, z, idx, sqd, _ = left_behind(L, hd)
        assert k == src.shape[0]
        assert (x, y, z) == tuple(np.ascontiguousarray(want[:, a]).tobytes() for a in range(3))
        assert sqd == sqd_ref.tobytes()
        np.testing.assert_array_equal(np.frombuffer(idx, np.int32), np.where(ok, idx_ref, -1))
        assert n.value == int(ok.sum())
        assert (np.abs(sums - M.fsums(terms)) <= M.sum_bounds(terms)).all()
