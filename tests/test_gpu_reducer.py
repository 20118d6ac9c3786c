"""GPU tests of the reducer workgroup of the fused single-rank pass.

A fused pass launch carries one workgroup more than the scan has chunks; that
workgroup (reducer_pass in slio_device.hip) stages the control block, forms
dx_new, collects the 64 segment rows as they become ready and runs the filter
step.  SLIO_NO_REDUCER=1, read when a handle is created, keeps the earlier
tail, where the last workgroup to arrive does all of that.  Both sum in the
same order and run the same step, so every comparison here is bitwise, between
two handles created under the two settings: x, P, the stats, the super rows of
every pass, plane / selection / residual and the last search's Nearest_Points
(ids and squared distances are derived one-to-one from the neighbour positions
the pass stores: map ids are unique).

A 200k-point synthetic map; scan sizes at the shapes of the row tree:
8,192 points = 64 chunks (one chunk per segment row, the smallest fusable
scan), 8,193 = 65 (one row with two chunks, a last chunk with one live point),
9,000 = 71 (uneven super rows, a partly filled last chunk), 12,837 = 101 (rows
of 1 and 2 chunks in all 8 supers), 8,191 = 64 again (a chunk is 128 points: the
last one has 127 live points) and 8,064 = 63 (below 64 chunks: two launches per
pass under either setting).
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import L, mk, results, state_of, upload_map, upload_scan  # noqa: E402,F401
from test_gpu_runtime import slio_state, state_array  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [8_192, 8_193, 9_000, 12_837, 8_191, 8_064]
N_SCAN = 13_000


@pytest.fixture(scope="module")
def pair(L):
    """(problem, handle with the reducer, handle created under SLIO_NO_REDUCER=1),
    each handle with its own upload of the map."""
    from agi_lidar_slam_amd import synth
    mp, fr = synth.make_problem(200_000, N_SCAN, pattern="avia")
    lib = L.load()
    old = os.environ.pop("SLIO_NO_REDUCER", None)
    hs = []
    try:
        hs.append(mk(L, n_max=N_SCAN))
        os.environ["SLIO_NO_REDUCER"] = "1"
        hs.append(mk(L, n_max=N_SCAN))
    finally:
        os.environ.pop("SLIO_NO_REDUCER", None)
        if old is not None:
            os.environ["SLIO_NO_REDUCER"] = old
    try:
        for h in hs:
            upload_map(L, h, mp)
        yield mp, fr, hs[0], hs[1]
    finally:
        for h in hs:
            lib.slio_destroy(h)


def _update(L, h, st, P0, maxit, mode, ext, n, expect=0):
    """One device-resident update and everything it leaves behind."""
    lib = L.load()
    xs = slio_state(st)
    P = P0.copy()
    stt = L.SlioIkfStats()
    rc = lib.slio_ikf_update_device(h, C.byref(xs), L.dptr(P), 0.001, maxit, ext, mode, L.ALLREDUCE_FN(), None,
                                    C.byref(stt))
    assert rc == expect, (rc, lib.slio_last_error().decode())
    if rc:
        return None
    sup = np.zeros(8 * 91)
    L.check(lib.slio_super_download(h, L.dptr(sup)), "super")
    idx, sqd, sel, pl, rs = results(L, h, n)
    return (state_array(xs), P, np.array([stt.passes, stt.searches, stt.valid_passes, stt.converged, stt.last_m]),
            sup, idx, sqd, sel, pl.view(np.uint32), rs.view(np.uint32))


def _same(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def _scan(L, hs, fr, npts):
    body = np.ascontiguousarray(fr.body[:npts])
    for h in hs:
        assert upload_scan(L, h, body) == 0
    return body


@pytest.mark.parametrize("ext", [0, 1])
@pytest.mark.parametrize("mode,maxit", [(1, 4), (0, 3)])
@pytest.mark.parametrize("npts", SIZES)
def test_reducer_bitwise(L, pair, npts, mode, maxit, ext):
    """Reducer against the last-arriver tail at every scan size, in the fixed
    flow (4 iterations) and the reference flow (3, with a reuse pass), D = 6
    and 12.  Updates of 1 .. maxit passes make each pass in turn the last one,
    whose super rows slio_super_download returns."""
    mp, fr, h_red, h_old = pair
    _scan(L, (h_red, h_old), fr, npts)
    st = state_of(fr)
    P0 = np.eye(24) * 1e-2
    for k in range(1, maxit + 1):
        red = _update(L, h_red, st, P0, k, mode, ext, npts)
        old = _update(L, h_old, st, P0, k, mode, ext, npts)
        _same(red, old)
        assert red[2][0] >= 1 and red[2][4] > 0, red[2]
        if mode == 1:
            assert red[2][0] == k and red[2][2] == k
    if mode == 0:
        print(f"{npts} points, reference flow: passes {red[2][0]} searches {red[2][1]}")


def test_reducer_path_is_taken(L, pair):
    """With the wait limit forced to 1 tick a reducer gives up at once, so
    SLIO_ETIMEOUT tells which launches carry one: the 64-chunk scan's on the
    reducer handle do; the 63-chunk scan's (two launches per pass) and the
    SLIO_NO_REDUCER handle's do not, and complete.  After the limit is back
    at its default the same handle gives the right bits again (its counters
    were reset)."""
    mp, fr, h_red, h_old = pair
    lib = L.load()
    st = state_of(fr)
    P0 = np.eye(24) * 1e-2
    try:
        _scan(L, (h_red, h_old), fr, 8_192)
        ref = _update(L, h_old, st, P0, 4, 1, 0, 8_192)
        for h in (h_red, h_old):
            L.check(lib.slio_debug_wait_limit(h, 1), "wait limit")
        assert _update(L, h_red, st, P0, 4, 1, 0, 8_192, expect=L.SLIO_ETIMEOUT) is None
        _same(_update(L, h_old, st, P0, 4, 1, 0, 8_192), ref)
        L.check(lib.slio_debug_wait_limit(h_red, 0), "wait limit")
        for _ in range(2):
            _same(_update(L, h_red, st, P0, 4, 1, 0, 8_192), ref)
        # below 64 chunks no launch has a reducer
        _scan(L, (h_red, h_old), fr, 8_064)
        L.check(lib.slio_debug_wait_limit(h_red, 1), "wait limit")
        _same(_update(L, h_red, st, P0, 4, 1, 0, 8_064), _update(L, h_old, st, P0, 4, 1, 0, 8_064))
    finally:
        for h in (h_red, h_old):
            lib.slio_debug_wait_limit(h, 0)


def test_reducer_timeout_reference_flow_recovers(L, pair):
    """The bounded wait in the reference flow and with D = 12: the update
    reports SLIO_ETIMEOUT, never a result, and the next update on the handle
    is bitwise right."""
    mp, fr, h_red, h_old = pair
    lib = L.load()
    st = state_of(fr)
    P0 = np.eye(24) * 1e-2
    _scan(L, (h_red, h_old), fr, 9_000)
    ref = _update(L, h_old, st, P0, 3, 0, 1, 9_000)
    try:
        L.check(lib.slio_debug_wait_limit(h_red, 1), "wait limit")
        assert _update(L, h_red, st, P0, 3, 0, 1, 9_000, expect=L.SLIO_ETIMEOUT) is None
    finally:
        lib.slio_debug_wait_limit(h_red, 0)
    _same(_update(L, h_red, st, P0, 3, 0, 1, 9_000), ref)


def test_reducer_back_to_back_updates(L, pair):
    """20 updates in a row on one handle, every one from another prior (pose,
    covariance, flow and D change): the rows' counter words are reset by the
    reducer as it takes each row, and no count or ready mark of an earlier
    update is ever seen."""
    mp, fr, h_red, h_old = pair
    _scan(L, (h_red, h_old), fr, 12_837)
    st0 = state_of(fr)
    rng = np.random.default_rng(20261021)
    for k in range(20):
        st = st0.copy()
        st[0:3] += rng.normal(0.0, 0.02, 3)
        P0 = np.eye(24) * (1e-2 * (1.0 + 0.25 * (k % 4)))
        mode, maxit, ext = (1, 4, 0) if k % 3 else (0, 3 + (k % 2), (k // 3) % 2)
        _same(_update(L, h_red, st, P0, maxit, mode, ext, 12_837),
              _update(L, h_old, st, P0, maxit, mode, ext, 12_837))


def test_reducer_early_end_then_normal_update(L, pair):
    """Reference flow from the true pose: the update converges and ends before
    maximum_iter, so its remaining launches find it ended and return in every
    workgroup, the reducer included; a normal update follows on the handle."""
    mp, fr, h_red, h_old = pair
    _scan(L, (h_red, h_old), fr, 9_000)
    P0 = np.eye(24) * 1e-2
    st_true = state_of(fr, pos=fr.gt_pos, rot=fr.gt_rot)
    red = _update(L, h_red, st_true, P0, 8, 0, 0, 9_000)
    old = _update(L, h_old, st_true, P0, 8, 0, 0, 9_000)
    _same(red, old)
    print(f"early end: passes {red[2][0]} of 8")
    assert red[2][0] < 8
    st = state_of(fr)
    _same(_update(L, h_red, st, P0, 4, 1, 0, 9_000), _update(L, h_old, st, P0, 4, 1, 0, 9_000))


def test_reducer_certified_passes(L, pair, monkeypatch):
    """kNN certificates (the passes after an update's first keep a query's 5
    nearest when the bound proves no other point can enter) at 8,192 + 640
    points: the reducer path certifies the same queries as the last-arriver
    tail and gives the bits of an update whose passes all search in full."""
    mp, fr, h_red, h_old = pair
    lib = L.load()
    npts = 8_192 + 640
    _scan(L, (h_red, h_old), fr, npts)
    st = state_of(fr)
    P0 = np.eye(24) * 1e-2

    def counts(h):
        out = (C.c_uint32 * 2)()
        L.check(lib.slio_debug_knn_cert(h, out), "cert")
        return np.array([int(out[0]), int(out[1])])

    try:
        monkeypatch.setenv("SLIO_NO_KNN_CERT", "1")
        lib.slio_debug_reload_switches(h_red)
        full = _update(L, h_red, st, P0, 4, 1, 0, npts)
    finally:
        monkeypatch.delenv("SLIO_NO_KNN_CERT")
        lib.slio_debug_reload_switches(h_red)
    per = []
    for h in (h_red, h_old, h_red):
        a = counts(h)
        _same(_update(L, h, st, P0, 4, 1, 0, npts), full)
        per.append(tuple(counts(h) - a))
    print(f"certified / searched per update: {per}")
    assert per[0] == per[1] == per[2]
    assert per[0][0] > 0 and per[0][1] >= npts
