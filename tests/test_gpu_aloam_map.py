"""GPU tests of A-LOAM's laserMapping on the device (slio_aloam_map_*,
include/slio_frontend.h) against the plain-Python restatement
tests/aloam_map_model.py, to the bit: both poses, q / t_wmap_wodom, every LM
iterate, cost and mu, all counters, the down-sampled clouds, the associations
and every touched cube.  The cases and the model's answers come from
tests/aloam_map_case.py, which asserts on the model that each case reaches what
it is there for.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import aloam_map_case as K  # noqa: E402
import aloam_map_model as M  # noqa: E402
import aloam_odom_case as OK  # noqa: E402
from test_aloam_map_cpu import bits, same_association, same_result, same_state  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ECAPACITY, ESTATE = -1, -4, -5
SMALL = dict(max_points=1 << 16, max_scan=8192)


@pytest.fixture(scope="module")
def A(L):
    from agi_lidar_slam_amd import aloam
    return aloam


def test_model_cases_are_fit():
    K.check_fixture()
    K.check_crafted()
    K.check_shifts()


# ------------------------------------------------------------------ crafted single associations
def test_crafted_associations(A):
    """Every crafted region in one map: the first sweep puts the map in, the
    second the queries; the association at the identity through the lockstep
    entries, then the evaluation and the sweep's result."""
    cmap, smap, qs = K.crafted()
    _, r1, slot = K.crafted_model()
    want = K.M_assoc()
    h = A.AloamMapping(K.FINE, K.FINE, **SMALL)
    try:
        h.process(K.xyzi(cmap), K.xyzi(smap), *K.IDENT)
        cq, sq = K.crafted_scan()
        same_result(h.process(K.xyzi(cq), K.xyzi(sq), *K.IDENT), r1, "crafted")
        h.associate(*K.IDENT)
        got = h.association()
        for name, s in slot.items():
            assert got[0][s] == want[0][s], (name, A.KINDS[got[0][s]], A.KINDS[want[0][s]])
            np.testing.assert_array_equal(got[2][s], want[2][s], err_msg=name)
        same_association(got, want, "crafted")
        xyz = np.concatenate([h.stack(0), h.stack(1)], 0)
        Aw, gw, cw, nw = M.evaluate(xyz, want[0], want[1], *K.IDENT)
        Ag, gg, cg, ng = h.evaluate(*K.IDENT)
        assert ng == nw and bits(Ag) == bits(Aw) and bits(gg) == bits(gw) and cg == cw
    finally:
        h.close()


# ------------------------------------------------------------------ the gate
@pytest.mark.parametrize("nc,ns,optimized", [(10, 50, 0), (11, 51, 1)])
def test_gate(A, nc, ns, optimized):
    c, s = (K.xyzi(x) for x in K.gate_clouds(nc, ns))
    h, m = A.AloamMapping(0.05, 0.05, **SMALL), M.Mapper(0.05, 0.05)
    try:
        for k, (q, t) in enumerate((K.IDENT, K.SIZE_POSE)):
            want = m.process(c, s, q, t)
            want["stack"], want["cubes"] = [x.copy() for x in m.stack], K.snapshot(m, want["touched"])
            got = h.process(c, s, q, t)
            same_result(got, want, f"gate {nc} / {ns}, sweep {k}")
            same_state(h, want, f"gate {nc} / {ns}, sweep {k}")
        assert got["map_size"] == [nc, ns] and got["optimized"] == optimized
        if not optimized:                                        # transformUpdate and the map update all the same
            assert bits(got["q_w_curr"]) == bits(K.SIZE_POSE[0]) and bits(got["t_w_curr"]) == bits(K.SIZE_POSE[1])
            assert int(h.cube_sizes(0).sum()) > nc
    finally:
        h.close()


# ------------------------------------------------------------------ scan sizes
@pytest.fixture(scope="module")
def sized(A):
    h = A.AloamMapping(0.02, 0.02, **SMALL)
    yield h
    h.close()


@pytest.mark.parametrize("nc,ns", K.SIZES)
def test_scan_sizes(sized, nc, ns):
    want = K.size_model(nc, ns)
    sized.reset()
    sized.process(*(K.xyzi(c) for c in K.size_map()), *K.IDENT)
    same_result(sized.process(*(K.xyzi(c) for c in K.size_scan(nc, ns)), *K.SIZE_POSE), want, f"{nc} / {ns}")
    same_state(sized, want, f"{nc} / {ns}")


# ------------------------------------------------------------------ the fixture
def test_fixture(A):
    want = K.model_run()
    h = A.AloamMapping(**SMALL)
    try:
        for k in range(K.N_SWEEPS):
            same_result(h.process(*K.last_clouds(k), *K.odom_pose(k)), want[k], f"sweep {k}")
            same_state(h, want[k], f"sweep {k}")
            sizes = [h.cube_sizes(kind) for kind in range(2)]
            for kind in range(2):
                np.testing.assert_array_equal(np.flatnonzero(sizes[kind]),
                                              sorted(i for (kd, i), c in want[k]["cubes"].items()
                                                     if kd == kind and len(c)))
                sur = np.concatenate([M.EMPTY] + [want[k]["cubes"].get((kind, i), M.EMPTY) for i in want[k]["valid"]])
                np.testing.assert_array_equal(h.surround(kind), sur)
                np.testing.assert_array_equal(h.map(kind), sur)   # (every point lies in the valid cubes here)
        full = K.xyzi(OK.raw_sweep(5, 300)[:500])
        full[:, 3] = np.arange(len(full), dtype=F)
        reg = h.register_cloud(full)
        np.testing.assert_array_equal(reg[:, :3], M.to_map(want[5]["q_w_curr"], want[5]["t_w_curr"], full[:, :3]))
        np.testing.assert_array_equal(reg[:, 3], full[:, 3])
        h.reset()                                                # and again from the start after reset
        same_result(h.process(*K.last_clouds(0), *K.odom_pose(0)), want[0], "after reset")
    finally:
        h.close()


# ------------------------------------------------------------------ the shift sequence
def test_shift_sequence(A):
    want = K.shift_model()
    h = A.AloamMapping(**SMALL)
    c, s = (K.xyzi(x) for x in K.shift_clouds())
    try:
        for k, t in enumerate(K.SHIFT_STEPS):
            same_result(h.process(c, s, K.IDENT[0], [float(v) for v in t]), want[k], f"step {k}")
            for kind in range(2):
                np.testing.assert_array_equal(h.cube_sizes(kind), want[k]["sizes"][kind], err_msg=f"step {k}")
            for (kind, ind), cloud in want[k]["cubes"].items():
                np.testing.assert_array_equal(h.cube(kind, ind), cloud, err_msg=f"step {k}, cube {kind} {ind}")
    finally:
        h.close()


# ------------------------------------------------------------------ the device-resident solve
def test_device_solve_matches_the_lockstep_loop(A, L):
    """Sweep 1's two passes: the device-resident loop against associate +
    evaluate on the device with the controller on the host, and the model."""
    want = K.model_run()[1]
    h = A.AloamMapping(**SMALL)
    lib = L.load()
    try:
        h.process(*K.last_clouds(0), *K.odom_pose(0))
        got = h.process(*K.last_clouds(1), *K.odom_pose(1))
        same_result(got, want, "sweep 1")
        q, t = M.associate_to_map(K.model_run()[0]["q_wmap_wodom"], K.model_run()[0]["t_wmap_wodom"], *K.odom_pose(1))
        for k in range(2):
            pw = want["passes"][k]
            h.associate(q, t)
            Ag, gg, cg, ng = h.evaluate(q, t)
            assert ng[:3] == [pw["corner"], pw["plane"], pw["degenerate"]] and cg == pw["cost_first"]
            lm = L.SlioAloamOdomLm()
            lm.q[:], lm.t[:] = q, t
            assert lib.slio_aloam_odom_lm_step(C.byref(lm), 0, None, None, 0.0) == 0
            lm.A[:], lm.g[:], lm.cost = list(Ag), list(gg), cg
            it = 0
            while True:
                assert lib.slio_aloam_odom_lm_step(C.byref(lm), 1, None, None, 0.0) == 0
                if lm.done:
                    break
                An, gn, cn, _ = h.evaluate(list(lm.qn), list(lm.tn))
                assert lib.slio_aloam_odom_lm_step(C.byref(lm), 2, L.dptr(An), L.dptr(gn), cn) == 0
                w = pw["iterates"][it]
                assert bits(lm.q) == bits(w["q"]) and bits(lm.t) == bits(w["t"]), (k, it)
                assert lm.cost == w["cost"] and lm.mu == w["mu"], (k, it)
                it += 1
            assert (it, lm.accepted, lm.stop) == (pw["iterations"], pw["accepted"], pw["stop"])
            q, t = list(lm.q), list(lm.t)
        assert bits(q) == bits(want["q_w_curr"]) and bits(t) == bits(want["t_w_curr"])
        same_association(h.association(), K_last_assoc(), "the second pass's association")
    finally:
        h.close()


def K_last_assoc():
    """The model's association of sweep 1's second pass."""
    m = M.Mapper()
    for k in range(2):
        m.process(*K.last_clouds(k), *K.odom_pose(k))
    return m.assoc


# ------------------------------------------------------------------ the chain
def test_chain_from_the_raw_sweep(A):
    """laserMapping(raw sweep) equals feeding the odometry's clouds and pose
    from the host; a registration without a mapper still gives the same clouds."""
    chain, plain = A.AloamScanRegistration(max_points=16384), A.AloamScanRegistration(max_points=16384)
    chain.enable_mapping(skip_frame_num=1, max_map_points=1 << 16)
    host = A.AloamMapping(**SMALL)
    try:
        for k in range(3):
            raw = OK.raw_sweep(k, 300)
            got = chain.laserMapping(raw)
            assert got["odometry"]["published"] == 1
            c, s = chain.odometry.last_clouds()
            want = host.process(c, s, got["odometry"]["q_w_curr"], got["odometry"]["t_w_curr"])
            assert got["mapping"] == want, k
            assert got["mapping"]["optimized"] == (k > 0)
            for kind in range(2):
                np.testing.assert_array_equal(chain.mapping.stack(kind), host.stack(kind))
                np.testing.assert_array_equal(chain.mapping.map(kind), host.map(kind))
            clouds = plain.laserCloudHandler(raw)
            for n, name in enumerate(A.CLOUDS):
                np.testing.assert_array_equal(chain._get(n).view(np.uint32), clouds[name].view(np.uint32))
            v = chain.view()
            reg = chain.mapping.register_device_cloud(v.cloud[0], int(v.count[0]))
            np.testing.assert_array_equal(reg, host.register_cloud(clouds["laserCloud"]))
        gated = A.AloamScanRegistration(max_points=16384)
        gated.enable_mapping(skip_frame_num=2, max_map_points=1 << 16)
        seen = [gated.laserMapping(OK.raw_sweep(k, 300))["mapping"] is not None for k in range(3)]
        assert seen == [True, False, True]                        # the odometry's published gate
        for x in (gated.mapping, gated.odometry, gated):
            x.close()
    finally:
        for x in (chain.mapping, chain.odometry, chain, plain, host):
            x.close()


# ------------------------------------------------------------------ states, errors, capacities
def test_states_errors_and_capacities(A, L):
    lib = L.load()
    h, other = A.AloamMapping(max_points=3, max_scan=2), A.AloamMapping(**SMALL)
    try:
        n64, n1, i4 = C.c_int64(), np.zeros(1, np.int32), np.zeros(M.NUM, np.int32)
        q, t, out = np.array([0, 0, 0, 1.0]), np.zeros(3), np.zeros(28)
        one = np.array([[1.0, 0.0, 0.0, 0.0]], F)
        f1 = (L.fptr(one), 1)
        r = L.SlioAloamMapResult()

        def all_estate():
            assert lib.slio_aloam_map_get_cube(h.h, 0, 0, None, 0, C.byref(n64)) == ESTATE
            assert lib.slio_aloam_map_cube_sizes(h.h, 0, L.iptr(i4)) == ESTATE
            assert lib.slio_aloam_map_get_surround(h.h, 0, None, 0, C.byref(n64)) == ESTATE
            assert lib.slio_aloam_map_get_map(h.h, 0, None, 0, C.byref(n64)) == ESTATE
            assert lib.slio_aloam_map_get_stack(h.h, 0, None, 0, C.byref(n64)) == ESTATE
            assert lib.slio_aloam_map_register_cloud(h.h, one.ctypes.data_as(C.c_void_p), 1, 0, L.fptr(one)) == ESTATE
            assert lib.slio_aloam_map_associate(h.h, L.dptr(q), L.dptr(t)) == ESTATE
            assert lib.slio_aloam_map_get_association(h.h, None, None, None, None, 0, L.iptr(n1)) == ESTATE
            assert lib.slio_aloam_map_evaluate(h.h, L.dptr(q), L.dptr(t), L.dptr(out), L.dptr(out), L.dptr(out),
                                               L.iptr(i4)) == ESTATE

        all_estate()
        run = lambda c, s, q_, t_, res=r: lib.slio_aloam_map_run(h.h, L.fptr(c), len(c), L.fptr(s), len(s),
                                                                 L.dptr(q_), L.dptr(t_), C.byref(res))
        three = np.repeat(one, 3, 0)
        assert run(one, one, np.array([0, 0, 0, np.nan]), t) == EINVAL
        assert run(one, one, np.zeros(4), t) == EINVAL
        assert run(one, one, q, np.array([np.inf, 0, 0])) == EINVAL
        assert lib.slio_aloam_map_run(h.h, None, 1, *f1, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
        assert lib.slio_aloam_map_run(h.h, L.fptr(one), -1, *f1, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
        assert lib.slio_aloam_map_run(h.h, *f1, *f1, L.dptr(q), L.dptr(t), None) == EINVAL
        assert lib.slio_aloam_map_run_view(h.h, None, L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
        assert run(three, one, q, t) == ECAPACITY                 # beyond max_scan
        all_estate()                                             # a refused call leaves the handle as it was
        spread = np.array([[0.0, 0, 0, 0], [5.0, 0, 0, 0]], F)
        assert run(spread, spread, q, t) == 0 and run(one, one, q, t) == 0   # exactly the capacity
        assert [len(h.cube(0, 2425)), len(h.cube(1, 2425))] == [3, 3]
        assert lib.slio_aloam_map_associate(h.h, L.dptr(q), L.dptr(t)) == ESTATE   # the gate stayed shut: no grid
        assert run(one, one, q, t) == ECAPACITY                   # and one more
        assert [len(h.cube(0, 2425)), len(h.cube(1, 2425))] == [3, 3]
        np.testing.assert_array_equal(h.stack(0), one[:, :3])
        assert lib.slio_aloam_map_get_cube(h.h, 0, 2425, L.fptr(np.zeros((3, 3), F)), 2, C.byref(n64)) == ECAPACITY
        assert lib.slio_aloam_map_get_cube(h.h, 2, 0, None, 0, C.byref(n64)) == EINVAL
        assert lib.slio_aloam_map_get_cube(h.h, 0, M.NUM, None, 0, C.byref(n64)) == EINVAL
        assert lib.slio_aloam_map_get_stack(h.h, 0, None, -1, C.byref(n64)) == EINVAL
        v = L.SlioAloamOdomView()
        v.device = 1
        assert lib.slio_aloam_map_run_view(h.h, C.byref(v), L.dptr(q), L.dptr(t), C.byref(r)) == EINVAL
        # two handles side by side: the other one runs the fixture's first sweeps undisturbed
        want = K.model_run()
        for k in range(2):
            same_result(other.process(*K.last_clouds(k), *K.odom_pose(k)), want[k], f"other, sweep {k}")
            assert run(one, one, q, t) == ECAPACITY
        assert lib.slio_aloam_map_evaluate(other.h, L.dptr(q), L.dptr(t), L.dptr(out), L.dptr(out), L.dptr(out),
                                           L.iptr(i4)) == ESTATE   # no association since the sweep
        other.associate(want[1]["q_w_curr"], want[1]["t_w_curr"])
        assert lib.slio_aloam_map_get_association(other.h, None, None, None, None, 1, L.iptr(n1)) == ECAPACITY
        assert lib.slio_aloam_map_associate(other.h, None, L.dptr(t)) == EINVAL
    finally:
        h.close()
        other.close()
