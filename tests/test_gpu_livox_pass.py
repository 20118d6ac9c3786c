"""GPU tests of livox_mapping's scan-to-map side on the device (slio_lvx_feed_host,
_build_maps, _pass, _normal_equations, _optimize, _process; LivoxMapping)
against the numpy restatement tests/livox_map_model.py, to the bit.  The
model's neighbours come from the oracle's kd-tree, its VoxelGrids from
oracle.voxel_grid; tests/livox_map_case.py asserts the fixture tie-free for
every query.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lego_map_model as LM  # noqa: E402
import livox_map_case as K  # noqa: E402
import livox_map_model as M  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ESTATE = -1, -5
ZERO = np.zeros(6, F)
EMPTY = np.zeros((0, 3), F)


def same_bits(got, want, what=""):
    g, w = np.ascontiguousarray(got, F), np.ascontiguousarray(want, F)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    nan = np.isnan(w)
    np.testing.assert_array_equal(np.isnan(g), nan, err_msg=what)
    np.testing.assert_array_equal(g.view(np.uint32)[~nan], w.view(np.uint32)[~nan], err_msg=what)


@pytest.fixture(scope="module")
def mapper(L, oracle_mod):
    """A mapper whose scan grid keeps the points apart, holding the cut's maps."""
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    m = LivoxMapping(leaf_corner=0.2, leaf_surf=K.LEAF_SURF, max_points=1 << 15)
    c, mp = K.cut(), K.maps()
    m.update_map(ZERO, c["corner_map"], c["surf_map"], [])
    counts = m.build_maps(mp["valid"])
    assert list(counts) == [len(mp["maps"][0]), len(mp["maps"][1])]
    for kind in range(2):       # laserCloud*FromMap: the model's concatenation, ids = positions
        same_bits(m.laserCloudFromMap(kind, mp["valid"]), mp["maps"][kind], f"FromMap {kind}")
    yield m
    m.close()


def check_pass(got, ref, kind, what):
    """World points, flags, and for every query the gate lets through the
    neighbours (ordered distances, indices in order: the fixture is tie-free)
    and the coefficient; -1 / +inf / 0 for the others."""
    Kn = M.KNN[kind]
    same_bits(got["world"], ref["world"], f"{what}: world")
    np.testing.assert_array_equal(got["sel"], ref["sel"], err_msg=f"{what}: sel")
    near = ref["near"]
    np.testing.assert_array_equal(got["nbr_idx"][near], ref["idx"][near][:, :Kn], err_msg=f"{what}: neighbours")
    same_bits(got["nbr_sqd"][near], ref["sqd"][near][:, :Kn], f"{what}: distances")
    assert (got["nbr_idx"][~near] == -1).all() and np.isinf(got["nbr_sqd"][~near]).all(), what
    same_bits(got["coeff"], ref["coeff"], f"{what}: coeff")


@pytest.mark.parametrize("kind", [0, 1])
def test_fused_pass_bit_exact(mapper, kind):
    big = K.reference(kind, 1500)["stats"]
    # every branch occurs (checked on the model, before the device runs): the
    # gate, the eigenvalue ratio (corner) / the plane check (surf), selected;
    # s <= 0.1 needs a residual of 1 m (corner) or of sqrt(|p|) ~ 6 m (surf),
    # which the 8-NN gate of 2.2 m excludes at |p| = 35 m: corner only
    assert big["gated"] >= 1 and big["rejected"] >= 1 and big["selected"] >= 1, big
    if kind == 0:
        assert big["weak"] >= 1, big
    c = K.cut()
    for n in K.SIZES:
        ref = K.reference(kind, n)
        counts = mapper.feed_host(c["corner_scan"][:n] if kind == 0 else EMPTY,
                                  c["surf_scan"][:n] if kind == 1 else EMPTY)
        assert counts[kind] == len(ref["scan"]) == n and counts[1 - kind] == 0
        same_bits(mapper.scan(kind), ref["scan"], f"kind {kind} n {n}: the fed scan")
        nsel = mapper.pass_(kind, c["tf"])
        assert nsel == int(ref["sel"].sum())
        check_pass(mapper.get_pass(kind), ref, kind, f"kind {kind} n {n}")


@pytest.mark.parametrize("nc,ns", [(255, 255), (256, 257), (1500, 1500), (0, 257), (257, 0)])
def test_normal_equations_bit_exact(mapper, nc, ns):
    """The 28 fp64 sums: a butterfly per wavefront, the four wavefronts in
    order, workgroups in order, corners before surfs (lego_map_model.tree_sum)."""
    c = K.cut()
    rc, rs = K.reference(0, nc), K.reference(1, ns)
    mapper.feed_host(c["corner_scan"][:nc], c["surf_scan"][:ns])
    mapper.pass_(0, c["tf"])
    mapper.pass_(1, c["tf"])
    AtA, AtB, nsel = mapper.normal_equations()
    wA, wB, wn = LM.normal_equations(c["tf"], [(rc["scan"], rc["coeff"], rc["sel"]),
                                               (rs["scan"], rs["coeff"], rs["sel"])])
    assert nsel == wn
    same_bits(AtA, wA, "AtA")
    same_bits(AtB, wB, "AtB")


# ------------------------------------------------------------------ exactness edges of the K-NN
def model_knn(oracle_mod, kind, mp, world):
    """K + 1 columns where the map has them (the tree up to 8, a float32 scan
    of the map beyond), else what there is with +inf."""
    Kn = M.KNN[kind]
    if len(mp) < Kn:
        return np.zeros((len(world), 0), np.int32), np.zeros((len(world), 0), F)
    d = world[:, None, :] - mp[None, :, :]
    d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
    k1 = min(Kn + 1, len(mp))
    order = np.argsort(d2, axis=1, kind="stable")[:, :k1]
    sqd = np.take_along_axis(d2, order, 1)
    ti, ts = oracle_mod.Tree(mp).knn(world, Kn)
    assert np.array_equal(ts, sqd[:, :Kn])          # the scan and the tree agree
    return np.concatenate([ti, order[:, Kn:].astype(np.int32)], 1), sqd


def run_edge(L, oracle_mod, kind, mp_pts, queries, what):
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    m = LivoxMapping(leaf_corner=0.2, leaf_surf=K.LEAF_SURF, max_points=1 << 14)
    try:
        model = M.CubeMap(oracle_mod.voxel_grid)
        cm, sm = (mp_pts, EMPTY) if kind == 0 else (EMPTY, mp_pts)
        m.update_map(ZERO, cm, sm, [])
        model.update(ZERO, cm, sm, [])
        valid = [int(v) for v in np.nonzero(model.sizes(kind))[0]]
        mp = model.concat(kind, valid)
        assert list(m.build_maps(valid))[kind] == len(mp_pts)
        q = np.ascontiguousarray(queries, F)
        if kind == 1:
            q = np.ascontiguousarray(oracle_mod.voxel_grid(q, K.LEAF_SURF), F)
        m.feed_host(q if kind == 0 else EMPTY, q if kind == 1 else EMPTY)
        world = M.to_map(ZERO, q)
        idx, sqd = model_knn(oracle_mod, kind, mp, world)
        assert M.tie_free(kind, sqd) and M.gate_clear(kind, sqd), what
        coeff, sel, near, stats = M.coeffs(kind, world, mp, idx, sqd)
        nsel = m.pass_(kind, ZERO)
        got = m.get_pass(kind)
        ref = dict(world=world, idx=idx, sqd=sqd, coeff=coeff, sel=sel, near=near)
        if idx.shape[1] < M.KNN[kind]:
            assert nsel == 0 and not got["sel"].any() and (got["nbr_idx"] == -1).all(), what
        else:
            check_pass(got, ref, kind, what)
            assert nsel == int(sel.sum())
        return stats, near
    finally:
        m.close()


def cloud(rng, n, lo, hi, wall=True):
    """Map points inside the box [lo, hi]^3, half of them on two walls and a
    floor (so that planes and lines exist), jittered."""
    p = rng.uniform(lo, hi, (n, 3))
    if wall:                                  # half of them; the rest fill the box
        p[:n // 2:3, 0] = lo + 0.5
        p[1:n // 2:3, 1] = lo + 0.7
        p[2:n // 2:3, 2] = lo + 0.2
    return (p + rng.normal(0, 0.004, p.shape)).astype(F)


@pytest.mark.parametrize("kind", [0, 1])
def test_knn_tiny_maps(L, oracle_mod, kind):
    """A map of K - 1 points: nothing selected, no fault; of exactly K points."""
    rng = np.random.default_rng(3 + kind)
    Kn = M.KNN[kind]
    pts = cloud(rng, Kn, 1.0, 1.6, wall=False)
    pts[:, 2] = 1.2 + 0.01 * rng.normal(size=Kn)                     # nearly a plane
    q = cloud(rng, 70, 1.0, 1.6, wall=False)                          # all within both gates of all K
    stats, near = run_edge(L, oracle_mod, kind, pts[:Kn - 1], q, "K - 1 map points")
    assert stats["gated"] == 70
    stats, near = run_edge(L, oracle_mod, kind, pts, q, "K map points")
    assert near.all()                                                # every query takes all K points


@pytest.mark.parametrize("kind", [0, 1])
def test_knn_across_cell_faces_and_outside_the_grid(L, oracle_mod, kind):
    """A dense map over 4 x 4 x 4 cells (the origin anchors the grid: cell faces
    at multiples of h) with queries next to x, y and z faces and to block
    corners, and queries 0.5, 1.5 and 3 cells outside the map's box."""
    rng = np.random.default_rng(11 + kind)
    h = 1.25 if kind == 0 else 2.25
    pts = np.concatenate([np.zeros((1, 3), F), cloud(rng, 2500 if kind == 0 else 4000, 0.05, 4 * h)])
    q = []
    for a in range(3):                       # beside a face of each axis, both sides
        for s in (-0.01, 0.01):
            p = rng.uniform(h, 3 * h, (12, 3))
            p[:, a] = 2 * h + s
            q.append(p)
    for s in (-0.01, 0.01):                  # beside a cell corner
        q.append(np.full((1, 3), 2 * h + s) + rng.normal(0, 0.002, (6, 3)))
    for cells in (0.5, 1.5, 3.0):            # outside the box, along each axis and both ways
        for a in range(3):
            for side in (0, 1):
                p = rng.uniform(h, 3 * h, (3, 3))
                p[:, a] = 4 * h + cells * h if side else -cells * h
                q.append(p)
    q = np.concatenate(q).astype(F)
    stats, near = run_edge(L, oracle_mod, kind, pts, q, "faces, corners, outside")
    inside = 72 + 12
    assert near[:inside].all()                          # the gate passes everywhere inside the dense map
    assert not near[inside + 18:].any()                 # 1.5 and 3 cells away: beyond both gates
    assert stats["selected"] >= 1 and stats["gated"] >= 36


def test_eighth_neighbour_around_the_gate(L, oracle_mod):
    """The 8th neighbour at squared distance just below 5.0 (selected or not as
    the model says, neighbours equal), just above it inside the block (the gate
    drops it), and at 2.3 m along +x from a query that sits just below a cell
    face, so that the neighbour lies two cells away, outside the block."""
    h = 2.25
    rng = np.random.default_rng(21)
    pts, q = [np.zeros((1, 3), F)], []
    for r, (d, qx) in enumerate(((np.sqrt(4.99), 3 * h + 1.0), (np.sqrt(5.01), 3 * h + 1.0), (2.3, 5 * h - 0.01))):
        base = np.array([qx, 7.0 + 12.0 * r, 7.0])
        seven = base + rng.normal(0, 0.05, (7, 3))
        seven[:, 2] = base[2] + 0.001 * rng.normal(size=7)           # a plane z = 7 with the eighth
        pts += [seven, (base + [d, 0.0, 0.0])[None, :]]
        q.append(base[None, :] + [0.0, 0.0, 0.01])
    stats, near = run_edge(L, oracle_mod, 1, np.concatenate(pts).astype(F), np.concatenate(q).astype(F), "gate")
    assert list(near) == [True, False, False]


# ------------------------------------------------------------------ errors
def test_state_and_argument_errors(L, mapper):
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    lib = L.load()
    fresh = LivoxMapping(max_points=1 << 10)
    try:
        n64, tf = C.c_int64(), np.zeros(6, F)
        i32 = C.c_int32()
        assert lib.slio_lvx_build_maps(fresh.h, None, 0, None) == ESTATE
        assert lib.slio_lvx_pass(fresh.h, 0, L.fptr(tf), C.byref(n64)) == ESTATE
        assert lib.slio_lvx_get_pass(fresh.h, 0, None, None, None, None, None) == ESTATE
        assert lib.slio_lvx_normal_equations(fresh.h, L.fptr(np.zeros(36, F)), L.fptr(np.zeros(6, F)), None) == ESTATE
        assert lib.slio_lvx_optimize(fresh.h, L.fptr(tf), C.byref(i32), None) == ESTATE
        assert lib.slio_lvx_get_scan(fresh.h, 0, None, 0, C.byref(n64)) == ESTATE
        for kind in (-1, 2):
            assert lib.slio_lvx_pass(fresh.h, kind, L.fptr(tf), None) == EINVAL
            assert lib.slio_lvx_get_pass(fresh.h, kind, None, None, None, None, None) == EINVAL
            assert lib.slio_lvx_get_scan(fresh.h, kind, None, 0, None) == EINVAL
        nan = np.array([0, 0, 0, np.nan, 0, 0], F)
        assert lib.slio_lvx_pass(fresh.h, 0, L.fptr(nan), None) == EINVAL
        assert lib.slio_lvx_pass(fresh.h, 0, None, None) == EINVAL
        assert lib.slio_lvx_optimize(fresh.h, L.fptr(nan), None, None) == EINVAL
        assert lib.slio_lvx_set_transform(fresh.h, L.fptr(nan)) == EINVAL
        assert lib.slio_lvx_normal_equations(fresh.h, None, None, None) == EINVAL
        bad = np.array([M.NUM], np.int32)
        assert lib.slio_lvx_build_maps(fresh.h, L.iptr(bad), 1, None) == EINVAL
        assert lib.slio_lvx_feed_host(fresh.h, None, 1, None, 0, None) == EINVAL
        assert lib.slio_lvx_feed_host(fresh.h, L.fptr(tf), -1, None, 0, None) == EINVAL
        big = np.zeros((1025, 3), F)
        assert lib.slio_lvx_feed_host(fresh.h, L.fptr(big), 1025, None, 0, None) == -4
        assert lib.slio_lvx_process(fresh.h, None, 1, None, 0, None, None) == EINVAL
    finally:
        fresh.close()
    for fn in (lib.slio_lvx_build_maps, ):
        assert fn(None, None, 0, None) == EINVAL
    assert lib.slio_lvx_pass(None, 0, None, None) == EINVAL
    assert lib.slio_lvx_process(None, None, 0, None, 0, None, None) == EINVAL
    assert lib.slio_lvx_get_transforms(None, None, None, None) == EINVAL


# ------------------------------------------------------------------ whole calls
def drive():
    """Six pairs of feature clouds of a sensor that moves 0.25 m per scan along
    x through x = 375 m (centerCubeI reaches 18: one shift) at z = -20 m, seeing
    the cut's walls 12 m ahead along its y axis; the sixth pair is 20 + 20
    points, too few for 50 rows.  Returns (start pose, [(corner, surf)])."""
    c = K.cut()
    ctr = c["surf_map"].mean(axis=0)
    start = np.array([0.0, 0.0, 0.0, 374.3, 3.0, -20.0], F)
    shift = (start[3:] + np.array([0.0, 12.0, 0.0], F) - ctr).astype(F)
    world_c, world_s = c["corner_map"] + shift, c["surf_map"] + shift
    rng = np.random.default_rng(2026)
    scans = []
    for k in range(6):
        tf = start + np.array([0.002 * k, -0.001 * k, 0.003 * k, 0.25 * k, 0.01 * k, -0.02 * k], F)
        R = np.linalg.inv(np.stack([M.to_map(np.concatenate([tf[:3], [0, 0, 0]]).astype(F), e[None, :])[0]
                                    for e in np.eye(3, dtype=F)], 1).astype(np.float64))
        nc, ns = (150, 700) if k < 5 else (20, 20)
        pc = world_c[rng.choice(len(world_c), nc, replace=False)] + rng.normal(0, 0.005, (nc, 3))
        ps = world_s[rng.choice(len(world_s), ns, replace=False)] + rng.normal(0, 0.005, (ns, 3))
        scans.append((((pc - tf[3:]) @ R.T).astype(F), ((ps - tf[3:]) @ R.T).astype(F)))
    return start, scans


def oracle_knn(oracle_mod):
    def f(kind, mp, world):
        Kn = M.KNN[kind]
        if len(mp) < Kn or len(world) == 0:
            return np.zeros((len(world), 0), np.int32), np.zeros((len(world), 0), F)
        return oracle_mod.Tree(mp).knn(world, Kn)
    return f


def test_process_six_scans_and_the_lockstep_entries(L, oracle_mod):
    from agi_lidar_slam_amd.livox_map import LivoxMapping
    from test_gpu_livox_map import check_maps
    start, scans = drive()
    model = M.Mapper(oracle_mod.voxel_grid, oracle_knn(oracle_mod))
    model.tobe[:] = start
    dev, lock = LivoxMapping(max_points=1 << 15), LivoxMapping(max_points=1 << 15)
    try:
        dev.transformTobeMapped = start
        tobe, aft, last = start.copy(), np.zeros(6, F), np.zeros(6, F)     # the lockstep caller's own state
        iters_seen, shifted = [], 0
        for k, (corner, surf) in enumerate(scans):
            cen0 = list(model.cen)
            it_m = model.process(corner, surf)
            shifted += model.cen != cen0
            got_aft = dev.process(corner, surf)
            assert dev.iterations == it_m, f"call {k}: iterations"
            same_bits(dev.transformTobeMapped, model.tobe, f"call {k}: transformTobeMapped")
            same_bits(got_aft, model.aft, f"call {k}: transformAftMapped")
            same_bits(dev.transformLastMapped, model.last, f"call {k}: transformLastMapped")
            assert list(dev.laserCloudCen) == model.cen
            check_maps(dev, model, f"call {k}")
            iters_seen.append(it_m)
            # the same call, stage by stage
            lock.select_cubes(tobe)
            lock.build_maps()
            lock.feed_host(corner, surf)
            tobe, it_l, _ = lock.optimize(tobe)
            if it_l:
                last, aft = aft, tobe.copy()
            lock.update_map(tobe, lock.scan(0), lock.scan(1))
            assert it_l == it_m
            same_bits(tobe, model.tobe, f"call {k}: lockstep transformTobeMapped")
            check_maps(lock, model, f"call {k}: lockstep")
        assert iters_seen[0] == 0                       # no map yet: only the append
        assert all(0 < i < 20 for i in iters_seen[1:5]), iters_seen     # converged
        assert iters_seen[5] == 20                      # fewer than 50 rows: twenty `continue`s
        assert shifted == 1
        same_bits(aft, model.aft, "lockstep transformAftMapped")
        # the drive stayed on the truth: 0.25 m per scan along x
        assert abs(float(model.tobe[3]) - (374.3 + 0.25 * 4)) < 0.05
    finally:
        dev.close()
        lock.close()
