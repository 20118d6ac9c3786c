"""The cases of the A-LOAM laserMapping tests (tests/test_aloam_map_cpu.py,
tests/test_gpu_aloam_map.py), generated here at import, the model's answers to
them computed once and shared, and the assertions made on the MODEL alone, so
that the restatement shows what a case is there for and not only the code under
test.

The fixture: six sweeps of the analytic room of tests/aloam_odom_case.py
(ground plane, walls, three pillars, 16 beams), horizon 300, a few thousand
points per sweep, through aloam_model.register; laserMapping takes each
sweep's cornerPointsLessSharp and surfPointsLessFlat (what the odometry hands
on as its last clouds).  The odometry input is the ground truth with a drift
that grows with the sweep.
"""
import functools
import math

import numpy as np

import aloam_map_model as M
import aloam_model as RM
import aloam_odom_case as OK

F = np.float32
N_SWEEPS = 6
IDENT = ([0.0, 0.0, 0.0, 1.0], [0.0, 0.0, 0.0])
FINE = 0.001          # a leaf too small for a 40 m cube: PCL's pass-through, the points keep their order


def xyzi(p):
    p = np.ascontiguousarray(p, F).reshape(-1, 3)
    return np.concatenate([p, np.zeros((len(p), 1), F)], 1)


# ---------------------------------------------------------------- the fixture
@functools.lru_cache(maxsize=None)
def last_clouds(k):
    """(laserCloudCornerLast, laserCloudSurfLast) of sweep k: (n, 4) float32."""
    w = RM.register(OK.raw_sweep(k, 300))
    return np.ascontiguousarray(w["cornerPointsLessSharp"]), np.ascontiguousarray(w["surfPointsLessFlat"])


def true_pose(k):
    a = 0.04 * k
    return [0.0, 0.0, math.sin(a / 2), math.cos(a / 2)], [0.25 * k, 0.06 * k, 0.0]


def odom_pose(k):
    """The truth with an injected drift: 4 mrad of yaw and (5, -3, 2) cm per sweep."""
    a = 0.04 * k + 0.004 * k
    return [0.0, 0.0, math.sin(a / 2), math.cos(a / 2)], [0.25 * k + 0.05 * k, 0.06 * k - 0.03 * k, 0.02 * k]


def pose_error(q, t, k):
    """(rotation error in rad, translation error in m) against sweep k's true pose."""
    qt, tt = true_pose(k)
    d = M.OM.qmul([-q[0], -q[1], -q[2], q[3]], qt)
    n = math.sqrt(sum(v * v for v in d))
    ang = 2 * math.atan2(math.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2) / n, abs(d[3]) / n)
    return ang, math.sqrt(sum((t[a] - tt[a]) ** 2 for a in range(3)))


def snapshot(m, touched):
    return {(kind, ind): m.cube(kind, ind).copy() for kind in range(2) for ind in touched}


@functools.lru_cache(maxsize=None)
def model_run():
    """The six sweeps through the model: per sweep the result, the stacks, and
    the contents of every touched cube."""
    m = M.Mapper()
    out = []
    for k in range(N_SWEEPS):
        r = m.process(*last_clouds(k), *odom_pose(k))
        r["stack"] = [s.copy() for s in m.stack]
        r["cubes"] = snapshot(m, r["touched"])
        out.append(r)
    return out


def check_fixture():
    """The issue's conditions on the fixture, asserted on the model; returns the figures."""
    run = model_run()
    fig = dict(clouds=[tuple(len(c) for c in last_clouds(k)) for k in range(N_SWEEPS)],
               stacks=[r["stack_size"] for r in run], maps=[r["map_size"] for r in run], errors=[])
    assert not run[0]["optimized"] and all(r["optimized"] for r in run[1:])
    for k in range(1, N_SWEEPS):
        eo, em = pose_error(*odom_pose(k), k), pose_error(run[k]["q_w_curr"], run[k]["t_w_curr"], k)
        fig["errors"].append((eo, em))
        assert em[1] < eo[1] and em[0] < eo[0], (k, eo, em)   # the mapped pose is closer to the truth
        for p in run[k]["passes"]:
            assert p["corner"] > 0 and p["plane"] > 0
    fig["iterations"] = [[p["iterations"] for p in r["passes"]] for r in run]
    fig["factors"] = [[(p["corner"], p["plane"], p["degenerate"], p["outliers"]) for p in r["passes"]] for r in run]
    assert all(len(r["touched"]) >= 1 for r in run)
    return fig


# ---------------------------------------------------------------- crafted single associations
def _below(x):
    return float(np.nextafter(F(x), F(-np.inf)))


def filler(n, z):
    """n points on a coarse lattice far from every crafted region (y < -8), spanning the 38 m that make FINE
    pass through."""
    i = np.arange(n)
    return np.stack([-19.0 + 38.0 * (i % 7) / 6.0, -19.0 + 1.5 * (i // 7), np.full(n, z)], 1).astype(F)


@functools.lru_cache(maxsize=None)
def plane_offsets():
    """Two offsets of the fifth neighbour from the plane of the other four, either side of the 0.2 threshold of
    the fitted plane (found on the model by bisection)."""
    def kind(h):
        nb = [[0.0, 0.0, 2.0], [0.4, 0.0, 2.0], [0.0, 0.4, 2.0], [0.4, 0.4, 2.0], [0.2, 0.2, float(F(2.0 + h))]]
        return M.fit_plane(nb)[0]
    lo, hi = 0.1, 0.6
    assert kind(lo) == M.PLANE and kind(hi) == M.REJECTED
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if kind(mid) == M.PLANE else (lo, mid)
    return lo * (1 - 1e-3), hi * (1 + 1e-3)


@functools.lru_cache(maxsize=None)
def crafted():
    """(corner map, surf map, queries): queries is name -> (class, point).  Every region is CRAFTED, 8 m from
    the next; check_crafted says on the model what each one reaches."""
    cm, sm, qs = [filler(14, -1.5)], [filler(56, -1.0)], {}

    def region(name, surf, centre, pts, query):
        c = np.array(centre, np.float64)
        (sm if surf else cm).append((c + np.array(pts, np.float64)).astype(F))
        qs[name] = (surf, (c + np.array(query, np.float64)).astype(F))

    line = [[0.1 * i, 0.0, 0.0] for i in range(5)]
    region("line", 0, (0, 0, 0), line, (0.2, 0.05, 0.0))
    region("isotropic", 0, (8, 0, 0), [[0.25, 0, 0], [-0.25, 0, 0], [0, 0.25, 0], [0, -0.25, 0], [0, 0, 0.25]],
           (0.01, 0.02, 0.03))
    region("coincident", 0, (16, 0, 0), [[0.1, 0.1, 0.1]] * 5, (0.0, 0.0, 0.0))
    near4 = [[0.1, 0, 0], [0.2, 0, 0], [0.3, 0, 0], [0.4, 0, 0]]
    region("gate_at", 0, (0, 8, 0), near4 + [[1.0, 0, 0]], (0.0, 0.0, 0.0))
    region("gate_below", 0, (0, -8, 0), near4 + [[_below(1.0), 0, 0]], (0.0, 0.0, 0.0))
    region("tie", 0, (16, 8, 0), near4 + [[-0.5, 0, 0], [0.5, 0, 0]], (0.0, 0.0, 0.0))
    region("few", 0, (0, 16, 0), near4[:3], (0.0, 0.0, 0.0))
    qs["padding"] = (0, np.array([20.5, 0.0, 0.0], F))            # beyond the map's box, inside the grid's padding
    qs["outside"] = (0, np.array([60.0, 40.0, 9.0], F))           # beyond the grid
    lo, hi = plane_offsets()
    sq = [[0.0, 0.0, 2.0], [0.4, 0.0, 2.0], [0.0, 0.4, 2.0], [0.4, 0.4, 2.0]]
    region("plane", 1, (0, 0, 0), sq + [[0.2, 0.2, 2.0]], (0.1, 0.1, 2.05))
    region("plane_in", 1, (8, 0, 0), sq + [[0.2, 0.2, 2.0 + lo]], (0.1, 0.1, 2.0))
    region("plane_out", 1, (16, 0, 0), sq + [[0.2, 0.2, 2.0 + hi]], (0.1, 0.1, 2.0))
    region("surf_collinear", 1, (0, 8, 0), [[0.1 * i, 1.0, 0.0] for i in range(5)], (0.2, 1.05, 0.0))
    region("surf_few", 1, (8, 8, 0), sq, (0.1, 0.1, 2.0))
    return np.concatenate(cm, 0), np.concatenate(sm, 0), qs


def crafted_scan():
    """The queries as the two incoming clouds."""
    _, _, qs = crafted()
    return (np.array([p for s, p in qs.values() if not s], F), np.array([p for s, p in qs.values() if s], F))


@functools.lru_cache(maxsize=None)
def crafted_model():
    """The map put in by a first sweep, the queries by a second, both at the identity and with the leaf FINE;
    returns (mapper, second result, name -> slot)."""
    cmap, smap, qs = crafted()
    m = M.Mapper(FINE, FINE)
    r0 = m.process(xyzi(cmap), xyzi(smap), *IDENT)
    assert not r0["optimized"]
    assert len(m.concat(0, r0["valid"])) == len(cmap) and len(m.concat(1, r0["valid"])) == len(smap)   # passed through
    cq, sq = crafted_scan()
    r1 = m.process(xyzi(cq), xyzi(sq), *IDENT)
    assert r1["optimized"] and r1["stack_size"] == [len(cq), len(sq)]
    slot = {}
    for name, (s, p) in qs.items():
        hit = np.flatnonzero((m.stack[s] == p[None, :]).all(1))
        assert len(hit) == 1, name
        slot[name] = int(hit[0]) + (len(cq) if s else 0)
    return m, r1, slot


def check_crafted():
    """Each crafted region reaches what it is there for, on the model."""
    cmap, smap, qs = crafted()
    m, r1, slot = crafted_model()
    # (the map the second sweep saw is the crafted map in its input order: the first sweep passed it through)
    kind, rec, idx, sqd = M_assoc()
    k = lambda name: int(kind[slot[name]])
    assert k("line") == M.EDGE and k("isotropic") == M.REJECTED and k("coincident") == M.DEGENERATE
    assert k("gate_at") == M.NONE and (idx[slot["gate_at"]] == -1).all()
    assert k("gate_below") != M.NONE and sqd[slot["gate_below"]][4] < F(1.0)
    assert sqd[slot["gate_below"]][4] == np.nextafter(F(1.0), F(0)) * np.nextafter(F(1.0), F(0))
    t = idx[slot["tie"]]
    assert sqd[slot["tie"]][4] == F(0.25) and cmap[t[4]][0] == F(15.5), (t, cmap[t[4]])   # the lower index of the two
    assert k("few") == M.NONE and k("padding") == M.NONE and k("outside") == M.NONE
    assert k("plane") == M.PLANE and k("plane_in") == M.PLANE and k("plane_out") == M.REJECTED
    assert k("surf_collinear") == M.DEGENERATE and k("surf_few") == M.NONE
    return {n: M_KINDS[k(n)] for n in qs}


M_KINDS = ("none", "edge", "plane", "degenerate", "rejected")


@functools.lru_cache(maxsize=None)
def M_assoc():
    m, _, _ = crafted_model()
    cmap, smap, _ = crafted()
    a = [M.associate(s, m.stack[s], (cmap, smap)[s], *IDENT) for s in range(2)]
    return tuple(np.concatenate([a[0][j], a[1][j]], 0) for j in range(4))


# ---------------------------------------------------------------- the gate
def gate_clouds(nc, ns):
    """A map of exactly nc corner and ns surf points (one pole, one patch of ground) and a scan on it."""
    pole = np.stack([np.full(nc, 2.0), np.full(nc, 1.0), -1.0 + 0.15 * np.arange(nc)], 1).astype(F)
    i = np.arange(ns)
    ground = np.stack([0.3 * (i % 8), 0.3 * (i // 8), np.full(ns, -1.7)], 1).astype(F)
    return pole, ground


# ---------------------------------------------------------------- scan sizes
@functools.lru_cache(maxsize=None)
def size_map():
    """Three poles and a patch of ground, 0.2 m apart: the map of the scan-size cases."""
    z = -1.0 + 0.2 * np.arange(16)
    poles = np.concatenate([np.stack([np.full(16, x), np.full(16, y), z], 1) for x, y in ((3, 2), (-4, 5), (6, -3))], 0)
    g = np.arange(-8, 8.01, 0.5)
    gx, gy = np.meshgrid(g, g)
    ground = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, -1.7)], 1)
    return poles.astype(F), ground.astype(F)


SIZES = ((0, 0), (1, 1), (63, 63), (64, 64), (65, 65), (255, 255), (256, 256), (257, 257), (0, 257), (0, 256))
SIZE_POSE = ([0.0, 0.0, math.sin(0.004), math.cos(0.004)], [0.04, -0.03, 0.02])


def size_scan(nc, ns):
    """nc points along the poles and ns on the ground, each alone in its voxel of the leaf 0.02."""
    rng = np.random.default_rng(7)
    i = np.arange(nc)
    base = np.array([(3, 2), (-4, 5), (6, -3)], np.float64)[i % 3]
    c = np.concatenate([base + rng.uniform(-0.02, 0.02, (nc, 2)), (-1.0 + 0.011 * i)[:, None] * np.ones((nc, 1))], 1)
    j = np.arange(ns)
    s = np.stack([-7.0 + 0.8 * (j % 18) + 0.1, -7.0 + 0.8 * (j // 18) + 0.1, -1.7 + rng.uniform(-0.02, 0.02, ns)], 1)
    return c.astype(F).reshape(-1, 3), s.astype(F).reshape(-1, 3)


@functools.lru_cache(maxsize=None)
def size_model(nc, ns):
    """The map by a first sweep at the identity (leaf 0.02), the scan by a second at SIZE_POSE."""
    m = M.Mapper(0.02, 0.02)
    m.process(*(xyzi(c) for c in size_map()), *IDENT)
    r = m.process(*(xyzi(c) for c in size_scan(nc, ns)), *SIZE_POSE)
    assert r["stack_size"] == [nc, ns] and r["optimized"], (nc, ns, r["stack_size"])
    r["stack"] = [s.copy() for s in m.stack]
    r["cubes"] = snapshot(m, r["touched"])
    return r


# ---------------------------------------------------------------- the shift sequence
# x < -375 gives centerCubeI = 2 (< 3), x >= 375 gives 18 (>= 21 - 3), the same for y; z < -125 gives
# centerCubeK = 2, z >= 125 gives 8 (>= 11 - 3); the centres move with every shift
SHIFT_STEPS = ((0, 0, 0), (-380, 0, 0), (380, 0, 0), (380, -380, 0), (380, 380, 0), (380, 380, -130),
               (380, 380, 130), (780, 380, 130))
SHIFT_WANT = ([0, 0, 0], [1, 0, 0], [-2, 0, 0], [0, 1, 0], [0, -2, 0], [0, 0, 1], [0, 0, -2], [-8, 0, 0])


def shift_clouds():
    return gate_clouds(12, 60)


@functools.lru_cache(maxsize=None)
def shift_model():
    """Per step: the result, the sizes of all cubes of both classes and the contents of the non-empty ones."""
    m = M.Mapper()
    c, s = (xyzi(x) for x in shift_clouds())
    out = []
    for t in SHIFT_STEPS:
        r = m.process(c, s, IDENT[0], [float(v) for v in t])
        r["sizes"] = [m.sizes(k) for k in range(2)]
        r["cubes"] = {(k, int(i)): m.cube(k, int(i)).copy() for k in range(2) for i in np.flatnonzero(r["sizes"][k])}
        out.append(r)
    return out


def check_shifts():
    run = shift_model()
    assert [r["shift"] for r in run] == [list(w) for w in SHIFT_WANT], [r["shift"] for r in run]
    assert run[1]["center"][0] == 3 and run[2]["center"][0] == 17            # 2 + 1 and 19 - 2
    seen = {(a, sgn) for r in run for a in range(3) for sgn in (1, -1) if r["shift"][a] * sgn > 0}
    assert len(seen) == 6                                                   # each of the six loops ran
    assert any(abs(v) >= 2 for r in run for v in r["shift"])                # two cubes in one step
    n_before, n_after = int(run[6]["sizes"][0].sum()), int(run[7]["sizes"][0].sum())
    assert n_after < n_before + run[7]["stack_size"][0]                     # a cube's content left the array
    return [r["shift"] for r in run]
