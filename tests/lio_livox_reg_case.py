"""The inputs of tests/test_lio_livox_reg_cpu.py and
tests/test_gpu_lio_livox_reg.py and the model's answers on them
(tests/lio_livox_reg_model.py), each computed once per process, with the
assertions that the fixtures reach every branch of the node.

A case is (params, kind, arrays): kind "msg" is a CustomMsg as dict(xyz,
reflectivity, line, offset_time) for FeatureExtract, kind "pc2" an (n, 4) cloud
for lidarCallBackPc2.

Crafted spots (spliced into line 2 of the dense frame, `crafted()`); the
natural frames of the scene reach the other branches on their own:
  - a break point whose left and right neighbours continue one straight line,
    so the fan test finds cc = 1 and demotes it to 101;
  - a break point whose three left neighbours are nearer than 1 m, so both fans
    stay zero, cc is 0 / 0 = NaN and the point goes to 101;
  - a flat stretch nearer than LidarNearestDis, which the collection skips;
  - evenly spaced collinear points with exactly representable coordinates,
    whose curvatures are all exactly 0, so only the sort's stability orders
    them.
The far picks beyond NumFlat need points beyond DistanceFaraway in parts of more
than NumFlat candidates: the "far" case lowers DistanceFaraway to 12 m and
PartNum to 20 on the same frame.

Not reached, and not forced: the `depth_right == 0` / `depth_left == 0` routes
of the break-point rules (:480, :520).  A point of depth 0 has x = 0, and the
ingest drops every x < 0.01 (fabs(x) < 0.01 for lidar_type 2) before
detectFeaturePoint sees it.
"""
import functools

import numpy as np

import lio_livox_reg_model as M

F = np.float32
SEED = 20261020
SMALL_M = (0, 1, 10, 11, 12)              # 11: the first size at which a loop body runs
PART_NUMS = (1, 100, 150)


@functools.lru_cache(maxsize=None)
def scene():
    from agi_lidar_slam_amd import synth
    return synth.make_scene(SEED, 1000)


@functools.lru_cache(maxsize=None)
def _frame(n_lines, rays, seed=1):
    from agi_lidar_slam_amd import synth
    pos = np.array([synth.SENSOR_STREET[0] - 3.0, synth.SENSOR_STREET[1] + 0.2, 1.6])
    return synth.make_livox_lines(scene(), pos, 0.0, n_lines, rays, seed=SEED + seed)


def copy(msg):
    return {k: v.copy() for k, v in msg.items()}


def retime(msg):
    """offset_time rising evenly to 0.1 s again, after an edit."""
    n = len(msg["xyz"])
    msg["offset_time"] = (np.arange(1, n + 1, dtype=np.float64) * (1e8 / max(n, 1))).astype(np.uint32)
    return msg


def crafted():
    """The four crafted spots as one run of points (x, y, z, reflectivity)."""
    rows = []
    # 101 by cc >= 0.95: 24 collinear points 0.3 m apart on a wall at 51 degrees to the ray, with one
    # 1.5 m step; depth rises along the line, so the point before the step is a left break point
    s = 0.3 * np.arange(24, dtype=np.float64)
    s[12:] += 1.2
    rows += [np.array([25.0, -10.0, 0.5]) + t * np.array([0.6, 0.8, 0.0]) for t in s]
    # a flat stretch nearer than 1 m: 16 points 1 cm apart at x = 0.8
    rows += [np.array([0.8, -0.08 + 0.01 * k, 0.0]) for k in range(16)]
    # 101 by NaN: three neighbours nearer than 1 m on the left, a 2.2 m step on the right
    rows += [np.array(p) for p in ((0.5, 0.6, 0.0), (0.6, 0.5, 0.0), (0.7, 0.3, 0.0), (0.8, 0.0, 0.0))]
    rows += [np.array([3.0 + 0.05 * k, 0.02 * k, 0.0]) for k in range(8)]
    # curvature ties: 24 collinear points 0.25 m apart, every coordinate a dyadic number
    rows += [np.array([16.0, -3.0 + 0.25 * k, 0.5]) for k in range(24)]
    xyz = np.array(rows, np.float64)
    refl = (37 * np.arange(len(xyz)) % 200).astype(np.float64)
    return np.concatenate([xyz, refl[:, None]], 1).astype(F)


def splice(msg, line, at, pts):
    """pts (k, 4) put into `line` after its at-th point."""
    pos = np.nonzero(msg["line"] == line)[0][at] + 1
    out = dict(xyz=np.concatenate([msg["xyz"][:pos], pts[:, :3], msg["xyz"][pos:]]),
               reflectivity=np.concatenate([msg["reflectivity"][:pos], pts[:, 3].astype(np.uint8),
                                            msg["reflectivity"][pos:]]),
               line=np.concatenate([msg["line"][:pos], np.full(len(pts), line, np.uint8), msg["line"][pos:]]))
    return retime({k: np.ascontiguousarray(v) for k, v in out.items()})


@functools.lru_cache(maxsize=None)
def dense():
    """Six lines of about 550 returns each, the crafted spots in line 2."""
    return splice(_frame(6, 700), 2, 300, crafted())


def cut_lines(msg, sizes):
    """The first sizes[l] points of each line l (all of it for None), order kept."""
    keep = np.zeros(len(msg["line"]), bool)
    for l, m in enumerate(sizes):
        idx = np.nonzero(msg["line"] == l)[0]
        keep[idx if m is None else idx[:m]] = True
    return retime({k: np.ascontiguousarray(v[keep]) for k, v in msg.items()})


def one_line(m, line=0):
    """m points on one line: the dense frame's lines one after another."""
    d = dense()
    order = np.argsort(d["line"], kind="stable")
    reps = -(-m // len(order))
    idx = np.tile(order, reps)[:m]
    return retime(dict(xyz=np.ascontiguousarray(d["xyz"][idx]), reflectivity=np.ascontiguousarray(d["reflectivity"][idx]),
                       line=np.full(m, line, np.uint8)))


def with_nonfinite(msg):
    """NaN / inf in line 1 at its start, at its end and in a run, and one in line 4."""
    msg = copy(msg)
    i1, i4 = np.nonzero(msg["line"] == 1)[0], np.nonzero(msg["line"] == 4)[0]
    for k, j in enumerate(list(i1[:3]) + list(i1[-3:]) + list(i1[200:207]) + [i4[100]]):
        msg["xyz"][j, k % 3] = np.nan if k % 2 else np.inf
    return msg


def with_signs(msg):
    """x < 0, |x| < 0.01 and NaN x in stretches of lines 0 and 3: what the three lidar types filter apart."""
    msg = copy(msg)
    i0, i3 = np.nonzero(msg["line"] == 0)[0], np.nonzero(msg["line"] == 3)[0]
    msg["xyz"][i0[100:160], 0] *= -1.0
    msg["xyz"][i0[300:304], 0] = [0.005, -0.005, 0.0, 0.0099]
    msg["xyz"][i3[50:53], 0] = [np.nan, -np.nan, 0.01]
    return msg


def as_pc2(msg):
    return np.ascontiguousarray(np.concatenate([msg["xyz"], msg["reflectivity"][:, None].astype(F)], 1), F)


def with_bad_intensity(cloud):
    """NaN and +-inf intensities in a Pc2 cloud (only x, y and z are tested for
    finiteness): alone, side by side in one line (every fourth point), and at a
    line's start, so that diffR is NaN or infinite for whole stretches of a
    part and the sort has to place them."""
    c = cloud.copy()
    for i, v in ((2, np.nan), (400, np.nan), (404, np.inf), (408, -np.inf), (412, np.nan), (801, np.inf),
                 (1203, -np.inf), (1207, -np.inf), (2002, np.nan), (2006, np.nan), (2010, np.nan), (2500, np.inf),
                 (2504, np.inf), (3001, np.nan)):
        c[i, 3] = v
    return c


def P(base=M.HORIZON, **kw):
    return dict(base, **kw)


def _part_sizes(p):
    # m - 11 in {PartNum - 1, PartNum, PartNum + 1} on three lines
    return cut_lines(dense(), (p + 10, p + 11, p + 12, 0, 0, 0))


def _zero_span():
    msg = copy(dense())
    msg["offset_time"][:] = 0
    return msg


CASES = {
    "dense": lambda: (P(), "msg", dense()),
    "far": lambda: (P(distance_faraway=12.0, part_num=20), "msg", dense()),
    "mid360": lambda: (P(M.MID360), "msg", with_signs(_frame(4, 600, seed=2))),
    "small_m": lambda: (P(), "msg", cut_lines(dense(), SMALL_M + (40,))),
    "unequal": lambda: (P(), "msg", cut_lines(dense(), (500, 37, None, 11, 260, 12))),
    "absent_line": lambda: (P(), "msg", cut_lines(dense(), (None, None, None, 0, None, None))),
    "n_scans_1": lambda: (P(n_scans=1), "msg", dense()),
    "n_scans_4": lambda: (P(n_scans=4), "msg", dense()),
    "nonfinite": lambda: (P(), "msg", with_nonfinite(dense())),
    "type0_signs": lambda: (P(lidar_type=0), "msg", with_signs(dense())),
    "type1_signs": lambda: (P(lidar_type=1), "msg", with_signs(dense())),
    "type2_signs": lambda: (P(lidar_type=2), "msg", with_signs(dense())),
    "pc2": lambda: (P(M.MID360), "pc2", as_pc2(with_signs(dense()))),
    "pc2_type0_6": lambda: (P(lidar_type=0), "pc2", as_pc2(with_nonfinite(dense()))),
    # parts of about 9 points (the register path) and of about 300 (the serial path)
    "pc2_bad_intensity": lambda: (P(M.MID360), "pc2", with_bad_intensity(as_pc2(dense()))),
    "pc2_bad_intensity_long_parts": lambda: (P(M.MID360, part_num=3), "pc2", with_bad_intensity(as_pc2(dense()))),
    "zero_span": lambda: (P(), "msg", _zero_span()),
    "empty": lambda: (P(), "msg", cut_lines(dense(), (0,) * 6)),
    "empty_pc2": lambda: (P(M.MID360), "pc2", np.zeros((0, 4), F)),
    "line_20000": lambda: (P(n_scans=1), "msg", one_line(M.MAX_LINE)),
}
for _p in PART_NUMS:
    CASES[f"parts_{_p}"] = functools.partial(lambda p: (P(part_num=p), "msg", _part_sizes(p)), _p)
CPU_CASES = tuple(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def run_model(prm, kind, data):
    return M.feature_extract_mid(prm, data) if kind == "pc2" else M.feature_extract(prm, **data)


@functools.lru_cache(maxsize=None)
def model(name):
    return run_model(*case(name))


def check_fit():
    """Every branch the issue lists is reached on the fixtures."""
    d, f = model("dense")["stats"], model("far")["stats"]
    assert d["lines_k2"] >= 1 and d["lines_k3"] >= 1, d
    assert f["far_pick_beyond_numflat"] >= 1, f
    for key in ("angle_pick", "pick300", "pick300_over_2", "skip_marked_by_previous_part", "previous_part_2_to_1",
                "gap_stopped_mark", "curvature_ties", "set150", "set100_left", "set100_right", "set101_cc",
                "set101_nan", "near_skipped", "stride1", "stride4"):
        assert d[key] >= 1, (key, d)
    # the ties are in the crafted collinear stretch: its curvatures are exactly zero
    fl = model("dense")
    assert fl["counts"][1] > 0 and fl["counts"][2] > 0
    nf = model("nonfinite")
    assert nf["finite_size"][1] == nf["line_size"][1] - 13 and nf["finite_size"][4] == nf["line_size"][4] - 1
    # the literal index: labels of line 1 land on points a finite-only index would not pick
    lab = nf["cloud"][:, 6]
    on_nonfinite = ~np.isfinite(nf["cloud"][:, :3]).all(1) & (lab > 0)
    assert on_nonfinite.any(), "no label landed on a non-finite point of line 1"
    ls = model("type0_signs")["line_size"], model("type2_signs")["line_size"]
    assert ls[0][0] < ls[1][0] < dense()["line"].tolist().count(0)
    assert model("small_m")["finite_size"][:5] == list(SMALL_M)
    for p in PART_NUMS:
        assert model(f"parts_{p}")["finite_size"][:3] == [p + 10, p + 11, p + 12]
    assert model("n_scans_1")["line_size"][1:] == [0] * 5 and model("n_scans_4")["line_size"][4:] == [0, 0]
    assert model("line_20000")["finite_size"][0] == M.MAX_LINE
    for name in ("pc2_bad_intensity", "pc2_bad_intensity_long_parts"):
        bad = model(name)
        assert sum(int((~np.isfinite(c[:, 3])).sum()) for c in bad["lines"]) == 14 and bad["counts"][2] > 0
    return d


def entry_offsets(visited, per_thread):
    """The offsets (0 .. 3) at which the line-feature chain enters the runs of
    per_thread loop positions that the chain kernel gives its threads."""
    seen = set()
    pos = np.nonzero(visited)[0] - 5
    for t in range(1, int(pos.max()) // per_thread + 1 if len(pos) else 0):
        after = pos[pos >= t * per_thread]
        if len(after):
            seen.add(int(after[0]) - t * per_thread)
    return seen
