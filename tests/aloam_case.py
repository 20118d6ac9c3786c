"""The clouds of the A-LOAM scanRegistration tests (tests/test_aloam_cpu.py,
tests/test_gpu_aloam.py) and the model's answers to them, computed once and
shared.  Every case is named; `check_*` assert on the MODEL that a case
reaches what it is there for, so the reference alone shows the branch and not
only the code under test.  Natural clouds come from synth.make_vlp16_sweep /
make_spinning_sweep; a case that is crafted says so.
"""
import functools
import math

import numpy as np

import aloam_model as M
from agi_lidar_slam_amd import synth

F = np.float32
VLP16 = -15.0 + 2.0 * np.arange(16)
# beams centred in the reference's bins: 32 lines, scanID = int((angle + 92/3) * 3/4) (:189)
HDL32 = -92.0 / 3.0 + (np.arange(32) + 0.5) * 4.0 / 3.0
# 64 lines (:195-198): the upper block int((2 - angle) * 3 + 0.5) -> 0 .. 32, the
# lower block 32 + int((-8.83 - angle) * 2 + 0.5) -> 33 .. 63, of which 51 .. 63
# are dropped by `scanID > 50` (:201).  (The top beam sits on `angle > 2`: its
# noise drops about half of it.)
HDL64 = np.concatenate([2.0 - np.arange(33) / 3.0, -8.83 - np.arange(1, 32) / 2.0])
LAYOUT = {"dense": 16, "hdl32": 32, "hdl64": 64}


def _xyz(sw):
    return np.stack([sw["x"], sw["y"], sw["z"]], 1).astype(F)


@functools.lru_cache(maxsize=None)
def dense():
    return _xyz(synth.make_vlp16_sweep(horizon=900))


def rot_z(xyz, a):
    c, s = F(math.cos(a)), F(math.sin(a))
    return np.stack([c * xyz[:, 0] - s * xyz[:, 1], s * xyz[:, 0] + c * xyz[:, 1], xyz[:, 2]], 1).astype(F)


def ring(n, elev_deg, seed, r0=20.0, az0=math.pi, turn=2 * math.pi, z_fixed=None):
    """CRAFTED: n points of one beam, clockwise from az0 over `turn`, on a wavy
    wall (range r0 +- 25 % with steps) so that sharp and flat stretches both
    occur.  z_fixed: the points coplanar at that height instead of on a cone."""
    rng = np.random.default_rng(seed)
    az = az0 - np.arange(n) * (turn / n)
    r = r0 * (1 + 0.2 * np.sin(7 * az) + 0.05 * (np.sin(31 * az) > 0.6)) + rng.normal(0, 0.004, n)
    z = np.full(n, z_fixed) if z_fixed is not None else r * math.tan(math.radians(elev_deg))
    return np.stack([r * np.cos(az), r * np.sin(az), z], 1).astype(F)


def at(az, elev_deg, r=10.0):
    e = math.radians(elev_deg)
    return np.array([[r * math.cos(e) * math.cos(az), r * math.cos(e) * math.sin(az), r * math.sin(e)]], F)


def one_scan(count, seed=3):
    """CRAFTED: one populated scan (id 8 of 16) of `count` coplanar ring points."""
    return ring(count, 1.0, seed, z_fixed=0.35)


@functools.lru_cache(maxsize=None)
def cut(name):
    d = dense()
    n = len(d)
    nan = np.full((1, 3), np.nan, F)
    if name == "dense":
        return d
    if name.startswith("rot"):                          # rot1, rot2, rot3
        return rot_z(d, float(name[3:]))
    if name.startswith("part40_rot"):                   # the first 40 % of the sweep: no switch point
        return rot_z(d[:int(0.4 * n)], float(name[10:]))
    if name == "late_near_start":
        # CRAFTED: in the sweep rotated by 1 rad (startOri = pi - 1) a few late points are moved
        # to an azimuth of 2.8 rad, more than 3/2 pi of orientation below endOri - 2 pi: the
        # second branch's += 2 pi
        c = cut("rot1").copy()
        for k, i in enumerate(range(n - 400, n - 380)):
            c[i] = at(2.8 + 0.005 * k, -15 + 2 * (i % 16))[0]
        return c
    if name == "hdl32":
        return _xyz(synth.make_spinning_sweep(HDL32, horizon=300))
    if name == "hdl64":
        return _xyz(synth.make_spinning_sweep(HDL64, horizon=250))
    if name == "empty":
        return np.zeros((0, 3), F)
    if name == "all_range":
        return (d[:300] * F(0.0005)).astype(F)
    if name == "all_scan_id":
        return np.concatenate([at(0.01 * k, 40.5 + 0.1 * (k % 7)) for k in range(200)])
    if name == "survivors_all_dropped":                 # non-finite, too close, and the rest outside the layout
        return np.concatenate([nan, d[:40] * F(0.0005), at(0.3, 50.7), nan, at(2.0, -50.7), d[40:60] * F(0.0005)])
    if name == "small_scans":
        # CRAFTED: scans of 16, 17, 18 and 23 points (scanEndInd - scanStartInd = 5, 6, 7, 12: the
        # skip boundary and one-point sectors), interleaved in firing order
        parts = [ring(c, -15 + 2 * k, 10 + k, turn=0.4) for k, c in enumerate((16, 17, 18, 23))]
        rows = [parts[k][i] for i in range(23) for k in range(4) if i < len(parts[k])]
        return np.array(rows, F)
    if name == "one_scan":
        return one_scan(300)
    if name == "nan_start":
        return np.concatenate([np.repeat(nan, 7, 0), d[:3000]])
    if name == "nan_end":
        return np.concatenate([d[:3000], np.repeat(nan, 9, 0)])
    if name == "nan_runs":
        c = d[:4000].copy()
        for a, b in ((0, 3), (100, 140), (255, 258), (1000, 1300), (3990, 4000)):
            c[a:b, (a // 7) % 3] = np.inf if a % 2 else np.nan
        return c
    if name == "early_outside_layout":
        # CRAFTED: the 4th point lies half a turn past the start at an elevation outside the
        # layout: it is dropped and must not set halfPassed
        a0 = math.atan2(float(d[0, 1]), float(d[0, 0]))
        return np.concatenate([d[:3], at(a0 - 3.5, 40.7), d[3:]])
    if name == "switch_first_kept":
        # CRAFTED: the first survivor (it fixes startOri) is outside the layout, and the first kept
        # point is already more than pi past it
        a0 = math.atan2(float(d[0, 1]), float(d[0, 0]))
        return np.concatenate([at(a0 + 3.5, 40.7), d[:3000]])
    if name == "repeated":
        # CRAFTED: four scans, each with runs of one repeated point (curvature ties, gap 0)
        parts = [ring(400, -15 + 2 * k, 20 + k) for k in range(4)]
        for q in parts:
            q[100:114] = q[100]
            q[250:262] = q[250]
        return np.concatenate(parts)
    if name == "vg_overflow":
        # CRAFTED: one scan (id 8 of 16) on a half circle 1.84 km out, z spread over 26 m: the
        # bounding box of its less-flat points has more than 2^31 voxels of 0.2 m
        k = np.arange(200)
        az = math.pi - k * (math.pi / 200)
        el = np.radians(1.0 + 0.4 * np.sin(1.7 * k))
        r = 1838.0
        return np.stack([r * np.cos(az), r * np.sin(az), r * np.tan(el)], 1).astype(F)
    raise KeyError(name)


def layout(name):
    return LAYOUT.get(name, 16)


@functools.lru_cache(maxsize=None)
def model(name):
    return M.register(cut(name), n_scans=layout(name))


CPU_CASES = ("dense", "rot1", "rot2", "rot3", "part40_rot1", "part40_rot2", "late_near_start", "empty", "all_range",
             "all_scan_id", "survivors_all_dropped", "small_scans", "one_scan", "nan_start", "nan_end", "nan_runs",
             "early_outside_layout", "switch_first_kept", "repeated", "hdl32", "hdl64", "vg_overflow")


# ---------------------------------------------------------------- fitness of the cases (on the model)
def scan_margin(name):
    """The least distance of a survivor's pre-truncation scan value to an
    integer, over the points the filters keep: either reading of the
    reference's atan (float or double) gives the same ids while it is large."""
    p = cut(name)
    p = p[np.isfinite(p).all(1)]
    p = p[(p * p).sum(1) >= 0.01]
    if not len(p):
        return 0.5
    v = M.scan_value(layout(name), M.elevation_deg(p))
    return float(np.min(np.abs(v - np.round(v))))


def check_margins():
    for name in CPU_CASES:
        assert scan_margin(name) > 1e-3, name


def check_dense_is_fit():
    w = model("dense")
    st, info = w["stats"], w["info"]
    assert len(cut("dense")) > 10000 and st["drop_scan"] == 0
    for k in ("break21", "flat", "break4", "seam_marks", "seam_suppressed", "end_minus", "first_minus",
              "second_minus", "half_passed"):
        assert st[k] > 0, k
    assert info["both_breaks"] > 0 and info["mark_ep5"] > 0
    assert 100 < info["max_sector"] < 200
    cnt = np.bincount(np.floor(w["laserCloud"][:, 3]).astype(int), minlength=16)
    assert cnt.min() > 250
    assert info["tied_sectors"] == 0                    # no curvature ties inside a sector of the natural sweep
    return st


def check_orientation_branches():
    """Every orientation branch is reached by some case (the issue's table)."""
    for name in ("rot1", "rot2", "rot3"):
        assert model(name)["stats"]["first_plus"] > 0, name
    for name in ("part40_rot1", "part40_rot2"):
        st = model(name)["stats"]
        assert st["end_plus"] == 1 and st["half_passed"] == 0, name
    assert model("late_near_start")["stats"]["second_plus"] > 0
    st = model("dense")["stats"]
    assert st["end_minus"] == 1 and st["first_minus"] > 0 and st["second_minus"] > 0


def check_crafted_cases():
    assert model("all_range")["stats"]["drop_range"] == 300 and model("all_range")["counts"].sum() == 0
    assert model("all_scan_id")["stats"]["drop_scan"] == 200 and model("all_scan_id")["counts"].sum() == 0
    st = model("survivors_all_dropped")["stats"]
    assert (st["drop_nonfinite"], st["drop_range"], st["drop_scan"]) == (2, 60, 2)
    w = model("small_scans")
    assert list(w["scan_end"][:4] - w["scan_start"][:4]) == [5, 6, 7, 12]
    assert w["stats"]["scans_skipped"] == 13 and w["counts"][0] == 74
    w = model("one_scan")
    assert w["stats"]["scans_skipped"] == 15 and w["counts"][1] > 0 and w["counts"][4] > 0
    assert model("early_outside_layout")["info"]["switch_kept"] == model("dense")["info"]["switch_kept"]
    assert model("early_outside_layout")["stats"]["drop_scan"] == 1
    assert model("switch_first_kept")["info"]["switch_kept"] == 0
    for name in ("nan_start", "nan_end", "nan_runs"):
        assert model(name)["stats"]["drop_nonfinite"] > 0
    assert model("repeated")["info"]["tied_sectors"] > 0
    assert model("vg_overflow")["stats"]["vg_overflow"] == 1
    st = model("hdl64")["stats"]
    assert st["drop_over50"] > 0 and st["drop_scan"] > st["drop_over50"]
    cnt = np.bincount(np.floor(model("hdl64")["laserCloud"][:, 3]).astype(int), minlength=64)
    assert cnt[51:].sum() == 0 and (cnt[1:51] > 0).all()
    cnt = np.bincount(np.floor(model("hdl32")["laserCloud"][:, 3]).astype(int), minlength=32)
    assert (cnt > 0).all() and model("hdl32")["stats"]["drop_scan"] == 0
