"""GPU tests of LIO-Livox's ScanRegistration on the device (slio_llreg_*,
include/slio_frontend.h) against the numpy restatement
tests/lio_livox_reg_model.py, to the bit: per-line flags, the line-feature
loop's visited mask, the lines' finite points, the sizes and the three clouds.
The inputs and the model's answers come from tests/lio_livox_reg_case.py, which
asserts them fit for purpose; the cases here add the seams of the kernels'
tiles (slio_llreg_tiles), the serial path of a long part, and the reuse of a
handle.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_livox_reg_case as K  # noqa: E402
import lio_livox_reg_model as M  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401
from test_lio_livox_reg_cpu import same_answer, same_points  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
EINVAL, ECAPACITY, ESTATE = -1, -4, -5


class Regs:
    """One handle per parameter set, made on first use."""

    def __init__(self):
        self.made = {}

    def get(self, prm):
        from agi_lidar_slam_amd.lio_livox import LioLivoxScanRegistration
        key = tuple(sorted(prm.items()))
        if key not in self.made:
            self.made[key] = LioLivoxScanRegistration(**prm)
        return self.made[key]

    def close(self):
        for r in self.made.values():
            r.close()


@pytest.fixture(scope="module")
def regs(L):
    r = Regs()
    yield r
    r.close()


@pytest.fixture(scope="module")
def tiles(L):
    from agi_lidar_slam_amd.lio_livox import tiles
    per_thread, per_wg, fast, block = tiles()
    assert per_wg >= M.MAX_LINE        # no seam between workgroups in a line's chain: one sees all of it
    return per_thread, fast, block


def device(reg, kind, data):
    """One message through the device, everything read back."""
    full, corner, surf = reg.FeatureExtract_Mid(data) if kind == "pc2" else reg.FeatureExtract(**data)
    ls, fs = reg.lines()
    per_line = [reg.flags(l) for l in range(M.MAX_SCANS)]
    return dict(cloud=full, corner=corner, surf=surf, counts=reg.counts, line_size=ls, finite_size=fs,
                flags=[p[0] for p in per_line], visited=[p[1] for p in per_line], lines=[p[2] for p in per_line])


def check(regs, prm, kind, data, what, want=None):
    want = K.run_model(prm, kind, data) if want is None else want
    same_answer(device(regs.get(prm), kind, data), want, what)
    return want


def test_fixtures_are_fit():
    K.check_fit()


@pytest.mark.parametrize("name", K.CPU_CASES)
def test_device_matches_model(regs, name):
    prm, kind, data = K.case(name)
    check(regs, prm, kind, data, name, K.model(name))


def test_line_of_20001_is_an_error_and_leaves_no_run(regs):
    reg = regs.get(K.P(n_scans=1))
    msg = K.one_line(M.MAX_LINE + 1)
    with pytest.raises(L_error(), match="20000"):
        reg.run(**msg)
    out = np.zeros((4, 8), F)
    assert reg.lib.slio_llreg_get_cloud(reg.h, 0, out.ctypes.data_as(C.POINTER(C.c_float)), 4) == ESTATE
    small = K.cut_lines(K.dense(), (300, 0, 0, 0, 0, 0))
    check(regs, K.P(n_scans=1), "msg", small, "a run after the refused one")


def L_error():
    from agi_lidar_slam_amd._lib import SlioError
    return SlioError


def test_chain_seams(regs, tiles):
    """A line cut so that m - 5, the loop's end, lies one and two positions
    either side of (and on) every seam between two threads' runs, and the
    chain entering the runs at all four offsets."""
    per_thread = tiles[0]
    lines = K.cut_lines(K.dense(), (0, None, None, 0, 0, 0))      # line 2 is the longest, with the crafted spots
    m_all = int((lines["line"] == 1).sum())
    seen = set()
    seams = [t * per_thread for t in range(1, (m_all - 10) // per_thread + 1)]
    assert len(seams) >= 8
    for s in seams:
        for d in (-2, -1, 0, 1, 2):
            m = s + 10 + d                                         # loop positions 5 .. m - 6: s + d of them
            msg = K.cut_lines(lines, (0, m, m, 0, 0, 0))
            want = check(regs, K.P(), "msg", msg, f"lines of {m}")
            for l in (1, 2):
                seen |= K.entry_offsets(want["visited"][l], per_thread)
    assert seen == {0, 1, 2, 3}


def test_block_seams(regs, tiles):
    """Messages of one below, exactly and one above a whole number of
    workgroups of the ingest, feature, flag and collection kernels."""
    block = tiles[2]
    d = K.dense()
    for n in (block - 1, block, block + 1, 2 * block - 1, 2 * block, 2 * block + 1, 7 * block, 7 * block + 1):
        msg = K.retime({k: np.ascontiguousarray(v[:n]) for k, v in d.items()})
        check(regs, K.P(), "msg", msg, f"message of {n}")
        check(regs, K.P(M.MID360), "pc2", K.as_pc2(msg), f"pc2 of {n}")


def test_part_lengths_around_the_register_window(regs, tiles):
    """Parts one below, at and one above the longest part the picking kernel
    resolves in registers, mixed in one line so that neighbour marks cross
    between a part on the register path and a part on the serial path; and
    parts of one point and of none (more parts than points)."""
    fast = tiles[1]
    for part_num, extra in ((4, -4), (4, 0), (4, 2), (4, 4), (9, 5)):
        m = 11 + part_num * fast + extra
        msg = K.cut_lines(K.dense(), (0, 0, m, m - 1, 0, 0))
        prm = K.P(part_num=part_num)
        want = check(regs, prm, "msg", msg, f"{part_num} parts over {m}")
        lens = {K.M._cdiv((m - 11) * (j + 1), part_num) - K.M._cdiv((m - 11) * j, part_num) for j in range(part_num)}
        if extra == 2:
            assert lens == {fast, fast + 1}
        assert want["counts"][2] > 0
    msg = K.cut_lines(K.dense(), (0, 0, 80, 300, 0, 0))
    check(regs, K.P(part_num=150), "msg", msg, "more parts than points")          # lengths 0 and 1
    check(regs, K.P(part_num=289), "msg", msg, "every part one point")            # line 3: m - 11 = 289


def test_long_parts_take_the_serial_path(regs, tiles):
    fast = tiles[1]
    msg = K.cut_lines(K.dense(), (None, None, None, 0, 0, 0))
    for part_num in (1, 3):
        want = check(regs, K.P(part_num=part_num), "msg", msg, f"PartNum {part_num}")
        assert min(want["finite_size"][:3]) - 11 > part_num * (fast + 1)             # every part is a long one
        assert want["stats"]["pick300"] >= 1 and want["counts"][2] > 0


def test_a_frame_of_six_lines_of_4000(regs):
    from agi_lidar_slam_amd import synth
    pos = np.array([synth.SENSOR_STREET[0] - 3.0, synth.SENSOR_STREET[1] + 0.2, 1.6])
    msg = synth.make_livox_lines(K.scene(), pos, 0.0, 6, 5600, seed=K.SEED + 5)
    msg = K.cut_lines(msg, (4000,) * 6)
    assert len(msg["xyz"]) == 24000
    want = check(regs, K.P(), "msg", msg, "6 x 4000")
    assert want["counts"][1] > 50 and want["counts"][2] > 5000


def test_two_sizes_on_one_handle(regs):
    """A long message, a short one, an empty one and the long one again: no
    state of a run survives into the next."""
    big = K.dense()
    small = K.cut_lines(big, (40, 12, 0, 300, 11, 0))
    empty = K.cut_lines(big, (0,) * 6)
    for what, msg in (("big", big), ("small", small), ("empty", empty), ("small again", small), ("big again", big)):
        check(regs, K.P(), "msg", msg, what)
    check(regs, K.P(), "pc2", K.as_pc2(small), "pc2 after msg")


def test_getters_against_the_view(regs):
    prm, kind, data = K.case("dense")
    reg = regs.get(prm)
    full, corner, surf = reg.FeatureExtract(**data)
    v = reg.view()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert [v.n_cloud, v.n_corner, v.n_surf] == [int(c) for c in reg.counts] and v.device == 0
    for ptr, n, got, name in ((v.cloud, v.n_cloud, full, "cloud"), (v.corner, v.n_corner, corner, "corner"),
                              (v.surf, v.n_surf, surf, "surf")):
        host = np.zeros((n, 8), F)
        assert hip.hipMemcpy(host.ctypes.data, ptr, host.nbytes, 2) == 0          # device -> host
        same_points(host, got, name)
    # the corner and surf clouds are the labelled points of the cloud, in cloud order
    same_points(full[full[:, 6] == 1], corner, "corner of cloud")
    same_points(full[full[:, 6] == 2], surf, "surf of cloud")


def test_errors_on_a_live_handle(regs):
    from agi_lidar_slam_amd import _lib as lb
    from agi_lidar_slam_amd.lio_livox import LioLivoxScanRegistration
    lib = lb.load()
    fresh = LioLivoxScanRegistration(max_points=1000, **K.P(n_scans=3))
    xyz, u8, u32 = np.ones((4, 3), F), np.zeros(4, np.uint8), np.arange(1, 5, dtype=np.uint32)
    xyzi, c3, i32 = np.ones((4, 4), F), np.zeros(3, np.int32), np.zeros(6, np.int32)
    msg = (lb.fptr(xyz), lb.u8ptr(u8), lb.u8ptr(u8), lb.u32ptr(u32))
    assert lib.slio_llreg_get_cloud(fresh.h, 0, lb.fptr(xyzi), 4) == ESTATE
    assert lib.slio_llreg_get_lines(fresh.h, lb.iptr(i32), lb.iptr(i32)) == ESTATE
    assert lib.slio_llreg_get_flags(fresh.h, 0, None, None, None, 4) == ESTATE
    assert lib.slio_llreg_get_view(fresh.h, C.byref(lb.SlioLlregView())) == ESTATE
    assert lib.slio_llreg_run(fresh.h, None, lb.u8ptr(u8), lb.u8ptr(u8), lb.u32ptr(u32), 4, lb.iptr(c3)) == EINVAL
    assert lib.slio_llreg_run(fresh.h, *msg, -1, lb.iptr(c3)) == EINVAL
    assert lib.slio_llreg_run(fresh.h, *msg, 4, None) == EINVAL
    assert lib.slio_llreg_run(fresh.h, *msg, 1001, lb.iptr(c3)) == ECAPACITY
    assert lib.slio_llreg_run_pc2(fresh.h, lb.fptr(xyzi), 4, lb.iptr(c3)) == EINVAL       # three lines
    assert b"n_scans >= 4" in lib.slio_last_error()
    assert lib.slio_llreg_run(fresh.h, *msg, 4, lb.iptr(c3)) == 0 and list(c3) == [4, 0, 0]
    assert lib.slio_llreg_get_cloud(fresh.h, 3, lb.fptr(xyzi), 4) == EINVAL
    assert lib.slio_llreg_get_cloud(fresh.h, 0, lb.fptr(np.zeros((4, 8), F)), 3) == ECAPACITY
    assert lib.slio_llreg_get_flags(fresh.h, 6, None, None, None, 4) == EINVAL
    assert lib.slio_llreg_get_flags(fresh.h, 0, lb.iptr(i32), None, None, 3) == ECAPACITY
    assert lib.slio_llreg_get_view(fresh.h, None) == EINVAL
    gone = C.c_void_p(fresh.h.value)
    fresh.close()
    assert lib.slio_llreg_run(gone, *msg, 4, lb.iptr(c3)) == EINVAL
    assert lib.slio_llreg_destroy(gone) == EINVAL
