"""CPU: the crafted UndistortPcl step-5 cases (tests/undistort_case.py) reach
what they are named for, and the oracle's restatement of the backward double
loop (orc_undistort_points, oracle/imu_oracle.cpp) agrees with the
independent longdouble reference on every one of them, within

    |got - ref| <= 0.5 ulp32(ref) + 64 * 2^-53 * (||P|| + ||T_LI|| + ||T_ei|| + 1)

(the final rounding to float; an fp64 chain of about 40 operations).  No GPU
needed."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import undistort_case as UC  # noqa: E402


def test_cases_reach_their_targets():
    assert UC.check_cases() == len(UC.NAMES) >= 30
    # what the bisection and the early stop k_undistort used to have get wrong
    missed = UC.bisection_misses()
    print("cases the former segment search / first-point loop gets wrong:", missed)
    assert set(missed) == {f"neg_offset_{d}_np{m}" for d in ("20us", "4ms") for m in (3, 6, 7, 12)} | {
        "first_skips_a_head"}


def test_oracle_vs_longdouble_reference(oracle_mod):
    worst, chain = (0.0, ""), (0.0, "")
    for name in UC.NAMES:
        c, m, (ref, scale, checked) = UC.solved(name)
        pts, t = oracle_mod.undistort_points(c["tab"], c["state"], c["pts"], c["t"])
        # the stable time order, the original bits of the times
        np.testing.assert_array_equal(t.view(np.uint32), m["t"].view(np.uint32), err_msg=name)
        src = c["pts"][m["order"]]
        # no segment: the point is not touched
        still = m["seg"] < 0
        np.testing.assert_array_equal(pts[still].view(np.uint32), src[still].view(np.uint32), err_msg=name)
        # non-finite rows stay in place and stay non-finite
        bad = ~np.isfinite(src).all(axis=1)
        assert not np.isfinite(pts[bad]).all(axis=1).any(), name
        r = UC.worst_ratio(pts, ref, scale, checked)
        worst = max(worst, (r, name))
        chain = max(chain, (UC.worst_chain_ratio(pts, ref, scale, checked), name))
        assert r <= 1.0, (name, r)
        # the share of points whose float differs from the once-rounded reference
        if checked.any():
            off = (pts[checked] != ref[checked].astype(np.float32)).any(axis=1).mean()
            assert off <= 0.01, (name, off)
        # the same input in time order gives the same output
        p2, t2 = oracle_mod.undistort_points(c["tab"], c["state"], *UC.presorted(c))
        np.testing.assert_array_equal(p2.view(np.uint32), pts.view(np.uint32), err_msg=name)
        np.testing.assert_array_equal(t2.view(np.uint32), t.view(np.uint32), err_msg=name)
    print(f"oracle vs longdouble reference: worst |err| / bound = {worst[0]:.4f} ({worst[1]}); worst "
          f"(|err| - half an ulp) / chain term = {chain[0]:.4f} ({chain[1]})")


def test_first_point_is_compensated_once_per_head(oracle_mod):
    """The first sorted point goes through the model's head list, one head at
    a time with a rounding to float in between: each step is a one-point scan
    on the two-row table (head, tail), held to the longdouble reference, and
    the chain of steps equals the full run bit for bit."""
    for name in ("first_late", "first_late_n1", "first_late_neg_offset", "first_skips_a_head"):
        c, m, _ = UC.solved(name)
        full, _ = oracle_mod.undistort_points(c["tab"], c["state"], c["pts"], c["t"])
        p, t = c["pts"][m["order"]][:1], c["t"][m["order"]][:1]
        assert len(m["first_heads"]) >= 2
        for k in m["first_heads"]:
            one = dict(c, tab=c["tab"][k:k + 2], pts=p, t=t)
            mk = UC.model(one)
            assert mk["seg"].tolist() == [0]
            ref, scale, _ = UC.reference(one, mk)
            p, _ = oracle_mod.undistort_points(one["tab"], c["state"], p, t)
            assert UC.worst_ratio(p, ref, scale, np.array([True])) <= 1.0, (name, k)
        np.testing.assert_array_equal(full[0].view(np.uint32), p[0].view(np.uint32), err_msg=name)
