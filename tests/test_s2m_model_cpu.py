"""The oracle of the LIO-SAM scan-to-map core (oracle/lio_s2m_oracle.cpp, the
float arithmetic the device is held to bit for bit) against the fp64 model
written from the geometry (tests/s2m_model.py), on the fixtures of
tests/s2m_case.py; and the conditions those fixtures must meet before
tests/test_gpu_lio_s2m.py runs anything on the device.  No GPU.

Tolerances, all from the oracle against the model, none from the device:

  coefficients   |oracle - model| <= C * unit per point, unit = the model's
                 conditioning scale (s2m_model.py: 2^-24 (1 + range)(1 + 1/d)
                 for corners, 2^-24 cond(A)(1 + |w - c|) for surfs).  Largest
                 ratio measured over cut() at both transforms and clusters()
                 at both transforms: corner 3.41 (a random line cluster,
                 d = 2 mm; 1.34 on cut(), where the largest error is 5.8e-4 at
                 d = 2.4 mm and 40 m range), surf 1.57 (cut(); largest error
                 5.5e-5).  C = 4 x that: CORNER_C = 13.7, SURF_C = 6.3.
  normal         max |oracle - model| / max |model| over the entries of A^T A
  equations      and of A^T B on cut() (1627 rows): measured 3.3e-8 / 4.4e-8 at
                 tf and 4.1e-8 / 4.0e-8 at tf_b = (0.3, -0.2, 1.1, ...); entry
                 by entry A^T A is within 5.1e-7 of its own size.  NE_TOL =
                 4 x the largest = 1.8e-7.  (A swapped or sign-flipped term of
                 the Jacobian moves entries by 1e-2 and more of the largest.)
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import s2m_case as K  # noqa: E402
import s2m_model as M  # noqa: E402

CORNER_C, SURF_C = 13.7, 6.3
NE_TOL = 1.8e-7
MARGIN_SHARE = 0.02
F = np.float32


def coeff_ratio(coeff, sel, model):
    """err / unit of the points both sides select, with finite coefficients
    and a finite conditioning scale; (ratios, how many compared)."""
    both = np.asarray(sel, bool) & model["sel"] & np.isfinite(coeff).all(axis=1) & np.isfinite(model["unit"])
    err = np.abs(np.asarray(coeff, np.float64)[both] - model["coeff"][both]).max(axis=1)
    return err / model["unit"][both], int(both.sum())


def check_against_model(coeff, sel, model, kind, what):
    """Flags equal outside the margin, coefficients within C * unit."""
    near = model["near"]
    assert near.mean() <= MARGIN_SHARE, (what, near.sum())
    np.testing.assert_array_equal(np.asarray(sel, bool)[~near], model["sel"][~near], err_msg=what)
    r, n = coeff_ratio(coeff, sel, model)
    print(f"{what}: {n} compared, largest |err| / unit {r.max():.3f}, margin points {int(near.sum())}")
    assert n > 0 and r.max() <= (CORNER_C if kind == 0 else SURF_C), (what, r.max())
    return r.max()


def ne_deviation(AtA, AtB, mA, mB):
    return (np.abs(np.asarray(AtA, np.float64).reshape(6, 6) - mA).max() / np.abs(mA).max(),
            np.abs(np.asarray(AtB, np.float64) - mB).max() / np.abs(mB).max())


# ------------------------------------------------------------------ the model itself
def test_model_jacobian_is_the_derivative():
    """The dR/d(angle) matrices against central differences of the residual."""
    rng = np.random.default_rng(1)
    tf = np.array([0.3, -0.2, 1.1, 3.0, -2.0, 0.5])
    p, c = rng.uniform(-30, 30, (50, 3)), rng.normal(size=(50, 3))
    J = M.jacobian(tf, p, c)
    for k in range(6):
        e = np.zeros(6)
        e[k] = 1e-6
        num = ((M.transform(tf + e, p) - M.transform(tf - e, p)) * c).sum(axis=1) / 2e-6
        np.testing.assert_allclose(J[:, k], num, rtol=0, atol=1e-7 * np.abs(J).max())
    np.testing.assert_allclose(M.to_body(tf, M.transform(tf, p)), p, rtol=0, atol=1e-12)
    R = M.rotation(tf)
    np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-15)
    assert np.linalg.det(R) > 0
    # yaw turns x towards y, pitch x towards -z, roll y towards z
    np.testing.assert_allclose(M.rotation([0, 0, np.pi / 2, 0, 0, 0]) @ [1, 0, 0], [0, 1, 0], atol=1e-15)
    np.testing.assert_allclose(M.rotation([0, np.pi / 2, 0, 0, 0, 0]) @ [1, 0, 0], [0, 0, -1], atol=1e-15)
    np.testing.assert_allclose(M.rotation([np.pi / 2, 0, 0, 0, 0, 0]) @ [0, 1, 0], [0, 0, 1], atol=1e-15)


def test_transform_oracle_against_model(oracle_mod):
    c = K.cut()
    for tf, scan in ((c["tf"], c["surf_scan"]), (c["tf_b"], c["surf_scan_b"])):
        w = oracle_mod.s2m_transform(tf, scan)
        w64 = M.transform(tf, scan)
        # five float operations per coordinate on values up to the range
        assert np.abs(w - w64).max() <= 8 * 2.0 ** -24 * np.abs(w64).max()
    # the two scans are the same world points
    np.testing.assert_allclose(M.transform(c["tf_b"], c["surf_scan_b"]), M.transform(c["tf"], c["surf_scan"]),
                               rtol=0, atol=2e-5)


# ------------------------------------------------------------------ cut()
@pytest.mark.parametrize("kind", [0, 1])
def test_cut_covers_every_branch(oracle_mod, kind):
    ref = K.cut_reference(kind)
    n = {k: int(v.sum()) for k, v in ref["branches"].items()}
    print(f"cut kind {kind}: {ref['sel'].size} points, {n}")
    assert n["selected"] >= 50 and n["gated"] >= 20 and n["shape"] >= 20, n
    if kind == 1:
        assert n["weight"] >= 1, n
    else:
        assert n["weight"] == 0, n          # (s2m_case.py: d < 1 once the gate has passed)
    assert sum(n.values()) == ref["sel"].size
    assert K.tie_free(ref["sqd6"])
    assert ref["sel"][0] == 1                # the (1, 1) prefix of the normal-equation cases has a row
    rb = K.cut_reference(kind, b=True)
    assert int(rb["sel"].sum()) >= 50
    # every prefix of the normal-equation cases selects something, and not everything
    assert ref["sel"].size >= 513
    for m in (255, 256, 257, 513):
        assert 0 < int(ref["sel"][:m].sum()) < m


@pytest.mark.parametrize("b", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_cut_oracle_against_model(oracle_mod, kind, b):
    ref = K.cut_reference(kind, b)
    check_against_model(ref["coeff"], ref["sel"], ref["model"], kind, f"cut kind {kind} tf_b {b}")


@pytest.mark.parametrize("b", [False, True])
def test_cut_normal_equations_oracle_against_model(oracle_mod, b):
    c = K.cut()
    tf = c["tf_b" if b else "tf"]
    clouds = [(r["scan"], r["coeff"], r["sel"]) for r in (K.cut_reference(0, b), K.cut_reference(1, b))]
    AtA, AtB, n = oracle_mod.s2m_normal_equations(tf, clouds)
    mA, mB, mn = M.normal_equations(tf, clouds)
    dA, dB = ne_deviation(AtA, AtB, mA, mB)
    print(f"normal equations at {'tf_b' if b else 'tf'}: {n} rows, deviation / largest entry AtA {dA:.2e}, AtB {dB:.2e}; "
          f"elementwise AtA {(np.abs(AtA - mA) / np.abs(mA)).max():.2e}")
    assert n == mn >= 100
    assert dA <= NE_TOL and dB <= NE_TOL
    if b:
        assert min(abs(np.sin(tf[:3])).min(), abs(np.cos(tf[:3])).min()) > 0.15     # no trig factor hides a term


# ------------------------------------------------------------------ clusters()
@pytest.mark.parametrize("kind", [0, 1])
def test_clusters_reach_their_branches(oracle_mod, kind):
    cl = K.clusters()[kind]
    ref = K.clusters_reference(kind)
    names = cl["names"]
    g = len(names)
    assert cl["map"].shape == (5 * g, 3) and cl["query"].shape == (g, 3)
    # the zero transform is exact: world == body bit for bit
    assert ref["world"].tobytes() == cl["query"].tobytes()
    # groups at least 5 m apart, every query's five neighbours its own group
    pts = cl["map"].astype(np.float64)
    gap = np.linalg.norm(pts[:, None] - pts[None], axis=2)
    gap[np.arange(5 * g)[:, None] // 5 == np.arange(5 * g)[None] // 5] = np.inf
    assert gap.min() >= 5.0
    assert (ref["idx"] // 5 == np.arange(g)[:, None]).all()
    identical = np.array([nm == "identical" for nm in names])
    assert K.tie_free(ref["sqd6"], exempt=identical)
    for moved in (False, True):
        assert K.tie_free(K.clusters_reference(kind, moved)["sqd6"], exempt=identical)
    br = ref["branches"]
    for i, nm in enumerate(names):
        want = cl["expect"][nm]
        got = [k for k, v in br.items() if v[i]]
        assert len(got) == 1
        if want == "nan_selected":
            cf = ref["coeff"][i]
            assert got == ["selected"] and np.isnan(cf[:3]).all() and cf[3] == 0, (nm, cf)
        elif want is not None:
            assert got == [want], (nm, got, ref["coeff"][i])
    i = names.index("gate_at_1")
    assert ref["sqd"][i, 4] == F(1.0) and ref["sqd"][names.index("gate_inside"), 4] == F(0.875)
    if kind == 0:
        # axis-aligned lines: diagonal covariance, the Jacobi loop leaves at once, the sort does the work;
        # three axes, three sort patterns -- the coefficient has no component along the line
        for a, ax in enumerate("xyz"):
            for j in range(3):
                cf = ref["coeff"][names.index(f"line_{ax}_{j}")]
                assert cf[a] == 0 and np.abs(cf).max() > 0.1, (ax, j, cf)
        m = ref["model"]
        for nm in names:
            if nm.startswith("ratio_"):
                k = names.index(nm)
                rho = m["l0"][k] / (3 * m["l1"][k])
                assert abs(rho - float(nm[6:])) < 2e-3 and not m["near"][k], (nm, rho)
    else:
        cf = ref["coeff"][names.index("query_at_origin")]
        assert not np.isfinite(cf).any(), cf
        assert ref["model"]["cond"][names.index("collinear")] == np.inf


@pytest.mark.parametrize("moved", [False, True])
@pytest.mark.parametrize("kind", [0, 1])
def test_clusters_oracle_against_model(oracle_mod, kind, moved):
    ref = K.clusters_reference(kind, moved)
    check_against_model(ref["coeff"], ref["sel"], ref["model"], kind, f"clusters kind {kind} moved {moved}")
    if moved:
        w0 = K.clusters()[kind]["query"].astype(np.float64)
        assert np.abs(ref["world"] - w0).max() < 5e-5 and not (ref["world"] == ref["scan"]).all()


# ------------------------------------------------------------------ the float32 rows
def test_exact_sums_bound_holds_for_the_oracle(oracle_mod):
    """The oracle sums the same float rows sequentially in fp64: it must sit
    within the derived bound of the exactly rounded sums (this checks
    s2m_case.rows_f32 / exact_sums / ulp_bound before the device is held to
    them)."""
    c = K.cut()
    rc, rs = K.cut_reference(0), K.cut_reference(1)
    for nc, ns in ((1, 1), (255, 257), (257, 255), (509, 2000)):
        clouds = [(c["corner_scan"][:nc], rc["coeff"][:nc], rc["sel"][:nc]),
                  (c["surf_scan"][:ns], rs["coeff"][:ns], rs["sel"][:ns])]
        AtA, AtB, n = oracle_mod.s2m_normal_equations(c["tf"], clouds)
        S, SB, T, TB, nsel = K.exact_sums(c["tf"], clouds)
        assert n == nsel
        # (the sequential sum of n terms is within n 2^-53 T)
        assert (np.abs(AtA - S) <= K.ulp_bound(S, T) + n * 2.0 ** -53 * T).all()
        assert (np.abs(AtB - SB) <= K.ulp_bound(SB, TB) + n * 2.0 ** -53 * TB).all()
        assert np.abs(S).max() > 0
