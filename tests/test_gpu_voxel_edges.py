"""GPU: the scan VoxelGrid (k_vg_bbox, k_vg_geom, k_vg_keys, the sort,
k_vg_heads, k_vg_centroids; Esekf.downsample_scan) against the oracle's
pcl::VoxelGrid restatement, bit-exact, where such kernels go wrong:
coordinates on the voxel faces and one ulp either side, a voxel whose sum is
long enough for the order of the additions to show, sizes around the 256-thread
block, non-finite rows, and the two sides of PCL's index-overflow test (on
overflow the output is the input, non-finite rows included)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_map import _box_edges  # noqa: E402
from test_gpu_parity import L  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def kf(L):
    from agi_lidar_slam_amd.esekf import Esekf
    k = Esekf(max_points=4096)
    yield k
    k.close()


def _down(kf, raw, leaf):
    n = kf.downsample_scan(raw, leaf)
    got = kf.feats_down_body()
    assert got.shape == (n, 3)
    return got


def _same(got, want):
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("leaf", [0.5, 0.2, 0.3])
def test_points_on_voxel_faces(L, oracle_mod, kf, leaf):
    """k * leaf in float, the floats next to it, and -0.0, for k in -40..40:
    floor(p * (1 / leaf)) decides the voxel, and for 0.2 and 0.3 the product
    rounds across an integer for some k."""
    rng = np.random.default_rng(int(leaf * 100))
    edges = np.concatenate([_box_edges(leaf, np.arange(-40, 41)), np.array([-0.0], F)])
    near = np.concatenate([_box_edges(leaf, np.arange(-1, 1)), np.array([-0.0], F)])
    # three clouds of 1,000: one axis over every face, the other two on the
    # faces around zero, so that voxels hold several points
    raw = np.empty((3000, 3), F)
    for a in range(3):
        for b in range(3):
            pool, half = (edges, 40 * leaf) if a == b else (near, leaf)
            raw[1000 * b:1000 * (b + 1), a] = np.where(rng.random(1000) < 0.7, rng.choice(pool, 1000),
                                                       rng.uniform(-half, half, 1000))
    raw[:3] = [[-0.0, 0.0, -0.0], [0.0, -0.0, 0.0], [-0.0, -0.0, -0.0]]
    raw = raw[rng.permutation(3000)]
    inv = F(1.0) / F(leaf)
    on_int = (edges * inv) == np.floor(edges * inv)
    assert on_int.sum() > 40 and (~on_int).sum() > 80 and np.signbit(raw).any()
    want = oracle_mod.voxel_grid(raw, leaf)
    assert 300 < want.shape[0] < 2000
    _same(_down(kf, raw, leaf), want)


def long_sum_cloud():
    """3,000 points of one 0.5 m voxel among 50 voxels of one point each, in
    shuffled order; returns (cloud, rows of the big voxel in input order)."""
    rng = np.random.default_rng(5)
    big = (np.array([10.0, -7.5, 3.0]) + rng.uniform(0.001, 0.499, (3000, 3))).astype(F)
    ones = (np.array([20.0, 0.0, 0.0]) + 0.5 * np.arange(50)[:, None] * np.array([1.0, 1.0, 0.0])
            + rng.uniform(0.01, 0.49, (50, 3))).astype(F)
    raw = np.concatenate([big, ones])
    tag = np.concatenate([np.ones(3000, bool), np.zeros(50, bool)])
    p = rng.permutation(3050)
    return np.ascontiguousarray(raw[p]), tag[p]


def test_long_sum_is_sequential(L, oracle_mod, kf):
    """CentroidPoint adds the points one by one in float: the centroid of a
    3,000-point voxel is the sequential sum in ascending input index divided
    by the count -- a pairwise or per-lane partial sum gives other bits."""
    raw, tag = long_sum_cloud()
    seq = np.add.accumulate(raw[tag], axis=0, dtype=F)[-1]
    cols = [np.ascontiguousarray(raw[tag][:, a]) for a in range(3)]
    pair = np.array([c.sum(dtype=F) for c in cols], F)   # numpy's pairwise sum of a contiguous column
    lanes = np.array([np.add.accumulate(c.reshape(-1, 4), axis=0, dtype=F)[-1].sum(dtype=F) for c in cols], F)
    assert (seq != pair).all() and (seq != lanes).all()
    cen = seq / F(3000)
    got = _down(kf, raw, 0.5)
    assert got.shape[0] == 51
    hit = np.nonzero((np.abs(got - cen) < 0.01).all(axis=1))[0]
    assert hit.size == 1
    _same(got[hit[0]], cen)
    _same(got, oracle_mod.voxel_grid(raw, 0.5))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257])
def test_sizes_around_a_block(L, oracle_mod, kf, n):
    rng = np.random.default_rng(n)
    raw = rng.uniform(-3, 3, (n, 3)).astype(F)
    want = oracle_mod.voxel_grid(raw, 0.5)
    assert 1 <= want.shape[0] <= n
    _same(_down(kf, raw, 0.5), want)
    # n copies of one point: one voxel, the sequential sum of n equal terms
    one = np.tile(np.array([[1.3, -2.7, 0.1]], F), (n, 1))
    want = oracle_mod.voxel_grid(one, 0.5)
    assert want.shape == (1, 3)
    _same(want[0], np.add.accumulate(one, axis=0, dtype=F)[-1] / F(n))
    _same(_down(kf, one, 0.5), want)


def test_non_finite_rows(L, oracle_mod, kf):
    """NaN and +-inf rows are no part of the box, of any voxel or of the count."""
    rng = np.random.default_rng(9)
    raw = rng.uniform(-5, 5, (1000, 3)).astype(F)
    bad = rng.choice(1000, 200, replace=False)
    raw[bad[:60], 0] = np.nan
    raw[bad[60:110], 1] = np.inf
    raw[bad[110:160], 2] = -np.inf
    raw[bad[160:]] = [np.inf, np.nan, -np.inf]
    want = oracle_mod.voxel_grid(raw, 0.5)
    keep = np.isfinite(raw).all(axis=1)
    _same(want, oracle_mod.voxel_grid(raw[keep], 0.5))
    _same(_down(kf, raw, 0.5), want)
    # all rows but one non-finite, the finite one in the middle and last
    for at in (137, 299):
        lone = np.full((300, 3), np.nan, F)
        lone[::3, 1] = np.inf
        lone[1::3, 2] = -np.inf
        lone[at] = [4.25, -1.5, 0.75]
        got = _down(kf, lone, 0.5)
        _same(got, lone[at:at + 1])
        _same(got, oracle_mod.voxel_grid(lone, 0.5))


def test_index_overflow_threshold(L, oracle_mod, kf):
    """PCL voxelises while dx * dy * dz <= INT32_MAX (int64 product of the
    per-axis cell counts) and otherwise returns its input as it is."""
    nan = np.nan
    fits = np.array([[0, 0, 0], [1289.5, 1289.5, 1289.5]], F)            # 1290^3 = 2,146,689,000
    over = np.array([[0, 0, 0], [nan, 1.0, 2.0], [1290.5, 1290.5, 1290.5]], F)   # 1291^3 = 2,151,685,171
    assert 1290 ** 3 <= 2 ** 31 - 1 < 1291 ** 3
    line_fits = np.array([[0, 0, 0], [0, 0, 2147483520.0]], F)           # 2147483521 cells along z
    line_over = np.array([[0, 0, 0], [0, 0, 2147483648.0]], F)           # 2147483649
    assert float(line_fits[1, 2]) == 2147483520.0 and float(line_over[1, 2]) == 2147483648.0
    for raw, passed in ((fits, False), (over, True), (line_fits, False), (line_over, True)):
        want = oracle_mod.voxel_grid(raw, 1.0)
        if passed:
            _same(want, raw)            # the input, the NaN row in place
        else:
            _same(want, raw[np.isfinite(raw).all(axis=1)])   # one point per voxel, in index order
        _same(_down(kf, raw, 1.0), want)
        _same(oracle_mod.voxel_grid(raw, 1.0, pcl_order=True), want)
