"""The fixture of tests/test_gpu_livox_pass.py: the cut around one wall corner
that tests/lego_map_case.py makes, used as plain geometry (no frame
conversion beyond the one the cut already carries) and moved so that the
wall corner stands at x = 25 m, z = -25 m: the maps straddle the cube boundary
at x = 25 and reach into cubes of negative coordinates (the `--` branch of
the cube index).  Computed once per process.

Tie cap: for EVERY query of both scans at the evaluation pose the fixture
asserts that no two of the K + 1 nearest float distances are equal (so the
5th != 6th and the 8th != 9th) and that no K-th distance lies within 1 ulp of
its gate.  No query is left out."""
import functools

import numpy as np

import lego_map_case as K
import livox_map_model as M

F = np.float32
SIZES = (1, 7, 8, 9, 63, 64, 65, 257, 1500)
LEAF_SURF = 1.0e-3      # the scan grid keeps every point apart: the sizes above are the scans' sizes


@functools.lru_cache(maxsize=None)
def cut():
    c = K.cut()
    ctr = c["surf_map"].mean(axis=0)
    d = np.array([25.0 - ctr[0], 0.0, -25.0 - ctr[2]], F)
    tf = c["tf_eval"].copy()
    tf[3:] = tf[3:] + d
    return dict(corner_map=(c["corner_map"] + d).astype(F), surf_map=(c["surf_map"] + d).astype(F),
                corner_scan=c["corner_scan"], surf_scan=c["surf_scan"], tf=tf.astype(F))


@functools.lru_cache(maxsize=None)
def maps():
    """The two maps as the cube store holds them after one unfiltered update at
    the zero pose, and the cube list (every non-empty cube, ascending) whose
    concatenation is laserCloud*FromMap."""
    from oracle import oracle as O
    O.build()
    c = cut()
    cm = M.CubeMap(O.voxel_grid)
    cm.update(np.zeros(6, F), c["corner_map"], c["surf_map"], [])
    valid = sorted(set(np.nonzero(cm.sizes(0))[0]) | set(np.nonzero(cm.sizes(1))[0]))
    valid = [int(v) for v in valid]
    out = dict(valid=valid, maps=[cm.concat(0, valid), cm.concat(1, valid)])
    # the placement the docstring promises
    ijk = [(v % M.W - 10, v // M.W % M.H - 5, v // (M.W * M.H) - 10) for v in valid]
    assert {i for i, _, _ in ijk} >= {0, 1} and min(k for _, _, k in ijk) < 0, ijk
    return out


@functools.lru_cache(maxsize=None)
def reference(kind, n):
    """The model on the first n points of the kind's scan: the scan as fed
    (the surf scan through the VoxelGrid of LEAF_SURF), world points, K + 1
    neighbours, coefficients, flags and branch counts."""
    from oracle import oracle as O
    O.build()
    c, mp = cut(), maps()["maps"][kind]
    scan = c["corner_scan"][:n] if kind == 0 else np.ascontiguousarray(O.voxel_grid(c["surf_scan"][:n], LEAF_SURF), F)
    world = M.to_map(c["tf"], scan)
    k1 = M.KNN[kind] + 1
    if k1 <= 8:
        idx, sqd = O.Tree(mp).knn(world, k1)
    else:
        # the oracle's tree answers up to k = 8: the eight come from it, the
        # ninth distance (for the tie cap only) from a plain float32 scan of
        # the map, which must agree with the tree on the first eight
        idx8, sqd8 = O.Tree(mp).knn(world, 8)
        d = world[:, None, :] - mp[None, :, :]
        d2 = (d[:, :, 0] * d[:, :, 0] + d[:, :, 1] * d[:, :, 1]) + d[:, :, 2] * d[:, :, 2]
        order = np.argsort(d2, axis=1, kind="stable")[:, :k1]
        sq9 = np.take_along_axis(d2, order, 1)
        assert sq9.dtype == F and np.array_equal(sq9[:, :8], sqd8)
        idx, sqd = np.concatenate([idx8, order[:, 8:].astype(np.int32)], 1), np.concatenate([sqd8, sq9[:, 8:]], 1)
    assert M.tie_free(kind, sqd), "a query ties: change the cut"
    assert M.gate_clear(kind, sqd), "a K-th distance within 1 ulp of the gate: change the cut"
    coeff, sel, near, stats = M.coeffs(kind, world, mp, idx, sqd)
    return dict(scan=scan, world=world, idx=idx, sqd=sqd, coeff=coeff, sel=sel, near=near, stats=stats)
