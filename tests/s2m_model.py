"""What LIO-SAM's scan-to-map measurement model means, in numpy float64.

Written from the geometry, not from the kernels' expressions (those are
restated line for line by oracle/lio_s2m_oracle.cpp, so a transcription slip
made once and copied would pass the bit-exact tests): a rotation matrix, a
line through a centroid along the top eigenvector (np.linalg.eigh), a
least-squares plane (np.linalg.lstsq), and the Jacobian of the residual from
the three dR/d(angle) matrices.  Inputs are the float values the device used
(world or body points, the five neighbours, the fifth squared distance),
widened to double.

    transform   w = Rz(yaw) Ry(pitch) Rx(roll) p + t
    corner      centroid c and covariance of the five neighbours; accepted when
                lambda0 > 3 lambda1; d = distance of w to the line through c
                along the top eigenvector, g = its unit gradient, s = 1 - 0.9 d;
                coefficients (s g, s d), selected when s > 0.1
    surf        x = lstsq(A x = -1), n = x / |x|, pd = 1 / |x|; accepted when
                every neighbour has |n.q + pd| <= 0.2; pd2 = n.w + pd,
                s = 1 - 0.9 |pd2| / sqrt(|w|); coefficients (s n, s pd2),
                selected when s > 0.1
    rows        J_i = d/d(roll, pitch, yaw, x, y, z) of c_i . (R p_i + t);
                AtA = sum J^T J, AtB = -sum J^T c_i.w

Both kinds need the fifth neighbour nearer than 1 m (sqd[4] < 1).

A point is *near a threshold* where a float evaluation may legitimately fall
on the other side: lambda0 within EIG of 3 lambda1 (relative to lambda0), s
within S of 0.1, a neighbour residual within RESID of 0.2, sqd[4] within GATE
of 1.  Only thresholds the point actually reaches count (a gated point has no
eigenvalues to be near).  Flag comparisons skip these points.

Conditioning: `unit` is the float32 error scale of a point's coefficients,
2^-24 times
    corner   (1 + max(|w|, |c|)) (1 + 1 / d)   -- the direction of w - foot
             divides by d, the coordinates carry 2^-24 of their size
    surf     cond(A) (1 + |w - c|)             -- the 5 x 3 solve, and the
             lever of the normal's error at the query
inf where d == 0 or A is rank deficient (cond above 1e6): nothing can be
said there, and nothing is compared.
"""
import numpy as np

D = np.float64
EIG, S, RESID, GATE = 1e-3, 1e-3, 1e-3, 1e-5
EPS32 = 2.0 ** -24


def rot_parts(roll, pitch, yaw):
    cr, sr, cp, sp, cy, sy = np.cos(roll), np.sin(roll), np.cos(pitch), np.sin(pitch), np.cos(yaw), np.sin(yaw)
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]], D)
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]], D)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]], D)
    dRx = np.array([[0, 0, 0], [0, -sr, -cr], [0, cr, -sr]], D)
    dRy = np.array([[-sp, 0, cp], [0, 0, 0], [-cp, 0, -sp]], D)
    dRz = np.array([[-sy, -cy, 0], [cy, -sy, 0], [0, 0, 0]], D)
    return Rx, Ry, Rz, dRx, dRy, dRz


def rotation(tf):
    """R = Rz(yaw) Ry(pitch) Rx(roll) of tf = (roll, pitch, yaw, x, y, z)."""
    tf = np.asarray(tf, D)
    Rx, Ry, Rz, *_ = rot_parts(*tf[:3])
    return Rz @ Ry @ Rx


def transform(tf, body):
    tf = np.asarray(tf, D)
    return np.asarray(body, D).reshape(-1, 3) @ rotation(tf).T + tf[3:6]


def to_body(tf, world):
    """The body points that tf maps onto world (fp64; the caller rounds)."""
    tf = np.asarray(tf, D)
    return (np.asarray(world, D).reshape(-1, 3) - tf[3:6]) @ rotation(tf)


def _finish(gate, accept, s, coeff, gate_near, shape_near, unit):
    with np.errstate(invalid="ignore"):
        sel = gate & accept & (s > 0.1)
        s_near = np.abs(s - 0.1) < S
    near = gate_near | (gate & (shape_near | (accept & s_near)))
    coeff = np.where((gate & accept)[:, None], coeff, 0.0)
    return dict(coeff=coeff, sel=sel, near=near, gate=gate, accept=gate & accept, s=s, unit=unit)


def corner(world, nb, sqd4):
    """world (n, 3), nb (n, 5, 3), sqd4 (n,): the float values, any dtype."""
    w, nb, sqd4 = np.asarray(world, D).reshape(-1, 3), np.asarray(nb, D).reshape(-1, 5, 3), np.asarray(sqd4, D)
    gate = sqd4 < 1.0
    c = nb.mean(axis=1)
    dl = nb - c[:, None, :]
    cov = np.einsum("nji,njk->nik", dl, dl) / 5.0
    lam, vec = np.linalg.eigh(cov)                       # ascending
    l0, l1, v = lam[:, 2], lam[:, 1], vec[:, :, 2]
    accept = l0 > 3.0 * l1
    r = w - c
    perp = r - (r * v).sum(axis=1)[:, None] * v
    d = np.linalg.norm(perp, axis=1)
    with np.errstate(all="ignore"):
        g = perp / d[:, None]
        s = 1.0 - 0.9 * d
        coeff = np.concatenate([s[:, None] * g, (s * d)[:, None]], axis=1)
        unit = EPS32 * (1.0 + np.maximum(np.linalg.norm(w, axis=1), np.linalg.norm(c, axis=1))) * (1.0 + 1.0 / d)
    out = _finish(gate, accept, s, coeff, np.abs(sqd4 - 1.0) < GATE, np.abs(l0 - 3.0 * l1) < EIG * l0, unit)
    out.update(d=d, l0=l0, l1=l1)
    return out


def surf(world, nb, sqd4):
    w, nb, sqd4 = np.asarray(world, D).reshape(-1, 3), np.asarray(nb, D).reshape(-1, 5, 3), np.asarray(sqd4, D)
    n_pts = w.shape[0]
    gate = sqd4 < 1.0
    x = np.zeros((n_pts, 3), D)
    cond = np.full(n_pts, np.inf, D)
    rhs = -np.ones(5, D)
    for i in range(n_pts):
        if not np.isfinite(nb[i]).all():
            continue
        x[i], _, _, sv = np.linalg.lstsq(nb[i], rhs, rcond=None)
        if sv[2] > 0:
            cond[i] = sv[0] / sv[2]
    cond[cond > 1e6] = np.inf
    with np.errstate(all="ignore"):
        nrm = np.linalg.norm(x, axis=1)
        n = x / nrm[:, None]
        pd = 1.0 / nrm
        res = np.abs((nb * n[:, None, :]).sum(axis=2) + pd[:, None])
        accept = (res <= 0.2).all(axis=1)
        pd2 = (n * w).sum(axis=1) + pd
        s = 1.0 - 0.9 * np.abs(pd2) / np.sqrt(np.linalg.norm(w, axis=1))
        coeff = np.concatenate([s[:, None] * n, (s * pd2)[:, None]], axis=1)
        c = nb.mean(axis=1)
        unit = EPS32 * cond * (1.0 + np.linalg.norm(w - c, axis=1))
        shape_near = (np.abs(res - 0.2) < RESID).any(axis=1)
    out = _finish(gate, accept, s, coeff, np.abs(sqd4 - 1.0) < GATE, shape_near, unit)
    out.update(pd2=pd2, res=res, cond=cond)
    return out


def coeffs(kind, world, nb, sqd4):
    return (corner if kind == 0 else surf)(world, nb, sqd4)


def jacobian(tf, body, normal):
    """(n, 6): d/d(roll, pitch, yaw, x, y, z) of normal_i . (R(tf) body_i + t)."""
    tf = np.asarray(tf, D)
    p, c = np.asarray(body, D).reshape(-1, 3), np.asarray(normal, D).reshape(-1, 3)
    Rx, Ry, Rz, dRx, dRy, dRz = rot_parts(*tf[:3])
    J = np.empty((p.shape[0], 6), D)
    for k, dR in enumerate((Rz @ Ry @ dRx, Rz @ dRy @ Rx, dRz @ Ry @ Rx)):
        J[:, k] = ((p @ dR.T) * c).sum(axis=1)
    J[:, 3:] = c
    return J


def normal_equations(tf, clouds):
    """clouds: [(body (n, 3), coeff (n, 4), sel (n,))].  fp64 (AtA (6, 6), AtB (6,), nsel)."""
    AtA, AtB, nsel = np.zeros((6, 6), D), np.zeros(6, D), 0
    for body, coeff, sel in clouds:
        m = np.asarray(sel, bool)
        if not m.any():
            continue
        cf = np.asarray(coeff, D).reshape(-1, 4)[m]
        J = jacobian(tf, np.asarray(body, D).reshape(-1, 3)[m], cf[:, :3])
        AtA += J.T @ J
        AtB -= J.T @ cf[:, 3]
        nsel += int(m.sum())
    return AtA, AtB, nsel
