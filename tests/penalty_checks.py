"""Float64 checks of volume penalisation, from the definition -- TEST
INFRASTRUCTURE ONLY.  HELPER MODULE, not a test.

The momentum equation of cell i gains  -V s (u - u_t),  s = sigma + forch |u|,
implicit in u and diagonal:

    diagonal          D_i = (the unpenalised diagonal) + V_i s_i      in prepare and in the assembly
    d_p               V_i / D_i   with prepare's penalised diagonal
    right-hand side   b_i = (the unpenalised right-hand side) + V_i s_i (scale u_t,i)
    everything else   unchanged: every off-diagonal momentum coefficient has the
                      BITS of a plain assembly of the same state and fluxes

and |u| is that of the iterate, the state prepare and the assembly read (not
u_old).  Everything else of the discretisation is tests/flow_checks.py's, which
writes the time coefficient of every diagonal as c.a_t(V).  So the first two
checks ARE flow_checks' (check_d_p: d_p of every cell; check_matrix_entries:
every stored entry of both matrices, the momentum diagonals among them),
evaluated with a_t(V) + V s in place of a_t(V); the third is flow_checks'
rhs64 plus the term.

Bounds, as k * eps32 * sum |terms| like the siblings: flow_checks' own, 16 eps32
= 32 half-ulp roundings of the magnitudes of an entry's terms (cell_tol, more
for a cell of many faces).  The penalty adds one positive term V s to a
diagonal, which enters the sum of magnitudes as itself, and carries at most 8
roundings of its own (x*x, y*y, their sum, the root, the product with forch, the
sum with sigma, the product with V, the addition to the diagonal): 8 half-ulps
of a term whose magnitude the bound counts 32 times.  The right-hand side's
term V s (scale u_t) carries 10 (the same, the scaling, the product) and enters
the magnitudes as V s |scale u_t|.  The bounds stand as they are.

WRONG: what a deliberately wrong check would use; a wrong restatement fails the
right checks, and the right restatement fails these (tests/test_penalty.py).
"""
import contextlib

import numpy as np

from tests import flow_checks as fc

EPS32 = fc.EPS32
WRONG = ("no_prepare", "unscaled", "u_old")


def _f32(x):
    return np.asarray(x, np.float32).astype(np.float64)


def coefficient(st, g, sigma, forch, wrong=()):
    """V s [N] in float64 from the float32 fields and the iterate"""
    s = _f32(sigma)
    if forch is not None:
        u = st.u_old if "u_old" in wrong else st.u
        s = s + _f32(forch) * np.hypot(u[:, 0], u[:, 1])
    return g.vol * s


@contextlib.contextmanager
def _with_penalty(pen):
    """for the duration: flow_checks' a_t(V) is a_t(V) + V s (pen None: as it is)"""
    plain = fc.Constants.a_t
    if pen is not None:
        fc.Constants.a_t = lambda self, vol: plain(self, vol) + pen
    try:
        yield
    finally:
        fc.Constants.a_t = plain


def check_d_p(st, sigma, forch, wrong=()):
    g = fc.Geometry(st.arrays)
    with _with_penalty(None if "no_prepare" in wrong else coefficient(st, g, sigma, forch, wrong)):
        return fc.check_d_p(st)["worst"]


def check_matrix(st, sigma, forch, wrong=()):
    g = fc.Geometry(st.arrays)
    with _with_penalty(coefficient(st, g, sigma, forch, wrong)):
        return fc.check_matrix_entries(st)["worst"]


def check_rhs(st, sigma, forch, target, scale, wrong=()):
    c = fc.Constants(st.constants)
    sc = 1.0 if "unscaled" in wrong else float(np.float32(scale))
    variants = []
    for g in fc._geometries(st, ()):
        b, m = fc.rhs64(g, c, st)
        if target is not None:
            pen = coefficient(st, g, sigma, forch, wrong)
            t = sc * _f32(target).reshape(-1, 2)
            b[:, :2] += pen[:, None] * t
            m[:, :2] += pen[:, None] * np.abs(t)
        variants.append((st.rhs - b.reshape(-1), np.repeat(g.cell_tol, 3) * m.reshape(-1)))
    return fc._judge("check_rhs with a penalty", variants,
                     lambda e: f"row {e} (cell {e // 3}, {'uvp'[e % 3]}): {st.rhs[e]:.9e}")


def check_off_diagonals(st, st_plain):
    """every stored entry of a momentum row except its own diagonal: the bits of the plain
    assembly of the same state; returns the entries compared"""
    assert np.array_equal(st.u, st_plain.u) and np.array_equal(st.p, st_plain.p)
    assert np.array_equal(st.flux.astype(np.float32).view(np.uint32), st_plain.flux.astype(np.float32).view(np.uint32))
    row, col = fc._stored_coupled(st.mesh, len(st.coupled))
    sel = (row % 3 != 2) & (row != col)
    a = st.coupled[sel].astype(np.float32).view(np.uint32)
    b = st_plain.coupled[sel].astype(np.float32).view(np.uint32)
    bad = a != b
    assert not np.any(bad), (f"f64 check_off_diagonals: A[{row[sel][bad][0]}, {col[sel][bad][0]}] differs from the "
                             f"plain assembly; {int(bad.sum())} entries")
    # and the diagonals do differ where the cell is penalised: the comparison is not vacuous
    d = (row % 3 != 2) & (row == col)
    assert np.any(st.coupled[d] != st_plain.coupled[d])
    return int(sel.sum())


def check_all(st, st_plain, sigma, forch, target, scale, wrong=()):
    """st, st_plain: captured flow_checks.FlowState of the penalised and of a plain
    solver on the same state.  Returns the worst error / bound per check."""
    return dict(d_p=check_d_p(st, sigma, forch, wrong), matrix=check_matrix(st, sigma, forch, wrong),
                rhs=check_rhs(st, sigma, forch, target, scale, wrong),
                off_diagonal_entries=check_off_diagonals(st, st_plain))


def force64(arrays, u, sigma, forch, target, scale, centre, box=None):
    """(values [5], magnitudes [5]) of penalty_force from the definition, numpy's pairwise sums"""
    d = np.float64
    u = np.asarray(u, d).reshape(-1, 2)
    s = _f32(sigma)
    if forch is not None:
        s = s + _f32(forch) * np.hypot(u[:, 0], u[:, 1])
    m = _f32(arrays["cell_vol"]) * s
    t = np.zeros_like(u) if target is None else float(np.float32(scale)) * _f32(target).reshape(-1, 2)
    cx, cy = np.asarray(arrays["cell_cx"], d), np.asarray(arrays["cell_cy"], d)
    inside = np.ones(len(s), bool)
    if box is not None:
        x0, y0, x1, y1 = box
        inside = (cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1)
    fx, fy = m * (u[:, 0] - t[:, 0]), m * (u[:, 1] - t[:, 1])
    ax, ay = m * (np.abs(u[:, 0]) + np.abs(t[:, 0])), m * (np.abs(u[:, 1]) + np.abs(t[:, 1]))
    rx, ry = cx - centre[0], cy - centre[1]
    val = [fx, fy, rx * fy - ry * fx, fx * t[:, 0] + fy * t[:, 1], (s > 0).astype(d)]
    mag = [ax, ay, np.abs(rx) * ay + np.abs(ry) * ax, ax * np.abs(t[:, 0]) + ay * np.abs(t[:, 1]), np.zeros(len(s))]
    return np.array([v[inside].sum() for v in val]), np.array([v[inside].sum() for v in mag])


def force_bound(mag, n):
    """A term is formed in float64 with at most 12 roundings (the root's chain, the products,
    the differences) and a sum of n terms in a tree of depth log2 n adds log2 n more: (12 +
    ceil(log2 n)) * 2^-53 * sum |terms|, doubled for the comparison value's own sum."""
    return 2.0 * (12.0 + np.ceil(np.log2(max(n, 2)))) * 2.0 ** -53 * mag


def check_force(got, arrays, u, sigma, forch, target, scale, centre, box=None):
    """got: ((Fx, Fy), torque, power, cells)"""
    val, mag = force64(arrays, u, sigma, forch, target, scale, centre, box)
    g = np.array([got[0][0], got[0][1], got[1], got[2], float(got[3])])
    return fc._judge("check_force", [(g - val, force_bound(mag, len(np.asarray(sigma))))],
                     lambda i: f"sum {i}: {g[i]:.17e} against {val[i]:.17e}")
