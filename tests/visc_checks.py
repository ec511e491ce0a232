"""Float64 checks of variable viscosity, from the discretisation -- TEST
INFRASTRUCTURE ONLY.  HELPER MODULE, not a test.

The momentum diffusion through face f between cells i and o with a viscosity
per cell is  nu_f A (u_o - u_i) / d  with the face viscosity

    nu_f = (mu_i + mu_o) / 2      interior face
    nu_f = mu_i                   boundary face (the value at the wall is the cell's)

and everything else of the discretisation is tests/flow_checks.py's, which
writes every diffusion coefficient as c.nu * A / dist.  So the checks here ARE
flow_checks' (check_d_p, check_matrix_entries, check_rhs: every stored entry
of both matrices, d_p of every cell, the complete right-hand side), evaluated
with c.nu an array over the cell-face incidences of Geometry.sides() instead
of one number:

    interior entry   A_uu[i,o] = -nu_f A / dist_n + min(F_out, 0)
    diagonal         a_t + sum nu_f A / dist_n + max(F_out, 0)
    d_p              V / (a_t + sum nu_f A / dist_c + max(F_out, 0))
    right-hand side  ... + sum over inlet faces (nu_f A / dist_n + max(-F_out, 0)) u_b

Bounds: flow_checks' own (16 eps32 = 32 half-ulps of the magnitudes of an
entry's terms, derived there).  The face viscosity adds one float32 rounding
to a diffusion coefficient (the sum mu_i + mu_o; the factor 0.5 is exact, the
float64 mean of two float32 values is exact): an interior entry then carries
about 7 half-ulp roundings of its 32, so the bounds stand as they are.

Two checks of their own:
  symmetry   the diffusion part of the matrix is symmetric bit for bit.  An
             entry is fl(-diff + min(F_out, 0)) and the two sides of a face see
             F_out and -F_out: on the side with F_out >= 0 the entry is -diff
             itself, so the other side's entry must be fl(that entry + its own
             F_out) exactly, in float32.
  wall force the viscous force on the force region's wall faces is sum mu_i u A /
             dist_c with the CELL's viscosity, within 16 eps32 of the sum of the
             magnitudes (bcvel_checks.check_wall_sums' count).

WRONG: what a deliberately wrong check would use; a wrong restatement fails the
right checks, and the right restatement fails these (tests/test_visc.py).
"""
import contextlib

import numpy as np

from tests import flow_checks as fc

EPS32 = fc.EPS32
WRONG = ("harmonic", "boundary_other", "uniform")


def face_viscosity(g, mu, wrong=()):
    """nu_f [F] in float64 from the float32 field"""
    mu = np.asarray(mu, np.float32).astype(np.float64)
    a, b = mu[g.own], mu[g.nb]
    mean = 2.0 * a * b / (a + b) if "harmonic" in wrong else 0.5 * (a + b)
    bnd = mu[np.minimum(g.own + 1, g.N - 1)] if "boundary_other" in wrong else a
    return np.where(g.internal, mean, bnd)


@contextlib.contextmanager
def _per_face(mu, wrong):
    """for the duration: flow_checks' checks read c.nu as an array over the
    incidences of Geometry.sides(), set by that call on the Constants the check made"""
    plain = fc.Constants
    held = {}

    def constants(c, w=()):
        held["c"] = plain(c, w)
        return held["c"]

    sides = fc.Geometry.sides

    def sides_with_nu(g):
        out = sides(g)
        if "uniform" not in wrong:
            held["c"].nu = face_viscosity(g, mu, wrong)[out[1]]
        return out

    fc.Constants, fc.Geometry.sides = constants, sides_with_nu
    try:
        yield
    finally:
        fc.Constants, fc.Geometry.sides = plain, sides


def check_symmetry(st):
    """bit for bit, over every interior face; returns the faces checked"""
    g = fc.Geometry(st.arrays)
    row, col = fc._stored_coupled(st.mesh, len(st.coupled))
    n3 = 3 * g.N
    keys = row * n3 + col
    order = np.argsort(keys)

    def entry(i, j):  # A_uu[i, j] as stored, float32
        k = (3 * i) * n3 + 3 * j
        pos = np.searchsorted(keys[order], k)
        assert np.array_equal(keys[order][pos], k)
        return st.coupled[order[pos]].astype(np.float32)

    f = np.nonzero(g.internal)[0]
    o, n = g.own[f], g.nb[f]
    flux = st.flux[f].astype(np.float32)  # out of the owner; the neighbour sees its negation
    a_on, a_no = entry(o, n), entry(n, o)
    up = flux >= 0  # the owner's entry is -diff itself
    pure = np.where(up, a_on, a_no)
    other = np.where(up, a_no, a_on)
    want = (pure + np.where(up, -flux, flux)).astype(np.float32)
    bad = want.view(np.uint32) != other.view(np.uint32)
    assert not np.any(bad), (f"f64 check_symmetry: face {f[bad][0]} (cells {o[bad][0]}, {n[bad][0]}): "
                             f"{other[bad][0]!r} != {want[bad][0]!r}; {int(bad.sum())} faces")
    return len(f)


def check_wall_force(st, mu, box, force_viscous, wrong=()):
    g = fc.Geometry(st.arrays)
    a = st.arrays
    x0, y0, x1, y1 = box
    x, y = a["face_cx"], a["face_cy"]
    f = np.nonzero((g.kind == fc.WALL) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1))[0]
    assert len(f) > 0
    if "uniform" in wrong:
        nu = np.full(len(f), fc.Constants(st.constants).nu)
    else:
        nu = face_viscosity(g, mu, wrong)[f]
    o = g.own[f]
    k = nu * g.area[f] / g.dist_c[f]
    worst = 0.0
    for comp in (0, 1):
        val, mag = (k * st.u[o, comp]).sum(), (k * np.abs(st.u[o, comp])).sum()
        worst = max(worst, fc._judge(f"check_wall_force [{'xy'[comp]}]", [(np.array([force_viscous[comp] - val]),
                                                                           np.array([16 * EPS32 * mag]))],
                                     lambda i: f"{force_viscous[comp]:.12e} against {val:.12e}"))
    return worst


def check_model(mesh, s, par, kind):
    """s: a solver with the model set and evaluated on its current state.  The shear rate
    against gdot = sqrt(2 ux^2 + 2 vy^2 + (uy + vx)^2) of flow_checks' float64 gradients: gdot
    is a norm of the gradient with |d gdot / d g_ij| <= sqrt 2, so its error is at most 2 times
    the sum of the four gradients' own bounds (flow_checks.check_gradients': cell_tol times the
    magnitudes) plus 8 eps32 gdot for its own six f32 operations and the root.  Then mu of the
    unclamped cells against the model evaluated with math.pow on the solver's own float32
    gdot, within 4 eps32 (one rounding to float32; pow_det's error is 1e-14)."""
    import math

    class _St:
        pass

    st = _St()
    st.u = np.asarray(s.get_u(), np.float64).reshape(-1, 2)
    st.p = np.asarray(s.get_p(), np.float64)
    g = fc.Geometry(mesh.arrays())
    c = fc.Constants(s.constants)
    gr = fc.gradients64(g, c, st)
    (ux, uy, mux, muy), (vx, vy, mvx, mvy) = gr["u"], gr["v"]
    gdot64 = np.sqrt(2.0 * ux * ux + 2.0 * vy * vy + (uy + vx) ** 2)
    gdot = np.asarray(s.shear_rate(), np.float64)
    bound = 2.0 * g.cell_tol * (mux + muy + mvx + mvy) + 8.0 * EPS32 * gdot64
    fc._judge("check_model shear rate", [(gdot - gdot64, bound)], lambda i: f"cell {i}: {gdot[i]:.9e}")
    q = {k: float(np.float32(v)) for k, v in par.items()}
    if kind == "power_law":
        m = np.array([q["K"] * math.pow(max(x, q["gamma_min"]), q["n"] - 1.0) for x in gdot])
    else:
        m = np.array([q["mu_inf"] + (q["mu0"] - q["mu_inf"]) * math.pow(1.0 + (q["lam"] * x) ** 2, (q["n"] - 1.0) / 2.0)
                      for x in gdot])
    want = np.minimum(np.maximum(m, q["mu_min"]), q["mu_max"])
    mu = np.asarray(s.viscosity_field(), np.float64)
    fc._judge("check_model viscosity", [(mu - want, 4.0 * EPS32 * want)], lambda i: f"cell {i}: {mu[i]:.9e}")


def check_all(st, mu, box, force_viscous, wrong=()):
    """st: a captured flow_checks.FlowState (scheme 0).  Returns the worst error / bound per check."""
    with _per_face(mu, wrong):
        res = dict(d_p=fc.check_d_p(st)["worst"], matrix=fc.check_matrix_entries(st)["worst"],
                   rhs=fc.check_rhs(st)["worst"])
    res["symmetry_faces"] = check_symmetry(st)
    res["wall_force"] = check_wall_force(st, mu, box, force_viscous, wrong)
    return res
