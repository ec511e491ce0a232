"""Float64 checks of a passive-scalar advance with wall conditions and sources,
written face by face from the discretisation and not from any restatement.

HELPER MODULE, not a test: numpy and scipy.sparse only.  It imports the
unchanged tests/scalar_checks.py for _Faces, the coefficient, range and
allowance helpers and the two solve checks, and none of the restatements.

The equation of cell i (tests/scalar_checks.py has the rest; rho density, a_t =
rho vol_i / dt) gains, per selected wall face f of i (walls are boundary type
3; x_f the face centre, g_f = rho D A_f / |x_f - x_i|) and per source cell,

    kind 1 (fixed value)   + g_f (phi_i - value)      on the left
    kind 2 (fixed flux)    + value A_f                on the right
    source cell            + vol_i rate               on the right

Scheme 1: the Green-Gauss gradient takes `value` as the face value of a
selected kind-1 face, and the clamp's range of cell i takes `value` as well.

Wall flux (what the selected faces give to the fluid, evaluated on a field phi):

    flux     = sum over the selected faces   g_f (value - phi_o)     kind 1
                                             value A_f               kind 2
    area     = sum A_f,    phi_area = sum A_f phi_o       o the face's owner

The budget: the rows summed over all cells as in scalar_checks.check_budget;
the new terms do not cancel, so

    (rho / dt) (I_new - I_old) = inlet + outlet + wall + defect - clamp
                                 + flux(phi_new) + rate sum of vol over the source cells

Bounds: the project's existing allowance, tol plus 16 eps32 of the sum T_i of
the magnitudes of the terms of row i's identity, with the new terms counted in
T_i: g_f (|phi_i| + |value|) per selected kind-1 face, |value| A_f per selected
kind-2 face, vol_i |rate| in a source cell; scheme 1's range term a_t max(|m_i|,
|M_i|) is taken over the widened range and the upwind gradient's magnitudes G
count |value| A_f / vol on a kind-1 face.  No new constant.  The device's
wall-flux sums are compared with the float64 ones to 16 eps32 of the sum of the
magnitudes of their terms (their f32 inputs c_k, A_k and phi_i carry a few
eps32 each and the sums run in f64).

A wall and a source are passed as dicts: wall = dict(kind, value, box), source
= dict(rate, box), box = (x0, y0, x1, y1) closed, x1 < x0 selecting nothing.
"""
import numpy as np
import scipy.sparse as sp

from tests import scalar_checks as sc
from tests.scalar_checks import INLET, WALL, _Faces, _coefficients, _params, _range64, _row_allowance

NO_WALL = dict(kind=0, value=0.0, box=(0.0, 0.0, -1.0, 0.0))
NO_SOURCE = dict(rate=0.0, box=(0.0, 0.0, -1.0, 0.0))


def _in_box(x, y, box):
    x0, y0, x1, y1 = (float(v) for v in box)
    if x1 < x0:
        return np.zeros(len(x), bool)
    return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


def selected_faces(arrays, wall):
    """the wall faces whose (unrounded) centre lies in the box, whatever the kind"""
    m = _Faces(arrays)
    return (m.kind == WALL) & _in_box(np.asarray(arrays["face_cx"], np.float64),
                                      np.asarray(arrays["face_cy"], np.float64), wall["box"])


def selected_cells(arrays, source):
    return _in_box(np.asarray(arrays["cell_cx"], np.float64), np.asarray(arrays["cell_cy"], np.float64), source["box"])


def _wall(arrays, m, rho, D, wall):
    """(faces selected with a kind, their g_f, value rounded to f32)"""
    value = float(np.float32(wall["value"]))
    sel = selected_faces(arrays, wall) if wall["kind"] != 0 else np.zeros(len(m.own), bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(D > 0.0, rho * D * m.area / m.dist, 0.0)
    return sel, g, value


def _source(arrays, m, source):
    rate = float(np.float32(source["rate"]))
    cells = selected_cells(arrays, source) if rate != 0.0 else np.zeros(m.N, bool)
    return cells, rate


def _added(arrays, m, rho, D, wall, source):
    """(what the wall adds to diag, what wall and source add to b), per cell"""
    sel, g, value = _wall(arrays, m, rho, D, wall)
    cells, rate = _source(arrays, m, source)
    o = m.own[sel]
    if wall["kind"] == 1:
        ddiag, db = m.scatter(o, g[sel]), m.scatter(o, g[sel] * value)
    else:
        ddiag, db = np.zeros(m.N), m.scatter(o, value * m.area[sel])
    return ddiag, db + np.where(cells, m.vol * rate, 0.0)


def system64(arrays, flux, density, dt, D, inlet, phi_old, wall=NO_WALL, source=NO_SOURCE):
    """(A, b) of scheme 0 with the wall and source terms"""
    A, b = sc.system64(arrays, flux, density, dt, D, inlet, phi_old)
    m = _Faces(arrays)
    rho, _, Dv, _ = _params(density, dt, D, inlet)
    ddiag, db = _added(arrays, m, rho, Dv, wall, source)
    return (A + sp.diags(ddiag)).tocsr(), b + db


def gradient64(arrays, inlet, phi_old, wall=NO_WALL):
    """scalar_checks.gradient64 with `value` as the face value of the selected
    kind-1 faces: (gx, gy, G)"""
    gx, gy, G = sc.gradient64(arrays, inlet, phi_old)
    if wall["kind"] != 1:
        return gx, gy, G
    m = _Faces(arrays)
    sel = selected_faces(arrays, wall)
    value = float(np.float32(wall["value"]))
    phi = np.asarray(phi_old, np.float64)
    o = m.own[sel]
    dv = value - phi[o]  # the face value moves from phi_o to value
    gx = gx + m.scatter(o, dv * m.nx[sel] * m.area[sel]) / m.vol
    gy = gy + m.scatter(o, dv * m.ny[sel] * m.area[sel]) / m.vol
    G = G + m.scatter(o, (abs(value) - np.abs(phi[o])) * m.area[sel]) / m.vol
    return gx, gy, G


def increments64(arrays, flux, inlet, phi_old, wall=NO_WALL):
    """Per face (h, U, D, weight) as scalar_checks.increments64 defines them,
    from the gradient above: van Leer's psi = (r + |r|) / (1 + |r|) of r = 2 g_U
    . (x_D - x_U) / (phi_D - phi_U) - 1, h = psi (phi_D - phi_U) / 2."""
    m = _Faces(arrays)
    F = np.asarray(flux, np.float64)
    phi = np.asarray(phi_old, np.float64)
    gx, gy, G = gradient64(arrays, inlet, phi_old, wall)
    fwd = F > 0.0
    U = np.where(fwd, m.own, m.nb)
    Dn = np.where(fwd, m.nb, m.own)
    sgn = np.where(fwd, 1.0, -1.0)
    d = phi[Dn] - phi[U]
    gd = sgn * (gx[U] * m.dvx + gy[U] * m.dvy)
    active = m.internal & (F != 0.0)
    with np.errstate(all="ignore"):
        r = 2.0 * gd / d - 1.0
        psi = np.where(np.isinf(r), np.where(r > 0.0, 2.0, 0.0), (r + np.abs(r)) / (1.0 + np.abs(r)))
        h = np.where(active & (d != 0.0), 0.5 * psi * d, 0.0)
    weight = np.where(active, np.abs(d) + 2.0 * G[U] * m.dist, 0.0)
    return h, U, Dn, weight


def range64(arrays, inlet, phi_old, wall=NO_WALL):
    """(m_i, M_i): phi_old over the cell, its face neighbours, the inlet value
    on inlet faces and `value` on selected kind-1 faces"""
    m = _Faces(arrays)
    mn, mx = _range64(m, float(np.float32(inlet)), np.asarray(phi_old, np.float64))
    if wall["kind"] == 1:
        o = m.own[selected_faces(arrays, wall)]
        value = float(np.float32(wall["value"]))
        np.minimum.at(mn, o, value)
        np.maximum.at(mx, o, value)
    return mn, mx


def rhs_limited64(arrays, flux, density, dt, D, inlet, phi_old, wall=NO_WALL, source=NO_SOURCE):
    """(b, clamp) of scheme 1 with the wall and source terms"""
    m = _Faces(arrays)
    rho, dtv, Dv, inl_v = _params(density, dt, D, inlet)
    F = np.asarray(flux, np.float64)
    phi = np.asarray(phi_old, np.float64)
    a_t = rho * m.vol / dtv
    h, U, Dn, _ = increments64(arrays, flux, inlet, phi_old, wall)
    move = np.abs(F) * h
    corr = m.scatter(U, move) - m.scatter(Dn, move)
    mn, mx = range64(arrays, inlet, phi_old, wall)
    t = a_t * phi - corr
    tc = np.minimum(np.maximum(t, a_t * mn), a_t * mx)
    _, c_own, _ = _coefficients(m, F, rho, Dv)
    inl = m.kind == INLET
    _, db = _added(arrays, m, rho, Dv, wall, source)
    return tc + m.scatter(m.own[inl], c_own[inl] * inl_v) + db, t - tc


def row_terms64(arrays, flux, density, dt, D, inlet, phi_old, phi, scheme, wall=NO_WALL, source=NO_SOURCE):
    """T_i with the new terms counted (module docstring)"""
    m = _Faces(arrays)
    rho, dtv, Dv, inl_v = _params(density, dt, D, inlet)
    F = np.asarray(flux, np.float64)
    old, new = np.abs(np.asarray(phi_old, np.float64)), np.abs(np.asarray(phi, np.float64))
    a_t = rho * m.vol / dtv
    _, c_own, c_nb = _coefficients(m, F, rho, Dv)
    i = m.internal
    o, n = m.own[i], m.nb[i]
    inl = m.kind == INLET
    T = a_t * new + m.scatter(o, c_own[i] * (new[o] + new[n])) + m.scatter(n, c_nb[i] * (new[n] + new[o]))
    T += m.scatter(m.own[inl], c_own[inl] * (new[m.own[inl]] + abs(inl_v)))
    sel, g, value = _wall(arrays, m, rho, Dv, wall)
    cells, rate = _source(arrays, m, source)
    ow = m.own[sel]
    if wall["kind"] == 1:
        T += m.scatter(ow, g[sel] * (new[ow] + abs(value)))
    elif wall["kind"] == 2:
        T += m.scatter(ow, abs(value) * m.area[sel])
    T += np.where(cells, m.vol * abs(rate), 0.0)
    if scheme == 0:
        return T + a_t * old
    mn, mx = range64(arrays, inlet, phi_old, wall)
    T += a_t * np.maximum(np.abs(mn), np.abs(mx))
    _, U, Dn, weight = increments64(arrays, flux, inlet, phi_old, wall)
    w = np.abs(F) * weight
    return T + m.scatter(U, w) + m.scatter(Dn, w)


def wall_flux64(arrays, density, D, phi, wall):
    """(flux, area, phi_area, the sum of the magnitudes of the flux's terms)"""
    m = _Faces(arrays)
    rho, _, Dv, _ = _params(density, 1.0, D, 0.0)
    sel, g, value = _wall(arrays, m, rho, Dv, wall)
    po = np.asarray(phi, np.float64)[m.own[sel]]
    if wall["kind"] == 1:
        flux, mag = np.sum(g[sel] * (value - po)), np.sum(g[sel] * (abs(value) + np.abs(po)))
    elif wall["kind"] == 2:
        flux = mag = np.sum(value * m.area[sel])
        mag = abs(mag)
    else:
        return 0.0, 0.0, 0.0, 0.0
    return float(flux), float(np.sum(m.area[sel])), float(np.sum(m.area[sel] * po)), float(mag)


def check_wall_flux(arrays, density, D, phi, wall, got, what=""):
    """The reported (flux, area, phi_area) against the float64 ones, each to 16
    eps32 of the sum of the magnitudes of its terms."""
    flux, area, phi_area, mag = wall_flux64(arrays, density, D, phi, wall)
    m = _Faces(arrays)
    sel = selected_faces(arrays, wall) if wall["kind"] != 0 else np.zeros(len(m.own), bool)
    mag_pa = float(np.sum(m.area[sel] * np.abs(np.asarray(phi, np.float64)[m.own[sel]])))
    for name, g, e, scale in (("flux", got[0], flux, mag), ("area", got[1], area, area),
                              ("phi_area", got[2], phi_area, mag_pa)):
        assert np.isfinite(g) and abs(g - e) <= sc.TOL_ROW * scale, (
            f"f64 check_wall_flux {what}: {name} {g:.12e} vs {e:.12e}: {abs(g - e):.3e} > {sc.TOL_ROW * scale:.3e}")


def check_budget(arrays, flux, density, dt, D, inlet, phi, integral_old, integral_new, clamp, A, tol, terms,
                 wall_flux, source=NO_SOURCE, what=""):
    """(rho / dt) (I_new - I_old) = inlet + outlet + wall + defect - sum clamp +
    wall_flux + rate sum vol, to sum_i (diag_i tol + 16 eps32 T_i).  wall_flux is
    the REPORTED flux on the new field.  Returns (error / bound, the parts)."""
    m = _Faces(arrays)
    rho, dtf, _, _ = _params(density, dt, D, inlet)
    parts = sc.budget64(arrays, flux, density, dt, D, inlet, phi)
    parts["clamp"] = -float(np.sum(clamp))
    parts["wall_flux"] = float(wall_flux)
    cells, rate = _source(arrays, m, source)
    parts["source"] = rate * float(np.sum(m.vol[cells]))
    lhs = rho / dtf * (float(integral_new) - float(integral_old))
    rhs = sum(parts.values())
    diag, allow = _row_allowance(A, tol, terms)
    bound = float(np.sum(diag * allow))
    err = abs(lhs - rhs)
    assert np.isfinite(err) and err <= bound, (
        f"f64 check_budget {what}: (rho / dt) (I_new - I_old) = {lhs:.9e} vs {rhs:.9e} ({parts}): "
        f"{err:.3e} > {bound:.3e}")
    return err / bound, parts
