"""Float64 checks of one passive-scalar advance, written face by face from the
discretisation and not from any restatement of the kernels.

HELPER MODULE, not a test: numpy and scipy.sparse only, and none of
tests/scalar_ref.py, scalar_krylov_ref.py, scalar_hr_ref.py is imported.

Everything loops over FACES with face_owner, face_neighbor and face_boundary
(0 none, 1 inlet, 2 outlet, 3 wall): the normal of a face points from its owner
to its neighbour and the by-face mass flux F (debug buffer 0) is positive from
owner to neighbour.  cell_faces is not read at all.  The geometry is the mesh
arrays rounded to f32 and widened (as tests/fv_checks.py takes them), and
density, dt, D and the inlet value are rounded to f32 likewise, so every bound
below is about arithmetic only.

The equation of cell i (rho density, a_t = rho vol_i / dt):

    a_t (phi_i - phi_old_i)
      + sum over internal faces f of i   (max(-F_out, 0) + g_f) (phi_i - phi_j)
      + sum over inlet faces f of i      (max(-F_out, 0) + g_f) (phi_i - inlet)
      = - corr_i - clamp_i

F_out the flux out of i through f (+F for the owner, -F for the neighbour), j
the cell across f, g_f = rho D A_f / |x_j - x_i| (inlet: |x_f - x_i|).  Walls
and outlets contribute nothing.  Scheme 0 has corr = clamp = 0.  Scheme 1:
every internal face with F != 0 has an upwind cell U and a downwind cell D, the
ratio r = 2 g_U . (x_D - x_U) / (phi_D - phi_U) - 1 of the Green-Gauss gradient
g_U of phi_old, van Leer's psi = (r + |r|) / (1 + |r|) and the increment h =
psi (phi_D - phi_U) / 2 (0 where phi_D == phi_U); |F| h is added to corr_U and
taken from corr_D.  Last, a_t phi_old_i - corr_i is clamped to a_t times the
range of phi_old over i, its face neighbours and the inlet value on inlet
faces; clamp_i is what the clamp took away (unclamped minus clamped).

Bounds.  tol is the solver's stopping tolerance on max |phi^{m+1} - phi^m|
(1e-6).  Every bound is tol's share plus a rounding bound in the style of
fv_checks.TOL_ROW, 16 eps32 times the sum T_i of the magnitudes of the terms
of row i's identity (row_terms64), not a measurement:

- check_solved: |b - A phi|_i / diag_i <= tol + 16 eps32 T_i / diag_i.
  Jacobi's last sweep gives phi^{m+1}_i = (b_i + sum c phi^m_j) / diag_i, so
  the residual of phi^{m+1} in the f32 system is sum c (phi^{m+1}_j - phi^m_j),
  at most (diag_i - a_t) tol; both methods end with that sweep.  The f32
  system differs from the f64 one by the rounding of its terms.  T_i holds
  a_t |phi_i|, a_t |phi_old_i|, per internal face c (|phi_i| + |phi_j|) and per
  inlet face c (|phi_i| + |inlet|).  Scheme 1: a_t |phi_old_i| becomes a_t
  max(|m_i|, |M_i|) (the clamp's bounds are products of their own), and every
  internal face with F != 0 adds |F| (|phi_D - phi_U| + 2 G_U |x_D - x_U|) to
  both of its rows, G_U = sum_f |vf| A_f / vol_U the magnitudes of the terms
  of the upwind gradient.  Where r > 0, h = d - d^2 / (2 gd) with d = phi_D -
  phi_U and gd = g_U . (x_D - x_U): |dh/dd| = |1 - d/gd| < 1 and 0 < dh/dgd =
  d^2 / (2 gd^2) < 2, h = 0 elsewhere and on r = 0, and the clamp is a
  contraction, so the right-hand side is Lipschitz in the rounded quantities
  with constant at most 2 and no cell is left out.
- check_against_direct_solve: A is strictly diagonally dominant by rows with
  excess at least a_t,i, so |A^-1|_inf <= 1 / min a_t (Varah) and
  max |phi - A^-1 b| <= max_i (diag_i (tol + 16 eps32 T_i / diag_i)) / min a_t.
- check_budget: the rows above summed over all cells.  The diffusive terms of
  an internal face cancel between its two rows, sum_i corr_i = 0, and
  max(-F_out, 0) (phi_i - phi_j) = F_out phi_upwind - F_out phi_i, whose first
  part also cancels between the two rows.  With netF_i the signed sum of the
  fluxes out of i over ALL its faces, the boundary faces give back what netF_i
  counts of them, and what is left is

    (rho / dt) (I_new - I_old)
      =   sum over inlet faces   max(-F, 0) inlet - max(F, 0) phi_o + g_f (inlet - phi_o)
        - sum over outlet faces  F phi_o
        - sum over wall faces    F phi_o          (F = 0 there by construction)
        + sum_i phi_i netF_i                      (the header's conservation defect)
        - sum_i clamp_i                           (zero under scheme 0)

  phi the new field, o the face's owner, I = sum vol phi (cfd_scalar_stats.
  integral, f64).  Tolerance: sum_i (diag_i tol + 16 eps32 T_i), the row
  bounds summed.

Worst error / (tol's share + rounding bound) measured on the CPU, on the
restatements' output over the whole case list of tests/scalar_cases.py
(tests/test_scalar_f64.py prints them per mesh with -s), never on the device.
No derivation had to be changed: every case passed as first written.
  check_solved               0.631  graded, density 1000, scheme 0, BiCGStab,
                                    D = 0.05, step profile, second advance
  check_against_direct_solve 0.045  strip130, density 1, scheme 0, Jacobi,
                                    D = 0.01, smooth profile, first advance
  check_budget               0.020  wheel100, density 1000, scheme 0, BiCGStab,
                                    D = 0.05, smooth profile, first advance
A row's allowance is tol = 1e-6 plus 16 eps32 T_i / diag_i, a few 1e-6 of a
cell value, so the checks resolve a few 1e-6 per row: the wrong conventions of
tests/test_scalar_f64.py miss by 1e-3 and more.
"""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spl

EPS32 = float(np.finfo(np.float32).eps)
TOL_ROW = 16.0 * EPS32
NONE = 0xFFFFFFFF
INLET, OUTLET, WALL = 1, 2, 3


def _f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


class _Faces:
    """The mesh by faces, f32-rounded and widened."""

    def __init__(self, arrays):
        a = arrays
        self.N = len(a["cell_vol"])
        self.own = a["face_owner"].astype(np.int64)
        nb = a["face_neighbor"].astype(np.int64)
        self.internal = nb != NONE
        self.nb = np.where(self.internal, nb, 0)
        self.kind = np.where(self.internal, 0, a["face_boundary"].astype(np.int64))
        self.area = _f32(a["face_area"])
        self.fx, self.fy = _f32(a["face_cx"]), _f32(a["face_cy"])
        self.nx, self.ny = _f32(a["face_nx"]), _f32(a["face_ny"])
        self.cx, self.cy = _f32(a["cell_cx"]), _f32(a["cell_cy"])
        self.vol = _f32(a["cell_vol"])
        o, n = self.own, self.nb
        # owner centre to neighbour centre (internal) or to the face centre (boundary)
        self.dvx = np.where(self.internal, self.cx[n] - self.cx[o], self.fx - self.cx[o])
        self.dvy = np.where(self.internal, self.cy[n] - self.cy[o], self.fy - self.cy[o])
        self.dist = np.hypot(self.dvx, self.dvy)

    def scatter(self, cells, values):
        out = np.zeros(self.N)
        np.add.at(out, cells, values)
        return out


def _params(density, dt, D, inlet):
    return tuple(float(np.float32(v)) for v in (density, dt, D, inlet))


def time_coefficient64(arrays, density, dt):
    """a_t = rho vol / dt per cell"""
    rho, dt, _, _ = _params(density, dt, 0.0, 0.0)
    return rho * _f32(arrays["cell_vol"]) / dt


def _coefficients(m, flux, rho, D):
    """per face: (g, the owner row's coefficient, the neighbour row's)"""
    F = np.asarray(flux, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = np.where(D > 0.0, rho * D * m.area / m.dist, 0.0)
    return g, np.maximum(-F, 0.0) + g, np.maximum(F, 0.0) + g


def system64(arrays, flux, density, dt, D, inlet, phi_old):
    """(A, b): the scipy CSR matrix of the rows above and scheme 0's right-hand
    side a_t phi_old + sum over inlet faces c inlet, in float64."""
    m = _Faces(arrays)
    rho, dt, D, inlet = _params(density, dt, D, inlet)
    F = np.asarray(flux, np.float64)
    a_t = rho * m.vol / dt
    g, c_own, c_nb = _coefficients(m, F, rho, D)
    i = m.internal
    o, n = m.own[i], m.nb[i]
    inl = m.kind == INLET
    diag = a_t + m.scatter(o, c_own[i]) + m.scatter(n, c_nb[i]) + m.scatter(m.own[inl], c_own[inl])
    rows = np.concatenate([np.arange(m.N), o, n])
    cols = np.concatenate([np.arange(m.N), n, o])
    vals = np.concatenate([diag, -c_own[i], -c_nb[i]])
    A = sp.csr_matrix((vals, (rows, cols)), shape=(m.N, m.N))
    b = a_t * np.asarray(phi_old, np.float64) + m.scatter(m.own[inl], c_own[inl] * inlet)
    return A, b


def gradient64(arrays, inlet, phi_old):
    """Green-Gauss gradient (gx, gy) of phi_old and G, the sum of the
    magnitudes of its terms: face value w phi_o + (1 - w) phi_n with w = |x_f -
    x_n| / (|x_f - x_o| + |x_f - x_n|), the inlet value on inlet faces, the
    cell's own value on walls and outlets."""
    m = _Faces(arrays)
    inlet = float(np.float32(inlet))
    phi = np.asarray(phi_old, np.float64)
    o, n = m.own, m.nb
    d_o = np.hypot(m.fx - m.cx[o], m.fy - m.cy[o])
    d_n = np.hypot(m.fx - m.cx[n], m.fy - m.cy[n])
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(m.internal, d_n / (d_o + d_n), 1.0)
    vf = np.where(m.internal, w * phi[o] + (1.0 - w) * phi[n], np.where(m.kind == INLET, inlet, phi[o]))
    i = m.internal
    gx = (m.scatter(o, vf * m.nx * m.area) - m.scatter(n[i], (vf * m.nx * m.area)[i])) / m.vol
    gy = (m.scatter(o, vf * m.ny * m.area) - m.scatter(n[i], (vf * m.ny * m.area)[i])) / m.vol
    G = (m.scatter(o, np.abs(vf) * m.area) + m.scatter(n[i], (np.abs(vf) * m.area)[i])) / m.vol
    return gx, gy, G


def increments64(arrays, flux, inlet, phi_old):
    """Per face: (h, U, D, weight): the limited increment of the face value over
    the upwind cell's, the upwind and downwind cells, and |phi_D - phi_U| + 2
    G_U |x_D - x_U|.  h = 0 on boundary faces and where F == 0."""
    m = _Faces(arrays)
    F = np.asarray(flux, np.float64)
    phi = np.asarray(phi_old, np.float64)
    gx, gy, G = gradient64(arrays, inlet, phi_old)
    fwd = F > 0.0
    U = np.where(fwd, m.own, m.nb)
    Dn = np.where(fwd, m.nb, m.own)
    sgn = np.where(fwd, 1.0, -1.0)  # x_D - x_U = sgn (x_n - x_o)
    d = phi[Dn] - phi[U]
    gd = sgn * (gx[U] * m.dvx + gy[U] * m.dvy)
    active = m.internal & (F != 0.0)
    with np.errstate(all="ignore"):
        r = 2.0 * gd / d - 1.0
        psi = np.where(np.isinf(r), np.where(r > 0.0, 2.0, 0.0), (r + np.abs(r)) / (1.0 + np.abs(r)))
        h = np.where(active & (d != 0.0), 0.5 * psi * d, 0.0)
    weight = np.where(active, np.abs(d) + 2.0 * G[U] * m.dist, 0.0)
    return h, U, Dn, weight


def _range64(m, inlet, phi):
    mn, mx = phi.copy(), phi.copy()
    i = m.internal
    o, n = m.own[i], m.nb[i]
    for lo_hi, f in ((mn, np.minimum), (mx, np.maximum)):
        f.at(lo_hi, o, phi[n])
        f.at(lo_hi, n, phi[o])
        f.at(lo_hi, m.own[m.kind == INLET], inlet)
    return mn, mx


def rhs_limited64(arrays, flux, density, dt, D, inlet, phi_old):
    """(b, clamp): scheme 1's right-hand side in float64 and, per cell, what the
    clamp took away (unclamped minus clamped; zero where it did not act)."""
    m = _Faces(arrays)
    rho, dt, D, inlet = _params(density, dt, D, inlet)
    F = np.asarray(flux, np.float64)
    phi = np.asarray(phi_old, np.float64)
    a_t = rho * m.vol / dt
    h, U, Dn, _ = increments64(arrays, flux, inlet, phi_old)
    move = np.abs(F) * h
    corr = m.scatter(U, move) - m.scatter(Dn, move)
    mn, mx = _range64(m, inlet, phi)
    t = a_t * phi - corr
    tc = np.minimum(np.maximum(t, a_t * mn), a_t * mx)
    _, c_own, _ = _coefficients(m, F, rho, D)
    inl = m.kind == INLET
    return tc + m.scatter(m.own[inl], c_own[inl] * inlet), t - tc


def row_terms64(arrays, flux, density, dt, D, inlet, phi_old, phi, scheme):
    """T_i: the sum of the magnitudes of the terms of row i's identity (module docstring)."""
    m = _Faces(arrays)
    rho, dt, D, inlet = _params(density, dt, D, inlet)
    F = np.asarray(flux, np.float64)
    old, new = np.abs(np.asarray(phi_old, np.float64)), np.abs(np.asarray(phi, np.float64))
    a_t = rho * m.vol / dt
    _, c_own, c_nb = _coefficients(m, F, rho, D)
    i = m.internal
    o, n = m.own[i], m.nb[i]
    inl = m.kind == INLET
    T = a_t * new + m.scatter(o, c_own[i] * (new[o] + new[n])) + m.scatter(n, c_nb[i] * (new[n] + new[o]))
    T += m.scatter(m.own[inl], c_own[inl] * (new[m.own[inl]] + abs(inlet)))
    if scheme == 0:
        return T + a_t * old
    mn, mx = _range64(m, inlet, np.asarray(phi_old, np.float64))
    T += a_t * np.maximum(np.abs(mn), np.abs(mx))
    _, U, Dn, weight = increments64(arrays, flux, inlet, phi_old)
    w = np.abs(F) * weight
    return T + m.scatter(U, w) + m.scatter(Dn, w)


def _row_allowance(A, tol, terms):
    diag = A.diagonal()
    assert np.all(diag > 0.0) and np.all(np.isfinite(terms))
    return diag, tol + TOL_ROW * terms / diag


def check_solved(A, b, phi, tol, terms, what=""):
    """|b - A phi|_i / diag_i <= tol + 16 eps32 T_i / diag_i on every row.
    Returns (rows checked, worst error / bound)."""
    phi = np.asarray(phi, np.float64)
    diag, allow = _row_allowance(A, tol, terms)
    res = np.abs(b - A @ phi) / diag
    assert np.all(np.isfinite(res)), f"f64 check_solved {what}: non-finite residual"
    ratio = res / allow
    w = int(np.argmax(ratio))
    assert ratio[w] <= 1.0, (f"f64 check_solved {what}: cell {w}: |b - A phi| / diag = {res[w]:.3e} > tol + bound = "
                             f"{allow[w]:.3e} (bound {allow[w] - tol:.3e}, {ratio[w]:.2f} x)")
    return len(res), float(ratio[w])


def check_against_direct_solve(A, b, phi, tol, terms, a_t, what=""):
    """max |phi - spsolve(A, b)| <= max_i (diag_i (tol + bound_i)) / min_i a_t,i.
    Returns error / bound."""
    phi = np.asarray(phi, np.float64)
    diag, allow = _row_allowance(A, tol, terms)
    exact = np.atleast_1d(spl.spsolve(A.tocsc(), b))
    err = np.abs(phi - exact)
    bound = float(np.max(diag * allow) / np.min(a_t))
    w = int(np.argmax(err))
    assert np.isfinite(err[w]) and err[w] <= bound, (
        f"f64 check_against_direct_solve {what}: cell {w}: phi {phi[w]:.9e} vs the float64 solve {exact[w]:.9e}: "
        f"{err[w]:.3e} > {bound:.3e}")
    return float(err[w] / bound)


def budget64(arrays, flux, density, dt, D, inlet, phi):
    """The right-hand side of the budget without the clamp, as a dict of its
    parts: inlet, outlet, wall, defect (module docstring)."""
    m = _Faces(arrays)
    rho, dt, D, inlet = _params(density, dt, D, inlet)
    F = np.asarray(flux, np.float64)
    phi = np.asarray(phi, np.float64)
    g, _, _ = _coefficients(m, F, rho, D)
    po = phi[m.own]
    inl, out, wall = m.kind == INLET, m.kind == OUTLET, m.kind == WALL
    i = m.internal
    net = m.scatter(m.own, F) - m.scatter(m.nb[i], F[i])
    return {"inlet": float(np.sum((np.maximum(-F, 0.0) * inlet - np.maximum(F, 0.0) * po + g * (inlet - po))[inl])),
            "outlet": float(-np.sum((F * po)[out])), "wall": float(-np.sum((F * po)[wall])),
            "defect": float(np.sum(phi * net))}


def check_budget(arrays, flux, density, dt, D, inlet, phi, integral_old, integral_new, clamp, A, tol, terms, what=""):
    """(rho / dt) (I_new - I_old) = inlet + outlet + wall + defect - sum clamp, to
    sum_i (diag_i tol + 16 eps32 T_i).  Returns (error / bound, the parts)."""
    rho, dtf, _, _ = _params(density, dt, D, inlet)
    parts = budget64(arrays, flux, density, dt, D, inlet, phi)
    parts["clamp"] = -float(np.sum(clamp))
    lhs = rho / dtf * (float(integral_new) - float(integral_old))
    rhs = sum(parts.values())
    diag, allow = _row_allowance(A, tol, terms)
    bound = float(np.sum(diag * allow))
    err = abs(lhs - rhs)
    assert np.isfinite(err) and err <= bound, (
        f"f64 check_budget {what}: (rho / dt) (I_new - I_old) = {lhs:.9e} vs {rhs:.9e} ({parts}): "
        f"{err:.3e} > {bound:.3e}")
    return err / bound, parts
