"""Float64 checks of the flow side of one outer iteration -- the Rhie-Chow face
flux, the Green-Gauss gradients, d_p, every entry of the coupled and of the
scalar matrix, the right-hand side and the under-relaxed update -- written face
by face from the discretisation and not from any restatement of the kernels.

HELPER MODULE, not a test: numpy and scipy only, and none of tests/refpy.py,
numpy_ref.py, wgsl_ref.py, oracle_py.py, buoyancy_ref.py is imported; of
tests/fv_checks.py only the storage order of the two matrices and the constants.

Everything loops over FACES with face_owner, face_neighbor and face_boundary
(0 none, 1 inlet, 2 outlet, 3 wall), the face areas, normals and centres and
the cell centres and volumes; cell_faces and the slot layout are not read.  The
geometry is the mesh arrays rounded to f32 and widened (as tests/fv_checks.py
and tests/scalar_checks.py take them) and so is every constant, so each bound
below is about arithmetic only.

Every check is STAGED: it takes the f32 outputs of the stage before it as its
inputs and verifies one stage's arithmetic.  FlowState holds them: u, p, d_p
and grad p as they stood BEFORE debug_prepare_assemble (`pre`), and after it
the flux (buffer 0), grad u, grad v, grad p (1, 2, 10), the new d_p, the
right-hand side (3), the two matrices (9, 8) and the two old velocities (11,
12).  Every upwind decision of the assembly checks reads the sign of the
stored f32 flux, as the kernel does.

Notation.  n: the stored normal of a face, from its owner O to its neighbour N
(a normal stored the other way, (x_f - x_O) . n < 0, is turned for the flux
alone; the gradients and the matrix take it as stored).  s = +1 for the owner,
-1 for the neighbour: s n points out of cell i, F_out = s F.  x_other: the
centre of the cell across the face, the face centre x_f on a boundary face.

Face geometry
    d_O = |x_f - x_O|, d_N = |x_f - x_N|
    lambda_f = d_N / (d_O + d_N)       the OWNER's weight; 1/2 where d_O + d_N <= 1e-6
                                       (the velocity in the gradients is then the plain mean)
    w_i      = lambda_f for the owner, 1 - lambda_f for the neighbour: a cell's own weight
    dist_n   = max(|(x_other - x_i) . n|, 1e-6)
    dist_c   = |x_other - x_i|
    u_b      = (inlet_velocity smoothstep(0, ramp_time, time), 0)

check_flux (buffer 0), every face, from the `pre` state
    internal  F = rho A [ u_f . n + dpf ( gp_f . n - (p_N - p_O) / dist_n ) ]
              u_f, dpf, gp_f: lambda_f (owner) + (1 - lambda_f) (neighbour)
    inlet     F = rho (u_b . n) A
    outlet    F = max(0, rho (u_O . n) A)
    wall      F = 0 exactly
  The body force of a driving scalar does not enter the flux: that is how the
  flux is defined today (a known inconsistency, not this check's business).

check_gradients (buffers 1, 2, 10), every cell
    g_i = (1 / V_i) sum_f phi_f s A n
    internal  phi_f = w_i phi_i + (1 - w_i) phi_j
    inlet     u = u_b, p = p_i      wall  u = 0, p = p_i      outlet  u = u_i, p = 0

check_d_p (get_d_p after prepare), every cell
    d_p = V / (a_t + sum_f ...),  a_t = rho V / dt  (BDF2: times (1 + 2r) / (1 + r), r = dt / dt_old)
    internal, inlet, wall   nu A / dist_c + max(F_out, 0)
    outlet                  max(F_out, 0)
  This diagonal takes the CENTRE distance dist_c, the assembled A_uu diagonal
  below the projected dist_n: the reference's convention (oracle.cpp
  prepare_cells(): `dist = sqrt(dvx * dvx + dvy * dvy); diff_coeff = viscosity
  * area / dist`, against assemble(): `dist = fmax(fabs(dvx * nx + dvy * ny),
  1e-6f)`).  test_checks_resolve_wrong_conventions shows that either check
  fails with the other's distance.

check_matrix_entries (buffers 9 and 8), every stored entry of every row
    A_uu[i,j] = A_vv[i,j] = -nu A / dist_n + min(F_out, 0)
    A_uu[i,i] = a_t + sum  internal, inlet  nu A / dist_n + max(F_out, 0)
                           wall             nu A / dist_n
                           outlet           max(F_out, 0)
    A_uv = A_vu = 0 exactly
    A_up[i,j] = A_pu[i,j] = (1 - w_i) A s n_x          (A_vp, A_pv: n_y)
    A_up[i,i] = sum  internal w_i A s n_x  +  inlet, wall  A s n_x
    A_pu[i,i] = sum  internal w_i A s n_x  +  outlet       A s n_x
    A_pp[i,j] = -dpf A / dist_n,  dpf = w_i d_p,i + (1 - w_i) d_p,j  (the new d_p)
    A_pp[i,i] = sum internal dpf A / dist_n  +  outlet  d_p,i A / dist_n
    scalar matrix = rho A_pp, entry by entry
  Supplements the identities of tests/fv_checks.py (row sums, closure,
  symmetry, dominance), which see none of nu A / d, of the split of the
  convective part or of a boundary row; it does not replace them.

check_rhs (buffer 3), every row
    momentum  Euler  a_t u^n                          (buffer 11)
              BDF2   (rho V / dt) ((1 + r) u^n - r^2 / (1 + r) u^{n-1})   (buffers 11, 12)
              + sum over inlet faces     (nu A / dist_n + max(-F_out, 0)) u_b
              - sum over internal faces  F_out (phi_HO - phi_UP)        schemes 1, 2
                  U = i where F_out > 0, else j;  D the other;  phi_UP = phi_U
                  scheme 1  phi_HO = phi_U + g_U . (x_f - x_U)
                  scheme 2  phi_HO = 5/8 phi_U + 3/8 phi_D + 1/8 g_U . (x_D - x_U)
              - rho V sum_f beta_f (phi_f,i - ref_f) g                  driving fields
    continuity  - sum over inlet faces (u_b . s n) A

check_update (k_update_fields)
    u_new = u + alpha_u (x_u - u),  p_new = p + alpha_p (x_p - p),  x buffer 4
check_fold
    the reported max |du|, max |dp| are the f32 maxima of |new - old| exactly
    (a max is order-independent).

Bounds.  All derived, in the house style: fv_checks.TOL_ROW = 16 eps32 times
the sum of the magnitudes of the terms of that face's, entry's or row's
formula.  Cancelling quantities are carried by magnitude: in gp_f . n - (p_N -
p_O) / dist_n every part counts by its absolute value, |p_N| + |p_O| for the
difference, and the ramp t^2 (3 - 2t) as t^2 (3 + 2t).  A quotient q by dist_n
= |dvx nx + dvy ny| inherits the cancellation of that sum: with each product
and the sum rounded once, |delta dist_n| <= eps (|dvx nx| + |dvy ny|) to first
order, so |delta q| <= |q| eps (|dvx nx| + |dvy ny|) / dist_n, and q counts as
|q| (|dvx nx| + |dvy ny|) / dist_n (at least |q|; exactly |q| on a floored
face, where dist_n is the constant).  dist_c and d_O, d_N are square roots of
sums of squares, and dvx = x_other - x_i is one rounding of f32 inputs: neither
amplifies.  d_p = V / D: every term of D is positive, so the bound is 16 eps32
d_p.  What the first derivation missed (the CPU oracle showed it: d_p of the
hub of wheel100, 100 faces, at 1.20 x): a cell's sum is a running f32 sum over
its faces, one more rounding of at most eps32 / 2 times the sum of the
magnitudes per term, and 16 eps32 covers "about a dozen" of them
(fv_checks).  So every per-cell sum (gradients, d_p, the diagonal blocks,
the right-hand side) takes (16 + max(faces_i - 12, 0) / 2) eps32: 60 eps32 on
that hub, 16 eps32 on every cell of up to 12 faces, which is every other
cell of the case list.

Branches that f64 and f32 can legitimately read differently, accepted either
way and counted (`either`, at most 1 % of a case's faces, asserted by the
drivers): the outlet clamp where |raw| is within its own bound; a distance sum
d_O + d_N within 16 eps32 of the 1e-6 floor (both lambdas are evaluated and
the better one taken); a stored internal flux of exactly 0 (both upwind
choices multiply by it: the same value either way, counted only).  A
projected distance at the floor needs no second branch: max(., 1e-6) is
continuous.  A face whose orientation (x_f - x_O) . n is within its rounding
of 0 would need one; Geometry asserts that there is none.

Worst error / bound measured on the CPU oracle over the whole case list of
tests/flow_cases.py (tests/test_flow_f64.py prints them per mesh with -s;
profiles/r14/f64_flow_deviation.txt), never on the device:
  check_flux            0.135  graded, scheme 1, Euler, density 1000
  check_gradients       0.143  channel13, scheme 0, Euler, density 1000
  check_d_p             0.320  wheel100, scheme 0, BDF2, density 1 (the hub, at its 60 eps32;
                               0.182 on voronoi, the worst cell of at most 12 faces)
  check_matrix_entries  0.319  wheel100, scheme 0, BDF2, density 1 (the hub's A_uu diagonal;
                               0.186 on voronoi)
  check_rhs             0.162  voronoi, scheme 2, Euler, density 1
  check_update          0.068  channel13
One derivation had to be corrected (the running sum, above); nothing else
failed as first written.  An entry's allowance is a few 1e-6 of its own terms,
so the wrong conventions of tests/test_flow_f64.py miss by 3 x at the least
(dist_n in d_p on voronoi) and by 500 x to 1e6 x elsewhere.
"""
import numpy as np

from tests import fv_checks as fv

EPS32 = fv.EPS32
TOL_ROW = fv.TOL_ROW
NONE = fv.NONE
INLET, OUTLET, WALL = 1, 2, 3
FLOOR = float(np.float32(1e-6))
D_P_GUARD = float(np.float32(1e-20))  # |diagonal| <= guard: d_p is 0
SUM_COVERED = 12  # terms of a running sum that TOL_ROW covers ("about a dozen": fv_checks)

# the deliberate errors of test_checks_resolve_wrong_conventions
WRONG = ("matrix_dist_c", "d_p_dist_n", "lambda_swapped", "rhie_chow_sign", "quick_swapped", "bdf2_r", "no_ramp",
         "outlet_p", "nu_scaled")


def _f32(x):
    return np.asarray(x).astype(np.float32).astype(np.float64)


class Constants:
    """The solver's constants, f32 widened."""

    def __init__(self, c, wrong=()):
        f = lambda v: float(np.float32(v))  # noqa: E731
        self.dt, self.dt_old, self.time = f(c.dt), f(c.dt_old), f(c.time)
        self.nu, self.rho = f(c.viscosity), f(c.density)
        self.alpha_u, self.alpha_p = f(c.alpha_u), f(c.alpha_p)
        self.scheme, self.time_scheme = int(c.scheme), int(c.time_scheme)
        if "nu_scaled" in wrong:
            self.nu *= 1.0 + 2.0 ** -10
        t = min(max(self.time / f(c.ramp_time), 0.0), 1.0)
        ramp, ramp_mag = t * t * (3.0 - 2.0 * t), t * t * (3.0 + 2.0 * t)
        if "no_ramp" in wrong:
            ramp = ramp_mag = 1.0
        self.ub, self.ub_mag = f(c.inlet_velocity) * ramp, abs(f(c.inlet_velocity)) * ramp_mag
        self.r = self.dt / self.dt_old
        self.bdf2_old = (self.r if "bdf2_r" in wrong else self.r * self.r) / (1.0 + self.r)

    def a_t(self, vol):
        tc = vol * self.rho / self.dt
        return tc * (1.0 + 2.0 * self.r) / (1.0 + self.r) if self.time_scheme == 1 else tc


class Geometry:
    """The mesh by faces, f32-rounded and widened.  alt: the faces whose distance
    sum is at the floor (`ambiguous`) take the other lambda."""

    def __init__(self, arrays, wrong=(), alt=False):
        a = arrays
        self.N, self.F = len(a["cell_vol"]), len(a["face_area"])
        self.own = a["face_owner"].astype(np.int64)
        nb = a["face_neighbor"].astype(np.int64)
        self.internal = nb != NONE
        self.nb = np.where(self.internal, nb, self.own)
        self.kind = np.where(self.internal, 0, a["face_boundary"].astype(np.int64))
        assert np.all(self.internal | np.isin(self.kind, (INLET, OUTLET, WALL)))
        self.area = _f32(a["face_area"])
        self.fx, self.fy = _f32(a["face_cx"]), _f32(a["face_cy"])
        self.nx, self.ny = _f32(a["face_nx"]), _f32(a["face_ny"])
        self.cx, self.cy = _f32(a["cell_cx"]), _f32(a["cell_cy"])
        self.vol = _f32(a["cell_vol"])
        o, n, i = self.own, self.nb, self.internal
        # the normal of the flux: turned where it is stored pointing into the owner
        rx, ry = self.fx - self.cx[o], self.fy - self.cy[o]
        out = rx * self.nx + ry * self.ny
        undecided = np.abs(out) <= TOL_ROW * (np.abs(rx * self.nx) + np.abs(ry * self.ny))
        assert not np.any(undecided & (out != 0.0)), f"face {np.nonzero(undecided & (out != 0.0))[0][:1]}: orientation"
        self.turned = out < 0.0
        self.fnx, self.fny = np.where(self.turned, -self.nx, self.nx), np.where(self.turned, -self.ny, self.ny)
        # the owner's weight
        d_o = np.hypot(rx, ry)
        d_n = np.where(i, np.hypot(self.fx - self.cx[n], self.fy - self.cy[n]), 0.0)
        tot = d_o + d_n
        self.ambiguous = i & (np.abs(tot - FLOOR) <= TOL_ROW * FLOOR)
        self.degenerate = i & ((tot <= FLOOR) != (self.ambiguous & alt))
        with np.errstate(divide="ignore", invalid="ignore"):
            lam = np.where(self.degenerate, 0.5, d_n / tot)
        if "lambda_swapped" in wrong:
            lam = 1.0 - lam
        self.lam = np.where(i, lam, 1.0)
        # owner centre to the neighbour's (internal) or to the face centre (boundary)
        self.dvx = np.where(i, self.cx[n] - self.cx[o], rx)
        self.dvy = np.where(i, self.cy[n] - self.cy[o], ry)
        proj = np.abs(self.dvx * self.nx + self.dvy * self.ny)
        self.floored = proj <= FLOOR
        self.dist_n = np.maximum(proj, FLOOR)
        self.dist_c = np.hypot(self.dvx, self.dvy)
        # what a quotient by dist_n counts for, over its own magnitude (module docstring)
        self.qamp = np.where(self.floored, 1.0,
                             np.maximum((np.abs(self.dvx * self.nx) + np.abs(self.dvy * self.ny)) / self.dist_n, 1.0))
        # a cell's sums run over its faces one by one: see "Bounds" in the module docstring
        faces_of = self.scatter(np.concatenate([o, n[i]]), 1.0)
        self.cell_tol = TOL_ROW + 0.5 * EPS32 * np.maximum(faces_of - SUM_COVERED, 0.0)
        pair = np.stack([np.minimum(o, n), np.maximum(o, n)])[:, i]
        assert pair.shape[1] == 0 or len(np.unique(pair, axis=1).T) == int(i.sum()), "two faces join the same two cells"

    def sides(self):
        """The (cell, face, s, own weight, other cell) of every cell-face incidence:
        every face from its owner, every internal face from its neighbour too."""
        f_all, f_in = np.arange(self.F), np.nonzero(self.internal)[0]
        cell = np.concatenate([self.own, self.nb[f_in]])
        face = np.concatenate([f_all, f_in])
        s = np.concatenate([np.ones(self.F), -np.ones(len(f_in))])
        w = np.concatenate([self.lam, 1.0 - self.lam[f_in]])
        other = np.concatenate([self.nb, self.own[f_in]])
        return cell, face, s, w, other

    def scatter(self, cells, values):
        out = np.zeros(self.N)
        np.add.at(out, cells, values)
        return out


class FlowState:
    """What the checks read of one solver: capture_pre before
    debug_prepare_assemble, capture_post after it.  All float64 from f32."""

    def __init__(self, mesh, solver):
        self.mesh, self.arrays = mesh, mesh.arrays()
        self.constants = solver.constants
        self.u = np.asarray(solver.get_u(), np.float64).reshape(-1, 2).copy()
        self.p = np.asarray(solver.get_p(), np.float64).copy()
        self.d_p_pre = np.asarray(solver.get_d_p(), np.float64).copy()
        self.grad_p_pre = solver.debug_buffer(10).astype(np.float64).reshape(-1, 2)
        self.buoyancy = None  # (gx, gy, [(beta, ref, phi), ...])

    def capture_post(self, solver):
        buf = lambda i: solver.debug_buffer(i).astype(np.float64)  # noqa: E731
        self.flux = buf(0)
        self.grad_u, self.grad_v, self.grad_p = buf(1).reshape(-1, 2), buf(2).reshape(-1, 2), buf(10).reshape(-1, 2)
        self.d_p = np.asarray(solver.get_d_p(), np.float64).copy()
        self.rhs, self.scalar, self.coupled = buf(3), buf(8), buf(9)
        self.u_old, self.u_old_old = buf(11).reshape(-1, 2), buf(12).reshape(-1, 2)
        assert np.array_equal(np.asarray(solver.get_u(), np.float64).reshape(-1, 2), self.u)  # prepare moves neither
        assert np.array_equal(np.asarray(solver.get_p(), np.float64), self.p)
        return self


def _geometries(st, wrong):
    g = Geometry(st.arrays, wrong)
    return [g] + ([Geometry(st.arrays, wrong, alt=True)] if np.any(g.ambiguous) else [])


def _judge(what, variants, label):
    """variants: (err, bound) arrays per geometry variant; elementwise the better
    one counts.  Returns the worst error / bound; raises naming the element."""
    ratio = None
    for err, bound in variants:
        assert np.all(np.isfinite(err)) and np.all(np.isfinite(bound)), f"f64 {what}: non-finite"
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err == 0.0, 0.0, np.abs(err) / bound)  # 0 / 0: exact; x / 0: inf
        ratio = r if ratio is None else np.minimum(ratio, r)
    if ratio.size == 0:
        return 0.0
    w = int(np.argmax(ratio))
    err, bound = variants[0]
    assert ratio[w] <= 1.0, (f"f64 {what}: {label(w)}: |error| {abs(err[w]):.3e} > bound {bound[w]:.3e} "
                             f"({ratio[w]:.2f} x)")
    return float(ratio[w])


# ------------------------------------------------------------------------- flux
def flux64(g, c, st, wrong=()):
    """(F, M, raw, clamp bound): the face flux in float64, the sum of the
    magnitudes of its terms, and on outlet faces the unclamped value and its bound."""
    o, n, lam, A = g.own, g.nb, g.lam, g.area
    nx, ny = g.fnx, g.fny
    u, p, dp, gp = st.u, st.p, st.d_p_pre, st.grad_p_pre
    mix = lambda q: lam * q[o] + (1.0 - lam) * q[n]  # noqa: E731
    un = mix(u[:, 0]) * nx + mix(u[:, 1]) * ny
    un_mag = mix(np.abs(u[:, 0])) * np.abs(nx) + mix(np.abs(u[:, 1])) * np.abs(ny)
    dpf = mix(dp)
    gpn = mix(gp[:, 0]) * nx + mix(gp[:, 1]) * ny
    gpn_mag = mix(np.abs(gp[:, 0])) * np.abs(nx) + mix(np.abs(gp[:, 1])) * np.abs(ny)
    dpn = (p[n] - p[o]) / g.dist_n
    dpn_mag = (np.abs(p[n]) + np.abs(p[o])) / g.dist_n * g.qamp
    rc = dpf * (gpn - dpn)
    if "rhie_chow_sign" in wrong:
        rc = -rc
    F_int = c.rho * A * (un + rc)
    M_int = c.rho * A * (un_mag + np.abs(dpf) * (gpn_mag + dpn_mag))
    F_in, M_in = c.rho * (c.ub * nx) * A, c.rho * c.ub_mag * np.abs(nx) * A
    raw = c.rho * (u[o, 0] * nx + u[o, 1] * ny) * A
    M_out = c.rho * (np.abs(u[o, 0] * nx) + np.abs(u[o, 1] * ny)) * A
    F = np.select([g.kind == 0, g.kind == INLET, g.kind == OUTLET], [F_int, F_in, np.maximum(raw, 0.0)], 0.0)
    M = np.select([g.kind == 0, g.kind == INLET, g.kind == OUTLET], [M_int, M_in, M_out], 0.0)
    return F, M, raw, TOL_ROW * M_out


def check_flux(st, wrong=()):
    """Buffer 0 on every face.  Returns {faces, either, worst} and the face kinds seen."""
    c = Constants(st.constants, wrong)
    variants, either = [], 0
    for g in _geometries(st, wrong):
        F, M, raw, cb = flux64(g, c, st, wrong)
        err = st.flux - F
        out = g.kind == OUTLET
        near = out & (np.abs(raw) <= cb)  # the clamp may go either way
        err = np.where(near, np.where(np.abs(st.flux) < np.abs(err), st.flux, err), err)
        either = int(near.sum() + g.ambiguous.sum())
        variants.append((err, TOL_ROW * M))
    g = Geometry(st.arrays, wrong)
    worst = _judge("check_flux", variants,
                   lambda f: f"face {f} (kind {g.kind[f]}, cells {g.own[f]}, {g.nb[f]}): {st.flux[f]:.9e}")
    return {"faces": g.F, "either": either, "worst": worst,
            "kinds": {k: int((g.kind == k).sum()) for k in (0, INLET, OUTLET, WALL)},
            "degenerate": int(g.degenerate.sum()), "floored": int(g.floored.sum()), "turned": int(g.turned.sum())}


# -------------------------------------------------------------------- gradients
def gradients64(g, c, st, wrong=()):
    """{name: (gx, gy, Mx, My)} for u, v, p: Green-Gauss in float64 and the
    magnitudes of its terms."""
    cell, face, s, w, other = g.sides()
    kind, A = g.kind[face], g.area[face]
    anx, any_ = s * A * g.nx[face], s * A * g.ny[face]
    inner = kind == 0
    out = {}
    for name, phi in (("u", st.u[:, 0]), ("v", st.u[:, 1]), ("p", st.p)):
        vf = w * phi[cell] + (1.0 - w) * phi[other]
        vm = w * np.abs(phi[cell]) + (1.0 - w) * np.abs(phi[other])
        if name == "p":
            keep = kind != OUTLET if "outlet_p" not in wrong else kind != 99
            bv = np.where(keep, phi[cell], 0.0)
            bm = np.abs(bv)
        else:
            ub, ubm = (c.ub, c.ub_mag) if name == "u" else (0.0, 0.0)
            bv = np.select([kind == INLET, kind == OUTLET], [ub, phi[cell]], 0.0)
            bm = np.select([kind == INLET, kind == OUTLET], [ubm, np.abs(phi[cell])], 0.0)
        vf, vm = np.where(inner, vf, bv), np.where(inner, vm, bm)
        out[name] = (g.scatter(cell, vf * anx) / g.vol, g.scatter(cell, vf * any_) / g.vol,
                     g.scatter(cell, vm * np.abs(anx)) / g.vol, g.scatter(cell, vm * np.abs(any_)) / g.vol)
    return out


def check_gradients(st, wrong=()):
    """Buffers 1, 2, 10 on every cell.  Returns {cells, either, worst}."""
    c = Constants(st.constants, wrong)
    dev = {"u": st.grad_u, "v": st.grad_v, "p": st.grad_p}
    geos = _geometries(st, wrong)
    worst = 0.0
    for name in "uvp":
        for k in (0, 1):
            variants = []
            for g in geos:
                ref = gradients64(g, c, st, wrong)[name]
                variants.append((dev[name][:, k] - ref[k], g.cell_tol * ref[2 + k]))
            worst = max(worst, _judge(f"check_gradients grad {name} [{'xy'[k]}]", variants,
                                      lambda i: f"cell {i}: {dev[name][i, k]:.9e}"))
    return {"cells": geos[0].N, "either": int(geos[0].ambiguous.sum()), "worst": worst}


# -------------------------------------------------------------------------- d_p
def check_d_p(st, wrong=()):
    """get_d_p after prepare on every cell.  Returns {cells, worst}."""
    c = Constants(st.constants, wrong)
    g = Geometry(st.arrays, wrong)
    cell, face, s, _, _ = g.sides()
    kind = g.kind[face]
    dist = g.dist_n[face] if "d_p_dist_n" in wrong else g.dist_c[face]
    with np.errstate(divide="ignore"):
        diff = np.where(kind == OUTLET, 0.0, c.nu * g.area[face] / dist)
    D = c.a_t(g.vol) + g.scatter(cell, diff + np.maximum(s * st.flux[face], 0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = np.where(np.abs(D) > D_P_GUARD, g.vol / D, 0.0)
    worst = _judge("check_d_p", [(st.d_p - ref, g.cell_tol * np.abs(ref))], lambda i: f"cell {i}: {st.d_p[i]:.9e}")
    return {"cells": g.N, "worst": worst}


# ----------------------------------------------------------------------- matrix
def _stored_coupled(mesh, n_values):
    """(row, column) in the 3N x 3N matrix of every stored value of buffer 9, in
    storage order (the layout is fv_checks._coupled_csr's, by construction)."""
    T = fv._coupled_csr(mesh, np.arange(1.0, n_values + 1.0)).tocoo()
    order = np.argsort(T.data)
    assert np.array_equal(T.data[order], np.arange(1.0, n_values + 1.0))
    return T.row[order].astype(np.int64), T.col[order].astype(np.int64)


def _place(keys_stored, keys, values):
    """values (with repeated keys added up) laid out on the stored entries;
    every key must be stored."""
    order = np.argsort(keys_stored)
    pos = np.searchsorted(keys_stored[order], keys)
    assert np.all(pos < len(order)) and np.array_equal(keys_stored[order][pos], keys), \
        "f64 check_matrix_entries: the discretisation has an entry the matrix does not store"
    out = np.zeros(len(keys_stored))
    np.add.at(out, order[pos], values)
    return out


def matrix64(g, c, st, wrong=()):
    """(rows, cols, values, magnitudes) of the 3N x 3N coupled matrix as COO with
    repeats (to be added up), and the same of the N x N scalar matrix."""
    cell, face, s, w, other = g.sides()
    kind, A = g.kind[face], g.area[face]
    inner, inlet, outlet, wall = kind == 0, kind == INLET, kind == OUTLET, kind == WALL
    Fo = s * st.flux[face]
    dist = g.dist_c[face] if "matrix_dist_c" in wrong else g.dist_n[face]
    amp = g.qamp[face]
    with np.errstate(divide="ignore"):
        diff = c.nu * A / dist
    anx, any_ = A * s * g.nx[face], A * s * g.ny[face]
    dpf = np.where(inner, w * st.d_p[cell] + (1.0 - w) * st.d_p[other], st.d_p[cell])
    with np.errstate(divide="ignore"):
        lap = dpf * A / dist
    R, Cc, V, M = [], [], [], []

    def add(mask, r, col, val, mag):
        R.append(r[mask]), Cc.append(col[mask]), V.append(val[mask]), M.append(mag[mask])

    every = np.ones(g.N, dtype=bool)
    ids = np.arange(g.N)
    for k in (0, 1):  # u, v
        add(inner, 3 * cell + k, 3 * other + k, -diff + np.minimum(Fo, 0.0), diff * amp + np.abs(np.minimum(Fo, 0.0)))
        conv = np.where(wall, 0.0, np.maximum(Fo, 0.0))
        dg = np.where(outlet, 0.0, diff)
        add(every[cell], 3 * cell + k, 3 * cell + k, dg + conv, dg * amp + conv)
        add(every, 3 * ids + k, 3 * ids + k, c.a_t(g.vol), c.a_t(g.vol))
        an = anx if k == 0 else any_
        add(inner, 3 * cell + k, 3 * other + 2, (1.0 - w) * an, np.abs((1.0 - w) * an))
        add(inner, 3 * cell + 2, 3 * other + k, (1.0 - w) * an, np.abs((1.0 - w) * an))
        gw = np.where(inner, w, np.where(inlet | wall, 1.0, 0.0)) * an
        add(every[cell], 3 * cell + k, 3 * cell + 2, gw, np.abs(gw))
        dw = np.where(inner, w, np.where(outlet, 1.0, 0.0)) * an
        add(every[cell], 3 * cell + 2, 3 * cell + k, dw, np.abs(dw))
    add(inner, 3 * cell + 2, 3 * other + 2, -lap, np.abs(lap) * amp)
    pd = np.where(inner | outlet, lap, 0.0)
    add(every[cell], 3 * cell + 2, 3 * cell + 2, pd, np.abs(pd) * amp)
    coupled = tuple(np.concatenate(x) for x in (R, Cc, V, M))
    sc = (np.concatenate([cell[inner], cell]), np.concatenate([other[inner], cell]),
          c.rho * np.concatenate([-lap[inner], pd]),
          c.rho * np.concatenate([(np.abs(lap) * amp)[inner], np.abs(pd) * amp]))
    return coupled, sc


def check_matrix_entries(st, wrong=()):
    """Buffers 9 and 8: every stored entry of every row.  Returns {entries,
    scalar_entries, either, worst, upwind: internal sides with F_out > 0, < 0, == 0}."""
    c = Constants(st.constants, wrong)
    n3 = 3 * len(st.p)
    row, col = _stored_coupled(st.mesh, len(st.coupled))
    srow, scol = fv._scalar_csr_fast(st.mesh)
    skeys = np.repeat(np.arange(len(srow) - 1), np.diff(srow)) * len(st.p) + scol
    assert len(skeys) == len(st.scalar)
    v9, v8 = [], []
    geos = _geometries(st, wrong)
    for g in geos:
        (r, cc, v, m), (sr, scc, sv, sm) = matrix64(g, c, st, wrong)
        ref, mag = _place(row * n3 + col, r * n3 + cc, v), _place(row * n3 + col, r * n3 + cc, m)
        tol = np.where(row // 3 == col // 3, g.cell_tol[row // 3], TOL_ROW)  # the diagonal blocks are sums over faces
        v9.append((st.coupled - ref, tol * mag))
        ref, mag = _place(skeys, sr * len(st.p) + scc, sv), _place(skeys, sr * len(st.p) + scc, sm)
        tol = np.where(skeys // len(st.p) == skeys % len(st.p), g.cell_tol[skeys // len(st.p)], TOL_ROW)
        v8.append((st.scalar - ref, tol * mag))
    name = "uvp"
    worst = _judge("check_matrix_entries coupled", v9, lambda e: (
        f"A_{name[row[e] % 3]}{name[col[e] % 3]}[{row[e] // 3}, {col[e] // 3}] = {st.coupled[e]:.9e}"))
    worst = max(worst, _judge("check_matrix_entries scalar", v8, lambda e: f"entry {e}: {st.scalar[e]:.9e}"))
    g = geos[0]
    Fi = st.flux[g.internal]
    return {"entries": len(st.coupled), "scalar_entries": len(st.scalar), "worst": worst,
            "either": int(g.ambiguous.sum() + (Fi == 0.0).sum()),
            "upwind": (int((Fi > 0.0).sum()), int((Fi < 0.0).sum()), int((Fi == 0.0).sum()))}


# -------------------------------------------------------------------------- rhs
def rhs64(g, c, st, wrong=()):
    """(rhs [N, 3], magnitudes [N, 3]) in float64."""
    cell, face, s, w, other = g.sides()
    kind, A = g.kind[face], g.area[face]
    inner, inlet = kind == 0, kind == INLET
    Fo = s * st.flux[face]
    b, m = np.zeros((g.N, 3)), np.zeros((g.N, 3))
    tv = c.rho * g.vol / c.dt
    for k in (0, 1):
        if c.time_scheme == 1:
            b[:, k] = tv * ((1.0 + c.r) * st.u_old[:, k] - c.bdf2_old * st.u_old_old[:, k])
            m[:, k] = tv * ((1.0 + c.r) * np.abs(st.u_old[:, k]) + c.bdf2_old * np.abs(st.u_old_old[:, k]))
        else:
            b[:, k] = tv * st.u_old[:, k]
            m[:, k] = tv * np.abs(st.u_old[:, k])
    # inlet faces: u_b = (ub, 0)
    diff = c.nu * A / g.dist_n[face]
    b[:, 0] += g.scatter(cell[inlet], ((diff + np.maximum(-Fo, 0.0)) * c.ub)[inlet])
    m[:, 0] += g.scatter(cell[inlet], ((diff * g.qamp[face] + np.maximum(-Fo, 0.0)) * c.ub_mag)[inlet])
    b[:, 2] -= g.scatter(cell[inlet], (c.ub * s * g.nx[face] * A)[inlet])
    m[:, 2] += g.scatter(cell[inlet], (c.ub_mag * np.abs(g.nx[face]) * A)[inlet])
    if c.scheme != 0:
        up = np.where(Fo > 0.0, cell, other)
        dn = np.where(Fo > 0.0, other, cell)
        if c.scheme == 1:
            rx, ry = g.fx[face] - g.cx[up], g.fy[face] - g.cy[up]
        else:
            rx, ry = g.cx[dn] - g.cx[up], g.cy[dn] - g.cy[up]
        wu, wd = (0.375, 0.625) if "quick_swapped" in wrong else (0.625, 0.375)
        for k, grad in ((0, st.grad_u), (1, st.grad_v)):
            phi = st.u[:, k]
            gr, gr_mag = grad[up, 0] * rx + grad[up, 1] * ry, np.abs(grad[up, 0] * rx) + np.abs(grad[up, 1] * ry)
            if c.scheme == 1:
                d = gr
                dm = 2.0 * np.abs(phi[up]) + gr_mag
            else:
                d = wu * phi[up] + wd * phi[dn] + 0.125 * gr - phi[up]
                dm = wu * np.abs(phi[up]) + wd * np.abs(phi[dn]) + 0.125 * gr_mag + np.abs(phi[up])
            b[:, k] -= g.scatter(cell[inner], (Fo * d)[inner])
            m[:, k] += g.scatter(cell[inner], (np.abs(Fo) * dm)[inner])
    if st.buoyancy is not None:
        gx, gy, fields = st.buoyancy
        for beta, ref, phi in fields:
            beta, ref, phi = float(np.float32(beta)), float(np.float32(ref)), _f32(phi)
            fb = c.rho * g.vol * beta * (phi - ref)
            fm = c.rho * g.vol * abs(beta) * (np.abs(phi) + abs(ref))
            for k, gk in ((0, float(np.float32(gx))), (1, float(np.float32(gy)))):
                b[:, k] -= fb * gk
                m[:, k] += fm * abs(gk)
    return b, m


def check_rhs(st, wrong=()):
    """Buffer 3 on every row.  Returns {rows, either, worst}."""
    c = Constants(st.constants, wrong)
    variants = []
    geos = _geometries(st, wrong)
    for g in geos:
        b, m = rhs64(g, c, st, wrong)
        variants.append((st.rhs - b.reshape(-1), np.repeat(g.cell_tol, 3) * m.reshape(-1)))
    worst = _judge("check_rhs", variants, lambda e: f"row {e} (cell {e // 3}, {'uvp'[e % 3]}): {st.rhs[e]:.9e}")
    g = geos[0]
    return {"rows": len(st.rhs), "worst": worst,
            "either": int(g.ambiguous.sum() + (st.flux[g.internal] == 0.0).sum())}


# ----------------------------------------------------------------------- update
def check_update(constants, u_old, p_old, x, u_new, p_new):
    """u_new = u + alpha_u (x_u - u), p_new = p + alpha_p (x_p - p) on every
    cell; x: buffer 4, [N, 3] or flat.  Returns {cells, worst}."""
    c = Constants(constants)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    worst = 0.0
    for name, old, xs, new, al in (("u", u_old[:, 0], x[:, 0], u_new[:, 0], c.alpha_u),
                                   ("v", u_old[:, 1], x[:, 1], u_new[:, 1], c.alpha_u),
                                   ("p", p_old, x[:, 2], p_new, c.alpha_p)):
        ref = old + al * (xs - old)
        mag = np.abs(old) + al * (np.abs(xs) + np.abs(old))
        worst = max(worst, _judge(f"check_update {name}", [(new - ref, TOL_ROW * mag)],
                                  lambda i: f"cell {i}: {new[i]:.9e}"))
    return {"cells": len(p_old), "worst": worst}


def check_fold(u_before, p_before, u_after, p_after, reported_u, reported_p):
    """The reported outer max |du| and max |dp| are the f32 maxima of the f32
    differences of the fields around the last update, exactly."""
    f = np.float32
    du = np.abs(np.asarray(u_after, f) - np.asarray(u_before, f)).max()
    dp = np.abs(np.asarray(p_after, f) - np.asarray(p_before, f)).max()
    assert f(reported_u) == du, f"f64 check_fold: reported max |du| {reported_u!r} != {du!r}"
    assert f(reported_p) == dp, f"f64 check_fold: reported max |dp| {reported_p!r} != {dp!r}"
    return float(du), float(dp)
