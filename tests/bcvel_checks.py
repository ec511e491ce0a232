"""Float64 checks of prescribed boundary velocities, written face by face from
the discretisation (include/cfd2_amd.h "Arithmetic of boundary velocities" names
the terms) and not from tests/bcvel_ref.py or the kernels.

HELPER MODULE, not a test.  Of tests/flow_checks.py it takes the mesh by faces
(Geometry: f32-rounded arrays widened, the flux normal, the owner's weight, the
two distances) and the constants; nothing of refpy.py or bcvel_ref.py.

The boundary velocity of a face, in float64:
    selected   ub = b * scale * ramp,  b = the f32 upload: for a wall face
               v - (v . n) n / (n . n) formed in float64 from the f32 (vx, vy)
               and the f64 normal, then rounded to f32 (`uploaded`)
    unselected inlet (inlet_velocity * ramp, 0);  unselected wall (0, 0)
    ramp = t^2 (3 - 2 t), t = clamp(time / ramp_time, 0, 1)
In f32 ub takes at most 7 roundings (t, t^2, 3 - 2t, their product, scale *
ramp, b * g, and the clamp none): K_UB = 7.

check_inlet_flux   every inlet face: F = rho (ub . nf) A.  Two products, their
    sum, times rho, times A on top of ub: bound 12 eps32 rho A (|ubx nfx| + |uby nfy|).
check_gradients    every cell: g = (1 / V) sum_f phi_f s A n with phi_f the
    interpolated value (internal), ub (inlet, selected wall), 0 (wall), u_i
    (outlet).  The face value carries at most 11 roundings (the weight 8, two
    products and a sum), times n, times A, the running sum one per face, the
    division one: bound (14 + faces_i) eps32 (1 / V) sum_f |phi_f| A |n|.
check_rhs          scheme 0, every row, the complete right-hand side:
    momentum   a_t u^n (BDF2: the two-level form) + sum over inlet faces (nu A /
               dist_n + max(-F_out, 0)) ub + sum over selected wall faces (nu A /
               dist_n) ub
    continuity -sum over inlet faces (ub . s n) A
    Per term: the time term 10 roundings, a boundary term 11 + 3 qamp (qamp: what
    a quotient by dist_n counts for, flow_checks), the running sum one per face:
    bound eps32 sum_terms (k_term + faces_i + 1) |term|.
check_wall_sums    the force region, in float64 on the device: F_p = p n A, F_v =
    nu (u - ub) A / dist_c, the torques r x F about (x0, y0), power = -sum (F_p +
    F_v) . ub over the selected faces.  The device works in f64 on f32 inputs;
    what is left is ub (7) and dist_c (a f32 root of a sum of squares: 5):
    bound 16 eps32 times the sum of the magnitudes of the terms.

WRONG (test_bcvel.py shows each is caught): "wall_sign" the wall term
subtracted, "no_uby" uby dropped at the inlet, "ramp_twice" the ramp applied
twice, "no_projection" the normal component kept.
"""
import numpy as np

from tests import flow_checks as fc

EPS32 = fc.EPS32
K_UB = 7
WRONG = ("wall_sign", "no_uby", "ramp_twice", "no_projection")


def uploaded(arrays, faces, v, wrong=()):
    """the f32 (bx, by) the host uploads for `faces` with the requested v [n, 2], widened"""
    a = arrays
    v = np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    nx, ny = a["face_nx"][faces].astype(np.float64), a["face_ny"][faces].astype(np.float64)
    wall = (a["face_boundary"][faces] & 3) == fc.WALL
    vn = (v[:, 0] * nx + v[:, 1] * ny) / (nx * nx + ny * ny)
    if "no_projection" in wrong:
        vn = 0.0 * vn
    out = np.where(wall[:, None], v - vn[:, None] * np.stack([nx, ny], 1), v)
    return out.astype(np.float32).astype(np.float64)


class Boundary:
    """ub [F, 2], its magnitude bound, and the selection by face."""

    def __init__(self, g, constants, faces, b, scales, wrong=()):
        c = constants
        f = lambda v: float(np.float32(v))  # noqa: E731
        t = min(max(f(c.time) / f(c.ramp_time), 0.0), 1.0)
        ramp = t * t * (3.0 - 2.0 * t)
        self.sel = np.zeros(g.F, bool)
        self.sel[faces] = True
        self.ub = np.zeros((g.F, 2))
        self.ub[g.kind == fc.INLET, 0] = f(c.inlet_velocity) * ramp
        gain = np.where(g.kind[faces] == fc.INLET, f(scales[0]), f(scales[1])) * ramp
        if "ramp_twice" in wrong:
            gain = gain * ramp
        self.ub[faces] = b * gain[:, None]
        if "no_uby" in wrong:
            self.ub[g.kind == fc.INLET, 1] = 0.0
        self.wall_sign = -1.0 if "wall_sign" in wrong else 1.0
        self.active = (g.kind == fc.INLET) | (self.sel & (g.kind == fc.WALL))  # faces whose ub enters


def _judge(what, err, bound, label):
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0.0, 0.0, np.abs(err) / bound)
    if r.size == 0:
        return 0.0
    w = int(np.argmax(r))
    assert r[w] <= 1.0, f"f64 {what}: {label} {w}: |error| {abs(err[w]):.3e} > bound {bound[w]:.3e} ({r[w]:.2f} x)"
    return float(r[w])


def check_inlet_flux(g, c, B, flux):
    f = np.nonzero(g.kind == fc.INLET)[0]
    tx, ty = B.ub[f, 0] * g.fnx[f], B.ub[f, 1] * g.fny[f]
    F = c.rho * (tx + ty) * g.area[f]
    M = c.rho * (np.abs(tx) + np.abs(ty)) * g.area[f]
    return _judge("inlet flux", flux[f] - F, 12 * EPS32 * M, "inlet face")


def check_gradients(g, B, u, grad_u, grad_v):
    cell, face, s, w, other = g.sides()
    worst = 0.0
    for comp, got in ((0, grad_u), (1, grad_v)):
        q = u[:, comp]
        kind = g.kind[face]
        phi = np.where(kind == 0, w * q[cell] + (1.0 - w) * q[other],
                       np.where(B.active[face], B.ub[face, comp], np.where(kind == fc.OUTLET, q[cell], 0.0)))
        mag = np.where(kind == 0, w * np.abs(q[cell]) + (1.0 - w) * np.abs(q[other]), np.abs(phi))
        nfaces = g.scatter(cell, 1.0)
        for d, n in ((0, g.nx), (1, g.ny)):
            val = g.scatter(cell, phi * s * g.area[face] * n[face]) / g.vol
            M = g.scatter(cell, mag * g.area[face] * np.abs(n[face])) / g.vol
            worst = max(worst, _judge(f"gradient of u{comp} d{d}", got[:, d] - val, (14 + nfaces) * EPS32 * M, "cell"))
    return worst


def check_rhs(g, c, B, flux, u_old, u_old_old, rhs):
    """scheme 0: the complete right-hand side of every row"""
    assert c.scheme == 0
    rhs = rhs.reshape(-1, 3)
    base = g.vol * c.rho / c.dt
    nfaces = g.scatter(np.concatenate([g.own, g.nb[g.internal]]), 1.0)
    bf = np.nonzero(B.active)[0]  # boundary faces: owned by their cell, s = +1, F_out = F
    o = bf
    cells = g.own[bf]
    diff = c.nu * g.area[bf] / g.dist_n[bf]
    inflow = np.where(g.kind[bf] == fc.INLET, np.maximum(-flux[bf], 0.0), 0.0)
    sign = np.where(g.kind[bf] == fc.WALL, B.wall_sign, 1.0)
    worst = 0.0
    for comp in (0, 1):
        if c.time_scheme == 1:
            t = base * ((1.0 + c.r) * u_old[:, comp] - c.bdf2_old * u_old_old[:, comp])
            tm = base * ((1.0 + c.r) * np.abs(u_old[:, comp]) + c.bdf2_old * np.abs(u_old_old[:, comp]))
        else:
            t, tm = c.a_t(g.vol) * u_old[:, comp], c.a_t(g.vol) * np.abs(u_old[:, comp])
        ub = B.ub[o, comp]
        val = t + g.scatter(cells, sign * diff * ub + inflow * ub)
        bound = EPS32 * ((10 + nfaces + 1) * tm
                         + g.scatter(cells, (11 + 3 * g.qamp[bf] + nfaces[cells] + 1) * (diff + inflow) * np.abs(ub)))
        worst = max(worst, _judge(f"rhs of u{comp}", rhs[:, comp] - val, bound, "row"))
    inl = np.nonzero(g.kind == fc.INLET)[0]
    tx, ty = B.ub[inl, 0] * g.nx[inl], B.ub[inl, 1] * g.ny[inl]
    val = -g.scatter(g.own[inl], (tx + ty) * g.area[inl])
    bound = EPS32 * g.scatter(g.own[inl], (K_UB + 4 + nfaces[g.own[inl]]) * (np.abs(tx) + np.abs(ty)) * g.area[inl])
    return max(worst, _judge("rhs of p", rhs[:, 2] - val, bound, "row"))


def check_wall_sums(g, c, B, arrays, region, u, p, x0, y0, force_viscous, motion):
    """region: bool [F], the wall faces of the force region; force_viscous: (fx, fy) of
    cfd_flow_diag; motion: (torque_pressure, torque_viscous, power).  Returns the worst ratio."""
    f = np.nonzero(region)[0]
    o = g.own[f]
    A, d = g.area[f], g.dist_c[f]
    ub = np.where(B.sel[f][:, None], B.ub[f], 0.0)
    Fp = (p[o] * A)[:, None] * np.stack([g.nx[f], g.ny[f]], 1)
    Fv = (c.nu * A / d)[:, None] * (u[o] - ub)
    Fv_mag = (c.nu * A / d)[:, None] * (np.abs(u[o]) + np.abs(ub))
    r = np.stack([arrays["face_cx"][f] - x0, arrays["face_cy"][f] - y0], 1)
    k = 16 * EPS32
    worst = 0.0
    for comp in (0, 1):
        worst = max(worst, _judge(f"viscous force {comp}", np.array([force_viscous[comp] - Fv[:, comp].sum()]),
                                  np.array([k * Fv_mag[:, comp].sum()]), "sum"))
    cross = lambda a, b: a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]  # noqa: E731
    cross_mag = lambda a, b: np.abs(a[:, 0] * b[:, 1]) + np.abs(a[:, 1] * b[:, 0])  # noqa: E731
    worst = max(worst, _judge("pressure torque", np.array([motion[0] - cross(r, Fp).sum()]),
                              np.array([k * cross_mag(r, Fp).sum()]), "sum"))
    worst = max(worst, _judge("viscous torque", np.array([motion[1] - cross(r, Fv).sum()]),
                              np.array([k * cross_mag(r, Fv_mag).sum()]), "sum"))
    power = -((Fp + Fv) * ub).sum()
    power_mag = ((np.abs(Fp) + Fv_mag) * np.abs(ub)).sum()
    return max(worst, _judge("power", np.array([motion[2] - power]), np.array([k * power_mag]), "sum"))
