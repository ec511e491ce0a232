"""Scheme 1 of the passive scalars ("limited linear": a van Leer-limited
linear-upwind face value as a deferred correction on phi_old, clamped to the
local extrema of phi_old) restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of scheme 1"), not
from the kernels, on top of tests/scalar_ref.py (coef, diag, the Jacobi sweep)
and tests/scalar_krylov_ref.py (method 1, which runs unchanged on the new b).
Every operation is one float32 rounding and every sum runs left to right in
slot order; the cell loops are vectorised across cells one slot at a time.

The slot geometry is rounded to float32 as csrc/host/topology.cpp does it:
    n_k     = the face normal cast from float64, negated for a non-owner
    dv_k    = the float32 centre difference (neighbour minus cell)
    lam_k   = d_o / (d_c + d_o), d_* = sqrt(dx*dx + dy*dy) from the cell's and
              the neighbour's centre to the face centre; d_c + d_o <= 1e-6
              (float32) marks the slot degenerate

`clamp=False` is a switch of the restatement only (the library has none): it
shows what the correction does without the clamp.

advance64_hr is the same scheme in float64 on the 1-D row of
scalar_ref.advance64: the discretisation alone, no mesh, no rounding model.
"""
from __future__ import annotations

import numpy as np

from tests.scalar_krylov_ref import ScalarKrylovRef
from tests.scalar_ref import F, NONE


class ScalarHRRef(ScalarKrylovRef):
    """assemble() returns scheme `scheme`'s system, so the inherited advance()
    and advance_krylov() run the scheme; `clamped` is the last assembly's count
    of cells the clamp changed."""

    def __init__(self, arrays, scheme=1, clamp=True):
        super().__init__(arrays)
        self.scheme, self.clamp, self.clamped = scheme, clamp, 0
        a = arrays
        face = self.face
        cell = np.arange(self.N)[:, None]
        cx, cy = a["cell_cx"].astype(F), a["cell_cy"].astype(F)
        fx, fy = a["face_cx"].astype(F)[face], a["face_cy"].astype(F)[face]
        Nx, Ny = a["face_nx"].astype(F)[face], a["face_ny"].astype(F)[face]
        self.nx = np.where(self.owner, Nx, -Nx)
        self.ny = np.where(self.owner, Ny, -Ny)
        ocx = np.where(self.internal, cx[self.other], fx)
        ocy = np.where(self.internal, cy[self.other], fy)
        self.dvx, self.dvy = ocx - cx[cell], ocy - cy[cell]

        def dist(ax, ay):
            dx, dy = ax - fx, ay - fy
            return np.sqrt(dx * dx + dy * dy)

        d_c, d_o = dist(cx[cell], cy[cell]), dist(ocx, ocy)
        tot = d_c + d_o
        ok = tot > F(1e-6)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.lam = np.where(ok, d_o / tot, F(0.5)).astype(F)
        self.degen = self.internal & ~ok
        for v in (self.nx, self.ny, self.dvx, self.dvy, self.lam, d_c, tot):
            assert v.dtype == F

    def gradient(self, phi, inlet_value):
        """g = (gx, gy) [N] each: Green-Gauss with the face values of the step's own gradients"""
        phi, inlet_value = np.asarray(phi, F), F(inlet_value)
        gx, gy = np.zeros(self.N, F), np.zeros(self.N, F)
        for k in range(self.S):
            m = self.used[:, k]
            po = phi[self.other[:, k]]
            lam = self.lam[:, k]
            vint = np.where(self.degen[:, k], F(0.5) * (phi + po), lam * phi + (F(1) - lam) * po)
            vf = np.where(self.internal[:, k], vint, np.where(self.inlet[:, k], inlet_value, phi)).astype(F)
            gx[m] = gx[m] + (vf * self.nx[:, k] * self.area[:, k])[m]
            gy[m] = gy[m] + (vf * self.ny[:, k] * self.area[:, k])[m]
        out = gx / self.vol, gy / self.vol
        assert out[0].dtype == F
        return out

    def correction(self, Fk, phi, gx, gy):
        """corr_i = sum over the internal slots with F != 0 of F_k * h_k, from +0"""
        corr = np.zeros(self.N, F)
        with np.errstate(all="ignore"):
            for k in range(self.S):
                o = self.other[:, k]
                Fm, po = Fk[:, k], phi[o]
                own, neg = Fm > 0, Fm < 0
                d = np.where(own, po - phi, phi - po)
                dot = np.where(own, gx, gx[o]) * self.dvx[:, k] + np.where(own, gy, gy[o]) * self.dvy[:, k]
                gd = np.where(own, dot, -dot)
                r = (F(2) * gd) / d - F(1)
                psi = np.where(r > 0, F(2) / (F(1) + F(1) / r), F(0))
                h = np.where(d != 0, (F(0.5) * psi) * d, F(0)).astype(F)
                act = self.internal[:, k] & (own | neg)
                corr[act] = corr[act] + (Fm * h)[act]
        assert corr.dtype == F
        return corr

    def assemble(self, face_flux, density, dt, D, inlet_value, phi_old):
        coef, diag, b0 = super().assemble(face_flux, density, dt, D, inlet_value, phi_old)
        self.clamped = 0
        if self.scheme == 0:
            return coef, diag, b0
        f = np.asarray(face_flux, F)[self.face]
        Fk = np.where(self.owner, f, -f)
        phi, inlet = np.asarray(phi_old, F), F(inlet_value)
        a_t = self.vol * F(density) / F(dt)
        gx, gy = self.gradient(phi, inlet)
        corr = self.correction(Fk, phi, gx, gy)
        mn, mx = phi.copy(), phi.copy()
        for k in range(self.S):
            v = np.where(self.inlet[:, k], inlet, phi[self.other[:, k]])
            on = self.internal[:, k] | self.inlet[:, k]
            mn = np.where(on & (v < mn), v, mn)
            mx = np.where(on & (v > mx), v, mx)
        t = a_t * phi - corr
        if self.clamp:
            lo, hi = a_t * mn, a_t * mx
            below, above = t < lo, t > hi
            self.clamped = int(np.count_nonzero(below | above))
            t = np.where(below, lo, np.where(above, hi, t))
        b = t.astype(F)
        for k in range(self.S):
            m = self.inlet[:, k]
            b[m] = b[m] + coef[m, k] * inlet
        assert b.dtype == F
        return coef, diag, b


def row_arrays(n):
    """Mesh arrays of the row of tests/test_scalar.py (n unit cells, inlet left,
    outlet right, walls above and below) with the face normals added, and its
    by-face flux of one unit left to right."""
    own, nb, bnd, fx, fy, nx, ny = [], [], [], [], [], [], []
    for j in range(n + 1):
        if j == 0:
            own.append(0), nb.append(NONE), bnd.append(1), nx.append(-1.0)
        elif j == n:
            own.append(n - 1), nb.append(NONE), bnd.append(2), nx.append(1.0)
        else:
            own.append(j - 1), nb.append(j), bnd.append(0), nx.append(1.0)
        fx.append(float(j)), fy.append(0.5), ny.append(0.0)
    for i in range(n):
        for y in (0.0, 1.0):
            own.append(i), nb.append(NONE), bnd.append(3)
            fx.append(i + 0.5), fy.append(y), nx.append(0.0), ny.append(2.0 * y - 1.0)
    cells = [[i, i + 1, n + 1 + 2 * i, n + 2 + 2 * i] for i in range(n)]
    arrays = dict(face_owner=np.array(own, np.uint32), face_neighbor=np.array(nb, np.uint32),
                  face_boundary=np.array(bnd, np.uint32), face_area=np.ones(len(own)), face_cx=np.array(fx),
                  face_cy=np.array(fy), face_nx=np.array(nx), face_ny=np.array(ny), cell_cx=np.arange(n) + 0.5,
                  cell_cy=np.full(n, 0.5), cell_vol=np.ones(n), cell_face_offsets=np.arange(0, 4 * n + 1, 4, dtype=np.uint32),
                  cell_faces=np.array(cells, np.uint32).reshape(-1))
    flux = np.zeros(len(own), np.float32)
    flux[1:n + 1] = 1.0
    flux[0] = -1.0
    return arrays, flux


def advance64_hr(n, flux, vol, density, dt, D, inlet_value, phi, sweeps=400, clamp=True):
    """Scheme 1 in float64 on the row of scalar_ref.advance64 (n cells, one
    uniform flux > 0 through every face, left boundary an inlet, right boundary
    an outlet, unit areas and distances; slot order left, right).  Returns
    (phi after one implicit step by `sweeps` Jacobi sweeps, clamped cells)."""
    assert flux > 0
    phi = np.asarray(phi, np.float64)
    a_t = vol * density / dt
    diff = density * D
    c_left = flux + diff  # the left slot's flux out of the cell is -flux
    c_right = diff        # internal right slots; the outlet slot has c = 0
    diag = np.full(n, a_t + c_left + c_right)
    diag[-1] = a_t + c_left
    # gradient: face values inlet_value | 0.5 (phi_i + phi_o) | phi_i (outlet), normals -1 and +1
    vf = np.concatenate([[inlet_value], 0.5 * (phi[:-1] + phi[1:]), [phi[-1]]])
    g = (vf[1:] - vf[:-1]) / vol

    def h(d, gd):
        with np.errstate(all="ignore"):
            r = 2.0 * gd / d - 1.0
            psi = np.where(r > 0, 2.0 / (1.0 + 1.0 / r), 0.0)
            return np.where(d != 0, 0.5 * psi * d, 0.0)

    corr = np.zeros(n)
    # left slot (F = -flux < 0, the left neighbour is upwind, dv = -1): cells 1 .. n-1
    corr[1:] += -flux * h(phi[1:] - phi[:-1], -(g[:-1] * -1.0))
    # right slot (F = +flux > 0, this cell is upwind, dv = +1): cells 0 .. n-2
    corr[:-1] += flux * h(phi[1:] - phi[:-1], g[:-1] * 1.0)
    lft = np.concatenate([[inlet_value], phi[:-1]])
    rgt = np.concatenate([phi[1:], [phi[-1]]])
    mn, mx = np.minimum(phi, np.minimum(lft, rgt)), np.maximum(phi, np.maximum(lft, rgt))
    t = a_t * phi - corr
    clamped = 0
    if clamp:
        lo, hi = a_t * mn, a_t * mx
        clamped = int(np.count_nonzero((t < lo) | (t > hi)))
        t = np.where(t < lo, lo, np.where(t > hi, hi, t))
    b = t
    b[0] += c_left * inlet_value
    x = phi.copy()
    for _ in range(sweeps):
        s = b.copy()
        s[1:] += c_left * x[:-1]
        s[:-1] += c_right * x[1:]
        x = s / diag
    return x, clamped
