"""Passive scalar transport restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the discretisation in include/cfd2_amd.h (the passive-scalar
section), not from the kernels.  Per owned cell i, with face slot k of cell i
= cell_faces[cell_face_offsets[i] + k], every operation one float32 rounding
and every sum left to right in slot order:

    F_k    = +f for the face's owner, -f otherwise (f = the by-face flux)
    a_t    = (vol_i * density) / dt
    diff_k = ((density * D) * A_k) / d_k
    cin_k  = -F_k if F_k < 0 else 0
    c_k    = cin_k + diff_k on internal and inlet (boundary type 1) slots, else 0
    diag_i = ((a_t + c_0) + c_1) + ...
    b_i    = a_t * phi_old_i, then + c_k * inlet_value per inlet slot
    sweep  phi_i <- (b_i + c_k0 * phi[o_k0] + c_k1 * phi[o_k1] ...) / diag_i
           over the internal slots only, the sum starting from b_i

The geometry is rounded to float32 as csrc/host/topology.cpp does it: centres,
areas and volumes cast from float64, d_k = sqrt(dx*dx + dy*dy) of the float32
centre differences (a boundary slot's "other centre" is its face centre).
The cell loops are vectorised across cells one slot at a time, which keeps
each cell's accumulation order.
"""
from __future__ import annotations

import numpy as np

F = np.float32
NONE = 0xFFFFFFFF


class ScalarRef:
    def __init__(self, arrays):
        """arrays: Mesh.arrays() (or any dict with the same keys)"""
        a = arrays
        self.N = N = len(a["cell_vol"])
        own = a["face_owner"].astype(np.int64)
        nb = a["face_neighbor"].astype(np.int64)
        bt = a["face_boundary"].astype(np.int64) & 3
        area = a["face_area"].astype(F)
        fx, fy = a["face_cx"].astype(F), a["face_cy"].astype(F)
        cx, cy = a["cell_cx"].astype(F), a["cell_cy"].astype(F)
        self.vol = a["cell_vol"].astype(F)
        offs = a["cell_face_offsets"].astype(np.int64)
        cf = a["cell_faces"].astype(np.int64)
        self.nface = nface = np.diff(offs)
        self.S = K = int(nface.max())  # the mesh's maximum face count
        cell = np.arange(N)[:, None]
        k = np.arange(K)[None, :]
        self.used = used = k < nface[:, None]
        face = cf[np.minimum(offs[:-1, None] + k, len(cf) - 1)]
        self.face = np.where(used, face, 0)
        face = self.face
        self.owner = own[face] == cell
        self.internal = used & (nb[face] != NONE)
        self.inlet = used & ~self.internal & (bt[face] == 1)
        self.other = np.where(self.internal, np.where(self.owner, nb[face], own[face]), 0)
        ocx = np.where(self.internal, cx[self.other], fx[face])
        ocy = np.where(self.internal, cy[self.other], fy[face])
        dvx, dvy = ocx - cx[cell], ocy - cy[cell]
        with np.errstate(invalid="ignore"):
            self.dist = np.sqrt(dvx * dvx + dvy * dvy).astype(F)
        self.area = area[face]

    # ---- float32: what the device computes ---------------------------------
    def assemble(self, face_flux, density, dt, D, inlet_value, phi_old):
        """(coef [N, S], diag [N], b [N]) in float32"""
        f = np.asarray(face_flux, F)[self.face]
        Fk = np.where(self.owner, f, -f)
        density, dt, D, inlet_value = F(density), F(dt), F(D), F(inlet_value)
        phi_old = np.asarray(phi_old, F)
        a_t = self.vol * density / dt
        rd = density * D
        with np.errstate(divide="ignore", invalid="ignore"):
            diff = rd * self.area / self.dist
        cin = np.where(Fk < 0, -Fk, F(0))
        coef = np.where(self.internal | self.inlet, cin + diff, F(0)).astype(F)
        diag = a_t.copy()
        b = a_t * phi_old
        for k in range(self.S):
            diag = diag + coef[:, k]
            m = self.inlet[:, k]
            b[m] = b[m] + coef[m, k] * inlet_value
        assert coef.dtype == F and diag.dtype == F and b.dtype == F
        return coef, diag, b

    def sweep(self, coef, diag, b, phi):
        s = b.copy()
        for k in range(self.S):
            m = self.internal[:, k]
            s[m] = s[m] + coef[m, k] * phi[self.other[m, k]]
        out = s / diag
        assert out.dtype == F
        return out

    def advance(self, face_flux, density, dt, D, inlet_value, phi, tol=1e-6, max_sweeps=200, check_interval=4):
        """one implicit step: (phi, sweeps, last delta (float32), converged)"""
        phi = np.asarray(phi, F)
        coef, diag, b = self.assemble(face_flux, density, dt, D, inlet_value, phi)
        ci = int(check_interval)
        max_sweeps = -(-int(max_sweeps) // ci) * ci
        sweeps, delta, converged = 0, F(0), False
        while sweeps < max_sweeps:
            for _ in range(ci):
                prev = phi
                phi = self.sweep(coef, diag, b, prev)
            sweeps += ci
            d = np.abs(phi - prev)
            delta = F(np.inf) if np.isnan(d).any() else F(d.max())
            if not np.isfinite(delta):
                raise FloatingPointError("non-finite Jacobi update")
            if delta <= F(tol):
                converged = True
                break
        return phi, sweeps, delta, converged

    # ---- float64: the same system (its float32 coefficients), rows evaluated in float64
    def residual64(self, coef, diag, b, phi):
        """max_i |b_i + sum_k c_k phi_other(k) - diag_i phi_i| / diag_i in float64"""
        c, d, rhs, p = (np.asarray(x, np.float64) for x in (coef, diag, b, phi))
        s = rhs.copy()
        for k in range(self.S):
            m = self.internal[:, k]
            s[m] += c[m, k] * p[self.other[m, k]]
        return float(np.max(np.abs(s - d * p) / d))


def advance64(n, flux, vol, density, dt, D, inlet_value, phi, sweeps=400):
    """The operator in float64 on a 1-D row of n cells with one uniform flux
    through every face (left boundary an inlet, right boundary an outlet, unit
    areas and distances): the discretisation alone, no mesh and no rounding
    model.  Returns phi after one implicit step (Jacobi, `sweeps` sweeps)."""
    phi = np.asarray(phi, np.float64)
    a_t = vol * density / dt
    diff = density * D
    c_left = max(flux, 0.0) + diff    # the left slot's flux out of the cell is -flux
    c_right = max(-flux, 0.0) + diff  # internal right slots; the outlet slot has c = 0
    diag = np.full(n, a_t + c_left + c_right)
    diag[-1] = a_t + c_left
    b = a_t * phi
    b[0] += c_left * inlet_value
    x = phi.copy()
    for _ in range(sweeps):
        s = b.copy()
        s[1:] += c_left * x[:-1]
        s[:-1] += c_right * x[1:]
        x = s / diag
    return x
