"""Wall conditions, sources and the wall-flux sums of the passive scalars
restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of wall conditions
and sources"), not from the kernels, on top of the unchanged
tests/scalar_hr_ref.py: a field without a selected face and without a source
cell is handed to ScalarHRRef.assemble as it stands.  Every operation is one
float32 rounding and every sum runs left to right in slot order; the cell loops
are vectorised across cells one slot at a time.

Selection, in float64 on the mesh arrays as the library does it on the mesh
view: a wall face (boundary type 3) is selected when its centre lies in the
closed box, a cell is a source cell when its centre does; x1 < x0 selects
nothing.

The pieces a deliberately wrong variant replaces (tests/test_scalar_bc.py) are
methods or attributes of their own: wall_dist, flux_term, source_term,
range_takes_wall, grad_takes_wall, flux_field.
"""
from __future__ import annotations

import numpy as np

from tests import refpy
from tests.scalar_hr_ref import ScalarHRRef
from tests.scalar_ref import F, NONE

KINDS = {"adiabatic": 0, "value": 1, "flux": 2}
NO_BOX = (0.0, 0.0, -1.0, 0.0)


def in_box(x, y, box):
    x0, y0, x1, y1 = (float(v) for v in box)
    if x1 < x0:
        return np.zeros(len(x), bool)
    return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


class ScalarBCRef(ScalarHRRef):
    range_takes_wall = True  # scheme 1: the clamp's range takes `value` on a kind-1 slot
    grad_takes_wall = True   # scheme 1: the gradient's face value on a kind-1 slot is `value`

    def __init__(self, arrays, scheme=1, clamp=True):
        super().__init__(arrays, scheme=scheme, clamp=clamp)
        a = arrays
        bt = a["face_boundary"].astype(np.int64) & 3
        wall_face = (a["face_neighbor"].astype(np.int64) == NONE) & (bt == 3)
        self.wallslot = self.used & ~self.internal & wall_face[self.face]
        self._fcx, self._fcy = a["face_cx"].astype(np.float64), a["face_cy"].astype(np.float64)
        self._ccx, self._ccy = a["cell_cx"].astype(np.float64), a["cell_cy"].astype(np.float64)
        self.wall_dist = self.dist
        self.set_wall(0, 0.0, NO_BOX)
        self.set_source(0.0, NO_BOX)

    # ---- selection ----------------------------------------------------------
    def set_wall(self, kind, value, box):
        """returns the wall faces in the box"""
        self.kind = KINDS.get(kind, kind)
        assert self.kind in (0, 1, 2)
        self.value = F(value)
        inb = self.wallslot & in_box(self._fcx, self._fcy, box)[self.face]
        self.faces = int(np.count_nonzero(inb))
        if self.kind != 0:
            assert not inb[:, 31:].any(), "a selected wall face at slot 31 or above"
        self.sel = inb if self.kind != 0 else np.zeros_like(inb)
        return self.faces

    def set_source(self, rate, box):
        """returns the cells in the box"""
        self.rate = F(rate)
        inb = in_box(self._ccx, self._ccy, box)
        self.cells = int(np.count_nonzero(inb))
        self.src = inb if self.rate != 0 else np.zeros_like(inb)
        return self.cells

    @property
    def plain(self):
        return not self.sel.any() and not self.src.any()

    # ---- the terms ----------------------------------------------------------
    def wall_coef(self, density, D):
        """c_k of a fixed-value wall slot, [N, S]: (density * D) * A_k / d_k"""
        rd = F(density) * F(D)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = rd * self.area / self.wall_dist
        assert c.dtype == F
        return c

    def flux_term(self, k):
        """a fixed-flux slot's term of b: value * A_k"""
        return self.value * self.area[:, k]

    def source_term(self):
        return self.vol * self.rate

    def _late_terms(self, b, coef, inlet_value):
        """b, then in ascending slot order the inlet, kind-1 and kind-2 terms, the source last"""
        for k in range(self.S):
            m = self.inlet[:, k]
            b[m] = b[m] + coef[m, k] * inlet_value
            m = self.sel[:, k]
            if self.kind == 1:
                b[m] = b[m] + coef[m, k] * self.value
            elif self.kind == 2:
                b[m] = b[m] + self.flux_term(k)[m]
        m = self.src
        b[m] = b[m] + self.source_term()[m]
        assert b.dtype == F
        return b

    def gradient(self, phi, inlet_value):
        if self.kind != 1 or not self.grad_takes_wall or not self.sel.any():
            return super().gradient(phi, inlet_value)
        phi, inlet_value = np.asarray(phi, F), F(inlet_value)
        gx, gy = np.zeros(self.N, F), np.zeros(self.N, F)
        for k in range(self.S):
            m = self.used[:, k]
            po = phi[self.other[:, k]]
            lam = self.lam[:, k]
            vint = np.where(self.degen[:, k], F(0.5) * (phi + po), lam * phi + (F(1) - lam) * po)
            vbnd = np.where(self.inlet[:, k], inlet_value, np.where(self.sel[:, k], self.value, phi))
            vf = np.where(self.internal[:, k], vint, vbnd).astype(F)
            gx[m] = gx[m] + (vf * self.nx[:, k] * self.area[:, k])[m]
            gy[m] = gy[m] + (vf * self.ny[:, k] * self.area[:, k])[m]
        out = gx / self.vol, gy / self.vol
        assert out[0].dtype == F
        return out

    def assemble(self, face_flux, density, dt, D, inlet_value, phi_old):
        if self.plain:
            return super().assemble(face_flux, density, dt, D, inlet_value, phi_old)
        f = np.asarray(face_flux, F)[self.face]
        Fk = np.where(self.owner, f, -f)
        density, dt, D, inlet = F(density), F(dt), F(D), F(inlet_value)
        phi = np.asarray(phi_old, F)
        a_t = self.vol * density / dt
        rd = density * D
        with np.errstate(divide="ignore", invalid="ignore"):
            diff = rd * self.area / self.dist
        cin = np.where(Fk < 0, -Fk, F(0))
        coef = np.where(self.internal | self.inlet, cin + diff, F(0)).astype(F)
        if self.kind == 1:
            coef = np.where(self.sel, self.wall_coef(density, D), coef).astype(F)
        diag = a_t.copy()
        for k in range(self.S):
            diag = diag + coef[:, k]
        self.clamped = 0
        if self.scheme == 0:
            b = self._late_terms(a_t * phi, coef, inlet)
            assert coef.dtype == F and diag.dtype == F
            return coef, diag, b
        gx, gy = self.gradient(phi, inlet)
        corr = self.correction(Fk, phi, gx, gy)
        mn, mx = phi.copy(), phi.copy()
        wall_v = self.sel if (self.kind == 1 and self.range_takes_wall) else np.zeros_like(self.sel)
        for k in range(self.S):
            v = np.where(self.inlet[:, k], inlet, np.where(wall_v[:, k], self.value, phi[self.other[:, k]]))
            on = self.internal[:, k] | self.inlet[:, k] | wall_v[:, k]
            mn = np.where(on & (v < mn), v, mn)
            mx = np.where(on & (v > mx), v, mx)
        t = a_t * phi - corr
        if self.clamp:
            lo, hi = a_t * mn, a_t * mx
            below, above = t < lo, t > hi
            self.clamped = int(np.count_nonzero(below | above))
            t = np.where(below, lo, np.where(above, hi, t))
        b = self._late_terms(t.astype(F), coef, inlet)
        return coef, diag, b

    # ---- the wall-flux sums -------------------------------------------------
    def flux_field(self, phi, phi_old):
        """the field the wall flux is evaluated on: the current one"""
        return phi

    def wall_flux(self, density, D, phi, phi_old=None):
        """(flux, area, phi_area): per cell in float64 in slot order over the
        selected slots, the cells in the canonical order"""
        if self.kind == 0 or not self.sel.any():
            return 0.0, 0.0, 0.0
        ph = np.asarray(self.flux_field(phi, phi_old), F).astype(np.float64)
        c = self.wall_coef(density, D).astype(np.float64)
        area = self.area.astype(np.float64)
        t = np.zeros((3, self.N))
        for k in range(self.S):
            m = self.sel[:, k]
            if self.kind == 1:
                t[0, m] += c[m, k] * (float(self.value) - ph[m])
            else:
                t[0, m] += float(self.value) * area[m, k]
            t[1, m] += area[m, k]
            t[2, m] += area[m, k] * ph[m]
        return tuple(float(refpy.canon_sum(t[j])) for j in range(3))
