"""Boussinesq buoyancy restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of buoyancy"), not
from the kernels, on top of the unchanged tests/refpy.py (the coupled step) and
tests/scalar_ref.py through tests/scalar_bc_ref.py (the scalar fields, scheme
0, with their wall conditions).  Per owned cell, after the assembly
refpy.assemble restates, over the fields with beta != 0 in ascending order,
every operation one float32 rounding:

    d  = phi_f[i] - ref_f
    fb = (vol_i * density) * (beta_f * d)
    rhs_u = rhs_u - fb * g_x
    rhs_v = rhs_v - fb * g_y

and nothing when no field drives or g = (0, 0).  step() wraps refpy.assemble
for its own duration, so every Picard iteration of a step adds the term from
the fields as they stood when the step began; advance_scalars() moves the
fields with the by-face fluxes of the step's last prepare.

The pieces a deliberately wrong variant replaces (tests/test_buoyancy.py) are
methods of their own: gravity, density, reference.
"""
from __future__ import annotations

import numpy as np

from tests import refpy
from tests.scalar_bc_ref import NO_BOX, ScalarBCRef

F = np.float32


class _Field:
    def __init__(self, arrays):
        self.R = ScalarBCRef(arrays, scheme=0)
        self.phi = np.zeros(self.R.N, F)
        self.D, self.inlet = F(0), F(0)
        self.beta, self.ref = F(0), F(0)
        self.stats = None


class BuoyantRefSolver(refpy.RefSolver):
    """refpy.RefSolver with GpuSolver's scalar and buoyancy surface, as far as
    the buoyancy tests use it.  M: a RefMesh of the same mesh built earlier
    (read-only, so it can be shared)."""

    def __init__(self, mesh, M=None, **cfg):
        if M is None:
            super().__init__(mesh, **cfg)
        else:
            build = refpy.RefMesh
            refpy.RefMesh = lambda _mesh: M
            try:
                super().__init__(mesh, **cfg)
            finally:
                refpy.RefMesh = build
        self._arrays = mesh.arrays()
        self.fields = []
        self.g = (F(0), F(0))
        self.last_step_dt = None
        self.sc_cfg = dict(tol=1e-6, max_sweeps=200, check_interval=4)

    # ---- the scalar surface -------------------------------------------------
    def enable_scalars(self, count, **cfg):
        self.fields = [_Field(self._arrays) for _ in range(count)]  # every beta back to 0
        self.sc_cfg = dict(tol=1e-6, max_sweeps=200, check_interval=4)
        self.sc_cfg.update({k: v for k, v in cfg.items() if v is not None})

    def set_scalar_params(self, field, diffusivity, inlet_value):
        self.fields[field].D, self.fields[field].inlet = F(diffusivity), F(inlet_value)

    def set_scalar(self, field, phi):
        self.fields[field].phi = np.asarray(phi, np.float64).astype(F)

    def get_scalar(self, field):
        return self.fields[field].phi.astype(np.float64)

    def set_scalar_wall(self, field, kind, value=0.0, box=NO_BOX):
        return self.fields[field].R.set_wall(kind, value, box)

    def advance_scalars(self, dt=None):
        dt = self.last_step_dt if dt is None else F(dt)
        assert dt is not None, "no step yet"
        for f in self.fields:
            f.phi, *f.stats = f.R.advance(self.last["fluxes"], self.c.density, dt, f.D, f.inlet, f.phi, **self.sc_cfg)

    # ---- buoyancy -----------------------------------------------------------
    def set_scalar_buoyancy(self, field, beta, ref=0.0):
        self.fields[field].beta, self.fields[field].ref = F(beta), F(ref)

    def set_gravity(self, gx, gy):
        self.g = (F(gx), F(gy))

    def buoyancy(self):
        drive = any(f.beta != 0 for f in self.fields)
        return dict(g=(float(self.g[0]), float(self.g[1])), beta=[float(f.beta) for f in self.fields],
                    ref=[float(f.ref) for f in self.fields], active=bool(drive and (self.g[0] != 0 or self.g[1] != 0)))

    # the three pieces of the term a wrong variant replaces
    def gravity(self):
        return self.g

    def density(self):
        return self.c.density

    def reference(self, f):
        return f.ref

    def driving(self):
        return [f for f in self.fields if f.beta != 0]

    def add_buoyancy(self, rhs):
        """rhs [3N] with the term added to its u and v rows (a copy); rhs itself when buoyancy is off"""
        gx, gy = self.gravity()
        drive = self.driving()
        if not drive or (gx == 0 and gy == 0):
            return rhs
        out = rhs.copy()
        ru, rv = out[0::3].copy(), out[1::3].copy()
        vr = self.M.vol * F(self.density())
        for f in drive:
            d = f.phi - F(self.reference(f))
            fb = vr * (f.beta * d)
            ru = ru - fb * gx
            rv = rv - fb * gy
        assert ru.dtype == F and rv.dtype == F
        out[0::3], out[1::3] = ru, rv
        return out

    def buoyancy_force(self):
        """(fx, fy, driving fields): the per-cell float64 terms in the canonical order"""
        gx, gy = (float(v) for v in self.g)
        drive = [f for f in self.fields if f.beta != 0]
        if not drive or (gx == 0 and gy == 0):
            return 0.0, 0.0, len(drive)
        vr = self.M.vol.astype(np.float64) * float(self.c.density)
        tx, ty = np.zeros(self.M.N), np.zeros(self.M.N)
        for f in drive:
            m = (vr * float(f.beta)) * (f.phi.astype(np.float64) - float(f.ref))
            tx = tx - m * gx
            ty = ty - m * gy
        return float(refpy.canon_sum(tx)), float(refpy.canon_sum(ty)), len(drive)

    # ---- the step -----------------------------------------------------------
    def step(self):
        plain = refpy.assemble

        def assemble(*args):
            mv, rhs, sv, dui, dvi, dpi = plain(*args)
            return mv, self.add_buoyancy(rhs), sv, dui, dvi, dpi

        dt = F(self.c.dt)
        refpy.assemble = assemble
        try:
            super().step()
        finally:
            refpy.assemble = plain
        self.last_step_dt = dt

    def debug_rhs(self):
        """cfd_debug_prepare_assemble + cfd_debug_buffer(3): prepare and assemble
        on the current state, no rotation; (rhs with the term, the plain rhs)"""
        st, old, old_old = self.ring[self.i_state], self.ring[self.i_old], self.ring[self.i_old_old]
        fl, gu, gv = refpy.prepare(self.M, st, old, self.c)
        rhs = refpy.assemble(self.M, st, old, old_old, fl, gu, gv, self.c)[1]
        self.last = dict(fluxes=fl, grad_u=gu, grad_v=gv)
        return self.add_buoyancy(rhs), rhs


def term64(vol32, density, betas, refs, phis, g):
    """The term in float64 from the maths, for the check
        |rhs_on - rhs_off - t64| <= 8 eps32 (|rhs_on| + vol rho sum_f |beta_f| (|phi_f| + |ref_f|) |g_c|):
    (t64 [N, 2], the magnitude [N, 2] the bound multiplies).  vol32: the float32
    volumes widened; betas, refs, g: the float32 parameters widened; phis: the
    fields as the solver holds them."""
    vol = np.asarray(vol32, np.float64)
    s = np.zeros(len(vol))
    mag = np.zeros(len(vol))
    for beta, ref, phi in zip(betas, refs, phis):
        phi = np.asarray(phi, np.float64)
        s += float(beta) * (phi - float(ref))
        mag += abs(float(beta)) * (np.abs(phi) + abs(float(ref)))
    g = np.asarray(g, np.float64)
    t = -(vol * float(density) * s)[:, None] * g[None, :]
    return t, (vol * float(density) * mag)[:, None] * np.abs(g)[None, :]


EPS32 = 2.0 ** -24  # the unit roundoff of float32


def check_rhs(rhs_on, rhs_off, t64, mag, what=""):
    """check 2, per cell and component; returns the worst ratio to the bound"""
    on = np.asarray(rhs_on, np.float64).reshape(-1, 3)
    off = np.asarray(rhs_off, np.float64).reshape(-1, 3)
    assert np.array_equal(on[:, 2], off[:, 2]), f"{what}: rhs_p changed"
    err = np.abs(on[:, :2] - off[:, :2] - t64)
    bound = 8.0 * EPS32 * (np.abs(on[:, :2]) + mag)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    assert np.all(err <= bound), f"{what}: worst error / bound {ratio:.3g}"
    return ratio
