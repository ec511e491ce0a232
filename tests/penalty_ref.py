"""Volume penalisation restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of volume
penalisation"), not from the kernels, on top of tests/visc_ref.py (so a buoyant
step with moving walls, a viscosity field and a penalty is covered).  Per cell
i, every operation one float32 rounding, uc the iterate prepare and the
assembly read:

    s   = sigma[i]  (+ forch[i] * sqrt(uc.x*uc.x + uc.y*uc.y)  with forch set)
    pen = vol[i] * s
    prepare : diag += pen      after the face loop, before d_p = vol / diag
    assemble: diag_u, diag_v += pen      after the face loop
              rhs_u += pen * (target_scale * target[i].x)    after the buoyancy term; target null: nothing
              rhs_v += pen * (target_scale * target[i].y)

The header says that nothing else in either kernel changes.  The restatement
says it the same way: `prepare` and `assemble` here ARE bcvel_ref's, with
visc_ref's one substitution (the diffusion coefficient) and one inserted line
each (asserted to apply exactly once), the way visc_ref builds its own.

The pieces a deliberately wrong variant replaces (tests/test_penalty.py) are
methods of PenaltyField: in_prepare, in_assembly_diagonal, scaled_target, speed_state.

The force diagnostic, per cell in float64 from the widened float32 values, then
refpy.canon_sum (the canonical leaf / chunk / segment / total order):

    s = sigma + forch * sqrt(ux*ux + uy*uy);  m = vol * s;  t = scale * target
    f = m * (u - t);  F = sum f;  tau = sum rx fy - ry fx;  P = sum f . t;  n = #(s > 0)
"""
from __future__ import annotations

import inspect

import numpy as np

from tests import bcvel_ref, refpy
from tests.buoyancy_ref import BuoyantRefSolver
from tests.refpy import F
from tests.visc_ref import ViscRefSolver


class PenaltyField:
    """The float32 fields and the coefficient of one sweep."""

    def __init__(self, sigma, forch=None, target=None):
        f32 = lambda a: np.asarray(a, np.float64).astype(F)  # noqa: E731  the interface takes float32
        self.sigma = f32(sigma).reshape(-1)
        self.forch = None if forch is None else f32(forch).reshape(-1)
        self.target = None if target is None else f32(target).reshape(-1, 2)
        ok = np.all(np.isfinite(self.sigma)) and np.all(self.sigma >= 0)
        if self.forch is not None:
            ok = ok and len(self.forch) == len(self.sigma) and np.all(np.isfinite(self.forch)) and np.all(self.forch >= 0)
        if self.target is not None:
            ok = ok and len(self.target) == len(self.sigma) and np.all(np.isfinite(self.target))
        if not ok:
            raise ValueError("penalty: every value finite, sigma and forch >= 0, one per cell")

    # ---- the four pieces a wrong variant replaces ------------------------------
    def in_prepare(self):
        return True

    def in_assembly_diagonal(self):
        return True

    def scaled_target(self, scale):
        return scale * self.target

    def speed_state(self, st, st_old):
        """the state whose |u| the Forchheimer part reads: the iterate"""
        return st

    # ---------------------------------------------------------------------------
    def coeff(self, vol, st, st_old):
        s = self.sigma
        if self.forch is not None:
            u = self.speed_state(st, st_old).u
            s = s + self.forch * np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])
        pen = vol * s
        assert pen.dtype == F
        return pen


class _Constants:
    """The solver's constants as prepare / assemble read them, plus the viscosity
    field (or none) and the penalty"""

    def __init__(self, c, fv, owner):
        self.__dict__.update(_c=c, _fv=fv, _owner=owner)

    def __getattr__(self, k):
        return getattr(self._c, k)

    def __setattr__(self, k, v):
        raise AttributeError("prepare and assemble only read the constants")

    def diff_coeff(self, site, cells, other, internal, area, dist, dist_swapped):
        if self._fv is None:
            return self._c.viscosity * area / dist  # the expression the substitution replaced
        return self._fv.diff_coeff(site, self._c, cells, other, internal, area, dist, dist_swapped)

    def pen_prepare(self, M, st, st_old, diag):
        pf = self._owner.pf
        if not pf.in_prepare():
            return diag
        return diag + pf.coeff(M.vol, st, st_old)

    def pen_assemble(self, M, st, st_old, diag_u, diag_v):
        o = self._owner
        pen = o.pf.coeff(M.vol, st, st_old)
        o._pen_rhs = None
        if o.pf.target is not None:
            t = o.pf.scaled_target(o.pen_scale)
            o._pen_rhs = (pen * t[:, 0], pen * t[:, 1])
        if not o.pf.in_assembly_diagonal():
            return diag_u, diag_v
        return diag_u + pen, diag_v + pen


def _rebuilt(fn, subs):
    src = inspect.getsource(fn)
    for old, new in subs:
        assert src.count(old) == 1, f"{fn.__name__}: {old!r} occurs {src.count(old)} times"
        src = src.replace(old, new)
    ns = dict(vars(bcvel_ref))
    exec(compile(src, f"<{fn.__name__} with a penalty>", "exec"), ns)
    return ns[fn.__name__]


prepare = _rebuilt(bcvel_ref.prepare, [
    ("diff = c.viscosity * area / dist_e", "diff = c.diff_coeff('prepare', cells, other, internal, area, dist_e, dist)"),
    ("        st.d_p = np.where(", "        diag = c.pen_prepare(M, st, st_old, diag)\n        st.d_p = np.where(")])
assemble = _rebuilt(bcvel_ref.assemble, [
    ("diff = c.viscosity * area / dist",
     "diff = c.diff_coeff('assemble', cells, other, internal, area, dist, np.sqrt(dvx * dvx + dvy * dvy))"),
    ("        # diagonal block (:422-461)",
     "        diag_u, diag_v = c.pen_assemble(M, st, st_old, diag_u, diag_v)\n        # diagonal block (:422-461)")])


class PenaltyRefSolver(ViscRefSolver):
    """ViscRefSolver with GpuSolver's penalty surface.  pf_class: a PenaltyField
    subclass (a wrong variant)."""

    def __init__(self, mesh, M=None, pf_class=PenaltyField, **cfg):
        super().__init__(mesh, M=M, **cfg)
        self.pf_class = pf_class
        self.pf = None
        self.pen_scale = F(1)
        self._pen_rhs = None

    # ---- the surface ------------------------------------------------------------
    def set_penalty(self, sigma, forch=None, target=None):
        pf = self.pf_class(sigma, forch, target)
        if len(pf.sigma) != self.M.N:
            raise ValueError("penalty: one value per cell")
        self.pf = pf

    def clear_penalty(self):
        self.pf = None

    def set_penalty_scale(self, s):
        self.pen_scale = F(s)

    def penalty(self):
        pf = self.pf
        return dict(active=pf is not None, target_scale=float(self.pen_scale), sigma=None if pf is None else pf.sigma,
                    forch=None if pf is None else pf.forch, target=None if pf is None else pf.target)

    # ---- the step ---------------------------------------------------------------
    def _wrapped(self):
        if self.pf is None:
            return super()._wrapped()
        bv, fv = self.bv, self.fv
        return (lambda M, st, old, c: prepare(M, st, old, _Constants(c, fv, self), bv),
                lambda M, st, old, oo, fl, gu, gv, c: assemble(M, st, old, oo, fl, gu, gv, _Constants(c, fv, self), bv))

    def add_buoyancy(self, rhs):
        """the buoyancy term, then the penalty's target term the last assemble left"""
        out = super().add_buoyancy(rhs)
        add, self._pen_rhs = self._pen_rhs, None
        if add is None:
            return out
        out = out.copy()
        out[0::3] = out[0::3] + add[0]
        out[1::3] = out[1::3] + add[1]
        assert out.dtype == F
        return out

    def step(self):
        if self.pf is None:
            return super().step()
        plain = refpy.prepare, refpy.assemble
        pending = [self.model is not None]  # a viscosity model, once, before the step's first prepare

        def prep(M, st, old, c):
            if pending[0]:
                pending[0] = False
                self._evaluate(st, old)
            return self._wrapped()[0](M, st, old, c)

        refpy.prepare, refpy.assemble = prep, lambda *a: self._wrapped()[1](*a)
        try:
            BuoyantRefSolver.step(self)  # its assemble wrapper calls add_buoyancy
        finally:
            refpy.prepare, refpy.assemble = plain

    def debug_prepare_assemble(self):
        if self.pf is None:
            return super().debug_prepare_assemble()
        st, old, old_old = self.ring[self.i_state], self.ring[self.i_old], self.ring[self.i_old_old]
        prep, asm = self._wrapped()
        fl, gu, gv = prep(self.M, st, old, self.c)
        mv, rhs, sv, dui, dvi, dpi = asm(self.M, st, old, old_old, fl, gu, gv, self.c)
        return dict(fluxes=fl, grad_u=gu, grad_v=gv, mv=mv, rhs=self.add_buoyancy(rhs), sv=sv, dui=dui, dvi=dvi, dpi=dpi)

    # ---- the diagnostic -----------------------------------------------------------
    def penalty_terms(self, centre=(0.0, 0.0), box=None):
        """the per-cell float64 terms [5, N] of penalty_force (zeros outside the box)"""
        if self.pf is None:
            raise ValueError("no penalty is set")
        d = np.float64
        pf, a = self.pf, self._arrays
        u = self.ring[self.i_state].u.astype(d)
        ux, uy = u[:, 0], u[:, 1]
        s = pf.sigma.astype(d)
        if pf.forch is not None:
            s = s + pf.forch.astype(d) * np.sqrt(ux * ux + uy * uy)
        m = self.M.vol.astype(d) * s
        tx = ty = np.zeros(self.M.N)
        if pf.target is not None:
            tx, ty = d(self.pen_scale) * pf.target[:, 0].astype(d), d(self.pen_scale) * pf.target[:, 1].astype(d)
        fx, fy = m * (ux - tx), m * (uy - ty)
        cx, cy = np.asarray(a["cell_cx"], d), np.asarray(a["cell_cy"], d)
        rx, ry = cx - d(centre[0]), cy - d(centre[1])
        t = np.stack([fx, fy, rx * fy - ry * fx, fx * tx + fy * ty, np.where(s > 0, 1.0, 0.0)])
        if box is not None:
            x0, y0, x1, y1 = box
            t = np.where((cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1), t, 0.0)
        return t

    def penalty_force(self, centre=(0.0, 0.0), box=None):
        """((Fx, Fy), torque, power, cells) as GpuSolver.penalty_force"""
        t = self.penalty_terms(centre, box)
        v = [float(refpy.canon_sum(row)) for row in t]
        return (v[0], v[1]), v[2], v[3], int(v[4])
