"""Variable viscosity restated in numpy float32 -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of variable
viscosity"), not from the kernels, on top of tests/refpy.py,
tests/buoyancy_ref.py and tests/bcvel_ref.py (so a buoyant step with moving
walls and a viscosity field is covered).  With the uploaded float32 mu[N],
every operation one float32 rounding:

    interior slot   mu_f = 0.5 * (mu[i] + mu[other])
    boundary slot   mu_f = mu[i]
    diff_coeff      = mu_f * area / dist      dist: each kernel's own, as before
    wall force      (double)mu[i] * u_rel * area / dist_e      in float64

The header says that mu_f replaces cfd_constants::viscosity *and nothing else*.
The restatement says it the same way: `prepare` and `assemble` here ARE
bcvel_ref's, with the one expression `c.viscosity * area / <dist>` of each
replaced by a call of FaceViscosity.diff_coeff (the functions are rebuilt from
bcvel_ref's source with that single substitution, asserted to apply exactly
once in each; a second copy of 270 lines could drift from the first).

The pieces a deliberately wrong variant replaces (tests/test_visc.py) are
methods of FaceViscosity: mean, boundary, distance, site_value.

The models ("Arithmetic of the viscosity models"), evaluated at the start of a
step from the velocity the step starts from, with prepare's own Green-Gauss
gradients of that velocity:

    f32  gdot = sqrt(2 (ux ux) + 2 (vy vy) + (uy + vx) (uy + vx))
    f64  power law  m = K pow_det(max(gdot, gamma_min), n - 1)
    f64  Carreau    m = mu_inf + (mu0 - mu_inf) pow_det(1 + (lam gdot) (lam gdot), (n - 1) / 2)
    f32  mu = float32(min(max(m, mu_min), mu_max))

pow_det is restated from the prose of csrc/hip/pow_det.hpp: frexp, the mantissa
into [sqrt(1/2), sqrt(2)), the atanh series of the logarithm to t^20 / 21 by
Horner, L = y (e ln2 + ln m), k = rint(L / ln2), the exponential's series to
degree 13 by Horner, ldexp.  ViscosityModel.shear_factor is the piece a wrong
variant replaces.
"""
from __future__ import annotations

import inspect

import numpy as np

from tests import bcvel_ref, refpy
from tests.bcvel_ref import BcvRefSolver
from tests.buoyancy_ref import BuoyantRefSolver
from tests.refpy import F
from tests.refpy import prepare as _plain_prepare


class FaceViscosity:
    """The field, and the face viscosity of one column of face slots."""

    def __init__(self, mu):
        mu = np.asarray(mu, np.float64).reshape(-1).astype(F)  # the interface takes float32
        if not (np.all(np.isfinite(mu)) and np.all(mu > 0)):
            raise ValueError("viscosity field: every value finite and > 0")
        self.mu = mu

    # ---- the four pieces a wrong variant replaces -----------------------------
    def mean(self, a, b):
        return F(0.5) * (a + b)

    def boundary(self, mu_cell, mu_other):
        return mu_cell

    def distance(self, site, own, swapped):
        """the kernel's own distance: dist_e in prepare, dist_a in assemble"""
        return own

    def site_value(self, site, mu_f, c):
        return mu_f

    # ---------------------------------------------------------------------------
    def diff_coeff(self, site, c, cells, other, internal, area, dist, dist_swapped):
        mu_i, mu_o = self.mu[cells], self.mu[other]
        mu_f = np.where(internal, self.mean(mu_i, mu_o), self.boundary(mu_i, mu_o)).astype(F)
        mu_f = self.site_value(site, mu_f, c)
        out = mu_f * area / self.distance(site, dist, dist_swapped)
        assert out.dtype == F
        return out


LN2 = 0.6931471805599453
SQRT_HALF = 0.7071067811865476
LN_TERMS, EXP_DEGREE = 10, 13


def pow_det(x, y):
    """x^y for x > 0, float64, elementwise: only + - * /, frexp, ldexp, rint"""
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    m, e = np.frexp(x)
    low = m < SQRT_HALF
    m = np.where(low, m * 2.0, m)
    e = e - low.astype(e.dtype)
    t = (m - 1.0) / (m + 1.0)
    t2 = t * t
    s = np.full(t.shape, 1.0 / (2 * LN_TERMS + 1))
    for k in range(LN_TERMS - 1, -1, -1):
        s = s * t2 + 1.0 / (2 * k + 1)
    lnm = 2.0 * t * s
    L = y * (e.astype(np.float64) * LN2 + lnm)
    k = np.rint(L / LN2)
    r = L - k * LN2
    p = np.ones(t.shape)
    for j in range(EXP_DEGREE, 0, -1):
        p = 1.0 + r * p / float(j)
    return np.ldexp(p, k.astype(np.int32))


def pow_det_bound(x, y):
    """the relative error bound the header states"""
    return (16.0 + 8.0 * np.abs(np.asarray(y, np.float64) * np.log(np.asarray(x, np.float64)))) * 2.0 ** -53


class ViscosityModel:
    """cfd_viscosity_model: the float32 parameters, and the evaluation"""
    KINDS = {"none": 0, "power_law": 1, "carreau": 2}

    def __init__(self, kind, K=0.0, n=1.0, gamma_min=0.0, mu0=0.0, mu_inf=0.0, lam=0.0, mu_min=0.0, mu_max=0.0):
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        p = dict(K=K, n=n, gamma_min=gamma_min, mu0=mu0, mu_inf=mu_inf, lam=lam, mu_min=mu_min, mu_max=mu_max)
        self.p = {k: F(v) for k, v in p.items()}
        pos = lambda v: np.isfinite(v) and v > 0  # noqa: E731
        q = self.p
        ok = self.kind in (1, 2) and np.isfinite(q["n"]) and pos(q["mu_min"]) and pos(q["mu_max"]) and \
            q["mu_min"] <= q["mu_max"]
        if self.kind == 1:
            ok = ok and pos(q["K"]) and pos(q["gamma_min"])
        if self.kind == 2:
            ok = ok and pos(q["mu0"]) and np.isfinite(q["mu_inf"]) and q["mu_inf"] >= 0 and pos(q["lam"])
        if not ok:
            raise ValueError("viscosity model: a bad kind or parameter")

    def shear_factor(self):
        return F(2)

    def shear_rate(self, gu, gv):
        ux, uy, vx, vy = gu[:, 0], gu[:, 1], gv[:, 0], gv[:, 1]
        two = self.shear_factor()
        sh = uy + vx
        gdot = np.sqrt(two * (ux * ux) + two * (vy * vy) + sh * sh)
        assert gdot.dtype == F
        return gdot

    def evaluate(self, gdot):
        """(mu float32 [N], clamped below [N], clamped above [N])"""
        q = {k: np.float64(v) for k, v in self.p.items()}
        g = gdot.astype(np.float64)
        if self.kind == 1:
            m = q["K"] * pow_det(np.maximum(g, q["gamma_min"]), q["n"] - 1.0)
        else:
            lg = q["lam"] * g
            m = q["mu_inf"] + (q["mu0"] - q["mu_inf"]) * pow_det(1.0 + lg * lg, (q["n"] - 1.0) / 2.0)
        below, above = m < q["mu_min"], m > q["mu_max"]
        return np.minimum(np.maximum(m, q["mu_min"]), q["mu_max"]).astype(F), below, above


class _Constants:
    """The solver's constants as prepare / assemble read them, plus the field"""

    def __init__(self, c, fv):
        self.__dict__.update(_c=c, _fv=fv)

    def __getattr__(self, k):
        return getattr(self._c, k)

    def __setattr__(self, k, v):
        raise AttributeError("prepare and assemble only read the constants")

    def diff_coeff(self, site, *a):
        return self._fv.diff_coeff(site, self._c, *a)


def _with_face_viscosity(fn, old, new):
    src = inspect.getsource(fn)
    assert src.count(old) == 1, f"{fn.__name__}: the diffusion coefficient is formed {src.count(old)} times"
    ns = dict(vars(bcvel_ref))
    exec(compile(src.replace(old, new), f"<{fn.__name__} with a face viscosity>", "exec"), ns)
    return ns[fn.__name__]


# in prepare `dist` is the Rhie-Chow distance |d . n| (assemble's dist_a on an
# interior face); in assemble dist_e is formed from the centre offsets at hand
prepare = _with_face_viscosity(
    bcvel_ref.prepare, "diff = c.viscosity * area / dist_e",
    "diff = c.diff_coeff('prepare', cells, other, internal, area, dist_e, dist)")
assemble = _with_face_viscosity(
    bcvel_ref.assemble, "diff = c.viscosity * area / dist",
    "diff = c.diff_coeff('assemble', cells, other, internal, area, dist, np.sqrt(dvx * dvx + dvy * dvy))")


class ViscRefSolver(BcvRefSolver):
    """BcvRefSolver with GpuSolver's viscosity-field surface.  fv_class: a
    FaceViscosity subclass (a wrong variant)."""

    def __init__(self, mesh, M=None, fv_class=FaceViscosity, model_class=ViscosityModel, **cfg):
        super().__init__(mesh, M=M, **cfg)
        self.fv_class, self.model_class = fv_class, model_class
        self.fv = None
        self.model = self.gdot = self.stats = None

    # ---- the surface ------------------------------------------------------------
    def set_viscosity_field(self, mu):
        mu = np.asarray(mu, np.float64).reshape(-1)
        if len(mu) != self.M.N:
            raise ValueError("viscosity field: one value per cell")
        self.fv = self.fv_class(mu)
        self.model = None  # setting a field clears a model

    def clear_viscosity_field(self):
        self.fv = self.model = None

    def set_viscosity_model(self, kind, **params):
        if kind in ("none", 0):
            self.model = None
            return
        self.model = self.model_class(kind, **params)
        self.viscosity_evaluate()

    def viscosity_evaluate(self):
        if self.model is None:
            raise ValueError("no viscosity model is set")
        self._evaluate(self.ring[self.i_state], self.ring[self.i_old])

    def _evaluate(self, st, old):
        """the model on the velocity of st: prepare's gradients, on a copy of the state"""
        prep = BcvRefSolver._wrapped(self)[0] if self.bv.sel.any() else _plain_prepare
        _, gu, gv = prep(self.M, st.copy(), old, self.c)
        self.gdot = self.model.shear_rate(gu, gv)
        mu, below, above = self.model.evaluate(self.gdot)
        self.fv = self.fv_class(mu)
        assert np.array_equal(self.fv.mu.view(np.uint32), mu.view(np.uint32))
        self.stats = dict(mu_min=float(mu.min()), mu_max=float(mu.max()), clamped_below=int(below.sum()),
                          clamped_above=int(above.sum()))

    def shear_rate(self):
        if self.model is None:
            raise ValueError("no viscosity model is set")
        return self.gdot.copy()

    def viscosity_stats(self):
        if self.model is None:
            raise ValueError("no viscosity model is set")
        return dict(self.stats)

    def viscosity_field(self):
        if self.fv is None:
            raise ValueError("no viscosity field is set")
        return self.fv.mu.copy()

    # ---- the step ---------------------------------------------------------------
    def _wrapped(self):
        if self.fv is None:
            return super()._wrapped()
        bv, fv = self.bv, self.fv
        return (lambda M, st, old, c: prepare(M, st, old, _Constants(c, fv), bv),
                lambda M, st, old, oo, fl, gu, gv, c: assemble(M, st, old, oo, fl, gu, gv, _Constants(c, fv), bv))

    def step(self):
        if self.fv is None:
            return super().step()
        plain = refpy.prepare, refpy.assemble
        pending = [self.model is not None]  # the model, once, before the step's first prepare

        def prep(M, st, old, c):
            if pending[0]:
                pending[0] = False
                self._evaluate(st, old)
            return self._wrapped()[0](M, st, old, c)

        refpy.prepare, refpy.assemble = prep, lambda *a: self._wrapped()[1](*a)
        try:
            BuoyantRefSolver.step(self)  # adds the Boussinesq source to whatever refpy.assemble is
        finally:
            refpy.prepare, refpy.assemble = plain

    def debug_prepare_assemble(self):
        if self.fv is None:
            return super().debug_prepare_assemble()
        st, old, old_old = self.ring[self.i_state], self.ring[self.i_old], self.ring[self.i_old_old]
        prep, asm = self._wrapped()
        fl, gu, gv = prep(self.M, st, old, self.c)
        mv, rhs, sv, dui, dvi, dpi = asm(self.M, st, old, old_old, fl, gu, gv, self.c)
        return dict(fluxes=fl, grad_u=gu, grad_v=gv, mv=mv, rhs=self.add_buoyancy(rhs), sv=sv, dui=dui, dvi=dvi, dpi=dpi)

    def velocity_gradients(self):
        st = self.ring[self.i_state].copy()
        _, gu, gv = self._wrapped()[0](self.M, st, self.ring[self.i_old], self.c) if (
            self.fv is not None or self.bv.sel.any()) else refpy.prepare(self.M, st, self.ring[self.i_old], self.c)
        return gu, gv

    # ---- diagnostics --------------------------------------------------------------
    def wall_viscosity(self, cells):
        """the float64 viscosity of the wall force of these cells' wall faces"""
        if self.fv is None:
            return np.full(len(cells), float(self.c.viscosity))
        return self.fv.mu[cells].astype(np.float64)

    def _wall_terms(self):
        f, o, Fp, Fv, ub, sel = super()._wall_terms()  # Fv = nu * u_rel * area / dist, left to right
        if self.fv is None:
            return f, o, Fp, Fv, ub, sel
        M, st, d = self.M, self.ring[self.i_state], np.float64
        area = M.area[f].astype(d)
        dvx, dvy = M.fx[f] - M.cx[o], M.fy[f] - M.cy[o]
        dist = np.sqrt(dvx * dvx + dvy * dvy).astype(d)
        rux = np.where(sel, st.u[o, 0].astype(d) - ub[:, 0], st.u[o, 0].astype(d))
        ruy = np.where(sel, st.u[o, 1].astype(d) - ub[:, 1], st.u[o, 1].astype(d))
        nu = self.wall_viscosity(o)
        return f, o, Fp, np.stack([nu * rux * area / dist, nu * ruy * area / dist], 1), ub, sel
