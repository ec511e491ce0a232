"""Float64 checks of passive scalar transport (tests/scalar_checks.py) over the
case list of tests/scalar_cases.py on the CPU: the oracle's fluxes and the numpy
restatements' scalars behind GpuSolver's surface; and the proof that the checks
bite (test_checks_catch_wrong_variants).  tests/test_gpu_scalar_f64.py runs the
same cases through the same drivers on the HIP path, which is bit-identical to
the restatements, so every bound it asserts is first shown to hold here."""
import numpy as np
import pytest

from tests import scalar_cases as cs
from tests.scalar_hr_ref import ScalarHRRef
from tests.scalar_ref import F


@pytest.mark.parametrize("density", cs.DENSITIES)
@pytest.mark.parametrize("name", cs.MESHES)
def test_advance_satisfies_the_float64_equations(name, density):
    """Every setting x field x 2 advances of one mesh and density: the rows of
    the float64 system are satisfied, the field is the float64 direct solve's,
    the integral's change is the boundary fluxes plus the conservation defect
    minus the clamp, each to tol plus 16 eps32 of the row's terms."""
    worst = {}
    cover = cs.run_mesh(cs.restated_solver(), name, density, worst=worst)
    cs.check_coverage(name, cover)
    print(name, density, cover, {k: f"{r:.3f} ({w})" for k, (r, w) in worst.items()})


def test_direct_solve_and_budget_checks_bite_alone():
    """check_solved comes first in an advance and catches every wrong variant
    below, so the other two are shown to fail on their own: one cell of phi
    moved by 1e-3 fails the direct-solve check (its bound is 1.2e-4 here: the
    largest row allowance over the smallest a_t, and the cells' volumes span
    16 : 1; it is the coarsest of the three by construction), and an integral off by 1e-4 of
    itself (a k_scalar_stats that lost one cell of 186) or a dropped clamp sum
    (2.1 here) fails the budget, whose bound is 0.94 here against parts of 43
    (inlet), -590 (outlet) and 739 (defect): 1.2e-5 of (rho / dt) I, a few
    eps32 of the f32 field times the 16 of the row bound.  voronoi, density
    1000, scheme 1, D = 0.01, smooth."""
    from tests import scalar_checks as sc
    name, rho, D = "voronoi", 1000.0, 0.01
    mesh = cs.mesh_of(name)
    a = mesh.arrays()
    s = cs.flow(cs.restated_solver(), mesh, rho)
    flux = s.debug_buffer(0)
    phi0, inlet = cs.initial(mesh, "smooth")
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    s.set_scalar(0, phi0)
    s.set_scalar_scheme(0, "vanleer")
    phi_old, i_old = s.get_scalar(0), s.scalar_stats(0).integral
    s.advance_scalars(cs.DT)
    phi, i_new = s.get_scalar(0), s.scalar_stats(0).integral
    args = (a, flux, rho, cs.DT, D, inlet)
    A, _ = sc.system64(*args, phi_old)
    b, clamp = sc.rhs_limited64(*args, phi_old)
    terms = sc.row_terms64(*args, phi_old, phi, 1)
    a_t = sc.time_coefficient64(a, rho, cs.DT)
    assert np.count_nonzero(clamp) > 0
    sc.check_against_direct_solve(A, b, phi, cs.TOL, terms, a_t)
    sc.check_budget(*args, phi, i_old, i_new, clamp, A, cs.TOL, terms)
    bad = phi.copy()
    bad[len(bad) // 2] += 1e-3
    with pytest.raises(AssertionError, match="f64 check_against_direct_solve"):
        sc.check_against_direct_solve(A, b, bad, cs.TOL, terms, a_t)
    with pytest.raises(AssertionError, match="f64 check_budget"):
        sc.check_budget(*args, phi, i_old, i_new * (1.0 + 1e-4), clamp, A, cs.TOL, terms)
    with pytest.raises(AssertionError, match="f64 check_budget"):
        sc.check_budget(*args, phi, i_old, i_new, np.zeros_like(clamp), A, cs.TOL, terms)


# ---------------------------------------------------------------- wrong variants
class _NoDensityInDiffusion(ScalarHRRef):
    def assemble(self, face_flux, density, dt, D, inlet_value, phi_old):
        return super().assemble(face_flux, density, dt, F(D) / F(density), inlet_value, phi_old)  # rd = D


class _NoDensityInTime(ScalarHRRef):
    def assemble(self, face_flux, density, dt, D, inlet_value, phi_old):
        # a_t = vol / dt; the diffusion keeps density * D
        coef, diag, b = super().assemble(face_flux, density, F(dt) * F(density), D, inlet_value, phi_old)
        return coef, diag, b


class _LamSwapped(ScalarHRRef):
    def __init__(self, arrays, **kw):
        super().__init__(arrays, **kw)
        self.lam = np.where(self.internal & ~self.degen, F(1) - self.lam, self.lam).astype(F)  # d_c / (d_c + d_o)


class _DvNegated(ScalarHRRef):
    def __init__(self, arrays, **kw):
        super().__init__(arrays, **kw)
        self.dvx, self.dvy = -self.dvx, -self.dvy


class _FluxNotNegated(ScalarHRRef):
    def __init__(self, arrays, **kw):
        super().__init__(arrays, **kw)
        self.owner = np.ones_like(self.owner)  # F_k = f on every slot; nothing else reads it after __init__


class _NormalNotNegated(ScalarHRRef):
    def __init__(self, arrays, **kw):
        super().__init__(arrays, **kw)
        self.nx = np.where(self.owner, self.nx, -self.nx)
        self.ny = np.where(self.owner, self.ny, -self.ny)


class _InletDistanceDoubled(ScalarHRRef):
    def __init__(self, arrays, **kw):
        super().__init__(arrays, **kw)
        self.dist = np.where(self.inlet, F(2) * self.dist, self.dist).astype(F)


class _ClampWithoutInlet(ScalarHRRef):
    def assemble(self, face_flux, density, dt, D, inlet_value, phi_old):
        coef, diag, b = super().assemble(face_flux, density, dt, D, inlet_value, phi_old)
        if self.scheme == 0:
            return coef, diag, b
        f = np.asarray(face_flux, F)[self.face]
        phi, inlet = np.asarray(phi_old, F), F(inlet_value)
        a_t = self.vol * F(density) / F(dt)
        corr = self.correction(np.where(self.owner, f, -f), phi, *self.gradient(phi, inlet))
        mn, mx = phi.copy(), phi.copy()
        for k in range(self.S):  # internal slots only
            v, on = phi[self.other[:, k]], self.internal[:, k]
            mn = np.where(on & (v < mn), v, mn)
            mx = np.where(on & (v > mx), v, mx)
        t = a_t * phi - corr
        lo, hi = a_t * mn, a_t * mx
        b = np.where(t < lo, lo, np.where(t > hi, hi, t)).astype(F)
        for k in range(self.S):
            m = self.inlet[:, k]
            b[m] = b[m] + coef[m, k] * inlet
        return coef, diag, b


JACOBI_0 = [(0, 0, 0.0), (0, 0, 0.01)]
JACOBI_1 = [(1, 0, 0.0), (1, 0, 0.01)]
# variant -> (class, the settings in which it is visible, the fields)
VARIANTS = {
    "density dropped from the diffusion coefficient": (_NoDensityInDiffusion, [(0, 0, 0.01)], cs.FIELDS),
    "density dropped from a_t": (_NoDensityInTime, JACOBI_0, cs.FIELDS),
    "lam swapped to d_c / (d_c + d_o)": (_LamSwapped, JACOBI_1, cs.FIELDS),
    "dv negated": (_DvNegated, JACOBI_1, cs.FIELDS),
    "flux not negated on non-owner slots": (_FluxNotNegated, JACOBI_0, cs.FIELDS),
    "normal not negated on non-owner slots": (_NormalNotNegated, JACOBI_1, cs.FIELDS),
    "inlet face distance doubled": (_InletDistanceDoubled, [(0, 0, 0.01)], cs.FIELDS),
    "clamp range without the inlet value": (_ClampWithoutInlet, JACOBI_1, ["smooth"]),
}
VARIANT_MESHES = ["rect", "voronoi", "graded"]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_checks_catch_wrong_variants(variant):
    """Each deliberately wrong restatement, run through the drivers at density
    1000 without the bit comparison, fails a float64 check on at least one mesh
    (the right restatement passes them all: the test above).

    Where a variant cannot show, by construction:
    - the diffusion variants (density dropped from rd, the inlet distance
      doubled) change nothing at D = 0: they run at D = 0.01 only;
    - lam, dv and the slot normal enter scheme 1's correction only: scheme 0
      cannot see them;
    - density dropped from a_t or from rd is the identity at density 1, as the
      issue of the whole suite was: all variants run at 1000;
    - the clamp's range matters only in a cell with an inlet face whose
      correction pushes it beyond its internal neighbours' range towards the
      inlet value: the step profile has phi = 1 = inlet at every inlet cell and
      cannot show it, the smooth profile (inlet 0.25 below every cell value)
      does on rect and graded (not on voronoi).

    As run: every variant is caught by check_solved, the first check of an
    advance, on its first visible case (all three meshes, the clamp variant on
    rect and graded)."""
    ref_class, settings, fields = VARIANTS[variant]
    cls = cs.restated_solver(ref_class)
    caught = []
    for name in VARIANT_MESHES:
        try:
            cs.run_mesh(cls, name, 1000.0, bit_exact=False, settings=settings, fields=fields)
        except AssertionError as e:
            assert "f64 check_" in str(e), e  # a check's own failure, not the driver's
            caught.append((name, str(e).split(":")[0]))
    print(variant, caught)
    assert caught, f"{variant}: passes every float64 check on {VARIANT_MESHES}"
