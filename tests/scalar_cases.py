"""Case list and drivers shared by tests/test_scalar_f64.py (CPU: the oracle's
fluxes, the restatements' scalars) and tests/test_gpu_scalar_f64.py (HIP path):
the float64 checks of tests/scalar_checks.py on one passive-scalar advance.

HELPER MODULE, not a test.  Every driver takes the solver class, so the two
test modules run the same cases through the same code.

Meshes, named by what they can show:
  rect          fewer than 64 cells
  voronoi       5 to 9 slots per cell
  graded        hanging faces, cells of 5 and more faces (tests/fv_cases.py)
  strip1        one cell: no internal slot
  strip2        two cells: one internal slot each
  strip130      more than two wavefronts of a 1-D row
  wheel100      a 100-face hub: 25 rounds of the four-at-a-time slot loops;
                scheme 1 is refused there (more than 32 faces per cell)
  obstacle_perm channel_obstacle(h = 0.1) renumbered by synthetic.perm_random
  fine_perm     channel_obstacle(h = 0.02) renumbered likewise: more than four
                1,024-cell blocks, every gather phi[o], g[o] far away

Flow: the "synthetic" mode of tests/test_gpu_scalar.py (set_u of a smooth field,
debug_prepare_assemble(False)) at density 1 and 1000; the scalars advance by dt
= 0.02, twice per case, each advance checked.  Settings: scheme 0 and 1 with
Jacobi at D = 0 and 0.01; scheme 0 and 1 with BiCGStab at D = 0.05.  Fields: the
smooth profile of tests/test_gpu_scalar.py with inlet 0.25, and the step x <
0.8 with inlet 1.

BiCGStab ends `converged` on every mesh of the list, the one-cell strip
included (its polish decides that), so none is left out of its settings.
"""
import functools
from types import SimpleNamespace

import numpy as np

from cfd2_amd import default_config
from tests import refpy
from tests import scalar_checks as sc
from tests.fv_cases import mesh_of as fv_mesh_of
from tests.scalar_hr_ref import ScalarHRRef
from tests.synthetic import perm_random, renumbered
from tests.test_gpu_scalar import _fields, _mesh

F = np.float32
TOL = float(F(1e-6))  # cfd_scalar_config_default
DT = 0.02
ADVANCES = 2
MESHES = ["rect", "voronoi", "graded", "strip1", "strip2", "strip130", "wheel100", "obstacle_perm", "fine_perm"]
DENSITIES = [1.0, 1000.0]
# (scheme, method, D)
SETTINGS = [(0, 0, 0.0), (0, 0, 0.01), (1, 0, 0.0), (1, 0, 0.01), (0, 1, 0.05), (1, 1, 0.05)]
FIELDS = ["smooth", "step"]
WIDE = ["wheel100"]  # more than 32 faces per cell: scheme 1 is refused
# where the step profile has its front inside the mesh and next to cells the
# flow crosses, so that the float64 reference's clamp acts in the first two advances
CLAMP_MESHES = ["rect", "voronoi", "graded", "strip130", "obstacle_perm", "fine_perm"]


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name in ("rect", "voronoi"):
        return _mesh(name)
    if name.endswith("_perm"):
        base = _mesh(name[:-5])
        return renumbered(base, perm_random(base.num_cells()))
    return fv_mesh_of(name)


def settings_of(name):
    return [s for s in SETTINGS if s[0] == 0 or name not in WIDE]


def initial(mesh, field):
    """(phi0, inlet value)"""
    if field == "smooth":
        return _fields(mesh)[1], 0.25
    return np.where(mesh.arrays()["cell_cx"] < 0.8, 1.0, 0.0), 1.0


def flow(cls, mesh, density):
    """tests/test_gpu_scalar.py _flow(mesh, "synthetic") with the density a parameter"""
    s = cls(mesh, config=default_config(fixed_outer=2, fixed_inner=5))
    s.set_dt(1e-3)
    s.set_viscosity(0.01)
    s.set_density(density)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    c = s.constants
    c.inlet_velocity = 1.3
    c.ramp_time = 0.1
    c.time = 0.04
    s.constants = c
    s.set_u(_fields(mesh)[0])
    s.debug_prepare_assemble(False)
    return s


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _restated(name, scheme):
    return ScalarHRRef(mesh_of(name).arrays(), scheme=scheme)


# ------------------------------------------------------------ the CPU stand-in
def restated_solver(ref_class=ScalarHRRef):
    """A class with GpuSolver's surface as the drivers use it: the flow is the CPU
    oracle's, the scalars (one field) are `ref_class`'s, a ScalarHRRef."""
    from tests.oracle_py import OracleSolver

    class RestatedSolver:
        _refs = {}

        def __init__(self, mesh, config=None):
            self._o = OracleSolver(mesh, config=config)
            self._mesh = mesh
            self._st = None

        def __getattr__(self, name):
            return getattr(self._o, name)

        @property
        def constants(self):
            return self._o.constants

        @constants.setter
        def constants(self, c):
            self._o.constants = c

        def close(self):
            pass

        def _ref(self, scheme):
            key = (id(self._mesh), scheme)
            if key not in self._refs:
                self._refs[key] = (self._mesh, ref_class(self._mesh.arrays(), scheme=scheme))
            return self._refs[key][1]

        def enable_scalars(self, count):
            assert count == 1
            self._phi = np.zeros(self._mesh.num_cells(), F)
            self._D, self._inlet, self._scheme, self._method = 0.0, 0.0, 0, 0
            self._st = SimpleNamespace(sweeps=0, converged=0, last_delta=F(0), dt_used=F(0))
            self._ks = SimpleNamespace(method=0, iterations=0, stop_reason=0, polish_sweeps=0, krylov_residual=F(0))
            self._hs = SimpleNamespace(scheme=0, clamped_cells=0)

        def set_scalar_params(self, field, D, inlet):
            self._D, self._inlet = D, inlet

        def set_scalar(self, field, phi):
            self._phi = np.asarray(phi, np.float64).astype(F)

        def get_scalar(self, field):
            return self._phi.astype(np.float64)

        def set_scalar_scheme(self, field, scheme="vanleer"):
            self._scheme = {"upwind": 0, "vanleer": 1}[scheme]

        def set_scalar_solver(self, field, method="bicgstab"):
            self._method = {"jacobi": 0, "bicgstab": 1}[method]

        def advance_scalars(self, dt):
            R = self._ref(self._scheme)
            args = (self._o.debug_buffer(0), self._o.constants.density, dt, self._D, self._inlet, self._phi)
            if self._method == 0:
                self._phi, sweeps, delta, conv = R.advance(*args)
                self._ks = SimpleNamespace(method=0, iterations=0, stop_reason=0, polish_sweeps=0, krylov_residual=F(0))
            else:
                r = R.advance_krylov(*args)
                self._phi, sweeps, delta, conv = r.phi, r.polish_sweeps, r.last_delta, r.converged
                self._ks = SimpleNamespace(method=1, iterations=r.iterations, stop_reason=r.stop_reason,
                                           polish_sweeps=r.polish_sweeps, krylov_residual=r.krylov_residual)
            self._st = SimpleNamespace(sweeps=sweeps, converged=int(conv), last_delta=delta, dt_used=F(dt))
            self._hs = SimpleNamespace(scheme=self._scheme, clamped_cells=R.clamped)

        def scalar_stats(self, field):
            vol = self._mesh.arrays()["cell_vol"].astype(F).astype(np.float64)
            phi = self._phi.astype(np.float64)
            return SimpleNamespace(min=float(phi.min()), max=float(phi.max()),
                                   integral=float(refpy.canon_sum(vol * phi)), **vars(self._st))

        def scalar_solver_stats(self, field):
            return self._ks

        def scalar_scheme_stats(self, field):
            return self._hs

    return RestatedSolver


# --------------------------------------------------------------------- drivers
def _assert_bit_exact(s, name, scheme, method, flux, density, D, inlet, phi_old, what):
    """the advance just made == the matching restatement from phi_old, bit for bit"""
    R = _restated(name, scheme)
    st, ks, hs = s.scalar_stats(0), s.scalar_solver_stats(0), s.scalar_scheme_stats(0)
    if method == 0:
        phi, sweeps, delta, conv = R.advance(flux, density, DT, D, inlet, phi_old)
    else:
        r = R.advance_krylov(flux, density, DT, D, inlet, phi_old)
        phi, sweeps, delta, conv = r.phi, r.polish_sweeps, r.last_delta, r.converged
        assert (ks.iterations, ks.stop_reason, ks.polish_sweeps) == (r.iterations, r.stop_reason, r.polish_sweeps), what
        assert np.array_equal(_bits(ks.krylov_residual), _bits(r.krylov_residual)), what
    assert ks.method == method and hs.scheme == scheme, what
    assert (st.sweeps, bool(st.converged)) == (sweeps, conv), (what, st.sweeps, sweeps)
    assert np.array_equal(_bits(st.last_delta), _bits(delta)), what
    assert hs.clamped_cells == R.clamped, (what, hs.clamped_cells, R.clamped)
    assert np.array_equal(_bits(s.get_scalar(0)), _bits(phi)), f"{what}: phi differs from the restatement"


def run_mesh(cls, name, density, bit_exact=True, settings=None, fields=FIELDS, worst=None):
    """Every setting x field of one mesh at one density on one handle: per
    advance the bit equality with the restatement and the three float64 checks.
    worst: a dict that receives, per check, the largest (error / bound, case).
    Returns the coverage counts: advances, rows checked, faces that carried a
    correction, cells the float64 reference clamped."""
    mesh = mesh_of(name)
    a = mesh.arrays()
    s = flow(cls, mesh, density)
    flux = s.debug_buffer(0)
    rho = float(s.constants.density)
    assert rho == density and np.all(np.isfinite(flux))
    assert np.abs(flux).max() > 0.0, "setup: no flux"
    cover = {"advances": 0, "rows": 0, "corrected": 0, "clamped": 0}

    def note(check, ratio, what):
        if worst is not None and ratio > worst.get(check, (0.0, ""))[0]:
            worst[check] = (ratio, what)

    for scheme, method, D in (settings_of(name) if settings is None else settings):
        for field in fields:
            phi0, inlet = initial(mesh, field)
            s.enable_scalars(1)
            s.set_scalar_params(0, D, inlet)
            s.set_scalar(0, phi0)
            if scheme:
                s.set_scalar_scheme(0, "vanleer")
            if method:
                s.set_scalar_solver(0, "bicgstab")
            phi_old = s.get_scalar(0)
            assert np.array_equal(phi_old, np.asarray(phi0, np.float64).astype(F).astype(np.float64))
            for k in range(ADVANCES):
                what = f"{name} rho {density} scheme {scheme} method {method} D {D} {field} advance {k}"
                i_old = s.scalar_stats(0).integral
                s.advance_scalars(DT)
                st = s.scalar_stats(0)
                phi = s.get_scalar(0)
                assert st.converged == 1 and st.last_delta <= TOL, f"{what}: not converged ({st.sweeps} sweeps)"
                assert st.dt_used == F(DT)
                if bit_exact:
                    _assert_bit_exact(s, name, scheme, method, flux, rho, D, inlet, phi_old, what)
                args = (a, flux, rho, DT, D, inlet)
                A, b = sc.system64(*args, phi_old)
                clamp = np.zeros(len(phi))
                if scheme == 1:
                    b, clamp = sc.rhs_limited64(*args, phi_old)
                    cover["corrected"] += int(np.count_nonzero(sc.increments64(a, flux, inlet, phi_old)[0]))
                    cover["clamped"] += int(np.count_nonzero(clamp))
                terms = sc.row_terms64(*args, phi_old, phi, scheme)
                rows, ratio = sc.check_solved(A, b, phi, TOL, terms, what)
                note("check_solved", ratio, what)
                ratio = sc.check_against_direct_solve(A, b, phi, TOL, terms, sc.time_coefficient64(a, rho, DT), what)
                note("check_against_direct_solve", ratio, what)
                ratio, _ = sc.check_budget(*args, phi, i_old, st.integral, clamp, A, TOL, terms, what)
                note("check_budget", ratio, what)
                cover["advances"] += 1
                cover["rows"] += rows
                phi_old = phi
    s.close()
    return cover


def check_coverage(name, cover, settings=None):
    """No check of run_mesh was vacuous on this mesh."""
    settings = settings_of(name) if settings is None else settings
    n = mesh_of(name).num_cells()
    assert cover["advances"] == len(settings) * len(FIELDS) * ADVANCES
    assert cover["rows"] == cover["advances"] * n > 0
    limited = any(s[0] == 1 for s in settings)
    internal = int((mesh_of(name).arrays()["face_neighbor"] != sc.NONE).sum())
    if limited and internal:
        assert cover["corrected"] > 0, cover
    else:
        assert cover["corrected"] == 0
    if limited and name in CLAMP_MESHES:
        assert cover["clamped"] > 0, cover


def run_wide_refusal(cls, name="wheel100"):
    """Scheme 1 on a mesh of more than 32 faces per cell: CFD_ERR_INVALID with
    the message of csrc/host/scalar.cpp, the field stays on scheme 0 and the
    handle advances as before."""
    import pytest
    mesh = mesh_of(name)
    assert int(np.diff(mesh.arrays()["cell_face_offsets"].astype(np.int64)).max()) > 32
    s = flow(cls, mesh, 1000.0)
    flux, rho = s.debug_buffer(0), float(s.constants.density)
    phi0, inlet = initial(mesh, "smooth")
    s.enable_scalars(1)
    s.set_scalar_params(0, 0.01, inlet)
    s.set_scalar(0, phi0)
    with pytest.raises(RuntimeError, match=r"status 1.*more than 32 faces"):
        s.set_scalar_scheme(0, "vanleer")
    assert s.scalar_scheme_stats(0).scheme == 0
    phi_old = s.get_scalar(0)
    s.advance_scalars(DT)
    assert s.scalar_scheme_stats(0).scheme == 0 and s.scalar_stats(0).converged == 1
    _assert_bit_exact(s, name, 0, 0, flux, rho, 0.01, inlet, phi_old, "after the refusal")
    s.set_scalar_scheme(0, "upwind")  # scheme 0 is still accepted
    s.close()
