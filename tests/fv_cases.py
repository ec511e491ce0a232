"""Case list and drivers shared by tests/test_fv_invariants.py (CPU oracle) and
tests/test_gpu_fv_invariants.py (HIP path): the float64 checks of
tests/fv_checks.py on the smallest meshes that hold every face kind.

HELPER MODULE, not a test.  Every driver takes the solver class, so the two
test modules run the same cases through the same code."""
import functools

import numpy as np

from cfd2_amd import default_config
from tests import fv_checks as fv
from tests.meshes import backwards_step, channel_obstacle

# Bounds of the two-sided residual check, both 4 x the worst figure the CPU
# oracle shows over the whole solve case list below
# (profiles/r07/f64_residual_deviation.txt, written by
# tools/f64_residual_deviation.py).  The HIP path is bit-identical to the
# oracle, so it adds no deviation of its own.
#  - solves that report a computed b - A x: | r - reported | / reported;
#  - solves that may report the Givens estimate (fv_checks.reports_estimate):
#    the estimate keeps falling after the true residual has reached what f32
#    resolves, so the deviation is measured in units of
#    fv_checks.residual_resolution, |eps32 (|b| + |A||x|)|_2.
COMPUTED_WORST_MEASURED = 1.208e-2  # voronoi, AMG: 1.2 %
ESTIMATE_WORST_MEASURED_EPS = 1.221  # wheel100, AMG
RESIDUAL_TOL = 4.0 * COMPUTED_WORST_MEASURED
ESTIMATE_FLOOR_EPS = 4.0 * ESTIMATE_WORST_MEASURED_EPS

MESHES = ["backwards_step", "channel_obstacle", "graded", "voronoi", "strip1", "strip2", "strip7", "strip130",
          "wheel100"]
MONOTONE_MESHES = ["backwards_step", "voronoi"]
MIN_INTERIOR_SHARE = 0.60  # of all cells of MESHES, covered by the interior-row identities


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "backwards_step":
        return backwards_step()  # 1,300 cells
    if name == "channel_obstacle":
        return channel_obstacle()
    if name == "graded":  # the sweep's graded recipe at h = 0.06: hanging faces, cells of 5+ faces
        from cfd2_amd.mesh import ChannelWithObstacle, generate_cut_cell_mesh
        geo = ChannelWithObstacle(length=3.0, height=1.0, obstacle_center=(1.0, 0.5), obstacle_radius=0.15)
        m = generate_cut_cell_mesh(geo, 0.03, 0.12, 1.2, (3.0, 1.0))
        m.smooth(geo, 0.3, 20)
        return m
    if name == "voronoi":
        from tests.voronoi import voronoi_channel
        return voronoi_channel(2000, seed=12345)
    if name.startswith("strip"):
        from tests.synthetic import strip
        return strip(int(name[5:]))
    if name.startswith("wheel"):
        from tests.synthetic import wheel
        return wheel(int(name[5:]))
    raise KeyError(name)


def _close(s):
    if hasattr(s, "close"):
        s.close()


# ------------------------------------------------------------- assembled system
def random_state_solver(cls, mesh, scheme, time_scheme, density, dt=0.002):
    """A solver with a random u, one cheap step behind it (so that p, d_p and
    grad_p are non-zero and the Rhie-Chow flux is live) and a dt change (BDF2:
    r = dt/dt_old = 0.75), the inlet ramp mid-way.  The caller closes it."""
    s = cls(mesh, config=default_config(fixed_outer=1, fixed_inner=6))
    rng = np.random.default_rng(1234)
    s.set_u(rng.uniform(-1, 1, size=(mesh.num_cells(), 2)))
    s.initialize_history()
    s.set_dt(dt)
    s.set_density(density)
    s.set_scheme(scheme)
    s.set_time_scheme(time_scheme)
    c = s.constants
    c.time = 0.05  # inlet ramp active
    s.constants = c
    s.update_constants()
    s.step()
    s.set_dt(0.75 * dt)
    s.update_constants()
    return s


def assembled_system(cls, mesh, scheme, time_scheme, density, dt=0.002):
    """random_state_solver, then debug_prepare_assemble(False) and (True) as
    test_prepare_assemble_kernels_bitexact runs them."""
    s = random_state_solver(cls, mesh, scheme, time_scheme, density, dt)
    s.debug_prepare_assemble(False)
    s.debug_prepare_assemble(True)
    sysm = fv.System(mesh, s)
    p = s.get_p()
    _close(s)
    assert np.all(np.isfinite(p)) and np.abs(p).max() > 0.0, "setup: p must be non-zero"
    assert np.abs(sysm.flux).max() > 0.0
    return sysm


def run_assembled(cls, mesh_name, density):
    """schemes {0,1,2} x time schemes {0,1}; returns the interior rows covered."""
    mesh = mesh_of(mesh_name)
    inner = int(fv.interior_mask(mesh).sum())
    for scheme in (0, 1, 2):
        for time_scheme in (0, 1):
            sysm = assembled_system(cls, mesh, scheme, time_scheme, density)
            assert float(sysm.constants.density) == density
            if time_scheme == 1:
                assert float(sysm.constants.dt) != float(sysm.constants.dt_old)
            try:
                covered = fv.check_assembled(sysm)
            except AssertionError as e:
                raise AssertionError(f"{mesh_name} scheme {scheme} time scheme {time_scheme} rho {density}: {e}") from e
            # never vacuous: the boundary-independent checks ran on every row and
            # every internal face, the interior identities on every interior row
            a = mesh.arrays()
            assert covered["interior"] == inner
            assert covered["rows"] == mesh.num_cells() > 0
            assert covered["faces"] == int((a["face_neighbor"] != fv.NONE).sum())
            assert covered["faces"] > 0 or mesh.num_cells() == 1
    return inner


def run_coverage(cls):
    """The interior-row identities cover at least MIN_INTERIOR_SHARE of all
    cells of the case list (counted by the checks themselves)."""
    covered = cells = 0
    for name in MESHES:
        mesh = mesh_of(name)
        covered += fv.check_assembled(assembled_system(cls, mesh, 0, 0, 1.0))["interior"]
        cells += mesh.num_cells()
    assert covered >= MIN_INTERIOR_SHARE * cells, (covered, cells)
    return covered, cells


# ------------------------------------------------------------------------ solve
def setup_solve(s, mesh, precond):
    """The reference's amg_test physics (tests/amg_test.rs:22-43) with the
    inlet ramp on (t = 0.05), so that the strips and the wheel, where the
    initial inflow block is empty, have a right-hand side too."""
    s.set_dt(0.001)
    s.set_viscosity(0.001)
    s.set_density(1.0)
    s.set_alpha_p(0.3)
    s.set_alpha_u(0.7)
    s.set_scheme(0)
    a = mesh.arrays()
    u = np.zeros((mesh.num_cells(), 2))
    u[(a["cell_cx"] < 0.05) & (a["cell_cy"] > 0.5), 0] = 1.0
    s.set_u(u)
    s.initialize_history()
    s.set_precond_type(precond)
    c = s.constants
    c.time = 0.05
    s.constants = c
    s.update_constants()


def solve_steps(cls, mesh, precond, max_restart, lag, steps=3):
    """fixed_outer = 1: the buffers after step() are the one system solved.
    Yields (System, x0, stats, cfg) per step."""
    cfg = default_config(fixed_outer=1, max_restart=max_restart, convergence_lag=lag)
    s = cls(mesh, config=cfg)
    setup_solve(s, mesh, precond)
    for _ in range(steps):
        x0 = s.debug_buffer(4).astype(np.float64)
        s.step()
        yield fv.System(mesh, s), x0, s.step_info().stats_p, cfg
    _close(s)


def run_solve(cls, mesh_name, precond, record=None):
    """max_restart {50, 3, 1} x convergence_lag {0, 1}, three steps each: the
    two-sided residual check and the convergence contract.  record: a list
    that receives (label, System, stats, cfg) instead of asserting.  Returns
    how many solves each branch of the contract was asserted on."""
    mesh = mesh_of(mesh_name)
    solves = {}
    for max_restart in (50, 3, 1):
        for lag in (0, 1):
            for k, (sysm, x0, stats, cfg) in enumerate(solve_steps(cls, mesh, precond, max_restart, lag)):
                what = f"{mesh_name} precond {precond} max_restart {max_restart} lag {lag} step {k}"
                assert np.linalg.norm(sysm.rhs) > 0.0, what  # never vacuous
                if record is not None:
                    record.append((what, sysm, stats, cfg))
                    continue
                fv.check_solve(sysm, stats, cfg, RESIDUAL_TOL, ESTIMATE_FLOOR_EPS, what)
                kind = fv.check_convergence_contract(sysm, stats, cfg, RESIDUAL_TOL, ESTIMATE_FLOOR_EPS, what)
                solves[kind] = solves.get(kind, 0) + 1
    return solves


def monotone_residuals(cls, mesh, precond, kmax=8, record=None):
    """fixed_inner = k, k = 1..kmax, a fresh solver per k from one identical
    state (max_restart 50 >= kmax): the true residuals, each checked from both
    sides against the reported one (a computed b - A x: no floor)."""
    out = []
    for k in range(1, kmax + 1):
        cfg = default_config(fixed_outer=1, fixed_inner=k, convergence_lag=0)
        s = cls(mesh, config=cfg)
        setup_solve(s, mesh, precond)
        s.step()
        sysm, stats = fv.System(mesh, s), s.step_info().stats_p
        _close(s)
        assert stats.iterations == k, (k, stats.iterations)
        if record is not None:
            record.append((f"monotone precond {precond} k {k}", sysm, stats, cfg))
            r = fv.true_residual(sysm)
        else:
            assert not fv.reports_estimate(sysm, stats, cfg)
            r = fv.check_residual(sysm, stats.residual, RESIDUAL_TOL, 0.0, f"monotone precond {precond} k {k}")
        out.append(r)
    return out


def run_monotone(cls, mesh_name, precond):
    r = monotone_residuals(cls, mesh_of(mesh_name), precond)
    fv.check_monotone(r, RESIDUAL_TOL, f"{mesh_name} precond {precond}")
    return r
