"""Passive scalar transport on the GPU (csrc/hip/scalar.hip) against the numpy
float32 restatement tests/scalar_ref.py, bit for bit, and against the
properties the discretisation promises.

Meshes, named by the failure they can show:
  rect      fewer than 64 cells (less than one wavefront)
  obstacle  channel_obstacle(h=0.1): cell count not a multiple of 64
  voronoi   seeded Voronoi: 5 to 9 faces per cell, the widest ELL
  fine      channel_obstacle(h=0.02): more than four 1,024-cell blocks and a ragged tail
  units4    bench_mesh(0.0066, 0): the reduction writes units of 4 chunks (stats only)

Flows: "steps" = two real step() calls at dt = 1e-3 in the middle of the inlet
ramp, the scalars advanced by the step's dt; "synthetic" = set_u of a smooth
field + debug_prepare_assemble(False), the scalars advanced by dt = 0.02.

Values fixed from runs of the restatement on the CPU (oracle fluxes), all
inside the default max_sweeps = 200 with tol = 1e-6, check_interval = 4.
Sweeps per advance (3 advances):
                   steps, dt 1e-3        synthetic, dt 0.02
  mesh             D = 0     D = 0.01    D = 0       D = 0.01
  rect             4         4           8           8
  obstacle         4         4           8           12
  voronoi          4         4           8           8
  fine             4         8           20          40, 36, 36
Maximum principle (synthetic flux, dt = 0.2, D = 0.002, 5 advances): rect 12 12
12 8 8, obstacle 32 28 28 28 28, voronoi 24 each, fine 136 132 132 128 128
sweeps; median CFL of the 8 smallest cells above 1 on each; the restatement's
overshoot above 1 was at most 6e-7 against e >= 1.9e-5.
"""
import functools

import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver, default_config
from cfd2_amd.mesh import RectangularChannel, generate_cut_cell_mesh, generate_voronoi_mesh
from tests import refpy
from tests.meshes import STEP, bench_mesh, channel_obstacle
from tests.scalar_ref import ScalarRef
from tests.test_gpu_parity import _assert_same_info

pytestmark = pytest.mark.gpu

F = np.float32
TOL = float(F(1e-6))  # cfd_scalar_config_default
SMALL = ["rect", "obstacle", "voronoi", "fine"]
STEP_DT, SYNTH_DT = 1e-3, 0.02


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "rect":
        geo = RectangularChannel(length=1.0, height=0.5)
        return generate_cut_cell_mesh(geo, 0.15, 0.15, 1.2, (1.0, 0.5))
    if name == "obstacle":
        return channel_obstacle(h=0.1)
    if name == "voronoi":
        return generate_voronoi_mesh(STEP, 0.12, 0.12, 1.2, (3.5, 1.0), seed=7)
    if name == "fine":
        return channel_obstacle(h=0.02)
    if name == "units4":
        return bench_mesh(0.0066, 0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref(name):
    return ScalarRef(_mesh(name).arrays())


def _check_shape(name):
    n = _mesh(name).num_cells()
    if name == "rect":
        assert n < 64
    elif name == "obstacle":
        assert n % 64 != 0
    elif name == "voronoi":
        nf = _ref(name).nface
        assert nf.min() <= 5 and nf.max() >= 7
    elif name == "fine":
        assert n > 4 * 1024 and n % 1024 != 0  # more than four 1,024-cell blocks, a ragged tail


def _fields(mesh):
    a = mesh.arrays()
    x, y = a["cell_cx"], a["cell_cy"]
    u = np.stack([0.8 + 0.5 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y), 0.3 * np.cos(1.3 * x) * np.sin(2.9 * y + 0.2)], 1)
    phi = 0.5 + 0.4 * np.sin(2.3 * x + 0.4) * np.cos(3.1 * y)
    return u, phi


def _flow(mesh, mode):
    """a solver whose device holds the fluxes of `mode`; returns (solver, dt to pass to advance_scalars)"""
    s = GpuSolver(mesh, config=default_config(fixed_outer=2, fixed_inner=5))
    s.set_dt(STEP_DT)
    s.set_viscosity(0.01)
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    c = s.constants
    c.inlet_velocity = 1.3
    c.ramp_time = 0.1  # time < ramp_time: the inlet ramp is on
    c.time = 0.04
    s.constants = c
    s.set_u(_fields(mesh)[0])
    if mode == "steps":
        s.initialize_history()
        s.step()
        s.step()
        return s, None
    s.debug_prepare_assemble(False)
    return s, SYNTH_DT


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


@pytest.mark.parametrize("D", [0.01, 0.0])
@pytest.mark.parametrize("mode", ["steps", "synthetic"])
@pytest.mark.parametrize("name", SMALL)
def test_bit_exact_against_the_restatement(name, mode, D):
    """check 1: phi after 1 and after 3 advances, the sweep counts and the bits
    of last_delta == tests/scalar_ref.py"""
    _check_shape(name)
    mesh, R = _mesh(name), _ref(name)
    s, dt = _flow(mesh, mode)
    flux = s.debug_buffer(0)
    density = s.constants.density
    inlet = 0.25
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    phi = _fields(mesh)[1].astype(F)
    s.set_scalar(0, phi)
    assert np.array_equal(s.get_scalar(0), phi.astype(np.float64))
    sweeps = []
    for k in range(3):
        phi, sw, delta, conv = R.advance(flux, density, STEP_DT if dt is None else dt, D, inlet, phi)
        s.advance_scalars(dt)
        st = s.scalar_stats(0)
        sweeps.append(st.sweeps)
        print(f"{name} {mode} D={D} advance {k}: sweeps {st.sweeps} (ref {sw}) delta {st.last_delta:.3e}")
        assert (st.sweeps, bool(st.converged)) == (sw, conv) and conv, k
        assert _bits(st.last_delta) == _bits(delta), k
        assert st.dt_used == F(STEP_DT if dt is None else dt)
        if k in (0, 2):
            got = s.get_scalar(0)
            assert np.array_equal(got.astype(F).astype(np.float64), got)  # widened f32
            assert np.array_equal(_bits(got), _bits(phi)), k
    assert all(x % 4 == 0 and x <= 200 for x in sweeps)
    s.close()


@pytest.mark.parametrize("name", SMALL)
def test_converged_means_solved(name):
    """check 2: the final iterate satisfies the system (its f32 coefficients,
    rows evaluated in f64) to tol + (S + 4) 2^-24 max|phi|: Jacobi's update is
    the scaled residual, the strictly diagonally dominant system contracts it,
    and the second term is the rounding of one row evaluation"""
    mesh, R = _mesh(name), _ref(name)
    s, dt = _flow(mesh, "synthetic")
    flux = s.debug_buffer(0)
    D, inlet = 0.01, 0.25
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    phi0 = _fields(mesh)[1].astype(F)
    s.set_scalar(0, phi0)
    s.advance_scalars(dt)
    st = s.scalar_stats(0)
    assert st.converged == 1 and st.last_delta <= TOL
    phi = s.get_scalar(0)
    coef, diag, b = R.assemble(flux, s.constants.density, dt, D, inlet, phi0)
    res = R.residual64(coef, diag, b, phi)
    bound = TOL + (R.S + 4) * 2.0 ** -24 * float(np.abs(phi).max())
    print(f"{name}: residual {res:.3e} bound {bound:.3e} sweeps {st.sweeps}")
    assert res <= bound
    s.close()


@pytest.mark.parametrize("name", SMALL)
def test_maximum_principle(name):
    """check 3: initial and inlet values in [0, 1], 5 advances at a dt whose
    CFL exceeds 1 on the smallest cells: every value stays in [-e, 1 + e], e =
    (total sweeps) (S + 4) 2^-24, the per-sweep rounding bound compounded"""
    mesh, R = _mesh(name), _ref(name)
    s, _ = _flow(mesh, "synthetic")
    dt, D = 0.2, 0.002
    flux = s.debug_buffer(0)[R.face]
    out = np.where(R.used, np.maximum(np.where(R.owner, flux, -flux), 0.0), 0.0).sum(1)
    cfl = dt * out / (s.constants.density * R.vol)
    smallest = np.argsort(R.vol, kind="stable")[:8]  # a single cut cell may have no outflow at all
    assert np.median(cfl[smallest]) > 1.0 and np.median(cfl) > 1.0
    s.enable_scalars(1)
    s.set_scalar_params(0, D, 1.0)
    x = mesh.arrays()["cell_cx"]
    s.set_scalar(0, np.where(x < 0.8, 1.0, 0.0))
    total = 0
    for k in range(5):
        s.advance_scalars(dt)
        st = s.scalar_stats(0)
        total += st.sweeps
        e = total * (R.S + 4) * 2.0 ** -24
        phi = s.get_scalar(0)
        print(f"{name} advance {k}: sweeps {st.sweeps} min {phi.min():.3e} max-1 {phi.max() - 1:.3e} e {e:.3e}")
        assert st.min == phi.min() and st.max == phi.max()
        assert phi.min() >= -e and phi.max() <= 1.0 + e, k
    s.close()


def test_step_is_untouched():
    """check 4: step() x3 against (step(); advance_scalars()) x3: u, p, step_info
    (all but the wall-clock solve time) and the face fluxes keep their bits"""
    mesh = _mesh("obstacle")
    a, _ = _flow(mesh, "synthetic")
    b, _ = _flow(mesh, "synthetic")
    b.enable_scalars(2)
    b.set_scalar_params(0, 0.01, 1.0)
    b.set_scalar_params(1, 0.0, 0.5)
    b.set_scalar(1, _fields(mesh)[1])
    for s in (a, b):
        s.initialize_history()
    for k in range(3):
        a.step()
        b.step()
        b.advance_scalars()
        b.scalar_stats(1)
        for g in ("get_u", "get_p", "get_d_p"):
            assert np.array_equal(getattr(a, g)(), getattr(b, g)()), (g, k)
        assert np.array_equal(_bits(a.debug_buffer(0)), _bits(b.debug_buffer(0))), k
        _assert_same_info(a, b, f"step {k}")
        assert bytes(a.constants) == bytes(b.constants)
    assert b.scalar_stats(0).max > 0.0  # the dye did enter
    a.close()
    b.close()


def test_fields_are_independent():
    """check 5: field 1 of a 3-field handle == the same field alone on a 1-field handle"""
    mesh = _mesh("obstacle")
    phi = _fields(mesh)[1]
    params = [(0.0, 1.0), (0.02, 0.25), (0.3, -2.0)]
    inits = [np.zeros_like(phi), phi, 3.0 - phi]
    s3, dt = _flow(mesh, "synthetic")
    s3.enable_scalars(3)
    for f in range(3):
        s3.set_scalar_params(f, *params[f])
        s3.set_scalar(f, inits[f])
    s1, _ = _flow(mesh, "synthetic")
    s1.enable_scalars(1)
    s1.set_scalar_params(0, *params[1])
    s1.set_scalar(0, inits[1])
    for k in range(2):
        s3.advance_scalars(dt)
        s1.advance_scalars(dt)
        assert np.array_equal(s3.get_scalar(1), s1.get_scalar(0)), k
        assert bytes(s3.scalar_stats(1)) == bytes(s1.scalar_stats(0)), k
    assert not np.array_equal(s3.get_scalar(0), s3.get_scalar(1))
    assert not np.array_equal(s3.get_scalar(2), s3.get_scalar(1))
    s3.close()
    s1.close()


def test_dt_bookkeeping():
    """check 6: advance_scalars() uses the dt of the last step(), not a later
    set_dt; before any step it has no dt to use"""
    mesh = _mesh("rect")
    s, _ = _flow(mesh, "synthetic")
    s.enable_scalars(1)
    with pytest.raises(RuntimeError, match=r"status 1.*last cfd_step"):
        s.advance_scalars()
    s.advance_scalars(0.5)  # an explicit dt needs no step
    assert s.scalar_stats(0).dt_used == 0.5
    dt1, dt2 = 2.5e-4, 7e-3
    s.set_dt(dt1)
    s.initialize_history()
    s.step()
    s.set_dt(dt2)
    s.advance_scalars()
    assert s.scalar_stats(0).dt_used == F(dt1)
    assert s.constants.dt == F(dt2)
    s.close()


def _check_stats(s, mesh, phi):
    s.set_scalar(0, phi)
    phi = s.get_scalar(0)  # the f32 values
    st = s.scalar_stats(0)
    assert st.min == phi.min() and st.max == phi.max()
    vol = mesh.arrays()["cell_vol"].astype(F).astype(np.float64)
    assert st.integral == float(refpy.canon_sum(vol * phi))


def test_stats_small_mesh():
    """check 7: min, max == numpy's; the integral == canon_sum of the f64 terms"""
    mesh = _mesh("obstacle")
    s = GpuSolver(mesh)
    s.enable_scalars(1)
    phi = _fields(mesh)[1]
    _check_stats(s, mesh, phi - 0.7)  # both signs
    _check_stats(s, mesh, -phi)
    _check_stats(s, mesh, np.zeros_like(phi))
    s.close()


def test_stats_units_of_four_chunks():
    """check 7 on >= 65,536 cells: the stats kernel writes units of 4 chunks"""
    mesh = _mesh("units4")
    n = mesh.num_cells()
    assert n >= 65536 and refpy._geom(n)[0] >= 4
    s = GpuSolver(mesh)
    s.enable_scalars(1)
    _check_stats(s, mesh, _fields(mesh)[1] - 0.7)
    s.close()


def test_refusals_and_bad_arguments():
    """check 8: a group refuses; bad arguments and calls before enable / after
    enable_scalars(0) return CFD_ERR_INVALID with a message"""
    mesh = _mesh("obstacle")
    g = GpuGroup(mesh, 2)
    with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
        g.enable_scalars(1)
    for r in g.ranks:
        with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
            r.enable_scalars(1)
    g.close()
    s = GpuSolver(mesh)
    calls = [lambda: s.set_scalar_params(0, 0.0, 1.0), lambda: s.get_scalar(0), lambda: s.advance_scalars(1e-3),
             lambda: s.scalar_stats(0), lambda: s.set_scalar(0, np.zeros(mesh.num_cells()))]
    for call in calls:  # before enable
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    for bad in (-1, 5):
        with pytest.raises(RuntimeError, match=r"status 1.*0\.\.4"):
            s.enable_scalars(bad)
    for kw, what in ((dict(tol=-1e-6), "tol"), (dict(tol=float("nan")), "tol"), (dict(check_interval=0), "check_interval"),
                     (dict(max_sweeps=0), "max_sweeps")):
        with pytest.raises(RuntimeError, match=rf"status 1.*{what}"):
            s.enable_scalars(1, **kw)
    s.enable_scalars(2)
    for f in (-1, 2):
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.get_scalar(f)
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.set_scalar_params(f, 0.0, 0.0)
    with pytest.raises(RuntimeError, match=r"status 1.*diffusivity"):
        s.set_scalar_params(0, -0.1, 0.0)
    s.enable_scalars(0)
    for call in calls:  # freed
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    s.enable_scalars(1)  # and back: zero fields
    assert not s.get_scalar(0).any()
    s.close()


def test_running_out_of_sweeps_is_not_an_error():
    """check 8: max_sweeps = check_interval = 2 and a huge dt: OK, converged == 0, sweeps == 2"""
    mesh = _mesh("obstacle")
    s, _ = _flow(mesh, "synthetic")
    s.enable_scalars(1, max_sweeps=2, check_interval=2)
    s.set_scalar_params(0, 0.01, 1.0)
    s.advance_scalars(1e6)
    st = s.scalar_stats(0)
    assert (st.sweeps, st.converged) == (2, 0) and st.last_delta > TOL
    s.enable_scalars(1, max_sweeps=5, check_interval=3)  # rounded up to a multiple of check_interval
    s.set_scalar_params(0, 0.01, 1.0)
    s.advance_scalars(1e6)
    st = s.scalar_stats(0)
    assert (st.sweeps, st.converged) == (6, 0)
    s.close()


def test_nan_is_reported_as_diverged():
    """a NaN difference reads as +inf, never as converged: CFD_ERR_DIVERGED (3)"""
    mesh = _mesh("rect")
    s, dt = _flow(mesh, "synthetic")
    s.enable_scalars(1)
    phi = _fields(mesh)[1]
    phi[3] = np.nan
    s.set_scalar(0, phi)
    with pytest.raises(RuntimeError, match=r"status 3.*diverged"):
        s.advance_scalars(dt)
    s.close()


def test_resume_through_the_public_api():
    """check 9: get_scalar, then set_scalar on a fresh twin brought to the same
    flow state, advances to the same bits"""
    mesh = _mesh("obstacle")
    a, _ = _flow(mesh, "steps")
    a.enable_scalars(1)
    a.set_scalar_params(0, 0.01, 1.0)
    a.set_scalar(0, _fields(mesh)[1])
    a.advance_scalars()
    kept = a.get_scalar(0)
    a.advance_scalars()
    b, _ = _flow(mesh, "steps")
    b.enable_scalars(1)
    b.set_scalar_params(0, 0.01, 1.0)
    b.set_scalar(0, kept)
    assert np.array_equal(b.get_scalar(0), kept)
    b.advance_scalars()
    assert np.array_equal(a.get_scalar(0), b.get_scalar(0))
    assert bytes(a.scalar_stats(0)) == bytes(b.scalar_stats(0))
    a.close()
    b.close()
