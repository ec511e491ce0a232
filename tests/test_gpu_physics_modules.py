"""The three opt-in physics features (passive scalars with buoyancy, prescribed
boundary velocities with the wall-motion sums, the force region) are
independent of one another: releasing one leaves the others' output byte for
byte what it was, a released feature refuses in its documented words, and the
step afterwards gives the bits of a solver that never had it.  Every comparison
is of bytes against a second solver of the same test.

Boundary velocities change the flow, so a solver that never had them reaches
the state of one that had only through a checkpoint, which stores the flow and
neither the scalars nor the boundary velocities (test_gpu_checkpoint.py: a
fresh handle resumes bit for bit)."""
import numpy as np
import pytest

from cfd2_amd import GpuSolver
from tests.meshes import channel_obstacle

pytestmark = pytest.mark.gpu

BODY = (0.7, 0.2, 1.3, 0.8)
SOURCE = (1.5, 0.2, 2.0, 0.8)
INVERTED = (1.0, 0.0, 0.0, 1.0)
GRAVITY = (0.5, -9.75)  # exact in f32
STEPS = 3
NOT_ENABLED = r"status 1.*passive scalars are not enabled"


@pytest.fixture(scope="module")
def mesh():
    return channel_obstacle(h=0.1)  # 296 cells around the disc: two 256-cell chunks, the second ragged


def _solver(mesh, history=True):
    s = GpuSolver(mesh)
    s.set_dt(0.001)
    s.set_viscosity(0.001)
    s.set_inlet_velocity(1.0)
    s.set_precond_type(1)
    if history:
        s.initialize_history()
    return s


def _scalars(s):
    """field 0: BiCGStab, van Leer, the body held at 1, a source box; field 1: plain.  Gravity on, every beta 0."""
    s.enable_scalars(2)
    s.set_scalar_params(0, 0.5, 1.0)
    s.set_scalar_solver(0, "bicgstab")
    s.set_scalar_scheme(0, "vanleer")
    assert s.set_scalar_wall(0, "value", 1.0, BODY) > 0
    assert s.set_scalar_source(0, 0.5, SOURCE) > 0
    s.set_scalar_params(1, 1e-3, 1.0)
    s.set_scalar_buoyancy(1, 0.0, 0.25)
    s.set_gravity(*GRAVITY)
    assert s.buoyancy()["active"] is False


def _velocities(s):
    assert s.set_inlet_profile(lambda x, y: (6.0 * y * (1.0 - y), 0.0 * y)) > 0
    n = s.boundary_velocity()["inlet_faces"]
    assert s.set_wall_motion(BODY, omega=0.5) > n
    assert s.boundary_velocity()["active"] is True


def _bits(s):
    return s.get_u().tobytes(), s.get_p().tobytes()


def _steps(s, n, scalars):
    """n steps, each followed by an advance: the u / p bytes after every step"""
    out = []
    for _ in range(n):
        s.step()
        out.append(_bits(s))
        if scalars:
            s.advance_scalars()
    return out


def _flow(mesh, scalars, velocities):
    s = _solver(mesh)
    if scalars:
        _scalars(s)
    if velocities:
        _velocities(s)
    assert s.set_force_region(*BODY) > 0
    return s, _steps(s, STEPS, scalars)


def _scalar_output(s):
    out = []
    for f in (0, 1):
        out += [s.get_scalar(f).tobytes(), bytes(s.scalar_stats(f)), bytes(s.scalar_wall_flux(f)),
                bytes(s.scalar_solver_stats(f)), bytes(s.scalar_scheme_stats(f))]
    return out


def _velocity_output(s):
    return [repr(sorted(s.boundary_velocity().items())), np.array(s.wall_motion(1.0, 0.5), np.float64).tobytes(),
            bytes(s.flow_diagnostics())]


def _assert_scalars_refuse(s):
    calls = (lambda: s.set_scalar_params(0, 1e-3, 1.0), lambda: s.set_scalar(0, np.zeros(s.num_cells)),
             lambda: s.get_scalar(0), s.advance_scalars, lambda: s.scalar_stats(0),
             lambda: s.set_scalar_solver(0, "bicgstab"), lambda: s.scalar_solver_stats(0),
             lambda: s.set_scalar_scheme(0, "vanleer"), lambda: s.scalar_scheme_stats(0),
             lambda: s.set_scalar_wall(0, "value", 1.0, BODY), lambda: s.set_scalar_source(0, 0.5, SOURCE),
             lambda: s.scalar_wall_flux(0), lambda: s.set_scalar_buoyancy(0, 0.1), s.buoyancy_force)
    for call in calls:
        with pytest.raises(RuntimeError, match=NOT_ENABLED):
            call()


def _resumed(mesh, path, scalars_of=None):
    """a fresh handle at the flow state saved in `path`, with the scalar fields of `scalars_of`"""
    s = _solver(mesh, history=False)
    s.load_state(path)
    if scalars_of is not None:
        _scalars(s)
        for f in (0, 1):
            s.set_scalar(f, scalars_of.get_scalar(f))
    return s


@pytest.fixture(scope="module")
def only_velocities(mesh):
    """the u / p bytes after each of STEPS + 1 steps of a solver with the boundary velocities alone"""
    s, out = _flow(mesh, False, True)
    out += _steps(s, 1, False)
    s.close()
    return out


def test_scalars_with_beta_zero_leave_the_step_alone(mesh, only_velocities):
    p, plain = _flow(mesh, False, False)
    p.close()
    assert plain != only_velocities[:STEPS], "the boundary velocities change the flow"
    for velocities, want in ((False, plain), (True, only_velocities[:STEPS])):
        s, got = _flow(mesh, True, velocities)
        assert s.scalar_solver_stats(0).method == 1 and s.scalar_solver_stats(0).iterations > 0
        assert s.scalar_scheme_stats(0).scheme == 1 and s.scalar_stats(1).sweeps > 0
        s.close()
        assert got == want, f"with the boundary velocities: {velocities}"


def test_enable_scalars_zero(mesh, only_velocities):
    s, got = _flow(mesh, True, True)
    assert got == only_velocities[:STEPS]
    s.set_scalar_buoyancy(1, 0.5, 0.25)  # cleared with the fields: the next step is not buoyant
    assert s.buoyancy()["active"] is True and s.buoyancy()["g"] == GRAVITY
    ref = _velocity_output(s)
    assert _velocity_output(s) == ref, "reading twice"
    s.enable_scalars(0)
    assert _velocity_output(s) == ref
    assert s.buoyancy() == dict(g=GRAVITY, beta=[], ref=[], active=False)
    _assert_scalars_refuse(s)
    assert _steps(s, 1, False) == only_velocities[STEPS:]
    s.enable_scalars(2)  # gravity survives, no beta does
    assert s.buoyancy() == dict(g=GRAVITY, beta=[0.0, 0.0], ref=[0.0, 0.0], active=False)
    s.close()


def test_clear_boundary_velocity(mesh, tmp_path):
    s, _ = _flow(mesh, True, True)
    path = str(tmp_path / "flow.bin")
    s.save_state(path)
    ref = _scalar_output(s)
    assert _scalar_output(s) == ref, "reading twice"
    s.clear_boundary_velocity()
    assert _scalar_output(s) == ref
    b = s.boundary_velocity()
    assert b["active"] is False and b["inlet_faces"] == 0 and b["wall_faces"] == 0
    o = _resumed(mesh, path, scalars_of=s)  # a solver with only the scalars
    for x in (s, o):
        x.step()
        x.advance_scalars()
    assert _bits(s) == _bits(o)
    assert _scalar_output(s) == _scalar_output(o)
    s.close()
    o.close()


@pytest.mark.parametrize("scalars_first", (True, False), ids=("scalars first", "velocities first"))
def test_release_both_then_the_region(mesh, tmp_path, scalars_first):
    s, _ = _flow(mesh, True, True)
    path = str(tmp_path / "flow.bin")
    s.save_state(path)
    scal, vel = _scalar_output(s), _velocity_output(s)
    if scalars_first:
        s.enable_scalars(0)
        assert _velocity_output(s) == vel
        s.clear_boundary_velocity()
    else:
        s.clear_boundary_velocity()
        assert _scalar_output(s) == scal
        s.enable_scalars(0)
    _assert_scalars_refuse(s)
    assert s.boundary_velocity()["active"] is False
    assert s.wall_motion().region_faces > 0 and s.flow_diagnostics().region_faces > 0
    assert s.set_force_region(*INVERTED) == 0
    assert s.wall_motion().region_faces == 0 and s.wall_motion().moving_faces == 0
    assert s.flow_diagnostics().region_faces == 0
    o = _resumed(mesh, path)  # untouched: never had a scalar, a boundary velocity or a force region
    assert _steps(s, 1, False) == _steps(o, 1, False)
    assert bytes(s.flow_diagnostics()) == bytes(o.flow_diagnostics())
    s.close()
    o.close()


def test_surface_follows_both_configurations(mesh):
    """the surface re-derives its channels and resets its statistics when the
    scalar or the boundary-velocity configuration changed, and only then"""
    s = _solver(mesh)
    assert s.select_surface(BODY) > 0
    s.enable_surface_stats()
    assert s.surface_info()["channels"] == 5
    s.enable_scalars(2)
    assert s.surface_info()["channels"] == 9
    s.enable_scalars(1)
    assert s.surface_info()["channels"] == 7

    def sampled():
        s.accumulate_surface_stats(0.5)
        assert s.surface_info()["samples"] == 1

    sampled()
    s.set_scalar_params(0, 1e-3, 1.0)
    s.set_scalar_source(0, 0.5, SOURCE)
    s.set_boundary_velocity_scale(0.5, 2.0)
    s.set_force_region(*BODY)
    assert s.surface_info()["samples"] == 1, "none of these resets the statistics"
    assert s.set_scalar_wall(0, "value", 1.0, BODY) > 0
    assert s.surface_info()["samples"] == 0
    sampled()
    assert s.set_wall_motion(BODY, omega=0.5) > 0
    assert s.surface_info()["samples"] == 0
    sampled()
    s.clear_boundary_velocity()
    assert s.surface_info()["samples"] == 0
    sampled()
    s.enable_scalars(0)
    assert s.surface_info() == dict(faces=s.surface_info()["faces"], channels=5, samples=0, total_weight=0.0,
                                    stats_on=True)
    s.close()


def test_order_of_checks(mesh):
    s = _solver(mesh)
    with pytest.raises(RuntimeError, match=r"status 1.*scalar field count must be 0\.\.4"):
        s.enable_scalars(5, tol=-1.0)  # the count before the configuration
    with pytest.raises(RuntimeError, match=NOT_ENABLED):
        s.set_scalar_solver(9, 7)
    s.enable_scalars(2)
    with pytest.raises(RuntimeError, match=r"status 1.*scalar field index 9 outside \[0, 2\)"):
        s.set_scalar_solver(9, 7)  # the index before the method
    with pytest.raises(RuntimeError, match=r"status 1.*scalar field index 9 outside \[0, 2\)"):
        s.set_scalar_params(9, -1.0, 0.0)  # the index before the diffusivity
    with pytest.raises(RuntimeError, match=r"status 1.*scalar field index 2 outside \[0, 2\)"):
        s.scalar_solver_stats(2)
    s.close()
