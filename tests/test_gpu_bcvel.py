"""Prescribed boundary velocities on the GPU (k_prepare_bcv, k_assemble_bcv,
k_assemble_buoyant_bcv in csrc/hip/flux.hip; k_flow_diag_bcv, k_wall_motion in
csrc/hip/diagnostics.hip): bit for bit against the numpy float32 restatement
tests/bcvel_ref.py, against the float64 checks tests/bcvel_checks.py written
from the discretisation, and against the properties include/cfd2_amd.h
("Arithmetic of boundary velocities") promises.  Cases: tests/bcvel_cases.py;
the CPU test tests/test_bcvel.py holds the restatement to the same checks.
"""
import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver, default_config
from tests import bcvel_cases as bc
from tests import buoyancy_cases as buoy
from tests.bcvel_ref import BcvRefSolver

pytestmark = pytest.mark.gpu

F = np.float32
EPS32 = 2.0 ** -24


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def _gpu(name, **cfg):
    return GpuSolver(bc.mesh_of(name), config=default_config(**(cfg or bc.FIXED)))


def _ref(name, **cfg):
    return BcvRefSolver(bc.mesh_of(name), M=bc.refmesh_of(name), **(cfg or bc.FIXED))


def _same_bits(g, r, ctx):
    for what, a, b in (("u", g.get_u(), r.get_u()), ("p", g.get_p(), r.get_p()), ("d_p", g.get_d_p(), r.get_d_p())):
        assert np.array_equal(_bits(a), _bits(b)), f"{ctx}: {what} differs in {int((_bits(a) != _bits(b)).sum())} words"


def _same_diagnostics(g, r, ctx):
    d = g.flow_diagnostics()
    fp, fv = r.wall_force()
    assert (list(d.force_pressure), list(d.force_viscous)) == (fp, fv), ctx
    assert tuple(g.wall_motion(*bc.OBSTACLE_CENTRE)) == r.wall_motion(*bc.OBSTACLE_CENTRE), ctx
    gu, gv = r.velocity_gradients()
    assert np.array_equal(_bits(g.vorticity()), _bits(gv[:, 0] - gu[:, 1])), ctx
    assert np.array_equal(_bits(g.divergence()), _bits(gu[:, 0] + gv[:, 1])), ctx


@pytest.mark.parametrize("time_scheme,scheme", bc.SCHEMES)
@pytest.mark.parametrize("name", bc.MESHES)
def test_bit_exact_against_the_restatement(name, time_scheme, scheme):
    """3 steps with the standard selection (inlet profile with v != 0, moving walls,
    scales != 1): u, p, d_p after every step, and the diagnostics after the last"""
    mesh = bc.mesh_of(name)
    g, r = _gpu(name), _ref(name)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=time_scheme, scheme=scheme)
        n = bc.select(s, name)
    assert g.boundary_velocity() == r.boundary_velocity() and g.boundary_velocity()["active"]
    assert n == g.boundary_velocity()["inlet_faces"] + g.boundary_velocity()["wall_faces"]
    for k in range(3):
        g.step()
        r.step()
        _same_bits(g, r, f"{name} time_scheme {time_scheme} scheme {scheme} step {k}")
    _same_diagnostics(g, r, name)
    g.close()


def test_bit_exact_buoyant_with_moving_walls():
    """the <BUOY, BCV> instance: a driving scalar field and the standard selection"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    g, r = _gpu(name), _ref(name)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
        buoy.setup_scalars(s, mesh)
        bc.select(s, name)
    assert g.buoyancy()["active"] and g.boundary_velocity()["active"]
    for k in range(3):
        g.step()
        r.step()
        _same_bits(g, r, f"buoyant step {k}")
        g.advance_scalars()
        r.advance_scalars()
        assert np.array_equal(_bits(g.get_scalar(0)), _bits(r.get_scalar(0))), k
    g.close()


def _system(s):
    s.debug_prepare_assemble()
    return [s.debug_buffer(i) for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10)]


@pytest.mark.parametrize("form", ["never", "cleared", "empty", "zero_walls"])
def test_noop_forms(form):
    """never set, set then cleared, an empty list (the plain kernels), and walls
    selected at velocity 0 under both scales (the BCV kernels adding zeros): 2 steps,
    then matrix, rhs, fluxes and gradients == an untouched handle, bit for bit"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    a, b = _gpu(name), _gpu(name)
    for s in (a, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
    if form == "cleared":
        bc.select(b, name)
        b.clear_boundary_velocity()
        b.set_boundary_velocity_scale(1.0, 1.0)
    elif form == "empty":
        assert b.set_boundary_velocity([], np.zeros((0, 2))) == 0
    elif form == "zero_walls":
        # a zero wall entry adds diff * (+0) to a right-hand side that is not -0 (it holds a_t u^n != 0
        # from the state of bc.fields): the same bits
        assert b.set_wall_motion(bc.OBSTACLE_BOX, velocity=(0.0, 0.0), omega=0.0) > 0
        b.set_boundary_velocity_scale(-2.5, 3.0)
    assert b.boundary_velocity()["active"] == (form == "zero_walls")
    for k in range(2):
        a.step()
        b.step()
        _same_bits(a, b, f"{form} step {k}")
    for i, (x, y) in enumerate(zip(_system(a), _system(b))):
        assert np.array_equal(_bits(x), _bits(y)), (form, i)
    a.close()
    b.close()


def test_scale_change_between_steps_under_graph_replay():
    """graph_enable(True): the scales are arguments of prepare and the assembly, which no
    graph holds; a change takes effect at the next step"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    g, r = _gpu(name), _ref(name)
    g.graph_enable(True)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=0, scheme=1)
        bc.select(s, name)
    for k, scales in enumerate([bc.SCALES, (1.5, -0.5), (0.25, 2.0), (0.25, 2.0)]):
        for s in (g, r):
            s.set_boundary_velocity_scale(*scales)
        g.step()
        r.step()
        _same_bits(g, r, f"graph step {k} scales {scales}")
    assert g.graph_stats()[2] > 0
    g.close()


@pytest.mark.parametrize("time_scheme", [0, 1])
@pytest.mark.parametrize("name", bc.MESHES)
def test_float64_checks_on_the_device(name, time_scheme):
    """tests/bcvel_checks.py through debug_prepare_assemble and debug_buffer: the inlet flux,
    the gradients, the complete right-hand side, the viscous force, torques and power"""
    g = _gpu(name)
    res = bc.run_checks(g, name, time_scheme)
    print(name, time_scheme, {k: round(v, 3) for k, v in res.items()})
    g.close()


def test_matrix_entries_unchanged():
    """the selection moves no matrix entry, diagonal inverse or d_p (buffers 5-9, get_d_p)"""
    name = "voronoi"
    mesh = bc.mesh_of(name)
    a, b = _gpu(name), _gpu(name)
    for s in (a, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=0)
    # the wall part alone: an inlet profile changes the inlet flux and with it the upwind entries
    b.set_wall_motion(**bc.wall_box(name))
    b.set_boundary_velocity_scale(*bc.SCALES)
    sa, sb = _system(a), _system(b)
    for i in (4, 5, 6, 7, 8):
        assert np.array_equal(_bits(sa[i]), _bits(sb[i])), i
    assert np.array_equal(_bits(a.get_d_p()), _bits(b.get_d_p()))
    assert not np.array_equal(_bits(sa[3]), _bits(sb[3]))  # the right-hand side does move
    a.close()
    b.close()


def test_parabolic_inlet_mass():
    """sum of the inlet fluxes of u = 6 U y (H - y) / H^2 == density * sum u(y_f) A_f, the
    midpoint rule over the inlet faces, within 12 eps32 of the sum of the magnitudes
    (check_inlet_flux's count per face) plus one rounding per face of the f64 sum's inputs"""
    name = "rect"
    mesh = bc.mesh_of(name)
    a = mesh.arrays()
    g = _gpu(name)
    bc.setup_flow(g, mesh, time=1.0)  # past the ramp
    H, U = bc.H_RECT, 1.2
    prof = lambda x, y: (6.0 * U * y * (H - y) / H ** 2, 0.0 * y)  # noqa: E731
    g.set_inlet_profile(prof)
    g.debug_prepare_assemble()
    inlet = bc.boundary_faces(a, 1)
    flux = g.debug_buffer(0).astype(np.float64)[inlet]
    rho = float(F(bc.DENSITY))
    u32 = prof(a["face_cx"][inlet], a["face_cy"][inlet])[0].astype(F).astype(np.float64)
    nx32, A32 = a["face_nx"][inlet].astype(F).astype(np.float64), a["face_area"][inlet].astype(F).astype(np.float64)
    terms = rho * u32 * nx32 * A32  # the flux normal of an inlet face points out of the domain: inflow < 0
    assert abs(flux.sum() - terms.sum()) <= 12 * EPS32 * np.abs(terms).sum()
    # and the integral itself: the midpoint rule over n equal faces exceeds the integral U H of the
    # parabola by -(H h^2 / 24) u'' = U H / (2 n^2), h = H / n; bound: the 12 eps32 above plus one
    # rounding each of u, n_x, A and y_f to f32
    n = len(inlet)
    assert abs(-flux.sum() / rho - U * H * (1.0 + 0.5 / n ** 2)) <= 16 * EPS32 * np.abs(terms).sum() / rho
    g.close()


def test_rotating_cylinder_signs():
    """from rest one step delivers power for either sense of rotation; in a stream 3 steps
    turn the lift opposite ways (tests/test_bcvel.py settled the step counts on the CPU)"""
    lift, power = bc.rotation_signs(lambda: _gpu("obstacle", fixed_outer=3, fixed_inner=10))
    print("lift", lift, "power", power)
    assert power[+1] > 0 and power[-1] > 0
    assert (lift[+1] - lift[0]) * (lift[-1] - lift[0]) < 0


def test_refusals():
    name = "rect"
    mesh = bc.mesh_of(name)
    a = mesh.arrays()
    g = _gpu(name)
    inlet = bc.boundary_faces(a, 1)
    g.set_boundary_velocity(inlet[:2], [[1.0, 0.0], [1.0, 0.5]])
    before = g.boundary_velocity()
    internal = np.nonzero(a["face_neighbor"] != 0xFFFFFFFF)[0][0]
    outlet = bc.boundary_faces(a, 2)[0]
    for bad, v in ((internal, 1.0), (outlet, 1.0), (len(a["face_area"]), 1.0), (inlet[3], float("nan"))):
        with pytest.raises(RuntimeError):
            g.set_boundary_velocity([inlet[2], bad], [[1.0, 0.0], [v, 0.0]])
        assert g.boundary_velocity() == before
    with pytest.raises(RuntimeError):  # the racy prepare of the reference-semantics mode has no BCV form
        g.debug_reference_semantics(2)
    g.clear_boundary_velocity()
    g.debug_reference_semantics(2)
    with pytest.raises(RuntimeError):
        g.set_boundary_velocity(inlet[:1], [[1.0, 0.0]])
    g.debug_reference_semantics(0)
    g.close()


def test_distributed_handle_refuses():
    mesh = bc.mesh_of("obstacle")
    a = mesh.arrays()
    grp = GpuGroup(mesh, 2, config=default_config(**bc.FIXED))
    inlet = bc.boundary_faces(a, 1)
    for h in grp.ranks:
        with pytest.raises(RuntimeError):
            h.set_boundary_velocity(inlet[:1], [[1.0, 0.0]])
        with pytest.raises(RuntimeError):
            h.set_boundary_velocity_scale(1.0, 2.0)
        with pytest.raises(RuntimeError):
            h.wall_motion(0.0, 0.0)
    grp.close()
