"""Prescribed boundary velocities on the CPU: the numpy restatement
tests/bcvel_ref.py against the float64 checks tests/bcvel_checks.py (cases:
tests/bcvel_cases.py), the deliberately wrong variants both ways, the host-side
projection, the refusals, and the Couette case.  tests/test_gpu_bcvel.py holds
the HIP path to the same restatement and checks.
"""
import numpy as np
import pytest

from tests import bcvel_cases as bc
from tests import bcvel_checks as ck
from tests.bcvel_ref import BcvRefSolver, BoundaryVelocities

F = np.float32
# max |u - U y / H| of the restatement after 5 Couette steps, measured on the CPU
# (profiles/r16/couette_deviation.txt): float32 rounding of an exact discrete solution
COUETTE_MEASURED = 2.98e-6
COUETTE_BOUND = 8 * COUETTE_MEASURED


def _ref(name, bv_class=BoundaryVelocities, **cfg):
    return BcvRefSolver(bc.mesh_of(name), M=bc.refmesh_of(name), bv_class=bv_class, **(cfg or bc.FIXED))


@pytest.mark.parametrize("name", bc.MESHES)
def test_case_shapes(name):
    bc.check_shape(name)


@pytest.mark.parametrize("time_scheme", [0, 1])
@pytest.mark.parametrize("name", bc.MESHES)
def test_restatement_passes_the_float64_checks(name, time_scheme):
    res = bc.run_checks(_ref(name), name, time_scheme)
    print(name, time_scheme, {k: round(v, 3) for k, v in res.items()})


@pytest.mark.parametrize("wrong", ck.WRONG)
@pytest.mark.parametrize("name", ["rect", "voronoi"])
def test_checks_catch_a_wrong_convention(name, wrong):
    """the checks, evaluated with one convention wrong, reject the correct restatement"""
    with pytest.raises(AssertionError, match="f64 "):
        bc.run_checks(_ref(name), name, 0, wrong=(wrong,))


class _WallSign(BoundaryVelocities):
    def wall_sign(self):
        return F(-1)


class _NoUby(BoundaryVelocities):
    def inlet_uby(self, uby):
        return uby * F(0)


class _RampTwice(BoundaryVelocities):
    def gain(self, scale, ramp):
        return F(scale) * ramp * ramp


class _NoProjection(BoundaryVelocities):
    def project(self, v, n):
        return v, np.zeros(len(v))


@pytest.mark.parametrize("variant", [_WallSign, _NoUby, _RampTwice, _NoProjection])
@pytest.mark.parametrize("name", ["rect", "obstacle"])
def test_checks_catch_a_wrong_restatement(name, variant):
    """the correct checks reject a restatement with one piece wrong"""
    with pytest.raises(AssertionError, match="f64 "):
        bc.run_checks(_ref(name, bv_class=variant), name, 0)


def test_plain_valued_selection_keeps_the_bits():
    """every inlet face selected at (inlet_velocity, 0), scale 1: the plain step's bits"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    a, b = _ref(name), _ref(name)
    for s in (a, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
    b.set_inlet_profile(lambda x, y: (1.3 + 0.0 * y, 0.0 * y))
    assert b.boundary_velocity()["active"]
    for _ in range(2):
        a.step()
        b.step()
    assert np.array_equal(a.get_u(), b.get_u()) and np.array_equal(a.get_p(), b.get_p())


def test_projection_and_replacement():
    mesh = bc.mesh_of("obstacle")
    a = mesh.arrays()
    r = _ref("obstacle")
    wall = bc.boundary_faces(a, 3)
    x, y = a["face_cx"][wall], a["face_cy"][wall]
    on = wall[(x > 0.7) & (x < 1.3) & (y > 0.2) & (y < 0.8)]
    v = np.tile([0.3, -0.7], (len(on), 1))
    assert r.set_boundary_velocity(on, v) == len(on)
    n = np.stack([a["face_nx"][on], a["face_ny"][on]], 1)
    b = np.stack([r.bv.bx[on], r.bv.by[on]], 1).astype(np.float64)
    assert np.abs((b * n).sum(1)).max() <= 4 * 2.0 ** -24 * np.abs(v).sum(1).max()  # impermeable to f32 rounding
    v32 = v.astype(F).astype(np.float64)
    assert r.boundary_velocity()["max_normal_removed"] == pytest.approx(np.abs((v32 * n).sum(1)).max(), rel=1e-12)
    assert np.array_equal(b, ck.uploaded(a, on, v))  # the checks' own projection: the same f32
    # an inlet face keeps its normal component; a later entry replaces an earlier one
    inlet = bc.boundary_faces(a, 1)
    assert r.set_boundary_velocity([inlet[0], inlet[0]], [[1.0, 0.5], [2.0, 0.25]]) == len(on) + 1
    assert (r.bv.bx[inlet[0]], r.bv.by[inlet[0]]) == (F(2.0), F(0.25))
    assert r.boundary_velocity()["inlet_faces"] == 1 and r.boundary_velocity()["wall_faces"] == len(on)
    assert r.set_boundary_velocity([], []) == 0 and not r.boundary_velocity()["active"]


def test_refusals_change_nothing():
    mesh = bc.mesh_of("rect")
    a = mesh.arrays()
    r = _ref("rect")
    inlet = bc.boundary_faces(a, 1)
    r.set_boundary_velocity(inlet[:2], [[1.0, 0.0], [1.0, 0.0]])
    before = r.boundary_velocity()
    internal = np.nonzero(a["face_neighbor"] != 0xFFFFFFFF)[0][0]
    outlet = bc.boundary_faces(a, 2)[0]
    for bad in (internal, outlet, len(a["face_area"])):
        with pytest.raises(ValueError):
            r.set_boundary_velocity([inlet[2], bad], [[1.0, 0.0], [1.0, 0.0]])
        assert r.boundary_velocity() == before


def test_couette_is_an_exact_discrete_solution():
    """the linear profile stays to float32 rounding over 5 steps; with the wall
    term's sign flipped it does not"""
    mesh = bc.mesh_of("rect")
    dev = {}
    for variant in (BoundaryVelocities, _WallSign):
        r = BcvRefSolver(mesh, M=bc.refmesh_of("rect"), bv_class=variant)
        bc.setup_couette(r, mesh)
        for _ in range(bc.COUETTE["steps"]):
            r.step()
        dev[variant] = bc.couette_deviation(r, mesh)
    print("Couette deviation", dev[BoundaryVelocities], "sign flipped", dev[_WallSign])
    assert dev[BoundaryVelocities] <= COUETTE_BOUND
    assert dev[_WallSign] > COUETTE_BOUND


def test_rotation_signs_on_the_restatement():
    """where the GPU test's step counts come from: from rest one step delivers power
    for either sense of rotation; in a stream 3 steps turn the lift opposite ways"""
    lift, power = bc.rotation_signs(lambda: _ref("obstacle", fixed_outer=3, fixed_inner=10))
    assert power[+1] > 0 and power[-1] > 0
    assert (lift[+1] - lift[0]) * (lift[-1] - lift[0]) < 0
