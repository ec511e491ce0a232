"""Variable viscosity on the CPU: the numpy restatement tests/visc_ref.py
against the float64 checks tests/visc_checks.py (cases: tests/visc_cases.py),
the deliberately wrong variants both ways, the uniform field's bits, and the
layered Couette case.  tests/test_gpu_visc.py holds the HIP path to the same
restatement and checks.
"""
import numpy as np
import pytest

from tests import bcvel_cases as bc
from tests import fv_checks as fv
from tests import visc_cases as vc
from tests import visc_checks as vk
from tests.visc_ref import FaceViscosity, ViscRefSolver

F = np.float32


def _ref(name, fv_class=FaceViscosity, **cfg):
    return ViscRefSolver(bc.mesh_of(name), M=bc.refmesh_of(name), fv_class=fv_class, **(cfg or bc.FIXED))


@pytest.mark.parametrize("time_scheme", [0, 1])
@pytest.mark.parametrize("name", bc.MESHES)
def test_restatement_passes_the_float64_checks(name, time_scheme):
    res = vc.run_checks(_ref(name), name, time_scheme)
    print(name, time_scheme, {k: round(v, 3) for k, v in res.items()})
    assert res["symmetry_faces"] > 0


@pytest.mark.parametrize("wrong", vk.WRONG)
@pytest.mark.parametrize("name", ["rect", "voronoi"])
def test_checks_catch_a_wrong_convention(name, wrong):
    """the checks, evaluated with one convention wrong, reject the correct restatement"""
    with pytest.raises(AssertionError, match="f64 "):
        vc.run_checks(_ref(name), name, 0, wrong=(wrong,))


class _Harmonic(FaceViscosity):
    def mean(self, a, b):
        return F(2) * a * b / (a + b)


# a boundary slot has no other cell: the restatement's stand-in index (cell 0) is read.  A no-op for a
# boundary face of cell 0 itself; every mesh of the list has boundary faces on other cells, with other values.
class _BoundaryOther(FaceViscosity):
    def boundary(self, mu_cell, mu_other):
        return mu_other


class _DistancesSwapped(FaceViscosity):
    def distance(self, site, own, swapped):
        return swapped


class _PrepareKeepsTheConstant(FaceViscosity):
    def site_value(self, site, mu_f, c):
        return np.full_like(mu_f, c.viscosity) if site == "prepare" else mu_f


@pytest.mark.parametrize("variant", [_Harmonic, _BoundaryOther, _DistancesSwapped, _PrepareKeepsTheConstant])
@pytest.mark.parametrize("name", ["voronoi", "obstacle"])
def test_checks_catch_a_wrong_restatement(name, variant):
    """the correct checks reject a restatement with one piece wrong"""
    with pytest.raises(AssertionError, match="f64 "):
        vc.run_checks(_ref(name, fv_class=variant), name, 0)


def test_asymmetric_mean_breaks_the_bit_symmetry():
    """a mean that is not commutative in floating point fails check_symmetry alone"""
    class _Lopsided(FaceViscosity):
        def mean(self, a, b):
            return a + F(0.5) * (b - a)

    with pytest.raises(AssertionError, match="f64 check_symmetry"):
        vc.run_checks(_ref("voronoi", fv_class=_Lopsided), "voronoi", 0)


def test_uniform_field_keeps_the_plain_bits():
    """mu == the constant viscosity everywhere: 0.5 * (m + m) == m, the plain step's bits"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    a, b = _ref(name), _ref(name)
    for s in (a, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
    b.set_viscosity_field(np.full(mesh.num_cells(), float(F(vc.NU))))
    for _ in range(2):
        a.step()
        b.step()
    assert np.array_equal(a.get_u(), b.get_u()) and np.array_equal(a.get_p(), b.get_p())
    for x, y in zip(vc.ref_system(a), vc.ref_system(b)):
        assert np.array_equal(np.asarray(x, F).view(np.uint32), np.asarray(y, F).view(np.uint32))
    b.clear_viscosity_field()
    with pytest.raises(ValueError):
        b.viscosity_field()


def test_refusals():
    r = _ref("rect")
    n = bc.mesh_of("rect").num_cells()
    for bad in (np.ones(n - 1), np.r_[np.ones(n - 1), 0.0], np.r_[np.ones(n - 1), -1.0],
                np.r_[np.ones(n - 1), np.nan], np.r_[np.ones(n - 1), np.inf]):
        with pytest.raises(ValueError):
            r.set_viscosity_field(bad)
    with pytest.raises(ValueError):
        r.viscosity_field()


# ---- layered Couette ----------------------------------------------------------------
MU1, MU2, U_BELT = 0.02, 0.1, 1.0


def _layered_profile(y, mean):
    """the discrete solution of two layers (mu1 below H / 2, mu2 above) between a wall at
    rest and a belt at U on rows of height h: a constant shear stress tau, so the step
    between two rows is tau h / nu_f with nu_f the face viscosity, half a step at a wall"""
    h = 0.125
    rows = np.round(y / h - 0.5).astype(int)
    nrow = int(round(bc.H_RECT / h))
    mu = np.where(np.arange(nrow) < nrow // 2, MU1, MU2)
    steps = np.r_[0.5 * h / mu[0], [h / mean(mu[j], mu[j + 1]) for j in range(nrow - 1)], 0.5 * h / mu[-1]]
    tau = U_BELT / steps.sum()
    return (tau * np.cumsum(steps)[:-1])[rows], mu[rows]


def _couette_residual(mean):
    """worst |row residual| / (16 eps32 * sum of the magnitudes of the row's terms) over the
    u rows of the system the restatement assembles on the profile"""
    mesh = bc.mesh_of("rect")
    a = mesh.arrays()
    r = _ref("rect")
    bc.setup_couette(r, mesh)  # constants, the belt (top wall at U); its state and inlet are replaced below
    u, mu = _layered_profile(a["cell_cy"], mean)
    r.set_u(np.stack([u, 0.0 * u], 1))
    r.initialize_history()
    inlet = bc.boundary_faces(a, 1)
    r.set_boundary_velocity(inlet, np.stack([_layered_profile(a["face_cy"][inlet], mean)[0], 0.0 * inlet], 1))
    r.set_viscosity_field(mu)
    o = r.debug_prepare_assemble()
    A = fv._coupled_csr(mesh, o["mv"].astype(np.float64)).tocsr()
    x = np.zeros(3 * mesh.num_cells())
    x[0::3], x[1::3], x[2::3] = r.get_u()[:, 0], r.get_u()[:, 1], r.get_p()
    rhs = o["rhs"].astype(np.float64)
    res = (A @ x - rhs)[0::3]
    mag = (abs(A) @ np.abs(x) + np.abs(rhs))[0::3]
    return float(np.max(np.abs(res) / (fv.TOL_ROW * mag)))


def test_layered_couette_is_an_exact_discrete_solution():
    """the piecewise-linear profile with the arithmetic mean on the interface leaves the
    assembled momentum rows a residual at rounding level (fv_checks.TOL_ROW of the row's
    terms); the profile of a harmonic interface does not"""
    good = _couette_residual(lambda a, b: 0.5 * (a + b))
    bad = _couette_residual(lambda a, b: 2.0 * a * b / (a + b))
    print("layered Couette residual / bound", good, "harmonic interface", bad)
    assert good <= 1.0
    assert bad > 100.0


# ---- pow_det and the models ---------------------------------------------------------
def _pow_grid():
    """seeded, log-uniform: x over the shear-rate arguments of both models (gamma_min 1e-3
    up to 1 + (lambda gdot)^2 of 1e8), y over n - 1 and (n - 1) / 2 for n in (0, 2); plus
    x = 1, y = 0 and x at both ends of the mantissa reduction and next to them"""
    rng = np.random.default_rng(3)
    x = 10.0 ** rng.uniform(-4.0, 8.0, 20000)
    y = rng.uniform(-1.0, 1.0, 20000)
    s = np.sqrt(0.5)
    edge = np.array([1.0, s, np.nextafter(s, 0.0), np.nextafter(s, 1.0), 2.0 * s, np.nextafter(2.0 * s, 0.0),
                     np.nextafter(2.0 * s, 2.0), 0.5, 2.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)])
    x[:len(edge)] = edge
    x[len(edge):2 * len(edge)] = edge * 2.0 ** 7
    y[2 * len(edge)] = 0.0
    y[0] = 0.37
    return x, y


def test_pow_det_against_math_pow_within_the_stated_bound():
    import math
    from tests.visc_ref import pow_det, pow_det_bound
    x, y = _pow_grid()
    got = pow_det(x, y)
    want = np.array([math.pow(a, b) for a, b in zip(x, y)])
    ratio = np.abs(got - want) / want / pow_det_bound(x, y)
    print("pow_det worst error / bound", ratio.max())
    assert np.all(ratio <= 1.0)
    assert pow_det(1.0, 0.37) == 1.0 and np.all(pow_det(x, 0.0) == 1.0)
    # the stated bound sits several decades below float32's epsilon over the models' range |y ln x| <= 10
    assert (16.0 + 8.0 * 10.0) * 2.0 ** -53 < 1e-6 * 2.0 ** -23


def test_pow_det_equals_the_compiled_host_copy_bit_for_bit():
    import ctypes as C
    import cfd2_amd.solver  # noqa: F401  (binds the argument types)
    from cfd2_amd import _ffi
    from tests.visc_ref import pow_det
    x, y = _pow_grid()
    out = np.zeros_like(x)
    dp = C.POINTER(C.c_double)
    _ffi.check(_ffi.lib().cfd_debug_pow_det(x.ctypes.data_as(dp), y.ctypes.data_as(dp), out.ctypes.data_as(dp), len(x)),
               "cfd_debug_pow_det")
    assert np.array_equal(out.view(np.uint64), pow_det(x, y).view(np.uint64))


@pytest.mark.parametrize("name,kind,rotation", vc.MODEL_CASES)
def test_model_cases_meet_the_shape_condition(name, kind, rotation):
    """on the restatement alone, at every step: the GPU test cannot pass on an all-clamped field"""
    r = _ref(name)
    vc.setup_model(r, name, kind, rotation)
    for k in range(vc.MODEL_STEPS + 1):
        vc.check_case_shape(r.viscosity_field(), r.viscosity_stats(), vc.MODELS[name, kind], (name, kind, rotation, k))
        if k < vc.MODEL_STEPS:
            r.step()


def test_shear_rate_and_model_against_float64():
    """the restated shear rate against sqrt(2 S : S) of flow_checks' float64 gradients, and mu
    against the model with math.pow; a shear rate without the factor 2 is caught"""
    from tests.visc_ref import ViscosityModel

    class _NoFactor2(ViscosityModel):
        def shear_factor(self):
            return F(1)

    name, kind = "voronoi", "carreau"
    for cls, ok in ((ViscosityModel, True), (_NoFactor2, False)):
        r = ViscRefSolver(bc.mesh_of(name), M=bc.refmesh_of(name), model_class=cls, **bc.FIXED)
        vc.setup_model(r, name, kind, False)
        if ok:
            vk.check_model(bc.mesh_of(name), r, vc.MODELS[name, kind], kind)
        else:
            with pytest.raises(AssertionError, match="f64 "):
                vk.check_model(bc.mesh_of(name), r, vc.MODELS[name, kind], kind)


def test_model_refusals():
    r = _ref("rect")
    good = dict(K=0.02, n=0.6, gamma_min=1e-3, mu_min=0.001, mu_max=1.0)
    for bad in (dict(K=0.0), dict(K=np.nan), dict(gamma_min=0.0), dict(mu_min=2.0), dict(mu_min=0.0), dict(n=np.inf)):
        with pytest.raises(ValueError):
            r.set_viscosity_model("power_law", **{**good, **bad})
    with pytest.raises(ValueError):
        r.shear_rate()


def test_shear_thinning_sign_on_the_restatement():
    """where the GPU test's case comes from: mu at the obstacle's wall below mu far from walls"""
    near, far = vc.shear_thinning_flow(_ref("obstacle", fixed_outer=3, fixed_inner=10))
    print("mean mu at the wall", near, "far from walls", far)
    assert near < far
