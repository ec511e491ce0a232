"""Boussinesq buoyancy on the GPU (k_assemble_buoyant in csrc/hip/flux.hip,
k_buoyancy_force in csrc/hip/scalar.hip): bit for bit against the numpy float32
restatement tests/buoyancy_ref.py, against the term in float64 written from the
maths, and against the properties include/cfd2_amd.h ("Arithmetic of
buoyancy") promises.  Meshes and the plume case: tests/buoyancy_cases.py; the
CPU test tests/test_buoyancy.py holds the restatement to the same checks.
"""
import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver, default_config
from tests import buoyancy_cases as bc
from tests import refpy
from tests.buoyancy_ref import BuoyantRefSolver
from tests.test_gpu_parity import _assert_same_info
from tests.test_refpy import _same_step

pytestmark = pytest.mark.gpu

F = np.float32
EPS32 = 2.0 ** -24
PLUME_FIXED = dict(fixed_outer=3, fixed_inner=10)  # tests/test_buoyancy.py settled the case with it


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def _gpu(name, **cfg):
    return GpuSolver(bc.mesh_of(name), config=default_config(**cfg))


def _bit_equality(name, time_scheme, scheme, two):
    mesh = bc.mesh_of(name)
    g = _gpu(name, **bc.FIXED)
    r = BuoyantRefSolver(mesh, M=bc.refmesh_of(name), **bc.FIXED)
    # units4 under the AMG preconditioner: the Jacobi one runs 149 pressure sweeps per
    # application there, which the numpy restatement needs 20 s for; AMG takes it half that
    precond = 1 if name == "units4" else 0
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=time_scheme, scheme=scheme, precond=precond)
        bc.setup_scalars(s, mesh, two=two)
    assert g.buoyancy() == r.buoyancy() and g.buoyancy()["active"]
    for k in range(3):
        ctx = f"{name} time_scheme {time_scheme} scheme {scheme} step {k}"
        g.step()
        r.step()
        _same_step(g, r, ctx)
        g.advance_scalars()
        r.advance_scalars()
        for f in range(2 if two else 1):
            assert np.array_equal(_bits(g.get_scalar(f)), _bits(r.get_scalar(f))), (ctx, f)
    g.close()


@pytest.mark.parametrize("time_scheme,scheme", bc.SCHEMES)
@pytest.mark.parametrize("name", bc.MESHES)
def test_bit_exact_against_the_restatement(name, time_scheme, scheme):
    """check 1: 3 alternating step() / advance_scalars() with one driving field:
    u, p, d_p, the step info and the field == tests/buoyancy_ref.py after every step"""
    _bit_equality(name, time_scheme, scheme, False)


def test_bit_exact_two_driving_fields():
    """check 1 with two driving fields of different beta and ref: the field order"""
    _bit_equality("obstacle", 0, 0, True)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("name", bc.MESHES + bc.STRIPS)
def test_float64_identity(name, two):
    """check 2, from the maths alone: with t64 = -vol rho sum_f beta_f (phi_f - ref_f) g in
    float64, per cell and component
        |rhs_on - rhs_off - t64| <= 8 eps32 (|rhs_on| + vol rho sum_f |beta_f| (|phi_f| + |ref_f|) |g_c|).
    8: the term takes at most five float32 roundings (d, beta d, vol rho, their
    product, times g) on a magnitude below the second summand, the final
    subtraction one on |rhs_on|; a second field adds one of each.  rhs_p and the
    three diagonal inverses keep their bits."""
    mesh = bc.mesh_of(name)
    s = _gpu(name)
    bc.setup_flow(s, mesh, scheme=2)
    bc.setup_scalars(s, mesh, two=two)
    u = bc.fields(mesh)[0]
    got = {}
    for on in (True, False):
        s.set_gravity(*(bc.G if on else (0.0, 0.0)))
        s.set_u(u)  # the same state for both: prepare refreshes d_p in place
        s.debug_prepare_assemble()
        got[on] = [s.debug_buffer(i) for i in (3, 5, 6, 7)]
    s.set_gravity(*bc.G)
    b = s.buoyancy()
    vol = mesh.arrays()["cell_vol"].astype(F).astype(np.float64)
    rho = float(s.constants.density)
    term, mag = np.zeros(len(vol)), np.zeros(len(vol))
    for f, (beta, ref) in enumerate(zip(b["beta"], b["ref"])):
        phi = s.get_scalar(f)
        term += beta * (phi - ref)
        mag += abs(beta) * (np.abs(phi) + abs(ref))
    gv = np.asarray(b["g"], np.float64)
    t64 = -(vol * rho * term)[:, None] * gv[None, :]
    bound_t = (vol * rho * mag)[:, None] * np.abs(gv)[None, :]
    on, off = (np.asarray(got[k][0], np.float64).reshape(-1, 3) for k in (True, False))
    err = np.abs(on[:, :2] - off[:, :2] - t64)
    bound = 8.0 * EPS32 * (np.abs(on[:, :2]) + bound_t)
    print(f"{name} two={two}: worst error / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}, max |t64| {np.abs(t64).max():.3e}")
    assert np.abs(t64).max() > 0.0
    assert np.all(err <= bound)
    assert np.array_equal(_bits(on[:, 2]), _bits(off[:, 2]))
    for i in (1, 2, 3):
        assert np.array_equal(_bits(got[True][i]), _bits(got[False][i])), i
    s.close()


def _two_steps(s):
    out = []
    for _ in range(2):
        s.step()
        out.append([s.get_u(), s.get_p(), s.get_d_p()])
    return out


@pytest.mark.parametrize("form", ["beta0", "g0", "phi=ref"])
def test_noop_forms(form):
    """check 3: every beta 0, g = (0, 0) (the plain kernel) or phi == ref
    everywhere (the buoyant kernel adding zeros): 2 steps == an untouched handle"""
    mesh = bc.mesh_of("obstacle")
    a, b = _gpu("obstacle", **bc.FIXED), _gpu("obstacle", **bc.FIXED)
    for s in (a, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
    bc.setup_scalars(b, mesh, two=True)
    if form == "beta0":
        b.set_scalar_buoyancy(0, 0.0, bc.REF)
        b.set_scalar_buoyancy(1, 0.0, 0.7)
    elif form == "g0":
        b.set_gravity(0.0, 0.0)
    else:
        b.set_scalar_buoyancy(1, 0.0, 0.0)
        b.set_scalar(0, np.full(mesh.num_cells(), float(F(bc.REF))))
    assert b.buoyancy()["active"] == (form == "phi=ref")
    if form == "phi=ref":
        for s in (a, b):
            s.debug_prepare_assemble()
        assert np.array_equal(_bits(a.debug_buffer(3)), _bits(b.debug_buffer(3)))
        for s in (a, b):  # back to the state of setup_flow
            s.set_u(bc.fields(mesh)[0])
    for k, (x, y) in enumerate(zip(_two_steps(a), _two_steps(b))):
        for p, q in zip(x, y):
            assert np.array_equal(p, q), (form, k)
    _assert_same_info(a, b, form)
    a.close()
    b.close()


def test_enable_clears_beta():
    """check 3: enable_scalars(0) and a re-enable: every beta and ref is 0 again, g stays"""
    mesh = bc.mesh_of("rect")
    s = _gpu("rect")
    bc.setup_scalars(s, mesh, two=True)
    assert s.buoyancy() == dict(g=(float(F(bc.G[0])), float(F(bc.G[1]))), beta=[bc.BETA, -0.125],
                                ref=[float(F(bc.REF)), float(F(0.7))], active=True)
    s.enable_scalars(0)
    assert s.buoyancy() == dict(g=(float(F(bc.G[0])), float(F(bc.G[1]))), beta=[], ref=[], active=False)
    s.enable_scalars(2)
    assert s.buoyancy() == dict(g=(float(F(bc.G[0])), float(F(bc.G[1]))), beta=[0.0, 0.0], ref=[0.0, 0.0], active=False)
    s.close()


def _force64(s, mesh):
    """the per-cell float64 terms from the solver's own settings, summed in the canonical
    order: the volumes and operand order of tests/test_gpu_scalar.py _check_stats"""
    b = s.buoyancy()
    vol = mesh.arrays()["cell_vol"].astype(F).astype(np.float64)
    vr = vol * float(s.constants.density)
    tx, ty = np.zeros(len(vol)), np.zeros(len(vol))
    n = 0
    for f, (beta, ref) in enumerate(zip(b["beta"], b["ref"])):
        if beta == 0.0:
            continue
        n += 1
        m = (vr * beta) * (s.get_scalar(f) - ref)
        tx = tx - m * b["g"][0]
        ty = ty - m * b["g"][1]
    return float(refpy.canon_sum(tx)), float(refpy.canon_sum(ty)), n


@pytest.mark.parametrize("name,two", [("obstacle", False), ("obstacle", True), ("units4", False)])
def test_buoyancy_force(name, two):
    """check 4: == refpy.canon_sum of the float64 per-cell terms, bit for bit"""
    mesh = bc.mesh_of(name)
    if name == "units4":
        assert refpy._geom(mesh.num_cells())[0] >= 4
    s = _gpu(name)
    s.set_density(bc.DENSITY)
    bc.setup_scalars(s, mesh, two=two)
    got = s.buoyancy_force()
    want = _force64(s, mesh)
    print(f"{name} two={two}: force {got}")
    assert tuple(got) == want and got.fields == (2 if two else 1)
    assert got.fx != 0.0 and got.fy != 0.0
    s.close()


def test_buoyancy_force_uniform_and_off():
    """check 4: a uniform field gives -rho beta (phi - ref) g times the canonical
    volume sum (every factor a power of two, so exactly); no driving field: (+0, +0)"""
    mesh = bc.mesh_of("obstacle")
    s = _gpu("obstacle")
    s.set_density(2.0)
    s.enable_scalars(2)
    s.set_gravity(0.25, -8.0)
    off = s.buoyancy_force()
    assert tuple(off) == (0.0, 0.0, 0) and not np.signbit(off.fx) and not np.signbit(off.fy)
    s.set_scalar(1, np.full(mesh.num_cells(), 0.75))
    s.set_scalar_buoyancy(1, 0.5, 0.25)
    vsum = float(refpy.canon_sum(mesh.arrays()["cell_vol"].astype(F).astype(np.float64)))
    assert tuple(s.buoyancy_force()) == (-2.0 * 0.5 * 0.5 * 0.25 * vsum, 2.0 * 0.5 * 0.5 * 8.0 * vsum, 1)
    s.set_gravity(0.0, 0.0)
    assert tuple(s.buoyancy_force()) == (0.0, 0.0, 1)
    s.close()


def test_plume_rises():
    """check 5: the obstacle mesh at rest, the obstacle's faces at phi = 1: at
    rest with beta = 0; with buoyancy the fluid above the obstacle rises, and
    sinks under g = (0, +9.81); the body force points the same way.  K, beta, dt
    and the box: tests/buoyancy_cases.py, settled on the CPU.  max_divergence is
    printed: the Rhie-Chow flux does not see the body force."""
    mesh = bc.mesh_of("obstacle")
    p = bc.PLUME
    rest = _gpu("obstacle", **PLUME_FIXED)
    assert bc.run_plume(rest, mesh, 0.0, p["g"]) == (0.0, 0.0)
    assert rest.get_scalar(0).max() > 0.0
    div0 = rest.flow_diagnostics().max_divergence
    rest.close()
    up = _gpu("obstacle", **PLUME_FIXED)
    v_up, umax = bc.run_plume(up, mesh, p["beta"], p["g"])
    f_up = up.buoyancy_force()
    d = up.flow_diagnostics()
    print(f"plume: mean v above {v_up:.3e}, max |u| {umax:.3e}, force {tuple(f_up)}, max_divergence {d.max_divergence:.3e} "
          f"(beta = 0: {div0:.3e}), max_speed {d.max_speed:.3e}")
    up.close()
    down = _gpu("obstacle", **PLUME_FIXED)
    v_down, _ = bc.run_plume(down, mesh, p["beta"], (0.0, 9.81))
    f_down = down.buoyancy_force()
    down.close()
    assert v_up > 0.0 and f_up.fy > 0.0
    assert v_down < 0.0 and f_down.fy < 0.0


def test_refusals():
    """check 6: a group member refuses ("one GPU"); scalars not enabled, a bad
    field index and a NaN beta, ref or g return CFD_ERR_INVALID with a message"""
    mesh = bc.mesh_of("obstacle")
    g = GpuGroup(mesh, 2)
    for r in g.ranks:
        with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
            r.set_scalar_buoyancy(0, 1.0)
        with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
            r.set_gravity(0.0, -9.81)
        with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
            r.buoyancy_force()
    with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
        g.set_scalar_buoyancy(0, 1.0)
    g.close()
    s = GpuSolver(mesh)
    for call in (lambda: s.set_scalar_buoyancy(0, 1.0), s.buoyancy_force):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    s.enable_scalars(2)
    for f in (-1, 2):
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.set_scalar_buoyancy(f, 1.0)
    nan, inf = float("nan"), float("inf")
    for beta, ref in ((nan, 0.0), (1.0, nan), (inf, 0.0), (1.0, -inf)):
        with pytest.raises(RuntimeError, match=r"status 1.*finite"):
            s.set_scalar_buoyancy(0, beta, ref)
    for gx, gy in ((nan, 0.0), (0.0, nan), (inf, 0.0)):
        with pytest.raises(RuntimeError, match=r"status 1.*finite"):
            s.set_gravity(gx, gy)
    assert s.buoyancy() == dict(g=(0.0, 0.0), beta=[0.0, 0.0], ref=[0.0, 0.0], active=False)  # a refused call changes nothing
    s.close()
