"""Case list and drivers shared by tests/test_flow_f64.py (CPU oracle) and
tests/test_gpu_flow_f64.py (HIP path): the float64 checks of
tests/flow_checks.py on the meshes of tests/fv_cases.py, one channel mesh of
more than eight blocks and one strip below the distance floor.

HELPER MODULE, not a test.  Every driver takes the solver class, so the two
test modules run the same cases through the same code."""
import functools

import numpy as np

from cfd2_amd import default_config
from tests import flow_checks as fl
from tests import fv_cases as fc

BLOCK = 256  # cells per block of the one-thread-per-cell kernels (device_util.hpp kBlock)
# channel13: ceil(N / 256) is at least 9 and no multiple of 8, so the 8-way
# block remapping of row_id() has a quotient and a remainder.
# tiny5: a strip of 5 cells of side 4e-7: every distance sum (4e-7) and every
# projected distance (4e-7 internal, 2e-7 boundary) is below the 1e-6 floor,
# decidedly: lambda takes its degenerate 1/2 and dist_n the floor.
MESHES = fc.MESHES + ["channel13", "tiny5"]
SCHEMES, TIME_SCHEMES, DENSITIES = (0, 1, 2), (0, 1), (1.0, 1000.0)
UPDATE_MESHES = ["strip7", "voronoi", "channel13"]
BUOYANT_MESHES = ["channel_obstacle", "voronoi"]
GRAVITY = (0.3, -9.81)
MAX_EITHER_SHARE = 0.01  # of a case's faces
CHECKS = ("check_flux", "check_gradients", "check_d_p", "check_matrix_entries", "check_rhs")


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "channel13":
        from tests.meshes import channel_obstacle
        return channel_obstacle(h=0.03, smooth_iters=20)
    if name == "tiny5":
        from tests.synthetic import strip
        return strip(5, h=4e-7)
    return fc.mesh_of(name)


def blocks(mesh):
    return -(-mesh.num_cells() // BLOCK)


def driving_fields(mesh):
    """Two driving fields (beta, ref, phi), smooth and non-uniform."""
    a = mesh.arrays()
    x, y = a["cell_cx"], a["cell_cy"]
    return [(0.5, 0.2, 0.5 + 0.4 * np.sin(2.3 * x) * np.cos(3.1 * y)),
            (-0.125, 0.7, 1.0 - 0.6 * np.cos(1.9 * x) * np.sin(2.7 * y + 0.1))]


def flow_state(cls, mesh, scheme, time_scheme, density, buoyant=False):
    """fv_cases.random_state_solver; the state before the prepare is read, one
    debug_prepare_assemble(True) runs, its outputs are read."""
    s = fc.random_state_solver(cls, mesh, scheme, time_scheme, density)
    fields = None
    if buoyant:
        fields = driving_fields(mesh)
        s.enable_scalars(len(fields))
        for k, (beta, ref, phi) in enumerate(fields):
            s.set_scalar_params(k, 0.0, 0.0)
            s.set_scalar(k, phi)
            s.set_scalar_buoyancy(k, beta, ref)
        s.set_gravity(*GRAVITY)
    st = fl.FlowState(mesh, s)
    s.debug_prepare_assemble(True)
    st.capture_post(s)
    if buoyant:
        st.buoyancy = (GRAVITY[0], GRAVITY[1], [(b, r, s.get_scalar(k)) for k, (b, r, _) in enumerate(fields)])
    fc._close(s)
    c = st.constants
    assert int(c.scheme) == scheme and int(c.time_scheme) == time_scheme and float(c.density) == density
    assert float(c.dt) == np.float32(0.75) * float(c.dt_old)  # BDF2: r = 0.75
    assert 0.0 < float(c.time) < float(c.ramp_time)  # the inlet ramp mid-way
    assert np.all(np.isfinite(st.p)) and (mesh.num_cells() == 1 or np.abs(st.p).max() > 0.0)
    assert np.abs(st.d_p_pre).max() > 0.0 and np.all(np.isfinite(st.rhs)) and np.abs(st.flux).max() > 0.0
    return st


def run_checks(st, what="", wrong=()):
    """Every staged check on one state; asserts that none is vacuous and that
    the either-branch faces are at most MAX_EITHER_SHARE.  Returns
    {check: result}."""
    a = st.arrays
    cells, faces = len(a["cell_vol"]), len(a["face_area"])
    out = {}
    for name in CHECKS:
        try:
            out[name] = getattr(fl, name)(st, wrong)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from e
    nnz = cells + 2 * int((a["face_neighbor"] != fl.NONE).sum())
    assert out["check_flux"]["faces"] == faces > 0  # every face
    assert out["check_gradients"]["cells"] == out["check_d_p"]["cells"] == cells > 0  # every cell
    assert out["check_matrix_entries"]["entries"] == 9 * nnz == len(st.coupled)  # every stored entry
    assert out["check_matrix_entries"]["scalar_entries"] == nnz == len(st.scalar)
    assert out["check_rhs"]["rows"] == 3 * cells  # every row
    for name, r in out.items():
        assert r.get("either", 0) <= MAX_EITHER_SHARE * faces, (what, name, r["either"], faces)
    return out


def run_mesh(cls, mesh_name, density, worst=None):
    """schemes {0, 1, 2} x time schemes {0, 1} of one mesh and density.
    worst: {check: (ratio, case)} updated in place.  Returns the coverage:
    face kinds, upwind directions, degenerate and floored faces seen."""
    mesh = mesh_of(mesh_name)
    cover = None
    for scheme in SCHEMES:
        for time_scheme in TIME_SCHEMES:
            what = f"{mesh_name} scheme {scheme} time scheme {time_scheme} rho {density}"
            out = run_checks(flow_state(cls, mesh, scheme, time_scheme, density), what)
            if worst is not None:
                for name, r in out.items():
                    if r["worst"] >= worst.get(name, (-1.0, ""))[0]:
                        worst[name] = (r["worst"], what)
            f, m = out["check_flux"], out["check_matrix_entries"]
            cover = {"kinds": f["kinds"], "degenerate": f["degenerate"], "floored": f["floored"],
                     "turned": f["turned"], "upwind": m["upwind"],
                     "either": max(r.get("either", 0) for r in out.values())}
    return cover


def run_buoyant(cls, mesh_name):
    """check_rhs with two driving fields and g = GRAVITY, scheme 2, BDF2,
    density 1000; the right-hand side differs from the non-buoyant one."""
    mesh = mesh_of(mesh_name)
    plain = flow_state(cls, mesh, 2, 1, 1000.0)
    st = flow_state(cls, mesh, 2, 1, 1000.0, buoyant=True)
    assert st.buoyancy is not None and len(st.buoyancy[2]) == 2
    out = run_checks(st, f"{mesh_name} buoyant")
    assert np.array_equal(st.flux, plain.flux) and np.array_equal(st.coupled, plain.coupled)
    moved = st.rhs.reshape(-1, 3) != plain.rhs.reshape(-1, 3)
    assert moved[:, :2].mean() > 0.9 and not moved[:, 2].any(), moved.mean(axis=0)
    with np.testing.assert_raises(AssertionError):  # and the check sees the term
        st.buoyancy = None
        fl.check_rhs(st)
    return out


def _update_solver(cls, mesh, fixed_outer):
    s = cls(mesh, config=default_config(fixed_outer=fixed_outer, fixed_inner=6, convergence_lag=0))
    rng = np.random.default_rng(4321)
    s.set_dt(0.002)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_u(rng.uniform(-1, 1, size=(mesh.num_cells(), 2)))
    s.set_p(rng.uniform(-1, 1, size=mesh.num_cells()))
    s.initialize_history()
    c = s.constants
    c.time = 0.05
    s.constants = c
    s.update_constants()
    return s


def run_update(cls, mesh_name):
    """fixed_outer = 1: the fields after one step against the fields before it
    and buffer 4.  fixed_outer = 2 from the same state: its first update is
    the first solver's (the step is deterministic), so the second update is
    checked from the first solver's fields, and the reported outer maxima
    are those of the second update exactly."""
    mesh = mesh_of(mesh_name)
    a = _update_solver(cls, mesh, 1)
    u0, p0 = np.array(a.get_u()).reshape(-1, 2), np.array(a.get_p())
    a.step()
    u1, p1 = np.array(a.get_u()).reshape(-1, 2), np.array(a.get_p())
    out = fl.check_update(a.constants, u0, p0, a.debug_buffer(4), u1, p1)
    assert out["cells"] == mesh.num_cells() and np.any(u1 != u0) and np.any(p1 != p0)
    fc._close(a)
    b = _update_solver(cls, mesh, 2)
    b.step()
    u2, p2 = np.array(b.get_u()).reshape(-1, 2), np.array(b.get_p())
    out2 = fl.check_update(b.constants, u1, p1, b.debug_buffer(4), u2, p2)
    info = b.step_info()
    assert int(info.outer_iterations) == 2
    du, dp = fl.check_fold(u1, p1, u2, p2, info.outer_residual_u, info.outer_residual_p)
    fc._close(b)
    assert du > 0.0 and dp > 0.0
    return max(out["worst"], out2["worst"])
