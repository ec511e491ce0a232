"""Cases shared by tests/test_visc.py (CPU: the restatement tests/visc_ref.py
against the float64 checks tests/visc_checks.py) and tests/test_gpu_visc.py (the
HIP path against both).  HELPER MODULE, not a test.

The meshes, the flow state, the schemes and the standard boundary-velocity
selection are those of tests/bcvel_cases.py (imported, not copied).

The test field (`field`): log-uniform over two decades around the constant
viscosity of bcvel_cases.setup_flow (0.01), from a seeded generator, every cell
drawn on its own: neighbours differ by factors up to 100, no value equals the
constant (asserted), all positive.
"""
import numpy as np

from tests import bcvel_cases as bc
from tests import flow_checks as fc

F = np.float32
NU = 0.01  # bcvel_cases.setup_flow's set_viscosity


def field(name, seed=5):
    mesh = bc.mesh_of(name)
    n = mesh.num_cells()
    mu = (NU * 10.0 ** np.random.default_rng(seed).uniform(-1.0, 1.0, n)).astype(F)
    a = mesh.arrays()
    inner = a["face_neighbor"] != 0xFFFFFFFF
    o, nb = a["face_owner"][inner].astype(np.int64), a["face_neighbor"][inner].astype(np.int64)
    ratio = np.maximum(mu[o] / mu[nb], mu[nb] / mu[o])
    assert np.all(mu > 0) and not np.any(mu == F(NU)) and ratio.max() > (15.0 if n < 100 else 50.0), ratio.max()
    return mu


def system(s):
    """debug_prepare_assemble on a GpuSolver: fluxes, gradients, rhs, inverses, both matrices, grad_p"""
    s.debug_prepare_assemble()
    return [s.debug_buffer(i) for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10)]


def ref_system(r):
    """the same of a ViscRefSolver, in system()'s order (without grad_p: the state holds it)"""
    o = r.debug_prepare_assemble()
    return [o["fluxes"], o["grad_u"].reshape(-1), o["grad_v"].reshape(-1), o["rhs"], o["dui"], o["dvi"], o["dpi"],
            o["sv"], o["mv"]]


# ---- the float64 checks on either solver ------------------------------------------
class _RefBuffers:
    """debug_buffer / debug_prepare_assemble of a GpuSolver over a ViscRefSolver, as
    flow_checks.FlowState reads them"""

    def __init__(self, r):
        self.r, self.constants, self.o = r, r.constants, None

    def get_u(self):
        return self.r.get_u()

    def get_p(self):
        return self.r.get_p()

    def get_d_p(self):
        return self.r.get_d_p()

    def debug_prepare_assemble(self):
        self.o = self.r.debug_prepare_assemble()

    def debug_buffer(self, i):
        r, o = self.r, self.o
        if i == 10:
            return r.ring[r.i_state].grad_p.reshape(-1)
        if i == 11:
            return r.ring[r.i_old].u.reshape(-1)
        if i == 12:
            return r.ring[r.i_old_old].u.reshape(-1)
        return {0: o["fluxes"], 1: o["grad_u"].reshape(-1), 2: o["grad_v"].reshape(-1), 3: o["rhs"], 8: o["sv"],
                9: o["mv"]}[i]


def run_checks(s, name, time_scheme, mu=None, wrong=()):
    """the test field on a fresh state of solver s (GpuSolver or ViscRefSolver; scheme 0,
    a force region round the standard walls), then every check of tests/visc_checks.py;
    returns the worst error / bound per check"""
    from tests import visc_checks as vk
    mesh = bc.mesh_of(name)
    mu = field(name) if mu is None else mu
    bc.setup_flow(s, mesh, time_scheme=time_scheme, scheme=0)
    s.set_viscosity_field(mu)
    s.set_force_region(*bc.wall_box(name)["box"])
    dev = s if hasattr(s, "debug_buffer") else _RefBuffers(s)
    st = fc.FlowState(mesh, dev)
    dev.debug_prepare_assemble()
    st.capture_post(dev)
    fv = tuple(s.flow_diagnostics().force_viscous) if hasattr(s, "flow_diagnostics") else tuple(s.wall_force()[1])
    return vk.check_all(st, mu, bc.wall_box(name)["box"], fv, wrong)


# ---- the models ---------------------------------------------------------------------
# n = 0.6 for the power law (the issue's).  K, lambda and the clamps are chosen per mesh so
# that the restatement ALONE meets the case-shape condition below at every step of the
# 4-step case, with and without the standard selection (tests/test_visc.py asserts it on the
# CPU): the shear rates of bc.setup_flow's state run 0.4 .. 17 on obstacle, 3 .. 67 on voronoi.
MODEL_STEPS = 4
CARREAU = dict(mu0=0.05, mu_inf=0.003, lam=1.0, n=0.4, mu_min=0.012, mu_max=1.0)
MODELS = {
    ("obstacle", "power_law"): dict(K=0.02, n=0.6, gamma_min=1e-3, mu_min=0.008, mu_max=0.03),
    ("voronoi", "power_law"): dict(K=0.05, n=0.6, gamma_min=1e-3, mu_min=0.004, mu_max=0.022),
    ("obstacle", "carreau"): CARREAU,
    ("voronoi", "carreau"): CARREAU,
}
MODEL_CASES = [(name, kind, rot) for (name, kind) in MODELS for rot in (False, True)]


def setup_model(s, name, kind, rotation):
    mesh = bc.mesh_of(name)
    bc.setup_flow(s, mesh, time_scheme=1, scheme=1)
    if rotation:
        bc.select(s, name)
    s.set_viscosity_model(kind, **MODELS[name, kind])


def check_case_shape(mu, stats, par, ctx):
    """at least 5 % of the cells clamped, at least 50 % unclamped, the unclamped
    viscosities spanning at least a factor 3"""
    n = len(mu)
    clamped = stats["clamped_below"] + stats["clamped_above"]
    free = mu[(mu > F(par["mu_min"])) & (mu < F(par["mu_max"]))]
    assert clamped >= 0.05 * n, (ctx, clamped, n)
    assert n - clamped >= 0.5 * n, (ctx, clamped, n)
    assert len(free) > 0 and free.max() / free.min() >= 3.0, (ctx, float(free.max() / free.min()))


def wall_and_far_cells(name):
    """(cells owning a wall face of the obstacle, the tenth of the cells farthest from any wall face)"""
    a = bc.mesh_of(name).arrays()
    wall = bc.boundary_faces(a, 3)
    x, y = a["face_cx"][wall], a["face_cy"][wall]
    x0, y0, x1, y1 = bc.OBSTACLE_BOX
    on = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    d = np.min(np.hypot(a["cell_cx"][:, None] - x[None, :], a["cell_cy"][:, None] - y[None, :]), axis=1)
    return np.unique(a["face_owner"][wall[on]]), np.argsort(d)[-len(d) // 10:]


def shear_thinning_flow(s, name="obstacle"):
    """a power-law fluid (n = 0.6) round the obstacle from rest, 3 solved steps; returns
    (mean mu over the obstacle's wall cells, mean mu over the far cells)"""
    s.set_dt(0.01)
    s.set_dt(0.01)
    s.set_viscosity(0.01)
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    c = s.constants
    c.inlet_velocity, c.ramp_time = 1.0, 0.02
    s.constants = c
    s.initialize_history()
    s.set_viscosity_model("power_law", K=0.01, n=0.6, gamma_min=1e-2, mu_min=1e-4, mu_max=1.0)
    for _ in range(3):
        s.step()
    s.viscosity_evaluate()
    mu = np.asarray(s.viscosity_field(), np.float64)
    near, far = wall_and_far_cells(name)
    return float(mu[near].mean()), float(mu[far].mean())
