"""Cases shared by tests/test_penalty.py (CPU: the restatement
tests/penalty_ref.py against the float64 checks tests/penalty_checks.py) and
tests/test_gpu_penalty.py (the HIP path against both).  HELPER MODULE, not a test.

The meshes, the flow state, the schemes and the standard boundary-velocity
selection are those of tests/bcvel_cases.py (imported, not copied).

The test field (`field`), from a seeded generator, every cell drawn on its own:
sigma log-uniform over six decades, 1 .. 1e6 (the time coefficient rho / dt of
bcvel_cases.setup_flow is 1500: both sides of it), about 30 % exact zeros;
forch log-uniform over four decades with about 30 % exact zeros; the target
uniform in [-1, 1]^2.  Every category is asserted to be populated: cells with
neither, with sigma only, with forch only, with both.
"""
import numpy as np

from cfd2_amd import penalty as builders
from cfd2_amd.mesh import RectangularChannel, generate_cut_cell_mesh
from tests import bcvel_cases as bc
from tests import flow_checks as fc
from tests import fv_checks as fv
from tests.visc_cases import _RefBuffers, ref_system, system  # noqa: F401  the same buffers

F = np.float32
SCALE = 0.75  # target_scale of the cases: not 1, so a dropped scale shows


def field(name, seed=9):
    n = bc.mesh_of(name).num_cells()
    rng = np.random.default_rng(seed)
    sigma = np.where(rng.uniform(size=n) < 0.3, 0.0, 10.0 ** rng.uniform(0.0, 6.0, n)).astype(F)
    forch = np.where(rng.uniform(size=n) < 0.3, 0.0, 10.0 ** rng.uniform(0.0, 4.0, n)).astype(F)
    target = rng.uniform(-1.0, 1.0, (n, 2)).astype(F)
    s0, f0 = sigma == 0, forch == 0
    for cat in (s0 & f0, ~s0 & f0, s0 & ~f0, ~s0 & ~f0):
        assert cat.sum() >= 2, (name, int(cat.sum()))
    live = sigma[~s0]
    assert live.max() / live.min() > (1e3 if n < 100 else 1e5)
    return sigma, forch, target


# (forch set, target set): each null and each set; the mixed forms run in test_gpu_penalty's replacement test
FORMS = [(False, False), (True, True)]


def set_field(s, name, forch=True, target=True, seed=9):
    sg, fo, tg = field(name, seed)
    s.set_penalty(sg, fo if forch else None, tg if target else None)
    s.set_penalty_scale(SCALE)
    return sg, (fo if forch else None), (tg if target else None)


# ---- the float64 checks on either solver ------------------------------------------
def run_checks(make, name, time_scheme, wrong=(), forch=True, target=True):
    """make(): a fresh solver (GpuSolver or PenaltyRefSolver) on mesh `name`.  Two of
    them take one step each from bcvel_cases.setup_flow's state (so the iterate differs
    from u_old), one with the test field; then debug_prepare_assemble on each and
    every check of tests/penalty_checks.py.  Returns the worst error / bound per check."""
    from tests import penalty_checks as pk
    mesh = bc.mesh_of(name)
    s, plain = make(), make()
    states = []
    for q in (s, plain):
        bc.setup_flow(q, mesh, time_scheme=time_scheme, scheme=0)
    sg, fo, tg = set_field(s, name, forch, target)
    s.step()
    _copy_state(s, plain)  # the plain solver takes the penalised one's state: the same iterate, u_old and d_p
    for q in (s, plain):
        dev = q if hasattr(q, "debug_buffer") else _RefBuffers(q)
        st = fc.FlowState(mesh, dev)
        dev.debug_prepare_assemble()
        states.append(st.capture_post(dev))
    assert np.abs(states[0].u - states[0].u_old).max() > 1e-3  # u_old is not the iterate
    res = pk.check_all(states[0], states[1], sg, fo, tg, SCALE, wrong)
    for q in (s, plain):
        if hasattr(q, "close"):
            q.close()
    return res


def _copy_state(src, dst):
    """dst takes src's whole ring (u, p, d_p, grad_p, both old levels) and time"""
    if hasattr(src, "ring"):
        dst.ring = [r.copy() for r in src.ring]
        dst.step_index, dst.i_state, dst.i_old, dst.i_old_old = src.step_index, src.i_state, src.i_old, src.i_old_old
        dst.c.time = src.c.time
        return
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "pen.state")
        src.save_state(path)
        dst.load_state(path)


# ---- a mesh above one reduction segment ----------------------------------------------
def segment_mesh():
    """a generate_cut_cell_mesh rectangle just above 32 768 cells (kernels.hpp red_geom): a
    segment is then G = 2 chunks and a unit U = 2 chunks, so the unit, segment and total trees
    all have more than one input, k_penalty_force runs in 34 blocks, and the last block, chunk
    and segment are partly empty"""
    mesh = generate_cut_cell_mesh(RectangularChannel(length=1.0, height=0.75), 0.0047, 0.0047, 1.2, (1.0, 0.75))
    n = mesh.num_cells()
    assert 32768 <= n < 40000 and n % 512 != 0 and n % 1024 != 0, n
    return mesh


# ---- a solid stops the flow ----------------------------------------------------------
DISC = dict(centre=(0.5, 0.375), radius=0.2, eta=1e-4, dt=0.01, steps=4)


def setup_channel(s, mesh, dt, viscosity=0.01, alpha_u=1.0):
    s.set_dt(dt)
    s.set_dt(dt)
    s.set_viscosity(viscosity)
    s.set_density(1.0)
    s.set_alpha_u(alpha_u)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    s.set_scheme(0)
    s.set_time_scheme(0)
    c = s.constants
    c.inlet_velocity = 1.0
    c.ramp_time = 0.1
    c.time = 1.0  # past the ramp
    s.constants = c
    s.initialize_history()


def solid_disc_case(s):
    """solid_disc at rest in the rectangular channel, a few solved steps; returns what
    solid_bound needs: (penalised cells, V sigma of them)"""
    mesh = bc.mesh_of("rect")
    setup_channel(s, mesh, DISC["dt"])
    f = builders.solid_disc(mesh, DISC["centre"], DISC["radius"], DISC["eta"], 1.0, DISC["dt"])
    s.set_penalty(**f)
    for _ in range(DISC["steps"]):
        s.step()
    cells = np.nonzero(f["sigma"] > 0)[0]
    assert len(cells) >= 4
    vol = np.asarray(mesh.arrays()["cell_vol"], F).astype(np.float64)
    return cells, vol[cells] * np.asarray(f["sigma"], F).astype(np.float64)[cells]


SOLID_CFG = dict(fixed_outer=3, fixed_inner=0)  # the linear solve stops on its own tolerance


def solid_bound(mesh, cells, pen, coupled, rhs, x, rtol):
    """Row i (u or v) of the last solved system reads, with B_i >= 0 the unpenalised diagonal
    (a sum of the positive time coefficient, diffusion coefficients and outflow fluxes),
        (B_i + pen_i) x_i + sum_{j != i} A_ij x_j = b_i - r_i     (target 0: nothing in b from the penalty)
    so  |x_i| <= (|b_i| + sum_{j != i} |A_ij x_j| + |r_i|) / (B_i + pen_i) <= (R_i + tol) / pen_i.
    R_i is the float64 sum of the absolute values of the row's other terms.  pen_i = V_i sigma_i
    comes from the field that was set, NOT from the stored diagonal, and tol is the linear
    solver's stop tolerance rtol * |b|_2, which bounds every |r_i| of a solve that met it and
    does not depend on the solution: a diagonal without the penalty, or a solve that did not
    converge, leaves |x_i| far above the bound.  Returns (|x| [cells, 2], bound [cells, 2])."""
    A = fv._coupled_csr(mesh, np.asarray(coupled, np.float64))
    x, b = np.asarray(x, np.float64), np.asarray(rhs, np.float64)
    tol = float(rtol) * np.sqrt((b * b).sum())
    absA = abs(A)
    got, bound = np.zeros((len(cells), 2)), np.zeros((len(cells), 2))
    for k in (0, 1):
        rows = 3 * cells + k
        others = absA[rows] @ np.abs(x) - np.abs(A.diagonal()[rows] * x[rows])
        got[:, k], bound[:, k] = np.abs(x[rows]), (np.abs(b[rows]) + others + tol) / pen
    return got, bound


# ---- the Darcy plug --------------------------------------------------------------------
# sigma = 20 against mu / h^2 = 0.01 / 0.125^2 = 0.64; the slab spans the channel's height
# and the three cell columns x = 0.4375, 0.5625, 0.6875.  The time step is small on purpose:
# the continuity row of the coupled system carries the compact pressure Laplacian d_p grad p
# without the interpolated-gradient term that compensates it, so at a steady state the mass
# flux is u (1 + sigma d_p) with d_p ~ 1 / (rho / dt + sigma), and the drop falls short of
# sigma U L by about sigma dt / rho (0.1 here; 0.58 was measured with sigma = 200, dt = 0.05,
# where sigma d_p ~ 1).  300 steps reach the steady state: the tests assert that the last step
# moves no velocity by more than STEADY.
DARCY = dict(sigma=20.0, x0=0.375, x1=0.75, U=1.0, dt=0.005, steps=300)
# |dp / (sigma U L) - 1| of the restatement on the CPU (tests/test_penalty.py measures it again
# and holds this constant to it): the GPU assertion is twice this; the case is wrongly built if
# it reaches 0.25
DARCY_MEASURED = 0.1311647733052571


STEADY = 1e-5  # the step's own convergence threshold on max |du| (coupled_solver.rs: res_u < 1e-5)


def darcy_case(s):
    """the slab, DARCY["steps"] steps; returns the last step's max |du|, which the tests hold to STEADY"""
    mesh = bc.mesh_of("rect")
    setup_channel(s, mesh, DARCY["dt"], alpha_u=0.7)
    s.set_penalty(**builders.porous_box(mesh, (DARCY["x0"], 0.0, DARCY["x1"], bc.H_RECT), DARCY["sigma"]))
    for _ in range(DARCY["steps"] - 1):
        s.step()
    before = np.asarray(s.get_u(), np.float64).reshape(-1, 2).copy()
    s.step()
    return float(np.abs(np.asarray(s.get_u(), np.float64).reshape(-1, 2) - before).max())


def darcy_deviation(s):
    """the pressure drop between the slab's ends along the centre line (the mean of the two
    rows next to it; the pressure at an end face is the mean of the two cell centres it lies
    between) against sigma U L; returns the deviation"""
    a = bc.mesh_of("rect").arrays()
    x, y = a["cell_cx"], a["cell_cy"]
    p = np.asarray(s.get_p(), np.float64)
    mid = np.abs(y - 0.5 * bc.H_RECT) < 0.07

    def at(xf):
        return p[mid & (np.abs(x - xf) < 0.07)].mean()

    drop = at(DARCY["x0"]) - at(DARCY["x1"])
    want = DARCY["sigma"] * DARCY["U"] * (DARCY["x1"] - DARCY["x0"])
    return abs(drop / want - 1.0)
