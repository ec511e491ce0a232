"""Volume penalisation on the GPU (k_prepare_pen, k_assemble_pen in
csrc/hip/flux.hip; k_penalty_force in csrc/hip/penalty.hip): bit for bit against
the numpy float32 restatement tests/penalty_ref.py, against the float64 checks
tests/penalty_checks.py written from the definition, and against the
properties include/cfd2_amd.h ("Arithmetic of volume penalisation") promises.
Cases: tests/penalty_cases.py; the CPU test tests/test_penalty.py holds the
restatement to the same checks.
"""
import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver, default_config
from cfd2_amd import penalty as builders
from tests import bcvel_cases as bc
from tests import buoyancy_cases as buoy
from tests import penalty_cases as pc
from tests import penalty_checks as pk
from tests import refpy
from tests import visc_cases as vc
from tests.penalty_ref import PenaltyRefSolver

pytestmark = pytest.mark.gpu

F = np.float32


def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def _bits64(x):
    return np.asarray(x, np.float64).view(np.uint64)


def _gpu(name, **cfg):
    return GpuSolver(bc.mesh_of(name), config=default_config(**(cfg or bc.FIXED)))


def _ref(name, **cfg):
    return PenaltyRefSolver(bc.mesh_of(name), M=bc.refmesh_of(name), **(cfg or bc.FIXED))


def _same_bits(g, r, ctx):
    for what, a, b in (("u", g.get_u(), r.get_u()), ("p", g.get_p(), r.get_p()), ("d_p", g.get_d_p(), r.get_d_p())):
        assert np.array_equal(_bits(a), _bits(b)), f"{ctx}: {what} differs in {int((_bits(a) != _bits(b)).sum())} words"


def _same_system(g, r, ctx):
    """fluxes, gradients, rhs, the diagonal inverses, the scalar and the coupled matrix"""
    for i, (x, y) in enumerate(zip(pc.system(g), pc.ref_system(r))):
        assert np.array_equal(_bits(x), _bits(y)), f"{ctx}: system buffer {i} differs"


def _same_force(g, r, centre, box, ctx):
    got, want = g.penalty_force(centre, box), r.penalty_force(centre, box)
    vals = lambda f: [f[0][0], f[0][1], f[1], f[2]]  # noqa: E731
    assert np.array_equal(_bits64(vals(got)), _bits64(vals(want))) and got[3] == want[3], (ctx, got, want)
    return got


@pytest.mark.parametrize("forch,target", pc.FORMS)
@pytest.mark.parametrize("time_scheme,scheme", bc.SCHEMES)
@pytest.mark.parametrize("name", bc.MESHES)
def test_bit_exact_against_the_restatement(name, time_scheme, scheme, forch, target):
    """3 steps with the test field, forch and target each null and set: u, p, d_p after
    every step; the system after the last"""
    mesh = bc.mesh_of(name)
    g, r = _gpu(name), _ref(name)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=time_scheme, scheme=scheme)
        sg, fo, tg = pc.set_field(s, name, forch, target)
    got = g.penalty()
    assert got["active"] and got["target_scale"] == pc.SCALE and np.array_equal(_bits(got["sigma"]), _bits(sg))
    assert (got["forch"] is None) == (fo is None) and (got["target"] is None) == (tg is None)
    for k in range(3):
        g.step()
        r.step()
        _same_bits(g, r, f"{name} time_scheme {time_scheme} scheme {scheme} forch {forch} target {target} step {k}")
    _same_system(g, r, name)
    g.close()


def test_bit_exact_buoyant_with_moving_walls_and_a_viscosity_field():
    """the <true, true, true> PEN instances: a driving scalar field, the standard selection,
    the viscosity test field and the penalty; then with one of the three switched off at a time"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    g, r = _gpu(name), _ref(name)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
        buoy.setup_scalars(s, mesh)
        bc.select(s, name)
        s.set_viscosity_field(vc.field(name))
        pc.set_field(s, name)
    assert g.buoyancy()["active"] and g.boundary_velocity()["active"]
    for k in range(3):
        g.step()
        r.step()
        _same_bits(g, r, f"buoyant, moving walls, viscosity field, step {k}")
    _same_system(g, r, "buoyant, moving walls, viscosity field")
    for s in (g, r):
        s.clear_viscosity_field()  # <BUOY, BCV>
    g.step()
    r.step()
    _same_bits(g, r, "buoyant, moving walls")
    for s in (g, r):
        s.set_gravity(0.0, 0.0)  # <BCV>
    g.step()
    r.step()
    _same_bits(g, r, "moving walls")
    for s in (g, r):
        s.set_gravity(0.0, -9.81)  # <BUOY, VISC>
        s.clear_boundary_velocity()
        s.set_viscosity_field(vc.field(name))
    g.step()
    r.step()
    _same_bits(g, r, "buoyant, viscosity field")
    g.close()


@pytest.mark.parametrize("form", ["never", "cleared", "zero"])
def test_noop_forms(form):
    """never set and set then cleared (the kernels of before), and sigma == 0 with null forch
    and target (the PEN kernels: x + 0.0f == x for the positive diagonals): 2 steps, then state,
    both matrices, rhs, fluxes and gradients == an untouched handle, bit for bit"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    a, b = _gpu(name), _gpu(name)
    for s in (a, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
        bc.select(s, name)
    if form == "cleared":
        pc.set_field(b, name)
        b.clear_penalty()
    elif form == "zero":
        b.set_penalty(np.zeros(mesh.num_cells()))
    assert b.penalty()["active"] == (form == "zero")
    for k in range(2):
        a.step()
        b.step()
        _same_bits(a, b, f"{form} step {k}")
    for i, (x, y) in enumerate(zip(pc.system(a), pc.system(b))):
        assert np.array_equal(_bits(x), _bits(y)), (form, i)
    a.close()
    b.close()


def test_replacement_between_steps_under_graph_replay():
    """graph_enable(True): prepare and the assembly read the fields when they run and no
    graph holds them; a replaced field and a new target_scale take effect at the next step"""
    name = "obstacle"
    mesh = bc.mesh_of(name)
    g, r = _gpu(name), _ref(name)
    g.graph_enable(True)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=0, scheme=1)
    plan = [(9, 0.75, True, True), (10, 0.75, True, True), (10, -0.5, True, True), (None, 1.0, True, True),
            (11, 1.25, False, True), (11, 0.0, True, False)]  # (seed, target_scale, forch set, target set)
    for k, (seed, scale, forch, target) in enumerate(plan):
        for s in (g, r):
            if seed is None:
                s.clear_penalty()
            else:
                pc.set_field(s, name, forch=forch, target=target, seed=seed)
            s.set_penalty_scale(scale)
        g.step()
        r.step()
        _same_bits(g, r, f"graph step {k}")
    assert g.graph_stats()[2] > 0
    g.close()


@pytest.mark.parametrize("time_scheme", [0, 1])
@pytest.mark.parametrize("name", bc.MESHES)
def test_float64_checks_on_the_device(name, time_scheme):
    """tests/penalty_checks.py through debug_prepare_assemble and debug_buffer: d_p, every entry
    of both matrices, the right-hand side, the bit identity of the off-diagonals"""
    res = pc.run_checks(lambda: _gpu(name), name, time_scheme)
    print(name, time_scheme, res)
    assert res["off_diagonal_entries"] > 0


@pytest.mark.parametrize("name", ["voronoi", "segments"])
def test_penalty_force(name):
    """bits equal the restatement's; within the derived float64 bound of the definition; the
    box form splits two bodies and the parts add up to the whole within that bound.
    "segments": 34 080 cells, where a segment is two chunks: the unit, segment and total trees
    all have several inputs and k_penalty_force runs in 34 blocks"""
    if name == "segments":
        mesh = pc.segment_mesh()
        M = refpy.RefMesh(mesh)
        centre, boxes = (0.5, 0.375), [(0.0, 0.0, 0.45, 0.75), (0.45 + 1e-9, 0.0, 1.0, 0.75)]
    else:
        mesh, M = bc.mesh_of(name), bc.refmesh_of(name)
        centre, boxes = bc.OBSTACLE_CENTRE, [(0.0, 0.0, 1.0, 1.0), (1.0 + 1e-9, 0.0, 3.0, 1.0)]
    n = mesh.num_cells()
    g = GpuSolver(mesh, config=default_config(**bc.FIXED))
    r = PenaltyRefSolver(mesh, M=M, **bc.FIXED)
    rng = np.random.default_rng(21)
    sg = np.where(rng.uniform(size=n) < 0.3, 0.0, 10.0 ** rng.uniform(0.0, 4.0, n)).astype(F)
    fo = (10.0 ** rng.uniform(0.0, 2.0, n)).astype(F)
    tg = rng.uniform(-1.0, 1.0, (n, 2)).astype(F)
    for s in (g, r):
        bc.setup_flow(s, mesh, time_scheme=0, scheme=0)
        s.set_penalty(sg, fo, tg)
        s.set_penalty_scale(pc.SCALE)
    a = mesh.arrays()
    whole = _same_force(g, r, centre, None, name)
    assert whole[3] == n and whole[0][0] != 0.0 and whole[1] != 0.0 and whole[2] != 0.0
    pk.check_force(whole, a, g.get_u(), sg, fo, tg, pc.SCALE, centre)
    parts = [_same_force(g, r, centre, box, (name, box)) for box in boxes]
    for box, part in zip(boxes, parts):
        assert 0 < part[3] < n
        pk.check_force(part, a, g.get_u(), sg, fo, tg, pc.SCALE, centre, box)
    assert parts[0][3] + parts[1][3] == n
    _, mag = pk.force64(a, g.get_u(), sg, fo, tg, pc.SCALE, centre)
    total = np.array([parts[0][0][0] + parts[1][0][0], parts[0][0][1] + parts[1][0][1], parts[0][1] + parts[1][1],
                      parts[0][2] + parts[1][2]])
    ref = np.array([whole[0][0], whole[0][1], whole[1], whole[2]])
    assert np.all(np.abs(total - ref) <= 2.0 * pk.force_bound(mag, n)[:4]), (total, ref)
    for s in (g, r):  # sigma and target only: s > 0 on fewer cells
        s.set_penalty(sg, None, tg)
    got = _same_force(g, r, centre, None, name + " without forch")
    assert got[3] == int((sg > 0).sum())
    g.close()


def test_a_solid_stops_the_flow():
    """|x_i| <= (R_i + tol) / (vol_i sigma_i) on the rows of the last solved system: tol is the
    solver's stop tolerance rtol |b|_2 and vol_i sigma_i the field that was set, neither taken
    from the solution or the stored diagonal (penalty_cases.solid_bound; tests/test_penalty.py
    shows a diagonal without the penalty misses it)"""
    cfg = default_config(**pc.SOLID_CFG)
    g = GpuSolver(bc.mesh_of("rect"), config=cfg)
    cells, pen = pc.solid_disc_case(g)
    got, bound = pc.solid_bound(bc.mesh_of("rect"), cells, pen, g.debug_buffer(9), g.debug_buffer(3), g.debug_buffer(4),
                                cfg.fgmres_rtol)
    print("solid disc: max |x| inside", got.max(), "largest bound", bound.max())
    assert np.all(got <= bound)
    # the state is the solution of that system: alpha_u = 1, so u = uo + (x - uo), which rounds
    # twice, each within eps32 / 2 of a magnitude below |uo| + |x| <= 2 max |u|
    u = np.abs(np.asarray(g.get_u()).reshape(-1, 2))
    assert np.all(u[cells] <= bound + 2.0 * pk.EPS32 * u.max())
    g.close()


def test_darcy_plug():
    """bit identity with the restatement, whose deviation tests/test_penalty.py measured
    (penalty_cases.DARCY_MEASURED), and the same assertions: steady, within twice that figure"""
    g, r = _gpu("rect"), _ref("rect")
    du = [pc.darcy_case(s) for s in (g, r)]
    _same_bits(g, r, "Darcy plug")
    dev = pc.darcy_deviation(g)
    print("Darcy plug: |dp / (sigma U L) - 1| =", dev, "last step's max |du|", du)
    assert du[0] <= pc.STEADY
    assert pc.DARCY_MEASURED < 0.25 and dev <= 2.0 * pc.DARCY_MEASURED
    g.close()


def test_refusals():
    name = "rect"
    mesh = bc.mesh_of(name)
    n = mesh.num_cells()
    g = _gpu(name)
    bc.setup_flow(g, mesh)
    with pytest.raises(RuntimeError):
        g.penalty_force()
    assert not g.penalty()["active"]
    sg, fo, tg = pc.field(name)
    g.set_penalty(sg, fo, tg)
    limit = g.penalty()["max_vol_sigma"]
    vol = np.asarray(mesh.arrays()["cell_vol"], np.float64)
    assert np.isfinite(limit) and limit > 0.0
    over = np.r_[sg[:-1], 1.01 * limit / float(F(vol[-1]))]
    bad_sigma = (sg[:-1], np.r_[sg, sg[:1]], np.r_[sg[:-1], -1.0], np.r_[sg[:-1], np.nan], np.r_[np.inf, sg[1:]], over,
                 np.r_[sg[:-1], 3e38])
    for bad in bad_sigma:
        with pytest.raises((RuntimeError, ValueError)):
            g.set_penalty(bad, fo[:len(bad)] if len(bad) <= n else np.r_[fo, fo[:1]],
                          tg[:len(bad)] if len(bad) <= n else np.r_[tg, tg[:1]])
    for bad in (np.r_[fo[:-1], -1.0], np.r_[fo[:-1], np.inf]):
        with pytest.raises(RuntimeError):
            g.set_penalty(sg, bad, tg)
    bad_t = tg.copy()
    bad_t[3, 1] = np.nan
    with pytest.raises(RuntimeError):
        g.set_penalty(sg, fo, bad_t)
    with pytest.raises(RuntimeError):
        g.set_penalty_scale(float("inf"))
    with pytest.raises(RuntimeError):
        g.penalty_force((float("nan"), 0.0))
    got = g.penalty()  # a refused call changes nothing
    assert np.array_equal(_bits(got["sigma"]), _bits(sg)) and np.array_equal(_bits(got["forch"]), _bits(fo))
    assert np.array_equal(_bits(got["target"]), _bits(tg))
    g.set_penalty(np.r_[sg[:-1], 0.99 * limit / float(F(vol[-1]))])  # just under the limit: taken
    g.set_penalty(sg, fo, tg)
    for flags in (1, 2):  # the in-place smoother, the racy prepare: no form with a penalty
        with pytest.raises(RuntimeError):
            g.debug_reference_semantics(flags)
    g.clear_penalty()
    for flags in (1, 2):
        g.debug_reference_semantics(flags)
        with pytest.raises(RuntimeError):
            g.set_penalty(sg)
        with pytest.raises(RuntimeError):
            g.penalty_force()
    g.debug_reference_semantics(0)
    g.set_penalty(sg)
    g.close()


def test_distributed_handle_refuses():
    mesh = bc.mesh_of("obstacle")
    grp = GpuGroup(mesh, 2, config=default_config(**bc.FIXED))
    for h in grp.ranks:
        with pytest.raises(RuntimeError):
            h.set_penalty(np.full(h.num_cells, 10.0))
        with pytest.raises(RuntimeError):
            h.set_penalty(np.full(mesh.num_cells(), 10.0))
        with pytest.raises(RuntimeError):
            h.set_penalty_scale(0.5)
        with pytest.raises(RuntimeError):
            h.penalty_force()
        assert not h.penalty()["active"]  # a read: answered, nothing is set
    grp.close()


def test_resume(tmp_path):
    """save_state, a fresh handle, load_state, the field and the scale set again: the
    uninterrupted run's bits"""
    name = "voronoi"
    mesh = bc.mesh_of(name)
    a = _gpu(name)
    bc.setup_flow(a, mesh, time_scheme=1, scheme=1)
    pc.set_field(a, name)
    a.step()
    a.step()
    path = str(tmp_path / "penalty.state")
    a.save_state(path)
    b = _gpu(name)
    b.load_state(path)
    assert not b.penalty()["active"] and b.penalty()["target_scale"] == 1.0  # a checkpoint stores none of it
    pc.set_field(b, name)
    for k in range(2):
        a.step()
        b.step()
        _same_bits(a, b, f"resumed step {k}")
    a.close()
    b.close()


def test_a_rotating_disc_delivers_power():
    """physics sign: a disc turning in a fluid at rest drags it along: the torque of the
    fluid on it opposes the rotation, and the fluid's force does negative work on it"""
    mesh = bc.mesh_of("rect")
    g = _gpu("rect", fixed_outer=3, fixed_inner=20)
    pc.setup_channel(g, mesh, 0.01)
    c = g.constants
    c.inlet_velocity = 0.0
    g.constants = c
    g.set_penalty(**builders.solid_disc(mesh, (0.5, 0.375), 0.2, 1e-3, 1.0, 0.01, omega=2.0))
    g.step()
    f = g.penalty_force((0.5, 0.375))
    print("rotating disc:", f)
    assert f.cells == 12 and f.power < 0.0 and f.torque < 0.0
    g.close()
