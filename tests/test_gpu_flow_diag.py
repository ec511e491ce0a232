"""Flow diagnostics on the GPU: the read-only pass (k_flow_diag) against the
oracle-verified k_prepare gradients of a twin solver, the reference's driver
loop (src/ui/app.rs:871-910) and float64 sums in the canonical order; rank
invariance of the distributed solver; the adaptive-dt loop end to end against
the CPU oracle."""
import functools
import math

import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver, adaptive_dt_rule, default_config
from cfd2_amd.mesh import RectangularChannel, generate_cut_cell_mesh, generate_voronoi_mesh
from tests import refpy
from tests.meshes import STEP, backwards_step, bench_mesh, channel_obstacle
from tests.oracle_py import OracleSolver
from tests.test_gpu_parity import _assert_same_info

pytestmark = pytest.mark.gpu

F = np.float32
NONE = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _mesh(name):
    if name == "rect":  # fewer than 64 cells: less than one wavefront
        geo = RectangularChannel(length=1.0, height=0.5)
        return generate_cut_cell_mesh(geo, 0.15, 0.15, 1.2, (1.0, 0.5))
    if name == "obstacle":  # not a multiple of 64 / 256; wall, inlet and outlet
        return channel_obstacle(h=0.1)
    if name == "step":
        return backwards_step()
    if name == "voronoi":  # variable face counts, the widest ELL
        return generate_voronoi_mesh(STEP, 0.12, 0.12, 1.2, (3.5, 1.0), seed=7)
    if name == "units4":  # >= 65,536 cells: the reduction writes units of 4 chunks
        return bench_mesh(0.0066, 0)
    raise KeyError(name)


def _fields(mesh):
    a = mesh.arrays()
    x, y = a["cell_cx"], a["cell_cy"]
    u = np.stack([0.8 + 0.5 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y), 0.3 * np.cos(1.3 * x) * np.sin(2.9 * y + 0.2)], 1)
    p = 1.0 + 0.4 * np.sin(1.9 * x) + 0.7 * y * y
    return u, p


def _set_constants(s, mid_ramp):
    c = s.constants
    c.inlet_velocity = 1.3
    c.viscosity = 0.01
    if mid_ramp:  # time < ramp_time: smoothstep strictly between 0 and 1
        c.ramp_time = 0.1
        c.time = 0.04
    else:         # ramp_time = 0 (time > 0: the ramp is 1 in every restatement)
        c.ramp_time = 0.0
        c.time = 0.01
    s.constants = c


def _twin_gradients(mesh, u, mid_ramp):
    """the existing k_prepare on a twin solver with the same state and constants"""
    t = GpuSolver(mesh)
    _set_constants(t, mid_ramp)
    t.set_u(u)
    t.debug_prepare_assemble(False)
    gu = t.debug_buffer(1).reshape(-1, 2)
    gv = t.debug_buffer(2).reshape(-1, 2)
    t.close()
    return gu, gv


def _ref_max_speed(u):
    """app.rs:889-895; numpy's elementwise f64 x*x + y*y and sqrt are the loop's operations"""
    v = np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])
    v = v[~np.isnan(v)]
    return float(v.max()) if len(v) and v.max() > 0.0 else 0.0


def _check_gradients(mesh, mid_ramp, with_refpy):
    u, _ = _fields(mesh)
    s = GpuSolver(mesh)
    _set_constants(s, mid_ramp)
    s.set_u(u)
    vort, div = s.vorticity(), s.divergence()
    gu, gv = _twin_gradients(mesh, u, mid_ramp)
    assert np.array_equal(vort.astype(F), gv[:, 0] - gu[:, 1])
    assert np.array_equal(div.astype(F), gu[:, 0] + gv[:, 1])
    assert np.array_equal(vort.astype(F).astype(np.float64), vort)  # widened f32
    if with_refpy:
        M = refpy.RefMesh(mesh)
        st = refpy.State(M.N)
        st.u = np.asarray(u, np.float64).astype(F)
        c = refpy.Constants()
        k = s.constants
        c.inlet_velocity, c.ramp_time, c.time = F(k.inlet_velocity), F(k.ramp_time), F(k.time)
        _, ru, rv = refpy.prepare(M, st, None, c)
        assert np.array_equal(vort.astype(F), rv[:, 0] - ru[:, 1])
        assert np.array_equal(div.astype(F), ru[:, 0] + rv[:, 1])
    return s, vort, div


def _check_max_and_sums(mesh, s, vort, div):
    d = s.flow_diagnostics()
    u = s.get_u()
    assert d.max_speed == _ref_max_speed(u)
    assert d.max_vorticity == float(np.abs(vort).max())
    assert d.max_divergence == float(np.abs(div).max())
    vol = mesh.arrays()["cell_vol"].astype(F).astype(np.float64)
    sq = u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]
    assert d.kinetic_energy == float(refpy.canon_sum(0.5 * vol * sq))
    assert d.enstrophy == float(refpy.canon_sum(0.5 * vol * vort * vort))
    assert tuple(d.force_pressure) == (0.0, 0.0) and tuple(d.force_viscous) == (0.0, 0.0)  # no region set
    assert d.region_faces == 0
    assert s.min_cell_size == float(np.min(np.sqrt(mesh.arrays()["cell_vol"])))


@pytest.mark.parametrize("mid_ramp", [False, True])
@pytest.mark.parametrize("name", ["rect", "obstacle", "step", "voronoi"])
def test_gradients_maxima_sums(name, mid_ramp):
    """checks 1-3: vorticity / divergence == the twin's k_prepare gradients and
    tests.refpy.prepare, bit for bit; max_speed == the reference's loop; the
    f64 sums == canon_sum of the numpy terms."""
    mesh = _mesh(name)
    if name == "rect":
        assert mesh.num_cells() < 64
    s, vort, div = _check_gradients(mesh, mid_ramp, with_refpy=name != "step")
    _check_max_and_sums(mesh, s, vort, div)
    s.close()


def test_units_of_four_chunks():
    """check 6: >= 65,536 cells, so the chunk kernels write units of 4 chunks"""
    mesh = _mesh("units4")
    n = mesh.num_cells()
    assert n >= 65536 and refpy._geom(n)[0] >= 4  # G >= 4, hence red_geom(N).U == 4
    s, vort, div = _check_gradients(mesh, True, with_refpy=False)
    _check_max_and_sums(mesh, s, vort, div)
    s.close()


def test_maximum_ignores_nan_and_zero_field_keeps_dt():
    mesh = _mesh("obstacle")
    u, _ = _fields(mesh)
    s = GpuSolver(mesh)
    un = u.copy()
    k = int(np.argmax(u[:, 0] ** 2 + u[:, 1] ** 2))
    un[k, 0] = np.nan  # the cell that held the maximum
    s.set_u(un)
    d = s.flow_diagnostics()
    assert d.max_speed == _ref_max_speed(s.get_u()) and math.isfinite(d.max_speed) and d.max_speed > 0.0
    s.set_u(np.zeros_like(u))
    assert s.flow_diagnostics().max_speed == 0.0
    s.set_dt(2.5e-4)
    before = s.constants
    assert s.adapt_dt(0.9) == before.dt
    after = s.constants
    assert (after.dt, after.dt_old) == (before.dt, before.dt_old)
    s.close()


def _region_terms(mesh, s, box):
    """numpy restatement of the wall-force terms on the selected faces"""
    a = mesh.arrays()
    wall = (a["face_neighbor"] == NONE) & (a["face_boundary"] == 3)
    x0, y0, x1, y1 = box
    sel = wall & (a["face_cx"] >= x0) & (a["face_cx"] <= x1) & (a["face_cy"] >= y0) & (a["face_cy"] <= y1)
    f = np.nonzero(sel)[0]
    own = a["face_owner"][f].astype(np.int64)
    area = a["face_area"][f].astype(F)
    nx, ny = a["face_nx"][f].astype(F), a["face_ny"][f].astype(F)  # boundary faces: out of their owner
    dvx = a["face_cx"][f].astype(F) - a["cell_cx"][own].astype(F)
    dvy = a["face_cy"][f].astype(F) - a["cell_cy"][own].astype(F)
    dist = np.sqrt(dvx * dvx + dvy * dvy).astype(np.float64)
    u, p = s.get_u()[own], s.get_p()[own]
    visc = float(s.constants.viscosity)
    A, nx, ny = area.astype(np.float64), nx.astype(np.float64), ny.astype(np.float64)
    return int(wall.sum()), len(f), dict(fpx=p * nx * A, fpy=p * ny * A, fvx=visc * u[:, 0] * A / dist,
                                        fvy=visc * u[:, 1] * A / dist, area=A)


def test_wall_force_region():
    """check 4: region count, closed surface under uniform pressure, and the
    smooth-field forces against math.fsum of the numpy terms."""
    mesh = _mesh("obstacle")
    u, p = _fields(mesh)
    box = (0.7, 0.2, 1.3, 0.8)  # around the obstacle (centre (1, 0.5), r 0.2), clear of the channel walls
    s = GpuSolver(mesh)
    _set_constants(s, False)
    n = mesh.num_cells()
    s.set_p(np.ones(n))
    nwall, nsel, t = _region_terms(mesh, s, box)
    assert s.set_force_region(*box) == nsel and 0 < nsel < nwall
    d = s.flow_diagnostics()
    assert d.region_faces == nsel
    bound = 8 * 2.0 ** -24 * float(np.sum(t["area"]))  # p = 1: sum |p n A| = sum A
    assert abs(d.force_pressure[0]) <= bound and abs(d.force_pressure[1]) <= bound
    assert tuple(d.force_viscous) == (0.0, 0.0)  # u = 0
    tol = (math.log2(n) + 8) * 2.0 ** -53
    for setter, field in ((s.set_p, p), (s.set_u, u)):
        setter(field)
        _, _, t = _region_terms(mesh, s, box)
        d = s.flow_diagnostics()
        got = dict(fpx=d.force_pressure[0], fpy=d.force_pressure[1], fvx=d.force_viscous[0], fvy=d.force_viscous[1])
        for key, val in got.items():
            assert abs(val - math.fsum(t[key])) <= tol * float(np.sum(np.abs(t[key]))), key
        moved = ("fpx", "fpy") if setter == s.set_p else ("fvx", "fvy")
        assert all(got[key] != 0.0 for key in moved)
    assert s.set_force_region(1.0, 0.0, 0.0, 1.0) == 0  # x1 < x0: none
    d = s.flow_diagnostics()
    assert tuple(d.force_pressure) == (0.0, 0.0) and tuple(d.force_viscous) == (0.0, 0.0) and d.region_faces == 0
    s.close()


def _physics(s, dt=1e-3):
    s.set_dt(dt)
    s.set_viscosity(0.01)
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)


def test_diagnostics_are_read_only():
    """check 5: a solver that calls every new getter between steps keeps the bits of one that does not"""
    mesh = _mesh("obstacle")
    cfg = dict(fixed_outer=2, fixed_inner=5)
    a, b = GpuSolver(mesh, config=default_config(**cfg)), GpuSolver(mesh, config=default_config(**cfg))
    for s in (a, b):
        _physics(s)
        s.initialize_history()
    for k in range(3):
        a.step()
        b.step()
        b.set_force_region(0.7, 0.2, 1.3, 0.8)
        b.flow_diagnostics()
        b.speed(), b.vorticity(), b.divergence()
        assert b.min_cell_size > 0.0
        for g in ("get_u", "get_p", "get_d_p"):
            assert np.array_equal(getattr(a, g)(), getattr(b, g)()), (g, k)
        _assert_same_info(a, b, f"step {k}")  # every step_info field but the wall-clock solve time
    a.close()
    b.close()


@pytest.mark.parametrize("nranks", [2, 3])
def test_rank_invariance(nranks, tmp_path):
    """check 7: every rank's cfd_flow_diag and the gathered fields == one GPU's,
    after set_u, after 2 steps and after load_state."""
    mesh = channel_obstacle(h=0.05)
    u, _ = _fields(mesh)
    cfg = dict(fixed_outer=2, fixed_inner=5)
    g = GpuGroup(mesh, nranks, config=default_config(**cfg))
    one = GpuSolver(mesh, config=default_config(**cfg))
    box = (0.7, 0.2, 1.3, 0.8)

    def same(ctx):
        assert bytes(g.flow_diagnostics()) == bytes(one.flow_diagnostics()), ctx  # the group call checks rank == rank
        assert np.array_equal(g.vorticity(), one.vorticity()), ctx
        assert np.array_equal(g.divergence(), one.divergence()), ctx
        assert np.array_equal(g.speed(), one.speed()), ctx

    for s in (g, one):
        _physics(s)
        _set_constants(s, True)
        s.set_u(u)
        assert s.set_force_region(*box) > 0
    same("after set_u")
    for s in (g, one):
        s.initialize_history()
        s.step()
        s.step()
    same("after 2 steps")
    assert one.flow_diagnostics().force_pressure[0] != 0.0
    path = str(tmp_path / "one.state")
    one.save_state(path)
    one.step()
    g2 = GpuGroup(mesh, nranks, config=default_config(**cfg))
    g2.set_force_region(*box)
    g2.load_state(path)
    one.load_state(path)
    g.close()
    g = g2
    same("after load_state")
    g.close()
    one.close()


def test_reference_adaptive_loop_end_to_end():
    """check 8: 8 x step_adaptive == OracleSolver.step() + the reference's rule
    on the oracle's get_u(); target_cfl = 0.01 makes the oracle take the 1.2x
    cap on some steps and the CFL-limited branch on others (found on the CPU)."""
    mesh = _mesh("obstacle")
    cfg = dict(fixed_outer=2, fixed_inner=5)
    target_cfl = 0.01
    hmin = float(np.min(np.sqrt(mesh.arrays()["cell_vol"])))

    def setup(s):
        _physics(s, dt=1e-4)
        s.set_ramp_time(0.0)
        s.set_inlet_velocity(1.3)
        s.initialize_history()

    o = OracleSolver(mesh, config=default_config(**cfg))
    setup(o)
    dts, branches = [], set()
    for _ in range(8):
        o.step()
        uo = np.asarray(o.get_u()).reshape(-1, 2)
        vmax = 0.0
        for vx, vy in uo:  # app.rs:889-895
            v = math.sqrt(vx * vx + vy * vy)
            if v > vmax:
                vmax = v
        cur = float(o.constants.dt)
        nxt, changed = adaptive_dt_rule(cur, target_cfl, hmin, vmax)
        if changed:
            branches.add("cap" if target_cfl * hmin / vmax > cur * 1.2 else "cfl")
            o.set_dt(np.float32(nxt))
        dts.append(F(o.constants.dt))
    assert {"cap", "cfl"} <= branches
    uo, po = np.asarray(o.get_u()).reshape(-1, 2), np.asarray(o.get_p())
    for make in (lambda: GpuSolver(mesh, config=default_config(**cfg)),
                 lambda: GpuGroup(mesh, 2, config=default_config(**cfg))):
        s = make()
        setup(s)
        assert s.min_cell_size == hmin
        got = [F(s.step_adaptive(target_cfl)) for _ in range(8)]
        assert [x.tobytes() for x in got] == [x.tobytes() for x in dts]
        assert np.array_equal(s.get_u(), uo) and np.array_equal(s.get_p(), po)
        s.close()


def test_group_needing_restore_refuses_diagnostics():
    """like cfd_group_step: a group whose step failed midway answers CFD_ERR_INVALID
    until it is restored or reset; the read-only calls themselves never set the mark"""
    mesh = _mesh("obstacle")
    g = GpuGroup(mesh, 2, config=default_config(fixed_outer=2, fixed_inner=5))
    _physics(g)
    g.initialize_history()
    g.flow_diagnostics()
    g.adapt_dt(0.9)
    assert not g.needs_restore
    with pytest.raises(RuntimeError):
        g.debug_fault_midstep(1)
    assert g.needs_restore
    for call in (g.flow_diagnostics, lambda: g.adapt_dt(0.9)):
        with pytest.raises(RuntimeError, match="status 1.*needs restore"):
            call()
    g.reset()
    g.flow_diagnostics()
    g.close()
