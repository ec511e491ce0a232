"""Tracer particles on the GPU: positions, cells, status, ages and every
statistic bit for bit against the numpy restatement (tests/particles_ref.py),
the float64 checks (tests/particles_checks.py) on the device's own result, the
stamped frame, the refusals, and that particles leave the solver's state alone."""
import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver
from tests import particles_cases as PC
from tests import particles_checks as K
from tests import particles_ref as R
from tests import render_ref as RR
from tests.test_particles import check_case

pytestmark = pytest.mark.gpu

F = np.float32


def _same(p, P):
    for name in ("x", "y", "age", "cell", "status"):
        a, b = getattr(p, name), getattr(P, name)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name


def _run(s, mesh, u, seeds, dt, steps, hop_cap=64):
    s.set_u(u)
    s.set_particle_mesh(mesh)
    s.enable_particles(len(seeds), hop_cap=hop_cap)
    assert s.particle_stats()["empty"] == len(seeds)
    s.seed_particles(seeds)
    for _ in range(steps):
        s.advance_particles(dt)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_matches_restatement_and_passes_the_checks(name):
    c = PC.CASES[name]
    mesh = PC.mesh_of(c["mesh"])
    seeds = PC.seeds_of(name)
    s = GpuSolver(mesh)
    _run(s, mesh, PC.field(mesh, c["field"]), seeds, c["dt"], c.get("steps", 1), c.get("hop_cap", 64))
    p, st = s.particles(), s.particle_stats()
    P, hops, capped = PC.reference(name)
    _same(p, P)
    assert st == P.stats()  # the statistics of the last advance, and the contacts since the seeding
    # the float64 checks on the device's own result (hops, contacts and capped per particle are the restatement's,
    # which the statistics above tie to the device's)
    dev = R.Set(P.n, P.hop_cap)
    dev.x, dev.y, dev.cell, dev.status, dev.age = p.x, p.y, p.cell, p.status, p.age
    dev.contacts, dev.hops, dev.capped = P.contacts, P.hops, P.capped
    check_case(name, dev, hops, capped)
    s.close()


def test_solved_flow_with_a_rake():
    """3 steps of the solved flow past the obstacle, a rake upstream re-seeded
    into a ring of slots every step (a streakline), against the restatement fed
    with the handle's own velocities"""
    mesh, pm = PC.mesh_of("obstacle"), PC.pmesh_of("obstacle")
    s = GpuSolver(mesh)
    s.set_dt(PC.RAKE_DT)
    s.set_viscosity(0.001)
    s.set_inlet_velocity(1.0)
    s.set_precond_type(1)
    s.initialize_history()
    rake = PC.RAKE
    s.set_particle_mesh(mesh)
    with pytest.raises(RuntimeError, match="there was none"):  # advance before a step
        s.enable_particles(8)
        s.advance_particles()
    s.enable_particles(3 * 65)
    P = R.Set(3 * 65)
    for k in range(3):
        s.step()
        s.seed_particles(rake, first=65 * k)
        P.seed(pm, rake, first=65 * k)
        s.advance_particles()
        R.advance(pm, s.get_u().astype(F), P, F(PC.RAKE_DT))
        _same(s.particles(), P)
        assert s.particle_stats() == P.stats()
    assert P.stats()["alive"] == 3 * 65 and P.stats()["hops_total"] > 0
    X = K.extent(pm.vx64, pm.vy64)
    assert not P.capped.any() and not P.contacts.any()
    p = s.particles()
    r = K.assert_containment(pm.polygon, p.x, p.y, p.cell, p.status, X)  # nobody is exempt; the cap is 1 %
    print("rake containment", r)
    s.close()


def test_seeding_permutation_and_block_tails():
    mesh, pm = PC.mesh_of("obstacle"), PC.pmesh_of("obstacle")
    seeds, outside, shared = PC.special_seeds()
    u = PC.field(mesh, (1.0, 0.25))
    s = GpuSolver(mesh)
    _run(s, mesh, u, seeds, 0.2, 0)
    p = s.particles()
    X = K.extent(pm.vx64, pm.vy64, seeds)
    K.assert_seeding(pm.polygon, pm.N, p.x, p.y, p.cell, p.status, X, outside, shared)
    s.advance_particles(0.2)
    q = s.particles()
    out = np.array(outside)
    K.assert_unmoved([a[out] for a in (p.x, p.y, p.age, p.status)], [a[out] for a in (q.x, q.y, q.age, q.status)])
    # the same positions in a shuffled slot order give the shuffled result, for every block tail
    base = PC.seeds_of("uniform_obstacle")
    for n in (1, 63, 64, 65, 257):
        perm = np.random.default_rng(n).permutation(n)
        res = []
        for xy in (base[:n], base[:n][perm]):
            s.enable_particles(n)
            s.seed_particles(xy)
            s.advance_particles(0.3)
            res.append(s.particles())
        for a, b in zip(*res):
            assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32)), n
    s.close()


def test_render_particles():
    name = "uniform_obstacle"
    c = PC.CASES[name]
    mesh, pm = PC.mesh_of(c["mesh"]), PC.pmesh_of(c["mesh"])
    s = GpuSolver(mesh)
    _run(s, mesh, PC.field(mesh, c["field"]), PC.seeds_of(name), c["dt"], 1)
    P, _, _ = PC.reference(name)
    s.set_render_mesh(mesh)
    with pytest.raises(RuntimeError, match="no view"):
        s.render_particles()
    s.set_view(96, 32)
    with pytest.raises(RuntimeError, match="no frame"):
        s.render_particles()
    frame = s.render("speed", range=(0.0, 2.0))
    box = RR.bounds(pm.vx64, pm.vy64, pm.idx)
    for colour in ((255, 255, 255, 255), (10, 200, 30, 128)):
        img = s.render_particles(colour)
        assert np.array_equal(img, R.stamp(P, frame, RR.View(96, 32, box), colour))
        K.assert_stamp(frame, img, box, P.x, P.y, P.status, colour, K.extent(pm.vx64, pm.vy64))
    assert np.array_equal(s.render("speed", range=(0.0, 2.0)), frame)  # the renderer's frame is untouched
    s.close()


def test_particles_are_read_only():
    mesh = PC.mesh_of("obstacle")

    def run(particles):
        s = GpuSolver(mesh)
        s.set_dt(0.001)
        s.set_viscosity(0.001)
        s.set_inlet_velocity(1.0)
        s.set_precond_type(1)
        s.initialize_history()
        if particles:
            s.set_particle_mesh(mesh)
            s.enable_particles(257)
            s.seed_particles(PC.seeds_of("uniform_obstacle"))
        for _ in range(2):
            s.step()
            if particles:
                s.advance_particles()
                s.particle_stats()
        out = s.get_u().tobytes(), s.get_p().tobytes()
        s.close()
        return out

    assert run(True) == run(False)


def test_refusals():
    mesh = PC.mesh_of("rect")
    s = GpuSolver(mesh)
    with pytest.raises(RuntimeError, match="no mesh"):
        s.enable_particles(4)
    for call in (lambda: s.seed_particles(np.zeros((1, 2))), lambda: s.advance_particles(0.1), s.particles,
                 s.particle_stats):
        with pytest.raises(RuntimeError, match="not enabled"):
            call()
    s.set_particle_mesh(mesh)
    with pytest.raises(RuntimeError, match="capacity"):
        s.enable_particles((1 << 24) + 1)
    with pytest.raises(RuntimeError, match="hop_cap"):
        s.enable_particles(4, hop_cap=-3)
    s.enable_particles(4)
    with pytest.raises(RuntimeError, match="exceeds the capacity"):
        s.seed_particles(np.zeros((3, 2)), first=2)
    with pytest.raises(RuntimeError, match="there was none"):
        s.advance_particles()
    s.enable_particles(0)  # capacity 0, then use
    with pytest.raises(RuntimeError, match="not enabled"):
        s.advance_particles(0.1)
    # malformed meshes: a refused call changes nothing
    s.enable_particles(4)
    t = mesh.topology()
    vx, vy, _ = mesh.vertices()
    args = [vx, vy, t["cell_vertex_offsets"], t["cell_vertices"], t["face_v1"], t["face_v2"]]
    rev = np.array(t["cell_vertices"]).copy()
    o = np.array(t["cell_vertex_offsets"], np.int64)
    rev[o[0]:o[1]] = rev[o[0]:o[1]][::-1]
    with pytest.raises(RuntimeError, match="counter-clockwise"):
        s.set_particle_polygons(vx, vy, args[2], rev, args[4], args[5])
    v1 = np.array(t["face_v1"]).copy()
    f = int(mesh.arrays()["cell_faces"][0])
    v1[f] = t["face_v2"][f]
    with pytest.raises(RuntimeError, match="two different"):
        s.set_particle_polygons(vx, vy, args[2], args[3], v1, args[5])
    s.seed_particles(np.array([[0.5, 0.25]]))  # the set and the mesh are still there
    assert s.particle_stats()["alive"] == 1
    s.set_particle_mesh(None)
    with pytest.raises(RuntimeError, match="not enabled"):
        s.particles()
    s.close()
    big = PC.mesh_of("obstacle")
    g = GpuGroup(big, 2)
    with pytest.raises(RuntimeError, match="one GPU only"):
        g.set_particle_mesh(big)
    with pytest.raises(RuntimeError, match="one GPU only"):
        g.enable_particles(4)
    g.close()
