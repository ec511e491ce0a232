"""Tracer particles on the CPU: the float64 checks (tests/particles_checks.py)
pass on the numpy restatement (tests/particles_ref.py) for every case, and each
check catches a deliberately wrong convention built into a copy of the rules."""
import numpy as np
import pytest

from tests import particles_cases as PC
from tests import particles_checks as K
from tests import particles_ref as R
from tests import render_ref as RR

F = np.float32


def check_case(name, P, hops, capped, seeds=None):
    """every float64 check that applies to the case, on a result (P, hops, capped)"""
    c = PC.case_of(name)
    pm = PC.pmesh_of(c["mesh"])
    seeds = PC.seeds_of(name) if seeds is None else seeds
    X = PC.extent_of(name, P)
    dt = float(F(c["dt"])) * c.get("steps", 1)
    st = P.stats() if hasattr(P, "stats") else None
    if st is not None:
        assert sum(st[k] for k in R.STATUS) == st["capacity"] == len(seeds)
    kind = c["kind"]
    # on an edge by construction, and so not undecided: a particle that stopped at the hop cap (the cap case alone),
    # and one that met a wall and lies on a wall edge of its cell now; one that has left the wall counts
    r = K.assert_containment(pm.polygon, P.x, P.y, P.cell, P.status, X, capped=capped if kind == "cap" else None,
                             contacts=P.contacts, on_wall=PC.on_wall_of(c["mesh"]))
    print(name, "containment", r)
    if kind == "uniform":
        K.assert_uniform(seeds, c["field"], dt, P.x, P.y, P.status, P.contacts, hops, capped, X)
    elif kind in ("outlet", "inlet"):
        want = R.EXITED_OUTLET if kind == "outlet" else R.EXITED_INLET
        counts = np.bincount(np.asarray(P.status, np.int64), minlength=5)
        K.assert_exit(seeds, c["field"][0], c["line"], want, P.x, P.status, P.age, hops, counts, len(seeds), X)
    elif kind == "wall":
        K.assert_wall(seeds, c["field"], dt, c["line"], P.x, P.y, P.status, P.contacts, hops, X)
    elif kind == "cap":
        assert np.any(capped) and np.all(hops[capped] == c["hop_cap"])
    elif kind == "split":
        worst = K.assert_path(PC.paths_of(name), P.x, P.y, P.status, P.contacts)
        print(name, "path: error / bound at most", worst)


@pytest.mark.parametrize("name", sorted(PC.CASES))
def test_checks_pass_on_the_restatement(name):
    P, hops, capped = PC.reference(name)
    check_case(name, P, hops, capped)
    if PC.case_of(name)["kind"] != "cap":
        assert not capped.any()  # a condition on the cases, checked here


@pytest.mark.parametrize("name", ["shear_voronoi", "solid_voronoi", "uniform_graded"])
def test_split_steps_agree(name):
    c = PC.CASES[name]
    P1, h1, _ = PC.reference(name)
    P2, h2, _ = PC.run(name, dt_parts=2)
    assert np.array_equal(P1.status, P2.status)
    if c["kind"] == "split":  # the bound of each run against the float64 path, from the normal speed of every crossing
        _, b1, why = PC.paths_of(name)
        _, b2, _ = PC.paths_of(name, advances=2 * c["steps"])
        keep = np.array([w is None for w in why])
        assert (~keep).sum() <= 0.01 * len(keep)
    else:  # a uniform field: both end at start + v dt within (hops + 1) eps_hop; the particles that met no wall
        eh = K.eps_hop_of(PC.extent_of(name, P1))
        b1, b2, keep = (h1 + 1.0) * eh, (h2 + 2.0) * eh, (P1.contacts == 0) & (P2.contacts == 0)
    K.assert_split((P1.x, P1.y), (P2.x, P2.y), b1, b2, keep)


def test_rake_stays_off_the_edges():
    """the streakline of the solved-flow test (tests/test_gpu_particles.py) in the inlet's own uniform flow, which the
    solved one is close to upstream of the obstacle: three rings of the rake, the undecided share under 1 %"""
    mesh, pm = PC.mesh_of("obstacle"), PC.pmesh_of("obstacle")
    u = PC.field(mesh, (1.0, 0.0)).astype(F)
    P = R.Set(3 * 65)
    for k in range(3):
        P.seed(pm, PC.RAKE, first=65 * k)
        R.advance(pm, u, P, F(PC.RAKE_DT))
    r = K.assert_containment(pm.polygon, P.x, P.y, P.cell, P.status, K.extent(pm.vx64, pm.vy64))
    assert r["alive"] == 3 * 65 and r["undecided"] == 0, r


def test_permutation_is_bitwise():
    name = "uniform_obstacle"
    seeds = PC.seeds_of(name)
    perm = np.random.default_rng(5).permutation(len(seeds))
    P, hops, _ = PC.reference(name)
    Q, hq, _ = PC.run(name, seeds=seeds[perm])
    for a, b in ((P.x, Q.x), (P.y, Q.y), (P.age, Q.age), (P.cell, Q.cell), (P.status, Q.status)):
        assert np.array_equal(a[perm].view(np.uint32), b.view(np.uint32))
    assert np.array_equal(hops[perm], hq)


def test_seeding():
    seeds, outside, shared = PC.special_seeds()
    assert len(shared) >= 4
    pm = PC.pmesh_of("obstacle")
    P = R.Set(len(seeds))
    P.seed(pm, seeds)
    X = K.extent(pm.vx64, pm.vy64, seeds)
    K.assert_seeding(pm.polygon, pm.N, P.x, P.y, P.cell, P.status, X, outside, shared)
    before = [a.copy() for a in (P.x, P.y, P.age, P.status)]
    u = PC.field(PC.mesh_of("obstacle"), (1.0, 0.25)).astype(F)
    R.advance(pm, u, P, 0.2)
    out = np.array(outside)
    K.assert_unmoved([b[out] for b in before], [a[out] for a in (P.x, P.y, P.age, P.status)])
    # the smallest-index owner is caught
    Q = R.Set(len(seeds))
    Q.seed(pm, seeds, owner="smallest")
    with pytest.raises(AssertionError):
        K.assert_seeding(pm.polygon, pm.N, Q.x, Q.y, Q.cell, Q.status, X, outside, shared)


def test_wrong_conventions_are_caught():
    # half-plane exits instead of segments, on the mesh whose hanging node makes a reflex cell: a particle of A is
    # beyond the line of A's face to B while still in A, is handed to B, which does not hold it, and goes round
    with pytest.raises(AssertionError):
        check_case("uniform_reflex", *PC.run("uniform_reflex", exits="halfplane"))
    # an age that forgets the partial step before an exit
    with pytest.raises(AssertionError):
        check_case("exit_outlet", *PC.run("exit_outlet", age_partial=False))
    # a wall that stops instead of sliding
    with pytest.raises(AssertionError):
        check_case("wall", *PC.run("wall", wall="stop"))


def test_half_planes_fail_where_segments_do_not():
    """what the half-plane rule does on the reflex cell, figure by figure: the segment rule carries every particle
    to start + v dt, in A, B or C (check_case above); under half-planes a particle whose target lies in A beyond the
    line of one of A's two inner faces is handed to a cell that does not hold it, goes round B, C and A with t = 0
    and stops at the hop cap on that line, short of its target.  The result differs in the positions, the ages and
    the statistics, so the device, which has to equal the segment run bit for bit on this case
    (tests/test_gpu_particles.py), cannot pass it with half-plane exits: the case pins the segment test there.
    No other case does: on the generated meshes, whose cells are all convex, the two rules give the same bits."""
    name = "uniform_reflex"
    pm = PC.pmesh_of("reflex")
    A = [c for c in range(pm.N) if pm.off[c + 1] - pm.off[c] == 6]
    assert len(A) == 1
    P, hops, capped = PC.reference(name)
    assert not capped.any() and hops.max() <= 2 and len(set(P.cell.tolist())) == 3 and A[0] in P.cell
    Q, hq, cq = PC.run(name, exits="halfplane")
    target = PC.seeds_of(name)[:, 0] + 0.25
    assert cq.sum() > len(cq) // 4 and np.all(hq[cq] == 64) and np.all(Q.x[cq] < target[cq] - 1e-3)
    assert np.all(np.abs(Q.x[~cq] - P.x[~cq]) < 1e-6) and np.all(P.cell[cq] == A[0])  # the others arrive
    assert not np.array_equal(Q.x, P.x) and not np.array_equal(Q.age, P.age) and Q.stats() != P.stats()
    for other in ("uniform_graded", "uniform_obstacle", "shear_voronoi"):
        P, _, _ = PC.reference(other)
        Q, _, _ = PC.run(other, exits="halfplane")
        assert np.array_equal(Q.x, P.x) and np.array_equal(Q.y, P.y) and np.array_equal(Q.cell, P.cell), other


def test_the_fallback_is_needed_and_used():
    """segments alone (no half-plane fallback for a path along a face's line): the wall slide of uniform_obstacle
    ends at a wall face's vertex and a particle gets past the obstacle's boundary, which containment catches"""
    name = "uniform_obstacle"
    with pytest.raises(AssertionError):
        check_case(name, *PC.run(name, fallback=False))


def _frame_case():
    name = "uniform_obstacle"
    P, _, _ = PC.reference(name)
    pm = PC.pmesh_of("obstacle")
    box = RR.bounds(pm.vx64, pm.vy64, pm.idx)
    view = RR.View(96, 32, box)
    frame = np.zeros((32, 96, 4), np.uint8)
    frame[..., 2], frame[..., 3] = 200, 255
    return P, pm, box, view, frame


def test_stamp_and_flipped_rows():
    P, pm, box, view, frame = _frame_case()
    X = K.extent(pm.vx64, pm.vy64)
    white = (255, 255, 255, 255)
    img = R.stamp(P, frame, view, white)
    assert img.shape == frame.shape and np.any(img != frame) and frame[..., 0].max() == 0  # a copy
    K.assert_stamp(frame, img, box, P.x, P.y, P.status, white, X)
    with pytest.raises(AssertionError):
        K.assert_stamp(frame, R.stamp(P, frame, view, white, flip_rows=True), box, P.x, P.y, P.status, white, X)


def test_statistics_of_the_restatement():
    P, hops, capped = PC.reference("cap2")
    st = P.stats()
    assert st["capped"] == int(capped.sum()) > 0 and st["hops_max"] == 2
    assert st["hops_total"] == int(hops.sum()) and st["capacity"] == 65
