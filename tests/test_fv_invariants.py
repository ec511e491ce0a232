"""Float64 invariants of the assembled system and of the FGMRES solve
(tests/fv_checks.py) on the CPU oracle, over the case list of
tests/fv_cases.py; and the proof that each check bites
(test_checks_detect_mutations).  tests/test_gpu_fv_invariants.py runs the
same cases on the HIP path."""
import numpy as np
import pytest

from tests import fv_cases as fc
from tests import fv_checks as fv
from tests.oracle_py import OracleSolver


@pytest.mark.parametrize("density", [1.0, 1000.0])
@pytest.mark.parametrize("mesh_name", fc.MESHES)
def test_assembled_system_invariants(mesh_name, density):
    """Schemes 0/1/2 x Euler/BDF2 (r = dt/dt_old = 0.75): momentum
    conservation, geometric closure, face weights, the pressure operator, the
    diagonal inverses, each to 16 eps32 of the row's terms.

    Found by reading oracle.cpp assemble(): SOU and QUICK keep the upwind
    matrix and put their correction `flux (phi_ho - phi_upwind)` into the
    right-hand side (deferred correction), so all three schemes satisfy the
    same row-sum identity; id 7 inverts the diagonal of the SCALAR (rho-scaled)
    pressure matrix, id 8, not A_pp's."""
    fc.run_assembled(OracleSolver, mesh_name, density)


def test_interior_rows_cover_the_case_list():
    """The interior-row identities cover >= 60 % of all cells of the case list
    (the strips have no interior cell, the wheel one): a broken interior mask
    cannot hide a failure."""
    covered, cells = fc.run_coverage(OracleSolver)
    assert covered >= 0.6 * cells


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("mesh_name", fc.MESHES)
def test_solve_true_residual_and_contract(mesh_name, precond):
    """fixed_outer = 1, max_restart {50, 3, 1} x convergence_lag {0, 1}, three
    steps each: the reported residual against |b - A x| in float64, two-sided,
    and what `converged` / the iteration cap (max_restart x max_outer_restarts)
    promise.

    Measured on the oracle over this whole list
    (profiles/r07/f64_residual_deviation.txt).  A solve that reports a
    computed b - A x (cap reached, stagnation exit, fixed schedule, stale
    read) deviates by at most 1.2 %: RESIDUAL_TOL = 4 x that = 4.8 %, purely
    relative.  A solve that ends `converged` below its target reports the
    Givens estimate, which keeps falling after the true residual has reached
    what f32 resolves of b - A x: up to 1444 x the reported value (strip130),
    yet at most 1.22 |eps32 (|b| + |A||x|)|_2.  Those alone get a floor,
    ESTIMATE_FLOOR_EPS = 4 x 1.22 of that unit, on top of the relative bound.

    The contract is the reference's, not the textbook's: relative to |b|, and
    `converged` is also set by three stagnating restarts and by the lag-1
    stale read (fv_checks.check_convergence_contract tells the exits apart
    by the reported value and names the lines).  The form
    rtol |b - A x0| + atol does not hold: 130 of the 324 solves here miss
    it, by up to 277 x (backwards_step, AMG, lag 1, one iteration)."""
    kinds = fc.run_solve(OracleSolver, mesh_name, precond)
    assert sum(kinds.values()) == 18 and "diverged" not in kinds
    assert kinds.get("target", 0) >= 5, kinds  # never vacuous: the target is asserted on real solves


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("mesh_name", fc.MONOTONE_MESHES)
def test_minimal_residual_monotone(mesh_name, precond):
    """fixed_inner = 1..8 from one state, a fresh solver each: the true
    residuals do not grow, r(8) < r(1)/2, the two-sided check at each k."""
    r = fc.run_monotone(OracleSolver, mesh_name, precond)
    assert len(r) == 8 and r[0] > 0.0


# ------------------------------------------------------------------ mutations
@pytest.fixture(scope="module")
def assembled():
    """dt = 0.02 -> 0.015, ten times the case list's.  At the case list's own
    dt = 0.002 the time coefficient vol rho / dt is most of a momentum row's
    magnitude, and 16 eps32 of the row's terms (about 7e-6 there) exceeds 1e-4
    of any face's flux (at most 5e-6): the momentum check of the case list
    cannot see a flux error of 1e-4, only one of about 2e-4 and more.  The
    diagonal is one f32 number that holds the time coefficient, so no
    tolerance below a few eps32 of it would be a rounding bound."""
    return fc.assembled_system(OracleSolver, fc.mesh_of("backwards_step"), 0, 0, 1.0, dt=0.02)


def _entry(mesh, i, j, sub, col):
    """Index into debug buffer 9 of entry (3i + sub, 3j + col)."""
    srow, scol = fv._scalar_csr_fast(mesh)
    nb = scol[srow[i]:srow[i + 1]]
    rank = int(np.nonzero(nb == j)[0][0])
    return 9 * srow[i] + sub * 3 * len(nb) + 3 * rank + col


def _interior_face(mesh, key, both=True):
    """The internal face with the largest key[f] whose owner (both: and
    neighbour) is an interior cell."""
    a = mesh.arrays()
    inner = fv.interior_mask(mesh)
    own, nb = a["face_owner"].astype(np.int64), a["face_neighbor"].astype(np.int64)
    ok = nb != fv.NONE
    ok[ok] = inner[own[ok]] & (inner[nb[ok]] | (not both))
    f = int(np.argmax(np.where(ok, key, -1.0)))
    return f, int(own[f]), int(nb[f])


def test_checks_detect_mutations(assembled):
    """Each mutation of a copy of the oracle's buffers of one backwards_step
    case makes the named check raise (and the unmutated buffers pass)."""
    mesh = assembled.mesh
    fv.check_assembled(assembled)
    f, o, n = _interior_face(mesh, np.abs(assembled.flux))

    m = assembled.copy()  # negate one interior off-diagonal of A_uu
    m.coupled[_entry(mesh, o, n, 0, 0)] *= -1.0
    assert m.coupled[_entry(mesh, o, n, 0, 0)] != 0.0
    with pytest.raises(AssertionError, match="momentum conservation A_uu"):
        fv.check_momentum(m)

    m = assembled.copy()  # one face's flux scaled by 1 + 1e-4 (the face of largest |flux|)
    m.flux[f] *= 1.0 + 1e-4
    with pytest.raises(AssertionError, match="momentum conservation"):
        fv.check_momentum(m)

    m = assembled.copy()  # scalar matrix scaled by 1.001
    m.scalar *= 1.001
    with pytest.raises(AssertionError, match="scalar matrix != rho \\* A_pp"):
        fv.check_pressure(m)


def test_checks_detect_swapped_face_weights():
    """The two weights of one internal face swapped in A_up (row o, face to
    n): the off-diagonal (1 - w) A nx becomes w A nx and the diagonal takes the
    difference, so the row sum stays and no single-row check sees it; the
    A_pu == A_up check fires, and so does the face-weight check across the
    two rows of the face.  On channel_obstacle, at the face next to a cut cell
    whose weights differ most: every cell of backwards_step is the same
    square, both weights of every face are 1/2 and the swap changes nothing."""
    mesh = fc.mesh_of("channel_obstacle")
    base = fc.assembled_system(OracleSolver, mesh, 0, 0, 1.0)
    fv.check_assembled(base)
    a = mesh.arrays()
    own, nb = a["face_owner"].astype(np.int64), a["face_neighbor"].astype(np.int64)
    an = (a["face_area"] * a["face_nx"]).astype(np.float64)
    G = base.block("u", "p")
    inner_faces = np.nonzero(nb != fv.NONE)[0]
    off = np.zeros(len(an))
    off[inner_faces] = np.asarray(G[own[inner_faces], nb[inner_faces]]).ravel()
    f, o, n = _interior_face(mesh, np.abs(2.0 * off - an), both=False)
    m = base.copy()
    e_off, e_diag = _entry(mesh, o, n, 0, 2), _entry(mesh, o, o, 0, 2)
    new_off = an[f] - m.coupled[e_off]
    m.coupled[e_diag] += m.coupled[e_off] - new_off
    m.coupled[e_off] = new_off
    assert abs(new_off - base.coupled[e_off]) > 1e-3 * abs(an[f])
    fv.check_momentum(m)
    for comp in "uv":  # the row sums of the gradient blocks still close
        Gm = m.block(comp, "p")
        fv._assert_rows(fv._rowsum(Gm), fv._abs_rowsum(Gm), fv.interior_mask(mesh), "row sums")
    with pytest.raises(AssertionError, match="A_pu == A_up"):
        fv.check_closure(m)
    with pytest.raises(AssertionError, match="face weights A_up"):
        fv.check_face_weights(m)


def test_residual_check_detects_mutations():
    """x scaled by 1 + 1e-3, and the reported residual at 0.9 x and 1.1 x:
    the two-sided check raises each time, on solves of the case list itself
    (backwards_step, Jacobi, max_restart 3, lag 0): step 0 reaches the cap
    after 19 restarts and reports a computed b - A x; steps that converge on an
    estimate are skipped."""
    mesh = fc.mesh_of("backwards_step")
    seen = 0
    for sysm, _, stats, cfg in fc.solve_steps(OracleSolver, mesh, 0, 3, 0):
        if fv.reports_estimate(sysm, stats, cfg):
            continue
        seen += 1
        assert stats.iterations > 3
        fv.check_solve(sysm, stats, cfg, fc.RESIDUAL_TOL, fc.ESTIMATE_FLOOR_EPS)
        m = sysm.copy()
        m.x *= 1.0 + 1e-3
        with pytest.raises(AssertionError, match="true residual"):
            fv.check_solve(m, stats, cfg, fc.RESIDUAL_TOL, fc.ESTIMATE_FLOOR_EPS)
        for factor in (0.9, 1.1):
            with pytest.raises(AssertionError, match="true residual"):
                fv.check_residual(sysm, factor * stats.residual, fc.RESIDUAL_TOL)
    assert seen >= 1
