"""Float64 checks of the AMG hierarchy and V-cycle (tests/amg_checks.py) on the
CPU oracle, over the case list of tests/amg_cases.py, and the proof that each
check can fail: deliberate errors applied to copies of the read-back and to the
f64 cycle.  tests/test_gpu_amg_f64.py runs the same drivers on the HIP path."""
import functools

import numpy as np
import pytest

from tests import amg_cases as ac
from tests import amg_checks as amg
from tests import fv_cases
from tests.oracle_py import OracleSolver

EPS32 = amg.EPS32
MULTI_LEVEL = ["strip130", "backwards_step", "graded", "voronoi"]


@functools.lru_cache(maxsize=None)
def _levels(name, density=1.0):
    mesh = fv_cases.mesh_of(name)
    s = ac.built_solver(OracleSolver, mesh, density)
    levels = amg.read_hierarchy(s)
    return levels, s.amg_levels(), s.debug_buffer(8), mesh


def _check(levels, reported, scalar, mesh):
    return amg.check_hierarchy(levels, reported, ac._scalar_csr_fast(mesh), scalar)


def _copy(levels):
    return [L.copy() for L in levels]


@pytest.mark.parametrize("density", ac.DENSITIES)
@pytest.mark.parametrize("name", list(ac.MESHES))
def test_hierarchy_and_vcycle_f64(name, density):
    """Every hierarchy check and every V-cycle check on the oracle; none
    vacuous (the drivers assert the counts against the levels' sizes; the f64
    cycle itself contracts in the energy norm on every case)."""
    levels, counts, rows = ac.run_case(OracleSolver, name, density)
    assert counts["source"] > 0 and counts["consequences"] > 0 and counts["stop"] == len(levels)
    if len(levels) > 1:
        assert counts["partition"] > 0 and counts["galerkin"] > 0
    assert rows == 4 * levels[0].n


def test_wide_columns_mesh_f64():
    """The renumbered 38 k-cell mesh of the 32-bit column tests, on the oracle."""
    levels, counts, rows = ac.run_wide_columns(OracleSolver)
    assert len(levels) >= 4 and counts["galerkin"] > 0 and rows == 4 * levels[0].n


def test_bound_k_is_four_times_the_measured_figure():
    """K quotes profiles/r07/f64_vcycle_deviation.txt."""
    import os
    import re
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r07",
                        "f64_vcycle_deviation.txt")
    m = re.search(r"^worst = (\S+): K = 4 x = (\S+)$", open(path).read(), flags=re.M)
    assert m and float(m.group(1)) == ac.VCYCLE_WORST_MEASURED and ac.K == 4.0 * ac.VCYCLE_WORST_MEASURED


# ------------------------------------------------ the checks must be able to fail
def _expect(check, levels, rest):
    with pytest.raises(AssertionError, match="^" + check + ":"):
        _check(levels, *rest)


def test_hierarchy_checks_detect_mutations():
    """Each deliberate error trips the check named for it and no earlier one
    (check_hierarchy runs source, partition, galerkin, consequences, stop rule
    in that order and the first failure names its check)."""
    levels, *rest = _levels("backwards_step")
    _check(levels, *rest)  # the unmutated read-back passes
    last = len(levels) - 1
    C = levels[last]
    r, c = C.rows_of_entries(), C.col.astype(np.int64)
    _, Kc, _ = amg.galerkin_terms(levels[last - 1])

    # one coarse entry scaled by 1 + 64 eps32 (an off-diagonal of fewer than 64 terms)
    offd = np.nonzero((r != c) & (Kc.data < 64) & (C.val != 0))[0]
    k = int(offd[np.argmin(Kc.data[offd])])
    m = _copy(levels)
    m[last].val[k] = np.float32(np.float64(C.val[k]) * (1.0 + 64.0 * EPS32))
    assert m[last].val[k] != C.val[k]
    _expect("galerkin", m, rest)

    # one coarse entry moved to a neighbouring column (free, not the diagonal, columns still ascending)
    end = C.row.astype(np.int64)[1:][r] - 1  # last entry of each entry's row
    k_all = np.arange(len(c))
    nxt = np.where(k_all < end, c[np.minimum(k_all + 1, len(c) - 1)], C.n)
    free = np.nonzero((r != c) & (c + 1 < nxt) & (c + 1 != r))[0]
    m = _copy(levels)
    m[last].col[free[0]] += 1
    _expect("galerkin", m, rest)

    # one row's agg pointed at a non-adjacent aggregate
    F = levels[0]
    A = F.matrix()
    i = F.n // 2
    near = set(F.agg[A[i].indices].tolist())
    far = next(a for a in range(F.nc) if a not in near)
    m = _copy(levels)
    m[0].agg[i] = far
    _expect("partition", m, rest)

    # two members swapped in r_col
    I = int(np.argmax(np.diff(F.r_row.astype(np.int64)) >= 2))
    k0 = int(F.r_row[I])
    m = _copy(levels)
    m[0].r_col[[k0, k0 + 1]] = m[0].r_col[[k0 + 1, k0]]
    _expect("partition", m, rest)

    # de of one row taken from its neighbour
    i = int(np.argmax(F.de[:-1] != F.de[1:]))
    m = _copy(levels)
    m[0].de[i] = F.de[i + 1]
    assert m[0].de[i] != F.de[i]
    _expect("source", m, rest)

    # an orphan aggregate id
    m = _copy(levels)
    m[0].agg[m[0].agg == 3] = 4
    _expect("partition", m, rest)


def _wide_columns_levels():
    mesh = ac.wide_columns_mesh()
    s = ac.built_solver(OracleSolver, mesh, fixed_inner=4)
    return amg.read_hierarchy(s), None, None, mesh


@pytest.mark.parametrize("name", MULTI_LEVEL + ["block_shuffle"])
def test_measured_k_still_discriminates(name):
    """Each error, applied inside the f64 cycle and compared with the unmutated
    one, exceeds K eps32 M on some row, on strip130, backwards_step, graded,
    voronoi and the block-shuffled 32-bit-column mesh.  Not on the other cases
    (worst ratio over the two vector pairs, against K = 4.9e-3): strip1 and
    strip7 have no post-sweep or prolongation to drop (ratio 0); on strip1 the
    omega error gives 9.3e-5 (ten sweeps of a one-row level converge whatever
    omega is) and nine sweeps 9.7e-3; strip7 shows omega (3.8) and nine sweeps
    (389); wheel100 shows omega (2.3e-2), the post-sweep (12) and the
    prolongation (650) but not nine sweeps, 2.7e-4 to 1.0e-3: its one-row
    coarse level has converged after nine.  On the six-level block_shuffle mesh
    the majorant has grown so far that only the smooth pair shows the errors
    (post-sweep 1.0, nine sweeps 7.6e-2, prolongation 0.19; the random pair
    shows the post-sweep alone, 4.8e-2) and the omega error stays below K on
    every pair (1.2e-3 at most): there the agreement check cannot see an
    omega off by 2^-10.  K is measured, not tuned, so this is reported, not
    repaired."""
    levels, _, _, mesh = _levels(name) if name != "block_shuffle" else _wide_columns_levels()
    pairs = ac.case_vectors(levels, mesh)
    pairs, unseen = (pairs[:2], ()) if name != "block_shuffle" else (pairs[1:2], ("omega 0.8 (1 + 2^-10)",))
    mutations = {
        "omega 0.8 (1 + 2^-10)": dict(omega=0.8 * (1.0 + 2.0 ** -10)),
        "post-sweep dropped": dict(post_sweep=False),
        "nine coarsest sweeps": dict(coarsest_sweeps=9),
        "one aggregate's prolongation dropped": dict(drop_aggregate=(0, levels[0].nc // 2)),
    }
    for label, x0, b, _ in pairs:
        ref = amg.vcycle64(levels, x0, b)
        for what, kw in mutations.items():
            if what in unseen:
                continue
            ratio, row = amg.vcycle_deviation(levels, x0, b, amg.vcycle64(levels, x0, b, **kw))
            assert ratio > ac.K, f"{name}: {label}: {what}: only {ratio:.3e} eps32 M at row {row}, K = {ac.K:.3e}"
            with pytest.raises(AssertionError, match="^agreement:"):
                amg.check_vcycle_agreement(levels, x0, b, amg.vcycle64(levels, x0, b, **kw), ac.K, what)
        assert amg.check_vcycle_agreement(levels, x0, b, ref, ac.K, label) == levels[0].n


def test_linearity_check_sees_stale_scratch():
    """A cycle that keeps something from the previous call fails check_linearity."""
    levels, _, _, mesh = _levels("strip130")
    _, x0, b, _ = ac.case_vectors(levels, mesh)[0]
    state = {"prev": np.zeros(levels[0].n, dtype=np.float32)}

    def leaky(x, rhs):
        out = (amg.vcycle64(levels, x, rhs) + 1e-3 * state["prev"]).astype(np.float32)
        state["prev"] = out
        return out

    with pytest.raises(AssertionError, match="^linearity:"):
        amg.check_linearity(leaky, x0, b)


# ------------------------------------------------- preconditioner identity
@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", list(ac.MESHES))
def test_precond_identity_f64(name, precond):
    """z_u = D_u^-1 (v_u - A_up z_p) per row, whatever solved the pressure block."""
    assert ac.run_precond_identity(OracleSolver, name, precond) == 4 * fv_cases.mesh_of(name).num_cells()


def test_precond_identity_detects_mutations():
    rec = []
    ac.run_precond_identity(OracleSolver, "backwards_step", 1, record=rec)
    sysm, v, z = rec[0]
    i = len(z) // 6
    # the velocity correction of one cell off by 64 eps32 of its terms
    zp = z.astype(np.float64)[2::3]
    term = abs(sysm.dinv[0][i]) * (abs(float(v[3 * i])) + (abs(sysm.block("u", "p")) @ np.abs(zp))[i])
    m = z.copy()
    m[3 * i] += np.float32(64.0 * EPS32 * term)
    with pytest.raises(AssertionError, match=f"^precond identity: .*cell {i}: z_u"):
        amg.check_precond_identity(sysm, v, m)
    # the correction of one cell dropped (z_v left at the prediction D_v^-1 v_v)
    m = z.copy()
    m[3 * i + 1] = np.float32(sysm.dinv[1][i] * float(v[3 * i + 1]))
    assert m[3 * i + 1] != z[3 * i + 1]
    with pytest.raises(AssertionError, match="^precond identity: .*z_v"):
        amg.check_precond_identity(sysm, v, m)
    # a diagonal inverse taken from the neighbouring cell
    j = int(np.argmax(sysm.dinv[0][:-1] != sysm.dinv[0][1:]))
    bad = sysm.copy()
    bad.dinv[0][j] = sysm.dinv[0][j + 1]
    with pytest.raises(AssertionError, match=f"^precond identity: .*cell {j}: z_u"):
        amg.check_precond_identity(bad, v, z)
    assert amg.check_precond_identity(sysm, v, z) == 2 * len(zp)


# ------------------------------------------------------------ the entry points
def test_debug_calls_leave_the_solver_state_untouched():
    """Stepping after the two read-backs gives the bits of a solver that never
    called them (the GPU module runs the same test on the HIP path)."""
    mesh = fv_cases.mesh_of("backwards_step")
    a, b = (ac.built_solver(OracleSolver, mesh, fixed_inner=6) for _ in range(2))
    levels = amg.read_hierarchy(a)
    rng = np.random.default_rng(7)
    a.debug_amg_vcycle(rng.standard_normal(levels[0].n), rng.standard_normal(levels[0].n))
    a.debug_apply_precond(rng.standard_normal(3 * levels[0].n))
    for _ in range(2):
        a.step()
        b.step()
        assert np.array_equal(a.get_u(), b.get_u()) and np.array_equal(a.get_p(), b.get_p())


def test_readbacks_need_a_built_hierarchy():
    from cfd2_amd import default_config
    mesh = fv_cases.mesh_of("strip7")
    s = OracleSolver(mesh, config=default_config(fixed_outer=1))
    with pytest.raises(RuntimeError, match="hierarchy"):
        s.debug_amg_level(0)
    with pytest.raises(RuntimeError, match="hierarchy"):
        s.debug_amg_vcycle(np.zeros(7), np.zeros(7))
    fv_cases.setup_solve(s, mesh, 1)
    s.step()
    with pytest.raises(RuntimeError, match="no such AMG level"):
        s.debug_amg_level(1)
