"""Float64 checks of the AMG hierarchy and V-cycle (tests/amg_checks.py) on the
HIP path: the drivers of tests/amg_cases.py on GpuSolver, the V-cycle checks
under every kernel variant of tests/test_gpu_parity.py::VARIANTS (the default
plan runs the suite's small meshes inside the one-workgroup tail kernel, so the
per-level kernels are forced with the existing knobs), the 32-bit column
levels, the wide (16-bit length) levels, both setups and the numeric refresh.
Independent of bit parity with the oracle: what is asserted is that the levels
are a correct Galerkin hierarchy of the step's matrix and that the kernels'
cycle is the V-cycle of those levels."""
import re

import numpy as np
import pytest

from cfd2_amd import GpuSolver
from tests import amg_cases as ac
from tests import amg_checks as amg
from tests import fv_cases
from tests.test_gpu_parity import VARIANTS, _assert_same_info

pytestmark = pytest.mark.gpu

PAIRS = {"CFD_AMG_FUSED_PAIR": "2", "CFD_AMG_TAIL_ROWS": "0"}  # both pair kernels wherever a pair is possible
VARIANT_MESHES = ["backwards_step", "graded", "strip130"]


def _id(env):
    return ",".join(f"{k}={v}" for k, v in env.items())


@pytest.mark.parametrize("density", ac.DENSITIES)
@pytest.mark.parametrize("name", list(ac.MESHES))
def test_hierarchy_and_vcycle_f64_gpu(name, density):
    levels, counts, rows = ac.run_case(GpuSolver, name, density)
    assert counts["source"] > 0 and counts["consequences"] > 0 and counts["stop"] == len(levels)
    if len(levels) > 1:
        assert counts["partition"] > 0 and counts["galerkin"] > 0
    assert rows == 4 * levels[0].n


@pytest.mark.parametrize("env", VARIANTS + [PAIRS], ids=_id)
@pytest.mark.parametrize("name", VARIANT_MESHES)
def test_vcycle_f64_under_kernel_variants(name, env, monkeypatch, capfd):
    """Agreement with the f64 cycle and non-expansion under each forced kernel
    form: per-level smoother, separate and fused residual-restriction and
    prolongation, both pair kernels, the lds / global / blob tails, predicated
    and full slot loads, nontemporal loads."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mesh = fv_cases.mesh_of(name)
    capfd.readouterr()
    s = ac.built_solver(GpuSolver, mesh, log_level=2)
    err = capfd.readouterr().err
    try:
        levels, _ = ac.hierarchy_counts(s, mesh)
        rows = ac.vcycle_checks(s, mesh, levels, f"{name} {_id(env)}", linearity=False)
        assert rows == 4 * mesh.num_cells()
    finally:
        s.close()
    m = re.search(r"tail from level (-?\d+) .*down-leg pairs:(.*), up-leg pairs:(.*)\n", err)
    assert m, "no AMG setup line"
    if env.get("CFD_AMG_TAIL_ROWS") == "0":
        assert int(m.group(1)) == len(levels), "the tail kernel still runs some level"
    if env is PAIRS:
        # a pair needs two levels on a leg, and the last level runs on neither
        for grp in (2, 3):
            pairs = [] if m.group(grp).strip() == "none" else m.group(grp).split()
            assert (len(pairs) > 0) == (len(levels) >= 3), (name, grp, pairs)


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("name", list(ac.MESHES))
def test_precond_identity_f64_gpu(name, precond):
    """z_u = D_u^-1 (v_u - A_up z_p) per row through the Schur prediction and
    correction kernels, with the Jacobi relaxation and with the V-cycle."""
    assert ac.run_precond_identity(GpuSolver, name, precond) == 4 * fv_cases.mesh_of(name).num_cells()


def test_debug_entries_refuse_a_distributed_handle():
    from cfd2_amd import GpuGroup, default_config
    mesh = fv_cases.mesh_of("backwards_step")
    g = GpuGroup(mesh, 2, config=default_config(fixed_outer=1, fixed_inner=4))
    try:
        r = g.ranks[0]
        n = r.num_cells
        for call in (lambda: r.debug_amg_level(0), lambda: r.debug_amg_vcycle(np.zeros(n), np.zeros(n)),
                     lambda: r.debug_apply_precond(np.zeros(3 * n))):
            with pytest.raises(RuntimeError, match=r"status 1\).*one GPU only"):
                call()
    finally:
        g.close()


def test_wide_columns_levels_f64(monkeypatch, capfd):
    """Level 0 on 32-bit columns (the block-shuffled 38 k-cell mesh): the
    hierarchy checks on every level and the V-cycle agreement, under the
    default plan and with every level launched."""
    mesh = ac.wide_columns_mesh()
    for tail_rows in (None, "0"):
        if tail_rows is not None:
            monkeypatch.setenv("CFD_AMG_TAIL_ROWS", tail_rows)
        capfd.readouterr()
        s = ac.built_solver(GpuSolver, mesh, fixed_inner=4, log_level=2)
        m = re.search(r"tail from level (-?\d+) ", capfd.readouterr().err)
        assert m, "no AMG setup line"
        try:
            assert (int(m.group(1)) == len(s.amg_levels())) == (tail_rows == "0"), "which levels the tail kernel runs"
            coupled16, lv16 = s.column_widths()
            assert coupled16 == 0 and lv16[0] == 0, "a 32-bit level must have run"
            levels, counts, rows = ac.run_wide_columns(GpuSolver, solver=s)
            assert [L.use16 for L in levels] == [bool(u) for u in lv16]
            assert counts["galerkin"] > 0 and rows == 4 * mesh.num_cells()
        finally:
            s.close()


@pytest.mark.parametrize("tail", ["blob2", "global"])
def test_wide_rows_levels_f64(monkeypatch, tail):
    """Levels with 16-bit row lengths (CFD_AMG_WIDE_LIMIT lowered, as
    test_wide_amg_rows_take_the_16bit_path_bitexact does): the read-back
    expands them, and they pass the hierarchy and V-cycle checks."""
    monkeypatch.setenv("CFD_AMG_WIDE_LIMIT", "5")
    monkeypatch.setenv("CFD_AMG_TAIL", tail)
    mesh = fv_cases.mesh_of("backwards_step")
    s = ac.built_solver(GpuSolver, mesh)
    try:
        assert s.amg_setup_info()[0] == 1
        levels, counts = ac.hierarchy_counts(s, mesh)
        assert not levels[0].wide and any(L.wide for L in levels[1:]), [L.wide for L in levels]
        assert ac.vcycle_checks(s, mesh, levels, f"wide rows, tail {tail}") == 4 * mesh.num_cells()
    finally:
        s.close()


@pytest.mark.parametrize("setup,path", [("host", 1), (None, 2)])
@pytest.mark.parametrize("name", ["backwards_step", "graded", "voronoi"])
def test_host_and_device_setup_pass_the_hierarchy_checks(name, setup, path, monkeypatch):
    """Each on its own, whatever test_amg_device_setup_matches_host says of
    their equality."""
    if setup:
        monkeypatch.setenv("CFD_AMG_SETUP", setup)
    mesh = fv_cases.mesh_of(name)
    s = ac.built_solver(GpuSolver, mesh)
    try:
        assert s.amg_setup_info()[0] == path
        levels, counts = ac.hierarchy_counts(s, mesh)
        assert counts["galerkin"] > 0 and len(levels) >= 3
    finally:
        s.close()


@pytest.mark.parametrize("name", ["backwards_step", "voronoi"])
def test_numeric_refresh_passes_the_galerkin_check(name):
    """amg_rebuild_interval = 1: the second step refreshes the values over the
    kept structure; the refreshed hierarchy is the Galerkin hierarchy of the
    second step's matrix."""
    mesh = fv_cases.mesh_of(name)
    s = ac.built_solver(GpuSolver, mesh, amg_rebuild_interval=1)
    try:
        first = s.debug_buffer(8)
        before = amg.read_hierarchy(s)
        digests = s.amg_setup_info()[1]
        s.set_dt(0.0007)  # a different time coefficient: the second step's matrix has other values
        s.update_constants()
        s.step()
        second = s.debug_buffer(8)
        assert not np.array_equal(first, second), "the matrix did not change: nothing to refresh"
        # the device setup's numeric refresh ran: path 2, other values in the same structure
        path, after = s.amg_setup_info()
        assert path == 2 and len(after) == len(digests) and all(a != b for a, b in zip(after, digests))
        levels, counts = ac.hierarchy_counts(s, mesh, second)
        assert counts["galerkin"] > 0
        for a, b in zip(before, levels):
            assert np.array_equal(a.row, b.row) and np.array_equal(a.col, b.col)
            assert a.nc == b.nc and (a.agg is None or np.array_equal(a.agg, b.agg))
        assert any(not np.array_equal(a.val, b.val) for a, b in zip(before[1:], levels[1:]))
        assert ac.vcycle_checks(s, mesh, levels, f"{name} refreshed", linearity=False) == 4 * mesh.num_cells()
    finally:
        s.close()


@pytest.mark.parametrize("graph", [False, True])
def test_debug_calls_leave_the_solver_state_untouched(graph):
    """A solver that calls the two entries between steps keeps the bits of one
    that does not (eager launches and hipGraph replay of the iteration)."""
    mesh = fv_cases.mesh_of("backwards_step")
    a, b = (ac.built_solver(GpuSolver, mesh, fixed_inner=6) for _ in range(2))
    try:
        for s in (a, b):
            s.graph_enable(graph)
        rng = np.random.default_rng(7)
        for _ in range(3):
            levels = amg.read_hierarchy(a)
            out = a.debug_amg_vcycle(rng.standard_normal(levels[0].n), rng.standard_normal(levels[0].n))
            assert np.all(np.isfinite(out))
            assert np.all(np.isfinite(a.debug_apply_precond(rng.standard_normal(3 * levels[0].n))))
            a.step()
            b.step()
            assert np.array_equal(a.get_u(), b.get_u()) and np.array_equal(a.get_p(), b.get_p())
            _assert_same_info(a, b, "after the debug calls")  # everything but the wall-clock time
    finally:
        a.close()
        b.close()


def test_readbacks_need_a_built_hierarchy():
    from cfd2_amd import default_config
    mesh = fv_cases.mesh_of("strip7")
    s = GpuSolver(mesh, config=default_config(fixed_outer=1))
    try:
        with pytest.raises(RuntimeError, match="status 1"):
            s.debug_amg_level(0)
        with pytest.raises(RuntimeError, match="status 1"):
            s.debug_amg_vcycle(np.zeros(7), np.zeros(7))
        fv_cases.setup_solve(s, mesh, 1)
        s.step()
        with pytest.raises(RuntimeError, match="status 1"):
            s.debug_amg_level(1)
        assert s.debug_amg_level(0)["n"] == 7
    finally:
        s.close()
