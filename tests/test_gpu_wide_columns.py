"""The 32-bit column forms of every row kernel, tied to the oracle bit for bit.

Every row kernel on the hot path exists twice: one form reads 16-bit column
deltas (use16 = 1), the other 32-bit absolute columns (use16 = 0).  The host
picks per matrix and per AMG level: 32-bit as soon as one |col - row| leaves
[-32768, 32767].  The cut-cell channels of the other tests are numbered column
by column and every other mesh there has fewer than 32,768 cells, so they all
run the 16-bit forms.  Here the same channel, just above 32,768 cells, is
RENUMBERED (tests/synthetic.py renumbered(): the mesh is the same, the cell
ids are not), which is what a Voronoi / Delaunay mesh of that size or any
mesh in generator order looks like to the kernels:

  far swap       first 64 cells <-> last 64: nearly every row stays regular
                 and consecutive (vector gathers, derived columns), the matrix
                 as a whole is 32-bit
  block shuffle  blocks of 1,024 cells in seeded random order: locality inside
                 a block, large deltas across block edges
  random         a seeded permutation: no regular row, every load scattered

Every case asserts through cfd_debug_column_widths that the form it is meant
to run did run, then GPU == OracleSolver on the same renumbered mesh with no
tolerance.  The oracle's answer for a mesh / preconditioner / schedule is
computed once and shared by the cases that use it (the kernel variants change
which kernel runs, never the result)."""
import functools
import re

import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver, default_config
from cfd2_amd import _ffi
from cfd2_amd.mesh import channel_obstacle_h
from cfd2_amd.solver import dist_plan
from tests import refpy
from tests.meshes import bench_mesh
from tests.oracle_py import OracleSolver
from tests.synthetic import (NONE, perm_block_shuffle, perm_far_swap, perm_random, red_units, renumbered)
from tests.test_gpu_parity import VARIANTS, _assert_same_fields, _assert_same_info, _setup_amg_test

pytestmark = pytest.mark.gpu

KINDS = ["far_swap", "block_shuffle", "random"]
SCHEDULE = dict(fixed_outer=2, fixed_inner=8)
BLOCK = 1024  # of the block shuffle: CFD_AMG_FUSED_PAIR=2 pairs level 0 on both legs at this size


@functools.lru_cache(maxsize=None)
def _base(which="base"):
    """base: 38,404 cells, the smallest channel where a delta can leave 16 bits
    (reduction geometry g = 1, G = 2, U = 2).  coarse32: 76,703 cells, the
    smallest whose AMG level 1 (37,105 rows under the block shuffle) clears
    32,768 rows by about 10 %."""
    m = bench_mesh(channel_obstacle_h(38000 if which == "base" else 76000), 30)
    n = m.num_cells()
    assert (36000 <= n <= 40000) if which == "base" else (70000 <= n <= 85000), n
    return m


@functools.lru_cache(maxsize=None)
def _mesh(kind, which="base"):
    base = _base(which)
    n = base.num_cells()
    perm = {"far_swap": perm_far_swap, "random": perm_random,
            "block_shuffle": lambda k: perm_block_shuffle(k, block=BLOCK)}[kind](n)
    m = renumbered(base, perm)
    a = m.arrays()
    nb = a["face_neighbor"].astype(np.int64)
    inner = nb != NONE
    # never vacuous: some face joins two cells more than 16 bits apart
    assert np.abs(a["face_owner"].astype(np.int64)[inner] - nb[inner]).max() > 32767, kind
    return m


class _Snapshot:
    """What _assert_same_fields / _assert_same_info read of a solver, frozen."""

    def __init__(self, s):
        self._u, self._p, self._d = s.get_u(), s.get_p(), s.get_d_p()
        for a in (self._u, self._p, self._d):
            a.setflags(write=False)
        self._info = bytes(s.step_info())

    def get_u(self): return self._u
    def get_p(self): return self._p
    def get_d_p(self): return self._d
    def step_info(self): return _ffi.StepInfo.from_buffer_copy(self._info)


@functools.lru_cache(maxsize=None)
def _oracle(kind, precond, steps=2, which="base", nranks=1, semantics=0, rebuild=0):
    """The oracle's state after each step, computed once per configuration."""
    mesh = _mesh(kind, which)
    cfg = dict(SCHEDULE)
    if rebuild:
        cfg["amg_rebuild_interval"] = rebuild
    o = OracleSolver(mesh, config=default_config(**cfg), nranks=nranks)
    if semantics:
        o.set_semantics(semantics)
    _setup_amg_test(o, mesh, precond)
    out = []
    for _ in range(steps):
        o.step()
        out.append(_Snapshot(o))
    levels = tuple(o.amg_levels())
    return out, levels


def _assert_wide(g, levels16=None, ctx=""):
    """The coupled kernels and AMG level 0 read 32-bit columns; levels16: the
    levels that must be on 16-bit deltas (fewer than 32,768 rows: no delta can
    leave 16 bits)."""
    cu, lv = g.column_widths()
    assert cu == 0, f"{ctx}: the coupled kernels ran on 16-bit deltas"
    if lv:
        assert lv[0] == 0, f"{ctx}: AMG level 0 ran on 16-bit deltas"
        rows = [r for r, _ in g.amg_levels()]
        for i, r in enumerate(rows):
            if r <= 32768:
                assert lv[i] == 1, f"{ctx}: level {i} ({r} rows) is 32-bit"
        for i in levels16 or ():
            assert lv[i] == 1 and rows[i] <= 32768, (ctx, i, lv, rows)
    return cu, lv


def _run(g, kind, precond, steps=2, ctx="", **okw):
    """`steps` steps, each == the oracle's; one GPU: the same level sizes too
    (a rank of a group reports its own rows of the distributed levels)."""
    ref, levels = _oracle(kind, precond, steps, **okw)
    for k in range(steps):
        g.step()
        _assert_same_fields(g, ref[k], f"{ctx} step {k}")
        _assert_same_info(g, ref[k], f"{ctx} step {k}")
    if precond == 1 and okw.get("nranks", 1) == 1:
        assert tuple(g.amg_levels()) == levels, ctx
    return ref


def test_base_mesh_reduces_in_units_of_two_chunks():
    """36,000..40,000 cells sit in g = 1, G = 2, U = 2 of the canonical
    reduction tree (kernels.hpp red_geom), between the small meshes (U = 1)
    and the units-of-four tests (U = 4); every case of this file runs there."""
    n = _base().num_cells()
    assert red_units(n) == (1, 2, 2) and refpy._geom(n)[0] == 2


@pytest.mark.parametrize("precond", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_renumbered_parity_default_knobs(kind, precond):
    """k_spmv2<false>, k_precond_predict2<false>, the 32-bit Schur correct and
    k_relax_pressure4; with AMG the level-0 smoother, residual, restriction,
    prolongation (32-bit) over 16-bit coarse levels and the tail."""
    mesh = _mesh(kind)
    g = GpuSolver(mesh, config=default_config(**SCHEDULE))
    _setup_amg_test(g, mesh, precond)
    assert g.column_widths() == (0, [])  # known at creation, before any launch
    _run(g, kind, precond, ctx=f"{kind} precond {precond}")
    cu, lv = _assert_wide(g, levels16=[1] if precond == 1 else None, ctx=kind)
    assert (len(lv) >= 3) == (precond == 1)
    assert np.abs(g.get_p()).max() > 0.0
    g.close()


# the rows of VARIANTS that change which row kernel runs (CFD_AMG_TAIL=lds/global
# change the single-workgroup tail only, far below 32,768 rows)
ROW_VARIANTS = [v for v in VARIANTS if "CFD_AMG_TAIL" not in v]


def test_row_variants_cover_the_knobs():
    keys = {(k, v) for e in ROW_VARIANTS for k, v in e.items()}
    for want in (("CFD_AMG_FULL", "0"), ("CFD_AMG_FULL", "1"), ("CFD_AMG_TAIL_ROWS", "0"),
                 ("CFD_AMG_FUSED_RR_ROWS", "0"), ("CFD_AMG_FUSED_RR_ROWS", "4000000000"),
                 ("CFD_AMG_FUSED_PROLONG_ROWS", "0"), ("CFD_AMG_FUSED_PROLONG_ROWS", "4000000000"),
                 ("CFD_NT", "127"), ("CFD_SMALL_MESH_FORMS", "0")):
        assert want in keys, want


@pytest.mark.parametrize("env", ROW_VARIANTS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
@pytest.mark.parametrize("kind", ["block_shuffle", "far_swap"])
def test_renumbered_kernel_variants(kind, env, monkeypatch):
    """Every AMG_ROWS_KERNEL dispatch (smooth, smooth-zero, smooth with fused
    prolongation, residual; full and predicated slot loads; nontemporal),
    k_amg_resrestrict<false> fused and split, the streaming coupled forms: the
    32-bit side of each on level 0."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    mesh = _mesh(kind)
    g = GpuSolver(mesh, config=default_config(**SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    _run(g, kind, 1, ctx=f"{kind} {env}")
    _assert_wide(g, levels16=[1], ctx=f"{kind} {env}")
    g.close()


def _pairs(err):
    """(down-leg pairs, up-leg pairs) of the AMG setup line (cfg.log_level 2)."""
    m = re.search(r"down-leg pairs:(.*), up-leg pairs:(.*)\n", err)
    assert m, "no AMG setup line"
    return tuple([] if m.group(i).strip() == "none" else [tuple(int(x) for x in p.split("+")) for p in m.group(i).split()]
                 for i in (1, 2))


# The up leg pairs greedily from the coarsest level the cycle runs
# (Solver::build_rr_pairs), so level 0 is in an up-leg pair only when the
# cycle runs an even number of levels.  With no tail the base mesh runs five
# (pairs 4+3, 2+1, level 0 alone); a tail of the levels of at most 600 rows
# (level 4 and below: ~300 rows) leaves four, and the pairs are 3+2, 1+0.
@pytest.mark.parametrize("tail_rows", ["0", "600"])
@pytest.mark.parametrize("kind", ["far_swap", "block_shuffle"])
def test_pairs_with_level0(kind, tail_rows, monkeypatch, capfd):
    """CFD_AMG_FUSED_PAIR=2: a down-leg pair that holds level 0
    (k_amg_resrestrict_pair<false, 256>), and, where the cycle runs an even
    number of levels, an up-leg pair that holds it
    (k_amg_prolong_smooth_pair<false, true>: 32-bit fine level, 16-bit coarse)."""
    monkeypatch.setenv("CFD_AMG_TAIL_ROWS", tail_rows)
    monkeypatch.setenv("CFD_AMG_FUSED_PAIR", "2")
    mesh = _mesh(kind)
    g = GpuSolver(mesh, config=default_config(log_level=2, **SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    capfd.readouterr()
    _run(g, kind, 1, ctx=f"pairs {kind}")
    down, up = _pairs(capfd.readouterr().err)
    print(f"{kind} tail rows {tail_rows}: down-leg pairs {down}, up-leg pairs {up}")
    assert (0, 1) in down, f"{kind}: no down-leg pair with level 0: {down}"
    if tail_rows != "0":
        assert (1, 0) in up, f"{kind}: no up-leg pair with level 0: {up}"
    else:
        assert up, up
    _assert_wide(g, levels16=[1], ctx=f"pairs {kind}")
    g.close()


def test_coarse_level_32bit(monkeypatch, capfd):
    """A mesh whose AMG level 1 has more than 32,768 rows and, block-shuffled,
    32-bit columns itself: k_amg_resrestrict<false> on level 1, the level-1
    row kernels, the down-leg pair 0+1 and the up-leg pair 1+0 with both
    levels 32-bit (k_amg_prolong_smooth_pair<false, false>)."""
    monkeypatch.setenv("CFD_AMG_TAIL_ROWS", "0")  # seven levels, six in the cycle: the up leg pairs 1+0
    monkeypatch.setenv("CFD_AMG_FUSED_PAIR", "2")
    kind = "block_shuffle"
    mesh = _mesh(kind, "coarse32")
    g = GpuSolver(mesh, config=default_config(log_level=2, **SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    capfd.readouterr()
    _run(g, kind, 1, steps=1, ctx="coarse32", which="coarse32")
    down, up = _pairs(capfd.readouterr().err)
    rows = [r for r, _ in g.amg_levels()]
    cu, lv = _assert_wide(g, ctx="coarse32")
    print(f"coarse32: rows {rows}, use16 {lv}, down-leg pairs {down}, up-leg pairs {up}")
    assert rows[1] >= 1.08 * 32768, rows
    assert lv[1] == 0, f"level 1 ({rows[1]} rows) ran on 16-bit deltas: {lv}"
    assert lv[2] == 1 and rows[2] < 32768
    assert (0, 1) in down and (1, 0) in up, (down, up)
    g.close()


def test_coarse_level_32bit_default_knobs():
    """The same mesh with the default knobs (no pairs, default tail)."""
    kind = "block_shuffle"
    mesh = _mesh(kind, "coarse32")
    g = GpuSolver(mesh, config=default_config(**SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    _run(g, kind, 1, steps=1, ctx="coarse32 default", which="coarse32")
    cu, lv = _assert_wide(g, ctx="coarse32 default")
    assert lv[1] == 0, lv
    g.close()


def test_reference_semantics_mode():
    """debug_reference_semantics(15): k_amg_smooth_ordered<false, *> and
    k_prepare_ordered on 32-bit columns == the oracle with the same flags."""
    kind = "far_swap"
    mesh = _mesh(kind)
    g = GpuSolver(mesh, config=default_config(**SCHEDULE))
    g.debug_reference_semantics(15)
    _setup_amg_test(g, mesh, 1)
    _run(g, kind, 1, ctx="reference semantics 15", semantics=15)
    _assert_wide(g, levels16=[1], ctx="reference semantics 15")
    plain, _ = _oracle(kind, 1)
    assert not np.array_equal(plain[-1].get_p(), g.get_p()), "flags 15 changed nothing: the mode did not run"
    g.close()


@pytest.mark.parametrize("kind", ["block_shuffle", "random"])
def test_device_setup_matches_host_setup(kind, monkeypatch):
    """The 32-bit branches of the device AMG setup (Galerkin product, packing
    of a 32-bit level): the hierarchy bytes of the device setup == the host
    setup's, level by level, and both runs == the oracle."""
    mesh = _mesh(kind)
    runs = {}
    for path in ("device", "host"):
        if path == "host":
            monkeypatch.setenv("CFD_AMG_SETUP", "host")
        else:
            monkeypatch.delenv("CFD_AMG_SETUP", raising=False)
        g = GpuSolver(mesh, config=default_config(**SCHEDULE))
        _setup_amg_test(g, mesh, 1)
        _run(g, kind, 1, ctx=f"{kind} {path} setup")
        _assert_wide(g, levels16=[1], ctx=f"{kind} {path} setup")
        runs[path] = (g.amg_setup_info(), g.amg_levels())
        g.close()
    (pd, dd), (ph, dh) = runs["device"][0], runs["host"][0]
    assert (pd, ph) == (2, 1), "device setup must be the path taken on one GPU"
    assert runs["device"][1] == runs["host"][1] and len(dd) >= 3
    assert dd == dh, [i for i, (a, b) in enumerate(zip(dd, dh)) if a != b]


def test_numeric_refresh_of_a_32bit_level():
    """amg_rebuild_interval = 1, three steps: Solver::level_csr and the numeric
    refresh read and refill a 32-bit level 0."""
    kind = "block_shuffle"
    mesh = _mesh(kind)
    g = GpuSolver(mesh, config=default_config(amg_rebuild_interval=1, **SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    _run(g, kind, 1, steps=3, ctx="refresh", rebuild=1)
    _assert_wide(g, levels16=[1], ctx="refresh")
    assert g.amg_setup_info()[0] == 2
    g.close()


def _rank_max_delta(mesh, nranks, rank):
    """(largest |local col - local row| over rank's owned rows, window rows):
    cfd_dist_plan's window -- low ghosts, owned rows padded to 64, high ghosts."""
    p = dist_plan(mesh, nranks, rank)
    c0, c1, ghost = p["c0"], p["c1"], p["ghost"].astype(np.int64)
    glo = int(np.searchsorted(ghost, c0))
    npad = -(-(c1 - c0) // 64) * 64
    a = mesh.arrays()
    own, nb = a["face_owner"].astype(np.int64), a["face_neighbor"].astype(np.int64)
    inner = nb != NONE
    row = np.concatenate([own[inner], nb[inner]])
    col = np.concatenate([nb[inner], own[inner]])
    mine = (row >= c0) & (row < c1)
    row, col = row[mine], col[mine]
    k = np.searchsorted(ghost, col)
    local = np.where((col >= c0) & (col < c1), col - c0, np.where(k < glo, k - glo, npad + (k - glo)))
    return int(np.abs(local - (row - c0)).max()), len(ghost), p


@pytest.mark.parametrize("nranks", [2, 3])
@pytest.mark.parametrize("kind", ["far_swap", "block_shuffle"])
def test_renumbered_several_ranks(kind, nranks, monkeypatch):
    """GpuGroup on a renumbered mesh, coarse levels distributed
    (CFD_AMG_REPLICATE_ROWS=200): R ranks == the oracle bit for bit.  The far
    swap makes the first and the last rank neighbours (on 3 ranks: two ranks
    that share no slab edge); the block shuffle makes every rank border every
    other, with ghost ranges of thousands of rows.  A rank's window (its slab
    plus ghosts) stays under 32,768 rows here, so each rank's own matrices are
    on 16-bit deltas again -- asserted, from the halo plan."""
    monkeypatch.setenv("CFD_AMG_REPLICATE_ROWS", "200")
    mesh = _mesh(kind)
    n = mesh.num_cells()
    from tests.synthetic import max_ranks
    assert nranks <= max_ranks(n)
    peers, ghosts = [], []
    for r in range(nranks):
        dmax, ng, p = _rank_max_delta(mesh, nranks, r)
        assert dmax <= 32767, (r, dmax)
        assert (p["c1"] - p["c0"]) % 512 == 0 or r == nranks - 1  # whole reduction segments (G = 2 chunks)
        peers.append(set(p["peers"]))
        ghosts.append(ng)
    if kind == "far_swap":
        assert nranks - 1 in peers[0] and 0 in peers[nranks - 1]
    else:
        assert all(peers[r] == set(range(nranks)) - {r} for r in range(nranks)), peers
        assert min(ghosts) > 1000, ghosts
    g = GpuGroup(mesh, nranks, config=default_config(**SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    _run(g, kind, 1, ctx=f"{kind} R={nranks}", nranks=nranks)
    cu, lv = g.column_widths()  # asserts that the ranks agree
    assert cu == 1 and lv[0] == 1, (cu, lv)
    g.close()


def test_renumbered_two_ranks_32bit_windows(monkeypatch):
    """Two ranks on the 76,703-cell block shuffle: each rank's window exceeds
    32,768 rows and holds deltas beyond 16 bits (computed from the halo plan),
    so the distributed kernels (halo rows, ghost columns) run their 32-bit
    forms on both ranks."""
    monkeypatch.setenv("CFD_AMG_REPLICATE_ROWS", "200")
    kind = "block_shuffle"
    mesh = _mesh(kind, "coarse32")
    for r in range(2):
        dmax, _, _ = _rank_max_delta(mesh, 2, r)
        assert dmax > 32767, (r, dmax)
    g = GpuGroup(mesh, 2, config=default_config(**SCHEDULE))
    _setup_amg_test(g, mesh, 1)
    _run(g, kind, 1, steps=1, ctx="coarse32 R=2", which="coarse32", nranks=2)
    for r in range(2):
        cu, lv = g.ranks[r].column_widths()
        assert cu == 0 and lv[0] == 0, (r, cu, lv)
    g.close()


def test_flow_diagnostics_on_32bit_neighbours():
    """flow_diagnostics() reads fs.other (absolute 32-bit neighbour ids) on the
    block shuffle: gradients == k_prepare's, maxima and the f64 sums == the
    numpy reference of tests/test_gpu_flow_diag.py, in units of two chunks."""
    from tests.test_gpu_flow_diag import _check_gradients, _check_max_and_sums
    mesh = _mesh("block_shuffle")
    assert red_units(mesh.num_cells())[2] == 2
    s, vort, div = _check_gradients(mesh, True, with_refpy=False)
    assert s.column_widths()[0] == 0
    _check_max_and_sums(mesh, s, vort, div)
    s.close()


def test_scalar_advance_on_32bit_neighbours():
    """One advance_scalars() on the block shuffle == tests/scalar_ref.py bit
    for bit (phi, sweeps, last_delta), and the statistics' f64 integral in
    units of two chunks."""
    from tests.scalar_ref import ScalarRef
    from tests.test_gpu_scalar import STEP_DT, _bits, _check_stats, _fields, _flow
    mesh = _mesh("block_shuffle")
    assert red_units(mesh.num_cells())[2] == 2
    R = ScalarRef(mesh.arrays())
    s, dt = _flow(mesh, "steps")
    assert s.column_widths()[0] == 0 and dt is None
    flux = s.debug_buffer(0)
    s.enable_scalars(1)
    s.set_scalar_params(0, 0.01, 0.25)
    phi = _fields(mesh)[1].astype(np.float32)
    s.set_scalar(0, phi)
    phi, sw, delta, conv = R.advance(flux, s.constants.density, STEP_DT, 0.01, 0.25, phi)
    s.advance_scalars(None)
    st = s.scalar_stats(0)
    assert (st.sweeps, bool(st.converged)) == (sw, conv) and conv
    assert _bits(st.last_delta) == _bits(delta)
    assert np.array_equal(_bits(s.get_scalar(0)), _bits(phi))
    _check_stats(s, mesh, _fields(mesh)[1] - 0.7)
    s.close()
