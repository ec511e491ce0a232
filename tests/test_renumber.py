"""tests/synthetic.py renumbered(): relabelling the cells of a mesh.  The GPU
tests of the 32-bit column kernels (tests/test_gpu_wide_columns.py) stand on
this helper, so it is pinned here without a GPU: identity and round trip
reproduce every array, the two independent CPU restatements (the oracle and
tests/refpy.py) agree bit for bit on renumbered meshes, and the float64
identities of the assembled system hold on one."""
import numpy as np
import pytest

from cfd2_amd import default_config
from tests import fv_cases as fc
from tests import fv_checks as fv
from tests import refpy
from tests.meshes import channel_obstacle
from tests.oracle_py import OracleSolver
from tests.synthetic import (NONE, inverse_perm, perm_block_shuffle, perm_far_swap, perm_random, red_units,
                             renumbered)
from tests.test_oracle import setup_amg_test
from tests.test_refpy import _same_step


def _small():
    return channel_obstacle(h=0.03)  # a few thousand cells, cut cells around the obstacle


def _perm(kind, n):
    if kind == "far_swap":
        return perm_far_swap(n)
    if kind == "block_shuffle":
        return perm_block_shuffle(n, block=256)  # several blocks on a small mesh
    return perm_random(n)


KINDS = ["far_swap", "block_shuffle", "random"]


def _same_arrays(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def test_identity_reproduces_every_array():
    m = _small()
    n = m.num_cells()
    assert 2000 < n < 6000
    _same_arrays(renumbered(m, np.arange(n)).arrays(), m.arrays())


@pytest.mark.parametrize("kind", KINDS)
def test_round_trip_reproduces_the_mesh(kind):
    m = _small()
    p = _perm(kind, m.num_cells())
    assert not np.array_equal(p, np.arange(len(p)))
    r = renumbered(m, p)
    _same_arrays(renumbered(r, inverse_perm(p)).arrays(), m.arrays())
    # and the relabelled mesh is the same mesh: per face, the same two cells
    a, b = m.arrays(), r.arrays()
    for k in ("face_boundary", "face_area", "face_nx", "face_ny", "face_cx", "face_cy"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(b["face_owner"], p[a["face_owner"].astype(np.int64)])
    inner = a["face_neighbor"] != NONE
    assert np.array_equal(b["face_neighbor"] == NONE, ~inner)
    assert np.array_equal(b["face_neighbor"][inner], p[a["face_neighbor"][inner].astype(np.int64)])
    for k in ("cell_cx", "cell_cy", "cell_vol"):
        assert np.array_equal(b[k][p], a[k]), k
    # every cell keeps its own faces in its own order
    oa, ob = a["cell_face_offsets"].astype(np.int64), b["cell_face_offsets"].astype(np.int64)
    for old in (0, 1, 63, 64, len(p) // 2, len(p) - 65, len(p) - 1):
        new = int(p[old])
        assert np.array_equal(a["cell_faces"][oa[old]:oa[old + 1]], b["cell_faces"][ob[new]:ob[new + 1]]), old


def test_permutation_builders():
    n = 5000
    for p in (perm_far_swap(n), perm_block_shuffle(n), perm_block_shuffle(n, block=256), perm_random(n)):
        assert np.array_equal(np.sort(p), np.arange(n))
    p = perm_far_swap(n)
    assert np.array_equal(p[:64], np.arange(n - 64, n)) and np.array_equal(p[n - 64:], np.arange(64))
    assert np.array_equal(p[64:n - 64], np.arange(64, n - 64))
    p = perm_block_shuffle(n)  # 4 blocks of 1024 and one of 904: consecutive inside a block
    for b in range(5):
        seg = p[b * 1024:min((b + 1) * 1024, n)]
        assert np.array_equal(seg - seg[0], np.arange(len(seg))), b
    assert np.array_equal(perm_block_shuffle(n), perm_block_shuffle(n))  # seeded
    assert not np.array_equal(perm_block_shuffle(n, seed=1), perm_block_shuffle(n, seed=2))
    assert np.array_equal(perm_random(n), perm_random(n))
    with pytest.raises(AssertionError, match="not a permutation"):
        renumbered(_small(), np.zeros(_small().num_cells(), dtype=np.int64))


def test_red_units_thresholds():
    """kernels.hpp red_geom restated: g = clamp(floor(log2(N / 16384)), 0, 8)."""
    assert red_units(32767) == (0, 1, 1)
    assert red_units(32768) == (1, 2, 2) and red_units(65535) == (1, 2, 2)
    assert red_units(65536) == (2, 4, 4) and red_units(131072) == (3, 8, 4)
    assert red_units(1 << 30) == (8, 256, 4)


@pytest.mark.parametrize("kind", KINDS)
def test_oracle_and_refpy_agree_on_renumbered_mesh(kind):
    """amg_test physics, AMG, 2 Picard x 8 FGMRES, two steps: the oracle and
    the numpy restatement read the relabelled mesh the same way."""
    base = _small()
    mesh = renumbered(base, _perm(kind, base.num_cells()))
    cfg = dict(convergence_lag=0, fixed_outer=2, fixed_inner=8)
    o = OracleSolver(mesh, config=default_config(**cfg))
    r = refpy.RefSolver(mesh, **cfg)
    for s in (o, r):
        setup_amg_test(s, mesh, 1)
    for k in range(2):
        o.step()
        r.step()
        _same_step(o, r, f"{kind} step {k}")
    assert o.amg_levels() == r.amg.sizes()
    assert np.abs(o.get_p()).max() > 0.0


def test_assembled_system_invariants_on_renumbered_mesh():
    """tests/fv_checks.py through the oracle on a fully shuffled mesh:
    conservation, closure, face weights, the pressure operator and the diagonal
    inverses do not depend on the cell order."""
    base = _small()
    mesh = renumbered(base, perm_random(base.num_cells()))
    for scheme, time_scheme in ((0, 0), (2, 1)):
        covered = fv.check_assembled(fc.assembled_system(OracleSolver, mesh, scheme, time_scheme, 1.0))
        assert covered["rows"] == mesh.num_cells()
        assert covered["interior"] == int(fv.interior_mask(base).sum()) > 0
