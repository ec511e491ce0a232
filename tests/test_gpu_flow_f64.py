"""The float64 flow checks of tests/test_flow_f64.py on the HIP path: the same
case list (tests/flow_cases.py), the same checks (tests/flow_checks.py), the
same derived bounds -- k_prepare, k_assemble, k_assemble_buoyant and
k_update_fields against the discretisation itself.  The buoyant right-hand side
is checked here alone: the oracle has no scalar fields."""
import pytest

from cfd2_amd import GpuSolver
from tests import flow_cases as cs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("density", cs.DENSITIES)
@pytest.mark.parametrize("name", cs.MESHES)
def test_flow_stages_satisfy_the_float64_formulas_gpu(name, density):
    worst = {}
    cover = cs.run_mesh(GpuSolver, name, density, worst)
    print(name, density, cover, {k: f"{r:.3f} ({w})" for k, (r, w) in worst.items()})


def test_block_remapping_has_quotient_and_remainder_gpu():
    big = cs.mesh_of("channel13")
    assert cs.blocks(big) >= 9 and cs.blocks(big) % 8 != 0, cs.blocks(big)


@pytest.mark.parametrize("name", cs.UPDATE_MESHES)
def test_update_and_max_difference_fold_gpu(name):
    cs.run_update(GpuSolver, name)


@pytest.mark.parametrize("name", cs.BUOYANT_MESHES)
def test_buoyant_right_hand_side_gpu(name):
    """Two driving fields with non-zero beta, g = (0.3, -9.81): every row of
    the right-hand side to its bound, and it differs from the non-buoyant one."""
    out = cs.run_buoyant(GpuSolver, name)
    print(name, {k: f"{r['worst']:.3f}" for k, r in out.items()})
