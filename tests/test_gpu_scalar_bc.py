"""Wall conditions, sources and the wall-flux sums of the passive scalars on the
HIP path (csrc/hip/scalar.hip: the boundary-condition forms of the assemblies
and the gradient, k_scalar_wall_flux): the drivers of tests/scalar_bc_cases.py,
which tests/test_scalar_bc.py runs on the CPU, with GpuSolver.  Per advance: bit
equality with tests/scalar_bc_ref.py (field, sweeps, last_delta, clamped_cells,
the three wall-flux doubles, the face and cell counts), then the float64 checks
of tests/scalar_bc_checks.py: rows, direct solve, wall-flux sums and the
extended budget, which ties cfd_scalar_wall_flux_get to the advance."""
import pytest

from cfd2_amd import GpuGroup, GpuSolver
from tests import scalar_bc_cases as bcs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("density", bcs.DENSITIES)
@pytest.mark.parametrize("name", bcs.MESHES)
def test_advance_with_walls_and_sources(name, density):
    """Fixed value, fixed flux, fixed value plus a source box, a source alone x
    scheme 0 / 1 under Jacobi and scheme 1 under BiCGStab x 2 advances on one
    handle.  fine_perm: more than four 1,024-cell blocks, most of them without
    a selected cell, so the wall-flux tree crosses blocks of +0."""
    cover = bcs.run_mesh(GpuSolver, name, density)
    bcs.check_coverage(name, cover)
    print(name, density, cover)


@pytest.mark.parametrize("scheme,method", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("value", [0.0, 1.0])
@pytest.mark.parametrize("name", ["rect", "obstacle_perm"])
def test_dye_with_a_fixed_value_wall_stays_in_bounds(name, value, scheme, method):
    bcs.run_bound(GpuSolver, name, value, scheme, method)


@pytest.mark.parametrize("scheme", [0, 1])
def test_trivial_selections_change_no_bit(scheme):
    bcs.run_noop(GpuSolver, scheme=scheme)


def test_heated_wall_without_flow():
    bcs.run_physics(GpuSolver)


def test_refusals_and_bad_arguments():
    bcs.run_refusals(GpuSolver, GpuGroup)
