"""Float64 checks of passive scalar transport (tests/scalar_checks.py) on the
HIP path (csrc/hip/scalar.hip): the case list and drivers of
tests/scalar_cases.py, which tests/test_scalar_f64.py runs on the CPU, with
GpuSolver.  Per advance: bit equality with the matching numpy restatement (at
density 1000 too, on the strips, the 100-face wheel and the renumbered meshes),
the rows of the float64 system, the float64 direct solve, and the integral's
budget, which ties cfd_scalar_stats.integral (k_scalar_stats) to the advance."""
import pytest

from cfd2_amd import GpuSolver
from tests import scalar_cases as cs

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("density", cs.DENSITIES)
@pytest.mark.parametrize("name", cs.MESHES)
def test_advance_satisfies_the_float64_equations(name, density):
    """Scheme 0 / 1 x Jacobi (D = 0, 0.01) and BiCGStab (D = 0.05, `converged`
    asserted) x smooth / step field x 2 advances on one handle.  The device's
    clamped_cells is compared with the restatement's count (bit-exact), not
    with the float64 reference's: borderline cells may differ there."""
    cover = cs.run_mesh(GpuSolver, name, density)
    cs.check_coverage(name, cover)
    print(name, density, cover)


def test_scheme_one_is_refused_above_32_faces():
    """wheel100: set_scalar_scheme(0, "vanleer") is CFD_ERR_INVALID ("more than
    32 faces per cell"), and the handle advances under scheme 0 afterwards with
    the restatement's bits."""
    cs.run_wide_refusal(GpuSolver)
