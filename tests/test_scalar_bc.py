"""Wall conditions, sources and the wall-flux sums of the passive scalars on the
CPU: the oracle's fluxes and the numpy restatement tests/scalar_bc_ref.py behind
GpuSolver's surface, through the drivers of tests/scalar_bc_cases.py and the
float64 checks of tests/scalar_bc_checks.py; and the proof that those checks
bite (test_checks_catch_wrong_variants).  tests/test_gpu_scalar_bc.py runs the
same drivers on the HIP path, which is bit-identical to the restatement, so
every bound it asserts is first shown to hold here.  Of the library itself this
module checks the host side only: the new ctypes structs against the C header,
the exported names and the null-argument statuses.  The refusals that need a
live handle are tested on the device only."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cfd2_amd import _ffi
from cfd2_amd.solver import _bind
from tests import scalar_bc_cases as bcs
from tests.scalar_bc_ref import ScalarBCRef
from tests.scalar_ref import F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "cfd2_amd.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define O(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void) {
  S(cfd_scalar_wall); O(cfd_scalar_wall, kind); O(cfd_scalar_wall, value); O(cfd_scalar_wall, x0);
  O(cfd_scalar_wall, y0); O(cfd_scalar_wall, x1); O(cfd_scalar_wall, y1);
  S(cfd_scalar_source); O(cfd_scalar_source, rate); O(cfd_scalar_source, reserved); O(cfd_scalar_source, x0);
  O(cfd_scalar_source, y0); O(cfd_scalar_source, x1); O(cfd_scalar_source, y1);
  S(cfd_scalar_wall_flux); O(cfd_scalar_wall_flux, flux); O(cfd_scalar_wall_flux, area);
  O(cfd_scalar_wall_flux, phi_area); O(cfd_scalar_wall_flux, faces); O(cfd_scalar_wall_flux, kind);
  S(cfd_scalar_config); S(cfd_scalar_stats); S(cfd_scalar_params); S(cfd_scalar_solver); S(cfd_scalar_solver_stats);
  S(cfd_scalar_scheme); S(cfd_scalar_scheme_stats);
  return 0;
}
"""


def test_struct_layouts_match_the_header(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc, "no C compiler"
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT_C)
    subprocess.run([cc, "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    new = {"cfd_scalar_wall": _ffi.ScalarWall, "cfd_scalar_source": _ffi.ScalarSource,
           "cfd_scalar_wall_flux": _ffi.ScalarWallFlux}
    types = dict(new, cfd_scalar_config=_ffi.ScalarConfig, cfd_scalar_stats=_ffi.ScalarStats,
                 cfd_scalar_params=_ffi.ScalarParams, cfd_scalar_solver=_ffi.ScalarSolver,
                 cfd_scalar_solver_stats=_ffi.ScalarSolverStats, cfd_scalar_scheme=_ffi.ScalarScheme,
                 cfd_scalar_scheme_stats=_ffi.ScalarSchemeStats)
    seen = 0
    for line in out.splitlines():
        t, f, v = line.split()
        got = C.sizeof(types[t]) if f == "size" else getattr(types[t], f).offset
        assert got == int(v), (t, f)
        seen += 1
    assert seen == len(types) + sum(len(t._fields_) for t in new.values())
    assert [C.sizeof(t) for t in new.values()] == [40, 40, 32]
    # the existing structs keep their layouts
    assert (C.sizeof(_ffi.ScalarConfig), C.sizeof(_ffi.ScalarStats), C.sizeof(_ffi.ScalarParams)) == (16, 40, 8)
    assert (C.sizeof(_ffi.ScalarScheme), C.sizeof(_ffi.ScalarSchemeStats)) == (16, 16)


def test_new_entries_are_exported():
    names = ["cfd_set_scalar_wall", "cfd_set_scalar_source", "cfd_scalar_wall_flux_get"]
    assert set(names) <= set(_ffi.EXPORTED)
    L = _bind()
    for n in names:
        getattr(L, n)
    import cfd2_amd
    for n in ("ScalarWall", "ScalarSource", "ScalarWallFlux"):
        getattr(cfd2_amd, n)
    for n in ("set_scalar_wall", "set_scalar_source", "scalar_wall_flux"):
        getattr(cfd2_amd.GpuSolver, n)


def test_null_arguments_return_status():
    L = _bind()
    wall, source, out = _ffi.ScalarWall(1, 1.0, 0.0, 0.0, 1.0, 1.0), _ffi.ScalarSource(1.0, 0, 0.0, 0.0, 1.0, 1.0), _ffi.ScalarWallFlux()
    n = C.c_uint32()
    for call in (lambda: L.cfd_set_scalar_wall(None, 0, C.byref(wall), C.byref(n)),
                 lambda: L.cfd_set_scalar_wall(None, 0, None, None),
                 lambda: L.cfd_set_scalar_source(None, 0, C.byref(source), C.byref(n)),
                 lambda: L.cfd_set_scalar_source(None, 0, None, None),
                 lambda: L.cfd_scalar_wall_flux_get(None, 0, C.byref(out)),
                 lambda: L.cfd_scalar_wall_flux_get(None, 0, None)):
        assert call() == 1  # CFD_ERR_INVALID
        assert b"null solver handle" in L.cfd_last_error()


@pytest.mark.parametrize("density", bcs.DENSITIES)
@pytest.mark.parametrize("name", bcs.MESHES)
def test_advance_with_walls_and_sources(name, density):
    """Fixed value, fixed flux, fixed value plus a source box, a source alone x
    scheme 0 / 1 under Jacobi and scheme 1 under BiCGStab x 2 advances: the rows
    of the float64 system with the wall and source terms, the float64 direct
    solve, the wall-flux sums and the extended budget."""
    worst = {}
    cover = bcs.run_mesh(bcs.restated_solver(), name, density, worst=worst)
    bcs.check_coverage(name, cover)
    print(name, density, cover, {k: f"{r:.3f} ({w})" for k, (r, w) in worst.items()})


@pytest.mark.parametrize("scheme,method", [(0, 0), (1, 0), (1, 1)])
@pytest.mark.parametrize("value", [0.0, 1.0])
@pytest.mark.parametrize("name", ["rect", "obstacle_perm"])
def test_dye_with_a_fixed_value_wall_stays_in_bounds(name, value, scheme, method):
    bcs.run_bound(bcs.restated_solver(), name, value, scheme, method)


@pytest.mark.parametrize("scheme", [0, 1])
def test_trivial_selections_change_no_bit(scheme):
    bcs.run_noop(bcs.restated_solver(), scheme=scheme)


def test_heated_wall_without_flow():
    bcs.run_physics(bcs.restated_solver())


def test_no_test_mesh_has_a_wall_face_at_slot_31():
    """The refusal of a selected wall face at slot 31 or above cannot be
    provoked on the meshes of tests/scalar_cases.py: the 100-face hub of
    wheel100 has internal faces only."""
    from tests import scalar_cases as cs
    for name in cs.MESHES:
        R = ScalarBCRef(cs.mesh_of(name).arrays(), scheme=0)
        assert not R.wallslot[:, 31:].any(), name


# ---------------------------------------------------------------- wrong variants
class _WallDistanceDoubled(ScalarBCRef):
    def __init__(self, arrays, **kw):
        super().__init__(arrays, **kw)
        self.wall_dist = np.where(self.wallslot, F(2) * self.dist, self.dist).astype(F)


class _FluxWrongSign(ScalarBCRef):
    def flux_term(self, k):
        return -super().flux_term(k)


class _SourceWithoutVolume(ScalarBCRef):
    def source_term(self):
        return np.full(self.N, self.rate, F)


class _ClampWithoutWall(ScalarBCRef):
    range_takes_wall = False


class _GradientWithoutWall(ScalarBCRef):
    grad_takes_wall = False


class _FluxOfOldField(ScalarBCRef):
    def flux_field(self, phi, phi_old):
        return phi_old


JACOBI_0, JACOBI_1 = [(0, 0, 0.01)], [(1, 0, 0.01)]
# variant -> (class, the settings in which it is visible, the cases)
VARIANTS = {
    "the wall distance doubled": (_WallDistanceDoubled, JACOBI_0, ("value",)),
    "the fixed-flux term with the wrong sign": (_FluxWrongSign, JACOBI_0, ("flux",)),
    "the source without vol": (_SourceWithoutVolume, JACOBI_0, ("source",)),
    "the clamp range without the wall value": (_ClampWithoutWall, JACOBI_1, ("value", "value+source")),
    "the gradient's wall face value left at the cell value": (_GradientWithoutWall, JACOBI_1, ("value", "value+source")),
    "the wall flux taken from phi_old": (_FluxOfOldField, JACOBI_0, ("value",)),
}
VARIANT_MESHES = ["rect", "voronoi", "graded"]


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_checks_catch_wrong_variants(variant):
    """Each deliberately wrong restatement, run through the drivers at density
    1000 without the bit comparison, fails a float64 check on at least one mesh
    (the right restatement passes them all: the first test).  The scheme-1
    variants run under scheme 1 only, where the gradient and the clamp exist;
    the wall-flux variant leaves the field right and is caught by the wall-flux
    check or the budget."""
    ref_class, settings, cases = VARIANTS[variant]
    cls = bcs.restated_solver(ref_class)
    caught = []
    for name in VARIANT_MESHES:
        try:
            bcs.run_mesh(cls, name, 1000.0, bit_exact=False, settings=settings, cases=cases)
        except AssertionError as e:
            assert "f64 check_" in str(e), e  # a check's own failure, not the driver's
            caught.append((name, str(e).split(":")[0]))
    print(variant, caught)
    assert caught, f"{variant}: passes every float64 check on {VARIANT_MESHES}"
