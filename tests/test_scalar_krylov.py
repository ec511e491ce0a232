"""The BiCGStab scalar solver, host side (no GPU): the new ctypes structs against
the C header, the defaults, the exported names, the null-handle statuses, and
the restatement tests/scalar_krylov_ref.py on the 1-D row of
tests/test_scalar.py: its accuracy against a float64 direct solve and its
breakdown path.

Bad methods, max_iters < 1, check_interval < 1, a bad field index and scalars
not enabled need a live handle; tests/test_gpu_scalar_krylov.py checks them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np

from cfd2_amd import _ffi, scalar_solver_default
from cfd2_amd.solver import _bind
from tests import scalar_ref
from tests.scalar_krylov_ref import ScalarKrylovRef, breakdown_case, solve64
from tests.test_scalar import _step_profile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "cfd2_amd.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define O(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void) {
  S(cfd_scalar_solver); O(cfd_scalar_solver, method); O(cfd_scalar_solver, max_iters);
  O(cfd_scalar_solver, check_interval); O(cfd_scalar_solver, reserved);
  S(cfd_scalar_solver_stats); O(cfd_scalar_solver_stats, method); O(cfd_scalar_solver_stats, iterations);
  O(cfd_scalar_solver_stats, stop_reason); O(cfd_scalar_solver_stats, polish_sweeps);
  O(cfd_scalar_solver_stats, krylov_residual); O(cfd_scalar_solver_stats, reserved);
  S(cfd_scalar_config); S(cfd_scalar_stats); S(cfd_scalar_params);
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
    types = {"cfd_scalar_solver": _ffi.ScalarSolver, "cfd_scalar_solver_stats": _ffi.ScalarSolverStats,
             "cfd_scalar_config": _ffi.ScalarConfig, "cfd_scalar_stats": _ffi.ScalarStats,
             "cfd_scalar_params": _ffi.ScalarParams}
    seen = 0
    for line in out.splitlines():
        t, f, v = line.split()
        got = C.sizeof(types[t]) if f == "size" else getattr(types[t], f).offset
        assert got == int(v), (t, f)
        seen += 1
    assert seen == 5 + len(_ffi.ScalarSolver._fields_) + len(_ffi.ScalarSolverStats._fields_)
    # the existing structs keep their layouts
    assert (C.sizeof(_ffi.ScalarConfig), C.sizeof(_ffi.ScalarStats), C.sizeof(_ffi.ScalarParams)) == (16, 40, 8)


def test_solver_defaults():
    cfg = scalar_solver_default()
    assert (cfg.method, cfg.max_iters, cfg.check_interval, cfg.reserved) == (0, 500, 8, 0)
    _bind().cfd_scalar_solver_default(None)  # a null pointer is ignored


def test_new_entries_are_exported():
    names = ["cfd_scalar_solver_default", "cfd_set_scalar_solver", "cfd_scalar_solver_stats_get"]
    assert set(names) <= set(_ffi.EXPORTED)
    L = _bind()
    for n in names:
        getattr(L, n)


def test_null_arguments_return_status():
    L = _bind()
    cfg = scalar_solver_default()
    st = _ffi.ScalarSolverStats()
    for call in (lambda: L.cfd_set_scalar_solver(None, 0, C.byref(cfg)), lambda: L.cfd_set_scalar_solver(None, 0, None),
                 lambda: L.cfd_scalar_solver_stats_get(None, 0, C.byref(st)),
                 lambda: L.cfd_scalar_solver_stats_get(None, 0, None)):
        assert call() == 1  # CFD_ERR_INVALID
        assert b"null solver handle" in L.cfd_last_error()


def row(n):
    """the row of test_row_restatement_agrees_with_the_float64_operator: n unit
    cells, unit flux left to right, inlet left, outlet right, walls above and below"""
    own, nb, bnd, fx, fy, area = [], [], [], [], [], []
    for j in range(n + 1):
        if j == 0:
            own.append(0), nb.append(scalar_ref.NONE), bnd.append(1)
        elif j == n:
            own.append(n - 1), nb.append(scalar_ref.NONE), bnd.append(2)
        else:
            own.append(j - 1), nb.append(j), bnd.append(0)
        fx.append(float(j)), fy.append(0.5), area.append(1.0)
    for i in range(n):
        for y in (0.0, 1.0):
            own.append(i), nb.append(scalar_ref.NONE), bnd.append(3)
            fx.append(i + 0.5), fy.append(y), area.append(1.0)
    cells = [[i, i + 1, n + 1 + 2 * i, n + 2 + 2 * i] for i in range(n)]
    arrays = dict(face_owner=np.array(own, np.uint32), face_neighbor=np.array(nb, np.uint32),
                  face_boundary=np.array(bnd, np.uint32), face_area=np.array(area), face_cx=np.array(fx),
                  face_cy=np.array(fy), cell_cx=np.arange(n) + 0.5, cell_cy=np.full(n, 0.5), cell_vol=np.ones(n),
                  cell_face_offsets=np.arange(0, 4 * n + 1, 4, dtype=np.uint32),
                  cell_faces=np.array(cells, np.uint32).reshape(-1))
    flux = np.zeros(len(own), np.float32)
    flux[1:n + 1] = 1.0
    flux[0] = -1.0
    return ScalarKrylovRef(arrays), flux


ROW_N, ROW_DT = 40, 0.8  # as the test the row comes from


def _errors(R, flux, D, dt):
    phi0 = _step_profile(ROW_N)
    coef, diag, b = R.assemble(flux, 1.0, dt, D, 1.0, phi0)
    exact = solve64(R, coef, diag, b)
    k = R.advance_krylov(flux, 1.0, dt, D, 1.0, phi0)
    j, sweeps, _, conv = R.advance(flux, 1.0, dt, D, 1.0, phi0, max_sweeps=100000)
    assert conv
    return k, float(np.abs(k.phi - exact).max()), sweeps, float(np.abs(j - exact).max())


def test_row_accuracy_against_the_float64_solve():
    """D = 0.02, the D > 0 of tests/test_scalar.py's row tests, at that row's dt
    = 0.8 and the default tol 1e-6: BiCGStab stops with reason 1 after 8
    iterations, 4 polish sweeps; its error against the float64 direct solve of
    the same f32-coefficient system is 5.80e-08, converged Jacobi's (20 sweeps)
    5.80e-08.

    Printed, not asserted: on this 1-D row with a step profile the order turns
    round when diffusion dominates (D = 5, dt = 8: BiCGStab 35 iterations,
    2.2e-05, Jacobi 700 sweeps, 4.5e-06; D = 50, dt = 8: 49 iterations, 3.0e-04,
    against 4,384 sweeps, 2.0e-05): both stop on the same update size, and what
    f32 BiCGStab leaves is not confined to the modes Jacobi damps slowly."""
    R, flux = row(ROW_N)
    k, ek, sweeps, ej = _errors(R, flux, 0.02, ROW_DT)
    print(f"D 0.02 dt 0.8: bicgstab {k.iterations} it + {k.polish_sweeps} sweeps err {ek:.3e}; jacobi {sweeps} sweeps err {ej:.3e}")
    assert k.converged and k.stop_reason == 1 and k.phi.dtype == np.float32
    assert ek <= ej
    for D, dt in ((5.0, 8.0), (50.0, 8.0)):
        k2, ek2, sw2, ej2 = _errors(R, flux, D, dt)
        print(f"D {D} dt {dt}: bicgstab {k2.iterations} it + {k2.polish_sweeps} sweeps err {ek2:.3e}; jacobi {sw2} sweeps err {ej2:.3e}")
        assert k2.converged


def test_row_pure_upwind_breaks_down():
    """D = 0 on the row: the matrix is lower bidiagonal and iteration 2 meets a
    zero denominator: reason 2, every value is finite and the polish (16
    sweeps) ends converged."""
    R, flux = row(ROW_N)
    k = R.advance_krylov(flux, 1.0, ROW_DT, 0.0, 1.0, _step_profile(ROW_N))
    print(f"iterations {k.iterations} reason {k.stop_reason} residual {k.krylov_residual:.3e} polish {k.polish_sweeps}")
    assert (k.stop_reason, k.iterations) == (2, 2)
    assert np.isfinite(k.x).all() and np.isfinite(k.phi).all()
    assert k.converged and k.polish_sweeps % 4 == 0
    assert not np.array_equal(k.x, _step_profile(ROW_N).astype(np.float32))  # the Krylov phase did move x


def test_channel_pure_upwind_breaks_down():
    """The breakdown case the device runs too (tests/test_gpu_scalar_krylov.py
    check 4): the 28-cell rectangular channel of tests/test_gpu_scalar.py, u =
    (1, 0), D = 0, dt = 0.2, the fluxes from the CPU oracle: reason 2 in
    iteration 2, finite, 8 polish sweeps, converged."""
    from cfd2_amd.mesh import RectangularChannel, generate_cut_cell_mesh
    from tests.oracle_py import OracleSolver
    mesh = generate_cut_cell_mesh(RectangularChannel(length=1.0, height=0.5), 0.15, 0.15, 1.2, (1.0, 0.5))
    u, phi0, D, inlet, dt = breakdown_case(mesh)
    s = OracleSolver(mesh)
    s.set_density(1.0)
    s.set_u(u)
    s.debug_prepare_assemble(False)
    R = ScalarKrylovRef(mesh.arrays())
    k = R.advance_krylov(s.debug_buffer(0), 1.0, dt, D, inlet, phi0)
    print(f"iterations {k.iterations} reason {k.stop_reason} residual {k.krylov_residual:.3e} polish {k.polish_sweeps}")
    assert (k.stop_reason, k.iterations) == (2, 2)
    assert np.isfinite(k.x).all() and np.isfinite(k.phi).all() and k.converged
