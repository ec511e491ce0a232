"""Scheme 1 of the passive scalars (limited linear, van Leer), host side (no
GPU): the new ctypes structs against the C header, the default, the exported
names, the null-handle statuses, and the restatement tests/scalar_hr_ref.py on
the 1-D row in float64: the front it keeps, its bound, and what the bound is
worth without the clamp.

A bad scheme, a bad field index, scalars not enabled and a distributed handle
need a live handle; tests/test_gpu_scalar_hr.py checks them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cfd2_amd import _ffi, scalar_scheme_default
from cfd2_amd.solver import _bind
from tests import scalar_ref
from tests.scalar_hr_ref import ScalarHRRef, advance64_hr, row_arrays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "cfd2_amd.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define O(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void) {
  S(cfd_scalar_scheme); O(cfd_scalar_scheme, scheme); O(cfd_scalar_scheme, reserved);
  S(cfd_scalar_scheme_stats); O(cfd_scalar_scheme_stats, scheme); O(cfd_scalar_scheme_stats, clamped_cells);
  O(cfd_scalar_scheme_stats, reserved);
  S(cfd_scalar_config); S(cfd_scalar_stats); S(cfd_scalar_params); S(cfd_scalar_solver); S(cfd_scalar_solver_stats);
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
    types = {"cfd_scalar_scheme": _ffi.ScalarScheme, "cfd_scalar_scheme_stats": _ffi.ScalarSchemeStats,
             "cfd_scalar_config": _ffi.ScalarConfig, "cfd_scalar_stats": _ffi.ScalarStats,
             "cfd_scalar_params": _ffi.ScalarParams, "cfd_scalar_solver": _ffi.ScalarSolver,
             "cfd_scalar_solver_stats": _ffi.ScalarSolverStats}
    seen = 0
    for line in out.splitlines():
        t, f, v = line.split()
        got = C.sizeof(types[t]) if f == "size" else getattr(types[t], f).offset
        assert got == int(v), (t, f)
        seen += 1
    assert seen == 7 + len(_ffi.ScalarScheme._fields_) + len(_ffi.ScalarSchemeStats._fields_)
    assert (C.sizeof(_ffi.ScalarScheme), C.sizeof(_ffi.ScalarSchemeStats)) == (16, 16)
    # the existing structs keep their layouts
    assert (C.sizeof(_ffi.ScalarConfig), C.sizeof(_ffi.ScalarStats), C.sizeof(_ffi.ScalarParams)) == (16, 40, 8)


def test_scheme_default():
    cfg = scalar_scheme_default()
    assert cfg.scheme == 0 and list(cfg.reserved) == [0, 0, 0]
    dirty = _ffi.ScalarScheme(7, (C.c_int32 * 3)(1, 2, 3))
    _bind().cfd_scalar_scheme_default(C.byref(dirty))
    assert dirty.scheme == 0 and list(dirty.reserved) == [0, 0, 0]
    _bind().cfd_scalar_scheme_default(None)  # a null pointer is ignored


def test_new_entries_are_exported():
    names = ["cfd_scalar_scheme_default", "cfd_set_scalar_scheme", "cfd_scalar_scheme_stats_get"]
    assert set(names) <= set(_ffi.EXPORTED)
    L = _bind()
    for n in names:
        getattr(L, n)
    import cfd2_amd
    for n in ("scalar_scheme_default", "ScalarScheme", "ScalarSchemeStats"):
        getattr(cfd2_amd, n)
    for n in ("set_scalar_scheme", "scalar_scheme_stats"):
        getattr(cfd2_amd.GpuSolver, n)


def test_null_arguments_return_status():
    L = _bind()
    cfg = scalar_scheme_default()
    st = _ffi.ScalarSchemeStats()
    for call in (lambda: L.cfd_set_scalar_scheme(None, 0, C.byref(cfg)), lambda: L.cfd_set_scalar_scheme(None, 0, None),
                 lambda: L.cfd_scalar_scheme_stats_get(None, 0, C.byref(st)),
                 lambda: L.cfd_scalar_scheme_stats_get(None, 0, None)):
        assert call() == 1  # CFD_ERR_INVALID
        assert b"null solver handle" in L.cfd_last_error()


ROW_N = 80


def _front(cfl, scheme, clamp=True):
    """the row of the design sketch: 80 unit cells, unit flux, inlet 1, phi = 0 at
    the start, D = 0, round(30 / CFL) implicit steps: (phi, largest value seen,
    smallest value seen)"""
    phi = np.zeros(ROW_N)
    hi, lo = 0.0, 0.0
    for _ in range(int(round(30 / cfl))):
        if scheme == 0:
            phi = scalar_ref.advance64(ROW_N, 1.0, 1.0, 1.0, cfl, 0.0, 1.0, phi)
        else:
            phi, _ = advance64_hr(ROW_N, 1.0, 1.0, 1.0, cfl, 0.0, 1.0, phi, clamp=clamp)
        hi, lo = max(hi, float(phi.max())), min(lo, float(phi.min()))
    return phi, hi, lo


def _width(phi):
    return int(np.count_nonzero((phi > 0.05) & (phi < 0.95)))


def test_row_front_is_sharper_and_bounded():
    """float64, 1-D row, the front after it travelled 30 cells.  Cells with 0.05 <
    phi < 0.95, upwind / scheme 1, as restated: CFL 0.25: 20 / 10, CFL 0.9: 25 /
    17, CFL 2: 31 / 26.  With the clamp nothing leaves [0, 1] (overshoot 0.0 at
    all three); without it the maximum exceeds 1 by 3.2e-3 at CFL 0.9 and by
    5.9e-3 at CFL 2, so the bound is the clamp's doing."""
    for cfl in (0.25, 0.9, 2.0):
        up, _, _ = _front(cfl, 0)
        hr, hi, lo = _front(cfl, 1)
        wu, wh = _width(up), _width(hr)
        print(f"CFL {cfl}: width upwind {wu} scheme 1 {wh}; max - 1 {hi - 1:.3e} min {lo:.3e}")
        assert wh < wu, cfl
        if cfl == 0.25:
            assert wh <= 0.7 * wu
        assert lo >= -1e-12 and hi <= 1.0 + 1e-12, cfl
    _, hi, _ = _front(0.9, 1, clamp=False)
    print(f"CFL 0.9 without the clamp: max - 1 {hi - 1:.3e}")
    assert hi - 1.0 > 1e-3


@pytest.mark.parametrize("cfl", [0.25, 0.9])
def test_row_smooth_profile_is_more_accurate(cfl):
    """a sine bump (0.5 (1 - cos) over 20 cells, inlet 0) carried 30 cells: the
    maximum and the mean error against the exact shifted profile are smaller
    under scheme 1 (restated: CFL 0.25 max 0.220 against 0.440, CFL 0.9 0.399
    against 0.520; what is left is implicit Euler's own diffusion)"""
    x = np.arange(ROW_N) + 0.5

    def bump(x0):
        s = (x - x0) / 20.0
        return np.where((s > 0) & (s < 1), 0.5 * (1 - np.cos(2 * np.pi * s)), 0.0)

    steps = int(round(30 / cfl))
    up, hr = bump(5.0), bump(5.0)
    for _ in range(steps):
        up = scalar_ref.advance64(ROW_N, 1.0, 1.0, 1.0, cfl, 0.0, 0.0, up)
        hr, _ = advance64_hr(ROW_N, 1.0, 1.0, 1.0, cfl, 0.0, 0.0, hr)
    exact = bump(5.0 + steps * cfl)
    eu, eh = np.abs(up - exact), np.abs(hr - exact)
    print(f"CFL {cfl}: max error upwind {eu.max():.3e} scheme 1 {eh.max():.3e}; mean {eu.mean():.3e} {eh.mean():.3e}")
    assert eh.max() < eu.max() and eh.mean() < eu.mean()
    assert hr.min() >= -1e-12 and hr.max() <= 1.0 + 1e-12


def test_row_restatement_agrees_with_the_float64_row():
    """ScalarHRRef (float32, mesh-driven: gradient, lambda, normals, slot order) on
    the row of unit cells == advance64_hr to float32 accuracy, over steps in
    which the clamp does and does not act; scheme 0 of the same class keeps
    ScalarRef's bits"""
    n, dt = 40, 0.8
    arrays, flux = row_arrays(n)
    R = ScalarHRRef(arrays)
    assert R.S == 4 and not R.degen.any() and np.all(R.lam[R.internal] == 0.5)
    phi32 = np.where((np.arange(n) + 0.5) / n < 0.3, 1.0, 0.0).astype(np.float32)
    phi64 = phi32.astype(np.float64)
    clamps = []
    for _ in range(6):
        phi32, sweeps, _, conv = R.advance(flux, 1.0, dt, 0.0, 1.0, phi32, tol=1e-7, max_sweeps=400)
        clamps.append(R.clamped)
        phi64, c64 = advance64_hr(n, 1.0, 1.0, 1.0, dt, 0.0, 1.0, phi64)
        assert conv and phi32.dtype == np.float32
        assert np.max(np.abs(phi32 - phi64)) <= 2e-5
    print("clamped cells per step", clamps)
    assert any(clamps)
    R0, base = ScalarHRRef(arrays, scheme=0), scalar_ref.ScalarRef(arrays)
    for got, want in zip(R0.assemble(flux, 1.0, dt, 0.01, 1.0, phi32), base.assemble(flux, 1.0, dt, 0.01, 1.0, phi32)):
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # coef and diag are scheme 0's under scheme 1 too; only b moves
    c1, d1, b1 = R.assemble(flux, 1.0, dt, 0.01, 1.0, phi32)
    c0, d0, b0 = base.assemble(flux, 1.0, dt, 0.01, 1.0, phi32)
    assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32)) and np.array_equal(d1.view(np.uint32), d0.view(np.uint32))
    assert not np.array_equal(b1, b0)


def test_constant_field_keeps_scheme_zero_bits():
    """a constant field has no face differences: h = 0 on every slot, b keeps
    scheme 0's bits whatever the inlet value, and nothing is clamped"""
    arrays, flux = row_arrays(24)
    R, base = ScalarHRRef(arrays), scalar_ref.ScalarRef(arrays)
    phi = np.full(24, 0.37, np.float32)
    for inlet in (0.37, 1.0):
        b1 = R.assemble(flux, 1.3, 0.5, 0.01, inlet, phi)[2]
        b0 = base.assemble(flux, 1.3, 0.5, 0.01, inlet, phi)[2]
        assert np.array_equal(b1.view(np.uint32), b0.view(np.uint32)) and R.clamped == 0
