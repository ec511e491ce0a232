"""Passive scalars, host side (no GPU): the ctypes structs against the C
header, the config defaults, the null-handle statuses of the new entries, and
the discretisation of tests/scalar_ref.py itself in float64 on a 1-D row.

A bad field index, a count outside 0..4, a negative diffusivity or tolerance
and check_interval < 1 need a live handle to be told apart from the
null-handle answer; tests/test_gpu_scalar.py checks them."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cfd2_amd import _ffi, scalar_config_default
from cfd2_amd.solver import _bind
from tests import scalar_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "cfd2_amd.h"
#define S(t) printf(#t " size %zu\n", sizeof(t))
#define O(t, f) printf(#t " " #f " %zu\n", offsetof(t, f))
int main(void) {
  S(cfd_scalar_params); O(cfd_scalar_params, diffusivity); O(cfd_scalar_params, inlet_value);
  S(cfd_scalar_config); O(cfd_scalar_config, tol); O(cfd_scalar_config, max_sweeps);
  O(cfd_scalar_config, check_interval); O(cfd_scalar_config, reserved);
  S(cfd_scalar_stats); O(cfd_scalar_stats, sweeps); O(cfd_scalar_stats, converged);
  O(cfd_scalar_stats, last_delta); O(cfd_scalar_stats, dt_used); O(cfd_scalar_stats, min);
  O(cfd_scalar_stats, max); O(cfd_scalar_stats, integral);
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
    want = {}
    for line in out.splitlines():
        t, f, v = line.split()
        want[(t, f)] = int(v)
    types = {"cfd_scalar_params": _ffi.ScalarParams, "cfd_scalar_config": _ffi.ScalarConfig,
             "cfd_scalar_stats": _ffi.ScalarStats}
    seen = 0
    for (t, f), v in want.items():
        got = C.sizeof(types[t]) if f == "size" else getattr(types[t], f).offset
        assert got == v, (t, f)
        seen += 1
    assert seen == 3 + sum(len(t._fields_) for t in types.values())


def test_config_defaults():
    cfg = scalar_config_default()
    assert cfg.tol == np.float32(1e-6)
    assert (cfg.max_sweeps, cfg.check_interval, cfg.reserved) == (200, 4, 0)
    _bind().cfd_scalar_config_default(None)  # a null pointer is ignored


def test_new_entries_are_exported():
    names = ["cfd_scalar_config_default", "cfd_scalars_enable", "cfd_set_scalar_params", "cfd_set_scalar",
             "cfd_get_scalar", "cfd_scalar_advance", "cfd_scalar_stats_get"]
    assert set(names) <= set(_ffi.EXPORTED)
    L = _bind()
    for n in names:
        getattr(L, n)


def test_null_arguments_return_status():
    L = _bind()
    inv = 1  # CFD_ERR_INVALID
    cfg = scalar_config_default()
    par = _ffi.ScalarParams(0.0, 1.0)
    st = _ffi.ScalarStats()
    buf = (C.c_double * 4)()
    calls = [lambda: L.cfd_scalars_enable(None, 1, C.byref(cfg)), lambda: L.cfd_scalars_enable(None, 1, None),
             lambda: L.cfd_scalars_enable(None, 9, None),
             lambda: L.cfd_set_scalar_params(None, 0, C.byref(par)), lambda: L.cfd_set_scalar(None, 0, buf),
             lambda: L.cfd_get_scalar(None, 0, buf), lambda: L.cfd_scalar_advance(None, 1e-3),
             lambda: L.cfd_scalar_stats_get(None, 0, C.byref(st))]
    for call in calls:
        assert call() == inv
        assert b"null solver handle" in L.cfd_last_error()


def _step_profile(n):
    x = (np.arange(n) + 0.5) / n
    return np.where(x < 0.3, 1.0, 0.0)


@pytest.mark.parametrize("D", [0.0, 0.02])
@pytest.mark.parametrize("cfl", [0.4, 3.0])
def test_row_advects_a_step_inside_bounds(cfl, D):
    """float64, 1-D row, uniform flux: a step profile moves downstream, stays in
    [0, 1] (the maximum principle of the bounded form) and is monotone; the
    front sits where the flux carried it."""
    n, flux, vol = 64, 1.0, 1.0
    dt = cfl * vol / flux
    phi = _step_profile(n)
    steps = 8
    for _ in range(steps):
        new = scalar_ref.advance64(n, flux, vol, 1.0, dt, D, 1.0, phi)
        assert new.min() >= -1e-12 and new.max() <= 1.0 + 1e-12
        assert np.all(np.diff(new) <= 1e-12)          # inlet value 1 upstream, no new extrema
        if D == 0.0:
            assert np.all(new >= phi - 1e-12)         # pure advection: the front only moves downstream
        phi = new
    front = np.interp(0.5, phi[::-1], np.arange(n)[::-1] + 0.5)  # where phi crosses 1/2
    assert abs(front - (0.3 * n + steps * cfl)) <= 2.0 + 2.0 * np.sqrt(steps * (cfl + 1 + 2 * D * dt))


@pytest.mark.parametrize("flux", [1.0, -1.0, 0.0])
def test_row_keeps_a_uniform_field(flux):
    """a uniform field equal to the inlet value is a fixed point for either flow direction"""
    n = 32
    phi = np.full(n, 0.37)
    out = scalar_ref.advance64(n, flux, 1.0, 1.3, 0.5, 0.01, 0.37, phi)
    assert np.max(np.abs(out - 0.37)) <= 1e-13


def test_row_restatement_agrees_with_the_float64_operator():
    """ScalarRef (float32, mesh-driven) on a 1-D row of unit cells == advance64 to float32 accuracy"""
    n = 40
    # n unit cells in a row: faces 0..n (face j between cells j-1 and j), plus top / bottom walls
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
    R = scalar_ref.ScalarRef(arrays)
    assert R.S == 4
    flux = np.zeros(len(own), np.float32)
    flux[1:n + 1] = 1.0   # the owner (left cell) loses mass through internal faces and the outlet
    flux[0] = -1.0        # inlet face: owned by cell 0, flux out of it negative
    phi0 = _step_profile(n)
    # the inlet's centre distance is 1/2, a row cell's 1: D = 0 keeps the two operators the same
    got, sweeps, delta, conv = R.advance(flux, 1.0, 0.8, 0.0, 1.0, phi0, tol=1e-7, max_sweeps=400)
    want = scalar_ref.advance64(n, 1.0, 1.0, 1.0, 0.8, 0.0, 1.0, phi0)
    assert conv and sweeps % 4 == 0 and got.dtype == np.float32
    assert np.max(np.abs(got - want)) <= 1e-5
    coef, diag, b = R.assemble(flux, 1.0, 0.8, 0.0, 1.0, phi0)
    assert R.residual64(coef, diag, b, got) <= 1e-7 + 8 * 2.0 ** -24
