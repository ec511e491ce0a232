"""Flow diagnostics, host side (no GPU): the adaptive time-step rule against a
restatement of the reference's driver loop (src/ui/app.rs:897-909), and the
argument checks of the new C entries."""
import ctypes as C
import math

import pytest

from cfd2_amd import _ffi, adaptive_dt_rule
from cfd2_amd.solver import _bind


def ref_rule(current_dt, target_cfl, min_cell_size, max_vel):
    """app.rs:897-909, statement by statement (Python floats are f64)."""
    if max_vel > 1e-6:
        next_dt = target_cfl * min_cell_size / max_vel
        if next_dt > current_dt * 1.2:
            next_dt = current_dt * 1.2
        next_dt = min(max(next_dt, 1e-9), 100.0)  # f64::clamp
        return next_dt, True
    return current_dt, False


RULE_TABLE = [
    # (current_dt, target_cfl, min_cell_size, max_vel)           branch
    (1e-4, 0.9, 0.05, 0.0),        # max_vel <= 1e-6: no change
    (1e-4, 0.9, 0.05, 1e-6),       # the bound itself: no change (strict >)
    (1e-4, 0.9, 0.05, 9.99e-7),
    (1e-3, 0.9, 0.01, 12.5),       # CFL-limited: 7.2e-4 < 1.2e-3
    (float(C.c_float(1.7e-4).value), 0.35, 0.0123456789, 1.2345678),  # CFL-limited, inexact operands
    (1e-4, 0.9, 0.05, 1.0),        # the 1.2x cap: 0.045 > 1.2e-4
    (float(C.c_float(1e-4).value), 0.9, 0.05, 1.000001e-6),  # cap, max_vel just above the bound
    (1e-12, 0.9, 0.05, 1.0),       # cap, then the lower clamp: 1.2e-12 -> 1e-9
    (1e-4, 1e-9, 1e-3, 10.0),      # CFL-limited below the lower clamp: 1e-13 -> 1e-9
    (90.0, 0.9, 1e4, 1e-3),        # cap 108 -> the upper clamp 100
    (1e3, 0.9, 1.0, 2e-3),         # CFL-limited 450 -> the upper clamp 100
]


@pytest.mark.parametrize("cur,cfl,h,vmax", RULE_TABLE)
def test_adaptive_dt_rule_matches_reference(cur, cfl, h, vmax):
    want, want_changed = ref_rule(cur, cfl, h, vmax)
    got, changed = adaptive_dt_rule(cur, cfl, h, vmax)
    assert changed == want_changed
    assert got == want and math.copysign(1.0, got) == math.copysign(1.0, want)


def test_rule_table_hits_every_branch():
    """the table above takes: no change, CFL-limited, the cap, both clamp ends"""
    seen = set()
    for cur, cfl, h, vmax in RULE_TABLE:
        if not vmax > 1e-6:
            seen.add("none")
            continue
        raw = cfl * h / vmax
        capped = raw > cur * 1.2
        seen.add("cap" if capped else "cfl")
        v = cur * 1.2 if capped else raw
        if v < 1e-9:
            seen.add("lo")
        if v > 100.0:
            seen.add("hi")
    assert seen == {"none", "cfl", "cap", "lo", "hi"}


def test_flow_diag_struct_layout():
    """cfd_flow_diag: 9 doubles + 2 uint32 = 80 bytes, no padding"""
    assert C.sizeof(_ffi.FlowDiag) == 80
    assert _ffi.FlowDiag.region_faces.offset == 72


def test_null_arguments_return_status():
    L = _bind()
    d = _ffi.FlowDiag()
    out = (C.c_double * 4)()
    n = C.c_uint32()
    dt = C.c_float()
    nxt, ch = C.c_double(), C.c_int32()
    inv = 1  # CFD_ERR_INVALID
    assert L.cfd_flow_diagnostics(None, C.byref(d)) == inv
    assert b"null" in L.cfd_last_error()
    assert L.cfd_get_derived(None, 1, out) == inv
    assert L.cfd_set_force_region(None, 0.0, 0.0, 1.0, 1.0, C.byref(n)) == inv
    assert L.cfd_adapt_dt(None, 0.9, C.byref(dt)) == inv
    assert L.cfd_min_cell_size(None) == 0.0
    assert L.cfd_adaptive_dt_rule(1e-4, 0.9, 0.05, 1.0, None, C.byref(ch)) == inv
    assert L.cfd_adaptive_dt_rule(1e-4, 0.9, 0.05, 1.0, C.byref(nxt), None) == inv
    assert L.cfd_group_flow_diagnostics(None, 2, C.byref(d)) == inv
    assert L.cfd_group_adapt_dt(None, 2, 0.9, C.byref(dt)) == inv
    harr = (C.c_void_p * 2)()  # two null handles
    assert L.cfd_group_flow_diagnostics(harr, 2, C.byref(d)) == inv
    assert L.cfd_group_flow_diagnostics(harr, 2, None) == inv
    assert L.cfd_group_adapt_dt(harr, 2, 0.9, None) == inv
    assert L.cfd_group_adapt_dt(harr, 0, 0.9, C.byref(dt)) == inv
