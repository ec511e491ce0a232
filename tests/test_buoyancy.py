"""Boussinesq buoyancy on the CPU: the restatement tests/buoyancy_ref.py against
itself and against the maths (include/cfd2_amd.h "Arithmetic of buoyancy").
The GPU test tests/test_gpu_buoyancy.py holds the HIP path to the same checks.

The plume case as the restatement runs it (tests/buoyancy_cases.py PLUME, K = 4,
fixed 3 Picard x 10 FGMRES): mean v over the box above the obstacle 2.6e-3 with
g = (0, -9.81) and -2.3e-3 with g = (0, +9.81), max |u| 0.11; the body force
on the fluid +/- 0.396.
"""
import numpy as np
import pytest

from tests import buoyancy_cases as bc
from tests import refpy
from tests.buoyancy_ref import BuoyantRefSolver, check_rhs, term64

F = np.float32
PLUME_FIXED = dict(fixed_outer=3, fixed_inner=10)


def _solver(name, cls=BuoyantRefSolver, **cfg):
    return cls(bc.mesh_of(name), M=bc.refmesh_of(name), **cfg)


def _same_state(a, b, ctx):
    for g in ("get_u", "get_p", "get_d_p"):
        assert np.array_equal(getattr(a, g)(), getattr(b, g)()), (ctx, g)
    assert a.info == b.info, ctx


@pytest.mark.parametrize("off", ["beta", "g"])
def test_off_reproduces_refsolver(off):
    """check 1: beta = 0 or g = (0, 0): refpy.RefSolver bit for bit, and the rhs object itself"""
    mesh = bc.mesh_of("obstacle")
    r = refpy.RefSolver(mesh, **bc.FIXED)
    b = _solver("obstacle", **bc.FIXED)
    for s in (r, b):
        bc.setup_flow(s, mesh, time_scheme=1, scheme=2)
    bc.setup_scalars(b, mesh)
    if off == "beta":
        b.set_scalar_buoyancy(0, 0.0, bc.REF)
    else:
        b.set_gravity(0.0, 0.0)
    assert not b.buoyancy()["active"]
    rhs = np.arange(3 * mesh.num_cells(), dtype=F)
    assert b.add_buoyancy(rhs) is rhs
    for k in range(2):
        r.step()
        b.step()
        b.advance_scalars()
        _same_state(r, b, f"{off} step {k}")
    assert refpy.assemble.__module__ == "tests.refpy"  # the wrapper is gone after step()
    assert b.buoyancy_force()[:2] == (0.0, 0.0)


def _identity(s, name, two):
    mesh = bc.mesh_of(name)
    bc.setup_flow(s, mesh, scheme=2)
    bc.setup_scalars(s, mesh, two=two)
    on, off = s.debug_rhs()
    b = s.buoyancy()
    vol = mesh.arrays()["cell_vol"].astype(F).astype(np.float64)
    phis = [s.get_scalar(f) for f in range(len(b["beta"]))]
    t64, mag = term64(vol, float(s.constants.density), b["beta"], b["ref"], phis, b["g"])
    assert np.abs(t64).max() > 0
    return check_rhs(on, off, t64, mag, name)


@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("name", bc.MESHES + bc.STRIPS)
def test_float64_identity(name, two):
    """check 2: |rhs_on - rhs_off - t64| <= 8 eps32 (|rhs_on| + vol rho sum |beta| (|phi| + |ref|) |g_c|)
    per cell and component; rhs_p untouched.  8: the term takes at most five
    float32 roundings, the final subtraction one (two fields: one more each)."""
    ratio = _identity(_solver(name), name, two)
    print(f"{name} two={two}: worst error / bound {ratio:.3f}")


class _FlippedG(BuoyantRefSolver):
    def gravity(self):
        return (-self.g[0], -self.g[1])


class _NoDensity(BuoyantRefSolver):
    def density(self):
        return F(1)


class _NoRef(BuoyantRefSolver):
    def reference(self, f):
        return F(0)


@pytest.mark.parametrize("cls", [_FlippedG, _NoDensity, _NoRef])
def test_wrong_restatements_fail_the_identity(cls):
    """check 3: the sign of g flipped, the density dropped, ref ignored: check 2 catches each"""
    with pytest.raises(AssertionError, match="worst error / bound"):
        _identity(_solver("obstacle", cls=cls), "obstacle", False)


def test_body_force():
    """the restatement's force: a uniform field gives -rho beta (phi - ref) g times the
    canonical volume sum, exactly when every factor is a power of two"""
    mesh = bc.mesh_of("obstacle")
    s = _solver("obstacle")
    s.set_density(2.0)
    s.enable_scalars(1)
    s.set_scalar(0, np.full(mesh.num_cells(), 0.75))
    s.set_scalar_buoyancy(0, 0.5, 0.25)
    s.set_gravity(0.25, -8.0)
    vsum = float(refpy.canon_sum(mesh.arrays()["cell_vol"].astype(F).astype(np.float64)))
    assert s.buoyancy_force() == (-2.0 * 0.5 * 0.5 * 0.25 * vsum, 2.0 * 0.5 * 0.5 * 8.0 * vsum, 1)


def test_plume_rises():
    """check 4: at rest with beta = 0; with buoyancy the fluid above the heated
    obstacle rises, and sinks under g = (0, +9.81); the body force points the same way"""
    mesh = bc.mesh_of("obstacle")
    p = bc.PLUME
    rest = _solver("obstacle", **PLUME_FIXED)
    v0, umax0 = bc.run_plume(rest, mesh, 0.0, p["g"])
    assert (v0, umax0) == (0.0, 0.0)
    assert rest.get_scalar(0).max() > 0.0  # the wall did heat the fluid
    up = _solver("obstacle", **PLUME_FIXED)
    v_up, umax = bc.run_plume(up, mesh, p["beta"], p["g"])
    down = _solver("obstacle", **PLUME_FIXED)
    v_down, _ = bc.run_plume(down, mesh, p["beta"], (0.0, 9.81))
    f_up, f_down = up.buoyancy_force(), down.buoyancy_force()
    print(f"plume: mean v above {v_up:.3e} (g down) {v_down:.3e} (g up), max |u| {umax:.3e}, force {f_up} {f_down}")
    assert v_up > 0.0 and f_up[1] > 0.0
    assert v_down < 0.0 and f_down[1] < 0.0
