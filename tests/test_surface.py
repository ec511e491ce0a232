"""Wall surface distributions on the CPU: the numpy restatement
tests/surface_ref.py against the float64 checks tests/surface_checks.py on
states the CPU oracle solved, the deliberately wrong conventions the checks must
reject, the post-processing of cfd2_amd/surface.py, and the C ABI's symbols.
tests/test_gpu_surface.py holds the HIP path to the same restatement and checks.
"""
import os
import re

import numpy as np
import pytest

from cfd2_amd import _ffi
from cfd2_amd import surface as post
from cfd2_amd.solver import _bind
from tests import surface_checks as ck
from tests.bcvel_ref import BoundaryVelocities
from tests.meshes import channel_obstacle
from tests.oracle_py import OracleSolver
from tests.refpy import Constants, _smoothstep
from tests.surface_ref import SurfaceRef, SurfaceStats
from tests.synthetic import strip

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BODY = (0.7, 0.2, 1.3, 0.8)  # the obstacle of channel_obstacle
NU = 0.01


@pytest.fixture(scope="module")
def solved():
    """(mesh, u, p) float32 after 2 oracle steps past the obstacle: computed once, shared, never modified"""
    mesh = channel_obstacle(h=0.1, smooth_iters=20)
    o = OracleSolver(mesh)
    o.set_dt(0.001)
    o.set_viscosity(NU)
    o.set_inlet_velocity(1.0)
    o.set_precond_type(1)
    o.initialize_history()
    for _ in range(2):
        o.step()
    u, p = o.get_u().astype(F), o.get_p().astype(F)
    u.setflags(write=False), p.setflags(write=False)
    return mesh, u, p


def _fields(n, seed=3):
    rng = np.random.default_rng(seed)
    return [dict(phi=rng.standard_normal(n).astype(F), diffusivity=0.02, wall=(1, 1.5, BODY)),
            dict(phi=rng.standard_normal(n).astype(F), diffusivity=0.3, wall=(2, -0.75, (0.0, 0.0, 3.0, 0.01))),
            dict(phi=rng.standard_normal(n).astype(F), diffusivity=0.1, wall=None)]


def _moving(mesh, ref, scale=0.6, time=0.05, ramp_time=0.1):
    """a rotating-cylinder selection on the body: (ubx, uby, moved) per surface face"""
    a = mesh.arrays()
    bv = BoundaryVelocities(a)
    x, y = np.asarray(a["face_cx"]), np.asarray(a["face_cy"])
    f = np.nonzero((bv.bt == 3) & (x >= BODY[0]) & (x <= BODY[2]) & (y >= BODY[1]) & (y <= BODY[3]))[0]
    bv.set(f, np.stack([-2.0 * (y[f] - 0.5), 2.0 * (x[f] - 1.0)], 1))
    bv.wall_scale = F(scale)
    c = Constants()
    c.time, c.ramp_time = F(time), F(ramp_time)
    return ref.wall_velocity(bv, c, _smoothstep(0.0, c.ramp_time, c.time))


def test_restatement_passes_the_checks_on_oracle_states(solved):
    mesh, u, p = solved
    n = mesh.num_cells()
    for box in (BODY, (0.0, 0.0, 3.0, 1.0)):
        ref = SurfaceRef(mesh.arrays(), box)
        assert ref.n > 8
        assert np.all(np.diff(ref.cell.astype(np.int64) * 64 + ref.slot) > 0), "order: cell, then slot"
        fields = _fields(n)
        ub = _moving(mesh, ref)
        assert ub[2].any() and np.abs(ub[0][ub[2]]).max() > 0.1
        for wv in (None, ub):
            ch = ref.sample(u, p, NU, 1.0, fields, wv)
            worst = ck.check(ch, ref.geometry(), u, p, NU, 1.0, fields, wv)
            print(box, wv is not None, {k: round(v, 3) for k, v in worst.items()})
            assert max(worst.values()) <= 1.0


def test_restatement_on_a_strip():
    m = strip(9)
    ref = SurfaceRef(m.arrays(), (0.0, -1.0, 1.0, 1.0))
    assert ref.n == 18 and np.array_equal(ref.cell, np.repeat(np.arange(9), 2))  # two wall slots per cell
    assert SurfaceRef(m.arrays(), (1.0, 0.0, 0.0, 1.0)).n == 0  # inverted
    rng = np.random.default_rng(0)
    u, p = rng.standard_normal((9, 2)).astype(F), rng.standard_normal(9).astype(F)
    ch = ref.sample(u, p, NU)
    assert ch.shape == (5, 18)
    ck.check(ch, ref.geometry(), u, p, NU)


class _OnTheFluid(SurfaceRef):
    def normal_sign(self):
        return -1.0


class _AbsoluteVelocity(SurfaceRef):
    def relative(self, u, ub):
        return u


class _AreaTimesDist(SurfaceRef):
    def diffusion(self, ad, dist):
        return lambda x: x * ad * dist


@pytest.mark.parametrize("variant", [_OnTheFluid, _AbsoluteVelocity, _AreaTimesDist])
def test_checks_reject_a_wrong_convention(solved, variant):
    mesh, u, p = solved
    good, bad = SurfaceRef(mesh.arrays(), BODY), variant(mesh.arrays(), BODY)
    fields = _fields(mesh.num_cells())[:1]
    ub = _moving(mesh, good)
    ck.check(good.sample(u, p, NU, 1.0, fields, ub), good.geometry(), u, p, NU, 1.0, fields, ub)
    with pytest.raises(AssertionError, match="f64 force"):
        ck.check(bad.sample(u, p, NU, 1.0, fields, ub), good.geometry(), u, p, NU, 1.0, fields, ub)


def test_fold_and_stats_restatements():
    """the fold adds a cell's terms in slot order; the statistics' first sample is exact"""
    m = strip(5)
    ref = SurfaceRef(m.arrays(), (0.0, -1.0, 1.0, 1.0))
    t = ref.fold(np.arange(10, dtype=np.float64), 5)
    assert np.array_equal(t, [1, 5, 9, 13, 17])
    st = SurfaceStats((2, 3))
    x = np.arange(6, dtype=np.float64).reshape(2, 3)
    st.accumulate(x, 0.25)
    assert np.array_equal(st.mean, x) and not st.m2.any() and st.samples == 1 and st.W == 0.25
    st.accumulate(3 * x, 0.75)
    assert np.allclose(st.mean, 2.5 * x) and np.allclose(st.variance(), 0.25 * 0.75 * (2 * x) ** 2)


def test_orderings_and_coefficients():
    th = np.array([0.1, 2.0, -3.0, -1.0, 3.1])
    g = dict(cx=1.0 + 0.2 * np.cos(th), cy=0.5 + 0.2 * np.sin(th), nx=-np.cos(th), ny=-np.sin(th),
             area=np.full(5, 0.1), dist_e=np.full(5, 0.05))
    assert list(post.order_by_angle(g, (1.0, 0.5))) == [2, 3, 0, 1, 4]
    assert list(post.order_by_x(g)) == list(np.lexsort((g["cy"], g["cx"])))
    # a flat bottom wall, n = (0, -1), t = (1, 0): tau = force_v.x / area, changing sign between x = 0.25 and 0.35
    x = 0.05 + 0.1 * np.arange(6)
    g = dict(cx=x, cy=np.zeros(6), nx=np.zeros(6), ny=-np.ones(6), area=np.full(6, 0.1), dist_e=np.full(6, 0.05))
    tau = np.array([3.0, 2.0, 1.0, -3.0, -2.0, -1.0])
    s = dict(p=2.0 + x, force_p=np.zeros((6, 2)), force_v=np.stack([tau * 0.1, np.zeros(6)], 1))
    c = post.coefficients(s, g, u_ref=2.0, density=0.5, p_ref=2.0)
    assert np.allclose(c["cp"], x) and np.allclose(c["cf"], tau) and np.allclose(c["tau"], tau)
    assert c["separation"].shape == (1, 2) and np.allclose(c["separation"][0], (0.25 + 0.1 * 0.25, 0.0))
    rev = post.coefficients(s, g, 2.0, 0.5, order=np.arange(6)[::-1])
    assert np.allclose(rev["separation"], c["separation"])
    tiny = dict(s, force_v=np.stack([np.array([1, 1, 1, -1, -1, -1]) * 1e-200, np.zeros(6)], 1))
    assert post.coefficients(tiny, g, 2.0, 0.5)["separation"].shape == (1, 2)  # cf[2] * cf[3] underflows to 0
    with pytest.raises(ValueError):
        post.coefficients(s, g, 0.0, 1.0)


NEW = ["cfd_surface_select", "cfd_surface_geometry_get", "cfd_surface_info_get", "cfd_surface_sample",
       "cfd_surface_stats_enable", "cfd_surface_stats_reset", "cfd_surface_stats_accumulate", "cfd_surface_stats_get"]


def test_header_declares_and_library_exports_the_surface_symbols():
    txt = open(os.path.join(ROOT, "include", "cfd2_amd.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = {m.group(1) for m in re.finditer(r"\b(cfd_[a-z0-9_]+)\s*\(", txt)}
    L = _bind()
    for name in NEW:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _ffi.EXPORTED, name
    assert "cfd_surface_info" in txt and _ffi.SurfaceInfo is not None
    import ctypes as C
    assert C.sizeof(_ffi.SurfaceInfo) == 32
    for name in NEW:  # a null handle is a status, not a crash
        fn = getattr(L, name)
        args = [None if hasattr(t, "contents") or t is C.c_void_p else 0 for t in fn.argtypes]
        assert fn(*args) != 0
