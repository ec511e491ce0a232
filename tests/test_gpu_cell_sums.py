"""The f64 cell sums of the diagnostics and of BiCGStab where the canonical tree
(kernels.hpp) leaves one block: every kernel that writes unit partials through
reduce_dev.hpp's sum_accumulate / sum_store, on tests.synthetic.strip(n) for

  n = 3 000    U = 1: four units per block, a partial last block
  n = 33 000   U = 2: 32 * 1024 + 232 cells, so the last block's second unit
               starts outside the mesh and must not be stored
  n = 70 000   U = 4: 68 * 1024 + 368 cells, one unit per block, the last partial

The fields are smooth functions of the cell index whose values float32 does not
hold exactly, so the order of the additions shows in the bits.  The force
region, the heated wall and the moving walls lie on a run of bottom-wall faces
across the boundary between the first two 1,024-cell blocks (the bottom wall
alone: with both walls of a cell the pressure force cancels cell by cell).
Either state setter clears the other field, so the flow sums are read twice:
with the velocity set (kinetic energy, enstrophy, the viscous force, torque
and power) and with the pressure set (the pressure force and torque; a strip's
walls are horizontal, so the x component is a sum of zeros).  Every sum == the
canonical sum (tests/refpy.canon_sum) of the float64 per-cell terms the
existing restatements form: tests/bcvel_ref.py (wall force, wall motion),
tests/buoyancy_ref.py (body force), tests/scalar_bc_ref.py (wall flux), and the
terms of tests/test_gpu_flow_diag.py and tests/test_gpu_scalar.py (kinetic
energy, enstrophy, the scalar integral).  One BiCGStab advance at n = 33 000
against tests/scalar_krylov_ref.py, compared as tests/test_gpu_scalar_krylov.py
compares."""
import functools

import numpy as np
import pytest

from cfd2_amd import GpuSolver, default_config
from tests import bcvel_cases as bc
from tests import refpy
from tests.bcvel_ref import BcvRefSolver
from tests.scalar_krylov_ref import ScalarKrylovRef
from tests.synthetic import red_units, strip
from tests.test_gpu_scalar import _bits, _flow
from tests.test_gpu_scalar_krylov import DT, _same

pytestmark = pytest.mark.gpu

F = np.float32
SIZES = {3000: 1, 33000: 2, 70000: 4}  # n: U
# strip(n): cell i spans x in [0.1 i, 0.1 i + 0.1], its two wall faces at x = 0.1 i + 0.05
REGION = (100.02, -1.0, 105.03, 0.05)   # the bottom wall of cells 1000 .. 1049: across cell 1024
MOVING = (101.02, -1.0, 103.53, 0.05)   # ... of cells 1010 .. 1034, a part of the run
FACES = dict(region=50, heated=50, moving=25)
PIVOT = (102.4, 0.3)
D, INLET, WALL_VALUE, BETA, REF, G = 0.05, 0.25, 0.7, 0.3, 0.45, (0.4, -9.81)


@functools.lru_cache(maxsize=None)
def _mesh(n):
    return strip(n)


def _fields(n):
    i = np.arange(n, dtype=np.float64)
    u = np.stack([0.8 + 0.5 * np.sin(0.0021 * i + 0.3), 0.3 * np.cos(0.0013 * i)], 1)
    p = 1.0 + 0.4 * np.sin(0.0019 * i)
    phi = 0.5 + 0.4 * np.sin(0.0023 * i + 0.4)
    return u, p, phi


def _setup(s, n):
    mesh = _mesh(n)
    bc.setup_flow(s, mesh)
    s.enable_scalars(1)
    s.set_scalar_params(0, D, INLET)
    s.set_scalar(0, _fields(n)[2])
    s.set_scalar_buoyancy(0, BETA, REF)
    s.set_gravity(*G)
    faces = dict(region=s.set_force_region(*REGION), heated=s.set_scalar_wall(0, "value", WALL_VALUE, REGION),
                 moving=s.set_wall_motion(MOVING, velocity=(0.3, 0.0)))
    return faces


@pytest.mark.parametrize("n", list(SIZES))
def test_sums_have_the_canonical_bits(n):
    mesh = _mesh(n)
    assert red_units(n)[2] == SIZES[n]
    g = GpuSolver(mesh, config=default_config(**bc.FIXED))
    r = BcvRefSolver(mesh, **bc.FIXED)
    assert _setup(g, n) == _setup(r, n) == FACES
    u0, p0, _ = _fields(n)
    vol = mesh.arrays()["cell_vol"].astype(F).astype(np.float64)

    phi = g.get_scalar(0)
    assert np.array_equal(_bits(phi), _bits(r.get_scalar(0)))
    integral = g.scalar_stats(0).integral
    print(f"n {n}: integral {integral!r}")
    assert integral == float(refpy.canon_sum(vol * phi))

    for what, field in (("u", u0), ("p", p0)):
        for s in (g, r):
            (s.set_u if what == "u" else s.set_p)(field)
        u, vort = g.get_u(), g.vorticity()
        d = g.flow_diagnostics()
        fp, fv = r.wall_force()
        wm = tuple(g.wall_motion(*PIVOT))
        ref_wm = r.wall_motion(*PIVOT)
        print(f"n {n}, {what} set: kinetic energy {d.kinetic_energy!r} enstrophy {d.enstrophy!r} forces "
              f"{list(d.force_pressure)} {list(d.force_viscous)} (ref {fp} {fv}) wall motion {wm} (ref {ref_wm})")
        assert d.kinetic_energy == float(refpy.canon_sum(0.5 * vol * (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])))
        assert d.enstrophy == float(refpy.canon_sum(0.5 * vol * vort * vort))
        assert d.region_faces == FACES["region"]
        assert (list(d.force_pressure), list(d.force_viscous)) == (fp, fv)
        assert wm == ref_wm and ref_wm[3:] == (FACES["region"], FACES["moving"])
        if what == "u":
            assert d.kinetic_energy > 0.0 and d.enstrophy > 0.0 and fv[0] != 0.0 and fv[1] != 0.0
            assert ref_wm[1] != 0.0 and ref_wm[2] != 0.0
        else:
            assert fp[1] != 0.0 and ref_wm[0] != 0.0

    wf = g.scalar_wall_flux(0)
    f0 = r.fields[0]
    ref_wf = f0.R.wall_flux(r.c.density, f0.D, f0.phi)
    print(f"n {n}: wall flux {(wf.flux, wf.area, wf.phi_area)} (ref {ref_wf})")
    assert (wf.flux, wf.area, wf.phi_area) == ref_wf and wf.faces == FACES["heated"]
    assert all(v != 0.0 for v in ref_wf)

    bf = g.buoyancy_force()
    print(f"n {n}: buoyancy force {tuple(bf)} (ref {r.buoyancy_force()})")
    assert tuple(bf) == r.buoyancy_force()
    assert bf[0] != 0.0 and bf[1] != 0.0
    g.close()


def test_bicgstab_dots_with_a_unit_outside_the_mesh():
    """one advance at n = 33 000 (U = 2, the last block's second unit outside the
    mesh): iterations, stop reason, polish sweeps, the bits of krylov_residual,
    last_delta and phi == tests/scalar_krylov_ref.py"""
    n = 33000
    mesh = _mesh(n)
    assert red_units(n)[2] == 2 and n % 1024 < 512
    phi = _fields(n)[2].astype(F)
    s, _ = _flow(mesh, "synthetic")
    s.enable_scalars(1)
    s.set_scalar_params(0, D, INLET)
    s.set_scalar(0, phi)
    s.set_scalar_solver(0, "bicgstab")
    r = ScalarKrylovRef(mesh.arrays()).advance_krylov(s.debug_buffer(0), s.constants.density, DT, D, INLET, phi)
    s.advance_scalars(DT)
    _same(s, r, f"strip({n})")
    assert r.iterations >= 2
    assert np.array_equal(_bits(s.get_scalar(0)), _bits(r.phi))
    s.close()
