"""Scheme 1 of the passive scalars (limited linear, van Leer) on the GPU
(k_scalar_grad and k_scalar_assemble_limited of csrc/hip/scalar.hip) against
the numpy restatement tests/scalar_hr_ref.py, bit for bit, and against what the
scheme promises.  Meshes and flows are those of tests/test_gpu_scalar.py:

  rect      fewer than 64 cells: one partly filled wavefront votes and counts
  obstacle  cell count not a multiple of 64
  voronoi   5 to 9 slots per cell: the four-at-a-time slot loops run 2 and 3 rounds
  fine      more than four 1,024-cell blocks and a ragged tail: the count is
            the sum of many blocks' atomic adds

None of the four has a degenerate slot (lambda falls back to 0.5 only when a
cell centre lies on its face), so that branch of the gradient is not run here.

Values fixed from runs of the restatement on the CPU (oracle fluxes).
Check 1, synthetic flow, dt = 0.02, inlet 0.25: clamped cells per advance
  rect 3 2 2, obstacle 10 8 9, voronoi 8 8 8, fine 26 61 59 (D = 0) and 26 45 37
  (D = 0.01); the sweep counts are those of scheme 0 (tests/test_gpu_scalar.py).
Check 3 (synthetic flux, dt = 0.2, D = 0.002, inlet 1, the step profile x < 0.8,
5 advances): clamped cells per advance
  rect 0 12 13 13 10, obstacle 0 47 56 58 59, voronoi 8 40 46 44 47,
  fine 18 1794 729 779 848; the overshoot above 1 was at most 6e-7 against
  e >= 5.7e-6, and the sweep counts are scheme 0's.
Check 4, fine after those 5 advances: 2,338 cells in (0.05, 0.95) under scheme
1, 2,421 under scheme 0 (the CFL is above 1 on most cells, where the table of
tests/test_scalar_hr.py says to expect a small gain).
Check 5, fine, D = 0.05, dt = 0.2, method 1: 77 iterations, reason 1, 4 polish
sweeps, 286 clamped cells."""
import functools

import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver
from tests.scalar_hr_ref import ScalarHRRef
from tests.test_gpu_scalar import SMALL, STEP_DT, _bits, _check_shape, _fields, _flow, _mesh

pytestmark = pytest.mark.gpu

F = np.float32
DYE_DT, DYE_D = 0.2, 0.002  # the maximum-principle setting of tests/test_gpu_scalar.py


@functools.lru_cache(maxsize=None)
def _href(name, scheme=1):
    return ScalarHRRef(_mesh(name).arrays(), scheme=scheme)


def _start(name, mode, D, inlet, phi, scheme="vanleer"):
    s, dt = _flow(_mesh(name), mode)
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    s.set_scalar(0, phi)
    if scheme is not None:
        s.set_scalar_scheme(0, scheme)
    return s, dt


def _step_profile(name):
    return np.where(_mesh(name).arrays()["cell_cx"] < 0.8, 1.0, 0.0).astype(F)


@functools.lru_cache(maxsize=None)
def _dye_ref(name, scheme):
    """the restatement's 5 advances of the step profile in the maximum-principle
    setting: a list of (phi, sweeps, clamped cells); the fluxes are the device's
    (the synthetic flow of this mesh, the same on every handle)"""
    s, _ = _flow(_mesh(name), "synthetic")
    flux, density = s.debug_buffer(0), s.constants.density
    s.close()
    R = _href(name, scheme)
    phi, out = _step_profile(name), []
    for _ in range(5):
        phi, sw, _, conv = R.advance(flux, density, DYE_DT, DYE_D, 1.0, phi)
        assert conv
        out.append((phi, sw, R.clamped))
    return out


def _width(phi):
    return int(np.count_nonzero((phi > 0.05) & (phi < 0.95)))


@pytest.mark.parametrize("D", [0.01, 0.0])
@pytest.mark.parametrize("mode", ["steps", "synthetic"])
@pytest.mark.parametrize("name", SMALL)
def test_bit_exact_against_the_restatement(name, mode, D):
    """check 1: phi after 1 and after 3 advances, the sweep counts, the bits of
    last_delta and clamped_cells == tests/scalar_hr_ref.py"""
    _check_shape(name)
    mesh, R = _mesh(name), _href(name)
    inlet = 0.25
    phi = _fields(mesh)[1].astype(F)
    s, dt = _start(name, mode, D, inlet, phi)
    flux, density = s.debug_buffer(0), s.constants.density
    for k in range(3):
        phi, sw, delta, conv = R.advance(flux, density, STEP_DT if dt is None else dt, D, inlet, phi)
        s.advance_scalars(dt)
        st, hs = s.scalar_stats(0), s.scalar_scheme_stats(0)
        print(f"{name} {mode} D={D} advance {k}: sweeps {st.sweeps} (ref {sw}) delta {st.last_delta:.3e} "
              f"clamped {hs.clamped_cells} (ref {R.clamped})")
        assert (st.sweeps, bool(st.converged)) == (sw, conv) and conv, k
        assert _bits(st.last_delta) == _bits(delta), k
        assert (hs.scheme, hs.clamped_cells) == (1, R.clamped), k
        if k in (0, 2):
            assert np.array_equal(_bits(s.get_scalar(0)), _bits(phi)), k
    s.close()


def test_scheme_zero_is_untouched():
    """check 2: a handle that selected scheme 1, advanced and went back to scheme
    0 gives the bits of a handle that never selected it; cfd_scalars_enable
    resets the scheme"""
    name, D, inlet = "obstacle", 0.01, 0.25
    phi0 = _fields(_mesh(name))[1].astype(F)
    a, dt = _start(name, "synthetic", D, inlet, phi0)
    b, _ = _start(name, "synthetic", D, inlet, phi0, scheme=None)
    a.advance_scalars(dt)
    b.advance_scalars(dt)
    assert a.scalar_scheme_stats(0).scheme == 1 and a.scalar_scheme_stats(0).clamped_cells > 0
    assert b.scalar_scheme_stats(0).scheme == 0 and b.scalar_scheme_stats(0).clamped_cells == 0
    assert not np.array_equal(a.get_scalar(0), b.get_scalar(0))  # scheme 1 did something
    a.set_scalar_scheme(0, "upwind")
    a.set_scalar(0, b.get_scalar(0))
    for k in range(2):
        a.advance_scalars(dt)
        b.advance_scalars(dt)
        assert np.array_equal(_bits(a.get_scalar(0)), _bits(b.get_scalar(0))), k
        assert bytes(a.scalar_stats(0)) == bytes(b.scalar_stats(0)), k
        assert bytes(a.scalar_scheme_stats(0)) == bytes(b.scalar_scheme_stats(0)), k
    a.set_scalar_scheme(0, "vanleer")
    now = b.get_scalar(0)
    a.enable_scalars(1)  # zero fields, default params, scheme 0 again
    a.set_scalar_params(0, D, inlet)
    a.set_scalar(0, now)
    a.advance_scalars(dt)
    b.advance_scalars(dt)
    assert a.scalar_scheme_stats(0).scheme == 0
    assert np.array_equal(_bits(a.get_scalar(0)), _bits(b.get_scalar(0)))
    a.close()
    b.close()


@pytest.mark.parametrize("name", SMALL)
def test_maximum_principle(name):
    """check 3: the setting of tests/test_gpu_scalar.py's maximum-principle test
    (synthetic flux, dt = 0.2, D = 0.002, 5 advances, a step profile in [0, 1],
    inlet 1) under scheme 1: every value stays in [-e, 1 + e], e = (total
    sweeps) (S + 4) 2^-24, the allowance of that test.  The clamp is exercised:
    the restatement counts clamped cells on every mesh, and the device counts
    the same ones."""
    ref = _dye_ref(name, 1)
    assert sum(c for _, _, c in ref) > 0
    R = _href(name)
    s, _ = _start(name, "synthetic", DYE_D, 1.0, _step_profile(name))
    total = 0
    for k in range(5):
        s.advance_scalars(DYE_DT)
        st, hs = s.scalar_stats(0), s.scalar_scheme_stats(0)
        total += st.sweeps
        e = total * (R.S + 4) * 2.0 ** -24
        phi = s.get_scalar(0)
        print(f"{name} advance {k}: sweeps {st.sweeps} clamped {hs.clamped_cells} min {phi.min():.3e} "
              f"max-1 {phi.max() - 1:.3e} e {e:.3e}")
        assert st.converged == 1
        assert st.min == phi.min() and st.max == phi.max()
        assert phi.min() >= -e and phi.max() <= 1.0 + e, k
        assert (st.sweeps, hs.clamped_cells) == ref[k][1:], k
    s.close()


def test_sharper_on_the_device():
    """check 4: on fine, the step profile advanced 5 times leaves fewer cells in
    (0.05, 0.95) under scheme 1 than under scheme 0; both counts are the
    restatement's"""
    widths = []
    for scheme in ("upwind", "vanleer"):
        s, _ = _start("fine", "synthetic", DYE_D, 1.0, _step_profile("fine"), scheme=scheme)
        for _ in range(5):
            s.advance_scalars(DYE_DT)
        phi = s.get_scalar(0)
        s.close()
        want = _dye_ref("fine", 0 if scheme == "upwind" else 1)[-1][0]
        assert np.array_equal(_bits(phi), _bits(want)), scheme
        widths.append(_width(phi))
        assert widths[-1] == _width(want)
    print(f"cells in (0.05, 0.95): upwind {widths[0]} scheme 1 {widths[1]}")
    assert widths[1] < widths[0]


def test_composes_with_bicgstab():
    """check 5: fine, scheme 1 with method 1 and D = 0.05: bit for bit against
    ScalarKrylovRef's advance fed the restated b (ScalarHRRef is one)"""
    name, D, inlet, dt = "fine", 0.05, 0.25, 0.2
    mesh, R = _mesh(name), _href(name)
    phi0 = _fields(mesh)[1].astype(F)
    s, _ = _start(name, "synthetic", D, inlet, phi0)
    s.set_scalar_solver(0, "bicgstab")
    r = R.advance_krylov(s.debug_buffer(0), s.constants.density, dt, D, inlet, phi0)
    s.advance_scalars(dt)
    st, ks, hs = s.scalar_stats(0), s.scalar_solver_stats(0), s.scalar_scheme_stats(0)
    print(f"iterations {ks.iterations} (ref {r.iterations}) reason {ks.stop_reason} polish {ks.polish_sweeps} "
          f"clamped {hs.clamped_cells} (ref {R.clamped})")
    assert r.converged and r.stop_reason == 1
    assert (ks.method, ks.iterations, ks.stop_reason, ks.polish_sweeps) == (1, r.iterations, r.stop_reason, r.polish_sweeps)
    assert st.sweeps == r.polish_sweeps and st.converged == 1
    assert _bits(ks.krylov_residual) == _bits(r.krylov_residual) and _bits(st.last_delta) == _bits(r.last_delta)
    assert (hs.scheme, hs.clamped_cells) == (1, R.clamped) and R.clamped > 0
    assert np.array_equal(_bits(s.get_scalar(0)), _bits(r.phi))
    s.close()


def test_constant_field_keeps_scheme_zero_bits():
    """check 6: a constant field has h = 0 on every slot: the restated b has
    scheme 0's bits, the device's advance gives scheme 0's phi bits (the inlet
    value differs, so phi does move), and nothing is clamped"""
    name, D, inlet, dt = "voronoi", 0.01, 1.0, 0.02
    const = np.full(_mesh(name).num_cells(), 0.37, F)
    a, _ = _start(name, "synthetic", D, inlet, const)
    b, _ = _start(name, "synthetic", D, inlet, const, scheme=None)
    flux, density = a.debug_buffer(0), a.constants.density
    b1 = _href(name).assemble(flux, density, dt, D, inlet, const)[2]
    b0 = _href(name, 0).assemble(flux, density, dt, D, inlet, const)[2]
    assert np.array_equal(_bits(b1), _bits(b0)) and _href(name).clamped == 0
    a.advance_scalars(dt)
    b.advance_scalars(dt)
    got = a.get_scalar(0)
    assert np.array_equal(_bits(got), _bits(b.get_scalar(0)))
    assert not np.array_equal(got.astype(F), const)
    hs = a.scalar_scheme_stats(0)
    assert (hs.scheme, hs.clamped_cells) == (1, 0)
    a.close()
    b.close()


def test_nan_is_reported_as_diverged():
    """check 6: one NaN cell passes through the correction and the clamp (comparisons): CFD_ERR_DIVERGED (3)"""
    mesh = _mesh("rect")
    phi = _fields(mesh)[1]
    phi[3] = np.nan
    s, dt = _start("rect", "synthetic", 0.01, 0.25, phi)
    with pytest.raises(RuntimeError, match=r"status 3.*diverged"):
        s.advance_scalars(dt)
    s.close()


def test_refusals_and_bad_arguments():
    """check 6: a group refuses; scalars not enabled, a bad field and a bad
    scheme return CFD_ERR_INVALID with a message"""
    mesh = _mesh("obstacle")
    g = GpuGroup(mesh, 2)
    with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
        g.set_scalar_scheme(0)
    with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
        g.scalar_scheme_stats(0)
    g.close()
    s = GpuSolver(mesh)
    for call in (lambda: s.set_scalar_scheme(0), lambda: s.scalar_scheme_stats(0)):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    s.enable_scalars(2)
    for f in (-1, 2):
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.set_scalar_scheme(f)
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.scalar_scheme_stats(f)
    for bad in (2, -1):
        with pytest.raises(RuntimeError, match=r"status 1.*scheme"):
            s.set_scalar_scheme(0, bad)
    assert s.scalar_scheme_stats(0).scheme == 0  # nothing was selected, nothing advanced
    s.set_scalar_scheme(1, "vanleer")
    s.enable_scalars(0)
    with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
        s.set_scalar_scheme(0)
    s.enable_scalars(1)  # and back: the work space is allocated anew on selection
    s.set_scalar_scheme(0)
    s.advance_scalars(0.02)
    hs = s.scalar_scheme_stats(0)
    assert (hs.scheme, hs.clamped_cells) == (1, 0)  # a zero field with inlet 0 stays zero
    s.close()
