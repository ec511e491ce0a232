"""The BiCGStab scalar solver on the GPU (csrc/hip/scalar.hip) against the numpy
restatement tests/scalar_krylov_ref.py, bit for bit, and against what it is
for.  Meshes and flows are those of tests/test_gpu_scalar.py:

  rect      fewer than 64 cells: one partly filled wavefront does every reduction
  obstacle  cell count not a multiple of 64
  voronoi   5 to 9 slots per cell: the four-at-a-time slot loop runs 2 and 3 rounds
  fine      more than four 1,024-cell blocks and a ragged tail
  units4    bench_mesh(0.0066, 0): the reductions write units of 4 chunks, and
            every iteration reduces four times; more than 256 sweep blocks, so
            the fold of the sweep's delta strides

Values fixed from runs of the restatement on the CPU (oracle fluxes, synthetic
flow, dt = 0.2, inlet 0.25, tol 1e-6, max_sweeps 200, check_interval 4): every
case ends converged with stop reason 1.  BiCGStab iterations / polish sweeps
per advance (3 advances):
  mesh        D = 0.05                     D = 0
  rect        9/4    9/4    10/4           7/4     8/4     7/4
  obstacle    16/4   16/4   15/4           14/4    14/4    14/4
  voronoi     12/4   11/4   10/4           11/4    10/4    10/4
  fine        75/4   69/4   63/4           67/24   66/20   69/4
  units4      211/28 216/4  228/76         233/172 232/168 224/100
fine, D = 0.05, dt = 0.2 (check 3): the restatement's Jacobi needs 752 sweeps
(the default 200 do not converge); error against the float64 direct solve:
Jacobi converged 7.7e-05, BiCGStab + polish 2.9e-05; f64 residual 9.6e-07
against a bound of 1.5e-06; max diag / a_t = 331, so e = 3.3e-04; the dye ends
in [2e-10, 1 + 1.2e-07].
Breakdown (check 4): rect, u = (1, 0) everywhere, D = 0, dt = 0.2, a step
profile: the matrix is lower triangular and iteration 2 meets a zero
denominator: reason 2, 8 polish sweeps, converged."""
import functools

import numpy as np
import pytest

from cfd2_amd import GpuGroup
from tests.scalar_krylov_ref import ScalarKrylovRef, breakdown_case, solve64
from tests.test_gpu_scalar import TOL, _bits, _check_shape, _fields, _flow, _mesh

pytestmark = pytest.mark.gpu

F = np.float32
DT = 0.2
ALL = ["rect", "obstacle", "voronoi", "fine", "units4"]


@functools.lru_cache(maxsize=None)
def _kref(name):
    return ScalarKrylovRef(_mesh(name).arrays())


def _start(name, D, inlet, phi, method="bicgstab", **kw):
    s, _ = _flow(_mesh(name), "synthetic")
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    s.set_scalar(0, phi)
    if method is not None:
        s.set_scalar_solver(0, method, **kw)
    return s


def _same(s, r, what):
    st, ks = s.scalar_stats(0), s.scalar_solver_stats(0)
    print(f"{what}: iterations {ks.iterations} (ref {r.iterations}) reason {ks.stop_reason} residual "
          f"{ks.krylov_residual:.3e} polish {ks.polish_sweeps} (ref {r.polish_sweeps}) delta {st.last_delta:.3e}")
    assert ks.method == 1
    assert (ks.iterations, ks.stop_reason, ks.polish_sweeps) == (r.iterations, r.stop_reason, r.polish_sweeps), what
    assert st.sweeps == ks.polish_sweeps and bool(st.converged) == r.converged, what
    assert _bits(ks.krylov_residual) == _bits(r.krylov_residual), what
    assert _bits(st.last_delta) == _bits(r.last_delta), what


@pytest.mark.parametrize("D", [0.05, 0.0])
@pytest.mark.parametrize("name", ALL)
def test_bit_exact_against_the_restatement(name, D):
    """check 1: phi after 1 and after 3 advances, iterations, stop reason,
    polish sweeps and the bits of krylov_residual and last_delta ==
    tests/scalar_krylov_ref.py; every case ends converged (module docstring)"""
    _check_shape(name)
    mesh, R = _mesh(name), _kref(name)
    if name == "units4":
        # the polish sweeps here are the only run of the block fold's strided
        # path (more per-block values than its 256 threads): one value per
        # 256-cell sweep block
        assert (mesh.num_cells() + 255) // 256 > 256
    inlet = 0.25
    phi = _fields(mesh)[1].astype(F)
    s = _start(name, D, inlet, phi)
    flux, density = s.debug_buffer(0), s.constants.density
    for k in range(3):
        r = R.advance_krylov(flux, density, DT, D, inlet, phi)
        phi = r.phi
        s.advance_scalars(DT)
        _same(s, r, f"{name} D={D} advance {k}")
        assert r.converged and r.stop_reason == 1, k
        if k in (0, 2):
            assert np.array_equal(_bits(s.get_scalar(0)), _bits(phi)), k
    s.close()


def test_read_cadence_is_invisible():
    """check 2: the Krylov check_interval 1, 8, 32 on fine: the same phi bits, iterations and reason"""
    mesh = _mesh("fine")
    phi0 = _fields(mesh)[1]
    got = []
    for ci in (1, 8, 32):
        s = _start("fine", 0.05, 0.25, phi0, check_interval=ci)
        s.advance_scalars(DT)
        ks = s.scalar_solver_stats(0)
        got.append((ks.iterations, ks.stop_reason, _bits(ks.krylov_residual), _bits(s.get_scalar(0))))
        s.close()
    assert got[0][0] % 8 != 0 and got[0][0] > 32  # the stop falls inside a batch of either size
    for g in got[1:]:
        assert g[:2] == got[0][:2] and g[2] == got[0][2]
        assert np.array_equal(g[3], got[0][3])


def test_it_does_what_jacobi_cannot():
    """check 3: fine, D = 0.05, dt = 0.2: Jacobi does not converge in the default
    200 sweeps, BiCGStab + polish does; its answer satisfies the system to the
    bound of test_converged_means_solved, and is no further from the float64
    direct solve than the Jacobi restatement run until it converges"""
    mesh, R = _mesh("fine"), _kref("fine")
    D, inlet = 0.05, 0.25
    phi0 = _fields(mesh)[1].astype(F)
    j = _start("fine", D, inlet, phi0, method=None)
    j.advance_scalars(DT)
    stj = j.scalar_stats(0)
    assert (stj.converged, stj.sweeps) == (0, 200) and stj.last_delta > TOL
    flux, density = j.debug_buffer(0), j.constants.density
    j.close()
    s = _start("fine", D, inlet, phi0)
    s.advance_scalars(DT)
    st = s.scalar_stats(0)
    assert st.converged == 1 and st.last_delta <= TOL
    phi = s.get_scalar(0)
    s.close()
    coef, diag, b = R.assemble(flux, density, DT, D, inlet, phi0)
    res = R.residual64(coef, diag, b, phi)
    bound = TOL + (R.S + 4) * 2.0 ** -24 * float(np.abs(phi).max())
    exact = solve64(R, coef, diag, b)
    jac, sweeps, _, conv = R.advance(flux, density, DT, D, inlet, phi0, max_sweeps=100000)
    ek, ej = float(np.abs(phi - exact).max()), float(np.abs(jac - exact).max())
    print(f"residual {res:.3e} bound {bound:.3e}; error bicgstab {ek:.3e}, jacobi ({sweeps} sweeps) {ej:.3e}")
    assert conv and sweeps > 200
    assert res <= bound
    assert ek <= ej


def test_dye_stays_in_bounds():
    """check 3, the dye bound: initial and inlet values in [0, 1] stay in [-e, 1
    + e], e = tol max_i(diag_i / a_t,i) + (S + 4) 2^-24: a converged x has x_i <=
    J(x)_i + tol, and J is a convex combination with weight a_t / diag on phi_old"""
    mesh, R = _mesh("fine"), _kref("fine")
    x = mesh.arrays()["cell_cx"]
    dye = np.where(x < 0.8, 1.0, 0.0)
    s = _start("fine", 0.05, 1.0, dye)
    flux, density = s.debug_buffer(0), s.constants.density
    _, diag, _ = R.assemble(flux, density, DT, 0.05, 1.0, dye)
    a_t = R.vol * F(density) / F(DT)
    e = TOL * float((diag / a_t).max()) + (R.S + 4) * 2.0 ** -24
    for k in range(2):
        s.advance_scalars(DT)
        st, ks = s.scalar_stats(0), s.scalar_solver_stats(0)
        phi = s.get_scalar(0)
        print(f"advance {k}: iterations {ks.iterations} polish {st.sweeps} min {phi.min():.3e} max-1 {phi.max() - 1:.3e} e {e:.3e}")
        assert st.converged == 1
        assert phi.min() >= -e and phi.max() <= 1.0 + e, k
    s.close()


def test_breakdown_on_the_device():
    """check 4: pure upwind on rect (tests/scalar_krylov_ref.breakdown_case, also
    in tests/test_scalar_krylov.py): reason 2, finite values, the restatement's bits"""
    mesh, R = _mesh("rect"), _kref("rect")
    u, phi0, D, inlet, dt = breakdown_case(mesh)
    s, _ = _flow(mesh, "synthetic")
    s.set_u(u)
    s.debug_prepare_assemble(False)
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    s.set_scalar(0, phi0)
    s.set_scalar_solver(0)
    r = R.advance_krylov(s.debug_buffer(0), s.constants.density, dt, D, inlet, phi0)
    s.advance_scalars(dt)
    _same(s, r, "breakdown")
    got = s.get_scalar(0)
    assert r.stop_reason == 2 and r.converged
    assert np.isfinite(got).all()
    assert np.array_equal(_bits(got), _bits(r.phi))
    s.close()


def test_isolation():
    """check 5: a BiCGStab field next to a Jacobi field leaves that field's bits
    alone; the step is untouched by Krylov advances in between; method 0 again
    gives today's Jacobi bits"""
    mesh = _mesh("obstacle")
    phi = _fields(mesh)[1]
    a, dt = _flow(mesh, "synthetic")  # Jacobi only
    a.enable_scalars(1)
    a.set_scalar_params(0, 0.02, 0.25)
    a.set_scalar(0, phi)
    b, _ = _flow(mesh, "synthetic")  # the same field 0, and field 1 on BiCGStab
    b.enable_scalars(2)
    b.set_scalar_params(0, 0.02, 0.25)
    b.set_scalar(0, phi)
    b.set_scalar_params(1, 0.05, 1.0)
    b.set_scalar(1, 1.0 - phi)
    b.set_scalar_solver(1)
    for s in (a, b):
        s.initialize_history()
    for k in range(2):
        a.step()
        b.step()
        for g in ("get_u", "get_p"):
            assert np.array_equal(getattr(a, g)(), getattr(b, g)()), (g, k)
        a.advance_scalars(dt)
        b.advance_scalars(dt)
        assert np.array_equal(a.get_scalar(0), b.get_scalar(0)), k
        assert bytes(a.scalar_stats(0)) == bytes(b.scalar_stats(0)), k
        assert b.scalar_solver_stats(1).iterations > 0 and b.scalar_solver_stats(0).method == 0
        assert bytes(b.scalar_solver_stats(0)) == bytes(a.scalar_solver_stats(0))
    # back to method 0: field 1 of b against a Jacobi-only twin started from b's current field
    now = b.get_scalar(1)
    b.set_scalar_solver(1, "jacobi")
    c, _ = _flow(mesh, "synthetic")
    c.initialize_history()
    c.step()
    c.step()
    c.enable_scalars(1)
    c.set_scalar_params(0, 0.05, 1.0)
    c.set_scalar(0, now)
    b.advance_scalars(dt)
    c.advance_scalars(dt)
    assert np.array_equal(b.get_scalar(1), c.get_scalar(0))
    assert bytes(b.scalar_stats(1)) == bytes(c.scalar_stats(0))
    assert b.scalar_solver_stats(1).method == 0 and b.scalar_solver_stats(1).iterations == 0
    for s in (a, b, c):
        s.close()


def test_refusals_and_bad_arguments():
    """check 6: a group refuses; scalars not enabled, a bad field, a bad method,
    max_iters < 1 and check_interval < 1 return CFD_ERR_INVALID with a message"""
    mesh = _mesh("obstacle")
    g = GpuGroup(mesh, 2)
    with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
        g.set_scalar_solver(0)
    with pytest.raises(RuntimeError, match=r"status 1.*one GPU"):
        g.scalar_solver_stats(0)
    g.close()
    s, _ = _flow(mesh, "synthetic")
    for call in (lambda: s.set_scalar_solver(0), lambda: s.scalar_solver_stats(0)):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    s.enable_scalars(2)
    for f in (-1, 2):
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.set_scalar_solver(f)
        with pytest.raises(RuntimeError, match=r"status 1.*field index"):
            s.scalar_solver_stats(f)
    for kw, what in ((dict(method=2), "method"), (dict(method=-1), "method"), (dict(max_iters=0), "max_iters"),
                     (dict(check_interval=0), "check_interval")):
        with pytest.raises(RuntimeError, match=rf"status 1.*{what}"):
            s.set_scalar_solver(0, **kw)
    assert s.scalar_solver_stats(0).method == 0  # nothing was selected
    s.set_scalar_solver(1, max_iters=3, check_interval=2)
    s.enable_scalars(0)
    with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
        s.set_scalar_solver(0)
    s.enable_scalars(1)  # and back: method 0 again, the work space allocated anew on selection
    s.set_scalar_solver(0, max_iters=3, check_interval=2)
    s.advance_scalars(DT)
    ks = s.scalar_solver_stats(0)
    assert (ks.method, ks.iterations, ks.stop_reason) == (1, 0, 1)  # a zero field is its own solution
    s.close()


def test_the_iteration_cap_is_reason_three():
    """max_iters = 5 on fine: reason 3 at iteration 5 whatever the read interval, and the polish still runs"""
    mesh, R = _mesh("fine"), _kref("fine")
    phi0 = _fields(mesh)[1].astype(F)
    ref = None
    for ci in (2, 8):
        s = _start("fine", 0.05, 0.25, phi0, max_iters=5, check_interval=ci)
        if ref is None:
            ref = R.advance_krylov(s.debug_buffer(0), s.constants.density, DT, 0.05, 0.25, phi0, max_iters=5)
        s.advance_scalars(DT)
        _same(s, ref, f"cap, interval {ci}")
        assert ref.stop_reason == 3 and ref.iterations == 5
        assert np.array_equal(_bits(s.get_scalar(0)), _bits(ref.phi))
        s.close()
