"""Case list and drivers shared by tests/test_scalar_bc.py (CPU: the oracle's
fluxes, the restatement's scalars) and tests/test_gpu_scalar_bc.py (HIP path):
wall conditions, sources and the wall-flux sums of the passive scalars.

HELPER MODULE, not a test.  Every driver takes the solver class, as
tests/scalar_cases.py does, so the two test modules run the same cases.

Meshes (the names of tests/scalar_cases.py) and their boxes:
  rect, voronoi, graded, strip1, strip130   the wall faces of the lower half of
                the wall-face centres' y range; on every one of them but strip1's
                neighbourless cell the inlet's corner cell has an inlet slot AND a
                selected wall slot
  obstacle_perm, fine_perm                  the box (0.7, 0.2, 1.3, 0.8) around the
                obstacle: its faces and none of the channel walls'; the step
                profile's front stands at x = 1.1, through the obstacle
The source box is the middle half of the cell centres' bounding box in x and y.

Flow, dt and advances are those of tests/scalar_cases.py; settings (scheme,
method, D): scheme 0 and scheme 1 under Jacobi at D = 0.01, scheme 1 under
BiCGStab at D = 0.05 (D > 0 throughout: a fixed-value wall acts through the
diffusion alone).  Wall value, flux and rate are sized so that each moves a
cell value by about 1e-2 per advance at either density: flux and rate carry
density * phi, so they scale with the density.
"""
import functools

import numpy as np

from tests import scalar_bc_checks as bc
from tests import scalar_cases as cs
from tests.scalar_bc_ref import ScalarBCRef

F = np.float32
TOL, DT, ADVANCES = cs.TOL, cs.DT, cs.ADVANCES
MESHES = ["rect", "voronoi", "graded", "strip1", "strip130", "obstacle_perm", "fine_perm"]
DENSITIES = cs.DENSITIES
SETTINGS = [s for s in cs.SETTINGS if s in ((0, 0, 0.01), (1, 0, 0.01), (1, 1, 0.05))]
assert len(SETTINGS) == 3
# where the float64 reference's clamp acts on a cell with a selected kind-1 slot:
# the smooth profile does it on the channel meshes, the front through the
# obstacle (below) on the two obstacle meshes, whose box holds the obstacle's
# faces alone
CLAMP_MESHES = [m for m in cs.CLAMP_MESHES if m in MESHES]
FRONT_X = 1.1  # the obstacle spans x in [0.8, 1.2]
OBSTACLE_BOX = (0.7, 0.2, 1.3, 0.8)
NO_BOX = (0.0, 0.0, -1.0, 0.0)
WALL_VALUE = 0.75
# case -> (wall kind, field profile, with a source)
CASES = {"value": (1, "step", False), "flux": (2, "smooth", False), "value+source": (1, "smooth", True),
         "source": (0, "step", True)}


@functools.lru_cache(maxsize=None)
def boxes(name):
    """(wall box, source box) of a mesh"""
    a = cs.mesh_of(name).arrays()
    x, y = a["cell_cx"], a["cell_cy"]
    sx, sy = 0.25 * (x.max() - x.min()), 0.25 * (y.max() - y.min())
    src = (x.min() + sx, y.min() + sy, x.max() - sx, y.max() - sy)
    if name.endswith("_perm"):
        return OBSTACLE_BOX, src
    wall = (a["face_neighbor"] == 0xFFFFFFFF) & ((a["face_boundary"] & 3) == 3)
    wy = a["face_cy"][wall]
    return (-1e9, -1e9, 1e9, 0.5 * (wy.min() + wy.max())), src


def initial(name, field):
    """(phi0, inlet value): scalar_cases.initial, but on the obstacle meshes the
    step profile's front stands at FRONT_X, inside the obstacle's box, instead of
    x = 0.8 where the obstacle begins: with it the float64 reference clamps
    cells that have a selected face (with the front at 0.8 it clamps none of
    them for any wall value)."""
    mesh = cs.mesh_of(name)
    if field == "step" and name.endswith("_perm"):
        return np.where(mesh.arrays()["cell_cx"] < FRONT_X, 1.0, 0.0), 1.0
    return cs.initial(mesh, field)


def wall_of(name, kind, density, value=None):
    if kind == 0:
        return dict(bc.NO_WALL)
    if value is None:
        value = WALL_VALUE if kind == 1 else 0.05 * density
    return dict(kind=kind, value=value, box=boxes(name)[0])


def source_of(name, on, density):
    return dict(rate=0.5 * density, box=boxes(name)[1]) if on else dict(bc.NO_SOURCE)


@functools.lru_cache(maxsize=None)
def _restated(name, scheme):
    return ScalarBCRef(cs.mesh_of(name).arrays(), scheme=scheme)


def restated(name, scheme, wall, source):
    R = _restated(name, scheme)
    R.set_wall(wall["kind"], wall["value"], wall["box"])
    R.set_source(source["rate"], source["box"])
    return R


# ------------------------------------------------------------ the CPU stand-in
def restated_solver(ref_class=ScalarBCRef):
    """scalar_cases.restated_solver with the wall, source and wall-flux calls
    of GpuSolver, the scalars `ref_class`'s, a ScalarBCRef."""
    from cfd2_amd import _ffi
    base = cs.restated_solver(ref_class)

    class RestatedBCSolver(base):
        _refs = {}

        def enable_scalars(self, count):
            super().enable_scalars(count)
            self._wall, self._source, self._prev = dict(bc.NO_WALL), dict(bc.NO_SOURCE), self._phi

        def _bc_ref(self):
            R = self._ref(self._scheme)
            R.set_wall(self._wall["kind"], self._wall["value"], self._wall["box"])
            R.set_source(self._source["rate"], self._source["box"])
            return R

        def set_scalar_wall(self, field, kind, value=0.0, box=NO_BOX):
            self._wall = dict(kind=kind, value=value, box=box)
            return self._bc_ref().faces

        def set_scalar_source(self, field, rate, box=NO_BOX):
            self._source = dict(rate=rate, box=box)
            return self._bc_ref().cells

        def advance_scalars(self, dt):
            self._bc_ref()
            self._prev = self._phi
            super().advance_scalars(dt)

        def scalar_wall_flux(self, field):
            R = self._bc_ref()
            f, a, pa = R.wall_flux(self._o.constants.density, self._D, self._phi, self._prev)
            return _ffi.ScalarWallFlux(flux=f, area=a, phi_area=pa, faces=R.faces, kind=R.kind)  # GpuSolver's own type

    return RestatedBCSolver


# --------------------------------------------------------------------- drivers
def _bits(x):
    return np.asarray(x, F).view(np.uint32)


def _assert_bit_exact(s, R, method, flux, density, D, inlet, phi_old, what):
    """the advance just made and its wall-flux sums == the restatement from phi_old, bit for bit"""
    st, ks, hs, wf = s.scalar_stats(0), s.scalar_solver_stats(0), s.scalar_scheme_stats(0), s.scalar_wall_flux(0)
    if method == 0:
        phi, sweeps, delta, conv = R.advance(flux, density, DT, D, inlet, phi_old)
    else:
        r = R.advance_krylov(flux, density, DT, D, inlet, phi_old)
        phi, sweeps, delta, conv = r.phi, r.polish_sweeps, r.last_delta, r.converged
        assert (ks.iterations, ks.stop_reason, ks.polish_sweeps) == (r.iterations, r.stop_reason, r.polish_sweeps), what
    assert ks.method == method and hs.scheme == R.scheme, what
    assert (st.sweeps, bool(st.converged)) == (sweeps, conv), (what, st.sweeps, sweeps)
    assert np.array_equal(_bits(st.last_delta), _bits(delta)), what
    assert hs.clamped_cells == R.clamped, (what, hs.clamped_cells, R.clamped)
    assert np.array_equal(_bits(s.get_scalar(0)), _bits(phi)), f"{what}: phi differs from the restatement"
    want = R.wall_flux(density, D, phi)
    got = (wf.flux, wf.area, wf.phi_area)
    assert np.array_equal(np.array(got).view(np.uint64), np.array(want).view(np.uint64)), (what, got, want)
    assert (wf.faces, wf.kind) == (R.faces, R.kind), what


def run_mesh(cls, name, density, bit_exact=True, settings=SETTINGS, cases=tuple(CASES), worst=None):
    """Every case x setting of one mesh at one density on one handle, two
    advances each: bit equality with the restatement (field, sweeps,
    last_delta, clamped_cells, the three wall-flux doubles, the counts), then in
    float64 the rows, the direct solve, the wall-flux sums and the extended
    budget.  Returns the coverage counts."""
    mesh = cs.mesh_of(name)
    a = mesh.arrays()
    s = cs.flow(cls, mesh, density)
    flux = s.debug_buffer(0)
    rho = float(s.constants.density)
    assert rho == density and np.all(np.isfinite(flux)) and np.abs(flux).max() > 0.0
    cover = {"advances": 0, "rows": 0, "faces": 0, "cells": 0, "clamped_at_wall": 0, "inlet_and_wall": 0}

    def note(check, ratio, what):
        if worst is not None and ratio > worst.get(check, (0.0, ""))[0]:
            worst[check] = (ratio, what)

    fm = bc._Faces(a)
    for case in cases:
        kind, field, with_source = CASES[case]
        wall, source = wall_of(name, kind, density), source_of(name, with_source, density)
        sel_faces = bc.selected_faces(a, wall) if kind else np.zeros(len(fm.own), bool)
        wall_cells = np.zeros(fm.N, bool)
        wall_cells[fm.own[sel_faces]] = True
        inlet_cells = np.zeros(fm.N, bool)
        inlet_cells[fm.own[fm.kind == bc.INLET]] = True
        cover["inlet_and_wall"] += int(np.count_nonzero(wall_cells & inlet_cells))
        for scheme, method, D in settings:
            phi0, inlet = initial(name, field)
            s.enable_scalars(1)
            s.set_scalar_params(0, D, inlet)
            s.set_scalar(0, phi0)
            if scheme:
                s.set_scalar_scheme(0, "vanleer")
            if method:
                s.set_scalar_solver(0, "bicgstab")
            faces = s.set_scalar_wall(0, wall["kind"], wall["value"], wall["box"])
            cells = s.set_scalar_source(0, source["rate"], source["box"])
            assert faces == int(np.count_nonzero(bc.selected_faces(a, wall))), (name, case, faces)
            assert cells == int(np.count_nonzero(bc.selected_cells(a, source))), (name, case, cells)
            assert (kind == 0 or faces > 0) and (not with_source or cells > 0), f"{name} {case}: an empty selection"
            cover["faces"] += faces if kind else 0
            cover["cells"] += cells if with_source else 0
            phi_old = s.get_scalar(0)
            for k in range(ADVANCES):
                what = f"{name} rho {density} {case} scheme {scheme} method {method} D {D} advance {k}"
                i_old = s.scalar_stats(0).integral
                s.advance_scalars(DT)
                st = s.scalar_stats(0)
                phi = s.get_scalar(0)
                wf = s.scalar_wall_flux(0)
                assert st.converged == 1 and st.last_delta <= TOL, f"{what}: not converged ({st.sweeps} sweeps)"
                if bit_exact:
                    _assert_bit_exact(s, restated(name, scheme, wall, source), method, flux, rho, D, inlet, phi_old, what)
                args = (a, flux, rho, DT, D, inlet)
                A, b = bc.system64(*args, phi_old, wall, source)
                clamp = np.zeros(len(phi))
                if scheme == 1:
                    b, clamp = bc.rhs_limited64(*args, phi_old, wall, source)
                    if kind == 1:
                        cover["clamped_at_wall"] += int(np.count_nonzero((clamp != 0.0) & wall_cells))
                terms = bc.row_terms64(*args, phi_old, phi, scheme, wall, source)
                rows, ratio = cs.sc.check_solved(A, b, phi, TOL, terms, what)
                note("check_solved", ratio, what)
                ratio = cs.sc.check_against_direct_solve(A, b, phi, TOL, terms, cs.sc.time_coefficient64(a, rho, DT), what)
                note("check_against_direct_solve", ratio, what)
                bc.check_wall_flux(a, rho, D, phi, wall, (wf.flux, wf.area, wf.phi_area), what)
                ratio, _ = bc.check_budget(*args, phi, i_old, st.integral, clamp, A, TOL, terms, wf.flux, source, what)
                note("check_budget", ratio, what)
                cover["advances"] += 1
                cover["rows"] += rows
                phi_old = phi
    s.close()
    return cover


def check_coverage(name, cover, settings=SETTINGS, cases=tuple(CASES)):
    """No check of run_mesh was vacuous on this mesh."""
    n = cs.mesh_of(name).num_cells()
    assert cover["advances"] == len(cases) * len(settings) * ADVANCES
    assert cover["rows"] == cover["advances"] * n > 0
    assert cover["faces"] > 0 and cover["cells"] > 0
    if name in CLAMP_MESHES and "value" in cases and any(s[0] == 1 for s in settings):
        assert cover["clamped_at_wall"] > 0, cover
    if not name.endswith("_perm") and name != "strip1":
        assert cover["inlet_and_wall"] > 0, cover


# ------------------------------------------------------------------- the bound
def run_bound(cls, name, value, scheme, method, advances=4):
    """Dye in [0, 1] (the step profile, inlet 1), kind 1 with `value` in {0, 1}:
    after every advance the field stays in [-e, 1 + e].  Jacobi: e = (total
    sweeps) (S + 4) 2^-24, scheme 0's allowance.  Method 1: e = tol max(diag /
    a_t), its own bound, at every advance (diag does not depend on the field)."""
    mesh = cs.mesh_of(name)
    s = cs.flow(cls, mesh, 1.0)
    flux, rho = s.debug_buffer(0), float(s.constants.density)
    D = 0.05 if method else 0.002
    dt = DT if method else 0.2
    phi0, inlet = cs.initial(mesh, "step")
    wall = wall_of(name, 1, rho, value)
    R = restated(name, scheme, wall, bc.NO_SOURCE)
    _, diag, _ = R.assemble(flux, rho, dt, D, inlet, phi0)
    ratio = float((diag / (R.vol * F(rho) / F(dt))).max())
    s.enable_scalars(1)
    s.set_scalar_params(0, D, inlet)
    s.set_scalar(0, phi0)
    if scheme:
        s.set_scalar_scheme(0, "vanleer")
    if method:
        s.set_scalar_solver(0, "bicgstab")
    assert s.set_scalar_wall(0, "value", value, wall["box"]) > 0
    total = 0
    for k in range(advances):
        s.advance_scalars(dt)
        st = s.scalar_stats(0)
        assert st.converged == 1
        total += st.sweeps
        e = TOL * ratio if method else total * (R.S + 4) * 2.0 ** -24
        phi = s.get_scalar(0)
        print(f"{name} value {value} scheme {scheme} method {method} advance {k}: min {phi.min():.3e} "
              f"max-1 {phi.max() - 1:.3e} e {e:.3e}")
        assert phi.min() >= -e and phi.max() <= 1.0 + e, (name, value, scheme, method, k, phi.min(), phi.max() - 1, e)
        assert st.min == phi.min() and st.max == phi.max()
    assert s.scalar_wall_flux(0).faces > 0
    s.close()


# ------------------------------------------------------------------- the no-op
def run_noop(cls, name="obstacle_perm", scheme=1):
    """A handle that sets kind 0, an empty box or rate 0 gives the bits of a
    handle that never called the setters; so does selecting a wall and a source
    and resetting them, and enable_scalars again resets them by itself."""
    mesh = cs.mesh_of(name)
    s = cs.flow(cls, mesh, 1000.0)
    phi0, inlet = cs.initial(mesh, "smooth")
    wbox, sbox = boxes(name)

    def run(setup):
        s.enable_scalars(1)
        s.set_scalar_params(0, 0.01, inlet)
        s.set_scalar(0, phi0)
        if scheme:
            s.set_scalar_scheme(0, "vanleer")
        setup()
        for _ in range(2):
            s.advance_scalars(DT)
        wf = s.scalar_wall_flux(0)
        assert (wf.flux, wf.area, wf.phi_area) == (0.0, 0.0, 0.0)
        return _bits(s.get_scalar(0)), s.scalar_stats(0).sweeps, s.scalar_scheme_stats(0).clamped_cells

    def same(x, y):
        return np.array_equal(x[0], y[0]) and x[1:] == y[1:]

    plain = run(lambda: None)

    def select():
        assert s.set_scalar_wall(0, "value", 0.9, wbox) > 0
        assert s.set_scalar_source(0, 50.0, sbox) > 0

    def selected_then_reset():
        select()
        s.set_scalar_wall(0, "adiabatic", 0.9, wbox)
        s.set_scalar_source(0, 0.0, sbox)

    s.enable_scalars(1)
    s.set_scalar_params(0, 0.01, inlet)
    s.set_scalar(0, phi0)
    select()
    s.advance_scalars(DT)
    assert not np.array_equal(_bits(s.get_scalar(0)), plain[0]) and s.scalar_wall_flux(0).flux != 0.0
    for what, setup in (("kind 0", lambda: s.set_scalar_wall(0, 0, 0.9, wbox)),
                        ("an empty wall box", lambda: s.set_scalar_wall(0, "value", 0.9, NO_BOX)),
                        ("a wall box without a wall face", lambda: s.set_scalar_wall(0, "flux", 0.9, (1e6, 1e6, 2e6, 2e6))),
                        ("rate 0", lambda: s.set_scalar_source(0, 0.0, sbox)),
                        ("an empty source box", lambda: s.set_scalar_source(0, 50.0, NO_BOX)),
                        ("selected, then reset", selected_then_reset),
                        ("enable_scalars after a selection", lambda: None)):
        assert same(run(setup), plain), f"{name}: {what} changes the bits"
        if what == "selected, then reset":
            select()  # left selected: the next run's enable_scalars alone must reset it
    s.close()


# ----------------------------------------------------------------- the physics
def run_physics(cls):
    """No flow on rect (set_u of zeros, inlet velocity 0, debug_prepare_assemble):
    with kind 2 on the lower wall each advance raises I by value area dt /
    density within the budget allowance; with kind 1 at value 1 from a zero
    field the field never decreases from advance to advance, the flux is
    positive while the field is below the value, and it falls."""
    name, rho, D = "rect", 1000.0, 0.01
    mesh = cs.mesh_of(name)
    a = mesh.arrays()
    s = cs.flow(cls, mesh, rho)
    c = s.constants
    c.inlet_velocity = 0.0
    s.constants = c
    s.set_u(np.zeros((mesh.num_cells(), 2)))
    s.debug_prepare_assemble(False)
    flux = s.debug_buffer(0)
    assert np.all(flux == 0.0)
    zero = np.zeros(mesh.num_cells())
    # kind 2.  Without diffusion nothing but the wall term is left in the budget;
    # with it the inlet faces (inlet value 0) take back g_f phi_o, the budget's
    # inlet part, which is subtracted before the comparison.
    wall = wall_of(name, 2, rho)
    value = float(np.float32(wall["value"]))
    for Dk in (0.0, D):
        s.enable_scalars(1)
        s.set_scalar_params(0, Dk, 0.0)
        assert s.set_scalar_wall(0, "flux", wall["value"], wall["box"]) > 0
        phi_old = zero
        for k in range(3):
            i_old = s.scalar_stats(0).integral
            s.advance_scalars(DT)
            st, wf, phi = s.scalar_stats(0), s.scalar_wall_flux(0), s.get_scalar(0)
            args = (a, flux, rho, DT, Dk, 0.0)
            A, _ = bc.system64(*args, phi_old, wall)
            terms = bc.row_terms64(*args, phi_old, phi, 0, wall)
            diag, allow = bc._row_allowance(A, TOL, terms)
            inlet_part = cs.sc.budget64(*args, phi)["inlet"]
            assert (inlet_part == 0.0) if Dk == 0.0 else (inlet_part < 0.0)
            scale = float(F(DT)) / rho
            rise = (st.integral - i_old) - inlet_part * scale
            assert abs(wf.flux - value * wf.area) <= bc.sc.TOL_ROW * abs(wf.flux)
            assert abs(rise - value * wf.area * scale) <= float(np.sum(diag * allow)) * scale, (Dk, k, rise)
            assert st.integral > i_old
            phi_old = phi
    # kind 1
    wall = wall_of(name, 1, rho, 1.0)
    s.enable_scalars(1)
    s.set_scalar_params(0, D, 0.0)
    assert s.set_scalar_wall(0, "value", 1.0, wall["box"]) > 0
    phi_old, last = zero, np.inf
    for k in range(4):
        s.advance_scalars(DT)
        phi, wf = s.get_scalar(0), s.scalar_wall_flux(0)
        assert np.all(phi >= phi_old), (k, float((phi - phi_old).min()))
        assert phi.max() < 1.0 and wf.flux > 0.0
        assert wf.flux < last, (k, wf.flux, last)
        assert abs(wf.phi_area / wf.area) < 1.0
        phi_old, last = phi, wf.flux
    s.close()


# ---------------------------------------------------------------- the refusals
def run_refusals(cls_solver, cls_group):
    """A rank of a group, scalars not enabled, a bad field, kind 3, non-finite
    values: CFD_ERR_INVALID with a message, and the handle is left as it was."""
    import pytest
    mesh = cs.mesh_of("obstacle_perm")
    g = cls_group(mesh, 2)
    for r in g.ranks:
        for call in (lambda: r.set_scalar_wall(0, 1, 1.0, OBSTACLE_BOX), lambda: r.set_scalar_source(0, 1.0, OBSTACLE_BOX),
                     lambda: r.scalar_wall_flux(0)):
            with pytest.raises(RuntimeError, match=r"status 1.*(one GPU|not enabled)"):
                call()
    g.close()
    s = cs.flow(cls_solver, mesh, 1.0)
    for call in (lambda: s.set_scalar_wall(0, 1, 1.0, OBSTACLE_BOX), lambda: s.set_scalar_source(0, 1.0, OBSTACLE_BOX),
                 lambda: s.scalar_wall_flux(0)):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    phi0, inlet = cs.initial(mesh, "smooth")
    s.enable_scalars(1)
    s.set_scalar_params(0, 0.01, inlet)
    s.set_scalar(0, phi0)
    assert s.set_scalar_wall(0, "value", 0.5, OBSTACLE_BOX) > 0
    for call, msg in ((lambda: s.set_scalar_wall(1, 1, 1.0, OBSTACLE_BOX), "field index"),
                      (lambda: s.set_scalar_source(-1, 1.0, OBSTACLE_BOX), "field index"),
                      (lambda: s.scalar_wall_flux(4), "field index"),
                      (lambda: s.set_scalar_wall(0, 3, 1.0, OBSTACLE_BOX), "kind must be"),
                      (lambda: s.set_scalar_wall(0, -1, 1.0, OBSTACLE_BOX), "kind must be"),
                      (lambda: s.set_scalar_wall(0, 1, float("nan"), OBSTACLE_BOX), "finite"),
                      (lambda: s.set_scalar_wall(0, 2, float("inf"), OBSTACLE_BOX), "finite"),
                      (lambda: s.set_scalar_source(0, float("nan"), OBSTACLE_BOX), "finite")):
        with pytest.raises(RuntimeError, match=rf"status 1.*{msg}"):
            call()
    wf = s.scalar_wall_flux(0)  # the refused calls changed nothing
    assert (wf.kind, wf.faces) == (1, int(np.count_nonzero(bc.selected_faces(mesh.arrays(), wall_of("obstacle_perm", 1, 1.0)))))
    s.advance_scalars(DT)
    assert s.scalar_wall_flux(0).flux != 0.0
    s.close()
