"""Wall surface distributions on the GPU: the device channels bit for bit against
the numpy restatement (tests/surface_ref.py), their fold against the existing
integrals' bits, moving walls, the shear of a known field, the running
statistics, that the module leaves the solver alone, and the refusals."""
from fractions import Fraction

import numpy as np
import pytest

from cfd2_amd import GpuGroup, GpuSolver
from cfd2_amd import surface as post
from tests import refpy
from tests import surface_checks as ck
from tests import tstats_checks as TK
from tests.bcvel_ref import BoundaryVelocities
from tests.meshes import channel_obstacle
from tests.surface_ref import SurfaceRef, SurfaceStats
from tests.synthetic import strip

pytestmark = pytest.mark.gpu

F = np.float32
EPS = 2.0 ** -52
H = 0.125          # strip spacing: every centre, area and distance is exact in float32
NS = 140           # strip cells: 280 wall faces, two 256-thread blocks
BODY = (0.7, 0.2, 1.3, 0.8)
EVERYTHING = (-1.0, -1.0, 100.0, 100.0)
# strip boxes by face count: x-width times one wall (y <= H / 2: bottom only) or both
STRIP_BOXES = {0: (0.0, 5.0, 1.0, 6.0), 1: (0.0, -1.0, H, H / 2), 63: (0.0, -1.0, 63 * H, H / 2),
               64: (0.0, -1.0, 32 * H, 2 * H), 65: (0.0, -1.0, 65 * H, H / 2), 2 * NS: EVERYTHING}


def same_bits(a, b, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), what


def bits(x):
    return np.float64(x).view(np.uint64)


@pytest.fixture(scope="module")
def obstacle():
    return channel_obstacle(h=0.025, smooth_iters=20)  # a few thousand cells, more than 256 wall faces


def random_state(s, seed, drive="u"):
    """a random float32 field; either setter clobbers the whole state, so u or p, not both"""
    rng = np.random.default_rng(seed)
    n = s.num_cells
    if drive == "u":
        s.set_u(rng.standard_normal((n, 2)).astype(F))
    else:
        s.set_p(rng.standard_normal(n).astype(F))


def state_of(s, nf=0):
    return s.get_u().astype(F), s.get_p().astype(F), [s.get_scalar(f).astype(F) for f in range(nf)]


def restated(s, mesh, box, fields=(), bv=None):
    """the restatement's channels of the handle's current state (its own read-backs widen float32 exactly)"""
    c = s.constants
    u, p, phis = state_of(s, len(fields))
    ref = SurfaceRef(mesh.arrays(), box)
    fields = [dict(fd, phi=phi) for fd, phi in zip(fields, phis)]
    wv = None
    if bv is not None:
        rc = refpy.Constants()
        rc.time, rc.ramp_time, rc.inlet_velocity = F(c.time), F(c.ramp_time), F(c.inlet_velocity)
        wv = ref.wall_velocity(bv, rc, refpy._smoothstep(0.0, rc.ramp_time, rc.time))
    return ref, ref.sample(u, p, c.viscosity, c.density, fields, wv), (u, p, fields, wv)


def compare(s, mesh, box, fields=(), bv=None, what=""):
    ref, want, inputs = restated(s, mesh, box, fields, bv)
    got = s.surface()
    same_bits(got["channels"], want, what)
    return ref, got, inputs


def flow(mesh):
    s = GpuSolver(mesh)
    s.set_dt(0.001)
    s.set_viscosity(0.001)
    s.set_inlet_velocity(1.0)
    s.set_precond_type(1)
    s.initialize_history()
    return s


# ------------------------------------------------------------------ 1. the bits
@pytest.mark.parametrize("faces", sorted(STRIP_BOXES))
def test_strip_bits_against_the_restatement(faces):
    mesh = strip(NS, H)
    s = GpuSolver(mesh)
    s.set_viscosity(0.01)
    box = STRIP_BOXES[faces]
    assert s.select_surface(box) == faces
    assert s.surface_info() == dict(faces=faces, channels=5, samples=0, total_weight=0.0, stats_on=False)
    g = s.surface_geometry()
    want = SurfaceRef(mesh.arrays(), box).geometry()
    for k in want:
        assert g[k].dtype == want[k].dtype and np.array_equal(g[k], want[k]), k
    if faces in (64, 2 * NS):  # one cell gives two faces: slots in ascending order
        assert np.array_equal(g["cell"][0::2], g["cell"][1::2]) and np.all(g["slot"][0::2] < g["slot"][1::2])
    for drive, key in (("u", "force_v"), ("p", "force_p")):
        random_state(s, faces, drive)
        ref, got, (u, p, _, _) = compare(s, mesh, box, what="random " + drive)
        assert got["p"].shape == (faces,) and got["force_p"].shape == (faces, 2) and got["force_v"].shape == (faces, 2)
        if faces:
            assert got[key].any()
            ck.check(got["channels"], g, u, p, s.constants.viscosity)
    # scalars on: 9 channels, a value wall on the bottom and a flux wall on the top of the first 40 cells
    s.enable_scalars(2)
    fields = [dict(diffusivity=0.02, wall=(1, 1.5, (0.0, -1.0, 40 * H, H / 2))),
              dict(diffusivity=0.3, wall=(2, -0.75, (0.0, H / 2, 40 * H, 2 * H)))]
    rng = np.random.default_rng(faces + 1)
    for f, fd in enumerate(fields):
        s.set_scalar_params(f, fd["diffusivity"], 0.0)
        s.set_scalar(f, rng.standard_normal(NS).astype(F))
        assert s.set_scalar_wall(f, fd["wall"][0], fd["wall"][1], fd["wall"][2]) == 40
    assert s.surface_info()["channels"] == 9
    ref, got, (u, p, fl, _) = compare(s, mesh, box, fields, what="with scalars")
    assert len(got["flux"]) == 2 and len(got["phi"]) == 2
    if faces >= 63:
        assert got["flux"][0].any() and got["flux"][1].any() == (faces in (64, 2 * NS))  # the flux wall is the top one
        ck.check(got["channels"], g, u, p, s.constants.viscosity, s.constants.density, fl)
    s.close()


def test_obstacle_bits_random_and_solved(obstacle):
    mesh = obstacle
    n = mesh.num_cells()
    assert 2000 < n < 8000
    s = flow(mesh)
    faces = s.select_surface(EVERYTHING)
    assert faces > 256  # two blocks
    body = SurfaceRef(mesh.arrays(), BODY).n
    assert 16 < body < faces
    for drive in ("u", "p"):
        random_state(s, 7, drive)
        assert s.select_surface(EVERYTHING) == faces
        compare(s, mesh, EVERYTHING, what="random " + drive + ", every wall")
        assert s.select_surface(BODY) == body
        compare(s, mesh, BODY, what="random " + drive + ", the body")
    s.set_u(np.zeros((n, 2)))
    s.initialize_history()
    for _ in range(2):
        s.step()
    _, got, _ = compare(s, mesh, BODY, what="after 2 solved steps")
    assert got["p"].any() and got["force_v"].any()
    s.select_surface(EVERYTHING)
    compare(s, mesh, EVERYTHING, what="after 2 solved steps, every wall")
    s.close()


# ------------------------------------------------------------ 2. the integrals
def test_folds_equal_the_integrals_bit_for_bit(obstacle):
    mesh = obstacle
    n = mesh.num_cells()
    s = flow(mesh)
    s.enable_scalars(2)
    inner = (0.7, 0.2, 1.0, 0.8)  # the scalar boxes lie inside the surface box
    s.set_scalar_params(0, 0.02, 0.0)
    s.set_scalar_params(1, 0.3, 0.0)
    assert s.set_scalar_wall(0, "value", 1.5, BODY) > 0
    assert 0 < s.set_scalar_wall(1, "flux", -0.75, inner) < s.set_scalar_wall(0, "value", 1.5, BODY)
    rng = np.random.default_rng(11)
    for f in range(2):
        s.set_scalar(f, rng.standard_normal(n).astype(F))
    for drive in ("u", "p", "solved"):
        if drive == "solved":  # u and p both at work
            s.set_u(np.zeros((n, 2)))
            s.initialize_history()
            s.step()
            s.step()
        else:
            random_state(s, 12, drive)
        for box in (BODY, EVERYTHING):
            faces = s.select_surface(box)
            assert s.set_force_region(*box) == faces
            ref = SurfaceRef(mesh.arrays(), box)
            ch = s.surface()["channels"]
            d = s.flow_diagnostics()
            want = [d.force_pressure[0], d.force_pressure[1], d.force_viscous[0], d.force_viscous[1]]
            for c in range(4):
                got = refpy.canon_sum(ref.fold(ch[1 + c], n))
                assert bits(got) == bits(want[c]), (drive, box, c, float(got), want[c])
            assert d.region_faces == faces
            live = dict(u=want[2:], p=want[:2], solved=want)[drive]
            assert all(w != 0.0 for w in live), (drive, want)
            for f in range(2):
                wf = s.scalar_wall_flux(f)
                got = refpy.canon_sum(ref.fold(ch[5 + 2 * f], n))
                assert wf.flux != 0.0 and bits(got) == bits(wf.flux), (drive, box, f, float(got), wf.flux)
    s.close()


# ------------------------------------------------------------- 3. moving walls
def _rotate(s, mesh, omega, scale):
    """set_wall_motion on the handle and the same selection on the restatement's side"""
    a = mesh.arrays()
    bv = BoundaryVelocities(a)
    x, y = np.asarray(a["face_cx"]), np.asarray(a["face_cy"])
    f = np.nonzero((bv.bt == 3) & (x >= BODY[0]) & (x <= BODY[2]) & (y >= BODY[1]) & (y <= BODY[3]))[0]
    xc, yc = 0.5 * (BODY[0] + BODY[2]), 0.5 * (BODY[1] + BODY[3])
    bv.set(f, np.stack([-omega * (y[f] - yc), omega * (x[f] - xc)], 1))
    bv.wall_scale = F(scale)
    assert s.set_wall_motion(BODY, omega=omega) == len(f)
    s.set_boundary_velocity_scale(1.0, scale)
    return bv, (xc, yc)


def test_moving_walls(obstacle):
    mesh = obstacle
    s = flow(mesh)
    s.select_surface(EVERYTHING)  # moved and unmoved faces in one surface
    c = s.constants
    c.time, c.ramp_time = 0.03, 0.1  # mid-ramp
    s.constants = c
    random_state(s, 21, "u")
    before = s.surface()["channels"]
    bv, centre = _rotate(s, mesh, omega=2.0, scale=0.6)
    for drive, key in (("u", "force_v"), ("p", "force_p")):
        random_state(s, 21, drive)
        s.select_surface(EVERYTHING)
        ref, got, (u, p, _, wv) = compare(s, mesh, EVERYTHING, bv=bv, what="rotating cylinder, " + drive)
        assert wv[2].sum() == SurfaceRef(mesh.arrays(), BODY).n and np.abs(wv[0][wv[2]]).max() > 0.05
        if drive == "u":
            assert not np.array_equal(got["channels"][3], before[3]) and np.array_equal(got["channels"][:3], before[:3])
        else:  # u = 0: the viscous force on a moved face is that of -u_wall
            assert got["channels"][3][wv[2]].any() and not got["channels"][3][~wv[2]].any()
        ck.check(got["channels"], s.surface_geometry(), u, p, c.viscosity, ub=wv)
        # the torque about the centre against cfd_wall_motion_get, over the body.  k_wall_motion's terms are
        # rx * fpy - ry * fpx and rx * fvy - ry * fvx of the same fpx .. fvy, summed per cell and then in the
        # canonical tree: the same terms as here, re-associated.  Two sums of n terms each within (n - 1) u sum|t|
        # of the exact sum differ by at most (n - 1) EPS sum|t|, EPS = 2u.
        body = s.select_surface(BODY)
        assert s.set_force_region(*BODY) == body
        sb = s.surface()
        g = s.surface_geometry()
        wm = s.wall_motion(*centre)
        assert wm.region_faces == body and wm.moving_faces == body
        rx, ry = g["cx"] - centre[0], g["cy"] - centre[1]
        total, tol = 0.0, 0.0
        for k, want in (("force_p", wm.torque_pressure), ("force_v", wm.torque_viscous)):
            t = rx * sb[k][:, 1] - ry * sb[k][:, 0]
            bound = (body - 1) * EPS * np.abs(t).sum()
            print(drive, k, float(t.sum()), want, abs(t.sum() - want) / max(bound, 1e-300))
            assert abs(t.sum() - want) <= bound, (drive, k)
            assert (want != 0.0) == (k == key or k == "force_v"), (drive, k)  # moving walls shear a fluid at rest
            total, tol = total + t.sum(), tol + bound
        # r x (force_p + force_v): one more rounding of the total on either side
        assert abs(total - (wm.torque_pressure + wm.torque_viscous)) <= tol + EPS * abs(total)
    random_state(s, 21, "u")
    # the empty selection: the plain instance again, and the bits it gave before the selection was made
    s.select_surface(EVERYTHING)
    s.clear_boundary_velocity()
    same_bits(s.surface()["channels"], before, "selection made and cleared")
    compare(s, mesh, EVERYTHING, what="plain instance after clearing")
    s.close()


# ------------------------------------------------------- 4. shear from the maths
def test_shear_and_cp_of_a_known_field():
    n, gamma, a, b, nu = 32, 3.0, 2.0, 0.5, 0.01
    mesh = strip(n, H)
    s = GpuSolver(mesh)
    s.set_viscosity(nu)
    xc, yc = (np.arange(n) + 0.5) * H, 0.5 * H
    gam = np.where(np.arange(n) < n // 2, gamma, -gamma)  # the shear flips half-way along
    u = np.stack([gam * yc, np.zeros(n)], 1).astype(F)
    p = (a + b * xc).astype(F)
    assert np.array_equal(p.astype(np.float64), a + b * xc)  # exact in float32: cp is linear to f64 rounding
    s.set_u(u)  # either setter clobbers the whole state: the shear first, then the pressure
    assert s.select_surface((0.0, -1.0, 100.0, H / 2)) == n  # the bottom wall
    g, sf = s.surface_geometry(), s.surface()
    assert np.array_equal(g["cell"], np.arange(n)) and np.all(g["ny"] == -1.0) and np.all(g["dist_e"] == yc)
    nu32 = float(F(nu))
    shear = sf["force_v"][:, 0] / g["area"]
    want = nu32 * u[:, 0].astype(np.float64) / g["dist_e"]  # viscosity * gamma * y_c / dist_e
    # surface_checks' bound: 8 EPS of the magnitude (three roundings in the channel, one in the division here)
    assert np.all(np.abs(shear - want) <= ck.BOUND * np.abs(want)) and np.all(np.abs(want) > 0)
    assert np.allclose(want, nu32 * gam, rtol=1e-6)  # dist_e = y_c: the wall shear stress nu du/dy
    ck.check(sf["channels"], g, u, np.zeros(n, F), nu)
    s.set_p(p)
    sp = s.surface()
    ck.check(sp["channels"], g, np.zeros((n, 2), F), p, nu)
    sf = dict(sf, p=sp["p"], force_p=sp["force_p"])
    u_ref, rho, p_ref = 1.5, 1.0, a
    c = post.coefficients(sf, g, u_ref, rho, p_ref, order=post.order_by_x(g))
    q = 0.5 * rho * u_ref ** 2
    cp_want = b * g["cx"] / q
    assert np.all(np.abs(c["cp"] - cp_want) <= ck.BOUND * (np.abs(p) + abs(p_ref)) / q)
    assert np.all(np.sign(c["cf"]) == np.sign(gam))  # t = (-ny, nx) = (1, 0) on the bottom wall
    sep = c["separation"]
    assert sep.shape == (1, 2) and g["cx"][n // 2 - 1] < sep[0, 0] < g["cx"][n // 2] and sep[0, 1] == 0.0
    s.close()


# -------------------------------------------------------------- 5. statistics
WEIGHTS = np.array([0.5, 0.125, 1.0, 0.3, 0.7, 2.0, 0.01], F)


def test_statistics():
    mesh = strip(NS, H)
    s = GpuSolver(mesh)
    s.set_viscosity(0.01)
    s.enable_scalars(1)
    s.set_scalar_params(0, 0.02, 0.0)
    s.set_scalar_wall(0, "value", 1.5, EVERYTHING)
    fields = [dict(diffusivity=0.02, wall=(1, 1.5, EVERYTHING))]
    box = STRIP_BOXES[65]
    assert s.select_surface(box) == 65
    with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
        s.accumulate_surface_stats(1.0)
    s.enable_surface_stats()
    with pytest.raises(RuntimeError, match=r"status 1.*there was none"):  # no step yet: no dt to take
        s.accumulate_surface_stats()
    for w in (float("nan"), float("inf")):
        with pytest.raises(RuntimeError, match=r"status 1.*finite"):
            s.accumulate_surface_stats(w)
    assert s.surface_info() == dict(faces=65, channels=7, samples=0, total_weight=0.0, stats_on=True)

    def drive(box, faces):
        st = SurfaceStats((7, faces))
        seq = []
        rng = np.random.default_rng(5)
        for k, w in enumerate(WEIGHTS):
            random_state(s, 100 + k, "up"[k % 2])
            s.set_scalar(0, rng.standard_normal(NS).astype(F))
            _, x, _ = restated(s, mesh, box, fields)
            s.accumulate_surface_stats(w)
            st.accumulate(x, w)
            seq.append(x)
            same_bits(s.surface_stats("mean")["channels"], st.mean, f"mean after sample {k}")
            same_bits(s.surface_stats("variance")["channels"], st.variance(), f"variance after sample {k}")
            info = s.surface_info()
            assert info["samples"] == k + 1 and bits(info["total_weight"]) == bits(st.W)
        return st, seq

    st, seq = drive(box, 65)
    # the exact weighted moments, per face and channel, within tests/tstats_checks' own bounds.  Its exact()
    # takes float32 samples: the channels that are widenings of a float32 field, p and phi, go through it
    # as they are; the other channels are float64 samples, so their exact moments are formed here in
    # rational arithmetic (the same definition) and held to the same mean_bound / cov_bound, whose
    # derivation nowhere uses the width of the samples.
    mean, var = s.surface_stats(0)["channels"], s.surface_stats(1)["channels"]
    for c in (0, 6):
        xs = [x[c].astype(F) for x in seq]
        assert all(np.array_equal(a.astype(np.float64), x[c]) for a, x in zip(xs, seq))
        TK.check_mean(mean[c], xs, WEIGHTS, f"channel {c} mean")
        TK.check_cov(var[c], xs, xs, WEIGHTS, f"channel {c} variance")
    wq = [Fraction(float(w)) for w in WEIGHTS]
    sw = sum(wq)
    K = len(WEIGHTS)
    for c in range(7):
        for j in range(65):
            xq = [Fraction(float(x[c, j])) for x in seq]
            m = sum(w * x for w, x in zip(wq, xq)) / sw
            v = sum(w * (x - m) ** 2 for w, x in zip(wq, xq)) / sw
            amax = max(abs(float(x)) for x in xq)
            assert abs(Fraction(float(mean[c, j])) - m) <= TK.mean_bound(K, amax), (c, j)
            assert abs(Fraction(float(var[c, j])) - v) <= TK.cov_bound(K, amax, amax), (c, j)
    s.reset_surface_stats()
    assert s.surface_info()["samples"] == 0 and s.surface_info()["total_weight"] == 0.0
    assert not s.surface_stats("mean")["channels"].any() and not s.surface_stats("variance")["channels"].any()
    again, _ = drive(box, 65)
    same_bits(again.mean, st.mean, "reset, then the same sequence")
    # a new selection resets, and keeps the statistics on
    assert s.select_surface(STRIP_BOXES[64]) == 64
    assert s.surface_info() == dict(faces=64, channels=7, samples=0, total_weight=0.0, stats_on=True)
    assert not s.surface_stats("mean")["channels"].any()
    drive(STRIP_BOXES[64], 64)
    s.close()


# ------------------------------------------------- 6. leaves the solver alone
def test_leaves_the_solver_alone(obstacle):
    mesh = obstacle

    def run(on):
        s = flow(mesh)
        layout = s.step_layout_bytes()
        if on:
            s.select_surface(BODY)
            s.enable_surface_stats()
            assert s.step_layout_bytes() == layout
        for _ in range(3):
            s.step()
            if on:
                s.surface()
                s.accumulate_surface_stats()
        if on:
            assert s.surface_info()["samples"] == 3
        info = s.step_info()
        info.stats_p.time_s = 0.0  # a wall-clock time
        out = s.get_u().tobytes(), s.get_p().tobytes(), bytes(info), s.step_layout_bytes()
        s.close()
        return out

    assert run(True) == run(False)


# -------------------------------------------------------------- 7. refusals
def test_refusals_change_nothing(obstacle):
    mesh = strip(NS, H)
    s = GpuSolver(mesh)
    s.set_viscosity(0.01)
    random_state(s, 3, "u")
    for call in (s.surface, s.surface_info, s.surface_geometry, s.enable_surface_stats, s.reset_surface_stats,
                 lambda: s.accumulate_surface_stats(1.0), s.surface_stats):
        with pytest.raises(RuntimeError, match=r"status 1.*no surface is selected"):
            call()
    box = STRIP_BOXES[64]
    assert s.select_surface(box) == 64
    want = s.surface()["channels"]
    for call in (s.surface_stats, lambda: s.surface_stats("variance"), s.reset_surface_stats,
                 lambda: s.accumulate_surface_stats(1.0)):
        with pytest.raises(RuntimeError, match=r"status 1.*not enabled"):
            call()
    s.enable_surface_stats()
    with pytest.raises(RuntimeError, match=r"status 1.*kind"):
        s.surface_stats(2)
    with pytest.raises(ValueError):
        s.surface_stats("rms")
    same_bits(s.surface()["channels"], want, "after the refused calls")
    # an inverted box clears the surface
    assert s.select_surface((1.0, 0.0, 0.0, 1.0)) == 0
    with pytest.raises(RuntimeError, match=r"status 1.*no surface is selected"):
        s.surface()
    assert s.select_surface(box) == 64 and s.surface_info()["stats_on"] is False
    # the rule for configuration changes under a surface: accepted, the channels re-derived, the statistics reset
    s.enable_surface_stats()
    s.accumulate_surface_stats(0.5)
    assert s.surface_info() == dict(faces=64, channels=5, samples=1, total_weight=0.5, stats_on=True)
    s.enable_scalars(2)
    assert s.surface_info() == dict(faces=64, channels=9, samples=0, total_weight=0.0, stats_on=True)
    assert not s.surface_stats("mean")["channels"].any()
    got = s.surface()["channels"]
    same_bits(got[:5], want, "the first five channels with scalars on")
    assert got.shape == (9, 64) and not got[5:].any()
    s.accumulate_surface_stats(0.25)
    s.set_scalar_params(0, 0.02, 0.0)
    assert s.surface_info()["samples"] == 1  # a parameter resets nothing
    s.set_scalar_wall(0, "value", 1.0, EVERYTHING)
    assert s.surface_info()["samples"] == 0 and s.surface()["flux"][0].any()
    s.accumulate_surface_stats(0.25)
    s.set_wall_motion(EVERYTHING, velocity=(1.0, 0.0))
    assert s.surface_info()["samples"] == 0
    s.accumulate_surface_stats(0.25)
    s.set_boundary_velocity_scale(1.0, 0.5)  # a parameter, not the selection: nothing resets
    s.set_viscosity(0.02)
    assert s.surface_info()["samples"] == 1
    s.clear_boundary_velocity()
    s.set_viscosity(0.01)
    s.enable_scalars(0)
    assert s.surface_info() == dict(faces=64, channels=5, samples=0, total_weight=0.0, stats_on=True)
    same_bits(s.surface()["channels"], want, "scalars and moving walls off again")
    s.close()
    # distributed handles: a 2-rank group and each of its members
    g = GpuGroup(obstacle, 2)
    with pytest.raises(RuntimeError, match=r"one GPU only"):
        g.select_surface(BODY)
    for name in ("surface", "surface_geometry", "surface_info", "enable_surface_stats", "reset_surface_stats",
                 "accumulate_surface_stats", "surface_stats"):
        with pytest.raises(AttributeError):  # none of the new names is forwarded to the ranks
            getattr(g, name)
    for r in g.ranks:
        for call in (lambda: r.select_surface(BODY), r.surface, r.surface_info, r.surface_geometry,
                     r.enable_surface_stats, r.reset_surface_stats, r.accumulate_surface_stats, r.surface_stats):
            with pytest.raises(RuntimeError, match=r"status 1.*surface distributions run on one GPU only"):
                call()
    g.close()
