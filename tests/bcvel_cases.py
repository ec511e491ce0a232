"""Cases shared by tests/test_bcvel.py (CPU: the restatement tests/bcvel_ref.py
against the float64 checks tests/bcvel_checks.py) and tests/test_gpu_bcvel.py
(the HIP path against both).  HELPER MODULE, not a test.

Meshes, the smallest on which the kernels can still go wrong:
  rect       RectangularChannel 8 x 6 cells: each inlet corner cell holds an inlet
             slot and a wall slot in ONE cell (one table row, two entries)
  obstacle   channel_obstacle(h = 0.05), a cut-cell mesh of 1-2 k cells: N no
             multiple of 64 or 256, the obstacle's walls on cut cells of 5 faces
  voronoi    a Voronoi channel with an obstacle, about 300 cells: non-orthogonal,
             5 to 9 faces per cell, every third normal stored against the flux
             direction (the arithmetic takes a normal as stored; the mesher
             never stores one that way)
  obstacle_perm  obstacle renumbered at random: the cells with a selected slot
             are scattered over the waves, and rows of the compact table follow
             cell order, not face order; asserted to straddle a 64-cell boundary

The standard selection (`select`): a rigid rotation of the obstacle's walls (or
of the bottom wall where there is no obstacle: a belt), a sheared and slanted
inlet profile with v != 0, and scales 0.75 / 1.25, so that no factor is 1 and
no component 0.
"""
import functools

import numpy as np

from cfd2_amd.mesh import ChannelWithObstacle, RectangularChannel, generate_cut_cell_mesh, generate_voronoi_mesh
from tests import refpy
from tests.meshes import channel_obstacle
from tests.synthetic import ArrayMesh, perm_random, renumbered

F = np.float32
MESHES = ["rect", "obstacle", "voronoi", "obstacle_perm"]
# (time_scheme, scheme): every pair the issue names
SCHEMES = [(ts, sc) for ts in (0, 1) for sc in (0, 1, 2)]
FIXED = dict(fixed_outer=2, fixed_inner=6)
DENSITY = 1.5  # not 1: a dropped density shows
OBSTACLE_BOX = (0.7, 0.2, 1.3, 0.8)
OBSTACLE_CENTRE = (1.0, 0.5)
OMEGA = 2.0
SCALES = (0.75, 1.25)
H_RECT, L_RECT = 0.75, 1.0


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "rect":
        return generate_cut_cell_mesh(RectangularChannel(length=L_RECT, height=H_RECT), 0.125, 0.125, 1.2,
                                      (L_RECT, H_RECT))
    if name == "obstacle":
        return channel_obstacle(h=0.05)
    if name == "voronoi":
        geo = ChannelWithObstacle(length=3.0, height=1.0, obstacle_center=OBSTACLE_CENTRE, obstacle_radius=0.2)
        base = generate_voronoi_mesh(geo, 0.09, 0.09, 1.2, (3.0, 1.0), seed=11)
        # the mesher stores every normal along the flux direction: every third face
        # (inlet, wall and internal ones among them) gets its normal stored the other way
        a = {k: np.array(v, copy=True) for k, v in base.arrays().items()}
        a["face_nx"][::3] *= -1.0
        a["face_ny"][::3] *= -1.0
        return ArrayMesh(**a)
    if name == "obstacle_perm":
        base = mesh_of("obstacle")
        return renumbered(base, perm_random(base.num_cells()))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def refmesh_of(name):
    return refpy.RefMesh(mesh_of(name))


def boundary_faces(arrays, kind):
    a = arrays
    return np.nonzero((a["face_neighbor"] == refpy.NONE) & ((a["face_boundary"] & 3) == kind))[0]


def check_shape(name):
    """the properties the case list promises"""
    mesh = mesh_of(name)
    a = mesh.arrays()
    n = mesh.num_cells()
    deg = np.diff(a["cell_face_offsets"])
    inlet, wall = boundary_faces(a, 1), boundary_faces(a, 3)
    if name == "rect":
        assert n == 48
        both = np.intersect1d(a["face_owner"][inlet], a["face_owner"][wall])
        assert len(both) == 2  # the two inlet corners
    elif name.startswith("obstacle"):
        assert 1000 <= n <= 2000 and n % 64 != 0 and n % 256 != 0
        x, y = a["face_cx"][wall], a["face_cy"][wall]
        on = (x >= OBSTACLE_BOX[0]) & (x <= OBSTACLE_BOX[2]) & (y >= OBSTACLE_BOX[1]) & (y <= OBSTACLE_BOX[3])
        cells = a["face_owner"][wall[on]]
        assert deg[cells].max() > 4
        if name.endswith("_perm"):
            assert len(np.unique(cells // 64)) > 1  # the selected cells straddle a wave boundary
    elif name == "voronoi":
        assert 200 <= n <= 450 and deg.min() <= 5 and deg.max() >= 7
        M = refmesh_of(name)
        o = M.own
        against = (M.fx - M.cx[o]) * M.nx + (M.fy - M.cy[o]) * M.ny < 0  # stored against the flux
        assert np.any(against[boundary_faces(a, 1)]) and np.any(against[boundary_faces(a, 3)])


def fields(mesh):
    """u [N, 2]: smooth, non-zero in both components"""
    a = mesh.arrays()
    x, y = a["cell_cx"], a["cell_cy"]
    return np.stack([0.8 + 0.5 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y),
                     0.3 * np.cos(1.3 * x) * np.sin(2.9 * y + 0.2)], 1)


def setup_flow(s, mesh, time_scheme=0, scheme=0, density=DENSITY, precond=0, time=0.04):
    """a non-trivial state in the middle of the inlet ramp, history initialised"""
    s.set_dt(2e-3)
    s.set_dt(1e-3)  # dt_old = 2e-3: a non-trivial BDF2 ratio
    s.set_viscosity(0.01)
    s.set_density(density)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(precond)
    s.set_scheme(scheme)
    s.set_time_scheme(time_scheme)
    c = s.constants
    c.inlet_velocity = 1.3
    c.ramp_time = 0.1
    c.time = time
    s.constants = c
    s.set_u(fields(mesh))
    s.initialize_history()


def inlet_profile(x, y):
    """sheared, slanted: u and v both vary along the inlet"""
    return 0.6 + 1.1 * y * (1.0 - 0.4 * y), 0.2 - 0.3 * y


def wall_box(name):
    """the moving walls of the standard selection, and their motion"""
    if name == "rect":  # the bottom wall as a belt with a normal part the host must remove
        return dict(box=(0.0, -1e-9, L_RECT, 1e-9), velocity=(0.9, 0.05), omega=0.0, centre=None)
    return dict(box=OBSTACLE_BOX, velocity=(0.1, -0.05), omega=OMEGA, centre=OBSTACLE_CENTRE)


def select(s, name, scales=SCALES):
    """the standard selection on solver s (GpuSolver or BcvRefSolver); returns the faces selected"""
    s.set_inlet_profile(inlet_profile)
    n = s.set_wall_motion(**wall_box(name))
    s.set_boundary_velocity_scale(*scales)
    s.set_force_region(*wall_box(name)["box"])
    return n


def selection_arrays(mesh, name):
    """(faces, v [n, 2] float64) of the standard selection, as set_inlet_profile and
    set_wall_motion form them (before the wall projection)"""
    a = mesh.arrays()
    inlet, wall = boundary_faces(a, 1), boundary_faces(a, 3)
    u, v = inlet_profile(a["face_cx"][inlet], a["face_cy"][inlet])
    w = wall_box(name)
    x0, y0, x1, y1 = w["box"]
    x, y = a["face_cx"][wall], a["face_cy"][wall]
    on = wall[(x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)]
    xc, yc = (0.5 * (x0 + x1), 0.5 * (y0 + y1)) if w["centre"] is None else w["centre"]
    U, V = w["velocity"]
    vw = np.stack([U - w["omega"] * (a["face_cy"][on] - yc), V + w["omega"] * (a["face_cx"][on] - xc)], 1)
    return np.concatenate([inlet, on]), np.concatenate([np.stack([u, v], 1), vw])


# ---- the Couette case -----------------------------------------------------------
COUETTE = dict(U=1.0, steps=5, dt=0.01, viscosity=0.05)


def setup_couette(s, mesh, sign_ok=True):
    """RectangularChannel, the top wall moving at U, the inlet profile U y / H, the
    initial field the same: the linear profile solves the discrete equations on
    the uniform mesh exactly (a linear face interpolation and a central wall
    gradient are exact for it, the convection of u along x vanishes)."""
    U = COUETTE["U"]
    a = mesh.arrays()
    s.set_dt(COUETTE["dt"])
    s.set_dt(COUETTE["dt"])
    s.set_viscosity(COUETTE["viscosity"])
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    s.set_scheme(0)
    s.set_time_scheme(0)
    c = s.constants
    c.inlet_velocity = 0.0
    c.ramp_time = 0.1
    c.time = 1.0  # past the ramp
    s.constants = c
    s.set_u(np.stack([U * a["cell_cy"] / H_RECT, 0.0 * a["cell_cy"]], 1))
    s.initialize_history()
    s.set_inlet_profile(lambda x, y: (U * y / H_RECT, 0.0 * y))
    s.set_wall_motion((0.0, H_RECT - 1e-9, L_RECT, H_RECT + 1e-9), velocity=(U, 0.0))


def couette_deviation(s, mesh):
    """max |u - (U y / H, 0)| over the cells"""
    a = mesh.arrays()
    u = np.asarray(s.get_u(), np.float64).reshape(-1, 2)
    exact = np.stack([COUETTE["U"] * a["cell_cy"] / H_RECT, 0.0 * a["cell_cy"]], 1)
    return float(np.abs(u - exact).max())


# ---- the float64 checks on either solver ------------------------------------------
def outputs(s):
    """debug_prepare_assemble on solver s (GpuSolver or BcvRefSolver): the float64
    images of what the checks read"""
    d = np.float64
    if hasattr(s, "debug_buffer"):
        s.debug_prepare_assemble()
        buf = lambda i: np.asarray(s.debug_buffer(i), d)  # noqa: E731
        fd = s.flow_diagnostics()
        return dict(flux=buf(0), grad_u=buf(1).reshape(-1, 2), grad_v=buf(2).reshape(-1, 2), rhs=buf(3),
                    u_old=buf(11).reshape(-1, 2), u_old_old=buf(12).reshape(-1, 2),
                    force_viscous=tuple(fd.force_viscous), motion=tuple(s.wall_motion(*OBSTACLE_CENTRE))[:3])
    o = s.debug_prepare_assemble()
    return dict(flux=o["fluxes"].astype(d), grad_u=o["grad_u"].astype(d), grad_v=o["grad_v"].astype(d),
                rhs=o["rhs"].astype(d), u_old=s.ring[s.i_old].u.astype(d), u_old_old=s.ring[s.i_old_old].u.astype(d),
                force_viscous=tuple(s.wall_force()[1]), motion=s.wall_motion(*OBSTACLE_CENTRE)[:3])


def run_checks(s, name, time_scheme, wrong=(), worst=None):
    """the standard selection on a fresh state of solver s, then every check of
    tests/bcvel_checks.py; returns the worst error / bound per check"""
    from tests import bcvel_checks as ck
    from tests import flow_checks as fc
    mesh = mesh_of(name)
    a = mesh.arrays()
    setup_flow(s, mesh, time_scheme=time_scheme, scheme=0)
    select(s, name)
    u = np.asarray(s.get_u(), np.float64).reshape(-1, 2).copy()
    p = np.asarray(s.get_p(), np.float64).copy()
    out = outputs(s)
    g = fc.Geometry(a)
    c = fc.Constants(s.constants)
    faces, v = selection_arrays(mesh, name)
    B = ck.Boundary(g, s.constants, faces, ck.uploaded(a, faces, v, wrong), SCALES, wrong)
    x, y = a["face_cx"], a["face_cy"]
    x0, y0, x1, y1 = wall_box(name)["box"]
    region = (g.kind == fc.WALL) & (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    res = dict(
        flux=ck.check_inlet_flux(g, c, B, out["flux"]),
        gradients=ck.check_gradients(g, B, u, out["grad_u"], out["grad_v"]),
        rhs=ck.check_rhs(g, c, B, out["flux"], out["u_old"], out["u_old_old"], out["rhs"]),
        wall=ck.check_wall_sums(g, c, B, a, region, u, p, *OBSTACLE_CENTRE, out["force_viscous"], out["motion"]))
    if worst is not None:
        for k, r in res.items():
            worst[k] = max(worst.get(k, 0.0), r)
    return res


# ---- physics signs: a rotating cylinder -------------------------------------------
ROTATION = dict(omega=3.0, dt=0.01, viscosity=0.01, steps_power=1, steps_lift=3)


def _rotating(s, omega, inlet):
    s.set_dt(ROTATION["dt"])
    s.set_dt(ROTATION["dt"])
    s.set_viscosity(ROTATION["viscosity"])
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    c = s.constants
    c.inlet_velocity = inlet
    c.ramp_time = 0.02
    s.constants = c
    s.initialize_history()
    s.set_force_region(*OBSTACLE_BOX)
    if omega:
        s.set_wall_motion(OBSTACLE_BOX, omega=omega, centre=OBSTACLE_CENTRE)


def _lift(s):
    if hasattr(s, "flow_diagnostics"):
        d = s.flow_diagnostics()
        return d.force_pressure[1] + d.force_viscous[1]
    fp, fv = s.wall_force()
    return fp[1] + fv[1]


def rotation_signs(make):
    """make(): a fresh solver on the obstacle mesh.  (lift {0, +1, -1} after
    steps_lift steps in a stream, power {+1, -1} after steps_power steps from rest)"""
    lift, power = {}, {}
    for sgn in (0, +1, -1):
        s = make()
        _rotating(s, sgn * ROTATION["omega"], 1.0)
        for _ in range(ROTATION["steps_lift"]):
            s.step()
        lift[sgn] = _lift(s)
        if sgn:
            s = make()
            _rotating(s, sgn * ROTATION["omega"], 0.0)
            for _ in range(ROTATION["steps_power"]):
                s.step()
            power[sgn] = tuple(s.wall_motion(*OBSTACLE_CENTRE))[2]
    return lift, power
