"""Cases shared by tests/test_buoyancy.py (CPU: the restatement against itself)
and tests/test_gpu_buoyancy.py (HIP path).  HELPER MODULE, not a test.

Meshes: tests/test_gpu_scalar.py's rect (fewer than 64 cells), obstacle (not a
multiple of 64), voronoi (5 to 9 faces per cell) and units4 (68,497 cells: 67
reduction blocks, units of 4 chunks), and tests/scalar_cases.py's strips of 1, 2
and 130 cells (N = 1, and a block tail).

The plume case (check 5 of the GPU test, check 4 of the CPU test, which settled
it): the obstacle mesh at rest with inlet_velocity = 0, the obstacle's faces
held at phi = 1, D = 0.02, dt = 0.02, beta = 1, K = 4 alternating step() /
advance_scalars().  The first step sees phi = 0 and stays at rest; each advance
heats another layer of cells around the obstacle.  ABOVE is the box directly
above the obstacle (centre (1.0, 0.5), radius 0.2, channel height 1).
"""
import functools

import numpy as np

from tests import refpy
from tests.scalar_cases import mesh_of as _strip
from tests.test_gpu_scalar import _fields, _mesh

F = np.float32
MESHES = ["rect", "obstacle", "voronoi", "units4"]
STRIPS = ["strip1", "strip2", "strip130"]
# (time_scheme, scheme)
SCHEMES = [(0, 0), (1, 0), (0, 2)]
FIXED = dict(fixed_outer=2, fixed_inner=6)
DENSITY = 1.5  # not 1: a dropped density shows
BETA, REF, G = 0.5, 0.2, (0.3, -9.81)
INLET_VALUE, DIFFUSIVITY = 0.25, 0.01

PLUME = dict(K=4, dt=0.02, beta=1.0, D=0.02, viscosity=0.01, wall_value=1.0, g=(0.0, -9.81))
OBSTACLE_BOX = (0.7, 0.2, 1.3, 0.8)
ABOVE = (0.8, 0.7, 1.2, 1.0)


def mesh_of(name):
    return _strip(name) if name.startswith("strip") else _mesh(name)


@functools.lru_cache(maxsize=None)
def refmesh_of(name):
    return refpy.RefMesh(mesh_of(name))


def fields(mesh):
    """(u [N, 2], phi [N]): tests/test_gpu_scalar.py's smooth profiles"""
    return _fields(mesh)


def second_field(mesh):
    a = mesh.arrays()
    return 1.0 - 0.6 * np.cos(1.9 * a["cell_cx"]) * np.sin(2.7 * a["cell_cy"] + 0.1)


def setup_flow(s, mesh, time_scheme=0, scheme=0, density=DENSITY, precond=0):
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
    c.time = 0.04
    s.constants = c
    s.set_u(fields(mesh)[0])
    s.initialize_history()


def setup_scalars(s, mesh, two=False):
    """one driving field (two: a second one with another beta and ref), non-uniform, with an inlet value"""
    s.enable_scalars(2 if two else 1)
    s.set_scalar_params(0, DIFFUSIVITY, INLET_VALUE)
    s.set_scalar(0, fields(mesh)[1])
    s.set_scalar_buoyancy(0, BETA, REF)
    if two:
        s.set_scalar_params(1, 0.0, 1.0)
        s.set_scalar(1, second_field(mesh))
        s.set_scalar_buoyancy(1, -0.125, 0.7)
    s.set_gravity(*G)


def setup_plume(s, beta, g):
    s.set_dt(PLUME["dt"])
    s.set_viscosity(PLUME["viscosity"])
    s.set_density(1.0)
    s.set_alpha_u(0.7)
    s.set_alpha_p(0.3)
    s.set_precond_type(0)
    c = s.constants
    c.inlet_velocity = 0.0
    s.constants = c
    s.initialize_history()
    s.enable_scalars(1)
    s.set_scalar_params(0, PLUME["D"], 0.0)
    faces = s.set_scalar_wall(0, "value", PLUME["wall_value"], OBSTACLE_BOX)
    assert faces > 0
    s.set_scalar_buoyancy(0, beta, 0.0)
    s.set_gravity(*g)


def run_plume(s, mesh, beta, g):
    """K alternating steps; the volume-weighted mean of v over the cells in ABOVE and max |u|"""
    setup_plume(s, beta, g)
    for _ in range(PLUME["K"]):
        s.step()
        s.advance_scalars()
    a = mesh.arrays()
    x, y, vol = a["cell_cx"], a["cell_cy"], a["cell_vol"]
    box = (x >= ABOVE[0]) & (x <= ABOVE[2]) & (y >= ABOVE[1]) & (y <= ABOVE[3])
    assert box.sum() >= 4
    u = np.asarray(s.get_u()).reshape(-1, 2)
    return float((vol[box] * u[box, 1]).sum() / vol[box].sum()), float(np.abs(u).max())
