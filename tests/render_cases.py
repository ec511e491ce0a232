"""The render cases shared by the CPU and the GPU tests: a mesh, an image size
and a view box each, with the numpy restatement's ownership map computed once
per case."""
import functools

import numpy as np

from cfd2_amd.mesh import RectangularChannel, generate_cut_cell_mesh, generate_voronoi_mesh
from tests import render_ref as R
from tests.meshes import STEP, bench_mesh, channel_obstacle

# name -> (mesh name, W, H, box (x0, y0, x1, y1) or None for the polygons' bounds)
CASES = {
    "rect": ("rect", 64, 32, None),                    # < 64 cells of ~9 x 8 pixels: every cell takes the wavefront path
    "obstacle": ("obstacle", 96, 32, None),            # mixed paths; the obstacle's hole is background
    # fewer pixels than one wavefront; most cells own nothing.  (Its box is a little inside the domain: over the
    # whole 3 x 1 domain the five rows of centres lie exactly on the mesh's grid lines, which is "on_edges" below.)
    "obstacle_7x5": ("obstacle", 7, 5, (0.02, 0.013, 2.97, 0.981)),
    # every centre on a grid line of the mesh, most on a vertex: ties between up to four cells, the largest index
    # winning.  The float64 check cannot decide such pixels (UNCAPPED: no cap on the undecided share, the three
    # violation counts still have to be zero); the GPU has to give the restatement's bits.
    "on_edges": ("obstacle", 15, 5, None),
    "voronoi": ("voronoi", 160, 48, None),             # fans of 5 to 8 vertices
    "zoom": ("obstacle", 33, 17, (0.33, 0.21, 0.48, 0.29)),    # ~1.5 cells: boxes far larger than the image, clipped
    "half_outside": ("obstacle", 48, 24, (-0.5, -0.3, 1.0, 0.6)),  # background pixels inside the image
    "outside": ("obstacle", 16, 8, (4.0, 2.0, 5.0, 3.0)),      # covered == 0, the image all zero
    "one_pixel": ("obstacle", 1, 1, (1.42, 0.42, 1.52, 0.5)),  # the smallest image (its centre inside a cell)
    "big": ("big", 128, 64, None),                     # >= 65 536 cells, many per pixel: contention, the largest-index rule
}


UNCAPPED = {"on_edges"}


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "rect":
        return generate_cut_cell_mesh(RectangularChannel(length=1.0, height=0.5), 0.15, 0.15, 1.2, (1.0, 0.5))
    if name == "obstacle":
        return channel_obstacle(h=0.1)
    if name == "voronoi":
        return generate_voronoi_mesh(STEP, 0.12, 0.12, 1.2, (3.5, 1.0), seed=7)
    if name == "big":
        return bench_mesh(0.0066, 0)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def polygons_of(name):
    return R.mesh_polygons(mesh_of(name))


@functools.lru_cache(maxsize=None)
def case(name):
    """mesh, W, H, the box as given (None: default), the box in numbers, the restatement's map (read-only)"""
    mname, W, H, box = CASES[name]
    vx, vy, off, idx = polygons_of(mname)
    full = box if box is not None else R.bounds(vx, vy, idx)
    owner = R.owner_map(vx, vy, off, idx, R.View(W, H, full))
    owner.setflags(write=False)
    return mesh_of(mname), W, H, box, full, owner


def nan_cell(mesh):
    return mesh.num_cells() // 2


def with_nan(mesh, u, p):
    """a state with one NaN cell (u and p), for the NaN colour"""
    u, p = np.array(u, np.float64), np.array(p, np.float64)
    u[nan_cell(mesh)] = np.nan
    p[nan_cell(mesh)] = np.nan
    return u, p
