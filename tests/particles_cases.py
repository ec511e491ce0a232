"""The particle cases shared by the CPU and the GPU tests: a mesh, a frozen
velocity field, seeds, a dt and a number of advances each.  The numpy
restatement's result is computed once per case and shared read-only."""
import functools

import numpy as np

from cfd2_amd.mesh import ChannelWithObstacle, Mesh, RectangularChannel, generate_cut_cell_mesh, generate_voronoi_mesh
from tests import particles_ref as R
from tests.meshes import STEP, backwards_step, channel_obstacle

F = np.float32


def write_mesh_file(path, vertices, cells, length):
    """a mesh written down by hand, as a mesh file (the format of Mesh.save: the
    magic, then per array a 64-bit count and the values) for Mesh.load.  cells:
    CCW vertex lists; the faces are the polygons' edges, owned by the lower cell
    and running in its CCW order; a boundary face is the inlet (1) at x = 0, the
    outlet (2) at x = length, a wall (3) elsewhere."""
    v = np.array(vertices, np.float64)
    key, faces = {}, []  # (v1, v2, owner, neighbour)
    cell_faces = []
    for c, poly in enumerate(cells):
        mine = []
        for a, b in zip(poly, poly[1:] + poly[:1]):
            k = (min(a, b), max(a, b))
            if k in key:
                faces[key[k]][3] = c
            else:
                key[k] = len(faces)
                faces.append([a, b, c, R.NONE])
            mine.append(key[k])
        cell_faces.append(mine)
    f = np.array(faces, np.int64)
    p1, p2 = v[f[:, 0]], v[f[:, 1]]
    d, mid = p2 - p1, 0.5 * (p1 + p2)
    L = np.hypot(d[:, 0], d[:, 1])
    code = np.where(f[:, 3] != R.NONE, 0, np.where(mid[:, 0] == 0.0, 1, np.where(mid[:, 0] == length, 2, 3)))
    area, cen = [], []
    for poly in cells:
        q = v[poly]
        x, y, xn, yn = q[:, 0], q[:, 1], np.roll(q[:, 0], -1), np.roll(q[:, 1], -1)
        w = x * yn - xn * y
        area.append(0.5 * w.sum())
        cen.append((((x + xn) * w).sum() / (3.0 * w.sum()), ((y + yn) * w).sum() / (3.0 * w.sum())))
    cen = np.array(cen)
    fixed = np.zeros(len(v), np.uint8)
    fixed[f[f[:, 3] == R.NONE][:, :2].ravel()] = 1
    u32, f64 = np.uint32, np.float64
    arrays = [(v[:, 0], f64), (v[:, 1], f64), (fixed, np.uint8), (f[:, 0], u32), (f[:, 1], u32), (f[:, 2], u32),
              (f[:, 3], u32), (code, u32), (d[:, 1] / L, f64), (-d[:, 0] / L, f64), (L, f64), (mid[:, 0], f64),
              (mid[:, 1], f64), (cen[:, 0], f64), (cen[:, 1], f64), (np.array(area), f64),
              (np.concatenate(cell_faces), u32), (np.cumsum([0] + [len(k) for k in cell_faces]), u32),
              (np.concatenate(cells), u32), (np.cumsum([0] + [len(k) for k in cells]), u32)]
    with open(path, "wb") as fh:
        fh.write(b"CFDMESH1")
        for a, dt in arrays:
            fh.write(np.uint64(len(a)).tobytes())
            fh.write(np.ascontiguousarray(a, dt).tobytes())


REFLEX_H = (0.65, 0.5)


def reflex_mesh():
    """2 x 1 in squares of 0.25, columns by rows like the generated channels, left
    inlet, right outlet, walls below and above: 31 cells.  In the block
    [0.5, 1] x [0.25, 0.75] the two squares of the left column are one coarse
    cell A, whose east side has the hanging node H between its two fine
    neighbours B (below) and C (above); H is moved from (0.75, 0.5) to
    (0.65, 0.5), far more than the smoothing moves one, so A is reflex at H.
    The lines of A's faces to B and to C run on through A's interior, and a
    point of A is beyond one of them over a whole region.  No generator makes
    such a cell (their cells are all convex), so the mesh is written as a mesh
    file and loaded: a handle can be made of it like of any other."""
    import os
    import tempfile
    h, nx, ny = 0.25, 8, 4
    vid, verts = {}, []

    def V(i, j):  # the grid vertex (i, j)
        if (i, j) not in vid:
            vid[(i, j)] = len(verts)
            verts.append(REFLEX_H if (i, j) == (3, 2) else (i * h, j * h))
        return vid[(i, j)]

    cells = []
    for i in range(nx):
        for j in range(ny):
            if (i, j) == (2, 1):    # A: two squares, H on the east side, the plain hanging node (2, 2) on the west
                cells.append([V(2, 1), V(3, 1), V(3, 2), V(3, 3), V(2, 3), V(2, 2)])
            elif (i, j) != (2, 2):  # (2, 2) is A's upper half
                cells.append([V(i, j), V(i + 1, j), V(i + 1, j + 1), V(i, j + 1)])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "reflex.mesh")
        write_mesh_file(path, verts, cells, nx * h)
        return Mesh.load(path)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "reflex":
        return reflex_mesh()
    if name == "obstacle":
        return channel_obstacle(h=0.05)            # ~1,100 cells, 3 x 1, a disc of r = 0.2 at (1, 0.5)
    if name == "step":
        return backwards_step(h=0.05)              # 3.5 x 1, the step to x = 0.5 below y = 0.5
    if name == "voronoi":
        return generate_voronoi_mesh(STEP, 0.12, 0.12, 1.2, (3.5, 1.0), seed=7)  # a few hundred cells of 5..9 faces
    if name == "rect":
        return generate_cut_cell_mesh(RectangularChannel(length=1.0, height=0.5), 0.15, 0.15, 1.2, (1.0, 0.5))  # < 64 cells
    if name == "graded":                           # quadtree level jumps: hanging nodes, moved by the smoothing
        geo = ChannelWithObstacle(length=3.0, height=1.0, obstacle_center=(1.0, 0.5), obstacle_radius=0.2)
        m = generate_cut_cell_mesh(geo, 0.06, 0.24, 1.2, (3.0, 1.0))
        m.smooth(geo, 0.3, 50)
        return m
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def pmesh_of(name):
    return R.PMesh(mesh_of(name))


def field(mesh, kind):
    """the frozen cell velocities (N, 2) float64 of a field kind"""
    a = mesh.arrays()
    cx, cy = np.array(a["cell_cx"]), np.array(a["cell_cy"])
    if isinstance(kind, tuple):
        return np.tile(np.array(kind, np.float64), (len(cx), 1))
    if kind == "shear":
        return np.stack([0.5 + cy, 0.0 * cy], 1)
    if kind == "solid":  # solid-body rotation about (1.75, 0.5)
        return np.stack([-(cy - 0.5), cx - 1.75], 1)
    raise KeyError(kind)


def _box_seeds(n, box, seed):
    rng = np.random.default_rng(seed)
    x0, y0, x1, y1 = box
    return np.stack([rng.uniform(x0, x1, n), rng.uniform(y0, y1, n)], 1)


# name -> dict(mesh, field, seeds (n, 2), dt, steps, hop_cap, kind)
#   kind: which float64 check applies besides containment
CASES = {
    # 257 particles over the whole channel, some into the obstacle (they slide round it)
    "uniform_obstacle": dict(mesh="obstacle", field=(1.0, 0.0), n=257, box=(0.05, 0.05, 2.5, 0.95), dt=0.3, kind="uniform"),
    # level jumps and smoothed hanging nodes, an oblique field
    "uniform_graded": dict(mesh="graded", field=(1.0, 0.125), n=65, box=(0.05, 0.05, 2.2, 0.7), dt=0.4, kind="uniform"),
    "uniform_voronoi": dict(mesh="voronoi", field=(1.0, 0.0), n=64, box=(0.6, 0.05, 2.6, 0.95), dt=0.5, kind="uniform"),
    "rect_one": dict(mesh="rect", field=(0.5, 0.125), n=1, box=(0.2, 0.1, 0.3, 0.2), dt=0.5, kind="uniform"),
    "exit_outlet": dict(mesh="step", field=(2.0, 0.0), n=63, box=(2.6, 0.05, 3.4, 0.95), dt=1.0, kind="outlet", line=3.5),
    "exit_inlet": dict(mesh="obstacle", field=(-2.0, 0.0), n=63, box=(0.05, 0.05, 0.7, 0.95), dt=1.0, kind="inlet", line=0.0),
    "wall": dict(mesh="rect", field=(1.0, -0.5), n=64, box=(0.05, 0.05, 0.4, 0.2), dt=0.5, kind="wall", line=0.0),
    "shear_voronoi": dict(mesh="voronoi", field="shear", n=65, box=(0.6, 0.05, 2.4, 0.95), dt=0.25, steps=2, kind="split"),
    "solid_voronoi": dict(mesh="voronoi", field="solid", n=63, box=(1.5, 0.25, 2.0, 0.75), dt=0.25, steps=2, kind="split"),
    # the reflex cell: the seeds start in the column west of A; the paths enter A and end between x = 0.55 and 0.7: some
    # in B or C, some in A short of the lines of A's faces to B and C, most in A beyond one of them
    "uniform_reflex": dict(mesh="reflex", field=(1.0, 0.0), n=63, box=(0.3, 0.3, 0.45, 0.7), dt=0.25, kind="uniform"),
    "cap2": dict(mesh="obstacle", field=(1.0, 0.0), n=65, box=(0.05, 0.05, 1.5, 0.95), dt=1.0, hop_cap=2, kind="cap"),
}


def case_of(name):
    return CASES[name]


@functools.lru_cache(maxsize=None)
def on_wall_of(mname):
    """on_wall for check_containment: cell -> which of its polygon's edges lie on
    the domain's boundary (an ALIVE particle there is on a wall: the others left)"""
    from tests import particles_checks as K
    pm = pmesh_of(mname)
    edges = K.boundary_edges(pm.off, pm.idx)

    def on_wall(c):
        p = pm.idx[pm.off[c]:pm.off[c + 1]].tolist()
        return np.array([(min(a, b), max(a, b)) in edges for a, b in zip(p, p[1:] + p[:1])])
    return on_wall


# the rake of the solved-flow test: 65 seeds upstream of the obstacle, off the mesh's lines (the cells there are
# squares of 0.05: x = 0.42 is on no vertical line, and no y = 0.21 + k 0.57 / 64 is a multiple of 0.05, the centre
# seed at 0.495 included, which a symmetric rake would leave on the edge y = 0.5 for good)
RAKE = np.stack([np.full(65, 0.42), np.linspace(0.21, 0.78, 65)], 1)
RAKE_DT = 0.02


def seeds_of(name):
    c = case_of(name)
    return _box_seeds(c["n"], c["box"], seed=sum(map(ord, name)))


def run(name, pm=None, seeds=None, dt_parts=1, **wrong):
    """the restatement's run of a case: the Set after the case's advances (each
    split into dt_parts equal parts), and the hops / capped summed over them"""
    c = case_of(name)
    pm = pm or pmesh_of(c["mesh"])
    seeds = seeds_of(name) if seeds is None else seeds
    u = field(mesh_of(c["mesh"]), c["field"]).astype(F)
    P = R.Set(len(seeds), c.get("hop_cap", 64))
    P.seed(pm, seeds, owner=wrong.pop("owner", "largest"))
    hops, capped = np.zeros(P.n, np.int64), np.zeros(P.n, bool)
    for _ in range(c.get("steps", 1) * dt_parts):
        R.advance(pm, u, P, F(c["dt"]) / F(dt_parts), **wrong)
        hops += P.hops
        capped |= P.capped
    return P, hops, capped


@functools.lru_cache(maxsize=None)
def reference(name):
    P, hops, capped = run(name)
    for a in (P.x, P.y, P.cell, P.status, P.age, hops, capped):
        a.setflags(write=False)
    return P, hops, capped


@functools.lru_cache(maxsize=None)
def paths_of(name, advances=None):
    """Independent path: the float64 paths of a case's seeds (tests/particles_checks.py,
    track_paths) through the field the particles saw, the f32 cell velocities, for
    the case's whole time; computed once"""
    from tests import particles_checks as K
    c = case_of(name)
    pm = pmesh_of(c["mesh"])
    steps = c.get("steps", 1)
    u = field(mesh_of(c["mesh"]), c["field"]).astype(F).astype(np.float64)
    X = K.extent(pm.vx64, pm.vy64, seeds_of(name))
    return K.track_paths(pm.polygon, pm.N, u, seeds_of(name), float(F(c["dt"])) * steps, X, advances or steps)


def extent_of(name, P):
    from tests import particles_checks as K
    pm = pmesh_of(case_of(name)["mesh"])
    ok = np.isfinite(P.x) & np.isfinite(P.y)
    return K.extent(pm.vx64, pm.vy64, seeds_of(name), P.x[ok], P.y[ok])


def special_seeds(mname="obstacle"):
    """Seeding: (seeds (n, 2), slots expected OUTSIDE, {slot: cells sharing the
    edge or vertex the seed sits on}).  The shared points are exact in f32: a
    vertex's own rounded coordinates, and the midpoint of an axis-parallel
    internal face between vertices of one f32 x (so that E is exactly 0)."""
    mesh, pm = mesh_of(mname), pmesh_of(mname)
    a, t = mesh.arrays(), mesh.topology()
    seeds = [(1.0, 0.5), (1.1, 0.55), (-1.0, 0.5), (5.0, 5.0), (1.5, -0.25)]
    outside = list(range(len(seeds)))
    shared = {}
    n = pm.off[1:] - pm.off[:-1]
    cid = np.repeat(np.arange(pm.N), n)
    for v in (40, 300, 777):  # vertices
        cells = set(cid[pm.idx == v].tolist())
        if len(cells) >= 2:
            shared[len(seeds)] = cells
            seeds.append((float(pm.x[v]), float(pm.y[v])))
    nb = np.array(a["face_neighbor"], np.int64)
    v1, v2 = np.array(t["face_v1"], np.int64), np.array(t["face_v2"], np.int64)
    vertical = np.nonzero((nb != R.NONE) & (pm.x[v1] == pm.x[v2]))[0]
    for f in vertical[[3, len(vertical) // 2, -5]]:
        ym = F(0.5) * (pm.y[v1[f]] + pm.y[v2[f]])
        shared[len(seeds)] = {int(a["face_owner"][f]), int(nb[f])}
        seeds.append((float(pm.x[v1[f]]), float(ym)))
    seeds += [(0.31, 0.42), (2.2, 0.77)]  # plain interior seeds
    return np.array(seeds, np.float64), outside, shared
