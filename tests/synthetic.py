"""Hand-built meshes for edge cases (a Mesh-like object over numpy arrays):
single cell, a 1-D strip of cells, deliberately broken meshes, and any mesh
with its cells renumbered (renumbered() and the seeded permutation builders)."""
import ctypes as C

import numpy as np

from cfd2_amd import _ffi

NONE = 0xFFFFFFFF


class ArrayMesh:
    """Same surface as cfd2_amd.Mesh (view / num_cells / num_faces / arrays)."""

    def __init__(self, **arrays):
        self._a = {k: np.ascontiguousarray(v) for k, v in arrays.items()}

    def arrays(self):
        return self._a

    def num_cells(self):
        return len(self._a["cell_cx"])

    def num_faces(self):
        return len(self._a["face_cx"])

    def view(self):
        a = self._a
        u32 = lambda k: a[k].ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
        f64 = lambda k: a[k].ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
        return _ffi.MeshView(self.num_cells(), self.num_faces(), u32("face_owner"), u32("face_neighbor"),
                             u32("face_boundary"), f64("face_area"), f64("face_nx"), f64("face_ny"),
                             f64("face_cx"), f64("face_cy"), f64("cell_cx"), f64("cell_cy"),
                             f64("cell_vol"), u32("cell_face_offsets"), u32("cell_faces"))


def strip(n, h=0.1):
    """n unit cells in a row along x: inlet on the left, outlet on the right,
    walls top and bottom (cell faces listed owner-side first)."""
    owner, nb, bt, area, nx, ny, fx, fy = [], [], [], [], [], [], [], []
    cell_faces = [[] for _ in range(n)]

    def face(o, ngh, b, a, nxx, nyy, cx, cy):
        f = len(owner)
        owner.append(o), nb.append(ngh), bt.append(b), area.append(a)
        nx.append(nxx), ny.append(nyy), fx.append(cx), fy.append(cy)
        cell_faces[o].append(f)
        if ngh != NONE:
            cell_faces[ngh].append(f)

    for i in range(n):
        x0 = i * h
        if i == 0:
            face(i, NONE, 1, h, -1.0, 0.0, x0, 0.5 * h)  # inlet
        face(i, NONE, 3, h, 0.0, -1.0, x0 + 0.5 * h, 0.0)  # bottom wall
        face(i, NONE, 3, h, 0.0, 1.0, x0 + 0.5 * h, h)  # top wall
        if i + 1 < n:
            face(i, i + 1, 0, h, 1.0, 0.0, x0 + h, 0.5 * h)
        else:
            face(i, NONE, 2, h, 1.0, 0.0, x0 + h, 0.5 * h)  # outlet
    offs = np.zeros(n + 1, dtype=np.uint32)
    for i in range(n):
        offs[i + 1] = offs[i] + len(cell_faces[i])
    return ArrayMesh(
        face_owner=np.array(owner, np.uint32), face_neighbor=np.array(nb, np.uint32),
        face_boundary=np.array(bt, np.uint32), face_area=np.array(area), face_nx=np.array(nx),
        face_ny=np.array(ny), face_cx=np.array(fx), face_cy=np.array(fy),
        cell_cx=np.array([(i + 0.5) * h for i in range(n)]), cell_cy=np.full(n, 0.5 * h),
        cell_vol=np.full(n, h * h), cell_face_offsets=offs,
        cell_faces=np.array([f for cf in cell_faces for f in cf], np.uint32))


def wheel(k, r1=0.3, r2=1.0):
    """A hub cell (regular k-gon, k internal faces) inside a ring of k sectors:
    the hub's scalar row has k + 1 entries (the widest row a mesh can give
    the layouts: topology rejects width > 127).  Sector outer faces are inlets
    where the outward normal points left, outlets where it points right,
    walls elsewhere."""
    th = 2.0 * np.pi * np.arange(k + 1) / k
    ci, si = np.cos(th), np.sin(th)
    owner, nb, bt, area, nx, ny, fx, fy = [], [], [], [], [], [], [], []
    n = k + 1  # cell 0 = hub, cell 1 + s = sector s
    cell_faces = [[] for _ in range(n)]

    def face(o, ngh, b, a, nxx, nyy, cx, cy):
        f = len(owner)
        owner.append(o), nb.append(ngh), bt.append(b), area.append(a)
        nx.append(nxx), ny.append(nyy), fx.append(cx), fy.append(cy)
        cell_faces[o].append(f)
        if ngh != NONE:
            cell_faces[ngh].append(f)

    def poly(xs, ys):  # shoelace area and centroid
        x2, y2 = np.roll(xs, -1), np.roll(ys, -1)
        c = xs * y2 - x2 * ys
        a = 0.5 * c.sum()
        return a, ((xs + x2) * c).sum() / (6 * a), ((ys + y2) * c).sum() / (6 * a)

    cx, cy, vol = [0.0] * n, [0.0] * n, [0.0] * n
    vol[0], cx[0], cy[0] = poly(r1 * ci[:k], r1 * si[:k])
    for s in range(k):
        a, x, y = poly(np.array([r1 * ci[s], r2 * ci[s], r2 * ci[s + 1], r1 * ci[s + 1]]),
                       np.array([r1 * si[s], r2 * si[s], r2 * si[s + 1], r1 * si[s + 1]]))
        vol[1 + s], cx[1 + s], cy[1 + s] = a, x, y
    for s in range(k):  # hub edges: hub -> sector s
        mx, my = 0.5 * r1 * (ci[s] + ci[s + 1]), 0.5 * r1 * (si[s] + si[s + 1])
        ln = np.hypot(mx, my)
        face(0, 1 + s, 0, 2 * r1 * np.sin(np.pi / k), mx / ln, my / ln, mx, my)
    for s in range(k):  # radial edge at th[s]: sector s-1 -> sector s
        o = 1 + (s - 1) % k
        face(o, 1 + s, 0, r2 - r1, -si[s], ci[s], 0.5 * (r1 + r2) * ci[s], 0.5 * (r1 + r2) * si[s])
    for s in range(k):  # outer boundary
        mx, my = 0.5 * r2 * (ci[s] + ci[s + 1]), 0.5 * r2 * (si[s] + si[s + 1])
        ln = np.hypot(mx, my)
        b = 1 if mx / ln < -0.5 else (2 if mx / ln > 0.5 else 3)
        face(1 + s, NONE, b, 2 * r2 * np.sin(np.pi / k), mx / ln, my / ln, mx, my)
    offs = np.zeros(n + 1, dtype=np.uint32)
    for i in range(n):
        offs[i + 1] = offs[i] + len(cell_faces[i])
    return ArrayMesh(
        face_owner=np.array(owner, np.uint32), face_neighbor=np.array(nb, np.uint32),
        face_boundary=np.array(bt, np.uint32), face_area=np.array(area), face_nx=np.array(nx),
        face_ny=np.array(ny), face_cx=np.array(fx), face_cy=np.array(fy),
        cell_cx=np.array(cx), cell_cy=np.array(cy), cell_vol=np.array(vol), cell_face_offsets=offs,
        cell_faces=np.array([f for cf in cell_faces for f in cf], np.uint32))


def broken(kind):
    m = strip(4)
    a = {k: v.copy() for k, v in m.arrays().items()}
    if kind == "owner_range":
        a["face_owner"][0] = 99
    elif kind == "neighbor_range":
        i = int(np.nonzero(a["face_neighbor"] != NONE)[0][0])
        a["face_neighbor"][i] = 77
    elif kind == "cell_faces_range":
        a["cell_faces"][0] = 1000
    elif kind == "empty":
        for k in a:
            a[k] = a[k][:0] if k != "cell_face_offsets" else np.zeros(1, np.uint32)
    return ArrayMesh(**a)


CELL_ARRAYS = ("cell_cx", "cell_cy", "cell_vol")


def renumbered(mesh, perm):
    """The same mesh with its cells relabelled: perm[old] = new.  Faces keep
    their numbers, arrays, owner / neighbour roles (so the normals stand) and
    each cell keeps its own face order; only the cell ids in face_owner /
    face_neighbor, the order of the per-cell arrays and the order of the
    cell_faces runs change."""
    a = mesh.arrays()
    perm = np.asarray(perm, dtype=np.int64)
    n = len(a["cell_cx"])
    assert perm.shape == (n,) and np.array_equal(np.sort(perm), np.arange(n)), "perm is not a permutation"
    old_of = np.empty(n, dtype=np.int64)  # old_of[new] = old
    old_of[perm] = np.arange(n)
    out = {k: np.array(v, copy=True) for k, v in a.items()}
    own = a["face_owner"].astype(np.int64)
    nb = a["face_neighbor"].astype(np.int64)
    out["face_owner"] = perm[own].astype(np.uint32)
    inner = nb != NONE
    nb2 = np.full(len(nb), NONE, dtype=np.int64)
    nb2[inner] = perm[nb[inner]]
    out["face_neighbor"] = nb2.astype(np.uint32)
    for k in CELL_ARRAYS:
        out[k] = a[k][old_of]
    offs = a["cell_face_offsets"].astype(np.int64)
    cnt = (offs[1:] - offs[:-1])[old_of]
    new_offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cnt, out=new_offs[1:])
    # slot s of new cell i reads old slot offs[old_of[i]] + (s - new_offs[i])
    src = np.repeat(offs[:-1][old_of] - new_offs[:-1], cnt) + np.arange(int(new_offs[-1]))
    out["cell_face_offsets"] = new_offs.astype(np.uint32)
    out["cell_faces"] = a["cell_faces"][src]
    return ArrayMesh(**out)


def inverse_perm(perm):
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return inv


def perm_far_swap(n, k=64):
    """First k cells exchanged with the last k: nearly every row keeps its
    neighbours at the same small distances, a handful reach across the mesh."""
    assert n >= 2 * k
    perm = np.arange(n, dtype=np.int64)
    perm[:k] = np.arange(n - k, n)
    perm[n - k:] = np.arange(k)
    return perm


def perm_block_shuffle(n, block=1024, seed=2024):
    """Blocks of `block` consecutive cells (the last one shorter) laid out in
    seeded random order; the order inside a block stands."""
    nb = -(-n // block)
    order = np.random.default_rng(seed).permutation(nb)  # order[k] = old block placed k-th
    size = np.minimum(block, n - order * block)
    start = np.zeros(nb, dtype=np.int64)
    np.cumsum(size[:-1], out=start[1:])
    perm = np.empty(n, dtype=np.int64)
    for k, ob in enumerate(order):
        perm[ob * block:ob * block + size[k]] = start[k] + np.arange(size[k])
    return perm


def perm_random(n, seed=2024):
    """A seeded permutation of all cells."""
    return np.random.default_rng(seed).permutation(n).astype(np.int64)


def red_units(n):
    """(g, G, U) of the canonical reduction tree for n cells (kernels.hpp
    red_geom): segments of G = 2^g chunks of 256 cells, written by the chunk
    kernels as units of U = min(G, 4) chunks."""
    g = 0
    while g < 8 and (n >> (g + 1)) >= 16384:
        g += 1
    return g, 1 << g, min(1 << g, 4)


def max_ranks(n):
    """Most ranks a mesh of n cells can take: one segment of the canonical
    reduction tree each (kernels.hpp red_geom)."""
    g = 0
    while g < 8 and (n >> (g + 1)) >= 16384:
        g += 1
    nch = -(-n // 256)
    return -(-nch // (1 << g))
