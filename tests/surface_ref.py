"""Wall surface distributions restated in numpy -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of the surface
channels"), not from the kernels.  A surface is the ordered list (ascending
cell, then ascending slot in the cell's face list) of the wall faces whose
float64 centre lies in a closed box.  Per face j = (cell i, slot k), every
operation one float64 rounding on the float32 inputs widened, left to right:

    0        p[i]
    1, 2     p[i] * nx * area;  p[i] * ny * area
    3, 4     viscosity * rux * area / dist_e;  likewise ruy
             rux = u[i].x, or u[i].x - ubx on a slot the boundary-velocity
             selection moves (ubx, uby: the float32 wall velocity of the step)
    5 + 2f   kind 1: c_k * (value - phi_f[i]), c_k = (density * D) * area / dist_e
             in float32;  kind 2: value * area;  +0 outside the field's selection
    6 + 2f   phi_f[i]

The float32 geometry is the solver's: normal out of the owner cell (a boundary
face's own normal), dist_e = |face centre - cell centre| from the float32
centres, in float32.  This module takes the fields and settings as arguments: it
never asks the library for an answer.

The pieces a deliberately wrong variant replaces (tests/test_surface.py) are
methods of SurfaceRef: normal_sign, relative, diffusion.
"""
from __future__ import annotations

import numpy as np

F = np.float32
D64 = np.float64
NONE = 0xFFFFFFFF


def in_box(x, y, box):
    x0, y0, x1, y1 = box
    if x1 < x0:
        return np.zeros(len(x), bool)
    return (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)


def wall_faces(arrays):
    """every wall face of the mesh in (cell, slot) order: face, cell, slot"""
    a = arrays
    wall = (np.asarray(a["face_neighbor"]) == NONE) & ((np.asarray(a["face_boundary"]).astype(np.int64) & 3) == 3)
    offs = np.asarray(a["cell_face_offsets"]).astype(np.int64)
    cf = np.asarray(a["cell_faces"]).astype(np.int64)
    pos = np.nonzero(wall[cf])[0]  # positions in cell_faces: ascending cell, then slot
    cell = np.searchsorted(offs, pos, side="right") - 1
    return cf[pos], cell, pos - offs[cell]


class SurfaceRef:
    """The surface of ``box`` on the mesh ``arrays`` (a dict of the mesh's arrays)."""

    def __init__(self, arrays, box):
        a = arrays
        face, cell, slot = wall_faces(a)
        keep = in_box(np.asarray(a["face_cx"], D64)[face], np.asarray(a["face_cy"], D64)[face], box)
        self.face, self.cell, self.slot = face[keep], cell[keep], slot[keep]
        f, i = self.face, self.cell
        self.n = len(f)
        self.cx, self.cy = np.asarray(a["face_cx"], D64)[f], np.asarray(a["face_cy"], D64)[f]
        self.area = np.asarray(a["face_area"])[f].astype(F)
        self.nx, self.ny = np.asarray(a["face_nx"])[f].astype(F), np.asarray(a["face_ny"])[f].astype(F)
        dvx = np.asarray(a["face_cx"])[f].astype(F) - np.asarray(a["cell_cx"])[i].astype(F)
        dvy = np.asarray(a["face_cy"])[f].astype(F) - np.asarray(a["cell_cy"])[i].astype(F)
        self.dist_e = np.sqrt(dvx * dvx + dvy * dvy)
        assert self.dist_e.dtype == F
        self._arrays = a

    def geometry(self):
        """what cfd_surface_geometry_get returns"""
        w = lambda v: v.astype(D64)  # noqa: E731
        return dict(cell=self.cell.astype(np.uint32), slot=self.slot.astype(np.uint32), cx=self.cx, cy=self.cy,
                    nx=w(self.nx), ny=w(self.ny), area=w(self.area), dist_e=w(self.dist_e))

    # ---- the three pieces a wrong variant replaces ------------------------------
    def normal_sign(self):
        return 1.0  # the force of the fluid ON the wall: the normal out of the cell

    def relative(self, u, ub):
        return u - ub  # the velocity of the fluid relative to the wall

    def diffusion(self, ad, dist):
        """x -> x * area / dist, left to right"""
        return lambda x: x * ad / dist

    # ---------------------------------------------------------------------------
    def wall_velocity(self, bv, c, ramp):
        """(ubx, uby, moved) per surface face from a tests/bcvel_ref.BoundaryVelocities"""
        ubx, uby, sw = bv.face_values(None, c, ramp)
        return ubx[self.face], uby[self.face], sw[self.face]

    def sample(self, u, p, viscosity, density=1.0, fields=(), wall_velocity=None):
        """channels (5 + 2 len(fields), n) float64.  u (N, 2), p (N) float32; fields: dicts
        of phi (float32 [N]), diffusivity and wall = None or (kind, value, box);
        wall_velocity: None or float32 (ubx [n], uby [n], moved [n])"""
        u, p = np.asarray(u), np.asarray(p)
        assert u.dtype == F and p.dtype == F
        i = self.cell
        ad, dist = self.area.astype(D64), self.dist_e.astype(D64)
        nx, ny = self.nx.astype(D64) * self.normal_sign(), self.ny.astype(D64) * self.normal_sign()
        pc = p[i].astype(D64)
        ch = [pc, pc * nx * ad, pc * ny * ad]
        rux, ruy = u[i, 0].astype(D64), u[i, 1].astype(D64)
        if wall_velocity is not None:
            ubx, uby, moved = wall_velocity
            assert ubx.dtype == F and uby.dtype == F
            rux = np.where(moved, self.relative(rux, ubx.astype(D64)), rux)
            ruy = np.where(moved, self.relative(ruy, uby.astype(D64)), ruy)
        nu = D64(F(viscosity))
        diff = self.diffusion(ad, dist)
        ch += [diff(nu * rux), diff(nu * ruy)]
        for fd in fields:
            phi = np.asarray(fd["phi"])
            assert phi.dtype == F
            ph = phi[i].astype(D64)
            flux = np.zeros(self.n)
            if fd.get("wall") is not None and fd["wall"][0] != 0:
                kind, value, box = fd["wall"]
                sel = in_box(self.cx, self.cy, box)
                value = F(value)
                if kind == 1:
                    rd = F(density) * F(fd["diffusivity"])
                    ck = rd * self.area / self.dist_e
                    assert ck.dtype == F
                    t = ck.astype(D64) * (D64(value) - ph)
                else:
                    t = D64(value) * ad
                flux = np.where(sel, t, 0.0)
            ch += [flux, ph]
        return np.stack(ch) if self.n else np.zeros((5 + 2 * len(fields), 0))

    def fold(self, terms, N):
        """per cell the terms added in slot order from +0: [N] (the input of refpy.canon_sum)"""
        t = np.zeros(N)
        for j in range(self.n):  # the surface's order is (cell, slot)
            t[self.cell[j]] = t[self.cell[j]] + terms[j]
        return t


class SurfaceStats:
    """The per-face, per-channel weighted West / Welford update ("Arithmetic of
    the time statistics" with the covariance of a channel with itself), float64."""

    def __init__(self, shape):
        self.mean, self.m2 = np.zeros(shape), np.zeros(shape)
        self.W, self.samples = D64(0.0), 0

    def accumulate(self, x, weight):
        w = D64(weight)
        Wn = self.W + w
        r = w / Wn
        d = x - self.mean
        self.mean = self.mean + r * d
        e = x - self.mean
        self.m2 = self.m2 + (w * d) * e
        self.W, self.samples = Wn, self.samples + 1

    def variance(self):
        return self.m2 / self.W if self.W > 0 else self.m2.copy()
