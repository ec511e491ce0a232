"""numpy restatement of the tracers (include/cfd2_amd.h, "The tracers"): the
per-slot geometry, the bin grid, locate, advance, the statistics and the stamp,
every operation in f32 with one rounding each, written from that text and not
from the kernels.  numpy evaluates x * y - z * w as three separately rounded
ufuncs, which is the header's "nothing fused".

The particles are advanced together, one hop per pass, the slots of a cell one
after the other: per particle that is the header's loop.  The keyword arguments
named WRONG build deliberately wrong conventions into a copy of the rules; the
float64 checks (tests/particles_checks.py) have to catch each.
"""
import numpy as np

F = np.float32
U = np.uint32
EMPTY, ALIVE, EXITED_OUTLET, EXITED_INLET, OUTSIDE = range(5)
STATUS = ("empty", "alive", "exited_outlet", "exited_inlet", "outside")
NOCELL = U(0xFFFFFFFF)
NONE = 0xFFFFFFFF


class PMesh:
    """geometry + bins: what cfd_particles_set_mesh derives from a cfd2_amd Mesh"""

    def __init__(self, mesh):
        a, t = mesh.arrays(), mesh.topology()
        vx, vy, _ = mesh.vertices()
        self.vx64, self.vy64 = np.array(vx, np.float64), np.array(vy, np.float64)
        self.x, self.y = self.vx64.astype(F), self.vy64.astype(F)  # rounded to f32 once
        self.off = np.array(t["cell_vertex_offsets"], np.int64)
        self.idx = np.array(t["cell_vertices"], np.int64)
        N = self.N = len(self.off) - 1
        foff, faces = np.array(a["cell_face_offsets"], np.int64), np.array(a["cell_faces"], np.int64)
        self.nface = foff[1:] - foff[:-1]
        wf = self.wf = int(self.nface.max())
        owner, nb = np.array(a["face_owner"], np.int64), np.array(a["face_neighbor"], np.int64)
        fv1, fv2 = np.array(t["face_v1"], np.int64), np.array(t["face_v2"], np.int64)
        self.other = np.full((N, wf), -1, np.int64)
        self.btype = np.zeros((N, wf), np.int64)   # 0 internal, 1 inlet, 2 outlet, 3 wall
        self.sa, self.sb = np.zeros((N, wf), np.int64), np.zeros((N, wf), np.int64)
        self.neg = np.zeros((N, wf), bool)
        self.nx, self.ny = np.zeros((N, wf), F), np.zeros((N, wf), F)
        for c in range(N):
            p = self.idx[self.off[c]:self.off[c + 1]]
            nxt = np.roll(p, -1)
            assert np.sum(self.vx64[p] * self.vy64[nxt] - self.vx64[nxt] * self.vy64[p]) > 0, "CCW polygons"
            for k, f in enumerate(faces[foff[c]:foff[c + 1]]):
                internal = nb[f] != NONE
                own = owner[f] == c
                self.other[c, k] = (nb[f] if own else owner[f]) if internal else -1
                self.btype[c, k] = 0 if internal else int(a["face_boundary"][f]) & 3
                sgn = F(1) if own else F(-1)
                self.nx[c, k], self.ny[c, k] = sgn * F(a["face_nx"][f]), sgn * F(a["face_ny"][f])  # out of this cell
                v1, v2 = fv1[f], fv2[f]
                hit = np.nonzero(((p == v1) & (nxt == v2)) | ((p == v2) & (nxt == v1)))[0]
                assert len(hit), "a face's vertices are consecutive in its cells' polygons"
                self.sa[c, k], self.sb[c, k] = min(v1, v2), max(v1, v2)
                self.neg[c, k] = nxt[hit[0]] < p[hit[0]]  # the polygon runs b -> a: g = -E
        # bins
        X, Y = self.x[self.idx], self.y[self.idx]
        self.bx0, self.by0 = X.min(), Y.min()
        self.nb = min(1024, int(np.ceil(np.sqrt(float(N)))))
        self.sx, self.sy = (X.max() - self.bx0) / F(self.nb), (Y.max() - self.by0) / F(self.nb)
        assert self.sx > 0 and self.sy > 0
        n = self.off[1:] - self.off[:-1]
        cid = np.repeat(np.arange(N), n)
        lo = [np.full(N, np.inf, F) for _ in range(2)]
        hi = [np.full(N, -np.inf, F) for _ in range(2)]
        for k, Q in enumerate((X, Y)):
            np.minimum.at(lo[k], cid, Q)
            np.maximum.at(hi[k], cid, Q)
        i0, i1 = self.bin_x(lo[0]), self.bin_x(hi[0])
        j0, j1 = self.bin_y(lo[1]), self.bin_y(hi[1])
        self.bins = [[] for _ in range(self.nb * self.nb)]
        for c in range(N):  # ascending cells: ascending lists
            for j in range(j0[c], j1[c] + 1):
                for i in range(i0[c], i1[c] + 1):
                    self.bins[j * self.nb + i].append(c)

    def _bin(self, q, q0, s):
        with np.errstate(invalid="ignore", over="ignore"):
            f = np.floor((np.asarray(q, F) - q0) / s)
            f = np.where(f >= 0, f, F(0))  # also a NaN
            return np.where(f > F(self.nb - 1), F(self.nb - 1), f).astype(np.int64)

    def bin_x(self, x):
        return self._bin(x, self.bx0, self.sx)

    def bin_y(self, y):
        return self._bin(y, self.by0, self.sy)

    def polygon(self, c):
        """the f64 polygon of cell c, (n, 2)"""
        p = self.idx[self.off[c]:self.off[c + 1]]
        return np.stack([self.vx64[p], self.vy64[p]], 1)


def _E(pm, a, b, qx, qy):
    """E of the edge between the INDICES a < b at q"""
    xa, ya = pm.x[a], pm.y[a]
    return (pm.x[b] - xa) * (qy - ya) - (pm.y[b] - ya) * (qx - xa)


def _poly_edge(pm, frm, to, qx, qy):
    flip = to < frm
    e = _E(pm, np.where(flip, to, frm), np.where(flip, frm, to), qx, qy)
    return np.where(flip, -e, e)


def _owns(pm, c, qx, qy):
    """the closed fan test of cell c at the f32 point q"""
    p = pm.idx[pm.off[c]:pm.off[c + 1]]
    if len(p) < 3:
        return False
    v0, v1, v2 = np.full(len(p) - 2, p[0]), p[1:-1], p[2:]
    with np.errstate(invalid="ignore", over="ignore"):
        area = _poly_edge(pm, v0, v1, pm.x[v2], pm.y[v2]) != 0  # no area: skipped
        s1, s2, s3 = (_poly_edge(pm, f, t, qx, qy) for f, t in ((v0, v1), (v1, v2), (v2, v0)))
        own = ((s1 >= 0) & (s2 >= 0) & (s3 >= 0)) | ((s1 <= 0) & (s2 <= 0) & (s3 <= 0))
    return bool((own & area).any())


def locate(pm, x, y, owner="largest"):
    """the cell of each f32 point, NOCELL where there is none.  WRONG: owner="smallest"."""
    x, y = np.asarray(x, F), np.asarray(y, F)
    out = np.full(len(x), NOCELL, U)
    b = pm.bin_y(y) * pm.nb + pm.bin_x(x)
    for s in range(len(x)):
        found = [c for c in pm.bins[b[s]] if _owns(pm, c, x[s], y[s])]
        if found:
            out[s] = max(found) if owner == "largest" else min(found)
    return out


class Set:
    """the particle set: SoA, all slots EMPTY"""

    def __init__(self, capacity, hop_cap=64):
        n = self.n = int(capacity)
        self.hop_cap = int(hop_cap)
        self.x, self.y, self.age = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
        self.cell = np.full(n, NOCELL, U)
        self.status = np.zeros(n, U)
        self.contacts, self.hops, self.capped = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, bool)

    def seed(self, pm, xy, first=0, owner="largest"):
        xy = np.asarray(xy, np.float64)
        s = slice(first, first + len(xy))
        assert first + len(xy) <= self.n
        self.x[s], self.y[s] = xy[:, 0].astype(F), xy[:, 1].astype(F)  # rounded to f32 once
        self.cell[s] = locate(pm, self.x[s], self.y[s], owner)
        self.status[s] = np.where(self.cell[s] == NOCELL, OUTSIDE, ALIVE)
        self.age[s], self.contacts[s], self.hops[s], self.capped[s] = 0, 0, 0, False

    def stats(self):
        d = {name: int((self.status == k).sum()) for k, name in enumerate(STATUS)}
        d.update(wall_contacts=int(self.contacts.sum()), hops_total=int(self.hops.sum()),
                 hops_max=int(self.hops.max(initial=0)), capped=int(self.capped.sum()), capacity=self.n)
        return d


def advance(pm, u, P, dt, exits="segment", age_partial=True, wall="slide", fallback=True):
    """advance: every ALIVE particle of the Set P by dt through the f32 velocities u (N, 2).
    WRONG: exits="halfplane", age_partial=False, wall="stop", fallback=False (segments alone)."""
    u = np.asarray(u, F)
    dt = F(dt)
    P.hops[:], P.capped[:] = 0, False
    act = np.nonzero(P.status == ALIVE)[0]
    px, py, age = P.x[act].copy(), P.y[act].copy(), P.age[act].copy()
    c = P.cell[act].astype(np.int64)
    r = np.full(len(act), dt, F)
    vx, vy = u[c, 0].copy(), u[c, 1].copy()
    skip = np.full(len(act), -1, np.int64)
    hops = np.zeros(len(act), np.int64)
    live = np.ones(len(act), bool)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        while live.any():
            ex, ey = px + vx * r, py + vy * r
            bt, bk = np.full(len(act), 2, F), np.full(len(act), -1, np.int64)
            ht, hk = bt.copy(), bk.copy()  # the exit by half-planes alone: the fallback
            for k in range(pm.wf):
                a, b, neg = pm.sa[c, k], pm.sb[c, k], pm.neg[c, k]
                xa, ya, xb, yb = pm.x[a], pm.y[a], pm.x[b], pm.y[b]
                Ee, Ep = _E(pm, a, b, ex, ey), _E(pm, a, b, px, py)
                ge, gp = np.where(neg, -Ee, Ee), np.where(neg, -Ep, Ep)
                ha = vx * (ya - py) - vy * (xa - px)
                hb = vx * (yb - py) - vy * (xb - px)
                across = ((ha >= 0) & (hb <= 0)) | ((ha <= 0) & (hb >= 0))
                if exits == "halfplane":
                    across = np.ones_like(across)
                t = np.where(gp <= 0, F(0), gp / (gp - ge)).astype(F)
                beyond = live & (k < pm.nface[c]) & (k != skip) & (ge < 0)
                take = beyond & across & (t < bt)
                bt, bk = np.where(take, t, bt), np.where(take, k, bk)
                half = beyond & (t < ht)
                ht, hk = np.where(half, t, ht), np.where(half, k, hk)
            for q in np.nonzero((bk < 0) & (hk >= 0) & fallback)[0]:  # no segment is crossed, yet e is beyond a face's line
                if not _owns(pm, c[q], ex[q], ey[q]):
                    bt[q], bk[q] = ht[q], hk[q]
            free = live & (bk < 0)
            px, py = np.where(free, ex, px), np.where(free, ey, py)
            age = np.where(free, age + r, age)
            cap = live & ~free & (hops == P.hop_cap)
            P.capped[act[cap]] = True
            live = live & ~free & ~cap
            step = r * bt
            px, py = np.where(live, px + vx * step, px), np.where(live, py + vy * step, py)
            kk = np.where(live, bk, 0)
            bty = pm.btype[c, kk]
            gone = live & ((bty == 1) | (bty == 2))
            if age_partial:
                age = np.where(live, age + step, age)
            else:
                age = np.where(live & ~gone, age + step, age)
            r = np.where(live, r - step, r)
            hops = hops + live
            inner, hit = live & (bty == 0), live & (bty == 3)
            P.status[act[gone & (bty == 2)]] = EXITED_OUTLET
            P.status[act[gone & (bty == 1)]] = EXITED_INLET
            nx, ny = pm.nx[c, kk], pm.ny[c, kk]
            dn = vx * nx + vy * ny
            sx, sy = (vx - dn * nx, vy - dn * ny) if wall == "slide" else (np.zeros_like(vx), np.zeros_like(vy))
            P.contacts[act[hit]] += 1
            c = np.where(inner, pm.other[c, kk], c)
            vx = np.where(inner, u[c, 0], np.where(hit, sx, vx)).astype(F)
            vy = np.where(inner, u[c, 1], np.where(hit, sy, vy)).astype(F)
            skip = np.where(inner, -1, np.where(hit, kk, skip))
            live = live & ~gone
    P.x[act], P.y[act], P.age[act], P.cell[act], P.hops[act] = px, py, age, c.astype(U), hops


def stamp(P, frame, view, colour=(255, 255, 255, 255), flip_rows=False):
    """stamp: a copy of the (H, W, 4) frame with every ALIVE particle in the view (a
    render_ref.View) as one pixel of colour.  WRONG: flip_rows."""
    out = np.array(frame, np.uint8)
    m = P.status == ALIVE
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor((P.x[m] - view.x0) / view.dx)
        fj = np.floor((view.y1 - P.y[m]) / view.dy)
        ok = (fi >= 0) & (fi < F(view.W)) & (fj >= 0) & (fj < F(view.H))
    i, j = fi[ok].astype(np.int64), fj[ok].astype(np.int64)
    if flip_rows:
        j = view.H - 1 - j
    out[j, i] = np.array(colour, np.uint8)
    return out
