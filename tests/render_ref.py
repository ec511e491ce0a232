"""numpy restatement of the picture (include/cfd2_amd.h, "The picture"): the
ownership map of a view and the RGBA8 image of a cell field, every operation in
f32 with one rounding each, written from that text and not from the kernels.
numpy evaluates x * y - z * w as three separately rounded ufuncs, which is the
header's "nothing fused".

The candidate (cell, pixel) pairs are enumerated flat, a chunk of triangles at
a time, so the cost is the sum of the pixel boxes and not cells x pixels.
"""
import numpy as np

F = np.float32
U = np.uint32
NONE = U(0xFFFFFFFF)
FIELDS = {"speed": 0, "ux": 1, "uy": 2, "p": 3, "vorticity": 4, "divergence": 5, "scalar": 6}
_PAIRS = 1 << 21  # candidate pairs per chunk


def mesh_polygons(mesh):
    """(vx, vy) f64, cell_vertex_offsets, cell_vertices of a cfd2_amd Mesh"""
    vx, vy, _ = mesh.vertices()
    t = mesh.topology()
    return (np.array(vx, np.float64), np.array(vy, np.float64), np.array(t["cell_vertex_offsets"], np.int64),
            np.array(t["cell_vertices"], np.int64))


def bounds(vx, vy, idx):
    """compute_bounds over the polygons' vertices, (x0, y0, x1, y1)"""
    x, y = vx[idx], vy[idx]
    return float(np.nanmin(x)), float(np.nanmin(y)), float(np.nanmax(x)), float(np.nanmax(y))


class View:
    """view: each bound rounded to f32 once; dx, dy; pixel centres"""

    def __init__(self, W, H, box):
        x0, y0, x1, y1 = (F(v) for v in box)
        assert x1 > x0 and y1 > y0 and 1 <= W <= 8192 and 1 <= H <= 8192
        self.W, self.H, self.x0, self.y1 = int(W), int(H), x0, y1
        self.dx = (x1 - x0) / F(W)
        self.dy = (y1 - y0) / F(H)
        assert self.dx > 0 and self.dy > 0

    def px(self, i):
        return self.x0 + (i.astype(F) + F(0.5)) * self.dx

    def py(self, j):
        return self.y1 - (j.astype(F) + F(0.5)) * self.dy


def _edge(x, y, frm, to, px, py):
    """edges: E of the edge between the INDICES a < b; traversed from b to a: -E"""
    flip = to < frm
    a, b = np.where(flip, to, frm), np.where(flip, frm, to)
    xa, ya = x[a], y[a]
    e = (x[b] - xa) * (py - ya) - (y[b] - ya) * (px - xa)
    return np.where(flip, -e, e)


def owner_map(vx, vy, off, idx, view, rule="largest", closed=True):
    """(H, W) uint32: the owner of each pixel centre, NONE where there is none.
    rule="smallest" and closed=False are deliberately WRONG variants (the
    float64 check has to catch them)."""
    x, y = np.asarray(vx, np.float64).astype(F), np.asarray(vy, np.float64).astype(F)  # rounded to f32 once
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    N, W, H = len(off) - 1, view.W, view.H
    n = off[1:] - off[:-1]
    cid = np.repeat(np.arange(N), n)
    mnx, mny = np.full(N, np.inf, F), np.full(N, np.inf, F)
    mxx, mxy = np.full(N, -np.inf, F), np.full(N, -np.inf, F)
    np.fmin.at(mnx, cid, x[idx])  # "a NaN coordinate is ignored by the comparisons"
    np.fmin.at(mny, cid, y[idx])
    np.fmax.at(mxx, cid, x[idx])
    np.fmax.at(mxy, cid, y[idx])
    with np.errstate(invalid="ignore", over="ignore"):
        fi0 = np.floor((mnx - view.x0) / view.dx - F(0.5))
        fi1 = np.ceil((mxx - view.x0) / view.dx - F(0.5))
        fj0 = np.floor((view.y1 - mxy) / view.dy - F(0.5))
        fj1 = np.ceil((view.y1 - mny) / view.dy - F(0.5))
        fi0 = np.where(fi0 < 0, F(0), fi0)
        fj0 = np.where(fj0 < 0, F(0), fj0)
        fi1 = np.where(fi1 > F(W - 1), F(W - 1), fi1)
        fj1 = np.where(fj1 > F(H - 1), F(H - 1), fj1)
        ok = (n >= 3) & (fi0 <= fi1) & (fj0 <= fj1)
    cells = np.nonzero(ok)[0]
    enc = np.zeros(W * H, np.int64) if rule == "largest" else np.full(W * H, N + 1, np.int64)
    if len(cells):
        # the fan triangles (v_0, v_i, v_i+1), 1 <= i <= n - 2, of the cells that have candidates
        nt = n[cells] - 2
        tc = np.repeat(cells, nt)
        loc = np.arange(len(tc)) - np.repeat(np.cumsum(nt) - nt, nt)
        v0, v1, v2 = idx[off[tc]], idx[off[tc] + 1 + loc], idx[off[tc] + 2 + loc]
        with np.errstate(invalid="ignore", over="ignore"):
            keep = ~(_edge(x, y, v0, v1, x[v2], y[v2]) == 0)  # no area: skipped
        tc, v0, v1, v2 = tc[keep], v0[keep], v1[keep], v2[keep]
        i0, j0 = fi0[tc].astype(np.int64), fj0[tc].astype(np.int64)
        bw, bh = fi1[tc].astype(np.int64) - i0 + 1, fj1[tc].astype(np.int64) - j0 + 1
        cnt = bw * bh
        start, end = 0, np.cumsum(cnt)
        while start < len(tc):
            stop = max(start + 1, int(np.searchsorted(end, (end[start - 1] if start else 0) + _PAIRS, "right")))
            s = slice(start, stop)
            c = cnt[s]
            t = np.repeat(np.arange(start, stop), c)
            q = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
            i, j = i0[t] + q % bw[t], j0[t] + q // bw[t]
            px, py = view.px(i), view.py(j)
            with np.errstate(invalid="ignore", over="ignore"):
                s1, s2, s3 = (_edge(x, y, a, b, px, py) for a, b in ((v0[t], v1[t]), (v1[t], v2[t]), (v2[t], v0[t])))
                if closed:
                    own = ((s1 >= 0) & (s2 >= 0) & (s3 >= 0)) | ((s1 <= 0) & (s2 <= 0) & (s3 <= 0))
                else:
                    own = ((s1 > 0) & (s2 > 0) & (s3 > 0)) | ((s1 < 0) & (s2 < 0) & (s3 < 0))
            pix, who = (j * W + i)[own], tc[t][own] + 1
            if rule == "largest":
                np.maximum.at(enc, pix, who)
            else:
                np.minimum.at(enc, pix, who)
            start = stop
    if rule != "largest":
        enc[enc == N + 1] = 0
    return (enc.astype(U) - U(1)).reshape(H, W)  # 0 -> NONE


def field_values(field, u=None, p=None, vorticity=None, divergence=None, scalar=None):
    """value: the f32 cell values of a field kind (name or 0..6) from the f32 arrays"""
    k = FIELDS[field] if isinstance(field, str) else int(field)
    if k <= 2:
        u = np.asarray(u, F)
        if k == 0:
            return np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1])  # f32, correctly rounded
        return u[:, k - 1].copy()
    src = {3: p, 4: vorticity, 5: divergence, 6: scalar}[k]
    return np.asarray(src, F).copy()


def value_key(v):
    """cfd_scalar_stats' order-preserving key of f32 values"""
    b = np.asarray(v, F).view(U)
    return np.where(b & U(0x80000000), ~b, b | U(0x80000000))


def key_value(k):
    k = np.asarray(k, U)
    return np.where(k & U(0x80000000), k & U(0x7FFFFFFF), ~k).astype(U).view(F)


def auto_range(val):
    """auto range: min and max over ALL cells through the keys, NaN ignored; none left: (0, 1)"""
    val = np.asarray(val, F)
    k = value_key(val[~np.isnan(val)])
    if len(k) == 0:
        return F(0), F(1)
    return F(key_value(k.min())), F(key_value(k.max()))


def colour(val, lo, hi):
    """colour: (n, 4) uint8 of f32 values over the range (lo, hi)"""
    val, lo, hi = np.asarray(val, F), F(lo), F(hi)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = hi - lo
        safe = F(1) if abs(r) < F(1e-10) else r
        q = (val - lo) / safe
        nan = np.isnan(q)
        t = np.where(q < 0, F(0), np.where(q > 1, F(1), q)).astype(F)
        t = np.where(nan, F(0), t)
        low = t < F(0.5)
        s = np.where(low, t * F(2), (t - F(0.5)) * F(2)).astype(F)
        one = F(1) - s
        zero = np.zeros_like(s)
        R, G, B = np.where(low, zero, s), np.where(low, s, one), np.where(low, one, zero)
        out = np.empty((len(val), 4), np.uint8)
        for k, c in enumerate((R, G, B)):
            out[:, k] = (c.astype(F) * F(255) + F(0.5)).astype(np.int32).astype(np.uint8)
    out[:, 3] = 255
    out[nan] = (0, 0, 0, 255)
    return out


def shade(owner, val, lo, hi):
    """(H, W, 4) uint8: the image of the cell values over the map"""
    img = np.zeros(owner.shape + (4,), np.uint8)
    owned = owner != NONE
    img[owned] = colour(np.asarray(val, F)[owner[owned].astype(np.int64)], lo, hi)
    return img


def render(owner, val, rng=None):
    """the image and the range used"""
    lo, hi = auto_range(val) if rng is None else (F(rng[0]), F(rng[1]))
    return shade(owner, val, lo, hi), (lo, hi)
