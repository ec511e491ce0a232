"""Float64 check of an ownership map, from the geometry alone: it knows the
polygons, the view box and the rule "the largest cell index among the cells
that contain the pixel centre", and nothing of the f32 arithmetic that built
the map (no edge orientation by vertex index, no pixel boxes, no f32 centres).

For every pixel, with its centre p in f64 and a margin eps:
  1. a stated owner c must contain p within eps: p is at most eps away from one
     of c's fan triangles;
  2. no cell with an index above c may contain p by more than eps (for a
     background pixel: no cell at all may): the disc of radius eps around p
     lies inside that cell's fan.
"By more than eps" is decided per fan, not per triangle, so that a centre on
the diagonal of a fan is still deep inside the cell: the disc lies inside the
union of a triangle T and its fan neighbours if p is more than eps inside every
edge line of T that is a polygon edge and, for each diagonal of T, more than eps
inside the two other edge lines of the neighbour across it (the part of the
disc beyond the diagonal then lies in that neighbour, the intersection of its
three half-planes).  Only neighbours of T's own winding count.  This is a lower
bound of the depth, so the check never accuses a correct map.

eps, derived (X = the largest |coordinate| among the vertices and the box):
  * vertices: each coordinate is rounded to f32 once, 2^-24 X each, so a vertex
    moves by at most sqrt(2) 2^-24 X and an edge line through two of them by
    at most 2 sqrt(2) 2^-24 X near the edge;
  * centres: the box bounds are rounded (2^-24 X each), dx carries two more
    roundings of a length <= 2 X, the product (i + 0.5) dx one of a length
    <= 2 X and the sum one of a value <= X: at most 8 x 2^-24 X per coordinate,
    8 sqrt(2) 2^-24 X for the point;
  * the edge function: each of its two products carries three roundings (two
    differences, one multiplication), the final subtraction keeps the sign;
    |product| <= L D with L the edge length and D the distance from p to the
    edge's first vertex, so the value is off by at most 2 L D x 3 x 2^-24 and
    the distance it stands for, value / L, by 6 D 2^-24 with D <= 2 sqrt(2) X:
    12 sqrt(2) 2^-24 X.
  Sum: 22 sqrt(2) 2^-24 X < 32 x 2^-24 X = eps.  No measured constant.

Undecided pixels: those with some cell within eps of p but not containing it by
more than eps -- the margin cannot say whether that cell may own them.  Their
share is about (edge length per unit area) x 2 eps: 2 x 10^-4 for cells of 0.1
in a 3 x 1 channel (eps = 6 x 10^-6), 0.4 % for the 65 536-cell mesh.  The
share is returned and capped at 5 % per case by the tests.
"""
import numpy as np

NONE = 0xFFFFFFFF
_PAIRS = 1 << 20


def margin(vx, vy, box):
    X = max(float(np.nanmax(np.abs(vx))), float(np.nanmax(np.abs(vy))), *(abs(float(b)) for b in box))
    return 32.0 * 2.0 ** -24 * X


def _line_dist(ax, ay, bx, by, px, py, sgn):
    """signed distance of p from the line a -> b, positive on the inside of a triangle of winding sgn"""
    ex, ey = bx - ax, by - ay
    return sgn * (ex * (py - ay) - ey * (px - ax)) / np.hypot(ex, ey)


def _seg_dist(ax, ay, bx, by, px, py):
    ex, ey = bx - ax, by - ay
    t = np.clip(((px - ax) * ex + (py - ay) * ey) / (ex * ex + ey * ey), 0.0, 1.0)
    return np.hypot(px - (ax + t * ex), py - (ay + t * ey))


def check_owner_map(vx, vy, off, idx, box, owner, eps=None):
    """Returns dict(eps, undecided, share, bad_owner, bad_higher, bad_background):
    the counts of pixels that break rule 1, rule 2 under an owner, rule 2 on the
    background.  A correct map has three zeros."""
    x, y = np.asarray(vx, np.float64), np.asarray(vy, np.float64)
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    owner = np.asarray(owner)
    H, W = owner.shape
    x0, y0, x1, y1 = (float(b) for b in box)
    if eps is None:
        eps = margin(x, y, box)
    dx, dy = (x1 - x0) / W, (y1 - y0) / H
    own = np.where(owner.ravel() == NONE, -1, owner.ravel().astype(np.int64))
    N = len(off) - 1
    n = off[1:] - off[:-1]
    cells = np.nonzero(n >= 3)[0]
    nt = n[cells] - 2
    tc = np.repeat(cells, nt)
    loc = np.arange(len(tc)) - np.repeat(np.cumsum(nt) - nt, nt) + 1  # i of (v_0, v_i, v_i+1)
    base = off[tc]

    def vert(k):  # vertex k of the triangle's polygon (clamped: used only where it exists)
        v = idx[base + np.clip(k, 0, n[tc] - 1)]
        return x[v], y[v]

    (ax, ay), (bx, by), (cx, cy) = vert(0 * loc), vert(loc), vert(loc + 1)
    (qx, qy), (rx, ry) = vert(loc - 1), vert(loc + 2)  # the fan neighbours' far vertices
    area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    area_p = (qx - ax) * (by - ay) - (qy - ay) * (bx - ax)  # (v_0, v_i-1, v_i)
    area_n = (cx - ax) * (ry - ay) - (cy - ay) * (rx - ax)  # (v_0, v_i+1, v_i+2)
    sgn = np.sign(area)
    has_p = (loc > 1) & (np.sign(area_p) == sgn)
    has_n = (loc < n[tc] - 2) & (np.sign(area_n) == sgn)
    lens = np.minimum(np.minimum(np.hypot(bx - ax, by - ay), np.hypot(cx - bx, cy - by)), np.hypot(ax - cx, ay - cy))
    good = (area != 0) & (lens > 0) & np.isfinite(area)
    # candidate pixels of a triangle: its f64 bounds widened by eps and a pixel
    tx0, tx1 = np.minimum(np.minimum(ax, bx), cx) - eps, np.maximum(np.maximum(ax, bx), cx) + eps
    ty0, ty1 = np.minimum(np.minimum(ay, by), cy) - eps, np.maximum(np.maximum(ay, by), cy) + eps
    with np.errstate(invalid="ignore"):
        i0 = np.clip(np.floor((tx0 - x0) / dx - 0.5) - 1, 0, W - 1)
        i1 = np.clip(np.ceil((tx1 - x0) / dx - 0.5) + 1, 0, W - 1)
        j0 = np.clip(np.floor((y1 - ty1) / dy - 0.5) - 1, 0, H - 1)
        j1 = np.clip(np.ceil((y1 - ty0) / dy - 0.5) + 1, 0, H - 1)
        good &= (tx1 >= x0 - dx) & (tx0 <= x1 + dx) & (ty1 >= y0 - dy) & (ty0 <= y1 + dy)
    T = np.nonzero(good)[0]
    i0, i1, j0, j1 = (a[T].astype(np.int64) for a in (i0, i1, j0, j1))
    bw = i1 - i0 + 1
    cnt = bw * (j1 - j0 + 1)
    deep = np.full(W * H, -1, np.int64)       # the largest cell that contains the centre by more than eps
    near_owner = np.zeros(W * H, bool)        # the stated owner is within eps
    undecided = np.zeros(W * H, bool)
    end = np.cumsum(cnt)
    start = 0
    while start < len(T):
        stop = max(start + 1, int(np.searchsorted(end, (end[start - 1] if start else 0) + _PAIRS, "right")))
        c = cnt[start:stop]
        k = np.repeat(np.arange(start, stop), c)
        q = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
        i, j = i0[k] + q % bw[k], j0[k] + q // bw[k]
        px, py = x0 + (i + 0.5) * dx, y1 - (j + 0.5) * dy
        t = T[k]
        g = lambda a: a[t]  # noqa: E731
        s = g(sgn)
        with np.errstate(invalid="ignore", divide="ignore"):
            d1 = _line_dist(g(ax), g(ay), g(bx), g(by), px, py, s)
            d2 = _line_dist(g(bx), g(by), g(cx), g(cy), px, py, s)
            d3 = _line_dist(g(cx), g(cy), g(ax), g(ay), px, py, s)
            plain = np.minimum(np.minimum(d1, d2), d3)
            # across the diagonal v_0 - v_i: the edges v_0 -> v_i-1 and v_i-1 -> v_i of the previous triangle
            dp = np.minimum(_line_dist(g(ax), g(ay), g(qx), g(qy), px, py, s),
                            _line_dist(g(qx), g(qy), g(bx), g(by), px, py, s))
            # across the diagonal v_i+1 - v_0: the edges v_i+1 -> v_i+2 and v_i+2 -> v_0 of the next triangle
            dn = np.minimum(_line_dist(g(cx), g(cy), g(rx), g(ry), px, py, s),
                            _line_dist(g(rx), g(ry), g(ax), g(ay), px, py, s))
            fan = np.minimum(np.minimum(np.where(g(has_p), dp, d1), d2), np.where(g(has_n), dn, d3))
            depth = np.fmax(plain, fan)  # a lower bound of the depth inside the cell's fan
            dist = np.where(plain >= 0, 0.0, np.minimum(np.minimum(
                _seg_dist(g(ax), g(ay), g(bx), g(by), px, py), _seg_dist(g(bx), g(by), g(cx), g(cy), px, py)),
                _seg_dist(g(cx), g(cy), g(ax), g(ay), px, py)))
        pix, cell = j * W + i, tc[t]
        is_deep, is_near = depth > eps, dist <= eps
        np.maximum.at(deep, pix[is_deep], cell[is_deep])
        near_owner[pix[is_near & (cell == own[pix])]] = True
        undecided[pix[is_near & ~is_deep]] = True
        start = stop
    owned = own >= 0
    return dict(eps=eps, undecided=int(undecided.sum()), share=float(undecided.mean()),
                bad_owner=int((owned & ~near_owner).sum()),
                bad_higher=int((owned & (deep > own)).sum()),
                bad_background=int((~owned & (deep >= 0)).sum()))


def assert_owner_map(vx, vy, off, idx, box, owner, cap=0.05):
    r = check_owner_map(vx, vy, off, idx, box, owner)
    assert r["share"] <= cap, r
    assert (r["bad_owner"], r["bad_higher"], r["bad_background"]) == (0, 0, 0), r
    return r
