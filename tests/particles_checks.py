"""Float64 checks of tracer particles, from the geometry and the velocity field
alone: they know the cells' polygons, the boundary lines and the field, and
nothing of the f32 arithmetic that moved the particles (no edge orientation by
vertex index, no bins, no slots).

Margins, derived (X = the largest |coordinate| among the vertices, the seeds
and the end points; u = 2^-24, the f32 unit roundoff):
  * eps, where a particle may lie relative to a face.  A vertex coordinate is
    rounded once (u X), so an edge line moves by at most 2 sqrt(2) u X near the
    edge.  The edge function carries three roundings per product and stands for
    a distance off by at most 12 sqrt(2) u X (tests/render_checks.py); the
    crossing parameter t uses two of them (at p and at e), so the crossing point
    is off the face's line by at most 24 sqrt(2) u X; the move p + v * (r * t)
    adds three roundings of values <= X per coordinate, 3 sqrt(2) u X.
    Sum: 29 sqrt(2) u X < 64 u X = eps.
  * eps_hop, what one move adds along a straight path.  s = r * t is rounded
    once, p + v * s twice per coordinate (values <= X), r - s once (a time
    <= dt, a length <= X after the velocity): at most 5 sqrt(2) u X < 8 u X per
    move, and the age takes the same roundings divided by |v|.  eps_hop = 8 u X;
    a path of h hops and the final free move is off by at most (h + 1) eps_hop.
    In a uniform field the crossing points do not matter (the velocity is the
    same on both sides), so eps does not enter the end position; it enters the
    age of an exit (the time to the boundary line) once, as eps / |v_n| with v_n
    the velocity normal to that line.
  * the path bound, where the field differs from cell to cell.  The f32
    particle changes its velocity where IT crosses the face: off the face's line
    by at most eps plus the error d it arrived with, so the change comes early or
    late by at most (eps + d) / |v_n|, v_n the arriving velocity normal to the
    face, and for that time the particle moves with the wrong one of the two
    velocities, which differ by |dv|.  With q = |dv| / |v_n| of that crossing,
    taken from the float64 path itself:  d' = d (1 + q) + eps q + eps_hop.  It
    starts at eps_hop (the seed's rounding) and takes one eps_hop more per
    advance (the free move that ends it).  Where q is not bounded the path is
    left out, by rules stated with track_path, under the 1 % cap.
No measured constant.
"""
import numpy as np

U24 = 2.0 ** -24
EMPTY, ALIVE, EXITED_OUTLET, EXITED_INLET, OUTSIDE = range(5)


def extent(*arrays):
    return max(float(np.nanmax(np.abs(np.asarray(a, np.float64)))) for a in arrays if np.size(a))


def eps_of(X):
    return 64.0 * U24 * X


def eps_hop_of(X):
    return 8.0 * U24 * X


def _seg_dist(a, b, p):
    """distances of the points p (n, 2) from the segments a[k] -> b[k] (m, 2): (n, m)"""
    e = b - a
    d = p[:, None, :] - a[None]
    L2 = (e * e).sum(1)
    t = np.clip((d * e[None]).sum(2) / np.where(L2 > 0, L2, 1.0), 0.0, 1.0)
    return np.hypot(d[..., 0] - t * e[None, :, 0], d[..., 1] - t * e[None, :, 1])


def inside_evenodd(poly, p):
    """even-odd test of the points p (n, 2) against the polygon (m, 2)"""
    a, b = poly, np.roll(poly, -1, 0)
    px, py = p[:, 0:1], p[:, 1:2]
    cond = (a[None, :, 1] > py) != (b[None, :, 1] > py)
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = a[None, :, 0] + (py - a[None, :, 1]) * (b[None, :, 0] - a[None, :, 0]) / (b[None, :, 1] - a[None, :, 1])
    return (np.sum(cond & (px < xi), 1) % 2) == 1


def edge_dist(poly, p):
    return _seg_dist(poly, np.roll(poly, -1, 0), p).min(1)


def boundary_edges(off, idx):
    """the polygon edges (unordered vertex index pairs) that only one cell has:
    the domain's boundary"""
    off, idx = np.asarray(off, np.int64), np.asarray(idx, np.int64)
    count = {}
    for c in range(len(off) - 1):
        p = idx[off[c]:off[c + 1]]
        for a, b in zip(p.tolist(), np.roll(p, -1).tolist()):
            count[(min(a, b), max(a, b))] = count.get((min(a, b), max(a, b)), 0) + 1
    return {e for e, n in count.items() if n == 1}


def check_containment(polygon, x, y, cell, status, X, capped=None, contacts=None, on_wall=None):
    """Containment: every ALIVE particle lies in its stated cell's real polygon
    (float64 even-odd test) or within eps of its boundary.  A particle closer
    than eps to an edge is undecided.  polygon(c) -> (n, 2) float64.  Two kinds
    of particle sit on an edge by construction, must not be outside either, and
    do not count for the undecided share: one that stopped at the hop cap in the
    last advance, on the face it would cross next (capped), and one that met a
    wall (contacts > 0) and is sliding along one NOW: on_wall(c) -> the wall
    edges of cell c as a bool per polygon edge (k -> k + 1), and only a particle
    within eps of one of them is exempt.  One that met a wall and left it again
    counts like any other."""
    eps = eps_of(X)
    capped = np.zeros(len(x), bool) if capped is None else np.asarray(capped, bool)
    slid = np.zeros(len(x), bool) if contacts is None or on_wall is None else np.asarray(contacts) > 0
    alive = np.nonzero(np.asarray(status) == ALIVE)[0]
    bad = und = exempt = 0
    for s in alive:
        p = np.array([[float(x[s]), float(y[s])]])
        poly = polygon(int(cell[s]))
        d = _seg_dist(poly, np.roll(poly, -1, 0), p)[0]
        if d.min() <= eps:
            if capped[s] or (slid[s] and np.any(d[np.asarray(on_wall(int(cell[s])), bool)] <= eps)):
                exempt += 1
            else:
                und += 1
        elif not inside_evenodd(poly, p)[0]:
            bad += 1
    return dict(eps=eps, alive=len(alive), bad=bad, undecided=und, exempt=exempt, share=und / max(1, len(alive) - exempt))


def assert_containment(polygon, x, y, cell, status, X, capped=None, contacts=None, on_wall=None, cap=0.01):
    r = check_containment(polygon, x, y, cell, status, X, capped, contacts, on_wall)
    assert r["bad"] == 0 and r["share"] <= cap, r
    return r


def assert_uniform(start, vel, dt, x, y, status, contacts, hops, capped, X):
    """Uniform field: a particle that met no wall and is still ALIVE ends at
    start + vel * dt within (hops + 1) eps_hop; no particle is capped."""
    assert not np.any(capped), "a condition on the case: no particle is capped"
    m = (np.asarray(status) == ALIVE) & (np.asarray(contacts) == 0)
    assert m.any()
    end = np.asarray(start, np.float64)[m] + np.asarray(vel, np.float64) * float(dt)
    err = np.hypot(np.asarray(x, np.float64)[m] - end[:, 0], np.asarray(y, np.float64)[m] - end[:, 1])
    tol = (np.asarray(hops, np.float64)[m] + 1.0) * eps_hop_of(X)
    assert np.all(err <= tol), (float(err.max()), float(tol.min()), int(np.argmax(err - tol)))
    return float((err / tol).max())


def assert_exit(start, speed, line_x, want, x, status, age, hops, counts, capacity, X):
    """Exits: a uniform flow (speed, 0) towards the boundary line x = line_x: every
    particle ends `want` on that line, its age the time to the line; the counts
    per status sum to the capacity."""
    assert sum(counts) == capacity
    assert np.all(np.asarray(status) == want), np.bincount(np.asarray(status, np.int64))
    x0 = np.asarray(start, np.float64)[:, 0]
    t = (line_x - x0) / speed
    tol = ((np.asarray(hops, np.float64) + 1.0) * eps_hop_of(X) + eps_of(X)) / abs(speed)
    assert np.all(np.abs(np.asarray(age, np.float64) - t) <= tol), float(np.abs(np.asarray(age, np.float64) - t).max())
    assert np.all(np.abs(np.asarray(x, np.float64) - line_x) <= eps_of(X))


def assert_wall(start, vel, dt, wall_y, x, y, status, contacts, hops, X):
    """Wall: a uniform field pointing into the flat wall y = wall_y (normal (0, -1)):
    the particle ends on the wall line within eps, it slid with the tangential
    part (vel.x, 0) for the time after the contact, and counted a contact."""
    s = np.asarray(start, np.float64)
    vx, vy = float(vel[0]), float(vel[1])
    assert vy < 0
    tc = (wall_y - s[:, 1]) / vy  # the time of contact
    assert np.all((tc > 0) & (tc < dt)), "a condition on the case: every seed reaches the wall"
    assert np.all(np.asarray(status) == ALIVE) and np.all(np.asarray(contacts) >= 1)
    assert np.all(np.abs(np.asarray(y, np.float64) - wall_y) <= eps_of(X))
    travel = np.asarray(x, np.float64) - (s[:, 0] + vx * tc)
    tol = (np.asarray(hops, np.float64) + 1.0) * eps_hop_of(X) + eps_of(X) * abs(vx / vy)  # the contact time through eps
    assert np.all(np.abs(travel - vx * (dt - tc)) <= tol), float(np.abs(travel - vx * (dt - tc)).max())


class Polygons:
    """every cell's float64 polygon, and all of them padded into one array for
    the brute-force containment (a padding edge has no length and never counts)"""

    def __init__(self, polygon, ncells):
        self.poly = [np.asarray(polygon(c), np.float64) for c in range(ncells)]
        m = max(len(p) for p in self.poly)
        pad = lambda q, p: np.concatenate([q, np.repeat(p[:1], m - len(p), 0)])
        self.a = np.stack([pad(p, p) for p in self.poly])
        self.b = np.stack([pad(np.roll(p, -1, 0), p) for p in self.poly])

    def containing(self, q):
        """the cells whose polygon holds q under the even-odd rule, all cells tried"""
        a, b = self.a, self.b
        cond = (a[..., 1] > q[1]) != (b[..., 1] > q[1])
        with np.errstate(divide="ignore", invalid="ignore"):
            xi = a[..., 0] + (q[1] - a[..., 1]) * (b[..., 0] - a[..., 0]) / (b[..., 1] - a[..., 1])
        return np.nonzero(np.sum(cond & (q[0] < xi), 1) % 2 == 1)[0]


def track_path(P, u, start, T, X, advances=1, hop_limit=256):
    """Independent path: the float64 path of one particle from `start` for the
    time T through the piecewise-constant field u (N, 2), P a Polygons.  In a
    cell the path is a segment; it is clipped against the cell's polygon (the
    first edge it crosses outwards), and after every move the cell is found
    again by brute-force containment of a point a little further along
    (eps / 1024, far above float64's rounding and far below eps).  No edge
    functions, no slots, no neighbour lists.
    Returns (end (2,), bound, why): the bound of the module docstring for the
    distance between this end and the f32 particle's, and why = None, or the
    reason the path is left out:
      "vertex"   it passes within eps + bound of a vertex of a cell it is in
                 (there the order of the cells is not decided);
      "grazing"  it crosses a face at a normal speed below 1 % of the faster of
                 the two velocities (q is not bounded);
      "edge"     it starts or ends within eps + bound of an edge (the last
                 crossing may or may not have happened);
      "left"     it leaves the mesh (the case is meant to have no such path);
      "stuck"    more than hop_limit crossings (velocities that point at each
                 other across a face)."""
    eps, eps_hop = eps_of(X), eps_hop_of(X)
    p, r, d_err = np.array(start, np.float64), float(T), eps_hop
    found = P.containing(p)
    if len(found) != 1 or edge_dist(P.poly[found[0]], p[None])[0] <= eps + d_err:
        return p, d_err, "edge"
    c = int(found[0])
    for _ in range(hop_limit):
        v, poly = np.asarray(u[c], np.float64), P.poly[c]
        a, e = poly, np.roll(poly, -1, 0) - poly
        d = v * r
        den = d[0] * e[:, 1] - d[1] * e[:, 0]  # d . (the edge's outward normal x its length): > 0 leaves
        ap = a - p
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (ap[:, 0] * e[:, 1] - ap[:, 1] * e[:, 0]) / den
            w = (ap[:, 0] * d[1] - ap[:, 1] * d[0]) / den
        out = (den > 0) & (w >= 0) & (w <= 1) & (s >= -1e-12) & (s <= 1)
        k = int(np.argmin(np.where(out, s, np.inf))) if out.any() else -1
        sk = max(float(s[k]), 0.0) if k >= 0 else 1.0
        q = p + d * sk
        if _seg_dist(p[None], q[None], poly).min() <= eps + d_err:
            return q, d_err, "vertex"
        if k < 0:
            d_err += advances * eps_hop
            if edge_dist(poly, q[None])[0] <= eps + d_err:
                return q, d_err, "edge"
            return q, d_err, None
        speed = float(np.hypot(*v))
        found = P.containing(q + v / speed * (eps / 1024.0))
        if len(found) != 1 or found[0] == c:
            return q, d_err, "left"
        n = int(found[0])
        vn = float(den[k] / r / np.hypot(*e[k]))
        dv = float(np.hypot(*(np.asarray(u[n], np.float64) - v)))
        if vn < 0.01 * max(speed, float(np.hypot(*u[n]))):
            return q, d_err, "grazing"
        d_err = d_err * (1.0 + dv / vn) + eps * dv / vn + eps_hop
        p, r, c = q, r - r * sk, n
    return p, d_err, "stuck"


def track_paths(polygon, ncells, u, starts, T, X, advances=1):
    """track_path for every start: (ends (n, 2), bounds (n,), reasons list)"""
    P = Polygons(polygon, ncells)
    res = [track_path(P, u, s, T, X, advances) for s in np.asarray(starts, np.float64)]
    return np.array([r[0] for r in res]), np.array([r[1] for r in res]), [r[2] for r in res]


def assert_path(paths, x, y, status, contacts, cap=0.01):
    """Independent path: every particle is ALIVE and met no wall (a condition on
    the case), at most 1 % of the float64 paths are left out, and every other
    particle ends within its path's bound of the path's end."""
    ends, bounds, why = paths
    assert np.all(np.asarray(status) == ALIVE) and not np.any(contacts), "a condition on the case"
    keep = np.array([w is None for w in why])
    assert (~keep).sum() <= cap * len(keep), [w for w in why if w]
    err = np.hypot(np.asarray(x, np.float64) - ends[:, 0], np.asarray(y, np.float64) - ends[:, 1])
    assert np.all(err[keep] <= bounds[keep]), (float((err / bounds)[keep].max()), int(np.argmax(np.where(keep, err / bounds, 0))))
    return float((err / bounds)[keep].max())


def assert_split(one, two, bound_one, bound_two, keep):
    """Split: one advance of dt and two of dt / 2 in a frozen field agree.  Both
    follow the same float64 path, each within its own bound of it (the halved
    run takes twice the advances), so they are within the sum of the two of each
    other; `keep` leaves out the paths that have no bound.  Not bitwise: the
    half step ends inside a cell."""
    (x1, y1), (x2, y2) = one, two
    err = np.hypot(np.asarray(x1, np.float64) - x2, np.asarray(y1, np.float64) - y2)
    tol = np.asarray(bound_one) + np.asarray(bound_two)
    assert np.any(keep) and np.all(err[keep] <= tol[keep]), (float((err / tol)[keep].max()),)


def assert_seeding(polygon, ncells, x, y, cell, status, X, expect_outside, on_shared):
    """Seeding: seeds listed in expect_outside (in the obstacle, off the domain)
    are OUTSIDE; a seed of on_shared {slot: cells that share the edge or vertex it
    sits on} goes to the largest of them; every other ALIVE seed lies in its cell."""
    for s in expect_outside:
        assert status[s] == OUTSIDE and cell[s] == 0xFFFFFFFF, (s, status[s], cell[s])
    for s, cells in on_shared.items():
        assert status[s] == ALIVE and int(cell[s]) == max(cells), (s, int(cell[s]), sorted(cells))
    rest = [s for s in range(len(x)) if s not in on_shared]
    idx = np.array(rest, np.int64)
    r = check_containment(polygon, np.asarray(x)[idx], np.asarray(y)[idx], np.asarray(cell)[idx], np.asarray(status)[idx], X)
    assert r["bad"] == 0, r


def assert_unmoved(before, after):
    """an OUTSIDE or EXITED particle never moves: position, age and status bit for bit"""
    for a, b in zip(before, after):
        assert np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def assert_stamp(frame, stamped, box, x, y, status, colour, X):
    """Stamp: every ALIVE particle whose position lies in a pixel by more than
    the centre margin of the picture (8 sqrt(2) u X < 16 u X) has that pixel in
    the colour; every pixel that changed holds the colour and has a particle
    within the margin of it; the alpha of row 0 is the TOP (y1)."""
    H, W = frame.shape[:2]
    x0, y0, x1, y1 = (float(b) for b in box)
    dx, dy = (x1 - x0) / W, (y1 - y0) / H
    eps = 16.0 * U24 * X
    col = np.array(colour, np.uint8)
    changed = np.any(frame != stamped, 2)
    assert np.all(stamped[changed] == col)
    m = np.asarray(status) == ALIVE
    px, py = np.asarray(x, np.float64)[m], np.asarray(y, np.float64)[m]
    fi, fj = (px - x0) / dx, (y1 - py) / dy
    i, j = np.floor(fi).astype(np.int64), np.floor(fj).astype(np.int64)
    deep = ((fi - i) * dx > eps) & ((i + 1 - fi) * dx > eps) & ((fj - j) * dy > eps) & ((j + 1 - fj) * dy > eps)
    inview = (i >= 0) & (i < W) & (j >= 0) & (j < H)
    assert (deep & inview).any()
    assert np.all(stamped[j[deep & inview], i[deep & inview]] == col)
    near = np.zeros((H, W), bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            ii, jj = i + di, j + dj
            ok = (ii >= 0) & (ii < W) & (jj >= 0) & (jj < H) & (deep & (di == 0) & (dj == 0) | ~deep)
            near[jj[ok], ii[ok]] = True
    assert not np.any(changed & ~near)
