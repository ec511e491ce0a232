"""What the surface channels must equal, from the definition alone
(include/cfd2_amd.h "Arithmetic of the surface channels"): the checks know the
surface's geometry (cfd_surface_geometry_get: the float32 values widened) and
the fields, nothing of how a sample was computed.

Every expression is a product / quotient of float64 images of float32 values.
It is evaluated here in exact rational arithmetic (fractions.Fraction of the
same bit patterns) and rounded once.  The sample under test evaluates it in
float64 left to right: at most four roundings (three operations, and the
difference value - phi or u - ub before them), each within u = 2^-53 relative
of a partial result that is itself within the magnitude below.  So a correct
sample is within 4u (1 + O(u)) = 2 EPS of the exact value, EPS = 2^-52; the
issue's constant is 8:

    |got - exact| <= 8 EPS * (the product of the magnitudes of the expression's
                              factors, a difference a - b counting |a| + |b|)

Only float64 rounding separates two evaluations, because every input is the
same float32 bit pattern; anything else -- a flipped normal, the absolute wall
velocity, area * dist for area / dist -- is an O(1) relative error.
Channel 0 and channel 6 + 2f are widenings: exact."""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
BOUND = 8 * EPS
F = np.float32


def _fr(a):
    return [Fraction(float(v)) for v in np.asarray(a, np.float64)]


def _close(got, exact, mag, what):
    """got [n] float64 against exact / mag (lists of Fraction)"""
    worst = 0.0
    for j, (g, e, m) in enumerate(zip(np.asarray(got, np.float64), exact, mag)):
        assert np.isfinite(g), f"f64 {what}: face {j} is not finite"
        err = abs(Fraction(float(g)) - e)
        bound = Fraction(BOUND) * m
        assert err <= bound, f"f64 {what}: face {j} off by {float(err / bound) if bound else float('inf'):.3g} x the bound"
        if bound:
            worst = max(worst, float(err / bound))
    return worst


def check(channels, geometry, u, p, viscosity, density=1.0, fields=(), ub=None):
    """channels (5 + 2 nf, n) of a sample.  geometry: the dict of
    cfd_surface_geometry_get.  u (N, 2), p (N): the float32 state.  fields: dicts of
    phi (float32 [N]), diffusivity, wall = None or (kind, value, box).  ub: None or
    (ubx [n], uby [n], moved [n]), the float32 wall velocity of the moved faces.
    Returns the worst error / bound per group."""
    u, p = np.asarray(u), np.asarray(p)
    assert u.dtype == F and p.dtype == F
    i = np.asarray(geometry["cell"], np.int64)
    n = len(i)
    channels = np.asarray(channels, np.float64)
    assert channels.shape == (5 + 2 * len(fields), n), channels.shape
    for k in ("nx", "ny", "area", "dist_e"):  # the geometry is float32 widened
        g = np.asarray(geometry[k], np.float64)
        assert np.array_equal(g.astype(F).astype(np.float64), g), f"f64 geometry {k} is not float32 widened"
    nx, ny, ad, dist = (_fr(geometry[k]) for k in ("nx", "ny", "area", "dist_e"))
    worst = {}
    assert np.array_equal(channels[0].view(np.uint64), p[i].astype(np.float64).view(np.uint64)), "f64 channel 0 is not p of the cell"
    pc = _fr(p[i])
    for c, nrm, name in ((1, nx, "force_p.x"), (2, ny, "force_p.y")):
        exact = [a * b * s for a, b, s in zip(pc, nrm, ad)]
        worst[name] = _close(channels[c], exact, [abs(e) for e in exact], name)
    nu = Fraction(float(F(viscosity)))
    for c, comp, name in ((3, 0, "force_v.x"), (4, 1, "force_v.y")):
        uc = _fr(u[i, comp])
        if ub is not None:
            moved = np.asarray(ub[2], bool)
            assert np.asarray(ub[comp]).dtype == F
            w = [b if m else Fraction(0) for b, m in zip(_fr(ub[comp]), moved)]
        else:
            w = [Fraction(0)] * n
        exact = [nu * (a - b) * s / d for a, b, s, d in zip(uc, w, ad, dist)]
        mag = [nu * (abs(a) + abs(b)) * s / d for a, b, s, d in zip(uc, w, ad, dist)]
        worst[name] = _close(channels[c], exact, mag, name)
    cx, cy = np.asarray(geometry["cx"], np.float64), np.asarray(geometry["cy"], np.float64)
    for f, fd in enumerate(fields):
        phi = np.asarray(fd["phi"])
        assert phi.dtype == F
        ph = _fr(phi[i])
        assert np.array_equal(channels[6 + 2 * f].view(np.uint64), phi[i].astype(np.float64).view(np.uint64)), \
            f"f64 channel {6 + 2 * f} is not phi of the cell"
        wall = fd.get("wall")
        exact, mag = [Fraction(0)] * n, [Fraction(0)] * n
        if wall is not None and wall[0] != 0:
            kind, value, (x0, y0, x1, y1) = wall
            sel = (cx >= x0) & (cx <= x1) & (cy >= y0) & (cy <= y1) & (not x1 < x0)
            v = Fraction(float(F(value)))
            if kind == 1:  # the coefficient is a float32 value by definition: two float32 roundings
                rd = F(density) * F(fd["diffusivity"])
                ck = _fr(rd * np.asarray(geometry["area"]).astype(F) / np.asarray(geometry["dist_e"]).astype(F))
                exact = [c * (v - a) if s else Fraction(0) for c, a, s in zip(ck, ph, sel)]
                mag = [abs(c) * (abs(v) + abs(a)) if s else Fraction(0) for c, a, s in zip(ck, ph, sel)]
            else:
                exact = [v * s_ if s else Fraction(0) for s_, s in zip(ad, sel)]
                mag = [abs(e) for e in exact]
        name = f"flux[{f}]"
        worst[name] = _close(channels[5 + 2 * f], exact, mag, name)
        off = [j for j in range(n) if mag[j] == 0 and exact[j] == 0]
        assert not np.any(np.signbit(channels[5 + 2 * f][off])), f"f64 {name}: an unselected slot is not +0"
    return worst
