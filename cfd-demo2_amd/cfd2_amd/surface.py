"""Post-processing of wall surface distributions (pure numpy): orderings of a
surface's faces and the usual coefficients from ``GpuSolver.surface()`` /
``surface_stats()`` and ``surface_geometry()``.

The channels are the force of the fluid ON the wall, per face: ``force_p = p n
area`` and ``force_v = viscosity u_rel area / dist_e``, with ``n`` the normal out
of the fluid cell (into the wall).  The tangent is ``t = (-ny, nx)``: n rotated
by +90 degrees."""
import numpy as np


def order_by_angle(geometry, centre):
    """Permutation that walks the faces by the polar angle (-pi, pi] of their
    centre about ``centre``, ascending (a closed body such as a cylinder); ties
    keep the surface's own order."""
    cx, cy = np.asarray(geometry["cx"], np.float64), np.asarray(geometry["cy"], np.float64)
    return np.argsort(np.arctan2(cy - float(centre[1]), cx - float(centre[0])), kind="stable")


def order_by_x(geometry):
    """Permutation that walks the faces by ascending x of their centre (a flat
    wall, a step); ties by ascending y."""
    cx, cy = np.asarray(geometry["cx"], np.float64), np.asarray(geometry["cy"], np.float64)
    return np.lexsort((cy, cx))


def coefficients(surface, geometry, u_ref, density, p_ref=0.0, order=None):
    """Pressure and skin-friction coefficients of a sample (or of a mean).

    ``cp = (p - p_ref) / q`` and ``cf = tau_t / q`` with ``q = density u_ref^2 /
    2`` and ``tau_t = (force_v . t) / area``, t = (-ny, nx): the wall shear
    stress the fluid exerts, signed along the tangent.  ``separation``: the
    positions (x, y), shape (m, 2), where cf changes sign between consecutive
    faces of ``order`` (default: the surface's own order), interpolated
    linearly in cf between the two face centres; a face with cf exactly 0
    counts once, at its centre.  All arrays come back in the surface's own
    order; ``order`` only decides which faces are neighbours."""
    q = 0.5 * float(density) * float(u_ref) ** 2
    if not q > 0.0:
        raise ValueError("coefficients: density * u_ref^2 must be positive")
    nx, ny = np.asarray(geometry["nx"], np.float64), np.asarray(geometry["ny"], np.float64)
    area = np.asarray(geometry["area"], np.float64)
    cx, cy = np.asarray(geometry["cx"], np.float64), np.asarray(geometry["cy"], np.float64)
    fv = np.asarray(surface["force_v"], np.float64)
    cp = (np.asarray(surface["p"], np.float64) - float(p_ref)) / q
    tau = (fv[:, 0] * -ny + fv[:, 1] * nx) / area
    cf = tau / q
    o = np.arange(len(cf)) if order is None else np.asarray(order, np.int64)
    sep = []
    for a, b in zip(o[:-1], o[1:]):
        fa, fb = cf[a], cf[b]
        if fa == 0.0:
            sep.append((cx[a], cy[a]))
        elif fb != 0.0 and np.signbit(fa) != np.signbit(fb):  # signs, not the product: it can underflow to 0
            t = fa / (fa - fb)
            sep.append((cx[a] + t * (cx[b] - cx[a]), cy[a] + t * (cy[b] - cy[a])))
    if len(o) and cf[o[-1]] == 0.0:
        sep.append((cx[o[-1]], cy[o[-1]]))
    return dict(cp=cp, cf=cf, tau=tau, separation=np.array(sep, np.float64).reshape(-1, 2))
