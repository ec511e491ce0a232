"""Fields for GpuSolver.set_penalty, built from the cell centres of a mesh.

Pure numpy.  Each builder returns ``dict(sigma=..., forch=..., target=...)``
(float64 arrays over the cells; ``forch`` / ``target`` None where the case has
none), so that ``solver.set_penalty(**porous_box(mesh, box, 50.0))`` works, and
two fields can be combined by adding their ``sigma``.
"""
from __future__ import annotations

import numpy as np


def _centres(mesh):
    a = mesh.arrays()
    return np.asarray(a["cell_cx"], np.float64), np.asarray(a["cell_cy"], np.float64)


def porous_box(mesh, box, sigma, forch=0.0):
    """A Darcy(-Forchheimer) medium: ``sigma`` (and ``forch``) in the cells whose
    centre lies in the closed ``box`` (x0, y0, x1, y1), 0 elsewhere; at rest."""
    x, y = _centres(mesh)
    x0, y0, x1, y1 = box
    inside = (x >= x0) & (x <= x1) & (y >= y0) & (y <= y1)
    return dict(sigma=np.where(inside, float(sigma), 0.0),
                forch=np.where(inside, float(forch), 0.0) if forch else None, target=None)


def solid_disc(mesh, centre, radius, eta, density, dt, omega=0.0):
    """A solid disc by Brinkman penalisation: ``sigma = density / eta`` in the
    cells whose centre lies within ``radius`` of ``centre``; the target is the
    rigid rotation ``omega`` about the centre (None for a disc at rest).  ``eta``
    is the penalisation time: the velocity inside relaxes towards the target as
    exp(-t / eta), so eta well below ``dt`` makes the disc solid within a step;
    ``dt`` is only checked against it."""
    if not (eta > 0 and density > 0 and dt > 0 and radius > 0):
        raise ValueError("solid_disc: eta, density, dt and radius must be > 0")
    if eta > dt:
        raise ValueError(f"solid_disc: eta = {eta} above dt = {dt}: the disc would not be solid within a step")
    x, y = _centres(mesh)
    rx, ry = x - centre[0], y - centre[1]
    inside = rx * rx + ry * ry <= radius * radius
    target = None
    if omega:
        target = np.stack([np.where(inside, -omega * ry, 0.0), np.where(inside, omega * rx, 0.0)], 1)
    return dict(sigma=np.where(inside, float(density) / float(eta), 0.0), forch=None, target=target)


def sponge(mesh, x0, x1, sigma_max):
    """A sponge layer: sigma rises smoothly in x from 0 at ``x0`` to ``sigma_max``
    at ``x1`` (t^2 (3 - 2 t), zero slope at both ends), 0 before x0 and
    sigma_max beyond x1; at rest."""
    if not x1 > x0:
        raise ValueError("sponge: x1 must be above x0")
    x, _ = _centres(mesh)
    t = np.clip((x - x0) / (x1 - x0), 0.0, 1.0)
    return dict(sigma=float(sigma_max) * t * t * (3.0 - 2.0 * t), forch=None, target=None)
