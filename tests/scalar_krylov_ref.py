"""The BiCGStab scalar solver restated in numpy -- TEST INFRASTRUCTURE ONLY.

Written from the prose of include/cfd2_amd.h ("Arithmetic of method 1"), not
from the kernels, on top of tests/scalar_ref.py (the assembled system, the
Jacobi sweep) and tests/refpy.canon_sum (the canonical sum).  Vectors are
float32 and every vector operation is one float32 rounding; the dots are
canonical sums of the float64 cell products; rho, alpha, omega and beta are
float64 and reach a vector operation rounded once to float32.  After a stop
x is not written again, so the batch size of the host's status reads cannot
show: there is none here.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import refpy
from tests.scalar_ref import F, ScalarRef

D64 = np.float64


@dataclass
class KrylovResult:
    phi: np.ndarray          # after the polish
    x: np.ndarray            # the frozen iterate of the Krylov phase
    iterations: int
    stop_reason: int         # 1 residual, 2 breakdown, 3 max_iters
    krylov_residual: np.float32
    polish_sweeps: int
    last_delta: np.float32
    converged: bool


def dot(a, b):
    return D64(refpy.canon_sum(a.astype(D64) * b.astype(D64)))


def maxabs(r):
    """max |r_i| as the device takes it: a NaN counts as +inf"""
    d = np.abs(r)
    return F(np.inf) if np.isnan(d).any() else F(d.max())


def _bad(v):
    return v == 0 or not np.isfinite(v)


class ScalarKrylovRef(ScalarRef):
    def apply(self, coef, diag, v):
        """(A v)_i = v_i - (sum over the internal slots of c_k v[o_k]) / diag_i, the sum from +0"""
        s = np.zeros(self.N, F)
        for k in range(self.S):
            m = self.internal[:, k]
            s[m] = s[m] + coef[m, k] * v[self.other[m, k]]
        out = v - s / diag
        assert out.dtype == F
        return out

    def krylov(self, coef, diag, b, x, tol=1e-6, max_iters=500):
        """the Krylov phase: (x, iterations, stop_reason, residual)"""
        tol = F(tol)
        x = np.asarray(x, F).copy()
        with np.errstate(all="ignore"):
            r = self.sweep(coef, diag, b, x) - x
            rh, p = r.copy(), r.copy()
            rho = dot(rh, r)
            res = maxabs(r)
            if res <= tol:
                return x, 0, 1, res
            k = 0
            while True:
                k += 1
                # a
                v = self.apply(coef, diag, p)
                d = dot(rh, v)
                alpha = rho / d
                af = F(alpha)
                if _bad(rho) or _bad(d) or _bad(af):
                    return x, k, 2, res
                # b
                s = r - af * v
                t = self.apply(coef, diag, s)
                ts, tt = dot(t, s), dot(t, t)
                if tt == 0:
                    x = x + af * p
                    return x, k, 2, maxabs(s)
                omega = ts / tt
                of = F(omega)
                if not np.isfinite(tt) or _bad(of):
                    return x, k, 2, res
                # c
                x = (x + af * p) + of * s
                r = s - of * t
                res = maxabs(r)
                rho1 = dot(rh, r)
                if res <= tol:
                    return x, k, 1, res
                if k == max_iters:
                    return x, k, 3, res
                # d
                beta = (rho1 / rho) * (alpha / omega)
                bf = F(beta)
                if _bad(rho1) or _bad(bf):
                    return x, k + 1, 2, res
                p = r + bf * (p - of * v)
                rho = rho1
                assert x.dtype == F and r.dtype == F and p.dtype == F

    def polish(self, coef, diag, b, phi, tol=1e-6, max_sweeps=200, check_interval=4):
        """the Jacobi loop of ScalarRef.advance from phi: (phi, sweeps, delta, converged)"""
        ci = int(check_interval)
        max_sweeps = -(-int(max_sweeps) // ci) * ci
        sweeps, delta, converged = 0, F(0), False
        while sweeps < max_sweeps:
            for _ in range(ci):
                prev = phi
                phi = self.sweep(coef, diag, b, prev)
            sweeps += ci
            d = np.abs(phi - prev)
            delta = F(np.inf) if np.isnan(d).any() else F(d.max())
            if not np.isfinite(delta):
                raise FloatingPointError("non-finite Jacobi update")
            if delta <= F(tol):
                converged = True
                break
        return phi, sweeps, delta, converged

    def advance_krylov(self, face_flux, density, dt, D, inlet_value, phi, tol=1e-6, max_sweeps=200, check_interval=4,
                       max_iters=500) -> KrylovResult:
        phi = np.asarray(phi, F)
        coef, diag, b = self.assemble(face_flux, density, dt, D, inlet_value, phi)
        x, it, reason, res = self.krylov(coef, diag, b, phi, tol, max_iters)
        out, sweeps, delta, conv = self.polish(coef, diag, b, x, tol, max_sweeps, check_interval)
        return KrylovResult(out, x, it, reason, res, sweeps, delta, conv)


def solve64(R: ScalarRef, coef, diag, b):
    """float64 direct solve of the same system (its float32 coefficients)"""
    import scipy.sparse as sp
    import scipy.sparse.linalg as spl
    rows, cols, vals = [np.arange(R.N)], [np.arange(R.N)], [diag.astype(D64)]
    for k in range(R.S):
        m = R.internal[:, k]
        rows.append(np.nonzero(m)[0])
        cols.append(R.other[m, k])
        vals.append(-coef[m, k].astype(D64))
    A = sp.csc_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(R.N, R.N))
    return spl.spsolve(A, b.astype(D64))


def breakdown_case(mesh):
    """Pure upwind on a rectangular channel mesh: u = (1, 0) everywhere (no flux
    through the horizontal faces), D = 0, a step profile.  The matrix is lower
    triangular in the flow direction and iteration 2 meets a zero denominator.
    Returns (u, phi0, D, inlet_value, dt)."""
    a = mesh.arrays()
    x = a["cell_cx"]
    u = np.tile([1.0, 0.0], (len(x), 1))
    phi0 = np.where(x < 0.3 * x.max(), 1.0, 0.0)
    return u, phi0, 0.0, 1.0, 0.2
