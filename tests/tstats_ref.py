"""Numpy restatement of the time statistics (include/cfd2_amd.h "Arithmetic of
the time statistics") and of the monitor's ring bookkeeping.  Every operation
is one elementwise float64 numpy call, so each rounds once and nothing is
fused; no sum or dot whose order numpy would choose.  The device must match it
bit for bit."""
import numpy as np

D = np.float64
KINDS = {"u": 0, "v": 1, "p": 2, "uu": 3, "uv": 4, "vv": 5, "pp": 6, "phi": 7, "phiphi": 8, "uphi": 9, "vphi": 10}


def plane_count(second_moments, nf):
    return 3 + (4 if second_moments else 0) + nf * (4 if second_moments else 2)


class Stats:
    """planes (P, n) float64 in the header's order, W, samples"""

    def __init__(self, n, second_moments=True, nf=0):
        self.n, self.m2, self.nf = n, bool(second_moments), nf
        self.planes = np.zeros((plane_count(second_moments, nf), n), D)
        self.W = D(0.0)
        self.samples = 0

    def reset(self):
        self.planes[:] = 0.0
        self.W = D(0.0)
        self.samples = 0

    def _mean(self, q, x, r):
        m = self.planes[q]
        d = x - m
        m = m + r * d
        self.planes[q] = m
        return d, x - m

    def accumulate(self, u, v, p, phis, weight):
        """u, v, p and every phi: float32 arrays of n cells; weight: what the call passes as a float32"""
        assert all(a.dtype == np.float32 and a.shape == (self.n,) for a in (u, v, p, *phis)) and len(phis) == self.nf
        w = D(np.float32(weight))
        Wn = self.W + w
        r = w / Wn
        P = self.planes
        du, eu = self._mean(0, u.astype(D), r)
        dv, ev = self._mean(1, v.astype(D), r)
        dp, ep = self._mean(2, p.astype(D), r)
        wdu, wdv = w * du, w * dv
        q = 3
        if self.m2:
            P[3] = P[3] + wdu * eu
            P[4] = P[4] + wdu * ev
            P[5] = P[5] + wdv * ev
            P[6] = P[6] + (w * dp) * ep
            q = 7
        for phi in phis:
            df, ef = self._mean(q, phi.astype(D), r)
            P[q + 1] = P[q + 1] + (w * df) * ef
            q += 2
            if self.m2:
                P[q] = P[q] + wdu * ef
                P[q + 1] = P[q + 1] + wdv * ef
                q += 2
        self.W = Wn
        self.samples += 1

    def plane_of(self, kind, field=0):
        k = KINDS[kind] if isinstance(kind, str) else int(kind)
        if k <= 2:
            return k, False
        if k <= 6:
            assert self.m2
            return k, True
        assert 0 <= field < self.nf and (k <= 8 or self.m2)
        return 3 + (4 if self.m2 else 0) + field * (4 if self.m2 else 2) + (k - 7), k >= 8

    def get(self, kind, field=0):
        q, cov = self.plane_of(kind, field)
        assert self.W > 0
        return self.planes[q] / self.W if cov else self.planes[q].copy()

    def kinds(self):
        """every (kind, field) these statistics hold"""
        out = [("u", 0), ("v", 0), ("p", 0)]
        if self.m2:
            out += [("uu", 0), ("uv", 0), ("vv", 0), ("pp", 0)]
        for f in range(self.nf):
            out += [("phi", f), ("phiphi", f)]
            if self.m2:
                out += [("uphi", f), ("vphi", f)]
        return out


def ring(total, capacity):
    """the monitor's ring after `total` records: the sample numbers still held,
    oldest first, and the slot of each (sample k lives in slot k % capacity)"""
    held = min(total, capacity)
    numbers = list(range(total - held, total))
    return numbers, [k % capacity for k in numbers]


# ---- wrong variants the checks must reject (tests/test_tstats.py) ----
class StatsF32(Stats):
    """f32 accumulators: the same update with every plane and every operation in float32"""

    def accumulate(self, u, v, p, phis, weight):
        s = Stats(self.n, self.m2, self.nf)
        s.planes = self.planes.astype(np.float32)
        s.W = np.float32(self.W)
        F = np.float32
        w = F(weight)
        Wn = F(s.W + w)
        r = F(w / Wn)
        P = s.planes

        def mean(q, x):
            d = x - P[q]
            P[q] = P[q] + r * d
            return d, x - P[q]

        du, eu = mean(0, u)
        dv, ev = mean(1, v)
        dp, ep = mean(2, p)
        q = 3
        if self.m2:
            P[3] += (w * du) * eu
            P[4] += (w * du) * ev
            P[5] += (w * dv) * ev
            P[6] += (w * dp) * ep
            q = 7
        for phi in phis:
            df, ef = mean(q, phi)
            P[q + 1] += (w * df) * ef
            q += 2
            if self.m2:
                P[q] += (w * du) * ef
                P[q + 1] += (w * dv) * ef
                q += 2
        self.planes = P.astype(D)
        self.W = D(Wn)
        self.samples += 1


class StatsUnweighted(Stats):
    """every sample counts 1, whatever its weight"""

    def accumulate(self, u, v, p, phis, weight):
        super().accumulate(u, v, p, phis, 1.0)


class StatsNewMeanTwice(Stats):
    """both factors of a covariance against the new mean: M += (w e_x) e_y"""

    def _mean(self, q, x, r):
        _, e = super()._mean(q, x, r)
        return e, e


class StatsOverSamples(Stats):
    """a covariance as M / samples in place of M / W"""

    def get(self, kind, field=0):
        q, cov = self.plane_of(kind, field)
        return self.planes[q] / D(self.samples) if cov else self.planes[q].copy()


WRONG = {"f32_accumulators": StatsF32, "unweighted": StatsUnweighted, "new_mean_twice": StatsNewMeanTwice,
         "over_samples": StatsOverSamples}
