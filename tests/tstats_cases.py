"""Sample sequences for the time statistics: what the CPU tests run through the
restatement and the GPU tests feed to the device with set_u / set_p /
set_scalar (float32 values, so both see the same numbers)."""
import numpy as np

from tests import tstats_ref as R

F = np.float32
# 5 unequal weights; the second is 2^20 times the first
WEIGHTS = np.array([2.0 ** -10, 2.0 ** 10, 1.5, 0.7, 3.0], F)
KINDS = ("unit", "offset", "nan")
FORMS = [(m2, nf) for m2 in (False, True) for nf in (0, 1, 4)]  # every kernel form
STRIPS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1025)


def sequence(n, nf, kind, drive="u", seed=0, K=5):
    """K samples of n cells: dicts of float32 u, v, p and phi (nf arrays).
    drive "u": u, v and the fields vary and p is 0 (set_u zeroes p); "p": p
    varies, u = v = 0 and the fields stay at the first sample's values.
    kind "unit": standard normal; "offset": 1e3 + 1e-3 * noise, a large mean
    under a small fluctuation; "nan": unit with a NaN in cell n // 2 of sample 2
    (u and field 0)."""
    rng = np.random.default_rng([seed, n, nf, KINDS.index(kind), drive == "p"])

    def noise():
        x = rng.standard_normal(n)
        return (1e3 + 1e-3 * x if kind == "offset" else x).astype(F)

    z = np.zeros(n, F)
    seq = []
    phi0 = [noise() for _ in range(nf)]
    for k in range(K):
        if drive == "u":
            s = dict(u=noise(), v=noise(), p=z, phi=[noise() for _ in range(nf)])
            if kind == "nan" and k == 2:
                s["u"][n // 2] = np.nan
                if nf:
                    s["phi"][0][n // 2] = np.nan
        else:
            s = dict(u=z, v=z, p=noise(), phi=phi0)
        seq.append(s)
    return seq


def run(seq, weights, second_moments, nf, cls=R.Stats, each=None):
    """the restatement (or a wrong variant) over a sequence; each(k, stats) after every sample"""
    st = cls(len(seq[0]["u"]), second_moments, nf)
    for k, (s, w) in enumerate(zip(seq, weights)):
        st.accumulate(s["u"], s["v"], s["p"], s["phi"], w)
        if each:
            each(k, st)
    return st
