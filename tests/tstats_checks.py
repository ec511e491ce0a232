"""What the time statistics must equal, from the mathematics alone: the exact
weighted mean and covariances of a recorded sample sequence, and how far the
incremental float64 update may be from them.

Exact values.  Samples and weights are float32, so each is an integer times
2^-149; with w_k, x_k, y_k as those integers (Python ints, exact)
    mean  = sum w x / sum w                                  (times 2^-149)
    cov   = (sum w x y * sum w - sum w x * sum w y) / (sum w)^2   (times 2^-298)
are ratios of integers, and int / int true division rounds them to float64
correctly.  No rounding enters before that last one.

Bounds (u = 2^-53, the unit roundoff; EPS = 2u; k samples; X, Y the largest
|x|, |y| of the cell's samples; rho_j = w_j / W_j, so that an error made at step
j reaches step k multiplied by at most W_j / W_k <= 1, and by w_j / W_k when it
sits in the term rho_j d_j; the w_j / W_k sum to 1).
 mean, step j:  W_j is a sum of j weights, j - 1 roundings, and r_j = w_j / W_j
   one more: r_j is off by j u relatively.  d_j = x_j - m_{j-1} rounds once, the
   product r_j d_j once: the term, at most rho_j 2X in size, is off by
   (j + 2) u relatively.  The sum m + r d rounds once, u X.  Together
     |m_k - mean| <= sum_j (w_j / W_k) 2X (j + 2) u + sum_j (W_j / W_k) X u
                  <= (2 (k + 2) + k) u X = (3k + 4) u X
   to first order in u.  MEAN_BOUND doubles it, (3k + 4) EPS X = c k EPS X with
   c <= 7: the doubling covers the higher-order terms and the half-ulp of the
   exact value's own rounding.
 covariance, step j:  d_j inherits the mean's error of step j - 1 and one
   rounding, e_j that of step j and one rounding: each within (3k + 4) u + 2 u
   of X (or Y).  The term (w d) e, at most w_j 4XY in size, has two product
   roundings.  Its error is at most
     w_j [2X ((3k + 4) + 2) u Y + 2Y ((3k + 4) + 2) u X + 2 u 4XY] = w_j (12k + 32) u XY.
   The sum M + term rounds once: u |M_j| <= u W_j 4XY.  So
     |M_k - exact| <= W_k (12k + 32 + 4k) u XY,
   and dividing by the computed W_k (k - 1 roundings, the division 1 more) adds
   k u |cov| <= k u XY:  |M_k / W_k - cov| <= (17k + 32) u XY to first order.
   COV_BOUND doubles it as above: (17k + 32) EPS XY.
 For k <= 64 these are 196 EPS X = 4.4e-14 X and 1120 EPS XY = 2.5e-13 XY,
 below 1e-12: f32 accumulators (1e-7), unweighted averaging, a covariance
 against the new mean twice and M / samples (all O(1) of the value) lie far
 outside."""
import numpy as np

EPS = 2.0 ** -52
SCALE = 2.0 ** 149


def mean_bound(k, X):
    return (3 * k + 4) * EPS * X


def cov_bound(k, X, Y):
    return (17 * k + 32) * EPS * X * Y


def _ints(a):
    a = np.asarray(a)
    assert a.dtype == np.float32
    return [int(v) for v in (a.astype(np.float64) * SCALE).tolist()]


def exact(xs, ys, weights):
    """xs, ys: K float32 arrays of n cells (ys None: the mean of xs alone);
    weights: K float32.  Returns (mean_x, cov_xy) as float64 arrays, correctly
    rounded; cells with a non-finite sample are NaN."""
    K, n = len(xs), len(xs[0])
    ok = np.ones(n, bool)
    for a in list(xs) + (list(ys) if ys is not None else []):
        ok &= np.isfinite(a)
    idx = np.nonzero(ok)[0]
    w = _ints(np.asarray(weights, np.float32))
    sw = sum(w)
    X = [_ints(a[idx]) for a in xs]
    mean = np.full(n, np.nan)
    cov = np.full(n, np.nan)
    Y = [_ints(a[idx]) for a in ys] if ys is not None else None
    for c, i in enumerate(idx):
        swx = sum(w[k] * X[k][c] for k in range(K))
        mean[i] = swx / (sw << 149)
        if Y is not None:
            swy = sum(w[k] * Y[k][c] for k in range(K))
            swxy = sum(w[k] * X[k][c] * Y[k][c] for k in range(K))
            cov[i] = (swxy * sw - swx * swy) / ((sw * sw) << 298)
    return mean, cov


def _amax(arrs):
    return np.max(np.abs(np.stack([a.astype(np.float64) for a in arrs])), axis=0)


def check_mean(got, xs, weights, what="mean"):
    """got against the exact weighted mean of xs, cell by cell, within MEAN_BOUND; NaN exactly where a sample is"""
    want, _ = exact(xs, None, weights)
    bad = np.isnan(want)
    assert np.array_equal(np.isnan(got), bad), f"{what}: NaN cells differ"
    err = np.abs(got[~bad] - want[~bad])
    bound = mean_bound(len(xs), _amax(xs)[~bad])
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    assert np.all(err <= bound), f"{what}: off by {worst:.3g} x the bound"
    return worst


def check_cov(got, xs, ys, weights, what="cov"):
    _, want = exact(xs, ys, weights)
    bad = np.isnan(want)
    assert np.array_equal(np.isnan(got), bad), f"{what}: NaN cells differ"
    err = np.abs(got[~bad] - want[~bad])
    bound = cov_bound(len(xs), _amax(xs)[~bad], _amax(ys)[~bad])
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if err.size else 0.0
    assert np.all(err <= bound), f"{what}: off by {worst:.3g} x the bound"
    return worst


def check_all(get, kinds, seq, weights):
    """every (kind, field) of `kinds` from get(kind, field) against the recorded
    sequence seq: a list of dicts u, v, p (float32 arrays) and phi (a list)"""
    def series(name, f):
        return [s["phi"][f] if name == "phi" else s[name] for s in seq]

    pairs = {"uu": ("u", "u"), "uv": ("u", "v"), "vv": ("v", "v"), "pp": ("p", "p"), "phiphi": ("phi", "phi"),
             "uphi": ("u", "phi"), "vphi": ("v", "phi")}
    worst = {}
    for kind, f in kinds:
        got = get(kind, f)
        if kind in pairs:
            a, b = pairs[kind]
            worst[(kind, f)] = check_cov(got, series(a, f), series(b, f), weights, f"<{kind}> field {f}")
        else:
            worst[(kind, f)] = check_mean(got, series(kind, f), weights, f"<{kind}> field {f}")
    return worst
