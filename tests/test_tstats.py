"""The time statistics on the CPU: the numpy restatement (tests/tstats_ref.py)
against the exact weighted mean and covariances (tests/tstats_checks.py), the
wrong conventions those checks reject, the update's exact properties, and the
monitor's ring bookkeeping."""
import numpy as np
import pytest

from tests import tstats_cases as TC
from tests import tstats_checks as K
from tests import tstats_ref as R

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("kind", TC.KINDS)
@pytest.mark.parametrize("drive", ("u", "p"))
def test_restatement_passes_the_checks(kind, drive):
    n, nf = 257, 2
    seq = TC.sequence(n, nf, kind, drive)
    st = TC.run(seq, TC.WEIGHTS, True, nf)
    assert st.samples == 5 and st.planes.shape == (R.plane_count(True, nf), n) == (15, n)
    worst = K.check_all(st.get, st.kinds(), seq, TC.WEIGHTS)
    print(kind, drive, "worst error / bound", max(worst.values()))
    # after every sample, not only at the end
    TC.run(seq, TC.WEIGHTS, True, nf, each=lambda k, s: K.check_all(s.get, s.kinds(), seq[:k + 1], TC.WEIGHTS[:k + 1]))


def test_bounds_stay_tight_up_to_64_samples():
    for k in range(1, 65):
        assert K.mean_bound(k, 1.0) < 1e-12 and K.cov_bound(k, 1.0, 1.0) < 1e-12
    # and a 64-sample sequence stays inside them
    n, nf = 33, 1
    seq = TC.sequence(n, nf, "unit", K=64)
    w = (0.25 + np.random.default_rng(5).random(64)).astype(F)
    st = TC.run(seq, w, True, nf)
    K.check_all(st.get, st.kinds(), seq, w)


@pytest.mark.parametrize("name", sorted(R.WRONG))
def test_checks_reject_wrong_variants(name):
    n, nf = 64, 1
    kinds = ("unit", "offset") if name == "f32_accumulators" else ("unit",)
    for kind in kinds:
        seq = TC.sequence(n, nf, kind)
        good = TC.run(seq, TC.WEIGHTS, True, nf)
        K.check_all(good.get, good.kinds(), seq, TC.WEIGHTS)
        bad = TC.run(seq, TC.WEIGHTS, True, nf, cls=R.WRONG[name])
        with pytest.raises(AssertionError, match="x the bound"):
            K.check_all(bad.get, bad.kinds(), seq, TC.WEIGHTS)


def test_one_sample_is_exact():
    n, nf = 65, 4
    seq = TC.sequence(n, nf, "offset", K=1)
    st = TC.run(seq, [F(0.37)], True, nf)
    s = seq[0]
    for kind, f in st.kinds():
        q, cov = st.plane_of(kind, f)
        if cov:
            assert np.array_equal(bits(st.planes[q]), np.zeros(n, np.uint64)), kind  # +0, not -0
        else:
            x = s["phi"][f] if kind == "phi" else s[kind]
            assert np.array_equal(bits(st.planes[q]), bits(x.astype(np.float64))), kind


def test_constant_sequence_has_zero_moments():
    n, nf = 65, 2
    one = TC.sequence(n, nf, "offset", K=1)[0]
    st = TC.run([one] * 5, TC.WEIGHTS, True, nf)
    for kind, f in st.kinds():
        q, cov = st.plane_of(kind, f)
        if cov:
            assert not st.planes[q].any(), kind
        else:
            x = one["phi"][f] if kind == "phi" else one[kind]
            assert np.array_equal(st.planes[q], x.astype(np.float64)), kind


def test_doubling_every_weight_changes_no_bit():
    n, nf = 129, 1
    seq = TC.sequence(n, nf, "unit")
    a = TC.run(seq, TC.WEIGHTS, True, nf)
    b = TC.run(seq, 2 * TC.WEIGHTS, True, nf)
    assert b.W == 2 * a.W
    for kind, f in a.kinds():
        assert np.array_equal(bits(a.get(kind, f)), bits(b.get(kind, f))), kind


def test_uv_is_symmetric_within_the_bound():
    n = 129
    seq = TC.sequence(n, 0, "unit")
    swapped = [dict(s, u=s["v"], v=s["u"]) for s in seq]
    a = TC.run(seq, TC.WEIGHTS, True, 0).get("uv")
    b = TC.run(swapped, TC.WEIGHTS, True, 0).get("uv")
    X = np.max(np.abs([s["u"] for s in seq]), axis=0).astype(np.float64)
    Y = np.max(np.abs([s["v"] for s in seq]), axis=0).astype(np.float64)
    assert np.all(np.abs(a - b) <= 2 * K.cov_bound(5, X, Y))
    assert not np.array_equal(bits(a), bits(b))  # (w d_u) e_v and (w d_v) e_u round differently: the bound is needed


def test_a_nan_stays_in_its_cell():
    n, nf = 257, 1
    seq = TC.sequence(n, nf, "nan")
    clean = [dict(s, u=np.where(np.isnan(s["u"]), F(0), s["u"]), phi=[np.where(np.isnan(p), F(0), p) for p in s["phi"]])
             for s in seq]
    a = TC.run(seq, TC.WEIGHTS, True, nf).planes
    b = TC.run(clean, TC.WEIGHTS, True, nf).planes
    c = n // 2
    keep = np.arange(n) != c
    assert np.array_equal(bits(a[:, keep]), bits(b[:, keep]))
    # u and field 0 carry the NaN: every plane they enter is NaN in that cell, v's and p's are not
    assert np.isnan(a[[0, 3, 4, 7, 8, 9, 10], c]).all() and not np.isnan(a[[1, 2, 5, 6], c]).any()


def test_ring_bookkeeping():
    assert R.ring(0, 3) == ([], [])
    assert R.ring(2, 3) == ([0, 1], [0, 1])
    assert R.ring(3, 3) == ([0, 1, 2], [0, 1, 2])
    assert R.ring(5, 3) == ([2, 3, 4], [2, 0, 1])  # the wrap: oldest first, sample k in slot k % capacity
    assert R.ring(7, 1) == ([6], [0])
