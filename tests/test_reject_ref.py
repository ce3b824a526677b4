"""CPU tests of the numpy restatement of the one-to-one and median-distance rejectors (tests/_reject_ref.py): the winners against the
definition written as a double loop, ties, the median's threshold and its edge cases, the order of the rules, and what the rejectors
are for -- an fp64 point-to-plane loop on the partial-overlap pair, lost without rejection and found with either."""
import numpy as np
import pytest

import _reject_ref as J
import _trim_ref as T

f32 = np.float32


@pytest.mark.parametrize("seed", range(6))
def test_winners_against_the_double_loop(seed):
    """small random inputs: few targets (every target is claimed often), few distinct distances (forced ties in d2), rows that are
    no candidates"""
    rng = np.random.default_rng(seed)
    n, n_t = 40 + 7 * seed, 1 + 2 * seed
    idx = rng.integers(0, n_t, n)
    d2 = rng.choice(np.array([0.0, 0.25, 0.5, 1.0, 3.0], f32), n)
    cand = rng.random(n) < 0.8
    idx[~cand & (rng.random(n) < 0.5)] = -1
    cand &= idx >= 0
    win = J.winners(idx, d2, cand)
    assert (win == J.winners_loop(idx, J.bits(d2), cand)).all()
    # one winner per distinct claimed target, and only candidates win
    assert int(win.sum()) == len(np.unique(idx[cand]))
    assert not (win & ~cand).any()
    # ties in d2 occur among the claimants of one target, and the lowest row takes them
    tied = False
    for j in np.unique(idx[cand]):
        rows = np.flatnonzero(cand & (idx == j))
        best = d2[rows].min()
        tied |= int((d2[rows] == best).sum()) > 1
        assert np.flatnonzero(win & (idx == j)).tolist() == [rows[d2[rows] == best].min()]
    assert tied or seed == 0


def test_claim_key_orders_by_distance_then_row():
    K = J.claim_keys(f32([1.0, 1.0, 0.5, 0.0]), [0, 1, 2, 3])
    assert K[3] < K[2] < K[0] < K[1]
    assert int(K[1]) == (0x3F800000 << 32) | 1


def test_median_threshold():
    d2 = f32([4, 1, 3, 2, 100])                       # k = ceil(2.5) = 3 -> med = 3
    assert J.median_tau(d2, 2.0) == f32(12)
    assert J.median_tau(d2[:4], 1.0) == f32(2)        # k = 2: the lower median, trim_k(0.5, 4)
    # fp32 and unfused: factor * factor is rounded before it meets med
    fac, med = f32(1.1), f32(0.3)
    assert J.median_tau(f32([med]), fac) == f32(f32(fac * fac) * med)
    # no population: 0; an overflow keeps all; Inf * 0 counts as +Inf
    assert J.median_tau(np.zeros(0, f32), 2.0) == 0 and J.bits(J.median_tau(np.zeros(0, f32), 2.0))[0] == 0
    assert np.isposinf(J.median_tau(f32([1e30]), 1e10))
    assert np.isposinf(J.median_tau(f32([0.0]), 1e30))


def _toy():
    n = 8
    p = np.zeros((n, 3), f32)
    p[:, 0] = np.arange(n)
    pn = np.tile(f32([0, 0, 1]), (n, 1))
    q = np.zeros((3, 3), f32)
    q[:, 0] = (1.0, 4.0, 6.5)
    qn = np.tile(f32([0, 0, 1]), (3, 1))
    return p, pn, q, qn


def test_order_of_the_rules():
    """gates, then one-to-one, then the quantile over the survivors"""
    p, pn, q, qn = _toy()
    idx = np.array([0, 0, 0, 1, 1, 1, 2, -1])
    # d2: 1 0 1 | 1 0 1 | .25 | none
    r = J.reject_pass(p, pn, q, qn, idx, one_to_one=True)
    assert (r["n_c"], r["n_u"], r["n_kept"]) == (7, 3, 3)
    assert np.flatnonzero(r["uniq"]).tolist() == [1, 4, 6] and np.isposinf(r["tau"])
    # a gated pair claims nothing: with rows 1 and 4 gated out (d2 0 < ... no: gate by distance keeps them); gate the far ones instead
    r = J.reject_pass(p, pn, q, qn, idx, one_to_one=True, max_d2=0.5)
    assert (r["n_c"], r["n_u"]) == (3, 3)
    # ties at d2 = 1 go to the lowest row once the closest row is no candidate
    idx2 = idx.copy()
    idx2[1] = -1
    r = J.reject_pass(p, pn, q, qn, idx2, one_to_one=True)
    assert np.flatnonzero(r["uniq"]).tolist() == [0, 4, 6]
    # the median is taken over the survivors (d2 0, 0, .25: k = 2, med = 0 -> tau = 0), not over the candidates (med = 1)
    r = J.reject_pass(p, pn, q, qn, idx, one_to_one=True, factor=2.0)
    assert r["tau"] == 0 and np.flatnonzero(r["kept"]).tolist() == [1, 4]
    r = J.reject_pass(p, pn, q, qn, idx, factor=0.5)           # candidates: 0 0 .25 1 1 1 1 -> k = 4, med = 1, tau = .25
    assert r["tau"] == f32(0.25) and (r["n_u"], r["n_kept"]) == (7, 3)
    # ... and so is a trim fraction
    r = J.reject_pass(p, pn, q, qn, idx, one_to_one=True, rho=0.7)      # k = ceil(2.1) = 3
    assert r["n_kept"] == 3 and r["tau"] == f32(0.25)
    # identity pairing is one-to-one as it is
    r = J.reject_pass(p[:3], pn[:3], q, qn, None, one_to_one=True)
    assert r["n_u"] == r["n_c"] == 3
    with pytest.raises(AssertionError):
        J.reject_pass(p, pn, q, qn, idx, factor=2.0, rho=0.5)


@pytest.fixture(scope="module")
def overlap():
    return T.partial_overlap(20000, 0xC4)


def test_partial_overlap_is_lost_without_rejection(overlap):
    plain = T.rms_spacings(J.reject_icp_fp64(overlap, iters=30), overlap)
    print("rms from the truth in spacings, no rejection: %.3f" % plain)
    assert plain > 10.0, plain


@pytest.mark.parametrize("name, kw, kept0", [("one-to-one", dict(one_to_one=True), 6251), ("median 2", dict(factor=2.0), 13014),
                                             ("one-to-one + median 2", dict(one_to_one=True, factor=2.0), 5398)])
def test_partial_overlap_is_found_with_a_rejector(overlap, name, kw, kept0):
    """point-to-plane, exact nearest neighbours, fp64, 30 fixed iterations; the bound is the project's bound for this pair, 0.1 sample
    spacings.  Measured: one-to-one 0.01128, median 2 0.02434, both 0.00430."""
    counts = []
    end = T.rms_spacings(J.reject_icp_fp64(overlap, iters=30, counts=counts, **kw), overlap)
    print("%s: kept in pass 0 %d, rms from the truth in spacings %.5f" % (name, counts[0], end))
    assert counts[0] == kept0
    assert end < 0.1, end
