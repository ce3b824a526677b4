"""CPU tests that pin the numpy reference of the outlier filters (tests/_outlier_ref.py) alone: what tests/test_gpu_outlier.py compares
the device against is itself checked here, against an independent brute force, on pinned counts and on the cases it must get right."""
import math

import numpy as np
import pytest

import _outlier_ref as X

F = np.float32

# removed points and threshold of the exact reference on cat.pcd.  A quick fp64 cKDTree run of the same definition (distances of
# the float64 points, numpy mean and std) gives the same four counts and thresholds that agree to 9 digits (3.42439210, 6.08256147,
# 7.36438041, 10.09637503): the fp32 d2 moves an m_i by parts in 1e7, and no cat point sits that close to its threshold.
CAT_PINS = {(8, 1.0): (592, 3.424392103557942), (20, 2.0): (87, 6.082561472306473), (50, 1.0): (663, 7.364380408439051),
            (64, 2.0): (63, 10.096375028386259)}


def brute_mean_dist(xyz, k):
    """independent of _knn_ref: a Python loop over the rows, the own row removed by index, a stable sort of the values"""
    xyz = np.ascontiguousarray(xyz, F)
    out = np.empty(len(xyz))
    for i in range(len(xyz)):
        d = xyz[i] - xyz
        d2 = np.delete((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], i)
        s = 0.0
        for v in np.sort(d2)[:k].astype(np.float64).tolist():
            s = s + math.sqrt(v)
        out[i] = s / float(k)
    return out


@pytest.mark.parametrize("k,std_mul", sorted(CAT_PINS))
def test_cat_counts_and_thresholds_are_pinned(cat, k, std_mul):
    x = cat["src"]
    r = X.statistical(x, k, std_mul)
    removed, thr = CAT_PINS[(k, std_mul)]
    assert len(x) - len(r["rows"]) == removed
    assert r["thr"] == thr
    assert r["rows"].dtype == np.int32 and (np.diff(r["rows"]) > 0).all()
    assert np.array_equal(r["rows"], np.nonzero(r["mean_dist"] <= r["thr"])[0])


def test_reference_equals_an_independent_brute_force(cat, bunny):
    for x, k in ((cat["src"][:700], 8), (cat["src"][:700], 64), (bunny, 20), (bunny, len(bunny) - 1)):
        a, b = X.mean_dist(x, k), brute_mean_dist(x, k)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_sequential_sum_is_not_numpys_pairwise_sum(cat):
    """why the reference uses cumsum: np.sum over 64 values adds pairwise and differs in the last bits on some rows"""
    x = cat["src"]
    _, d2 = X.K.knn(x, 65)
    r = np.sqrt(d2[:, 1:].astype(np.float64))
    assert (np.cumsum(r, axis=1)[:, -1] != r.sum(axis=1)).any()


def test_duplicates_push_the_own_row_out_of_the_set():
    """70 copies of one point and k = 64: for the copies with a high row the 65 nearest are all copies with a lower row"""
    rng = np.random.default_rng(3)
    x = np.concatenate([np.tile(rng.random((1, 3)).astype(F), (70, 1)), rng.random((60, 3)).astype(F)])
    m = X.mean_dist(x, 64)
    assert (m[:70] == 0.0).all() and (m[70:] > 0).all()
    assert np.array_equal(m.view(np.uint64), brute_mean_dist(x, 64).view(np.uint64))


def test_noisy_cat_both_filters_remove_exactly_the_injected_points(cat):
    xyz, injected, origin = X.noisy_cat(cat["src"])
    assert injected.sum() == 55 and len(xyz) == 3400 + 55 and np.array_equal(xyz[~injected], cat["src"][origin[~injected]])
    for r in (X.statistical(xyz, 8, 1.0), X.radius(xyz, 4 * X.CAT_SPACING, 3)):
        removed = np.ones(len(xyz), bool)
        removed[r["rows"]] = False
        assert removed[injected].all()              # every injected point goes
        assert not removed[~injected].any()         # no surface point does


def test_all_points_identical():
    x = np.tile(np.array([[0.5, -1.25, 3.0]], F), (40, 1))
    r = X.statistical(x, 8, 1.0)
    assert (r["mean_dist"] == 0).all() and (r["mu"], r["sd"], r["thr"]) == (0.0, 0.0, 0.0)
    assert np.array_equal(r["rows"], np.arange(40))
    q = X.radius(x, 1.0, 39)
    assert (q["neighbors"] == 39).all() and len(q["rows"]) == 40 and len(X.radius(x, 1.0, 40)["rows"]) == 0


def test_statistics_formula():
    m = np.array([1.0, 2.0, 4.0, 9.0])
    mu, sd, thr = X.statistics(m, 0.5)
    assert mu == 4.0 and sd == np.sqrt((102.0 - 256.0 / 4.0) / 3.0) and thr == mu + 0.5 * sd
    assert np.array_equal(X.kept(m, thr), [0, 1, 2])
    mu, sd, thr = X.statistics(np.array([1.0, np.inf]), 1.0)          # an overflowed d2: the threshold is NaN and keeps nothing
    assert np.isnan(thr) and len(X.kept(np.array([1.0, np.inf]), thr)) == 0
