"""CPU tests of the numpy restatement of trimmed ICP (tests/_trim_ref.py): the rank formula, ties, the edge cases, and what the
feature is for -- an fp64 point-to-plane loop on a partial-overlap pair, lost without trimming and found with it."""
import math

import numpy as np

import _trim_ref as T

f32 = np.float32


def test_rank_formula():
    # k = ceil(double(fp32 rho) * n_c), clamped to [1, n_c]
    assert T.trim_k(0.5, 7) == 4
    assert T.trim_k(0.5, 8) == 4
    assert T.trim_k(0.25, 8) == 2 and T.trim_k(0.25, 9) == 3
    assert T.trim_k(1.0, 11) == 11
    assert T.trim_k(1e-9, 5) == 1                      # clamped from below
    assert T.trim_k(0.5, 1) == 1 and T.trim_k(1e-9, 1) == 1
    assert T.trim_k(0.5, 0) == 0
    # rho is an fp32 value: fp32 0.6 = 0.60000002384185791015625 lies above 0.6, so 0.6 * 10 lands just above 6 in double and
    # the ceiling is 7, where the decimal 0.6 would give 6; fp32 0.9 lies below 0.9 and gives 9 either way
    assert float(f32(0.6)) > 0.6 and float(f32(0.9)) < 0.9
    assert T.trim_k(0.6, 10) == 7 == math.ceil(float(f32(0.6)) * 10.0)
    assert math.ceil(0.6 * 10) == 6
    assert T.trim_k(0.9, 10) == 9
    # 0.1 in fp32 is above 0.1 as well: 0.1 * 10 -> 2, not 1
    assert T.trim_k(0.1, 10) == 2
    # fp32 values whose double product lands ON an integer stay there: dyadic fractions
    for rho, n, k in ((0.75, 4, 3), (0.375, 8, 3), (0.5, 2 ** 30, 2 ** 29), (0.625, 2 ** 31 - 8, 5 * (2 ** 28 - 1))):
        assert float(f32(rho)) == rho
        assert T.trim_k(rho, n) == k, (rho, n)
    # an fp32 value just below 3/7 * 7 = 3 exactly? (3/7 is not dyadic: its fp32 rounding times 7 is not 3)
    r = f32(3.0 / 7.0)
    assert T.trim_k(r, 7) == (3 if float(r) * 7.0 <= 3.0 else 4)
    # the product is taken in double: fp32 would round 0.3f * 16777217 differently
    n = 16777217
    assert T.trim_k(0.3, n) == math.ceil(float(f32(0.3)) * n)


def test_ties_are_all_kept():
    k, tau, keep = T.trim_select(np.array([0, 0, 1, 1, 1, 2, 5], f32), 0.5)
    assert (k, float(tau), int(keep.sum())) == (4, 1.0, 5)
    assert keep.tolist() == [True, True, True, True, True, False, False]
    # any order of the candidates
    k, tau, keep = T.trim_select(np.array([5, 1, 0, 2, 1, 0, 1], f32), 0.5)
    assert (k, float(tau), int(keep.sum())) == (4, 1.0, 5)


def test_fraction_one_keeps_all():
    d2 = np.random.default_rng(1).random(1000).astype(f32)
    k, tau, keep = T.trim_select(d2, 1.0)
    assert k == 1000 and tau == d2.max() and keep.all()


def test_one_and_no_candidate():
    k, tau, keep = T.trim_select(np.array([3.5], f32), 0.25)
    assert (k, float(tau), keep.tolist()) == (1, 3.5, [True])
    k, tau, keep = T.trim_select(np.zeros(0, f32), 0.25)
    assert (k, float(tau), keep.size) == (0, 0.0, 0)


def test_trim_pass_counts_gated_pairs_out():
    """candidates are the pairs that exist and pass the gates; the rank is taken among them"""
    n = 8
    p = np.zeros((n, 3), f32)
    p[:, 0] = np.arange(n)
    pn = np.tile(f32([0, 0, 1]), (n, 1))
    q = p.copy()
    q[:, 1] = f32([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 3.0, 0.05])
    qn = pn.copy()
    qn[7] = (0, 0, -1)                                  # dropped by the normal gate
    idx = np.arange(n)
    idx[0] = -1                                         # no pair
    r = T.trim_pass(p, pn, q, qn, idx, 0.5, max_d2=1.0, min_ndot=0.0)
    assert r["cand"].tolist() == [False, True, True, True, True, True, False, False]
    assert r["n_c"] == 5 and r["k"] == 3
    assert r["tau"] == f32(0.3) * f32(0.3)
    assert r["kept"].tolist() == [False, True, True, True, False, False, False, False]


def test_partial_overlap_needs_trimming():
    """point-to-plane, exact nearest neighbours, fp64, 30 fixed iterations on the partial-overlap surface pair (n = 20 000, seed
    0xC4: 57 % of the source has a counterpart).  Measured: untrimmed ends 34-64 spacings rms from the truth, rho = 0.5 ends
    0.004-0.007 spacings away."""
    d = T.partial_overlap(20000, 0xC4)
    assert abs(d["spacing"] - math.sqrt(0.7 / 20000)) < 1e-15
    plain = T.rms_spacings(T.plane_icp_fp64(d, 1.0, 30), d)
    trimmed = T.rms_spacings(T.plane_icp_fp64(d, 0.5, 30), d)
    print("rms from the truth in spacings: untrimmed %.3f, rho = 0.5 %.5f" % (plain, trimmed))
    assert plain > 10.0, plain
    assert trimmed < 0.05, trimmed
