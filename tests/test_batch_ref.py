"""CPU tests of tests/_batch_ref.py, the numpy restatement of one problem of the batched alignment: its passes against the oracle's
pass on the cat pair, the three modes from the perturbed known answer (the guesses tests/test_gpu_batch.py reuses), and every stop
path of the loop on a constructed case -- the threshold, max_iters, fixed_iters, the eps rule and a degenerate record."""
import os

import numpy as np
import pytest

import _batch_ref as B
import _record_ref as RR

f32 = np.float32
MODES = (RR.MODE_PAPER, RR.MODE_P2P, RR.MODE_PLANE)
# "converged": the source moved by the result lies within this rms distance of where the known answer puts it -- a hundredth of the
# cat's point spacing (1.38: a quarter of the 5.53 its FPFH radius is quoted as four spacings of)
CONVERGED_RMS = 0.0138


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def small(cat):
    """every fourth point of the cat pair (850 points, the same rows of both clouds): the stop-path cases"""
    return {k: cat[k][::4].copy() for k in ("src", "src_n", "tgt", "tgt_n")}


@pytest.fixture(scope="module")
def fixed10(sym, small):
    """ten fixed PAPER iterations from the first guess: the diffs the threshold cases are cut from"""
    g = B.perturbed(B.CAT_TRUTH, (0, 0, 1), 3.0, (1.0, -0.5, 0.25), small["tgt"].astype(np.float64).mean(0))
    return g, B.run(sym, RR.MODE_PAPER, small["src"], small["src_n"], small["tgt"], small["tgt_n"], g, max_iters=10, fixed_iters=1)


@pytest.mark.parametrize("mode", (RR.MODE_PAPER, RR.MODE_P2P))
def test_pass_matches_the_oracles_pass(oracle, cat, mode):
    """one_pass against the oracle: its apply, its brute-force pairs and its 40-double reduction, at the identity and at a guess, with
    and without the gates"""
    pivot = B.pivot_ref(cat["tgt"])
    for X in (np.eye(4, dtype=f32), B.cat_guesses(cat)[3]):
        for mcd, mnd in ((0.0, -2.0), (3.0, 0.5)):
            S, M, n = B.one_pass(mode, X, cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], pivot, mcd, mnd)
            p, pn = oracle.apply(X, cat["src"]), oracle.apply(X, cat["src_n"], False)
            idx, _ = oracle.nn_brute(p, cat["tgt"])
            So = oracle.reduce40(p, pn, cat["tgt"], cat["tgt_n"], idx, pivot, float(RR.f32_max_d2(mcd)), mnd, p2p=(mode == RR.MODE_P2P))
            assert 0 < n <= len(cat["src"]) and So[34] == n
            assert (mcd == 0.0) == (n == len(cat["src"]))
            RR.assert_record(S, So, M, RR.TOL_EXACT, (mode, mcd, mnd))


def test_pivot_is_the_fp64_mean(cat):
    pv = B.pivot_ref(cat["tgt"])
    assert pv.dtype == f32 and np.allclose(pv, cat["tgt"].astype(np.float64).mean(0), rtol=1e-7, atol=0)


@pytest.mark.parametrize("mode", MODES)
def test_reference_converges_from_the_perturbed_answer(sym, cat, mode):
    """ten iterations from each of the six guesses end at the known answer; the guesses themselves are far from it"""
    for k, g in enumerate(B.cat_guesses(cat)):
        assert B.truth_error(g, cat) > 100 * CONVERGED_RMS, k
        r = B.run(sym, mode, cat["src"], None if mode == RR.MODE_PLANE else cat["src_n"], cat["tgt"], cat["tgt_n"], g, max_iters=10,
                  diff_threshold=0.0)
        err = B.truth_error(r["X"][-1], cat)
        print("mode %d guess %d: %d iterations, rms from the truth %.2e -> %.2e" % (mode, k, r["iters"], B.truth_error(g, cat), err))
        assert r["status"] == B.OK and r["iters"] == 10 and r["passes"] == 11 and len(r["records"]) == 11
        assert err < CONVERGED_RMS, (mode, k, err)


def test_stop_by_threshold(sym, small, fixed10):
    g, full = fixed10
    d = [float(x) for x in full["diffs"]] + [float(full["diff_final"])]
    assert d[0] > d[2] > d[4] > 0
    run = lambda thr: B.run(sym, RR.MODE_PAPER, small["src"], small["src_n"], small["tgt"], small["tgt_n"], g, max_iters=10, diff_threshold=thr)
    r = run(d[0] * 2)                      # below the threshold at once: no iteration
    assert (r["status"], r["iters"], r["passes"], len(r["diffs"])) == (B.OK, 0, 1, 0) and r["diff_initial"] == r["diff_final"] == f32(d[0])
    r = run(0.5 * (d[1] + d[2]))           # after the second iteration
    assert (r["status"], r["iters"], r["passes"]) == (B.OK, 2, 3)
    assert [float(x) for x in r["diffs"]] == d[:2] and float(r["diff_final"]) == d[2]
    r = run(d[2])                          # the loop runs WHILE diff > threshold: a diff at the threshold stops it
    assert r["iters"] == 2
    assert np.array_equal(r["X"][2], full["X"][2])


def test_stop_by_max_iters_and_fixed_iters(sym, small, fixed10):
    g, full = fixed10
    a = (small["src"], small["src_n"], small["tgt"], small["tgt_n"], g)
    r = B.run(sym, RR.MODE_PAPER, *a, max_iters=4, diff_threshold=0.0)
    assert (r["status"], r["iters"], r["passes"]) == (B.OK, 4, 5) and np.array_equal(r["X"][4], full["X"][4])
    r = B.run(sym, RR.MODE_PAPER, *a, max_iters=0, diff_threshold=0.0)
    assert (r["status"], r["iters"], r["passes"]) == (B.OK, 0, 1) and np.array_equal(r["X"][0], g)
    big = float(full["diff_initial"]) * 10
    assert B.run(sym, RR.MODE_PAPER, *a, max_iters=3, diff_threshold=big)["iters"] == 0
    r = B.run(sym, RR.MODE_PAPER, *a, max_iters=3, diff_threshold=big, fixed_iters=1)      # fixed_iters ignores the threshold
    assert (r["status"], r["iters"], r["passes"]) == (B.OK, 3, 4)


def test_stop_by_the_eps_rule(sym, small, fixed10):
    g, full = fixed10
    a = (small["src"], small["src_n"], small["tgt"], small["tgt_n"], g)
    er, et = 1e-4, 1e-3
    r = B.run(sym, RR.MODE_PAPER, *a, max_iters=10, diff_threshold=0.0, eps_rotation=er, eps_translation=et)
    assert r["status"] == B.OK and 1 < r["iters"] < 10 and r["passes"] == r["iters"] + 1      # the pass that applies the small increment ran
    inc = lambda k: r["X"][k + 1].astype(np.float64) @ np.linalg.inv(r["X"][k].astype(np.float64))
    assert B.small_increment(inc(r["iters"] - 1), 2 * er, 2 * et) and not B.small_increment(inc(0), er, et)
    # one bound alone does not arm the rule, and fixed_iters disables it
    assert B.run(sym, RR.MODE_PAPER, *a, max_iters=10, diff_threshold=0.0, eps_rotation=er)["iters"] == 10
    assert B.run(sym, RR.MODE_PAPER, *a, max_iters=10, fixed_iters=1, eps_rotation=er, eps_translation=et)["iters"] == 10


@pytest.mark.parametrize("mode", MODES)
def test_stop_by_a_degenerate_record(sym, small, mode):
    # collinear clouds: the normal equations are rank deficient
    t = np.linspace(0.0, 10.0, 50)
    line = np.stack([t, 2 * t, -t], 1).astype(f32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (50, 1))
    r = B.run(sym, mode, line + f32(0.01), nrm, line, nrm, max_iters=5, diff_threshold=0.0)
    assert (r["status"], r["iters"], r["passes"]) == (B.ERR_DEGENERATE, 0, 1) and len(r["diffs"]) == 1
    assert np.array_equal(r["X"][-1], np.eye(4, dtype=f32))
    # every pair gated: an empty record
    r = B.run(sym, mode, small["src"], small["src_n"], small["tgt"], small["tgt_n"], max_iters=5, diff_threshold=-1.0, max_corr_dist=1e-3)
    assert (r["status"], r["iters"]) == (B.ERR_DEGENERATE, 0) and r["last"][34] == 0 and r["diff_final"] == 0
