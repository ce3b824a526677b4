"""The one-to-one and median-distance rejectors on the GPU (run with -m gpu on a real MI355X): symmicp_set_one_to_one,
symmicp_set_median_factor, the claim of target rows behind the first, and what they are for.

  1. the claim alone (symmicp_ctx_unique_probe) against the numpy restatement, exactly;
  2. every pass of a rejecting context against the restatement (tests/_reject_ref.py): the rejection state (n_c, n_u, kept, tau's
     bits), the record, the pair count and the reported pairs -- modes x pairings x rejections, with a Huber loss, with both gates,
     COLOR, IDENTITY, ties in d2 under both source orders, ragged sizes;
  3. off means off: both options switched off explicitly are bit for bit a context that never heard of them, a trimmed context is what
     it was, a rejecting align stays in the host loop, a setter acts at the next pass; which of the three state getters answers
     after a pass with which rejectors (with the reciprocal one of test_gpu_recip.py), and that none does after set_config / set_source;
  4. the refusals;
  5. the partial-overlap pair through Engine, MyICP (Python and C++) and the command-line driver.
The pairs of a pass come from a twin context without rejection driven by the same transforms (its pairs and distances are held to
the oracle's brute force by test_gpu_pass_matrix.py)."""
import os
import subprocess

import numpy as np
import pytest

import _record_ref as R
import _reject_ref as J
import _trim_ref as T
from conftest import ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def surf():
    return T.partial_overlap(20000, 0xC4)


def mode_code(sym, mode):
    return {"quirks": sym.MODE_QUIRKS, "paper": sym.MODE_PAPER, "p2p": sym.MODE_P2P, "plane": sym.MODE_PLANE, "gicp": sym.MODE_GICP}[mode]


def corr_code(sym, corr):
    return {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[corr]


REJECTIONS = {
    "one-to-one": dict(one_to_one=True),
    "median2": dict(factor=2.0),
    "one-to-one+median2": dict(one_to_one=True, factor=2.0),
    "one-to-one+rho0.7": dict(one_to_one=True, rho=0.7),
}


def apply_rejection(e, rej):
    """the options in the order the definition applies them"""
    if rej.get("one_to_one"):
        e.set_one_to_one(True)
    if rej.get("factor", 0.0) > 0:
        e.set_median_factor(rej["factor"])
    if rej.get("rho", 1.0) < 1:
        e.set_trim_fraction(rej["rho"])


def tau_bits(x):
    return int(f32(x).view(np.uint32))


# ---- 1. the claim -----------------------------------------------------------------------------------------------------------------
PROBE_SIZES = [1, 63, 64, 65, 257, 100_003]
PATTERNS = ["one-target", "random", "equal-d2"]


def probe_input(pattern, n, rng, unpaired):
    """-> (target rows, d2 bits, n_t).  d2 are non-negative fp32 drawn from few values, so ties in d2 occur wherever rows meet"""
    n_t = max(1, n // 3)
    d2 = (rng.integers(0, 6, n).astype(f32) * f32(0.125)).view(np.uint32).copy()
    if pattern == "one-target":
        rows = np.full(n, n_t - 1, np.int32)
    elif pattern == "random":
        rows = rng.integers(0, n_t, n).astype(np.int32)
    else:
        rows = rng.integers(0, n_t, n).astype(np.int32)
        d2[:] = np.uint32(0x3F000000)              # only the row decides
    if unpaired:
        rows[rng.random(n) < 0.3] = -1
        if n > 1:
            rows[0] = -7
    return rows, d2, n_t


@pytest.mark.parametrize("n", PROBE_SIZES)
def test_unique_probe_equals_the_restatement(sym, cat, n):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        e.set_one_to_one(True)
        e.set_median_factor(2.0)
        it0 = e.begin()

        def state():
            return (e.correspondences(), e.certificates(), e.index_info(), e.rejection_state(), e.one_to_one(), e.median_factor(), e.trim_fraction())
        before = state()
        for pi, pattern in enumerate(PATTERNS):
            for unpaired in (False, True):
                rows, d2, n_t = probe_input(pattern, n, np.random.default_rng(100 * pi + n % 997 + int(unpaired)), unpaired)
                win = e.unique_probe(rows, d2, n_t)
                cand = rows >= 0
                want = J.winners(rows, d2.view(f32), cand)
                assert np.array_equal(win, want), (pattern, unpaired, n, int((win != want).sum()))
                assert int(win.sum()) == len(np.unique(rows[cand]))
                if pattern == "one-target" and cand.any():
                    # one winner: the smallest d2 bits, then the lowest row
                    k = np.flatnonzero(cand)
                    assert np.flatnonzero(win).tolist() == [k[np.lexsort((k, d2[k]))[0]]]
                if pattern == "equal-d2":
                    # the lowest row of every target
                    first = {}
                    for i in np.flatnonzero(cand):
                        first.setdefault(int(rows[i]), int(i))
                    assert np.flatnonzero(win).tolist() == sorted(first.values())
        after = state()
        for a, b in zip(before[:2], after[:2]):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        assert str(before[2]) == str(after[2]) and before[3:] == after[3:]
        assert after[4:] == (True, 2.0, 1.0)
        # ... and the alignment goes on as one that was never probed
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as t:
            t.set_target(cat["tgt"], cat["tgt_n"])
            t.set_source(cat["src"], cat["src_n"])
            t.set_one_to_one(True)
            t.set_median_factor(2.0)
            assert np.array_equal(t.begin()["sums"], it0["sums"])
            assert np.array_equal(t.step()["sums"], e.step()["sums"])


def test_unique_probe_refuses_bad_arguments(sym):
    with sym.Engine() as e:
        rows, d2 = np.zeros(4, np.int32), np.zeros(4, np.uint32)
        for call in (lambda: e.unique_probe(rows[:0], d2[:0], 3), lambda: e.unique_probe(rows, d2, 0)):
            with pytest.raises(sym.SymmIcpError) as x:
                call()
            assert x.value.status == sym.ERR_ARG
        # a row at or past n_t is no pair
        assert e.unique_probe(np.array([0, 2, 0, 1], np.int32), np.array([5, 1, 5, 9], np.uint32), 2).tolist() == [True, False, False, True]


# ---- 2. every pass ----------------------------------------------------------------------------------------------------------------
def check_passes(sym, d, mode, corr, rej, loss=False, mcd=0.0, mnd=-2.0, steps=3, tag="", sort_source=None, bite=True):
    """begin and `steps` steps of a rejecting context against the numpy restatement; -> the number of passes checked"""
    m = mode_code(sym, mode)
    src, src_n, tgt, tgt_n = d["src"], d["src_n"], d["tgt"], d["tgt_n"]
    kw = dict(mode=m, corr=corr_code(sym, corr), max_iters=steps + 2, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=mnd)
    if sort_source is not None:
        kw["sort_source"] = sort_source
    max_d2 = R.f32_max_d2(mcd)
    identity = corr == "identity"
    o2o, factor, rho = bool(rej.get("one_to_one")), rej.get("factor", 0.0), rej.get("rho", 1.0)
    ref_kw = dict(one_to_one=o2o, factor=factor, rho=rho, max_d2=max_d2, min_ndot=mnd)
    with sym.Engine(**kw) as e, sym.Engine(**kw) as twin:
        for x in (e, twin):
            x.set_target(tgt, tgt_n)
            x.set_source(src, src_n)
        apply_rejection(e, rej)
        assert (e.one_to_one(), e.median_factor(), e.trim_fraction()) == (o2o, f32(factor), f32(rho))
        code, scale = 0, 1.0
        if loss:
            # a Huber scale that bites: the median |r| of the first pass's kept pairs, from the numpy rows
            twin.begin()
            idx0 = None if identity else twin.correspondences()[0]
            p0, pn0 = R.moved(np.eye(4), src, src_n, m)
            r0 = J.reject_pass(p0, pn0, tgt, tgt_n, idx0, **ref_kw)
            j0 = np.arange(len(src)) if identity else idx0
            k0 = r0["kept"]
            res = R.pass_terms(m, p0[k0], pn0[k0], tgt[j0[k0]], tgt_n[j0[k0]], np.zeros(3, f32))[1]
            scale = float(np.median(np.abs(res)))
            assert scale > 0
            code = sym.LOSS_HUBER
            e.set_robust_loss("huber", scale)
        it = e.begin()
        done = 0
        for k in range(steps + 1):
            t = "%s pass %d" % (tag, k)
            X = e.transform()
            twin.begin(guess=X)
            idx, d2 = twin.correspondences()
            p, pn = R.moved(X, src, src_n, m)
            if identity:
                assert np.array_equal(idx, np.arange(len(src)))
            ref = J.reject_pass(p, pn, tgt, tgt_n, None if identity else idx, **ref_kw)
            has = idx >= 0
            assert np.array_equal(d2[has], ref["d2"][has]), t
            nc, nu, kept, tau = e.rejection_state()
            print("%s: n_c %d n_u %d kept %d tau %g" % (t, nc, nu, kept, tau))
            assert (nc, nu, kept) == (ref["n_c"], ref["n_u"], ref["n_kept"]), (t, nc, nu, kept, ref["n_c"], ref["n_u"], ref["n_kept"])
            assert tau_bits(tau) == tau_bits(ref["tau"]), (t, tau, ref["tau"])
            if rho < 1:
                ts = e.trim_state()                      # (its candidates are the select's population)
                assert ts[:2] == (nu, kept) and tau_bits(ts[2]) == tau_bits(tau), (t, ts)
            S, M, n_kept = T.trimmed_record(m, p, pn, tgt, tgt_n, None if identity else idx, ref["kept"], e.pivot(), code, scale)
            assert n_kept == kept
            R.assert_record(it["sums"], S, M, R.TOL_REC if code else R.TOL_EXACT, t)
            assert it["pairs"] == kept, (t, it["pairs"], kept)
            if code and k == 0:
                assert 0.0 < S[34] < kept
            ie, _ = e.correspondences()
            assert np.array_equal(ie, np.where(ref["kept"], idx, -1)), (t, int((ie != np.where(ref["kept"], idx, -1)).sum()))
            if k == 0 and bite:
                # the rejector bites
                if o2o and not identity:
                    assert 0 < nu < nc, (t, nu, nc)
                if factor > 0 or rho < 1:
                    assert 0 < kept < nu, (t, kept, nu)
                if mcd > 0 or mnd > -1:
                    assert ref["n_c"] < int(has.sum()), "the gates dropped nothing"
            done += 1
            if k == steps:
                break
            it = e.step(check=False)
            if it["status"] != 0:
                break
        return done


GRID = [(m, c, r) for m in ("paper", "p2p", "plane", "gicp") for c in ("brute", "tree") for r in REJECTIONS]


@pytest.mark.parametrize("mode,corr,rej", GRID, ids=["%s-%s-%s" % g for g in GRID])
@pytest.mark.parametrize("loss", ["none", "huber"])
def test_every_pass(sym, cat, surf, mode, corr, rej, loss):
    for name, d in (("cat", cat), ("surface", surf)):
        assert check_passes(sym, d, mode, corr, REJECTIONS[rej], loss == "huber", tag=name) == 4, name


@pytest.mark.parametrize("mode", ["paper", "p2p", "plane", "gicp"])
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_every_pass_with_both_gates(sym, cat, surf, mode, corr):
    """a gated pair claims nothing: a distance gate at the 0.8 quantile of the first pass's distances, and every third source normal
    reversed under min_normal_dot = 0 (trimming's recipe)"""
    for name, d0 in (("cat", cat), ("surface", surf)):
        d = dict(d0, src_n=d0["src_n"].copy())
        d["src_n"][::3] *= -1
        d2_0 = R.nn_ref(d["src"], d["tgt"])[1]
        mcd = float(np.sqrt(np.quantile(d2_0, 0.8)))
        assert check_passes(sym, d, mode, corr, REJECTIONS["one-to-one+median2"], False, mcd, 0.0, tag=name) >= 2, name


@pytest.mark.parametrize("mode", ["paper", "plane"])
def test_identity_pairing(sym, cat, mode):
    """identity pairs are one-to-one: the option alone launches nothing and is bit for bit off; the median gets the every-pass check,
    with and without the option (n_u = n_c)"""
    kw = dict(mode=mode_code(sym, mode), corr=sym.CORR_IDENTITY, max_iters=6, fixed_iters=1)
    its = []
    for on in (False, True):
        with sym.Engine(**kw) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            if on:
                e.set_one_to_one(True)
            its.append([e.begin()] + [e.step() for _ in range(3)])
            with pytest.raises(sym.SymmIcpError) as x:
                e.rejection_state()
            assert x.value.status == sym.ERR_STATE
            assert (e.correspondences()[0] == np.arange(len(cat["src"]))).all()
    for a, b in zip(*its):
        assert np.array_equal(a["sums"], b["sums"]) and a["diff"] == b["diff"]
    assert check_passes(sym, cat, mode, "identity", dict(factor=1.5), tag="identity median") == 4
    assert check_passes(sym, cat, mode, "identity", dict(one_to_one=True, factor=1.5), tag="identity both") == 4


@pytest.mark.parametrize("corr", ["brute", "tree"])
@pytest.mark.parametrize("sort_source", [0, 1])
def test_ties_go_to_the_lowest_caller_row(sym, cat, corr, sort_source):
    """the source twice over: every claim ties on d2 with its copy's, and the copy in the first half must win whatever order the
    share is kept in"""
    s, sn = cat["src"], cat["src_n"]
    n = len(s)
    d = dict(src=np.concatenate([s, s]), src_n=np.concatenate([sn, sn]), tgt=cat["tgt"], tgt_n=cat["tgt_n"])
    assert check_passes(sym, d, "paper", corr, dict(one_to_one=True), tag="ties", sort_source=sort_source) == 4
    kw = dict(mode=sym.MODE_PAPER, corr=corr_code(sym, corr), max_iters=3, fixed_iters=1, sort_source=sort_source)
    with sym.Engine(**kw) as e, sym.Engine(**kw) as twin:
        for x in (e, twin):
            x.set_target(d["tgt"], d["tgt_n"])
            x.set_source(d["src"], d["src_n"])
        e.set_one_to_one(True)
        e.begin()
        twin.begin()
        idx, d2 = twin.correspondences()
        assert np.array_equal(idx[:n], idx[n:]) and np.array_equal(d2[:n], d2[n:])      # equal d2 bits among the claimants of one target
        ref = J.reject_pass(d["src"], d["src_n"], d["tgt"], d["tgt_n"], idx, one_to_one=True)
        ie = e.correspondences()[0]
        assert np.array_equal(ie >= 0, ref["uniq"])
        assert (ie[n:] == -1).all() and 0 < int((ie[:n] >= 0).sum()) == ref["n_u"] == len(np.unique(idx))
        assert e.rejection_state()[:3] == (2 * n, ref["n_u"], ref["n_u"])


@pytest.mark.parametrize("n_s", [1, 255, 257])
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_ragged_sizes(sym, cat, corr, n_s):
    d = dict(src=cat["src"][:n_s], src_n=cat["src_n"][:n_s], tgt=cat["tgt"], tgt_n=cat["tgt_n"])
    # (one source point: one candidate, which wins and is its own median -- nothing can bite)
    done = check_passes(sym, d, "paper", corr, REJECTIONS["one-to-one+median2"], tag="n_s=%d" % n_s, bite=n_s > 1)
    assert done >= (1 if n_s == 1 else 4)         # (one pair solves nothing: the step after the first pass is degenerate)


def test_color_mode(sym, oracle):
    """COLOR on its own fixture: the record of the kept set through the colour restatement"""
    import _color_ref as CR
    from symmicp import synth
    d = dict(synth.ridge_textured())
    d["tgt_g"] = sym.intensity_gradient(d["tgt"], d["tgt_n"], d["tgt_i"], 10)
    for corr in ("brute", "tree"):
        with sym.Engine(mode=sym.MODE_COLOR, corr=corr_code(sym, corr), max_iters=30, host_loop=1) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            e.set_target_intensity(d["tgt_i"], d["tgt_g"])
            e.set_source_intensity(d["src_i"])
            e.set_one_to_one(True)
            e.set_median_factor(2.0)
            it = e.begin()
            for k in range(3):
                X = e.transform()
                p, pn = oracle.apply(X, d["src"], True), oracle.apply(X, d["src_n"], False)
                pairs, rd = oracle.nn_brute(p, d["tgt"])
                ref = J.reject_pass(p, pn, d["tgt"], d["tgt_n"], pairs, one_to_one=True, factor=2.0)
                nc, nu, kept, tau = e.rejection_state()
                assert (nc, nu, kept, tau_bits(tau)) == (ref["n_c"], ref["n_u"], ref["n_kept"], tau_bits(ref["tau"])), (corr, k)
                if k == 0:
                    assert 0 < kept < nu < nc
                want = np.where(ref["kept"], pairs, -1)
                assert np.array_equal(e.correspondences()[0], want), (corr, k)
                S, M, kept_mask = CR.color_record(p, pn, d["src_i"], d["tgt"], d["tgt_n"], d["tgt_g"], d["tgt_i"], want, e.pivot(), CR.LAMBDA_DEFAULT)
                assert np.array_equal(kept_mask, ref["kept"])
                gpu = np.asarray(it["sums"], np.float64)
                err = np.abs(gpu[:37] - S[:37])
                bad = np.nonzero(err > 1e-9 * np.maximum(M[:37], 1e-300))[0]           # (test_gpu_color.py's comparison)
                assert bad.size == 0, (corr, k, [(int(b), gpu[b], S[b]) for b in bad[:6]])
                assert gpu[37] == S[37] and it["pairs"] == kept == int(ref["kept"].sum()), (corr, k)
                it = e.step()


# ---- 3. off means off ---------------------------------------------------------------------------------------------------------------
def _align_with_log(sym, d, set_off, **kw):
    with sym.Engine(**kw) as e:
        if set_off:
            e.set_one_to_one(0)
            e.set_median_factor(0.0)
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_loop_log(True)
        r = e.align()
        for call in (e.rejection_state, e.trim_state):
            with pytest.raises(sym.SymmIcpError) as x:
                call()
            assert x.value.status == sym.ERR_STATE
        return r, e.loop_log(), e.stats()


@pytest.mark.parametrize("data", ["cat", "cube100k"])
def test_off_is_bit_identical(sym, cat, data):
    from symmicp import synth
    d = cat if data == "cat" else synth.c3_uniform(100_000)
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1)
    ra, la, sa = _align_with_log(sym, d, True, **kw)
    rb, lb, sb = _align_with_log(sym, d, False, **kw)
    assert ra["status"] == rb["status"] == 0
    assert sa["loop_passes"] > 0 and sb["loop_passes"] > 0
    assert sa["loop_passes"] == sb["loop_passes"] and sa["passes"] == sb["passes"]
    assert ra["iters"] == rb["iters"] and ra["transform"].tobytes() == rb["transform"].tobytes()
    assert ra["diffs"].tobytes() == rb["diffs"].tobytes() and f32(ra["diff_final"]) == f32(rb["diff_final"])
    assert len(la) == len(lb) > 0
    for x, y in zip(la, lb):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    # ... and so are the records of single passes
    recs = []
    for set_off in (True, False):
        with sym.Engine(**dict(kw, max_iters=4)) as e:
            if set_off:
                e.set_one_to_one(0)
                e.set_median_factor(0.0)
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            recs.append([e.begin()["sums"].copy()] + [e.step()["sums"].copy() for _ in range(2)])
    for a, b in zip(*recs):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_a_trimmed_context_is_what_it_was(sym, cat, corr):
    """rho = 0.5 alone, with the new options at their defaults set explicitly: trim state, record and pairs through the existing
    restatement (tests/_trim_ref.py), and no rejection state"""
    m = sym.MODE_PAPER
    kw = dict(mode=m, corr=corr_code(sym, corr), max_iters=5, fixed_iters=1)
    identity = corr == "identity"
    with sym.Engine(**kw) as e, sym.Engine(**kw) as twin:
        for x in (e, twin):
            x.set_target(cat["tgt"], cat["tgt_n"])
            x.set_source(cat["src"], cat["src_n"])
        e.set_one_to_one(0)
        e.set_median_factor(0.0)
        e.set_trim_fraction(0.5)
        it = e.begin()
        for k in range(3):
            X = e.transform()
            twin.begin(guess=X)
            idx, _ = twin.correspondences()
            p, pn = R.moved(X, cat["src"], cat["src_n"], m)
            ref = T.trim_pass(p, pn, cat["tgt"], cat["tgt_n"], None if identity else idx, 0.5)
            nc, kept, tau = e.trim_state()
            assert (nc, kept, tau_bits(tau)) == (ref["n_c"], int(ref["kept"].sum()), tau_bits(ref["tau"]))
            with pytest.raises(sym.SymmIcpError) as x:
                e.rejection_state()
            assert x.value.status == sym.ERR_STATE
            S, M, _ = T.trimmed_record(m, p, pn, cat["tgt"], cat["tgt_n"], None if identity else idx, ref["kept"], e.pivot())
            R.assert_record(it["sums"], S, M, R.TOL_EXACT, "trim alone pass %d" % k)
            assert np.array_equal(e.correspondences()[0], np.where(ref["kept"], idx, -1))
            it = e.step()


@pytest.mark.parametrize("rej", list(REJECTIONS))
def test_rejecting_align_is_the_host_loop(sym, cat, rej):
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=12, fixed_iters=1)
    with sym.Engine(**kw) as e, sym.Engine(**kw) as s:
        for x in (e, s):
            x.set_target(cat["tgt"], cat["tgt_n"])
            x.set_source(cat["src"], cat["src_n"])
            apply_rejection(x, REJECTIONS[rej])
        e.set_loop_log(True)
        r = e.align()
        assert r["status"] == 0 and r["iters"] == 12
        assert e.stats()["loop_passes"] == 0 and len(e.loop_log()) == 0
        its = [s.begin()] + [s.step() for _ in range(12)]
        assert np.array_equal(r["diffs"], np.array([it["diff"] for it in its[:12]], f32))
        assert f32(r["diff_final"]) == f32(its[12]["diff"])
        assert r["transform"].tobytes() == s.transform().tobytes()
        a, b = e.rejection_state(), s.rejection_state()
        assert a[:3] == b[:3] and tau_bits(a[3]) == tau_bits(b[3])


def test_setters_act_at_the_next_pass(sym, cat):
    n = len(cat["src"])
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=10, fixed_iters=1) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        it = e.begin()
        assert it["pairs"] == n
        with pytest.raises(sym.SymmIcpError) as x:
            e.rejection_state()
        assert x.value.status == sym.ERR_STATE
        e.set_one_to_one(True)
        with pytest.raises(sym.SymmIcpError):
            e.rejection_state()                                  # (nothing happens before the next pass)
        it = e.step()
        nc, nu, kept, tau = e.rejection_state()
        assert nc == n and 0 < nu == kept == it["pairs"] < n and np.isposinf(tau)
        assert int((e.correspondences()[0] >= 0).sum()) == nu
        e.set_median_factor(1.0)
        assert e.rejection_state()[:3] == (nc, nu, kept)
        it = e.step()
        nc, nu2, kept2, tau = e.rejection_state()
        assert nc == n and T.trim_k(0.5, nu2) <= kept2 == it["pairs"] < nu2 and np.isfinite(tau)
        e.set_one_to_one(False)
        it = e.step()
        nc, nu3, kept3, _ = e.rejection_state()
        assert nc == nu3 == n and T.trim_k(0.5, n) <= kept3 == it["pairs"] < n
        e.set_median_factor(0.0)
        it = e.step()
        assert it["pairs"] == n
        with pytest.raises(sym.SymmIcpError) as x:
            e.rejection_state()
        assert x.value.status == sym.ERR_STATE
        assert (e.correspondences()[0] >= 0).all()


# ---- 3b. which getter answers after which pass -----------------------------------------------------------------------------------------
# Every allowed combination of the four rejectors on a 300-point source against a 257-point target (both ragged against 64 and 256:
# the tail lanes of the claim and the key kernels), and one IDENTITY row (257 against 257: identity pairing needs equal sizes).  The
# three state getters answer exactly after the passes their rejectors ran in; the expected figures are the numpy restatements' over
# the oracle's brute-force pairs.
QUANTILES = {"rho0.7": dict(rho=0.7), "median2": dict(factor=2.0), "noquantile": {}}
VALIDITY = [(c, q, o, r) for c in ("brute", "tree") for q in QUANTILES for o in (False, True) for r in (False, True)]
VALIDITY.append(("identity", "rho0.7", False, False))


@pytest.fixture(scope="module")
def ragged():
    """-> the clouds, and the pairs of the first pass from the identity (the oracle's brute force), shared and left unchanged"""
    from symmicp import synth
    d = synth.c4_surface(300)
    d = dict(src=d["src"], src_n=d["src_n"], tgt=d["tgt"][:257].copy(), tgt_n=d["tgt_n"][:257].copy())
    d["idx"] = R.nn_ref(d["src"], d["tgt"])[0]
    return d


def _getter(sym, call):
    """-> (status, values)"""
    try:
        return 0, call()
    except sym.SymmIcpError as x:
        return x.status, None


@pytest.mark.parametrize("corr,quantile,o2o,recip", VALIDITY, ids=["%s-%s-%s-%s" % (c, q, "o2o" if o else "many", "recip" if r else "forward") for c, q, o, r in VALIDITY])
def test_getters_validity_matrix(sym, ragged, corr, quantile, o2o, recip):
    import _recip_ref as RC
    identity = corr == "identity"
    m = sym.MODE_PAPER
    n_s = 257 if identity else 300
    src, src_n, tgt, tgt_n = ragged["src"][:n_s], ragged["src_n"][:n_s], ragged["tgt"], ragged["tgt_n"]
    idx = None if identity else ragged["idx"]
    rho, factor = QUANTILES[quantile].get("rho", 1.0), QUANTILES[quantile].get("factor", 0.0)
    p, pn = R.moved(np.eye(4), src, src_n, m)
    if recip:
        ref = RC.recip_pass(p, pn, tgt, tgt_n, idx, src, np.eye(4, dtype=f32), factor=factor, rho=rho)
        population, claimed = ref["n_r"], ref["n_u"]
    else:
        ref = J.reject_pass(p, pn, tgt, tgt_n, idx, one_to_one=o2o, factor=factor, rho=rho)
        population, claimed = ref["n_u"], None
    want_trim = (population, ref["n_kept"], tau_bits(ref["tau"])) if rho < 1 else None
    want_rej = (ref["n_c"], population, ref["n_kept"], tau_bits(ref["tau"])) if (factor > 0 or o2o or recip) else None
    want_recip = (claimed, population) if recip else None
    with sym.Engine(mode=m, corr=corr_code(sym, corr), max_iters=4, fixed_iters=1) as e:
        e.set_target(tgt, tgt_n)
        e.set_source(src, src_n)
        apply_rejection(e, dict(one_to_one=o2o, **QUANTILES[quantile]))
        if recip:
            e.set_reciprocal(True)

        def states():
            return [_getter(sym, g) for g in (e.trim_state, e.rejection_state, e.reciprocal_state)]
        assert [s for s, _ in states()] == [sym.ERR_STATE] * 3          # no pass yet
        e.begin()
        (st_t, t), (st_j, j), (st_r, r) = states()
        print("%s %s o2o=%d recip=%d: trim %s rejection %s reciprocal %s" % (corr, quantile, o2o, recip, t, j, r))
        assert (st_t, st_j, st_r) == tuple(0 if w is not None else sym.ERR_STATE for w in (want_trim, want_rej, want_recip))
        if want_trim:
            assert (t[0], t[1], tau_bits(t[2])) == want_trim
        if want_rej:
            assert (j[0], j[1], j[2], tau_bits(j[3])) == want_rej
        if want_recip:
            assert tuple(r) == want_recip and r[0] >= r[1]
            assert j[1] == r[1]                                         # the select's population is the survivors
        if want_trim and want_rej:
            assert t[1] == j[2] and tau_bits(t[2]) == tau_bits(j[3]) and j[1] == t[0]
        if want_rej and (identity or not (o2o or recip)):
            assert j[1] == j[0]                                         # no claim: every candidate is "unique"
        # ... and none of them answers for a pass that has not run under the new configuration or on the new source
        e.set_config(max_iters=5)
        assert [s for s, _ in states()] == [sym.ERR_STATE] * 3
        e.begin()
        assert [s for s, _ in states()] == [st_t, st_j, st_r]
        e.set_source(src, src_n)
        assert [s for s, _ in states()] == [sym.ERR_STATE] * 3


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(sym, call, status):
    with pytest.raises(sym.SymmIcpError) as x:
        call()
    assert x.value.status == status, x.value


def test_refusals(sym, cat):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        assert e.one_to_one() is False and e.median_factor() == 0.0
        e.set_median_factor(1.5)
        for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
            _refused(sym, lambda: e.set_median_factor(bad), sym.ERR_ARG)
            assert e.median_factor() == 1.5
        # the two quantile rules exclude each other, whichever comes second
        _refused(sym, lambda: e.set_trim_fraction(0.5), sym.ERR_ARG)
        assert e.trim_fraction() == 1.0
        e.set_trim_fraction(1.0)
        e.set_median_factor(0.0)
        e.set_trim_fraction(0.5)
        _refused(sym, lambda: e.set_median_factor(2.0), sym.ERR_ARG)
        assert e.median_factor() == 0.0
        e.set_median_factor(0.0)
        e.set_trim_fraction(1.0)
        # a rejecting context cannot become QUIRKS ...
        e.set_one_to_one(True)
        _refused(sym, lambda: e.set_config(mode=sym.MODE_QUIRKS), sym.ERR_ARG)
        e.cfg.mode = sym.MODE_PAPER
        e.set_one_to_one(False)
        e.set_median_factor(2.0)
        _refused(sym, lambda: e.set_config(mode=sym.MODE_QUIRKS), sym.ERR_ARG)
        e.cfg.mode = sym.MODE_PAPER
        _refused(sym, e.rejection_state, sym.ERR_STATE)          # no pass yet
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        _refused(sym, e.rejection_state, sym.ERR_STATE)
        e.begin()
        assert e.rejection_state()[0] == len(cat["src"])
        e.set_median_factor(0.0)
        e.begin()
        _refused(sym, e.rejection_state, sym.ERR_STATE)          # that pass rejected nothing
    # ... and a QUIRKS context takes neither option
    with sym.Engine(mode=sym.MODE_QUIRKS, corr=sym.CORR_IDENTITY) as e:
        _refused(sym, lambda: e.set_one_to_one(True), sym.ERR_ARG)
        _refused(sym, lambda: e.set_median_factor(2.0), sym.ERR_ARG)
        assert e.one_to_one() is False and e.median_factor() == 0.0
        e.set_one_to_one(False)
        e.set_median_factor(0.0)
    # sharded contexts: both orders
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.comm_init_rank(2, 0, None)
        _refused(sym, lambda: e.set_one_to_one(True), sym.ERR_STATE)
        _refused(sym, lambda: e.set_median_factor(2.0), sym.ERR_STATE)
        assert e.one_to_one() is False and e.median_factor() == 0.0
        e.set_one_to_one(False)
        e.set_median_factor(0.0)
    for opt in ("one", "median"):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
            if opt == "one":
                e.set_one_to_one(True)
            else:
                e.set_median_factor(2.0)
            _refused(sym, lambda: e.comm_init_rank(2, 1, None), sym.ERR_STATE)
            _refused(sym, lambda: e.comm_init_shm(2, 0, "symmicp_reject_test_%d" % os.getpid()), sym.ERR_STATE)
            assert e.local_count() == 0


# ---- 5. what they are for -----------------------------------------------------------------------------------------------------------
# The bound is the project's bound for this pair (tests/test_gpu_trim.py): 0.1 sample spacings.  The fp64 reference loop ends at
# 0.01128 (one-to-one), 0.02434 (median 2) and 0.00430 (both) (tests/test_reject_ref.py), 4 to 20 times below it, and the unrejected
# loop ends 400 times above it, so a rejector that rejects nothing cannot pass.
BOUND = 0.1
END_TO_END = {"one-to-one": dict(one_to_one=True), "median2": dict(factor=2.0), "both": dict(one_to_one=True, factor=2.0)}


def test_partial_overlap_through_engine(sym, surf):
    out = {}
    for name, rej in [("plain", {})] + list(END_TO_END.items()):
        with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1) as e:
            e.set_target(surf["tgt"], surf["tgt_n"])
            e.set_source(surf["src"], surf["src_n"])
            apply_rejection(e, rej)
            r = e.align()
            assert r["iters"] == 30
            out[name] = T.rms_spacings(r["transform"], surf)
            if rej:
                assert r["status"] == 0 and e.stats()["loop_passes"] == 0
    print("rms from the truth in spacings: %s" % ", ".join("%s %.5f" % kv for kv in out.items()))
    assert out["plain"] > 10.0, out
    for name in END_TO_END:
        assert out[name] <= BOUND, out


def levels_for(surf):
    return [(2.0 * surf["spacing"], 15, 0.0), (0.0, 30, 0.0)]


@pytest.mark.parametrize("name", list(END_TO_END))
def test_partial_overlap_through_python_myicp(sym, surf, name):
    icp = sym.MyICP(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1, verbose=False)
    icp.setInputSource(surf["src"], surf["src_n"])
    icp.setInputTarget(surf["tgt"], surf["tgt_n"])
    icp.setOneToOne(bool(END_TO_END[name].get("one_to_one")))
    icp.setMedianFactor(END_TO_END[name].get("factor", 0.0))
    r = icp.align()
    assert r["status"] == 0
    rms = T.rms_spacings(icp.getFinalTransformation(), surf)
    print("MyICP %s: %.5f spacings" % (name, rms))
    assert rms <= BOUND, rms


def test_partial_overlap_through_cpp_myicp(sym, surf, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_reject")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for name, arr in (("src", surf["src"]), ("src_n", surf["src_n"]), ("tgt", surf["tgt"]), ("tgt_n", surf["tgt_n"]),
                      ("levels", np.array(levels_for(surf), f32))):
        np.ascontiguousarray(arr, f32).tofile(tmp_path / (name + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rms = {k: T.rms_spacings(np.fromfile(tmp_path / ("out_%s.f32" % k), f32).reshape(4, 4), surf) for k in ("plain", "unique", "median", "both", "levels")}
    print("C++ MyICP: %s" % rms)
    assert rms["plain"] > 10.0, rms
    for k in ("unique", "median", "both"):
        assert rms[k] <= BOUND, rms


def test_partial_overlap_through_the_driver(sym, surf, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    sym.pcd_write(str(tmp_path / "a.pcd"), surf["src"], None, binary=True)
    sym.pcd_write(str(tmp_path / "b.pcd"), surf["tgt"], None, binary=True)
    args = ["--mode", "plane", "--corr", "tree", "--iters", "30", "--threshold", "0"]
    rms = {}
    for name, extra in (("plain", []), ("one-to-one", ["--one-to-one"]), ("median", ["--median-factor", "2"])):
        r = subprocess.run([exe] + args + extra + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")
        k = out.index("Result transform:")
        X = np.array([[float(v) for v in out[k + 1 + i].split()] for i in range(4)])
        rms[name] = T.rms_spacings(X, surf)
    print("icp_align: %s" % rms)
    assert rms["plain"] > 10.0 and rms["one-to-one"] <= BOUND and rms["median"] <= BOUND, rms
    # --median-factor needs a number > 0, no trim fraction beside it, and both need a mode other than quirks
    for bad in (["--median-factor", "0"], ["--median-factor", "-1"], ["--median-factor", "x"], ["--median-factor", "inf"],
                ["--mode", "paper", "--median-factor", "2", "--trim", "0.5"], ["--mode", "quirks", "--one-to-one"],
                ["--mode", "quirks", "--median-factor", "2"]):
        assert subprocess.run([exe, "--corr", "tree"] + bad + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True).returncode == 64, bad
