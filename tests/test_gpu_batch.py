"""The batched alignment on the GPU (symmicp_ctx_batch_align, icp-symm_amd/csrc/kernels_batch.hip): one workgroup per problem, the
whole loop inside it.

  1. every pass of every problem against numpy: the record of X_k = trace_X[b][k], formed by _record_ref about the returned pivot,
     against trace_sums[b][k] at TOL_EXACT (fp64 sums of exact terms: only the order differs) and the pair count exactly;
  2. chaining and the stop rule from the device's own records: X_{k+1} against mat4_mul(symmicp.solve(record_k), X_k) within the
     bound of tests/test_gpu_solve.py carried through the product, and iters, diffs, diff_initial, diff_final and status as
     _batch_ref.stop_rule gives them on the traced records;
  3. purity: a problem alone, in a batch of 37, in the permuted batch and run twice gives byte-identical result structs; 300
     problems (30 distinct ones, ten times each) give ten identical copies of what the 30 give alone;
  4. against the engine's host loop with brute-force pairs (a different order of the fp64 sums): the same iteration count,
     transforms within ENGINE_BOUND;
  5. edge shapes: the sizes around every split, sweep and tile edge of the kernel, B in {1, 2, 37}, sixteen guesses on one pair, PLANE
     without source normals, a problem whose every pair is gated, collinear clouds, max_iters = 0;
  6. the known answer from the perturbed guesses of tests/test_batch_ref.py, and alignMultiStart in Python and C++;
  7. a batch call between two symmicp_step calls leaves the context as it was."""
import os
import subprocess

import numpy as np
import pytest

import _batch_ref as B
import _record_ref as RR
import _solve_ref as SR
from conftest import ROOT
from test_batch_ref import CONVERGED_RMS

pytestmark = pytest.mark.gpu

f32 = np.float32
MODES = (RR.MODE_PAPER, RR.MODE_P2P, RR.MODE_PLANE)
OUT16_ULPS = 32          # tests/test_gpu_solve.py: device against host increment, per entry, in units of 2^-24 x the translations' scale
# Largest |transform entry - the engine's| measured over test_against_the_engine's problems on an MI355X: 1.421e-14 (DESIGN.md 4,
# "Batched alignment": every entry of magnitude 1 has the engine's bits, a near-zero entry of the rotation block differs); the bound is
# 4 x that, capped by the project's parity bar of 1e-4
ENGINE_MEASURED = 1.421e-14
ENGINE_BOUND = min(4 * ENGINE_MEASURED, 1e-4)

# (src_count, tgt_count): the smallest and largest clouds; the sizes around a wave (64), the workgroup (512), one sweep of kBatchQ x
# workgroup queries (2048) and the split thresholds of batch_splits (256, 512, 1024); target counts around the LDS tile (4096 = the
# limit), and around the edges of the target split: rows_per_split = 4 * ceil(ceil(nt / 4) / S) with S = 8, 4, 2
EDGE_SHAPES = [(1, 1), (1, 2), (3, 2), (3, 4096), (63, 31), (64, 32), (65, 33), (200, 36), (256, 29), (257, 16), (257, 17), (511, 4095),
               (512, 4096), (513, 9), (1024, 7), (1024, 8), (1025, 1500), (2047, 700), (2048, 3400), (2049, 3400), (4096, 4096), (4096, 1),
               (3400, 3400)]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def pools(cat):
    """the cat pair and, behind it, a jittered copy of its first 1000 rows: pools of 4400 rows, so that a range of 4096 exists"""
    rng = np.random.default_rng(20261019)
    def pool(xyz, nrm):
        return (np.concatenate([xyz, xyz[:1000] + rng.normal(0, 0.3, (1000, 3)).astype(f32)]).astype(f32),
                np.concatenate([nrm, nrm[:1000]]).astype(f32))
    sx, sn = pool(cat["src"], cat["src_n"])
    tx, tn = pool(cat["tgt"], cat["tgt_n"])
    return dict(src=sx, src_n=sn, tgt=tx, tgt_n=tn)


def edge_problems(pools, shapes):
    """row ranges for the shapes, at varied offsets (the same offset in both pools where the counts agree)"""
    Ns, Nt = len(pools["src"]), len(pools["tgt"])
    out = []
    for k, (ns, nt) in enumerate(shapes):
        sf = (k * 37) % (Ns - ns + 1)
        tf = sf if ns == nt else (k * 53) % (Nt - nt + 1)
        out.append((sf, ns, tf, nt))
    return out


def guesses_for(cat, n):
    g = B.cat_guesses(cat)
    return np.stack([g[k % len(g)] for k in range(n)])


def run_batch(eng, sym, pools, mode, problems, guesses, trace=True, **cfg):
    """-> dict(res = result dicts, X, S = traces, cfg, mode, problems, guesses)"""
    cfg = dict(dict(max_iters=3, diff_threshold=0.0), **cfg)
    src_n = None if mode == RR.MODE_PLANE else pools["src_n"]
    r = eng.batch_align(pools["src"], src_n, pools["tgt"], pools["tgt_n"], problems, guesses, trace=trace, mode=mode, **cfg)
    res, X, S = r if trace else (r, None, None)
    return dict(res=res, X=X, S=S, cfg=cfg, mode=mode, problems=problems, guesses=guesses, pools=pools)


@pytest.fixture(scope="module")
def traced(eng, sym, cat, pools):
    """about 40 problems across the three modes, three iterations each, traced: every edge shape in PAPER, every second one in P2P
    and PLANE (PLANE without source normals).  Shared by the record, chaining and edge tests."""
    runs = []
    for mode, shapes in ((RR.MODE_PAPER, EDGE_SHAPES), (RR.MODE_P2P, EDGE_SHAPES[1::2]), (RR.MODE_PLANE, EDGE_SHAPES[0::2])):
        probs = edge_problems(pools, shapes)
        runs.append(run_batch(eng, sym, pools, mode, probs, guesses_for(cat, len(probs))))
    assert sum(len(r["problems"]) for r in runs) >= 40
    return runs


def each_problem(runs):
    for run in runs:
        p = run["pools"]
        for b, (sf, ns, tf, nt) in enumerate(run["problems"]):
            src_n = np.zeros((ns, 3), f32) if run["mode"] == RR.MODE_PLANE else p["src_n"][sf:sf + ns]
            yield run, b, p["src"][sf:sf + ns], src_n, p["tgt"][tf:tf + nt], p["tgt_n"][tf:tf + nt]


def host_solve(sym, mode, pivot):
    def solve(S):
        r = sym.solve(mode, S, pivot)
        return r[0], np.asarray(r[6], f32).reshape(4, 4), r[5]
    return solve


# ---- 1. every pass against numpy ------------------------------------------------------------------------------------------------
def test_every_pass_matches_the_numpy_record(traced):
    n_pass = 0
    for run, b, src, src_n, tgt, tgt_n in each_problem(traced):
        r = run["res"][b]
        mean = tgt.astype(np.float64).mean(0)
        assert np.all(np.abs(r["pivot"] - mean) <= 1e-6 * np.abs(mean) + 1e-30), (run["mode"], b, r["pivot"], mean)
        passes = r["iters"] + 1
        for k in range(passes):
            S, M, n = B.one_pass(run["mode"], run["X"][b][k], src, src_n, tgt, tgt_n, r["pivot"])
            RR.assert_record(run["S"][b][k], S, M, RR.TOL_EXACT, (run["mode"], run["problems"][b], k))
            assert run["S"][b][k][34] == n == len(src)
            n_pass += 1
        assert not run["X"][b][passes:].any() and not run["S"][b][passes:].any()          # rows not reached stay zero
        assert np.array_equal(run["X"][b][0], run["guesses"][b].reshape(4, 4))
        assert np.array_equal(r["sums"], run["S"][b][passes - 1]) and r["pairs"] == r["sums"][34]
        assert np.array_equal(r["transform"], run["X"][b][passes - 1])
    assert n_pass > 100


def test_gates_match_the_numpy_record(eng, sym, cat, pools):
    """max_corr_dist (the fp32 square) and min_normal_dot on every pass, PAPER and P2P"""
    for mode in (RR.MODE_PAPER, RR.MODE_P2P):
        probs = edge_problems(pools, [(513, 513), (2049, 3400), (200, 36)])
        run = run_batch(eng, sym, pools, mode, probs, guesses_for(cat, 3), max_iters=2, max_corr_dist=2.5, min_normal_dot=0.7)
        for run_, b, src, src_n, tgt, tgt_n in each_problem([run]):
            r = run["res"][b]
            for k in range(r["iters"] + 1):
                S, M, n = B.one_pass(mode, run["X"][b][k], src, src_n, tgt, tgt_n, r["pivot"], 2.5, 0.7)
                RR.assert_record(run["S"][b][k], S, M, RR.TOL_EXACT, (mode, b, k))
                assert run["S"][b][k][34] == n
            S0, _, n0 = B.one_pass(mode, run["X"][b][0], src, src_n, tgt, tgt_n, r["pivot"])
            assert 0 < run["S"][b][0][34] < n0                                              # the gates dropped some pairs, not all


# ---- 2. chaining and the stop rule from the device's own records ----------------------------------------------------------------
def check_chain_and_rule(sym, run, b):
    r = run["res"][b]
    mode, pivot, cfg = run["mode"], r["pivot"], run["cfg"]
    solve = host_solve(sym, mode, pivot)
    want = B.stop_rule(lambda k, X: run["S"][b][k], solve, cfg, run["guesses"][b] if run["guesses"] is not None else None)
    tag = (mode, run["problems"][b], cfg)
    assert (r["status"], r["iters"]) == (want["status"], want["iters"]), (tag, r["status"], r["iters"], want["status"], want["iters"])
    assert r["diff_initial"] == want["diff_initial"] and r["diff_final"] == want["diff_final"], tag
    assert np.array_equal(r["diffs"][:len(want["diffs"])], np.array(want["diffs"], f32)[:64]), tag
    for k in range(r["iters"]):
        st, pb, qb, a, t, rc, Xi = sym.solve(mode, run["S"][b][k], pivot)
        assert st == 0, tag
        Xk = run["X"][b][k].astype(np.float64)
        if mode == RR.MODE_P2P:      # (symmicp.solve reports no centroids for P2P: the scale from the record's own)
            S = run["S"][b][k]
            scale = 1.0 + float(np.abs(S[27:30] / S[34] + pivot).sum() + np.abs(S[30:33] / S[34] + pivot).sum())
        else:
            scale = 1.0 + float(np.abs(pb).sum() + np.abs(qb).sum() + np.abs(t).sum())
        # every entry of the product sums four (increment entry x X_k entry): the increment's bound times the column's magnitudes
        bound = OUT16_ULPS * 2.0 ** -24 * scale * np.abs(Xk).sum(0)[None, :] + 4 * 2.0 ** -24 * (np.abs(Xi.astype(np.float64)) @ np.abs(Xk))
        err = np.abs(run["X"][b][k + 1].astype(np.float64) - SR.mat4_mul(Xi, run["X"][b][k]).astype(np.float64))
        assert np.all(err <= bound), (tag, k, err.max(), bound.min())
    if r["iters"] and r["status"] == 0:
        assert r["rcond"] == f32(sym.solve(mode, run["S"][b][r["iters"] - 1], pivot)[5]), tag
    return r


def test_chaining_and_stop_rule_on_the_traced_records(sym, traced):
    n_ok = 0
    for run in traced:
        for b in range(len(run["problems"])):
            r = check_chain_and_rule(sym, run, b)
            n_ok += r["status"] == 0 and r["iters"] == 3
    assert n_ok >= 30


def test_every_stop_path(eng, sym, cat, pools):
    """the threshold (at once, midway, exactly at a diff), max_iters, fixed_iters and the eps rule, each on six guesses"""
    probs = [(0, 850, 0, 850)] * 6
    g = guesses_for(cat, 6)
    base = run_batch(eng, sym, pools, RR.MODE_PAPER, probs, g, max_iters=10, fixed_iters=1)
    d = [float(x) for x in base["res"][0]["diffs"]] + [float(base["res"][0]["diff_final"])]
    assert all(r["iters"] == 10 and r["status"] == 0 for r in base["res"])
    seen = set()
    for cfg in (dict(diff_threshold=d[0] * 4), dict(diff_threshold=0.5 * (d[1] + d[2])), dict(diff_threshold=d[2]),
                dict(diff_threshold=0.0, max_iters=4), dict(diff_threshold=d[0] * 4, max_iters=3, fixed_iters=1),
                dict(diff_threshold=0.0, eps_rotation=1e-4, eps_translation=1e-3),
                dict(diff_threshold=0.0, eps_rotation=1e-4), dict(fixed_iters=1, eps_rotation=1e-4, eps_translation=1e-3)):
        run = run_batch(eng, sym, pools, RR.MODE_PAPER, probs, g, **dict(dict(max_iters=10), **cfg))
        for b in range(6):
            check_chain_and_rule(sym, run, b)
        seen.add((tuple(sorted(cfg)), run["res"][0]["iters"]))
    iters = sorted(i for _, i in seen)
    assert iters[0] == 0 and 2 in iters and 3 in iters and 4 in iters and 10 in iters
    assert any("eps_translation" in k and "fixed_iters" not in k and 1 < i < 10 for k, i in seen)      # the eps rule ended a run early


# ---- 3. purity --------------------------------------------------------------------------------------------------------------------
def mixed37(cat, pools):
    probs = edge_problems(pools, EDGE_SHAPES) + [(0, 3400, 0, 3400)] * 6 + edge_problems(pools, [(700, 650), (90, 1200), (1500, 1500), (300, 300),
                                                                                               (2500, 2000), (40, 40), (1100, 900), (128, 128)])
    assert len(probs) == 37
    return probs, guesses_for(cat, 37)


def raw(run):
    return [r["raw"] for r in run["res"]]


def test_purity_alone_in_a_batch_permuted_and_twice(eng, sym, cat, pools):
    probs, g = mixed37(cat, pools)
    whole = raw(run_batch(eng, sym, pools, RR.MODE_PAPER, probs, g, trace=False))
    assert len(set(whole)) > 30
    assert raw(run_batch(eng, sym, pools, RR.MODE_PAPER, probs, g, trace=False)) == whole                 # twice
    perm = np.random.default_rng(3).permutation(37)
    permuted = raw(run_batch(eng, sym, pools, RR.MODE_PAPER, [probs[i] for i in perm], g[perm], trace=False))
    assert [permuted[list(perm).index(b)] for b in range(37)] == whole
    for b in range(37):                                                                                    # alone (B = 1)
        assert raw(run_batch(eng, sym, pools, RR.MODE_PAPER, [probs[b]], g[b:b + 1], trace=False))[0] == whole[b], probs[b]
    two = raw(run_batch(eng, sym, pools, RR.MODE_PAPER, [probs[20], probs[4]], g[[20, 4]], trace=False))    # B = 2
    assert two == [whole[20], whole[4]]
    with sym.Engine() as other:                                                                            # another context, the same bits
        assert raw(run_batch(other, sym, pools, RR.MODE_PAPER, probs, g, trace=False)) == whole


def test_purity_300_problems_more_than_the_cus(eng, sym, cat, pools):
    shapes = [(64 + 37 * k, 50 + 61 * k) for k in range(24)] + [(2049, 1800), (1025, 2100), (3400, 3400), (513, 4096), (4096, 300), (2048, 2048)]
    probs = edge_problems(pools, shapes)
    g = guesses_for(cat, 30)
    for mode in (RR.MODE_PAPER, RR.MODE_PLANE):
        alone = [raw(run_batch(eng, sym, pools, mode, [probs[b]], g[b:b + 1], trace=False))[0] for b in range(30)]
        order = np.random.default_rng(5).permutation(300) % 30
        big = raw(run_batch(eng, sym, pools, mode, [probs[i] for i in order], g[order], trace=False))
        assert len(big) == 300 and len(set(alone)) == 30
        assert all(big[k] == alone[order[k]] for k in range(300))


# ---- 4. against the engine --------------------------------------------------------------------------------------------------------
def test_against_the_engine(eng, sym, cat, pools):
    """Engine(corr=BRUTE, host_loop=1, apply=CUMULATIVE, sort_source=0, fixed_iters=1): the same loop with the records summed in
    another order (and the pivot formed on the device).  The same iteration count; transforms entry by entry within ENGINE_BOUND."""
    shapes = [(3400, 3400), (64, 64), (513, 513), (1025, 1025), (2049, 2049)]
    worst = 0.0
    for mode in MODES:
        probs = [(0, 3400, 0, 3400)] * 6 + edge_problems(pools, shapes[1:])
        g = guesses_for(cat, len(probs))
        run = run_batch(eng, sym, pools, mode, probs, g, trace=False, max_iters=10, fixed_iters=1)
        with sym.Engine(mode=mode, corr=sym.CORR_BRUTE, host_loop=1, apply=sym.APPLY_CUMULATIVE, sort_source=0, fixed_iters=1, max_iters=10) as e:
            last = None
            for b, (sf, ns, tf, nt) in enumerate(probs):
                if (sf, ns, tf, nt) != last:
                    e.set_target(pools["tgt"][tf:tf + nt], pools["tgt_n"][tf:tf + nt])
                    e.set_source(pools["src"][sf:sf + ns], None if mode == RR.MODE_PLANE else pools["src_n"][sf:sf + ns])
                    last = (sf, ns, tf, nt)
                re = e.align(g[b])
                r = run["res"][b]
                assert (r["status"], re["status"]) == (0, 0) and r["iters"] == re["iters"] == 10, (mode, probs[b], r["status"], re["status"])
                diff = float(np.abs(r["transform"].astype(np.float64) - re["transform"].astype(np.float64)).max())
                worst = max(worst, diff)
                assert diff <= ENGINE_BOUND, (mode, probs[b], diff)
    print("batch against the engine: largest |transform difference| = %.3e (bound %.1e)" % (worst, ENGINE_BOUND))


# ---- 5. edge shapes ---------------------------------------------------------------------------------------------------------------
def test_edge_shapes_ran_every_branch(traced):
    """the traced runs hold every edge shape; their records and chains are checked above -- here: the small ones end DEGENERATE by
    the solve, alone, and the others ran their three iterations"""
    for run in traced:
        for b, (sf, ns, tf, nt) in enumerate(run["problems"]):
            r = run["res"][b]
            if ns >= 63 and nt >= 29:
                assert (r["status"], r["iters"]) == (0, 3), (run["mode"], ns, nt, r["status"], r["iters"])
            if ns == 1:
                assert (r["status"], r["iters"]) == (B.ERR_DEGENERATE, 0) and r["pairs"] == 1
            assert np.isfinite(r["transform"]).all() and r["pairs"] == ns


def test_sixteen_guesses_on_one_pair(eng, sym, cat, pools):
    g = guesses_for(cat, 16)
    for k in range(16):
        g[k, :3, 3] += f32(0.05 * k)
    for mode in MODES:
        run = run_batch(eng, sym, pools, mode, [(0, 3400, 0, 3400)] * 16, g, trace=False, max_iters=10)
        res = run["res"]
        assert all(r["status"] == 0 and r["iters"] == 10 for r in res)
        assert len(set(raw(run))) == 16 and all(np.array_equal(r["pivot"], res[0]["pivot"]) for r in res)
        assert all(B.truth_error(r["transform"], cat) < CONVERGED_RMS for r in res), [B.truth_error(r["transform"], cat) for r in res]
        for b in (0, 7, 15):
            assert raw(run_batch(eng, sym, pools, mode, [(0, 3400, 0, 3400)], g[b:b + 1], trace=False, max_iters=10))[0] == run["res"][b]["raw"]


def test_a_fully_gated_problem_is_degenerate_alone(eng, sym, cat, pools):
    probs = edge_problems(pools, [(513, 513), (1025, 1025), (300, 300), (2049, 2049)])
    g = guesses_for(cat, 4)
    far = g.copy()
    far[2, :3, 3] += f32(1000.0)                                   # problem 2 starts 1000 units off: every pair is beyond max_corr_dist
    kw = dict(trace=False, max_iters=3, max_corr_dist=8.0, fixed_iters=1)      # (fixed: an empty record's diff of 0 is not above any threshold >= 0)
    with_it = run_batch(eng, sym, pools, RR.MODE_PAPER, probs, far, **kw)
    r = with_it["res"][2]
    assert (r["status"], r["iters"], r["pairs"], r["diff_initial"], r["diff_final"]) == (B.ERR_DEGENERATE, 0, 0.0, 0.0, 0.0)
    assert np.array_equal(r["transform"], far[2]) and not r["sums"].any()
    keep = [0, 1, 3]
    without = run_batch(eng, sym, pools, RR.MODE_PAPER, [probs[b] for b in keep], g[keep], **kw)
    assert [with_it["res"][b]["raw"] for b in keep] == raw(without)
    assert all(x["status"] == 0 and x["iters"] == 3 and 0 < x["pairs"] for x in without["res"])


@pytest.mark.parametrize("mode", MODES)
def test_collinear_clouds_end_degenerate(eng, sym, mode):
    """Two lines of 70 points, the source shifted a little: one along x (rows 0 .. 69), one skew (rows 70 .. 139).  On the line along x
    every sum that could lift the rank is an exact zero, so the solve of every mode refuses the first iteration.  On the skew line
    PAPER's and PLANE's normal equations are refused the same way; P2P's solve (solve_core.h: the singular values through a Jacobi
    sweep of H^T H) sees a rank-one H only down to the sweep's rounding, about 1e-8 of the largest, against its bar of 1e-12 -- on
    the host as on the device -- so there the problem ends as the host's solve says on the traced records, whichever way."""
    t = np.arange(70, dtype=np.float64)
    z = np.zeros(70)
    line = np.concatenate([np.stack([t, z, z], 1), np.stack([t, 2 * t, -t], 1) / 7.0]).astype(f32)
    nrm = np.tile(np.array([[0.0, 0.0, 1.0]], f32), (140, 1))
    src = line + np.array([0.25, 0.0, 0.0], f32)
    probs, cfg = [(0, 70, 0, 70), (5, 50, 0, 70), (70, 70, 70, 70), (75, 50, 70, 70)], dict(max_iters=5, diff_threshold=0.0)
    res, X, S = eng.batch_align(src, None if mode == RR.MODE_PLANE else nrm, line, nrm, probs, trace=True, mode=mode, **cfg)
    run = dict(res=res, X=X, S=S, cfg=cfg, mode=mode, problems=probs, guesses=None)
    for b, r in enumerate(res):
        check_chain_and_rule(sym, run, b)
        assert r["pairs"] == probs[b][1] and r["diff_initial"] > 0 and np.array_equal(r["transform"], X[b][r["iters"]])
        if b < 2 or mode != RR.MODE_P2P:
            assert (r["status"], r["iters"]) == (B.ERR_DEGENERATE, 0) and np.array_equal(r["transform"], np.eye(4, dtype=f32)), (mode, b)


def test_max_iters_zero_and_the_module_function(eng, sym, cat, pools):
    g = guesses_for(cat, 2)
    run = run_batch(eng, sym, pools, RR.MODE_PAPER, [(0, 513, 0, 513), (0, 64, 0, 64)], g, max_iters=0)
    for b, r in enumerate(run["res"]):
        assert (r["status"], r["iters"]) == (0, 0) and np.array_equal(r["transform"], g[b]) and r["diff_initial"] == r["diff_final"] > 0
        assert run["X"].shape == (2, 1, 4, 4) and run["S"][b][0][34] == run["problems"][b][1]
    # symmicp.batch_align (a context of its own) and NULL guesses (the identity)
    a = sym.batch_align(pools["src"], pools["src_n"], pools["tgt"], pools["tgt_n"], [(0, 513, 0, 513)], max_iters=2, diff_threshold=0.0)
    b = eng.batch_align(pools["src"], pools["src_n"], pools["tgt"], pools["tgt_n"], [(0, 513, 0, 513)], np.eye(4, dtype=f32)[None], max_iters=2,
                        diff_threshold=0.0)
    assert a[0]["raw"] == b[0]["raw"] and a[0]["iters"] == 2
    with pytest.raises(sym.SymmIcpError) as err:
        eng.batch_align(pools["src"], pools["src_n"], pools["tgt"], pools["tgt_n"], [(0, 4097, 0, 513)])
    assert err.value.status == sym.ERR_SIZE and "4096" in str(err.value)


# ---- 6. known answer --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_known_answer_from_the_perturbed_guesses(eng, sym, cat, mode):
    g = B.cat_guesses(cat)
    res = eng.align_multistart(cat["src"], None if mode == RR.MODE_PLANE else cat["src_n"], cat["tgt"], cat["tgt_n"], g, mode=mode, max_iters=10,
                               diff_threshold=0.0)
    for k, r in enumerate(res):
        err = B.truth_error(r["transform"], cat)
        assert r["status"] == 0 and r["iters"] == 10 and err < CONVERGED_RMS, (mode, k, err)


def test_myicp_multistart_picks_a_converged_start(sym, cat):
    g = list(B.cat_guesses(cat))
    g.insert(2, B.perturbed(B.CAT_TRUTH, (0, 0, 1), 170.0, (40.0, 0, 0), cat["tgt"].astype(np.float64).mean(0)))      # a hopeless start
    m = sym.MyICP(mode=sym.MODE_PAPER, max_iters=10, diff_threshold=0.0, verbose=False)
    m.setInputSource(cat["src"], cat["src_n"])
    m.setInputTarget(cat["tgt"], cat["tgt_n"])
    best = m.alignMultiStart(np.stack(g))
    res = m.multiStartResults()
    assert len(res) == 7 and best != 2 and res[best]["status"] == 0
    key = lambda r: (r["pairs"], -r["diff_final"])
    assert all(r["status"] != 0 or key(r) < key(res[best]) or (key(r) == key(res[best]) and k >= best) for k, r in enumerate(res))
    assert np.array_equal(m.getFinalTransformation(), res[best]["transform"])
    assert B.truth_error(m.getFinalTransformation(), cat) < CONVERGED_RMS


def test_cpp_myicp_multistart(sym, cat, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_multistart")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    g = B.cat_guesses(cat)
    for name, arr in (("src", cat["src"]), ("src_n", cat["src_n"]), ("tgt", cat["tgt"]), ("tgt_n", cat["tgt_n"]), ("guesses", g)):
        np.ascontiguousarray(arr, f32).tofile(tmp_path / (name + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    best = np.fromfile(tmp_path / "out_best.f32", f32).reshape(4, 4)
    allr = np.fromfile(tmp_path / "out_all.f32", f32)
    assert B.truth_error(best, cat) < CONVERGED_RMS
    assert (allr[:4 * len(g)].reshape(-1, 4)[:, :2] == [0, 10]).all()
    with sym.Engine() as e:                                   # the same bits as the Python route
        res = e.align_multistart(cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], g, mode=sym.MODE_PAPER, max_iters=10, diff_threshold=0.0)
    assert np.array_equal(allr[4 * len(g):].reshape(-1, 4, 4), np.stack([r["transform"] for r in res]))


# ---- 7. the context is untouched --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("corr", ("BRUTE", "TREE"))
def test_a_batch_call_between_two_steps_leaves_the_context_alone(sym, cat, pools, corr):
    g = B.cat_guesses(cat)[1]
    def steps(with_call):
        with sym.Engine(mode=sym.MODE_PAPER, corr=getattr(sym, "CORR_" + corr), max_iters=10) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            out = [e.begin(g), e.step()]
            if with_call:
                r = e.batch_align(pools["src"], pools["src_n"], pools["tgt"], pools["tgt_n"], [(0, 2049, 0, 3400), (5, 300, 9, 300)],
                                  guesses_for(cat, 2), max_iters=3, diff_threshold=0.0)
                assert all(x["status"] == 0 and x["iters"] == 3 for x in r)
            out += [e.step(), e.step()]
            return out, e.transform(), e.pivot(), e.correspondences()
    (a, Xa, pa, ca), (b, Xb, pb, cb) = steps(False), steps(True)
    for x, y in zip(a, b):
        assert x["sums"].tobytes() == y["sums"].tobytes() and x["increment"].tobytes() == y["increment"].tobytes()
        assert (x["status"], x["iter"], x["diff"], x["rcond"], x["pairs"]) == (y["status"], y["iter"], y["diff"], y["rcond"], y["pairs"])
    assert np.array_equal(Xa, Xb) and np.array_equal(pa, pb) and all(np.array_equal(u, v) for u, v in zip(ca, cb))
