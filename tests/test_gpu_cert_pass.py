"""k_pass_certified: the pass of a converged alignment in which no pair needs a scan (icp-symm_amd/csrc/kernels_pass.hip), chosen per
chunk of passes by run_batch (engine_loop.cpp) and switched by SYMMICP_CERT_PASS (0: never, 1: by the rule, 2: from the first device
pass whatever the counts say).  The switch is read when a context is created, so every run here sets it before its Engine.

What is checked: the pairs after a run bit for bit against the exact search, the record of EVERY certified-only pass against the numpy
record (_record_ref, at test_gpu_pass_matrix.py's bars: TOL_EXACT unweighted, TOL_REC weighted), diffs and transform against the run
without the kernel or the host loop at test_device_loop_matches_host_loop's bars (diffs rtol 2e-6 / atol 1e-6, transform 1e-6 of its
scale), and the redo path: a certified-only pass that comes back incomplete is repeated by the host and the kernel is not chosen again
in that alignment.  Bit identity with the fused pass is not asked for: which thread accumulates a neighbourhood-settled pair already
depends on LDS atomic order there."""
import numpy as np
import pytest

import _record_ref as R

pytestmark = pytest.mark.gpu

LOOP_REDO_PASS = 2


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def cat15(cat):
    """the reference's cat cloud against itself moved by 15 degrees (synth.perturbed), same row order"""
    from symmicp import synth
    return synth.perturbed(cat["src"], cat["src_n"])


@pytest.fixture(scope="module")
def cat_near(cat):
    """... moved slightly: 2 degrees and a third of a point spacing"""
    from symmicp import synth
    return synth.perturbed(cat["src"], cat["src_n"], deg=2.0, t=(0.3, -0.5, 0.2))


@pytest.fixture(scope="module")
def c4s(sym):
    from symmicp import synth
    return synth.c4_surface(20000)


@pytest.fixture(scope="module")
def c5s(sym):
    from symmicp import synth
    return synth.c5_scan(64 * 1024)


def run(sym, monkeypatch, d, cert, n=None, loss=None, no_hood=False, comm=False, **kw):
    """one alignment with SYMMICP_CERT_PASS = cert (None: unset) -> everything the checks read.  comm: on a one-rank RCCL communicator
    (SYMMICP_FORCE_COMM=1, as test_rccl_path_single_rank_communicator): every device pass then goes k_final_reduce -> ncclAllReduce ->
    k_reduce_solve<false>, the path of a sharded run"""
    if cert is None:
        monkeypatch.delenv("SYMMICP_CERT_PASS", raising=False)
    else:
        monkeypatch.setenv("SYMMICP_CERT_PASS", str(cert))
    if no_hood:
        monkeypatch.setenv("SYMMICP_NO_NEIGHBOURHOOD", "1")
    else:
        monkeypatch.delenv("SYMMICP_NO_NEIGHBOURHOOD", raising=False)
    src, sn = d["src"][:n], d["src_n"][:n]
    kw.setdefault("mode", sym.MODE_PAPER)
    if comm:
        monkeypatch.setenv("SYMMICP_FORCE_COMM", "1")
    else:
        monkeypatch.delenv("SYMMICP_FORCE_COMM", raising=False)
    with sym.Engine(corr=sym.CORR_TREE, **kw) as e:
        if comm:
            e.comm_init_rank(1, 0, sym.comm_get_unique_id())
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(src, sn)
        if loss:
            e.set_robust_loss(*loss)
        e.set_loop_log(True)
        r = e.align()
        out = dict(res=r, log=e.loop_log(), stats=e.stats(), pairs=e.correspondences(), T=e.transform(), pivot=e.pivot())
    print("comm=%d cert=%s n=%d iters=%d status=%d loop_passes=%d kernels=%s reasons=%s" % (
        comm, cert, len(src), r["iters"], r["status"], out["stats"]["loop_passes"], "".join(str(x["kernel"]) for x in out["log"]),
        sorted({(x["batch"], x["reason"]) for x in out["log"]})))
    return out


def certified_passes(log):
    return [x for x in log if x["kernel"] == 1]


_TREES = {}


def nn_exact(p, q):
    """_record_ref.nn_ref, with its k-d tree route for the 20 000-point pair too (one exact search per certified-only pass: the brute
    force is 0.8 s each): the tree over the target is built once, it proposes 16 candidates in fp64, the fp32 dist2 of each is
    evaluated as the kernels do and the smallest (d2, row) wins; a row whose 16th candidate is not clearly farther than its winner
    goes to the brute force."""
    if len(q) <= 8192:
        return R.nn_ref(p, q)
    from scipy.spatial import cKDTree
    from oracle import oracle
    p, q = np.asarray(p, np.float32), np.asarray(q, np.float32)
    key = (q.ctypes.data, len(q))
    if key not in _TREES:
        _TREES[key] = (cKDTree(q.astype(np.float64)), q)          # (q kept: the key is its address)
    dist, cand = _TREES[key][0].query(p.astype(np.float64), k=16)
    d2c = np.stack([R.dist2(p, q[cand[:, c]]) for c in range(16)], 1)
    order = np.lexsort((cand, d2c), axis=1)[:, 0]                  # smallest d2, ties to the lowest row
    rows = np.arange(len(p))
    best, bd = cand[rows, order].astype(np.int64), d2c[rows, order].copy()
    unsure = dist[:, -1] <= np.sqrt(bd.astype(np.float64)) * (1 + 1e-4) + 1e-30
    if unsure.any():
        best[unsure], bd[unsure] = oracle.nn_brute(p[unsure], q)
    return best.astype(np.int32), bd.astype(np.float32)


def assert_final_pairs(out, d, n=None, mode=R.MODE_PAPER):
    """the pairs the run left: the exact nearest neighbours of the source as its last pass moved it, indices and d2 bit for bit"""
    p, _ = R.moved(out["T"], d["src"][:n], d["src_n"][:n], mode)
    ri, rd = nn_exact(p, d["tgt"])
    idx, d2 = out["pairs"]
    assert np.array_equal(idx, ri), int((idx != ri).sum())
    assert np.array_equal(d2, rd)


def assert_certified_records(out, d, n=None, mode=R.MODE_PAPER, loss=0, scale=1.0, max_d2=0.0, min_ndot=-2.0):
    """the record of every certified-only pass is the numpy record of the exact pairs under the transform that pass applied: the X of
    the log's entry before it (solved from the previous pass's record)"""
    by_iter = {x["iter"]: x for x in out["log"]}
    done = 0
    for x in certified_passes(out["log"]):
        prev = by_iter[x["iter"] - 1]
        assert prev["solved"] == 1
        p, pn = R.moved(prev["X"], d["src"][:n], d["src_n"][:n], mode)
        idx, _ = nn_exact(p, d["tgt"])
        S, M, kept = R.record(mode, p, pn, d["tgt"], d["tgt_n"], idx, out["pivot"], loss, scale, max_d2, min_ndot)
        R.assert_record(x["sums"], S, M, R.TOL_REC if loss else R.TOL_EXACT, "pass %d" % x["iter"])
        done += 1
    return done


def assert_same_alignment(a, b):
    """test_device_loop_matches_host_loop's bars"""
    ra, rb = a["res"], b["res"]
    assert ra["status"] == rb["status"] == 0, (ra["error"], rb["error"])
    assert ra["iters"] == rb["iters"], (ra["iters"], rb["iters"])
    k = ra["iters"]
    assert np.allclose(ra["diffs"][:k], rb["diffs"][:k], rtol=2e-6, atol=1e-6), (ra["diffs"][:k], rb["diffs"][:k])
    assert np.abs(ra["transform"] - rb["transform"]).max() < 1e-6 * max(1.0, float(np.abs(ra["transform"]).max()))
    assert abs(ra["diff_final"] - rb["diff_final"]) <= 2e-6 * max(1.0, abs(ra["diff_final"]))
    assert a["stats"]["passes"] == b["stats"]["passes"]


# ---- the kernel ran and is right ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("data", ["cat_near", "c4s"])
def test_rule_picks_the_kernel_and_it_is_right(sym, monkeypatch, request, data):
    d = request.getfixturevalue(data)
    kw = dict(max_iters=25, fixed_iters=1)
    on = run(sym, monkeypatch, d, None, **kw)
    off = run(sym, monkeypatch, d, 0, **kw)
    assert len(certified_passes(on["log"])) >= 1 and not certified_passes(off["log"])
    assert not any(x["redo_certified"] for x in on["log"] + off["log"])
    assert on["stats"]["loop_passes"] > 0 and off["stats"]["loop_passes"] > 0
    for o in (on, off):
        assert o["res"]["iters"] == 25
        assert_final_pairs(o, d)
    assert assert_certified_records(on, d) == len(certified_passes(on["log"]))
    assert_same_alignment(on, off)


# ---- ragged shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 203, 255, 256, 257, 2047, 2049, 3400])
def test_ragged_sizes(sym, monkeypatch, cat_near, n):
    """one partial tile, fewer tiles than blocks, tile counts that are no multiple of 8 (the padding of xcd_remap); the kernel forced
    on from the first device pass.  n = 1: a single pair leaves the normal equations rank-deficient, so no alignment of one point
    gets past its first solve and no device pass (of any kernel) runs -- the run must end as it does without the kernel.  n = 7 is the
    smallest share here that does run the kernel: seven lanes of one partial tile."""
    d = cat_near
    kw = dict(max_iters=16, fixed_iters=1)
    on = run(sym, monkeypatch, d, 2, n=n, **kw)
    if n == 1:
        off = run(sym, monkeypatch, d, 0, n=n, **kw)
        assert on["res"]["status"] == off["res"]["status"] != 0 and on["res"]["iters"] == off["res"]["iters"]
        assert on["stats"]["loop_passes"] == off["stats"]["loop_passes"] == 0
        return
    assert on["res"]["status"] == 0 and on["res"]["iters"] == 16
    assert len(certified_passes(on["log"])) >= 1, [(x["iter"], x["kernel"], x["reason"]) for x in on["log"]]
    assert_final_pairs(on, d, n)
    assert assert_certified_records(on, d, n) >= 1


@pytest.mark.parametrize("cert", [None, 2])
def test_sharded_path_one_rank_communicator(sym, monkeypatch, cat_near, cert):
    """the device loop of a sharded run on this one GPU: a one-rank RCCL communicator puts k_final_reduce (which packs the pairs
    searched and, above their 32 bits, the pairs scanned into slot 38), the all-reduce and k_reduce_solve<false> (which unpacks them:
    run_batch's rule reads the scan count from there) behind every device pass.  A share of 3399 rows (no multiple of 256 or of 4),
    by the rule and forced: certified-only passes in the log, their records the numpy records, pairs, diffs and transform those of
    the run without a communicator."""
    kw = dict(max_iters=25, fixed_iters=1)
    on = run(sym, monkeypatch, cat_near, cert, n=3399, comm=True, **kw)
    ref = run(sym, monkeypatch, cat_near, 0, n=3399, **kw)
    cp = certified_passes(on["log"])
    assert len(cp) >= 1 and on["stats"]["loop_passes"] > 0 and not any(x["redo_certified"] for x in on["log"])
    # the same passes run certified-only as without a communicator: the rule saw the same scan counts through the packed slot
    same = run(sym, monkeypatch, cat_near, cert, n=3399, **kw)
    assert [(x["iter"], x["kernel"]) for x in on["log"]] == [(x["iter"], x["kernel"]) for x in same["log"]]
    if cert is None:
        assert any(x["kernel"] == 0 for x in on["log"][1:]), "no fused head: the scan count of the early passes was lost"
    assert assert_certified_records(on, cat_near, 3399) == len(cp)
    assert_final_pairs(on, cat_near, 3399)
    assert np.array_equal(on["pairs"][0], ref["pairs"][0]) and np.array_equal(on["pairs"][1], ref["pairs"][1])
    assert_same_alignment(on, ref)


@pytest.mark.parametrize("no_hood", [False, True])
def test_sharded_path_incomplete_pass_comes_back(sym, monkeypatch, c5s, no_hood):
    """... and the incomplete pass through the summed count words: the forced kernel on the scan pair, one-rank communicator.  The
    count word the kernel bumps travels in slot 39 through the all-reduce; k_reduce_solve<false> must stop with LOOP_REDO_PASS."""
    kw = dict(max_iters=40, fixed_iters=1)
    dev = run(sym, monkeypatch, c5s, 2, no_hood=no_hood, comm=True, **kw)
    host = run(sym, monkeypatch, c5s, 2, no_hood=no_hood, host_loop=1, **kw)
    log = dev["log"]
    redo = [x for x in log if x["redo_certified"]]
    shown = [(x["batch"], x["iter"], x["kernel"], x["reason"]) for x in log]
    assert len(redo) == 1 and redo[0]["reason"] == LOOP_REDO_PASS, shown
    assert not [x for x in log if x["batch"] > redo[0]["batch"] and x["kernel"] == 1], shown
    assert dev["stats"]["loop_passes"] > 0
    assert np.array_equal(dev["pairs"][0], host["pairs"][0]) and np.array_equal(dev["pairs"][1], host["pairs"][1])
    assert_same_alignment(dev, host)


def test_sharded_external_exchange_with_the_switch(sym, monkeypatch, cat_near):
    """two contexts with external exchange, shares 1025 / 1025 (the second one starts at an unaligned row), the kernel forced on.
    External exchanges run on the host (batch_eligible keeps them out of the device loop), so no device pass -- certified-only or
    fused -- can run here: this only holds that the forced switch leaves such a run alone (the sharded device loop:
    test_sharded_path_one_rank_communicator).  Pairs tile the unsharded pairs, the
    rank records add up to the numpy record."""
    monkeypatch.setenv("SYMMICP_CERT_PASS", "2")
    d, n, steps = cat_near, 2050, 6
    src, sn = d["src"][:n], d["src_n"][:n]
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=steps + 1, fixed_iters=1)
    engs = [sym.Engine(**kw) for _ in range(2)]
    try:
        for r, e in enumerate(engs):
            e.comm_init_rank(2, r, None)
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(src, sn)
        assert [e.local_offset() for e in engs][1] % 4 != 0
        its = [e.begin() for e in engs]
        for k in range(steps + 1):
            total = np.sum([np.asarray(it["sums"], np.float64) for it in its], axis=0)
            p, pn = R.moved(engs[0].transform(), src, sn, R.MODE_PAPER)
            ri, rd = nn_exact(p, d["tgt"])
            idx = np.full(n, -1, np.int32)
            d2 = np.zeros(n, np.float32)
            for e in engs:
                i_r, d_r = e.correspondences()
                has = i_r >= 0
                assert np.array_equal(np.flatnonzero(has), np.arange(e.local_offset(), e.local_offset() + e.local_count()))
                idx[has], d2[has] = i_r[has], d_r[has]
            assert np.array_equal(idx, ri) and np.array_equal(d2, rd)
            S, M, _ = R.record(R.MODE_PAPER, p, pn, d["tgt"], d["tgt_n"], ri, engs[0].pivot())
            R.assert_record(total, S, M, R.TOL_EXACT * 10, "pass %d" % k)
            if k == steps:
                break
            for e in engs:
                e.set_sums(total)
            its = [e.step() for e in engs]
        assert all(e.stats()["loop_passes"] == 0 for e in engs)
    finally:
        for e in engs:
            e.close()


# ---- instantiations and gates ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,loss", [("paper", ("huber", 2.0)), ("plane", None), ("gicp", None)])
def test_instantiations_match_the_host_loop(sym, monkeypatch, cat15, mode, loss):
    """W (Huber-weighted PAPER), PLANE (reads no source normals) and GICP on the 15-degree cat start (scales: test_gpu_pass_matrix.py's
    HUBER), each against its host-loop run"""
    m = {"paper": sym.MODE_PAPER, "plane": sym.MODE_PLANE, "gicp": sym.MODE_GICP}[mode]
    kw = dict(mode=m, max_iters=40, fixed_iters=1)
    dev = run(sym, monkeypatch, cat15, None, loss=loss, **kw)
    host = run(sym, monkeypatch, cat15, None, loss=loss, host_loop=1, **kw)
    assert len(certified_passes(dev["log"])) >= 1 and host["stats"]["loop_passes"] == 0
    code = sym.loss_code(loss[0]) if loss else 0
    assert assert_certified_records(dev, cat15, mode=m, loss=code, scale=loss[1] if loss else 1.0) >= 1
    assert_final_pairs(dev, cat15, mode=m)
    assert_same_alignment(dev, host)


def test_gates_drop_pairs(sym, monkeypatch, c4s):
    """max_corr_dist at the 0.9 quantile of the pair distances at the true transform and every seventh source normal reversed
    (min_normal_dot = 0): both gates drop pairs in every certified-only pass"""
    d = dict(c4s, src_n=c4s["src_n"].copy())
    d["src_n"][::7] *= -1
    p, _ = R.moved(d["truth"], d["src"], d["src_n"], R.MODE_PAPER)
    mcd = float(np.sqrt(np.quantile(nn_exact(p, d["tgt"])[1], 0.9)))
    kw = dict(max_iters=25, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=0.0)
    dev = run(sym, monkeypatch, d, None, **kw)
    host = run(sym, monkeypatch, d, None, host_loop=1, **kw)
    cp = certified_passes(dev["log"])
    assert len(cp) >= 1
    assert all(0 < x["sums"][34] < 0.8 * len(d["src"]) for x in cp)
    assert assert_certified_records(dev, d, max_d2=R.f32_max_d2(mcd), min_ndot=0.0) == len(cp)
    assert_final_pairs(dev, d)
    assert_same_alignment(dev, host)


# ---- incomplete pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_hood", [False, True])
@pytest.mark.parametrize("data", ["cat15", "c5s"])
def test_incomplete_pass_is_redone_once(sym, monkeypatch, request, data, no_hood):
    """the kernel forced on while pairs are still settling: a certified-only pass comes back incomplete (LOOP_REDO_PASS), the host
    repeats it through the search kernels and the kernel is not chosen again in that alignment.  With SYMMICP_NO_NEIGHBOURHOOD=1
    every failed single certificate is incomplete.
    The scan pair is still settling when its device loop starts and must show the redo.  The 15-degree cat start is not: a device
    loop is only entered after a pass that searched at most N / 256 pairs (batch_eligible: 13 of 3400), the pair is a cloud against
    its own moved copy, and measured on the MI355X every forced certified-only pass of it completes (device passes 5 .. 40, with and
    without neighbourhoods).  So for that pair a redo is accepted, not demanded: with one, everything below holds as for the scan
    pair; without one, every device pass ran certified-only and is checked against the numpy record."""
    d = request.getfixturevalue(data)
    kw = dict(max_iters=40, fixed_iters=1)
    dev = run(sym, monkeypatch, d, 2, no_hood=no_hood, **kw)
    host = run(sym, monkeypatch, d, 2, no_hood=no_hood, host_loop=1, **kw)
    log = dev["log"]
    redo = [x for x in log if x["redo_certified"]]
    shown = [(x["batch"], x["iter"], x["kernel"], x["reason"]) for x in log]
    if data == "c5s" or redo:
        assert len(redo) == 1 and redo[0]["reason"] == LOOP_REDO_PASS, shown
        assert not [x for x in log if x["batch"] > redo[0]["batch"] and x["kernel"] == 1], shown
    else:
        assert all(x["kernel"] == 1 for x in log if x["iter"] > log[0]["iter"]) and len(certified_passes(log)) >= 1, shown
    assert dev["stats"]["loop_passes"] > 0
    assert np.array_equal(dev["pairs"][0], host["pairs"][0]) and np.array_equal(dev["pairs"][1], host["pairs"][1])
    if data == "cat15":          # (the 64k scan pair: one exact search per pass is too slow for the suite; its pairs are the host loop's)
        assert assert_certified_records(dev, d) == len(certified_passes(log))
        assert_final_pairs(dev, d)
    assert_same_alignment(dev, host)


# ---- stop flag -------------------------------------------------------------------------------------------------------------------
def test_threshold_stop_inside_the_device_passes(sym, monkeypatch, cat15):
    """an alignment stopped by the reference's rule (diff <= diff_threshold, fixed_iters off) ends at the same iteration whichever
    kernel runs the passes -- never, by the rule, forced -- and the stop lies inside the device passes: the flag is raised in the
    middle of a chunk of queued passes, and the certified-only launches behind it must return at once.
    The 15-degree cat start has converged to the last bits when its device loop starts, but its diff still steps down there
    (measured: 18712, 6740, 1976, 122.9, 9.01e-3, then 1.144e-2 / 8.76e-3, 1.138e-2 / 8.71e-3 in turn, device passes from 5 on): the
    threshold is put halfway between the last clear new minimum of a fixed-count run (0.1 % below everything before it) and the
    smallest diff before it -- three orders of magnitude more room than the 2e-6 the runs' diffs may differ by.  (Measured: the stop
    comes at iteration 6, the second device pass, two queued passes behind it; by the rule and forced, pass 5 ran certified-only.)"""
    d = cat15
    fixed = run(sym, monkeypatch, d, 0, max_iters=40, fixed_iters=1)
    df = fixed["res"]["diffs"].astype(np.float64)
    first_dev = fixed["log"][0]["iter"] + 1
    # (not the last pass of a chunk -- a run that can stop queues 4, 8, 16 passes -- so that launches are queued behind the stop)
    ks = [k for k in range(first_dev + 1, 40) if df[k] < 0.999 * df[:k].min() and k - first_dev + 1 not in (4, 12, 28)]
    assert ks, (first_dev, df)
    k = ks[-1]
    thr = float(0.5 * (df[k] + df[:k].min()))
    kw = dict(max_iters=40, diff_threshold=thr)
    runs = [run(sym, monkeypatch, d, cert, **kw) for cert in (0, None, 2)]
    for o in runs:
        assert o["res"]["iters"] == k < 40 and o["stats"]["loop_passes"] > 0, (o["res"]["iters"], k, thr, df)
    assert not certified_passes(runs[0]["log"])
    for o in runs[1:]:
        assert len(certified_passes(o["log"])) >= 1, [(x["iter"], x["kernel"]) for x in o["log"]]
        assert_same_alignment(o, runs[0])
        assert_final_pairs(o, d)


def test_threshold_recipe_at_20000_points(sym, monkeypatch, c4s):
    """test_device_loop_matches_host_loop's paper_tree_threshold recipe (diff_threshold = 2.5e-4 per point, max_iters 25) at 20 000
    points: the same iteration whichever kernel runs the passes.  Measured: at this size the pair's diff is 386.2, 97.67, 94.8199 and
    then 94.81994 for good (the sparser sampling leaves 4.7e-3 per point), so the recipe's threshold is never reached and every run
    ends at max_iters; the stop inside the device passes is test_threshold_stop_inside_the_device_passes."""
    d = c4s
    kw = dict(max_iters=25, diff_threshold=float(len(d["src"])) * 2.5e-4)
    runs = [run(sym, monkeypatch, d, cert, **kw) for cert in (0, None, 2)]
    assert runs[0]["res"]["iters"] == 25 and runs[0]["stats"]["loop_passes"] > 0
    assert not certified_passes(runs[0]["log"]) and certified_passes(runs[1]["log"]) and certified_passes(runs[2]["log"])
    for o in runs[1:]:
        assert_same_alignment(o, runs[0])
        assert_final_pairs(o, d)
