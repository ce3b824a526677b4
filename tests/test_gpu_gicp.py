"""GPU tests of the plane-to-plane mode (SYMMICP_MODE_GICP, run with -m gpu on a real MI355X): the epsilon setter, every pass kind's
pairs against the oracle's brute-force nearest neighbours and its record against the numpy GICP record of _gicp_ref.py, the record's
dependence on epsilon and the normals, the device-driven loop against the host loop and the device's solve against the host's,
power-of-two units, convergence, sharding by external exchange, the Python class and the command-line driver.

Records are compared slot by slot at a fraction of the sum of the slot's term magnitudes: 1e-9 unweighted (the numpy terms repeat
the kernels' fp32 rows exactly; only the fp64 summation order differs) and 1e-6 with a robust loss (test_gpu_robust.py's bar)."""
import os

import numpy as np
import pytest

from _frames import scale_record
import _record_ref as R
from _gicp_ref import FP64_C, direct_record, fp64_excess, gicp_pass_record, gicp_record, gicp_terms
from _plane_ref import plane_record, rot_err

pytestmark = pytest.mark.gpu

EPS_MIN = float(np.nextafter(np.float32(2.0 ** -25), np.float32(1)))     # the smallest eps accepted: fl32(1 - eps) = 1 - 2^-24
SCALES = {"none": 1.0, "huber": 3.0, "tukey": 60.0, "cauchy": 6.0, "geman_mcclure": 12.0}   # (cat15: r = sqrt(d^T M d) spans ~0 .. 100)


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def cat15(cat):
    from symmicp import synth
    return synth.perturbed(cat["src"], cat["src_n"])


@pytest.fixture(scope="module")
def c4(sym):
    from symmicp import synth
    return synth.c4_surface(200000)


def _corr(sym, name):
    return {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[name]


def assert_record(gpu, ref, mag, weighted, tag=""):
    gpu = np.asarray(gpu, np.float64)
    tol = 1e-6 if weighted else 1e-9
    err = np.abs(gpu[:37] - ref[:37])
    bad = np.nonzero(err > tol * np.maximum(mag[:37], 1e-300))[0]
    assert bad.size == 0, (tag, [(int(k), gpu[k], ref[k], mag[k]) for k in bad[:6]])
    assert gpu[37] == ref[37], (tag, gpu[37], ref[37])           # the pair count, exactly


def _positions(sym, oracle, e, src, src_n):
    """where the pass put the source: cumulative apply moves the original points, incremental ones are read back"""
    if e.cfg.apply == sym.APPLY_INCREMENTAL:
        return e.source()
    X = e.transform()
    return oracle.apply(X, src, True), oracle.apply(X, src_n, False)


def _check_pass(sym, oracle, e, it, d, corr, loss, scale, eps=1e-3, min_ndot=None, max_dist=None, tag=""):
    p, pn = _positions(sym, oracle, e, d["src"], d["src_n"])
    idx, d2 = e.correspondences()
    if corr == "identity":
        idx = None
    else:
        ri, rd = oracle.nn_brute(p, d["tgt"])
        assert np.array_equal(idx, ri), (tag, int((idx != ri).sum()))
        assert np.array_equal(d2, rd), (tag, int((d2 != rd).sum()))
    from _record_ref import f32_max_d2
    md2 = f32_max_d2(max_dist) if max_dist else 0.0
    mn = -2.0 if min_ndot is None else min_ndot
    S, M, kept = gicp_pass_record(p, pn, d["tgt"], d["tgt_n"], idx, e.pivot(), eps, sym.loss_code(loss), scale, md2, mn)
    if (min_ndot is not None or max_dist is not None) and tag == "begin":
        assert 0 < kept < len(p), kept                           # the gate bites
    assert_record(it["sums"], S, M, loss != "none", tag)


# ---- 1. the epsilon setter -----------------------------------------------------------------------------------------------------
def test_epsilon_setter(sym):
    for mode in (sym.MODE_GICP, sym.MODE_PAPER, sym.MODE_QUIRKS):        # accepted in every mode, read by GICP only
        with sym.Engine(mode=mode) as e:
            assert e.gicp_epsilon() == np.float32(1e-3)
            # (2^-25 and 1e-8: 1.0f - eps == 1.0f, a pair of equal normals would be singular)
            for bad in (0.0, -1e-3, 1.5, float("nan"), float("inf"), -float("inf"), 1e-8, 2.0 ** -25):
                with pytest.raises(sym.SymmIcpError) as x:
                    e.set_gicp_epsilon(bad)
                assert x.value.status == sym.ERR_ARG, bad
                assert e.gicp_epsilon() == np.float32(1e-3)
            for good in (1.0, 1e-6, 0.25, EPS_MIN):
                e.set_gicp_epsilon(good)
                assert e.gicp_epsilon() == np.float32(good)
            with pytest.raises(sym.SymmIcpError):
                e.set_gicp_epsilon(2.0 ** -25)
            assert e.gicp_epsilon() == np.float32(EPS_MIN)              # a refused eps leaves the one set before
        import ctypes as C
        with sym.Engine(mode=mode) as e:                                  # the C ABI itself
            L = sym.lib()
            for bad in (1e-8, 2.0 ** -25):
                assert L.symmicp_set_gicp_epsilon(e._h, C.c_float(bad)) == sym.ERR_ARG
            assert L.symmicp_set_gicp_epsilon(e._h, C.c_float(EPS_MIN)) == 0


def test_gicp_needs_source_normals(sym, cat15):
    d = cat15
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        with pytest.raises(sym.SymmIcpError) as x:
            e.set_source(d["src"], None)
        assert x.value.status == sym.ERR_ARG
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE) as e:      # a PLANE source without normals cannot switch to GICP
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], None)
        with pytest.raises(sym.SymmIcpError) as x:
            e.set_config(mode=sym.MODE_GICP)
        assert x.value.status == sym.ERR_STATE


# ---- 2. every pass kind, every loss --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", list(SCALES))
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_gicp_passes_match_numpy_record(sym, oracle, cat15, corr, loss):
    d = cat15
    with sym.Engine(mode=sym.MODE_GICP, corr=_corr(sym, corr), max_iters=30, host_loop=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        if loss != "none":
            e.set_robust_loss(loss, SCALES[loss])
        it = e.begin()
        _check_pass(sym, oracle, e, it, d, corr, loss, SCALES[loss], tag="begin")
        for k in range(3):
            it = e.step()
            _check_pass(sym, oracle, e, it, d, corr, loss, SCALES[loss], tag="step %d" % (k + 1))


@pytest.mark.parametrize("variant", ["normal_gate", "distance_gate", "incremental", "epsilon"])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_gicp_gates_apply_and_epsilon(sym, oracle, cat15, corr, variant):
    """min_normal_dot, max_corr_dist, write-back (APPLY_INCREMENTAL), and an epsilon set between passes (it takes effect at the next)"""
    d = cat15
    kw = {"normal_gate": dict(min_normal_dot=0.97), "distance_gate": dict(max_corr_dist=8.0),
          "incremental": dict(apply=sym.APPLY_INCREMENTAL), "epsilon": {}}[variant]
    with sym.Engine(mode=sym.MODE_GICP, corr=_corr(sym, corr), max_iters=30, host_loop=1, **kw) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        gates = dict(min_ndot=kw.get("min_normal_dot"), max_dist=kw.get("max_corr_dist"))
        it = e.begin()
        _check_pass(sym, oracle, e, it, d, corr, "none", 1.0, tag="begin", **gates)
        eps = 1e-3
        for k in range(3):
            if variant == "epsilon":
                eps = (0.05, 1.0, 1e-5)[k]
                e.set_gicp_epsilon(eps)
            it = e.step()
            _check_pass(sym, oracle, e, it, d, corr, "none", 1.0, eps, tag="step %d" % (k + 1), **gates)
        if variant == "incremental":
            assert np.abs(e.source()[1] - oracle.apply(e.transform(), d["src_n"], False)).max() < 1e-5


@pytest.mark.parametrize("loss", ["none", "huber"])
def test_fused_pass_record(sym, oracle, c4, loss):
    """a converged GICP alignment runs pass after pass on the device (k_pass_fused<true, W, GICP>, k_reduce_solve's solve_plane).
    The record it leaves is the numpy record of its pairs: the next host step solves from it."""
    d = c4
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        scale = 1e-5                                                   # (below every residual: Huber weights 1 / |u|)
        if loss != "none":
            e.set_robust_loss(loss, scale)
        res = e.align()
        assert res["status"] == 0, res["error"]
        assert e.stats()["loop_passes"] > 0
        X = e.transform()
        p, pn = oracle.apply(X, d["src"], True), oracle.apply(X, d["src_n"], False)
        idx, _ = e.correspondences()
        keep = idx >= 0
        args = (p[keep], pn[keep], d["tgt"][idx[keep]], d["tgt_n"][idx[keep]], e.pivot())
        S, M = gicp_record(*args, 1e-3, sym.loss_code(loss), scale)
        if loss == "none":          # the fused loop's final pairs against the fp64 definition
            assert fp64_excess(S, M, direct_record(*args, 1e-3), 1e-3) <= FP64_C
        if loss != "none":
            w = gicp_terms(*args, 1e-3, 1, scale)[0][:, 34]
            assert w.sum() < 0.9 * len(w)                              # the weights bite
        st, _, _, _, _, _, Xs = sym.solve(sym.MODE_GICP, S, e.pivot())
        assert st == 0
        it = e.step()
        assert np.abs(it["increment"] - Xs).max() < 1e-6, (it["increment"], Xs)


def edge_pairs():
    """hand-placed pairs at the closed form's edges, 4 apart (every pairing pairs row i with row i), offsets of ~0.05:
    a = b (cs clamps to 1: lambda_u = 2 eps), a = -b (u = 0, lambda_v = 2 eps), orthogonal normals, zero normals on either side and
    on both (M = 1/2 I), slightly non-unit fp32 normals.  41 rows: the identity pass runs k_pass_identity<1>"""
    s = np.float32(1.0000001)
    A = [(0, 0, 1), (0.6, 0.8, 0), (0, 0, 1), (0.6, 0.8, 0), (1, 0, 0), (0, 0.6, 0.8), (0, 0, 0), (0, 1, 0), (0, 0, 0),
         (0.6000001, 0.8, 0), (0, 0, s), (0.48, 0.6, 0.64)]
    B = [(0, 0, 1), (0.6, 0.8, 0), (0, 0, -1), (-0.6, -0.8, 0), (0, 1, 0), (1, 0, 0), (0, 0, 1), (0, 0, 0), (0, 0, 0),
         (0.6, 0.8000001, 0), (0, 0, s), (0.48, 0.6, 0.64)]
    rng = np.random.default_rng(7)
    n = 41
    k = np.arange(n) % len(A)
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(3), indexing="ij"), -1).reshape(-1, 3)[:n]
    tgt = (4.0 * g + 1.0).astype(np.float32)
    src = (tgt + rng.uniform(-0.05, 0.05, size=(n, 3))).astype(np.float32)
    sn = np.float32(A)[k]
    tn = np.float32(B)[k]
    return dict(src=src, src_n=sn, tgt=tgt, tgt_n=tn), k == 8


@pytest.mark.parametrize("eps", [1.0, 1e-3, 1e-5, EPS_MIN])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_edge_pairs_match_numpy_record(sym, corr, eps):
    """the record of the edge pairs, every pairing, down to the smallest accepted eps: finite, the numpy record's (TOL_EXACT), and
    the pairs with zero normals on both sides give the fp64 point-to-point record at weight 1/2 (M = 1/2 I)"""
    d, zero = edge_pairs()
    with sym.Engine(mode=sym.MODE_GICP, corr=_corr(sym, corr), max_iters=3, fixed_iters=1) as e:
        e.set_gicp_epsilon(eps)
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        it = e.begin()
        idx, _ = e.correspondences()
        assert np.array_equal(idx, np.arange(len(d["src"])))
        S, M, kept = gicp_pass_record(d["src"], d["src_n"], d["tgt"], d["tgt_n"], None, e.pivot(), eps)
        assert np.isfinite(it["sums"]).all() and np.isfinite(S).all()
        assert kept == len(d["src"])
        R.assert_record(it["sums"], S, M, R.TOL_EXACT, "eps %g" % eps)
    z = {k: v[zero] for k, v in d.items()}
    with sym.Engine(mode=sym.MODE_GICP, corr=_corr(sym, corr), max_iters=3, fixed_iters=1) as e:
        e.set_gicp_epsilon(eps)
        e.set_target(z["tgt"], z["tgt_n"])
        e.set_source(z["src"], z["src_n"])
        gpu = np.asarray(e.begin()["sums"])
        pv = e.pivot()
        _, M, _ = gicp_pass_record(z["src"], z["src_n"], z["tgt"], z["tgt_n"], None, pv, eps)
    # (the points about the pivot as the kernel forms them, in fp32; their differences are then exact)
    P, Q = z["src"] - pv, z["tgt"] - pv
    assert np.array_equal((P - Q).astype(np.float64), P.astype(np.float64) - Q.astype(np.float64))
    D = direct_record(P, z["src_n"], Q, z["tgt_n"], np.zeros(3), eps)
    sl = list(range(27)) + [35]
    assert (np.abs(gpu[sl] - D[sl]) <= 1e-12 * np.maximum(M[sl], 1e-300)).all(), (gpu[sl], D[sl])


def test_smallest_epsilon_cat_against_itself(sym, cat):
    """eps = the float above 2^-25: the cat cloud against itself (every pair a = b, cs = 1, lambda_u = 2^-23) gives a finite
    record, the numpy record's"""
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_IDENTITY, max_iters=3, fixed_iters=1) as e:
        e.set_gicp_epsilon(EPS_MIN)
        assert e.gicp_epsilon() == np.float32(EPS_MIN)
        e.set_target(cat["src"], cat["src_n"])
        e.set_source(cat["src"], cat["src_n"])
        it = e.begin()
        S, M, kept = gicp_pass_record(cat["src"], cat["src_n"], cat["src"], cat["src_n"], None, e.pivot(), EPS_MIN)
    assert np.isfinite(it["sums"]).all() and np.isfinite(S).all()
    R.assert_record(it["sums"], S, M, R.TOL_EXACT, "eps min")


# ---- fp64: the record against the definition, not a restatement -------------------------------------------------------------------
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_first_pass_meets_the_fp64_bar(sym, cat15, corr):
    """the first pass of every pairing against gicp_direct (np.linalg.inv(C_p + C_q) in fp64) at _gicp_ref's bar, FP64_C x
    2^-24 / eps of each slot's magnitude: a mistake the kernel and gicp_terms shared (a wrong lambda, gamma_u and gamma_v swapped, a
    lost 1/2 on the axis rows) fails here though it passes every restated-record test"""
    d = cat15
    with sym.Engine(mode=sym.MODE_GICP, corr=_corr(sym, corr), max_iters=3, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        gpu = np.asarray(e.begin()["sums"])
        idx, _ = e.correspondences()
        pv = e.pivot()
    _, M, _ = gicp_pass_record(d["src"], d["src_n"], d["tgt"], d["tgt_n"], idx, pv)
    D = direct_record(d["src"], d["src_n"], d["tgt"][idx], d["tgt_n"][idx], pv, 1e-3)
    assert fp64_excess(gpu, M, D, 1e-3) <= FP64_C, fp64_excess(gpu, M, D, 1e-3)


# ---- 3. epsilon and the normals ---------------------------------------------------------------------------------------------------
def _records(sym, d, src_n, tgt_n, n=3, mode=None, eps=None, **kw):
    with sym.Engine(mode=sym.MODE_GICP if mode is None else mode, max_iters=30, host_loop=1, **kw) as e:
        if eps is not None:
            e.set_gicp_epsilon(eps)
        e.set_target(d["tgt"], tgt_n)
        e.set_source(d["src"], src_n)
        recs = [e.begin()["sums"]]
        for _ in range(n):
            recs.append(e.step()["sums"])
        return np.array(recs), e.transform().copy()


@pytest.mark.parametrize("corr", ["identity", "tree"])
def test_epsilon_one_ignores_the_normals(sym, cat15, corr):
    """eps = 1: every covariance is I, the record of random normals and of zero normals is the same, to the bit"""
    d = cat15
    rng = np.random.default_rng(3)
    rn = rng.normal(size=d["src_n"].shape).astype(np.float32)
    z = np.zeros_like(d["src_n"])
    r0, X0 = _records(sym, d, d["src_n"], d["tgt_n"], eps=1.0, corr=_corr(sym, corr))
    r1, X1 = _records(sym, d, rn, rn[::-1].copy(), eps=1.0, corr=_corr(sym, corr))
    r2, X2 = _records(sym, d, z, z, eps=1.0, corr=_corr(sym, corr))
    assert np.array_equal(r0, r1) and np.array_equal(r0, r2)
    assert np.array_equal(X0, X1) and np.array_equal(X0, X2)


@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_record_is_not_plane_record(sym, oracle, cat15, corr):
    """eps = 1e-3: the GICP record of a pass differs from PLANE's of the same pass (no PLANE instantiation reused), and each matches
    its own numpy record"""
    d = cat15
    out = {}
    for mode in (sym.MODE_GICP, sym.MODE_PLANE):
        with sym.Engine(mode=mode, corr=_corr(sym, corr), max_iters=30, host_loop=1) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            out[mode] = (np.asarray(e.begin()["sums"]), e.correspondences()[0], e.pivot())
    (g, ig, pv), (pl, ip, _) = out[sym.MODE_GICP], out[sym.MODE_PLANE]
    assert np.array_equal(ig, ip)
    assert np.abs(g[:27] - pl[:27]).max() > 1e-3 * np.abs(pl[:27]).max()
    idx = np.arange(len(d["src"])) if corr == "identity" else ig
    Sp, Mp = plane_record(d["src"], d["tgt"][idx], d["tgt_n"][idx], pv)
    assert_record(pl, Sp, Mp, False, "plane")
    Sg, Mg = gicp_record(d["src"], d["src_n"], d["tgt"][idx], d["tgt_n"][idx], pv)
    assert_record(g, Sg, Mg, False, "gicp")


# ---- 4. device loop = host loop; the device's solve = the host's --------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tree_c4", "identity_cat15"])
def test_device_loop_matches_host_loop(sym, c4, cat15, case):
    d, kw = (c4, dict(corr=sym.CORR_TREE, max_iters=25)) if case == "tree_c4" else (cat15, dict(corr=sym.CORR_IDENTITY, max_iters=8))
    res = {}
    for host_loop in (1, 0):
        with sym.Engine(mode=sym.MODE_GICP, fixed_iters=1, host_loop=host_loop, **kw) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            res[host_loop] = (e.align(), e.stats())
    (rh, sh), (rd, sd) = res[1], res[0]
    assert rh["status"] == rd["status"] == 0
    assert rh["iters"] == rd["iters"] == kw["max_iters"]
    n = rh["iters"]
    assert np.allclose(rh["diffs"][:n], rd["diffs"][:n], rtol=2e-6, atol=1e-6), (rh["diffs"][:n], rd["diffs"][:n])
    assert np.abs(rh["transform"] - rd["transform"]).max() < 1e-6 * max(1.0, float(np.abs(rh["transform"]).max()))
    assert sh["loop_passes"] == 0 and sd["loop_passes"] > 0
    assert sd["passes"] == sh["passes"]


def test_solve_probe_matches_host_solve(sym, cat15):
    """the device's solve of real GICP records (symmicp_ctx_solve_probe, exact conditioning): status, pbar, qbar, a, t and rcond
    are the host's bits, and the increment is the device's PLANE solve of the same record, to the bit"""
    d = cat15
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=30, host_loop=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        recs = [np.asarray(e.begin()["sums"])]
        for _ in range(5):
            recs.append(np.asarray(e.step()["sums"]))
        pv = e.pivot()
        S = np.stack(recs)
        g = e.solve_probe(sym.MODE_GICP, S, True, pivot=pv)
        pl = e.solve_probe(sym.MODE_PLANE, S, True, pivot=pv)
    for i, s in enumerate(S):
        st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_GICP, s, pv)
        assert g["status"][i] == st == 0, (i, g["status"][i], st)
        for k, v in (("pbar", pb), ("qbar", qb), ("a", a), ("t", t)):
            assert np.array_equal(g[k][i].view(np.uint32), np.asarray(v, np.float32).view(np.uint32)), (i, k)
        assert g["rcond"][i].view(np.uint32) == np.float32(rc).view(np.uint32), i
        assert np.abs(g["out16"][i] - X).max() < 1e-5 * max(1.0, float(np.abs(X).max()))
    for k in ("status", "pbar", "qbar", "a", "t", "rcond", "out16"):
        assert np.array_equal(g[k], pl[k]), k


# ---- 5. power-of-two units ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-8, 8])
def test_power_of_two_units_run_the_same_passes(sym, cat15, k):
    s = np.float32(2.0 ** k)
    d = cat15
    ds = dict(src=d["src"] * s, src_n=d["src_n"], tgt=d["tgt"] * s, tgt_n=d["tgt_n"])
    out = []
    for dd in (d, ds):
        with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=30, host_loop=1) as e:
            e.set_target(dd["tgt"], dd["tgt_n"])
            e.set_source(dd["src"], dd["src_n"])
            passes = [e.begin()]
            pairs = [e.correspondences()]
            for _ in range(5):
                passes.append(e.step())
                pairs.append(e.correspondences())
            out.append((passes, pairs, e.transform().copy()))
    (p0, c0, X0), (p1, c1, X1) = out
    for a, b, (i0, d0), (i1, d1) in zip(p0, p1, c0, c1):
        assert np.array_equal(i0, i1) and np.array_equal(d1, d0 * s * s)
        assert np.array_equal(np.asarray(b["sums"]), scale_record(a["sums"], float(s)))
        assert np.array_equal(b["increment"][:3, :3], a["increment"][:3, :3])
        assert np.array_equal(b["increment"][:3, 3], a["increment"][:3, 3] * s)
    assert np.array_equal(X1[:3, :3], X0[:3, :3]) and np.array_equal(X1[:3, 3], X0[:3, 3] * s)
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=30) as e:      # and the device loop
        e.set_target(ds["tgt"], ds["tgt_n"])
        e.set_source(ds["src"], ds["src_n"])
        r = e.align()
        assert r["status"] == 0, r["error"]


# ---- 6. convergence -------------------------------------------------------------------------------------------------------------
def test_converges_on_the_cat_pair_from_identity(sym, cat):
    """cat_out = Rz(45 deg) cat + (2.5, 0, 0): from the identity, with PLANE's test's stop settings (60 iterations), within 1e-4 of
    the truth.  The iterations PAPER, PLANE and GICP need under the reference's stop rule (diff <= 1) are printed."""
    src, tgt = cat["src"], cat["tgt"]
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    T = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=60, fixed_iters=1) as e:
        e.set_target(tgt, cat["tgt_n"])
        e.set_source(src, cat["src_n"])
        r = e.align()
    assert r["status"] == 0, r["error"]
    assert np.abs(r["transform"] - T).max() < 1e-4, r["transform"]
    iters = {}
    for name, mode in (("paper", sym.MODE_PAPER), ("plane", sym.MODE_PLANE), ("gicp", sym.MODE_GICP)):
        with sym.Engine(mode=mode, corr=sym.CORR_TREE, max_iters=60) as e:
            e.set_target(tgt, cat["tgt_n"])
            e.set_source(src, cat["src_n"])
            r = e.align()
        assert r["status"] == 0, (name, r["error"])
        iters[name] = (r["iters"], float(np.abs(r["transform"] - T).max()))
    print("cat pair from the identity: iterations, max |T - truth|:", iters)


def test_converges_on_the_c4_pair(sym, c4):
    """the synthetic surface pair from the identity: within 1e-4 of the generating motion (3 degrees + a translation)"""
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=40, fixed_iters=1) as e:
        e.set_target(c4["tgt"], c4["tgt_n"])
        e.set_source(c4["src"], c4["src_n"])
        r = e.align()
    assert r["status"] == 0, r["error"]
    ang, dt = rot_err(r["transform"], c4["truth"])
    assert ang < 1e-4 and dt < 1e-4, (ang, dt)


# ---- 7. sharding by external exchange -----------------------------------------------------------------------------------------------
def test_external_exchange_two_shards(sym, c4):
    d = c4
    kw = dict(mode=sym.MODE_GICP, corr=sym.CORR_TREE, max_iters=30)
    with sym.Engine(**kw) as ref:
        ref.set_gicp_epsilon(0.01)
        ref.set_target(d["tgt"], d["tgt_n"])
        ref.set_source(d["src"], d["src_n"])
        rec_ref = np.asarray(ref.begin()["sums"], np.float64)
        T_ref = []
        for _ in range(4):
            ref.step()
            T_ref.append(ref.transform())
    engs = [sym.Engine(**kw) for _ in range(2)]
    try:
        for r, e in enumerate(engs):
            e.comm_init_rank(2, r, None)
            e.set_gicp_epsilon(0.01)
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
        assert all(0 < e.local_count() < len(d["src"]) for e in engs)
        total = np.sum([np.asarray(e.begin()["sums"], np.float64) for e in engs], axis=0)
        # the shards' records add up to the single context's (fp64 summation order apart)
        assert np.abs(total[:37] - rec_ref[:37]).max() <= 1e-11 * np.abs(rec_ref[:37]).max()
        for k in range(4):
            for e in engs:
                e.set_sums(total)
            total = np.sum([np.asarray(e.step()["sums"], np.float64) for e in engs], axis=0)
            assert np.array_equal(engs[0].transform(), engs[1].transform()), k
            assert np.abs(engs[0].transform() - T_ref[k]).max() < 1e-6, k
    finally:
        for e in engs:
            e.close()


# ---- 8. the Python class and the command-line driver ---------------------------------------------------------------------------
def test_myicp_and_driver_mode_gicp(sym, cat, tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT, GOLDEN
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    shutil.copy(os.path.join(GOLDEN, "cat.pcd"), tmp_path / "cat.pcd")
    shutil.copy(os.path.join(GOLDEN, "cat_out.pcd"), tmp_path / "cat_out.pcd")
    r = subprocess.run([exe, "--mode", "gicp", "--corr", "tree", "cat.pcd", "cat_out.pcd"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # the library's own GICP result: normals of both clouds from the same GPU k-NN PCA the class uses
    sn, _ = sym.estimate_normals(cat["src"], 10)
    tn, _ = sym.estimate_normals(cat["tgt"], 10)
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE) as e:
        e.set_target(cat["tgt"], tn)
        e.set_source(cat["src"], sn)
        rg = e.align()
    assert rg["status"] == 0
    assert sym.format_result(rg["transform"]) in r.stdout, r.stdout[-600:]
    # the Python class: both clouds' normals estimated
    m = sym.MyICP(mode=sym.MODE_GICP, corr=sym.CORR_TREE, verbose=False)
    m.setInputSource(cat["src"])
    m.setInputTarget(cat["tgt"])
    res = m.align()
    assert m.normals_src is not None and m.normals_tgt is not None and res["status"] == 0
    assert np.array_equal(res["transform"], rg["transform"])
    # and its epsilon: eps = 1 is point-to-point at weight 1/2, a different result
    m.setGicpEpsilon(1.0)
    r1 = m.align()
    assert r1["status"] == 0 and not np.array_equal(r1["transform"], rg["transform"])
    with sym.Engine(mode=sym.MODE_GICP, corr=sym.CORR_TREE) as e:
        e.set_gicp_epsilon(1.0)
        e.set_target(cat["tgt"], tn)
        e.set_source(cat["src"], sn)
        assert np.array_equal(e.align()["transform"], r1["transform"])
    r2 = subprocess.run([exe, "--mode", "gicp", "--gicp-epsilon", "1", "--corr", "tree", "cat.pcd", "cat_out.pcd"], cwd=tmp_path,
                        capture_output=True, text=True, timeout=300)
    assert r2.returncode == 0 and sym.format_result(r1["transform"]) in r2.stdout, r2.stderr
