"""The record of every pass kernel, after every pass (run with -m gpu on a real MI355X).

A pass is one of k_pass_identity (VEC 4 or 1), k_nn_brute + k_pass_indexed, the tree's k_search_cells / k_search_walk +
k_accumulate, and k_pass_fused (device-driven loop), each in its W (robust weight) x PL (PLANE) instantiations and each applying
the two pair gates.  Here their records are held, pass after pass, to the numpy record of _record_ref.py built from the engine's
own moved source, its pairs (checked bit for bit against the oracle's brute force first) and its pivot:
  1. the matrix: mode x pairing x gate x loss x apply mode over ragged sizes (n = 0, 1, 2, 3 mod 4);
  2. the gate boundaries: pairs exactly at max_d2 and min_ndot and one ulp either side, through every pass kernel;
  3. sharded runs of every pairing (external exchange, unaligned shares);
  4. the device-driven loop with gates against the host loop."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import _record_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def mode_code(sym, mode):
    return {"quirks": sym.MODE_QUIRKS, "paper": sym.MODE_PAPER, "p2p": sym.MODE_P2P, "plane": sym.MODE_PLANE, "gicp": sym.MODE_GICP}[mode]


def corr_code(sym, corr):
    return {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[corr]


def pass_record(e, d, mode, loss, scale, max_d2, min_ndot, incremental, identity):
    """check the pass the engine just ran: its pairs and distances bit for bit, then -> (numpy record, magnitudes, kept pairs)"""
    src, src_n, tgt, tgt_n = d["src"], d["src_n"], d["tgt"], d["tgt_n"]
    if incremental:
        p, pn = e.source()                     # the pass wrote the points it accumulated back
    else:
        p, pn = R.moved(e.transform(), src, src_n, mode)
    idx, d2 = e.correspondences()
    if identity:
        assert np.array_equal(idx, np.arange(len(src)))
        assert np.array_equal(d2, R.dist2(p, tgt))
    else:
        ri, rd = R.nn_ref(p, tgt)
        assert np.array_equal(idx, ri), int((idx != ri).sum())
        assert np.array_equal(d2, rd)
    return R.record(mode, p, pn, tgt, tgt_n, idx, e.pivot(), loss, scale, max_d2, min_ndot)


# ---- 1. the matrix ----------------------------------------------------------------------------------------------------
MODES = ["quirks", "paper", "p2p", "plane", "gicp"]          # (appended: earlier cases keep their ids and sizes)
CORRS = ["identity", "brute", "tree"]
GATES = ["none", "dist", "normal", "both"]
SIZES = [3400, 1201, 2002, 203]            # 0, 1, 2, 3 mod 4 (203 < one block of 256)
# cat: c of the 15-degree start spans ~0 .. 100 (GICP: r = sqrt(d^T M d), test_gpu_gicp.py's scale)
HUBER = {"quirks": 1.0, "paper": 2.0, "p2p": None, "plane": 1.0, "gicp": 3.0}
MATRIX = [(m, c, g, l, a) for m in MODES for c in CORRS for g in GATES for l in ("none", "huber") for a in ("incr", "cumul")
          if not (m == "quirks" and l == "huber")]
N_PASSES = 4


def matrix_data(cat, n, flip):
    """cat against itself moved by 15 degrees (same rows), the first n rows; flip: every third source normal reversed (pairs the
    normal gate drops)"""
    from symmicp import synth
    d = synth.perturbed(cat["src"][:n], cat["src_n"][:n])
    if flip:
        d["src_n"] = d["src_n"].copy()
        d["src_n"][::3] *= -1
    return d


@pytest.mark.parametrize("mode,corr,gate,loss,apply", MATRIX, ids=["-".join(c) for c in MATRIX])
def test_matrix(sym, cat, mode, corr, gate, loss, apply):
    k = MATRIX.index((mode, corr, gate, loss, apply))
    n = SIZES[k % len(SIZES)]
    d = matrix_data(cat, n, gate in ("normal", "both"))
    m = mode_code(sym, mode)
    code = sym.loss_code(loss)
    # the distance gate at the median first-pass distance: it drops about half the pairs of the first pass
    if corr == "identity":
        d2_0 = R.dist2(d["src"], d["tgt"])
    else:
        d2_0 = R.nn_ref(d["src"], d["tgt"])[1]
    scale = HUBER[mode] if mode != "p2p" else 0.5 * float(np.sqrt(np.median(d2_0)))     # (P2P: r = |p - q|)
    mcd = float(np.sqrt(np.median(d2_0))) if gate in ("dist", "both") else 0.0
    mnd = 0.0 if gate in ("normal", "both") else -2.0
    max_d2 = R.f32_max_d2(mcd)
    incr = apply == "incr"
    kw = dict(mode=m, corr=corr_code(sym, corr), apply=sym.APPLY_INCREMENTAL if incr else sym.APPLY_CUMULATIVE,
              max_iters=N_PASSES + 2, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=mnd)
    with sym.Engine(**kw) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        if code:
            e.set_robust_loss(loss, scale)
        it = e.begin()
        for k in range(N_PASSES):
            tag = "pass %d" % k
            S, M, kept = pass_record(e, d, m, code, scale, max_d2, mnd, incr, corr == "identity")
            R.assert_record(it["sums"], S, M, R.TOL_REC if code else R.TOL_EXACT, tag)
            assert it["pairs"] == kept, (tag, it["pairs"], kept)
            if k == 0:
                assert kept > 0
                if gate != "none":
                    assert kept < n, "the gate dropped nothing"
                else:
                    assert kept == n
                if code:
                    assert 0.0 < S[34] < kept           # the weights bite
            if kept == 0:
                break                                   # (QUIRKS under a distance gate can move every pair out of it)
            if k + 1 < N_PASSES:
                it = e.step()
                assert it["status"] == 0, (tag, it["status"])
        if corr == "tree":
            ce, _, _, _ = e.certificates()
            assert (ce[:, 3] > 0).any()                 # the passes after the first hold pair certificates (stats() counts no settled pairs)
        if corr == "identity":
            assert e.stats()["passes"] >= N_PASSES


def test_matrix_identity_grid_stride_in_a_subprocess(sym):
    """one block per identity pass (SYMMICP_ID_BLOCKS: the VEC 4 grid; SYMMICP_PASS_BLOCKS: the VEC 1 grid): every thread strides
    over many rows, the rows of the last stride ragged"""
    if os.environ.get("SYMMICP_ID_BLOCKS"):
        pytest.skip("already the child")
    env = dict(os.environ, SYMMICP_ID_BLOCKS="1", SYMMICP_PASS_BLOCKS="1")
    n_ident = sum(1 for c in MATRIX if c[1] == "identity")            # (every mode's, GICP's included)
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_matrix and identity and not subprocess and not kernels", "-W", "ignore"],
                       env=env, capture_output=True, text=True, timeout=900, cwd=os.path.dirname(HERE))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r"\b%d passed" % n_ident, r.stdout) and "failed" not in r.stdout, r.stdout[-500:]


def test_matrix_takes_both_identity_kernels():
    """the sizes reach k_pass_identity<1> (the run_pass vec4 test: n, n_t and the shard offset all multiples of 4) and <4>, in every
    mode on its own (each mode has its own instantiations), and the one-block grid"""
    for mode in [None] + MODES:
        ident = [SIZES[MATRIX.index(c) % len(SIZES)] for c in MATRIX if c[1] == "identity" and mode in (None, c[0])]
        assert {n % 4 for n in ident} == {0, 1, 2, 3}, mode
        assert min(ident) < 256, mode
    assert sum(1 for c in MATRIX if c[0] == "gicp") == 48


# ---- the fused pass ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c4(sym):
    from symmicp import synth
    d = synth.c4_surface(200000)
    return with_converged_gates(d)


def with_converged_gates(d, flip=7):
    """a distance gate that still bites once the alignment has converged -- the 0.9 quantile of the pair distances at the true
    transform -- and every `flip`-th source normal reversed, which the normal gate drops at any pose"""
    p, _ = R.moved(d["truth"], d["src"][::10], d["src_n"][::10], R.MODE_PAPER)
    d2 = R.nn_ref(p, d["tgt"])[1]
    d = dict(d, mcd=float(np.sqrt(np.quantile(d2, 0.9))), src_n=d["src_n"].copy(), flip=flip)
    d["src_n"][::flip] *= -1
    # and robust-loss scales that bite there: the 0.9 quantile of |c| of each mode's pairs at the true transform
    idx = R.nn_ref(p, d["tgt"])[0]
    pn = R.moved(d["truth"], d["src"][::10], d["src_n"][::10], R.MODE_PAPER)[1]
    d["c_scale"] = {m: float(np.quantile(np.abs(R.pass_terms(m, p, pn, d["tgt"][idx], d["tgt_n"][idx], np.zeros(3, np.float32))[1]), 0.9))
                    for m in (R.MODE_PAPER, R.MODE_PLANE, R.MODE_GICP)}
    return d


def final_record(e, d, m, loss, scale, mnd):
    """the pairs the engine holds after its last pass, checked bit for bit, and the numpy record of that pass with both gates ->
    (record, magnitudes, kept, pairs dropped by the distance gate alone, pairs dropped by the normal gate alone)"""
    p, pn = R.moved(e.transform(), d["src"], d["src_n"], m)
    idx, d2 = e.correspondences()
    ri, rd = R.nn_ref(p, d["tgt"])
    assert np.array_equal(idx, ri) and np.array_equal(d2, rd)
    max_d2 = R.f32_max_d2(d["mcd"])
    S, M, kept = R.record(m, p, pn, d["tgt"], d["tgt_n"], idx, e.pivot(), loss, scale, max_d2, mnd)
    q, qn = d["tgt"][idx], d["tgt_n"][idx]
    far = ~R.gate(p, pn, q, qn, max_d2)
    bent = ~R.gate(p, pn, q, qn, 0.0, mnd)
    return S, M, kept, int((far & ~bent).sum()), int((bent & ~far).sum())


def assert_gates_bite(n, kept, far_only, bent_only):
    assert far_only > 0 and bent_only > 0, (far_only, bent_only)      # each gate drops pairs the other keeps
    assert 0 < kept < n - far_only - bent_only + 1, (kept, n)


@pytest.mark.parametrize("mode,loss", [("paper", "none"), ("paper", "huber"), ("plane", "none"), ("plane", "huber"), ("gicp", "none"),
                                       ("gicp", "huber")])
def test_fused_pass_record_with_both_gates(sym, c4, mode, loss):
    """a converged alignment runs pass after pass on the device (k_pass_fused), both gates biting in those passes.  The record the
    device loop leaves must be the numpy record of the pairs it left: its diff (slot 33) is the last device pass's, and the next host
    step solves from the record"""
    d = c4
    m = mode_code(sym, mode)
    code = sym.loss_code(loss)
    mnd = 0.0
    with sym.Engine(mode=m, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1, max_corr_dist=d["mcd"], min_normal_dot=mnd) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        scale = d["c_scale"][m]
        if code:
            # (weights this small from the 3-degree start leave too little of the record for the solve: converge unweighted, then
            # run the weighted loop from there)
            res = e.align()
            assert res["status"] == 0, res["error"]
            e.set_robust_loss(loss, scale)
            res = e.align(guess=e.transform())
        else:
            res = e.align()
        assert res["status"] == 0, res["error"]
        assert e.stats()["loop_passes"] > 0
        S, M, kept, far_only, bent_only = final_record(e, d, m, code, scale, mnd)
        assert_gates_bite(len(d["src"]), kept, far_only, bent_only)
        assert abs(res["diff_final"] - S[33]) <= 1e-6 * S[33], (res["diff_final"], S[33])
        if code:
            assert 0.0 < S[34] < kept
        st, _, _, _, _, _, X = sym.solve(m, S, e.pivot())
        assert st == 0
        it = e.step()
        assert it["status"] == 0
        assert np.abs(it["increment"] - X).max() < 1e-6, (it["increment"], X)


# ---- 2. gate boundaries -------------------------------------------------------------------------------------------------------
GRID = 2.0 ** -15       # every coordinate and offset of the boundary data: their sums, differences and squares are exact in fp32


def exact_offset(t):
    """an offset (a, b, 0) -- a >= b >= 0 on the 2^-15 grid -- whose fp32 dist2 from the origin is exactly t (a^2 + b^2 = t with
    no rounding; t in [2^-7, 2^-6), on its 2^-30 grid), or None"""
    t = np.float32(t)
    T = float(t) / GRID ** 2
    assert T == int(T)
    T = int(T)
    for A in range(math.isqrt(T // 2), math.isqrt(T) + 1):
        B = math.isqrt(max(T - A * A, 0))
        if A >= B and A * A + B * B == T:
            off = np.array([A * GRID, B * GRID, 0], np.float32)
            assert R.dist2(off[None], np.zeros((1, 3), np.float32))[0] == t
            return off
    return None


# max_corr_dist whose fp32 square differs from the fp32 rounding of its double square (an engine that squared in double would keep
# or drop the pairs one ulp off) and whose square, one ulp below and one above are each the fp32 dist2 of a grid offset
def pinned_mcd():
    for k in range(1, 100000):
        m = 0.1 + k * 1e-6
        M = R.f32_max_d2(m)
        if M != np.float32(m * m) and all(exact_offset(t) is not None
                                          for t in (np.nextafter(M, np.float32(0)), M, np.nextafter(M, np.float32(1)))):
            return m
    raise AssertionError


# three rows +, three rows - in a 3 x 3 block of the (x, z) lattice whose two centroids agree: +-signed offsets on them add up to
# zero, and so do their moments (sum of s_r q_r x off = 0)
BALANCED = [((0, 0), 1), ((2, 1), 1), ((1, 2), 1), ((2, 0), -1), ((0, 2), -1), ((1, 1), -1)]


def boundary_data(n_cells, mcd, mnd):
    """source row i sits next to target row i on a 3-D lattice of spacing 4 (the pairing of every kind is row i -> row i):
    18 rows at d2 = max_d2 - 1 ulp, max_d2, max_d2 + 1 ulp (6 each, offsets in x and y; normals along z);
    18 rows at ndot = min_ndot - 1 ulp, min_ndot, min_ndot + 1 ulp (normals along z, offset along y); the rest on their target
    with axis normals.  Every offset lies in the plane of its normals (c = 0 for every pair: PAPER, PLANE and GICP's u and v
    rows) and every six rows of one offset are signed as BALANCED (a y level each), so that the offsets and their moments about
    any point cancel exactly (GICP's axis rows, 1/2 J^T d): the solve returns the identity, and the points stay where they are pass
    after pass."""
    g = int(np.ceil(n_cells ** (1 / 3)))
    L = np.stack(np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij"), -1).reshape(-1, 3)[:n_cells]
    row = {tuple(v): i for i, v in enumerate(L)}
    tgt = (4.0 * L).astype(np.float32)
    src = tgt.copy()
    axes = np.eye(3, dtype=np.float32)
    tn = axes[np.arange(n_cells) % 3].copy()
    sn = tn.copy()
    # the six rows of group k: y level k, x in 0..2, z in 0..2 (distance rows) or 3..5 (normal rows)
    group = lambda k, z0: [(row[(x, k, z0 + z)], sg) for (x, z), sg in BALANCED]                  # noqa: E731
    d_rows, n_rows = [], []
    M = R.f32_max_d2(mcd)
    for k, t in enumerate([np.nextafter(M, np.float32(0)), M, np.nextafter(M, np.float32(1))]):
        off = exact_offset(t)
        for r, sg in group(k, 0):
            src[r] = tgt[r] + np.float32(sg) * off
            assert R.dist2(src[r:r + 1], tgt[r:r + 1])[0] == t
            sn[r] = tn[r] = (0, 0, 1)
            d_rows.append(r)
    G = np.float32(mnd)
    for k, t in enumerate([np.nextafter(G, np.float32(-1)), G, np.nextafter(G, np.float32(2))]):
        for r, sg in group(k, 3):
            src[r] = tgt[r] + np.float32([0, 0.0625 * sg, 0])
            sn[r] = (0, 0, 1)
            tn[r] = (0, 0, t)
            n_rows.append(r)
    d = dict(src=src, src_n=sn, tgt=tgt, tgt_n=tn)
    keep = R.gate(src, sn, tgt, tn, M, G)
    drop = np.concatenate([d_rows[12:], n_rows[:6]])
    assert keep.sum() == n_cells - 12 and not keep[drop].any()     # exactly the 6 + 6 rows beyond a bound drop
    off = (src - tgt).astype(np.float64)
    assert not off.sum(0).any() and not np.cross(tgt.astype(np.float64), off).sum(0).any()
    return d


BOUNDARY_CASES = [("identity", 216), ("identity", 215), ("identity", 217), ("brute", 215), ("tree", 215)]


# (PAPER's cases keep the ids they had before GICP's joined them)
@pytest.mark.parametrize("mode,corr,n", [pytest.param(m, c, n, id=("" if m == "paper" else m + "-") + "%s-%d" % (c, n))
                                         for m in ("paper", "gicp") for c, n in BOUNDARY_CASES])
def test_gate_boundaries_are_kept(sym, mode, corr, n):
    """the first pass (identity transform) over the boundary pairs: k_pass_identity<4> (n = 216) and <1>, k_pass_indexed, k_accumulate"""
    mcd, mnd = pinned_mcd(), 0.75
    d = boundary_data(n, mcd, mnd)
    M = R.f32_max_d2(mcd)
    m = mode_code(sym, mode)
    with sym.Engine(mode=m, corr=corr_code(sym, corr), max_iters=3, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=mnd) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        it = e.begin()
        idx, d2 = e.correspondences()
        assert np.array_equal(idx, np.arange(n)) and np.array_equal(d2, R.dist2(d["src"], d["tgt"]))
        S, Mg, kept = R.record(m, d["src"], d["src_n"], d["tgt"], d["tgt_n"], None, e.pivot(), 0, 1.0, M, mnd)
        assert kept == n - 12
        assert it["sums"][34] == kept, (it["sums"][34], kept)
        R.assert_record(it["sums"], S, Mg, R.TOL_EXACT, "begin")


@pytest.mark.parametrize("mode", ["paper", "plane", "gicp"])
def test_gate_boundaries_through_the_fused_pass(sym, mode):
    """the device-driven loop over the boundary pairs: k_pass_fused's fused_accumulate gates.  The diff of every pass (slot 33,
    sum of sqrt(d2) over the kept pairs) counts the kept distance-boundary and normal-boundary pairs"""
    mcd, mnd = pinned_mcd(), 0.75
    n = 216
    d = boundary_data(n, mcd, mnd)
    m = mode_code(sym, mode)                          # (each OBJ instantiation of the fused pass gates on its own)
    M = R.f32_max_d2(mcd)
    with sym.Engine(mode=m, corr=sym.CORR_TREE, max_iters=12, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=mnd) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        r = e.align()
        assert r["status"] == 0, r["error"]
        assert e.stats()["loop_passes"] > 0
        assert np.array_equal(e.transform(), np.eye(4, dtype=np.float32))
        S, _, kept = R.record(m, d["src"], d["src_n"], d["tgt"], d["tgt_n"], None, e.pivot(), 0, 1.0, M, mnd)
    want = np.float32(S[33])
    # one pair more or less moves the sum by 0.0625 at least (the normal-boundary rows) out of ~3
    assert np.all(r["diffs"][:r["iters"]] == want), (r["diffs"], want)
    assert r["diff_final"] == want


def test_max_d2_is_the_fp32_square():
    m = pinned_mcd()
    assert R.f32_max_d2(m) == np.float32(np.float32(m) * np.float32(m)) != np.float32(m * m)


# ---- 3. sharded pass kinds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [3, 5])
@pytest.mark.parametrize("mode", ["paper", "p2p", "plane", "gicp"])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_sharded_pass_kinds(sym, cat, world, mode, corr):
    """external exchange over `world` ranks (shares whose offsets are not all multiples of 4),
    a distance gate and Huber weights: the rank records add up to the unsharded record, the pairs tile the unsharded pairs, every rank
    computes the same 4x4 and it follows the unsharded run"""
    from symmicp import synth
    n = 3400 if world == 3 else 3398                 # shares 1134 / 1133 / 1133 and 680 / 680 / 680 / 679 / 679
    d = synth.perturbed(cat["src"][:n], cat["src_n"][:n])
    m = mode_code(sym, mode)
    d2_0 = R.dist2(d["src"], d["tgt"]) if corr == "identity" else R.nn_ref(d["src"], d["tgt"])[1]
    mcd = float(np.sqrt(np.quantile(d2_0, 0.75)))
    scale = HUBER[mode] if mode != "p2p" else 0.5 * float(np.sqrt(np.median(d2_0)))
    kw = dict(mode=m, corr=corr_code(sym, corr), max_iters=6, fixed_iters=1, max_corr_dist=mcd)
    steps = 3
    with sym.Engine(**kw) as ref:
        ref.set_target(d["tgt"], d["tgt_n"])
        ref.set_source(d["src"], d["src_n"])
        ref.set_robust_loss("huber", scale)
        recs_ref = [ref.begin()["sums"]]
        pairs_ref = [ref.correspondences()]
        T_ref = []
        for _ in range(steps):
            recs_ref.append(ref.step()["sums"])
            pairs_ref.append(ref.correspondences())
            T_ref.append(ref.transform())
        S, M, kept = R.record(m, *R.moved(ref.transform(), d["src"], d["src_n"], m), d["tgt"], d["tgt_n"], pairs_ref[-1][0],
                              ref.pivot(), 1, scale, R.f32_max_d2(mcd))
        R.assert_record(recs_ref[-1], S, M, R.TOL_REC, "unsharded")
        assert 0 < recs_ref[0][37] < n                 # the gate drops pairs of the first pass
    engs = [sym.Engine(**kw) for _ in range(world)]
    try:
        for r, e in enumerate(engs):
            e.comm_init_rank(world, r, None)
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            e.set_robust_loss("huber", scale)
        offs = [e.local_offset() for e in engs]
        assert sum(e.local_count() for e in engs) == n and any(o % 4 for o in offs), offs       # (k_pass_identity<1>)
        its = [e.begin() for e in engs]
        for k in range(steps + 1):
            total = np.sum([np.asarray(it["sums"], np.float64) for it in its], axis=0)
            # the shards' records sum to the unsharded one up to the order of the fp64 sums: the bar of the numpy record
            S, M, _ = R.record(m, *R.moved(engs[0].transform(), d["src"], d["src_n"], m), d["tgt"], d["tgt_n"], pairs_ref[k][0],
                               engs[0].pivot(), 1, scale, R.f32_max_d2(mcd))
            R.assert_record(total, recs_ref[k], M, R.TOL_EXACT * 10, "pass %d" % k)
            R.assert_record(total, S, M, R.TOL_REC, "pass %d vs numpy" % k)
            idx = np.full(n, -1, np.int32)
            d2 = np.zeros(n, np.float32)
            owned = np.zeros(n, np.int32)
            for e in engs:
                i_r, d_r = e.correspondences()
                if corr == "identity":
                    # an unsorted share reports its pairs at share rows 0 .. count - 1 (include/symmicp.h,
                    # symmicp_get_correspondences): move them to the caller's rows
                    o, c = e.local_offset(), e.local_count()
                    assert (i_r[c:] == -1).all()
                    i_r, d_r = np.roll(i_r, o), np.roll(d_r, o)
                has = i_r >= 0
                assert np.array_equal(np.flatnonzero(has), np.arange(e.local_offset(), e.local_offset() + e.local_count()))
                owned += has
                idx[has] = i_r[has]
                d2[has] = d_r[has]
            assert np.all(owned == 1)
            assert np.array_equal(idx, pairs_ref[k][0]) and np.array_equal(d2, pairs_ref[k][1])
            if k == steps:
                break
            for e in engs:
                e.set_sums(total)
            its = [e.step() for e in engs]
            Ts = [e.transform() for e in engs]
            assert all(np.array_equal(Ts[0], T) for T in Ts[1:])
            assert np.abs(Ts[0] - T_ref[k]).max() < 1e-6
    finally:
        for e in engs:
            e.close()


# ---- 4. device loop with gates ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c5s(sym):
    """the scan-like pair of test_device_loop_matches_host_loop's straggler case: its work list of far stragglers stays non-empty for
    a dozen passes, so the device-driven run carries the straggler stage (k_search_walk + k_accumulate_list behind every fused pass)"""
    from symmicp import synth
    return with_converged_gates(synth.c5_scan(64 * 16384))


def identity_with_outliers(cat):
    """cat[:3399] against itself moved by 15 degrees (row for row; 3399 % 4 != 0: k_pass_identity<1>), every tenth target row
    pushed far away and every third source normal reversed: the distance gate (set just above the largest distance of the other
    rows) and the normal gate keep dropping those rows however the alignment goes"""
    from symmicp import synth
    d = synth.perturbed(cat["src"][:3399], cat["src_n"][:3399])
    ok = np.ones(3399, bool)
    ok[::10] = False
    mcd = 1.01 * float(np.sqrt(R.dist2(d["src"], d["tgt"])[ok].max()))
    d["tgt"] = d["tgt"].copy()
    d["tgt"][~ok] += np.float32(20.0 * mcd)
    d["src_n"] = d["src_n"].copy()
    d["src_n"][::3] *= -1
    return dict(d, mcd=mcd)


@pytest.mark.parametrize("case", ["paper_tree", "plane_tree", "paper_identity_ragged", "paper_tree_stragglers", "gicp_tree",
                                  "gicp_identity_ragged"])
def test_device_loop_with_gates_matches_host_loop(sym, cat, c4, case, request):
    """as test_device_loop_matches_host_loop (test_gpu_parity.py), with both gates biting in the passes the device runs: the last
    device pass's diff (slot 33) is the numpy record's at the final pose, with the gates' drops"""
    mode = mode_code(sym, case.split("_")[0])
    ragged = case.endswith("_identity_ragged")
    mnd = 0.5 if ragged else 0.0
    if ragged:
        d = identity_with_outliers(cat)
        assert len(d["src"]) % 4 != 0
        kw = dict(mode=mode, corr=sym.CORR_IDENTITY, max_iters=8, fixed_iters=1)
    elif case == "paper_tree_stragglers":
        d = request.getfixturevalue("c5s")
        kw = dict(mode=mode, corr=sym.CORR_TREE, max_iters=40, fixed_iters=1)
    else:
        d = c4
        kw = dict(mode=mode, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1)
    kw.update(max_corr_dist=d["mcd"], min_normal_dot=mnd)
    res = {}
    for host_loop in (1, 0):
        with sym.Engine(host_loop=host_loop, **kw) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            r = e.align()
            st = e.stats()
            if host_loop == 0:
                if ragged:
                    p, pn = R.moved(e.transform(), d["src"], d["src_n"], kw["mode"])
                    S, _, kept = R.record(kw["mode"], p, pn, d["tgt"], d["tgt_n"], None, e.pivot(), 0, 1.0, R.f32_max_d2(d["mcd"]), mnd)
                    q, qn = d["tgt"], d["tgt_n"]
                    far = ~R.gate(p, pn, q, qn, R.f32_max_d2(d["mcd"]))
                    bent = ~R.gate(p, pn, q, qn, 0.0, mnd)
                    assert_gates_bite(len(p), kept, int((far & ~bent).sum()), int((bent & ~far).sum()))
                else:
                    S, _, kept, far_only, bent_only = final_record(e, d, kw["mode"], 0, 1.0, mnd)
                    assert_gates_bite(len(d["src"]), kept, far_only, bent_only)
                assert abs(r["diff_final"] - S[33]) <= 1e-6 * S[33], (r["diff_final"], S[33])
            res[host_loop] = (r, st)
    (rh, sh), (rd, sd) = res[1], res[0]
    assert rh["status"] == rd["status"] == 0
    assert rh["iters"] == rd["iters"] == kw["max_iters"], (rh["iters"], rd["iters"])
    n = rh["iters"]
    assert np.allclose(rh["diffs"][:n], rd["diffs"][:n], rtol=2e-6, atol=1e-6), (rh["diffs"][:n], rd["diffs"][:n])
    assert np.abs(rh["transform"] - rd["transform"]).max() < 1e-6 * max(1.0, float(np.abs(rh["transform"]).max()))
    assert abs(rh["diff_final"] - rd["diff_final"]) <= 2e-6 * max(1.0, abs(rh["diff_final"]))
    assert sh["loop_passes"] == 0 and sd["loop_passes"] > 0
    if kw["corr"] == sym.CORR_TREE:
        assert sd["passes"] == sh["passes"]
    if case == "paper_tree_stragglers":
        assert sd["loop_straggler_passes"] > 0, sd
