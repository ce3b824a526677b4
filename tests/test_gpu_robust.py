"""GPU tests of the robust loss (symmicp_set_robust_loss, run with -m gpu on a real MI355X): the weighted reduction record of
every accumulating kernel against an fp64 numpy record built here from the engine's own points and pairs, off-means-off, the
device-driven loop against the host loop, and recovery from outliers that the unweighted loop cannot shake off.

The numpy record repeats the kernels' fp32 expressions (rows of func.cpp:51-58, the weight of robust_loss.h) element by
element and sums in fp64, so the two agree to the summation order: a slot is compared at 1e-6 of the sum of its terms'
magnitudes (a slot that cancels to ~0 is not held to its own tiny value)."""
import os

import numpy as np
import pytest

from _record_ref import TOL_REC, np_weight, record_terms, xf_rows

pytestmark = pytest.mark.gpu


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
def c4(sym):
    """the 200k-point surface pair of test_device_loop_matches_host_loop, and a residual scale: the median |c| of its first pairs"""
    from symmicp import synth
    d = synth.c4_surface(200000)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.begin()
        _, _, r = engine_record(e, d, 0, 1.0)
    d["c_median"] = float(np.median(np.abs(r)))
    return d


def engine_record(e, d, loss, scale, p2p=False, identity=False):
    """the record the engine's current pairs must give: the source moved by e.transform() the way the pass kernels move it
    (cumulative apply, normals rotated only), e.correspondences(), e.pivot() and the target"""
    p, pn = xf_rows(e.transform(), d["src"], 1.0), xf_rows(e.transform(), d["src_n"], 0.0)
    tgt, tgt_n = d["tgt"], d["tgt_n"]
    idx, d2 = e.correspondences()
    if identity:
        idx = np.arange(len(p), dtype=np.int64)
    keep = idx >= 0
    T, r = record_terms(p[keep], pn[keep], tgt[idx[keep]], tgt_n[idx[keep]], e.pivot(), loss, scale, p2p)
    return T.sum(0), np.abs(T).sum(0), r


def assert_record(gpu, ref, mag, tag=""):
    gpu = np.asarray(gpu, np.float64)
    err = np.abs(gpu[:37] - ref[:37])
    bad = np.nonzero(err > TOL_REC * np.maximum(mag[:37], 1e-300))[0]
    assert bad.size == 0, (tag, [(int(k), gpu[k], ref[k], mag[k]) for k in bad[:6]])
    assert gpu[37] == ref[37], (tag, gpu[37], ref[37])       # the pair count, exactly


def rot_err(X, truth):
    """rotation angle of X R_truth^T (stable near 0) and the largest translation error"""
    Rd = np.asarray(X, np.float64)[:3, :3] @ np.asarray(truth, np.float64)[:3, :3].T
    s = np.linalg.norm(Rd - Rd.T) / (2.0 * np.sqrt(2.0))
    c = (np.trace(Rd) - 1.0) / 2.0
    return float(np.arctan2(s, c)), float(np.abs(np.asarray(X, np.float64)[:3, 3] - np.asarray(truth, np.float64)[:3, 3]).max())


# ---- 1. record parity --------------------------------------------------------------------------------------------------
SCALES = {"huber": 2.0, "tukey": 40.0, "cauchy": 4.0, "geman_mcclure": 8.0}      # (cat: c of the 15-degree start spans ~0 .. 100)
CASES = [("paper", "identity"), ("paper", "brute"), ("paper", "tree"), ("p2p", "tree")]


@pytest.mark.parametrize("loss", list(SCALES))
@pytest.mark.parametrize("mode,corr", CASES)
def test_weighted_record_matches_numpy(sym, cat15, loss, mode, corr):
    d = cat15
    p2p = mode == "p2p"
    m = sym.MODE_P2P if p2p else sym.MODE_PAPER
    cr = {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[corr]
    code = sym.loss_code(loss)
    scale = SCALES[loss] * (4.0 if p2p else 1.0)
    with sym.Engine(mode=m, corr=cr, max_iters=30) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_robust_loss(loss, scale)
        assert e.robust_loss() == (code, np.float32(scale))
        it = e.begin()
        ref, mag, r = engine_record(e, d, code, scale, p2p, corr == "identity")
        assert_record(it["sums"], ref, mag, "begin")
        assert it["pairs"] == ref[37]
        w = np_weight(code, scale, r)
        assert 0.0 < w.sum() < len(w)                   # the weights bite: neither all 1 nor all 0
        for k in range(2):
            it = e.step()
            ref, mag, _ = engine_record(e, d, code, scale, p2p, corr == "identity")
            assert_record(it["sums"], ref, mag, "step %d" % (k + 1))
        if corr == "tree":
            # the passes after the first one settle pairs by their certificates (k_search_cells) or search them again
            ce, _, _, _ = e.certificates()
            assert (ce[:, 3] > 0).any()


@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_weighted_record_of_the_fused_pass(sym, c4, loss):
    """a converged alignment runs pass after pass on the device (k_pass_fused: certified pairs, neighbourhood certificates,
    k_reduce_solve's solve).  The record the device loop leaves must be the numpy record of the pairs it left: the next
    host step solves from it."""
    d = c4
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        scale = d["c_median"] * (2.0 if loss == "huber" else 8.0)
        e.set_robust_loss(loss, scale)
        res = e.align()
        assert res["status"] == 0, res["error"]
        st = e.stats()
        assert st["loop_passes"] > 0, st                  # the fused pass ran
        ref, mag, _ = engine_record(e, d, sym.loss_code(loss), scale)
        s_ok, _, _, _, _, _, X = sym.solve(sym.MODE_PAPER, np.concatenate([ref, np.zeros(sym.NSUM - len(ref))]), e.pivot())
        assert s_ok == 0
        it = e.step()
        assert it["status"] == 0
        assert np.abs(it["increment"] - X).max() < 1e-6, (it["increment"], X)


# ---- 2. off means off ----------------------------------------------------------------------------------------------------
def _run_steps(sym, d, n_steps, setup=None, **kw):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, **kw) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        if setup:
            setup(e)
        recs = [e.begin()["sums"]]
        for _ in range(n_steps):
            recs.append(e.step()["sums"])
        return np.array(recs), e.transform().copy()


def test_loss_none_is_bit_for_bit_unweighted(sym, cat15):
    r0, X0 = _run_steps(sym, cat15, 4)
    r1, X1 = _run_steps(sym, cat15, 4, setup=lambda e: e.set_robust_loss(sym.LOSS_NONE, 5.0))
    r2, X2 = _run_steps(sym, cat15, 4, setup=lambda e: (e.set_robust_loss("huber", 3.0), e.set_robust_loss("none", 0.0)))
    assert np.array_equal(r0, r1) and np.array_equal(X0, X1)
    assert np.array_equal(r0, r2) and np.array_equal(X0, X2)
    assert (r0[:, 37] == 0).all()
    # Huber with an enormous scale weighs every pair 1: the same sums, and the pair count in slot 37
    r3, X3 = _run_steps(sym, cat15, 4, setup=lambda e: e.set_robust_loss("huber", 1e30))
    assert np.abs(r3[:, :37] - r0[:, :37]).max() <= 1e-12 * np.abs(r0[:, :37]).max()
    assert np.abs(X3 - X0).max() <= 1e-12 * max(1.0, np.abs(X0).max()) + 1e-30
    assert np.array_equal(r3[:, 37], r0[:, 34])
    # the device-driven loop too
    out = []
    for setup in (None, lambda e: e.set_robust_loss("none", 1.0)):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30) as e:
            e.set_target(cat15["tgt"], cat15["tgt_n"])
            e.set_source(cat15["src"], cat15["src_n"])
            if setup:
                setup(e)
            out.append(e.align())
    assert out[0]["iters"] == out[1]["iters"] and np.array_equal(out[0]["transform"], out[1]["transform"])


# ---- 3. device loop = host loop ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_device_loop_matches_host_loop_weighted(sym, c4, loss):
    d = c4
    res = {}
    scale = d["c_median"] * (2.0 if loss == "huber" else 8.0)
    for host_loop in (1, 0):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1, host_loop=host_loop) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            e.set_robust_loss(loss, scale)
            res[host_loop] = (e.align(), e.stats())
    (rh, sh), (rd, sd) = res[1], res[0]
    assert rh["status"] == rd["status"] == 0
    assert rh["iters"] == rd["iters"] == 25
    n = rh["iters"]
    assert np.allclose(rh["diffs"][:n], rd["diffs"][:n], rtol=2e-6, atol=1e-6), (rh["diffs"][:n], rd["diffs"][:n])
    assert np.abs(rh["transform"] - rd["transform"]).max() < 1e-6 * max(1.0, float(np.abs(rh["transform"]).max()))
    assert sh["loop_passes"] == 0 and sd["loop_passes"] > 0
    assert sd["passes"] == sh["passes"]
    # and the loss changed the answer (the same run unweighted ends elsewhere)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        ru = e.align()
    assert not np.array_equal(ru["transform"], rd["transform"])


# ---- 4. outliers ---------------------------------------------------------------------------------------------------------
def with_outliers(cat, frac=0.3, seed=7):
    """cat against itself moved by 15 degrees; 30 % of the source rows replaced by points drawn uniformly from the source's
    bounding box grown by half on every side, with random unit normals"""
    from symmicp import synth
    d = synth.perturbed(cat["src"], cat["src_n"])
    src, sn = d["src"].copy(), d["src_n"].copy()
    rng = np.random.default_rng(seed)
    n = len(src)
    rows = rng.choice(n, int(frac * n), replace=False)
    lo, hi = src.min(0), src.max(0)
    c, h = (lo + hi) / 2, (hi - lo) / 2 * 1.5
    src[rows] = rng.uniform(c - h, c + h, (len(rows), 3)).astype(np.float32)
    v = rng.normal(size=(len(rows), 3))
    sn[rows] = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    d.update(src=src, src_n=sn, extent=float(np.linalg.norm(hi - lo)))
    return d


# Calibrated with a CPU IRLS (cKDTree pairs + the library's host solve on the weighted numpy record, 60 iterations): unweighted
# 0.088 rad / 1.2e-2 of the extent off the truth; Tukey annealed 200 -> 2 and Geman-McClure at 2 both below 1e-5 rad / 1e-5.
UNWEIGHTED_MIN_ROT = 0.02


def test_outliers_defeat_the_unweighted_loop(sym, cat):
    d = with_outliers(cat)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=60, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        r = e.align()
    assert r["status"] == 0
    ang, dt = rot_err(r["transform"], d["truth"])
    assert ang > UNWEIGHTED_MIN_ROT, (ang, dt)


def test_outliers_geman_mcclure(sym, cat):
    d = with_outliers(cat)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=60, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_robust_loss(sym.LOSS_GEMAN_MCCLURE, 2.0)
        r = e.align()
    assert r["status"] == 0, r["error"]
    ang, dt = rot_err(r["transform"], d["truth"])
    assert ang < 1e-3 and dt < 1e-3 * d["extent"], (ang, dt)


def test_outliers_tukey_annealed_through_step(sym, cat):
    d = with_outliers(cat)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=1000) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_robust_loss("tukey", 200.0)
        e.begin()
        for k in range(60):
            it = e.step()
            assert it["status"] == 0
            assert it["pairs"] == len(d["src"])
            e.set_robust_loss("tukey", max(2.0, 200.0 * 0.5 ** (k + 1)))
        X = e.transform()
    ang, dt = rot_err(X, d["truth"])
    assert ang < 1e-3 and dt < 1e-3 * d["extent"], (ang, dt)


# ---- 5. annealing between steps --------------------------------------------------------------------------------------------
def test_new_scale_takes_effect_at_the_next_pass(sym, cat15):
    d = cat15
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_robust_loss("cauchy", 8.0)
        e.begin()
        e.step()
        e.set_robust_loss("cauchy", 1.0)
        it = e.step()
        ref, mag, _ = engine_record(e, d, sym.LOSS_CAUCHY, 1.0)
        assert_record(it["sums"], ref, mag, "annealed")
        ref8, _, _ = engine_record(e, d, sym.LOSS_CAUCHY, 8.0)
        assert abs(it["sums"][34] - ref8[34]) > 1e-3 * ref8[34]          # not the old scale's record


# ---- 6. errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors(sym, cat15):
    d = cat15
    with sym.Engine(mode=sym.MODE_QUIRKS, corr=sym.CORR_IDENTITY) as e:
        for loss in ("huber", "tukey", sym.LOSS_CAUCHY, sym.LOSS_GEMAN_MCCLURE):
            with pytest.raises(sym.SymmIcpError) as x:
                e.set_robust_loss(loss, 1.0)
            assert x.value.status == sym.ERR_ARG
        e.set_robust_loss("none", 0.0)                      # allowed
        assert e.robust_loss() == (sym.LOSS_NONE, 0.0)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        for loss, scale in [(5, 1.0), (-1, 1.0), ("huber", 0.0), ("huber", -2.0), ("tukey", float("nan")), ("cauchy", float("inf"))]:
            with pytest.raises(sym.SymmIcpError) as x:
                e.set_robust_loss(loss, scale)
            assert x.value.status == sym.ERR_ARG, (loss, scale)
        assert e.robust_loss() == (sym.LOSS_NONE, 0.0)     # a refused call changes nothing
        e.set_robust_loss("huber", 1.5)
        # switching a context that carries a loss into QUIRKS is refused the same way
        with pytest.raises(sym.SymmIcpError) as x:
            e.set_config(mode=sym.MODE_QUIRKS)
        assert x.value.status == sym.ERR_ARG
        e.cfg.mode = sym.MODE_PAPER
        assert e.robust_loss() == (sym.LOSS_HUBER, np.float32(1.5))


def test_tukey_below_every_residual_is_degenerate(sym, cat15):
    d = cat15
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.begin()
        _, _, r = engine_record(e, d, 0, 1.0)
        scale = float(np.abs(r[r != 0]).min()) * 1e-3
        e.set_robust_loss("tukey", scale)
        X0 = e.transform().copy()
        it = e.begin()
        assert it["sums"][34] < 6.0                        # (pairs with c == 0 exactly keep weight 1)
        with pytest.raises(sym.SymmIcpError) as x:
            e.step()
        assert x.value.status == sym.ERR_DEGENERATE
        assert np.isfinite(e.transform()).all() and np.array_equal(e.transform(), X0)
        r = e.align()
        assert r["status"] == sym.ERR_DEGENERATE and np.isfinite(r["transform"]).all()


# ---- 7. the command-line driver ----------------------------------------------------------------------------------------------
def test_driver_loss(sym, cat, tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT, GOLDEN
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    shutil.copy(os.path.join(GOLDEN, "cat.pcd"), tmp_path / "cat.pcd")
    shutil.copy(os.path.join(GOLDEN, "cat_out.pcd"), tmp_path / "cat_out.pcd")
    scale = 0.5
    r = subprocess.run([exe, "--mode", "paper", "--corr", "tree", "--loss", "huber", "--loss-scale", str(scale), "cat.pcd", "cat_out.pcd"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    k = out.index("Result transform:")
    T = np.array([[float(v) for v in out[k + 1 + i].split()] for i in range(4)])
    # the same run through the Python engine, normals from the same GPU k-NN PCA the class uses (myicp.cpp:152-172)
    src, tgt = cat["src"], cat["tgt"]
    sn, _ = sym.estimate_normals(src, 10)
    tn, _ = sym.estimate_normals(tgt, 10)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_target(tgt, tn)
        e.set_source(src, sn)
        e.set_robust_loss("huber", scale)
        rp = e.align()
    assert rp["status"] == 0
    assert np.abs(T - rp["transform"]).max() < 1e-4, (T, rp["transform"])
    # a loss with the reference's arithmetic is a usage error
    r = subprocess.run([exe, "--mode", "quirks", "--loss", "huber", "--loss-scale", "1", "cat.pcd", "cat_out.pcd"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 64
    # the class itself refuses it as well
    m = sym.MyICP(mode=sym.MODE_QUIRKS, verbose=False)
    m.setRobustLoss("huber", 1.0)
    m.setInputSource(src, cat["src_n"])
    m.setInputTarget(tgt, cat["tgt_n"])
    with pytest.raises(sym.SymmIcpError) as x:
        m.align()
    assert x.value.status == sym.ERR_ARG
