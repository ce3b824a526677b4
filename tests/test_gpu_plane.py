"""GPU tests of the point-to-plane mode (SYMMICP_MODE_PLANE, run with -m gpu on a real MI355X): every pass kind's pairs against the
oracle's brute-force nearest neighbours and its record against the numpy PLANE record of _plane_ref.py, a source without normals
against the same source with them, the device-driven loop against the host loop, power-of-two units, convergence, sharding by
external exchange, and the command-line driver.

Records are compared slot by slot at a fraction of the sum of the slot's term magnitudes: 1e-9 unweighted (the numpy terms repeat
the kernels' fp32 rows exactly; only the fp64 summation order differs) and 1e-6 with a robust loss (test_gpu_robust.py's bar)."""
import os

import numpy as np
import pytest

from _frames import scale_record
from _plane_ref import plane_record, plane_terms, rot_err

pytestmark = pytest.mark.gpu

SCALES = {"none": 1.0, "huber": 1.0, "tukey": 20.0, "cauchy": 2.0, "geman_mcclure": 4.0}   # (cat15: |c| spans ~0 .. 50)


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
    return oracle.apply(X, src, True), (None if src_n is None else oracle.apply(X, src_n, False))


def _check_pass(sym, oracle, e, it, d, corr, loss, scale, min_ndot=None, tag=""):
    p, pn = _positions(sym, oracle, e, d["src"], d["src_n"])
    idx, d2 = e.correspondences()
    if corr == "identity":
        idx = np.arange(len(p), dtype=np.int32)
    else:
        ri, rd = oracle.nn_brute(p, d["tgt"])
        assert np.array_equal(idx, ri), (tag, int((idx != ri).sum()))
        assert np.array_equal(d2, rd), (tag, int((d2 != rd).sum()))
    keep = idx >= 0
    if min_ndot is not None:
        nq = d["tgt_n"][idx]
        dot = (pn[:, 0] * nq[:, 0] + pn[:, 1] * nq[:, 1]) + pn[:, 2] * nq[:, 2]
        keep &= ~(dot < np.float32(min_ndot))
        if tag == "begin":
            assert 0 < keep.sum() < len(keep)                   # the gate bites
    code = sym.loss_code(loss)
    S, M = plane_record(p[keep], d["tgt"][idx[keep]], d["tgt_n"][idx[keep]], e.pivot(), code, scale)
    assert_record(it["sums"], S, M, code != 0, tag)


# ---- 1. every pass kind, every loss --------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", list(SCALES))
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_plane_passes_match_numpy_record(sym, oracle, cat15, corr, loss):
    d = cat15
    with sym.Engine(mode=sym.MODE_PLANE, corr=_corr(sym, corr), max_iters=30, host_loop=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], None)
        if loss != "none":
            e.set_robust_loss(loss, SCALES[loss])
        it = e.begin()
        _check_pass(sym, oracle, e, it, dict(d, src_n=None), corr, loss, SCALES[loss], tag="begin")
        for k in range(3):
            it = e.step()
            _check_pass(sym, oracle, e, it, dict(d, src_n=None), corr, loss, SCALES[loss], tag="step %d" % (k + 1))


@pytest.mark.parametrize("variant", ["normal_gate", "incremental"])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_plane_passes_that_read_source_normals(sym, oracle, cat15, corr, variant):
    """the paths that still load source normals: the min_normal_dot gate, and write-back (APPLY_INCREMENTAL)"""
    d = cat15
    kw = dict(min_normal_dot=0.97) if variant == "normal_gate" else dict(apply=sym.APPLY_INCREMENTAL)
    with sym.Engine(mode=sym.MODE_PLANE, corr=_corr(sym, corr), max_iters=30, **kw) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        it = e.begin()
        gate = kw.get("min_normal_dot")
        _check_pass(sym, oracle, e, it, d, corr, "none", 1.0, gate, "begin")
        for k in range(3):
            it = e.step()
            _check_pass(sym, oracle, e, it, d, corr, "none", 1.0, gate, "step %d" % (k + 1))
        if variant == "incremental":
            assert np.abs(e.source()[1] - oracle.apply(e.transform(), d["src_n"], False)).max() < 1e-5


@pytest.mark.parametrize("loss", ["none", "huber"])
def test_fused_pass_record(sym, oracle, c4, loss):
    """a converged PLANE alignment runs pass after pass on the device (k_pass_fused<true, W, true>, k_reduce_solve's solve_plane).
    The record it leaves is the numpy record of its pairs: the next host step solves from it."""
    d = c4
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=25, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], None)
        scale = 1e-5                                                   # (~2x the median |c| at the truth)
        if loss != "none":
            e.set_robust_loss(loss, scale)
        res = e.align()
        assert res["status"] == 0, res["error"]
        assert e.stats()["loop_passes"] > 0
        p = oracle.apply(e.transform(), d["src"], True)
        idx, _ = e.correspondences()
        keep = idx >= 0
        S, _ = plane_record(p[keep], d["tgt"][idx[keep]], d["tgt_n"][idx[keep]], e.pivot(), sym.loss_code(loss), scale)
        if loss != "none":
            w = plane_terms(p[keep], d["tgt"][idx[keep]], d["tgt_n"][idx[keep]], e.pivot(), 1, scale)[0][:, 34]
            assert w.sum() < 0.9 * len(w)                              # the weights bite
        st, _, _, _, _, _, X = sym.solve(sym.MODE_PLANE, S, e.pivot())
        assert st == 0
        it = e.step()
        assert np.abs(it["increment"] - X).max() < 1e-6, (it["increment"], X)


# ---- 2. source normals not needed ----------------------------------------------------------------------------------------
def _passes(sym, d, nrm, n=5, **kw):
    with sym.Engine(mode=sym.MODE_PLANE, max_iters=30, **kw) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], nrm)
        recs = [e.begin()["sums"]]
        for _ in range(n):
            recs.append(e.step()["sums"])
        return np.array(recs), e.transform().copy()


@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_no_source_normals_is_bit_identical(sym, cat15, c4, corr):
    d = cat15
    r0, X0 = _passes(sym, d, d["src_n"], corr=_corr(sym, corr))
    r1, X1 = _passes(sym, d, None, corr=_corr(sym, corr))
    assert np.array_equal(r0, r1) and np.array_equal(X0, X1)
    if corr == "tree":                                  # and through the device loop (fused pass)
        out = []
        for nrm in (c4["src_n"], None):
            with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=20, fixed_iters=1) as e:
                e.set_target(c4["tgt"], c4["tgt_n"])
                e.set_source(c4["src"], nrm)
                out.append((e.align(), e.stats()))
        assert out[0][1]["loop_passes"] > 0 and out[1][1]["loop_passes"] == out[0][1]["loop_passes"]
        assert np.array_equal(out[0][0]["transform"], out[1][0]["transform"])
        assert np.array_equal(out[0][0]["diffs"], out[1][0]["diffs"])
        # 12 B per source point less: no source normals streamed
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
            e.set_target(c4["tgt"], c4["tgt_n"])
            e.set_source(c4["src"], c4["src_n"])
            e.begin()
            b_paper = e.stats()["bytes_algorithmic_per_pass"]
        assert out[1][1]["bytes_algorithmic_per_pass"] == b_paper - 12 * len(c4["src"])


def test_null_normals_rules(sym, cat15):
    d = cat15
    for mode in (sym.MODE_QUIRKS, sym.MODE_PAPER, sym.MODE_P2P):
        with sym.Engine(mode=mode, corr=sym.CORR_TREE) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            with pytest.raises(sym.SymmIcpError) as x:
                e.set_source(d["src"], None)
            assert x.value.status == sym.ERR_ARG, mode
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, min_normal_dot=0.5) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        with pytest.raises(sym.SymmIcpError) as x:
            e.set_source(d["src"], None)                  # nothing to gate on
        assert x.value.status == sym.ERR_ARG
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_IDENTITY, apply=sym.APPLY_INCREMENTAL) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], None)
        for kw, status in ((dict(mode=sym.MODE_PAPER), sym.ERR_STATE), (dict(mode=sym.MODE_QUIRKS), sym.ERR_STATE),
                           (dict(mode=sym.MODE_P2P), sym.ERR_STATE), (dict(min_normal_dot=0.5), sym.ERR_ARG)):
            with pytest.raises(sym.SymmIcpError) as x:
                e.set_config(**kw)
            assert x.value.status == status, kw
            e.cfg = sym.default_config(mode=sym.MODE_PLANE, corr=sym.CORR_IDENTITY, apply=sym.APPLY_INCREMENTAL)
        e.set_config(max_iters=5)                         # PLANE itself stays allowed
        e.begin()
        e.step()
        _, nrm = e.source()
        assert (nrm == 0).all()                           # documented: zero normals
        # a source WITH normals lifts the restriction
        e.set_source(d["src"], d["src_n"])
        e.set_config(mode=sym.MODE_PAPER)


# ---- 3. device loop = host loop --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tree_c4", "identity_cat15"])
def test_device_loop_matches_host_loop(sym, c4, cat15, case):
    d, kw = (c4, dict(corr=sym.CORR_TREE, max_iters=25)) if case == "tree_c4" else (cat15, dict(corr=sym.CORR_IDENTITY, max_iters=8))
    res = {}
    for host_loop in (1, 0):
        with sym.Engine(mode=sym.MODE_PLANE, fixed_iters=1, host_loop=host_loop, **kw) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], None)
            res[host_loop] = (e.align(), e.stats())
    (rh, sh), (rd, sd) = res[1], res[0]
    assert rh["status"] == rd["status"] == 0
    assert rh["iters"] == rd["iters"] == kw["max_iters"]
    n = rh["iters"]
    assert np.allclose(rh["diffs"][:n], rd["diffs"][:n], rtol=2e-6, atol=1e-6), (rh["diffs"][:n], rd["diffs"][:n])
    assert np.abs(rh["transform"] - rd["transform"]).max() < 1e-6 * max(1.0, float(np.abs(rh["transform"]).max()))
    assert sh["loop_passes"] == 0 and sd["loop_passes"] > 0
    assert sd["passes"] == sh["passes"]


# ---- 4. power-of-two units ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-8, 8])
def test_power_of_two_units_run_the_same_passes(sym, cat15, k):
    s = np.float32(2.0 ** k)
    d = cat15
    ds = dict(src=d["src"] * s, tgt=d["tgt"] * s, tgt_n=d["tgt_n"])
    out = []
    for dd in (d, ds):
        with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, host_loop=1) as e:
            e.set_target(dd["tgt"], dd["tgt_n"])
            e.set_source(dd["src"], None)
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
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30) as e:      # and the device loop
        e.set_target(ds["tgt"], ds["tgt_n"])
        e.set_source(ds["src"], None)
        r = e.align()
        assert r["status"] == 0, r["error"]


# ---- 5. convergence ---------------------------------------------------------------------------------------------------------
def test_converges_on_the_cat_pair(sym, cat):
    """from the truth Rz(45 deg) + 2.5 x perturbed by 10 degrees and 10 % of the extent"""
    from symmicp import synth
    src, tgt = cat["src"], cat["tgt"]
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    T = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    ext = float(np.linalg.norm(src.max(0) - src.min(0)))
    cen = src.astype(np.float64).mean(0)
    R = synth.rotation(10.0, (0.3, 0.5, 0.8))
    D = synth.rigid4(R, cen - R @ cen + 0.1 * ext * np.array([0.6, -0.64, 0.48]))
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=60, fixed_iters=1) as e:
        e.set_target(tgt, cat["tgt_n"])
        e.set_source(src, None)
        r = e.align((D @ T).astype(np.float32))
    assert r["status"] == 0, r["error"]
    assert np.abs(r["transform"] - T).max() < 1e-4, r["transform"]


def test_converges_on_the_c4_pair(sym, c4):
    """the synthetic surface pair from the identity: within 1e-4 of the generating motion (3 degrees + a translation)"""
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=40, fixed_iters=1) as e:
        e.set_target(c4["tgt"], c4["tgt_n"])
        e.set_source(c4["src"], None)
        r = e.align()
    assert r["status"] == 0, r["error"]
    ang, dt = rot_err(r["transform"], c4["truth"])
    assert ang < 1e-4 and dt < 1e-4, (ang, dt)


# ---- 6. sharding by external exchange -----------------------------------------------------------------------------------------
def test_external_exchange_two_shards(sym, c4):
    d = c4
    kw = dict(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30)
    with sym.Engine(**kw) as ref:
        ref.set_target(d["tgt"], d["tgt_n"])
        ref.set_source(d["src"], None)
        rec_ref = np.asarray(ref.begin()["sums"], np.float64)
        T_ref = []
        for _ in range(4):
            ref.step()
            T_ref.append(ref.transform())
    engs = [sym.Engine(**kw) for _ in range(2)]
    try:
        for r, e in enumerate(engs):
            e.comm_init_rank(2, r, None)
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], None)
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


# ---- 7. the command-line driver ------------------------------------------------------------------------------------------------
def test_driver_mode_plane(sym, cat, tmp_path):
    import shutil
    import subprocess
    from conftest import ROOT, GOLDEN
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    shutil.copy(os.path.join(GOLDEN, "cat.pcd"), tmp_path / "cat.pcd")
    shutil.copy(os.path.join(GOLDEN, "cat_out.pcd"), tmp_path / "cat_out.pcd")
    r = subprocess.run([exe, "--mode", "plane", "--corr", "tree", "cat.pcd", "cat_out.pcd"], cwd=tmp_path, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    # the library's own PLANE result: target normals from the same GPU k-NN PCA the class uses, none for the source
    tn, _ = sym.estimate_normals(cat["tgt"], 10)
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE) as e:
        e.set_target(cat["tgt"], tn)
        e.set_source(cat["src"], None)
        rp = e.align()
    assert rp["status"] == 0
    block = sym.format_result(rp["transform"])
    assert block in r.stdout, (block, r.stdout[-600:])
    # the Python class takes the same path: no source normals estimated
    m = sym.MyICP(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, verbose=False)
    m.setInputSource(cat["src"])
    m.setInputTarget(cat["tgt"])
    res = m.align()
    assert m.normals_src is None and res["status"] == 0
    assert np.array_equal(res["transform"], rp["transform"])
