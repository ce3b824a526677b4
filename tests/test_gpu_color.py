"""GPU tests of colored ICP (SYMMICP_MODE_COLOR, run with -m gpu on a real MI355X).

  * the intensity gradient against its fp64 restatement (_color_ref.gradient, fed the neighbour sets of symmicp.knn): per point
    |g_dev - fl32(g_ref)|_inf <= 2^-22 |g_ref|_inf, degenerate rows exactly 0, the context untouched;
  * every pass of begin + 5 steps against the numpy COLOR record (_color_ref.color_record) and the oracle's brute-force nearest
    neighbours: IDENTITY, BRUTE and TREE, with and without Huber, max_corr_dist, min_normal_dot and a trim fraction of 0.6, on the
    textured ridge pair and on a ragged pair -- at test_gpu_plane.py's bars for PLANE's record: 1e-9 of a slot's term magnitudes
    unweighted, 1e-6 with a robust loss, the pair count exactly;
  * lambda = 1 gives a PLANE context's record bit for bit, lambda = 0 the photometric rows alone;
  * intensities and a colour weight set on a PLANE, PAPER or GICP context change no bit of its align;
  * the refusals; determinism; and the end-to-end run (TREE, 30 fixed iterations, lambda = 0.968, the gradient from the device)
    through Engine, symmicp.MyICP, tests/cpp/myicp_color.cpp and icp_align on PCD files with an rgb field: rms distance from the
    truth <= 0.05 sample spacings (20 x the fp64 reference loop's 0.00251; the start is 9.0), every solve's rcond >= 1e-3.

Measured on the MI355X (ridge pair, 20 000 points): see DESIGN.md 4, "Colored ICP"."""
import os
import subprocess

import numpy as np
import pytest

import _color_ref as CR
import _record_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32
BOUND = 0.05           # spacings: 20 x the fp64 reference loop's 0.00251 (fp32 rows, rgb quantisation to 1/765)
RCOND_MIN = 1e-3       # the reference's smallest rcond is 0.081


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def _with_gradient(sym, d):
    d = dict(d)
    d["tgt_g"] = sym.intensity_gradient(d["tgt"], d["tgt_n"], d["tgt_i"], 10)
    return d


@pytest.fixture(scope="module")
def ridge(sym):
    from symmicp import synth
    return _with_gradient(sym, synth.ridge_textured())


@pytest.fixture(scope="module")
def ragged(sym):
    """n_s != n_t, neither a multiple of 4: two cuts of a smaller ridge pair"""
    from symmicp import synth
    d = synth.ridge_textured(6001, seed=0xD1)
    d = dict(d, src=d["src"][:5003], src_n=d["src_n"][:5003], src_i=d["src_i"][:5003])
    return _with_gradient(sym, d)


def _identity_twin(sym, d, n=None):
    """a pair identity pairing makes sense on: the target is the source's own sampling under the true motion (row i <-> row i)"""
    n = len(d["src"]) if n is None else n
    T = d["truth"]
    src = d["src"][:n].astype(np.float64)
    e = dict(d, src=d["src"][:n], src_n=d["src_n"][:n], src_i=d["src_i"][:n], tgt=(src @ T[:3, :3].T + T[:3, 3]).astype(f32),
             tgt_n=(d["src_n"][:n].astype(np.float64) @ T[:3, :3].T).astype(f32), tgt_i=d["src_i"][:n].copy())
    return _with_gradient(sym, e)


def _corr(sym, name):
    return {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[name]


def _engine(sym, d, corr, mode=None, lam=None, **kw):
    e = sym.Engine(mode=sym.MODE_COLOR if mode is None else mode, corr=_corr(sym, corr), max_iters=30, **kw)
    e.set_target(d["tgt"], d["tgt_n"])
    e.set_source(d["src"], d["src_n"])
    e.set_target_intensity(d["tgt_i"], d["tgt_g"])
    e.set_source_intensity(d["src_i"])
    if lam is not None:
        e.set_color_weight(lam)
    return e


def assert_record(gpu, ref, mag, weighted, tag=""):
    """test_gpu_plane.py's comparison of PLANE's record, taken over unchanged"""
    gpu = np.asarray(gpu, np.float64)
    tol = 1e-6 if weighted else 1e-9
    err = np.abs(gpu[:37] - ref[:37])
    bad = np.nonzero(err > tol * np.maximum(mag[:37], 1e-300))[0]
    assert bad.size == 0, (tag, [(int(k), gpu[k], ref[k], mag[k]) for k in bad[:6]])
    assert gpu[37] == ref[37], (tag, gpu[37], ref[37])           # the pair count, exactly


# ---- 1. the gradient ---------------------------------------------------------------------------------------------------------
def _degenerate_cloud():
    """a flat patch with exact duplicates (rows 0..39 repeated), a collinear run far from everything else, twelve copies of one
    point, and a zero normal (on a flat neighbourhood nothing stands in for the normal direction: A is singular)"""
    rng = np.random.default_rng(5)
    n = 1500
    xy = rng.uniform(size=(n, 2))
    x = np.concatenate([xy, np.zeros((n, 1))], 1)
    x[40:80] = x[0:40]                                            # duplicates: twins at d2 == 0
    x[100:140] = np.stack([5.0 + 0.01 * np.arange(40), np.full(40, 5.0), np.full(40, 5.0)], 1)      # collinear, isolated
    x[200:212] = x[200]                                           # 12 copies of one point: a neighbourhood of duplicates only
    nrm = np.zeros((n, 3))
    nrm[:, 2] = 1.0
    nrm[300] = 0.0                                                # a zero normal
    it = 0.5 + 0.3 * np.sin(7 * x[:, 0]) * np.cos(5 * x[:, 1])
    return x.astype(f32), nrm.astype(f32), it.astype(f32)


def _check_gradient(sym, xyz, nrm, it, k, tag):
    rows, _ = sym.knn(xyz, k)
    g_ref, degenerate = CR.gradient(xyz, nrm, it, rows)
    g = sym.intensity_gradient(xyz, nrm, it, k)
    assert g.dtype == np.float32 and g.shape == (len(xyz), 3)
    assert np.all(g[degenerate] == 0.0), tag
    err = np.abs(g.astype(np.float64) - g_ref.astype(f32).astype(np.float64)).max(1)
    bar = 2.0 ** -22 * np.abs(g_ref).max(1)
    worst = float((err / np.maximum(bar, 1e-300))[~degenerate].max()) if (~degenerate).any() else 0.0
    print("gradient %s k=%d: %d points, %d degenerate, worst error / bar %.3g, exact bits on %d" % (
        tag, k, len(xyz), int(degenerate.sum()), worst, int((g == g_ref.astype(f32)).all(1).sum())))
    assert np.all(err <= bar), (tag, int((err > bar).sum()), worst)
    return g, degenerate


def test_gradient_matches_the_reference(sym, ridge, cat):
    g, deg = _check_gradient(sym, ridge["tgt"], ridge["tgt_n"], ridge["tgt_i"], 10, "ridge target")
    assert deg.sum() == 0 and np.array_equal(g, ridge["tgt_g"])
    rng = np.random.default_rng(3)
    _check_gradient(sym, cat["src"], cat["src_n"], (0.5 + 0.01 * cat["src"][:, 0] + 0.1 * rng.uniform(size=len(cat["src"]))).astype(f32), 10, "cat")
    _check_gradient(sym, cat["src"], cat["src_n"], cat["src"][:, 1].copy(), 16, "cat k=16")
    x, n, it = _degenerate_cloud()
    for k in (3, 10):
        g, deg = _check_gradient(sym, x, n, it, k, "degenerate cloud")
        assert deg[100:140].all() and deg[300] and deg[200:212].all(), k       # collinear, zero normal, duplicates only
        assert not deg[400:].all()


def test_gradient_leaves_the_context_untouched(sym, ridge, cat):
    d = ridge
    with _engine(sym, d, "tree", fixed_iters=1) as e:
        e.set_config(max_iters=8)
        r1 = e.align()
        idx1, d21 = e.correspondences()
        g = e.intensity_gradient(cat["src"], cat["src_n"], cat["src"][:, 2].copy(), 10)
        assert np.array_equal(g, sym.intensity_gradient(cat["src"], cat["src_n"], cat["src"][:, 2].copy(), 10))
        assert np.array_equal(e.intensity_gradient(d["tgt"], d["tgt_n"], d["tgt_i"], 10), d["tgt_g"])
        assert np.array_equal(e.source_intensity(), d["src_i"])              # read back in the caller's row order
        r2 = e.align()
        idx2, d22 = e.correspondences()
    assert r1["status"] == r2["status"] == 0 and r1["iters"] == r2["iters"] == 8
    assert np.array_equal(r1["transform"], r2["transform"]) and np.array_equal(r1["diffs"], r2["diffs"])
    assert np.array_equal(idx1, idx2) and np.array_equal(d21, d22)


# ---- 2. records ----------------------------------------------------------------------------------------------------------------
VARIANTS = {
    "plain": dict(),
    "huber": dict(loss="huber"),
    "gates": dict(gates=True),
    "trim": dict(trim=0.6),
    "all": dict(loss="huber", gates=True, trim=0.6),
}
HUBER_SCALE = 2e-3        # of r = sqrt(lam c_G^2 + om c_C^2): between the converged and the starting residuals of the ridge pairs


def _check_pass(sym, oracle, e, it, d, corr, v, lam, tag, first):
    X = e.transform()
    p, pn = oracle.apply(X, d["src"], True), oracle.apply(X, d["src_n"], False)
    idx, d2 = e.correspondences()
    if corr == "identity":
        pairs = np.arange(len(p), dtype=np.int64)
    else:
        pairs, rd = oracle.nn_brute(p, d["tgt"])
    loss = sym.loss_code(v.get("loss", "none"))
    max_d2 = R.f32_max_d2(v["max_dist"]) if v.get("gates") else 0.0
    min_ndot = v["min_ndot"] if v.get("gates") else -2.0
    S, M, kept = CR.color_record(p, pn, d["src_i"], d["tgt"], d["tgt_n"], d["tgt_g"], d["tgt_i"], pairs, e.pivot(), lam, loss, HUBER_SCALE,
                                 max_d2, min_ndot, v.get("trim", 1.0))
    if corr != "identity":
        # correspondences are the exact nearest neighbours; after a trimmed pass the rows that were no candidate or were trimmed
        # away report -1 (symmicp_get_correspondences)
        want = np.where(kept, pairs, -1) if "trim" in v else pairs
        assert np.array_equal(idx, want), (tag, int((idx != want).sum()))
        assert np.array_equal(d2[idx >= 0], rd[idx >= 0]), tag
    if first and (v.get("gates") or "trim" in v):
        assert 0 < kept.sum() < len(kept), tag                    # the gates / the trim bite
    if first and loss:
        w = CR.color_terms(p[kept], d["tgt"][pairs[kept]], d["tgt_n"][pairs[kept]], d["tgt_g"][pairs[kept]], d["tgt_i"][pairs[kept]],
                           d["src_i"][kept], e.pivot(), lam, loss, HUBER_SCALE)[0][:, 34]
        assert w.sum() < 0.95 * len(w), tag                       # the weights bite
    assert_record(it["sums"], S, M, loss != 0, tag)
    assert it["pairs"] == kept.sum(), tag


def _run_record_matrix(sym, oracle, d, corr, variant, lam=CR.LAMBDA_DEFAULT):
    v = dict(VARIANTS[variant])
    kw = {}
    if v.get("gates"):
        # bounds that drop a part of the starting pairs: the median pair distance of the first pass, and a normal gate just inside
        # the 3 degrees the clouds start apart
        p0 = d["src"]
        j = np.arange(len(p0)) if corr == "identity" else oracle.nn_brute(p0, d["tgt"])[0]
        v["max_dist"] = float(np.sqrt(np.median(R.dist2(p0, d["tgt"][j]).astype(np.float64))))
        v["min_ndot"] = float(np.median(R.ndot(d["src_n"], d["tgt_n"][j])))
        kw = dict(max_corr_dist=v["max_dist"], min_normal_dot=v["min_ndot"])
    with _engine(sym, d, corr, lam=lam, host_loop=1, **kw) as e:
        if "loss" in v:
            e.set_robust_loss(v["loss"], HUBER_SCALE)
        if "trim" in v:
            e.set_trim_fraction(v["trim"])
        it = e.begin()
        _check_pass(sym, oracle, e, it, d, corr, v, lam, "%s %s begin" % (corr, variant), True)
        for k in range(5):
            it = e.step()
            _check_pass(sym, oracle, e, it, d, corr, v, lam, "%s %s step %d" % (corr, variant, k + 1), False)
        st = e.stats()
        nrm_read = 0 if kw.get("min_normal_dot", -2.0) <= -1.0 else 12
        base = 36 + nrm_read if corr == "identity" else 44 + nrm_read
        extra = 0 if corr == "identity" else 12 * len(d["tgt"])
        assert st["bytes_algorithmic_per_pass"] == len(d["src"]) * (base + 20) + extra      # + 4 B intensity per point, 16 B per pair


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_passes_match_the_numpy_record_on_the_ridge_pair(sym, oracle, ridge, corr, variant):
    _run_record_matrix(sym, oracle, ridge, corr, variant)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_identity_passes_match_the_numpy_record(sym, oracle, ridge, variant):
    """identity pairing on the source's own sampling under the true motion: 20 000 rows (16-byte column loads) and 4 999 (the general form)"""
    _run_record_matrix(sym, oracle, _identity_twin(sym, ridge), "identity", variant)
    _run_record_matrix(sym, oracle, _identity_twin(sym, ridge, 4999), "identity", variant)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_passes_match_the_numpy_record_on_a_ragged_pair(sym, oracle, ragged, corr, variant):
    assert len(ragged["src"]) % 4 and len(ragged["tgt"]) % 4 and len(ragged["src"]) != len(ragged["tgt"])
    _run_record_matrix(sym, oracle, ragged, corr, variant)


# ---- 3. lambda = 1 and lambda = 0 ----------------------------------------------------------------------------------------------
def _cat_colored(sym, cat):
    from symmicp import synth
    d = synth.perturbed(cat["src"], cat["src_n"])
    rng = np.random.default_rng(11)
    d["src_i"] = rng.uniform(size=len(d["src"])).astype(f32)
    d["tgt_i"] = rng.uniform(size=len(d["tgt"])).astype(f32)
    d["tgt_g"] = rng.normal(size=d["tgt"].shape).astype(f32)
    return d


@pytest.mark.parametrize("loss", ["none", "huber"])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_lambda_1_is_planes_record_bit_for_bit(sym, cat, ridge, corr, loss):
    for d, scale in ((_cat_colored(sym, cat), 1.0), (ridge if corr != "identity" else _identity_twin(sym, ridge), HUBER_SCALE)):
        recs = []
        for mode, lam in ((sym.MODE_PLANE, None), (sym.MODE_COLOR, 1.0)):
            with _engine(sym, d, corr, mode=mode, lam=lam, host_loop=1, max_corr_dist=float(np.abs(d["tgt"]).max()) * 0.5,
                         min_normal_dot=-0.5) as e:
                if loss != "none":
                    e.set_robust_loss(loss, scale)
                e.set_trim_fraction(0.9)
                out = [e.begin()]
                for _ in range(5):
                    out.append(e.step(check=False))
                recs.append((np.array([o["sums"] for o in out]), [o["status"] for o in out], e.transform().copy()))
        assert recs[0][1] == recs[1][1]
        assert np.array_equal(recs[0][0], recs[1][0]) and np.array_equal(recs[0][2], recs[1][2])
        assert np.isfinite(recs[0][0]).all()


@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_lambda_0_leaves_the_photometric_rows_alone(sym, oracle, ridge, corr):
    d = ridge if corr != "identity" else _identity_twin(sym, ridge)
    _run_record_matrix(sym, oracle, d, corr, "plain", lam=0.0)
    # ... and the target's normals do not enter slots 0..26 (no normal gate is set): other normals, the same bits there
    other = dict(d, tgt_n=np.roll(d["tgt_n"], 1, axis=1).copy())
    recs = []
    for dd in (d, other):
        with _engine(sym, dd, corr, lam=0.0, host_loop=1) as e:
            recs.append(e.begin()["sums"])
    assert np.array_equal(recs[0][:27], recs[1][:27]) and np.array_equal(recs[0][27:37], recs[1][27:37])
    with _engine(sym, other, corr, lam=0.5, host_loop=1) as e:
        assert not np.array_equal(e.begin()["sums"][:27], recs[0][:27])


# ---- 4. off means off ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["PLANE", "PAPER", "GICP"])
def test_attributes_change_no_bit_of_the_other_modes(sym, cat, mode):
    d = _cat_colored(sym, cat)
    out = []
    for colored in (False, True):
        with sym.Engine(mode=getattr(sym, "MODE_" + mode), corr=sym.CORR_TREE, max_iters=30) as e:
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            if colored:
                e.set_target_intensity(d["tgt_i"], d["tgt_g"])
                e.set_source_intensity(d["src_i"])
                e.set_color_weight(0.3)
                assert abs(e.color_weight() - 0.3) < 1e-7
            r = e.align()
            out.append((r, e.begin()["sums"], e.stats()["loop_passes"]))
    (r0, s0, l0), (r1, s1, l1) = out
    assert r0["status"] == r1["status"] == 0 and r0["iters"] == r1["iters"] and l0 == l1
    assert np.array_equal(r0["transform"], r1["transform"]) and np.array_equal(r0["diffs"], r1["diffs"]) and np.array_equal(s0, s1)


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------
def _status(sym, fn, *a, **kw):
    with pytest.raises(sym.SymmIcpError) as x:
        fn(*a, **kw)
    return x.value.status


def test_refusals(sym, ridge):
    d = ridge
    n = len(d["src"])
    with sym.Engine(mode=sym.MODE_COLOR, corr=sym.CORR_TREE, max_iters=5) as e:
        assert abs(e.color_weight() - 0.968) < 1e-7                          # the default
        # the attributes follow their clouds
        assert _status(sym, e.set_source_intensity, d["src_i"]) == sym.ERR_STATE
        assert _status(sym, e.set_target_intensity, d["tgt_i"], d["tgt_g"]) == sym.ERR_STATE
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        assert _status(sym, e.begin) == sym.ERR_STATE                        # no attribute at all
        assert e.align()["status"] == sym.ERR_STATE
        e.set_source_intensity(d["src_i"])
        assert _status(sym, e.begin) == sym.ERR_STATE                        # the target's is missing
        # wrong n, non-finite values, NULL
        assert _status(sym, e.set_source_intensity, d["src_i"][:-1]) == sym.ERR_SIZE
        assert _status(sym, e.set_target_intensity, d["tgt_i"][:-1], d["tgt_g"][:-1]) == sym.ERR_SIZE
        bad = d["src_i"].copy()
        bad[n // 2] = np.nan
        assert _status(sym, e.set_source_intensity, bad) == sym.ERR_ARG
        bad[n // 2] = np.inf
        assert _status(sym, e.set_target_intensity, bad, d["tgt_g"]) == sym.ERR_ARG
        badg = d["tgt_g"].copy()
        badg[7, 1] = np.nan
        assert _status(sym, e.set_target_intensity, d["tgt_i"], badg) == sym.ERR_ARG
        L = sym.lib()
        assert L.symmicp_set_source_intensity(e._h, None, 1, n) == sym.ERR_ARG
        assert L.symmicp_set_target_intensity(e._h, sym._fptr(d["tgt_i"]), 1, None, 3, 1, n) == sym.ERR_ARG      # grad is required
        # (the source's attribute survived the refused calls)
        e.set_target_intensity(d["tgt_i"], d["tgt_g"])
        assert e.begin()["status"] == 0
        # lambda outside [0, 1]: refused, the old value stays
        e.set_color_weight(0.75)
        for lam in (-0.01, 1.01, float("nan"), float("inf")):
            assert _status(sym, e.set_color_weight, lam) == sym.ERR_ARG
            assert e.color_weight() == 0.75
        for lam in (0.0, 1.0):
            e.set_color_weight(lam)
        # a new cloud drops its attribute
        e.set_source(d["src"], d["src_n"])
        assert _status(sym, e.begin) == sym.ERR_STATE
        e.set_source_intensity(d["src_i"])
        e.begin()
        e.set_target(d["tgt"], d["tgt_n"])
        assert _status(sym, e.begin) == sym.ERR_STATE
        # source normals stay required (nrm == NULL is PLANE-only)
        assert _status(sym, e.set_source, d["src"], None) == sym.ERR_ARG
    # sharding: a COLOR context takes no communicator of more than one rank, a sharded context no COLOR config
    with sym.Engine(mode=sym.MODE_COLOR, corr=sym.CORR_TREE) as e:
        assert _status(sym, e.comm_init_rank, 2, 0, None) == sym.ERR_STATE
        assert _status(sym, e.comm_init_shm, 2, 0, "symmicp_color_test") == sym.ERR_STATE
        assert "COLOR" in e._L.symmicp_last_error(e._h).decode()
        e.comm_init_rank(1, 0, None)                                         # one rank is no sharding
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE) as e:
        e.comm_init_rank(2, 0, None)                                         # external exchange: sharded
        assert _status(sym, e.set_config, mode=sym.MODE_COLOR) == sym.ERR_STATE
    with pytest.raises(sym.SymmIcpError) as x:
        sym.Engine(mode=6)
    assert x.value.status == sym.ERR_ARG
    # voxel levels
    m = sym.MyICP(mode=sym.MODE_COLOR, corr=sym.CORR_TREE, verbose=False)
    assert _status(sym, m.setVoxelLevels, [(0.05, 5, 0.0)]) == sym.ERR_ARG
    m._levels = [(0.05, 5, 0.0)]
    m.setInputSource(d["src"], d["src_n"], d["src_i"])
    m.setInputTarget(d["tgt"], d["tgt_n"], d["tgt_i"])
    assert _status(sym, m.align) == sym.ERR_ARG


# ---- 6. end to end -----------------------------------------------------------------------------------------------------------------
def _engine_run(sym, d, lam=CR.LAMBDA_DEFAULT):
    """30 fixed iterations through begin / step: -> (4x4, smallest rcond of the 30 solves)"""
    with _engine(sym, d, "tree", lam=lam, fixed_iters=1) as e:
        e.begin()
        rc = [e.step()["rcond"] for _ in range(30)]
        return e.transform().copy(), float(min(rc))


def test_end_to_end_engine_and_determinism(sym, ridge):
    d = ridge
    assert abs(CR.rms_spacings(np.eye(4), d) - 9.0) < 0.01
    X, rc = _engine_run(sym, d)
    rms = CR.rms_spacings(X, d)
    print("Engine COLOR: %.5f spacings from the truth, smallest rcond %.3g" % (rms, rc))
    # what PLANE does on this pair is not asserted
    with _engine(sym, d, "tree", mode=sym.MODE_PLANE, fixed_iters=1) as e:
        r = e.align()
        print("Engine PLANE on the same pair: status %d after %d iterations, %.3f spacings from the truth" % (
            r["status"], r["iters"], CR.rms_spacings(r["transform"], d)))
    assert rms <= BOUND, rms
    assert rc >= RCOND_MIN, rc
    # symmicp_align runs the same host loop: the same bits, twice, and no pass inside a device-driven run
    for _ in range(2):
        with _engine(sym, d, "tree", fixed_iters=1) as e:
            r = e.align()
            assert r["status"] == 0 and r["iters"] == 30
            assert np.array_equal(r["transform"], X)
            assert e.stats()["loop_passes"] == 0
    X2, rc2 = _engine_run(sym, d)
    assert np.array_equal(X, X2) and rc == rc2


def test_end_to_end_python_myicp(sym, ridge):
    d = ridge
    m = sym.MyICP(mode=sym.MODE_COLOR, corr=sym.CORR_TREE, max_iters=30, verbose=False, fixed_iters=1)
    m.setInputSource(d["src"], d["src_n"], d["src_i"])
    m.setInputTarget(d["tgt"], d["tgt_n"], d["tgt_i"])
    r = m.align()
    assert r["status"] == 0 and r["iters"] == 30
    rms = CR.rms_spacings(m.getFinalTransformation(), d)
    X, rc = _engine_run(sym, d)
    print("symmicp.MyICP COLOR: %.5f spacings, rcond %.3g (the Engine run's bits: %s)" % (rms, rc, np.array_equal(X, r["transform"])))
    assert rms <= BOUND, rms
    assert np.array_equal(X, r["transform"]) and rc >= RCOND_MIN          # the same run as the Engine's, whose solves are checked
    m.setColorWeight(0.5)
    r5 = m.align()
    rms5 = CR.rms_spacings(r5["transform"], d)
    print("symmicp.MyICP COLOR, lambda 0.5: %.5f spacings" % rms5)
    assert r5["status"] == 0 and rms5 <= BOUND and not np.array_equal(r5["transform"], r["transform"])


def test_end_to_end_cpp_myicp(sym, ridge, tmp_path):
    d = ridge
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_color")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for name in ("src", "src_n", "tgt", "tgt_n", "src_i", "tgt_i"):
        np.ascontiguousarray(d[name], f32).tofile(tmp_path / (name + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    X = np.fromfile(tmp_path / "out_color.f32", f32).reshape(4, 4)
    Xh = np.fromfile(tmp_path / "out_half.f32", f32).reshape(4, 4)
    rms, rmsh = CR.rms_spacings(X, d), CR.rms_spacings(Xh, d)
    Xe, rc = _engine_run(sym, d)
    print("C++ MyICP COLOR: %.5f spacings (lambda 0.5: %.5f), rcond %.3g (the Engine run's bits: %s)" % (rms, rmsh, rc, np.array_equal(X, Xe)))
    assert rms <= BOUND and rmsh <= BOUND, (rms, rmsh)
    assert np.array_equal(X, Xe) and rc >= RCOND_MIN


def _write_rgb_pcd(path, xyz, intensity):
    words = CR.rgb_pack(intensity)
    with open(path, "w") as f:
        f.write("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS x y z rgb\nSIZE 4 4 4 4\nTYPE F F F U\nCOUNT 1 1 1 1\n"
                "WIDTH %d\nHEIGHT 1\nVIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA ascii\n" % (len(xyz), len(xyz)))
        for (x, y, z), w in zip(xyz, words):
            f.write("%.9g %.9g %.9g %d\n" % (x, y, z, w))
    return CR.rgb_intensity(words)


def test_end_to_end_driver_on_rgb_files(sym, ridge, tmp_path):
    d = ridge
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    si = _write_rgb_pcd(tmp_path / "a.pcd", d["src"], d["src_i"])
    ti = _write_rgb_pcd(tmp_path / "b.pcd", d["tgt"], d["tgt_i"])
    got, kind = sym.pcd_read_intensity(str(tmp_path / "a.pcd"))
    assert kind == 2 and np.array_equal(got, si) and np.abs(si - d["src_i"]).max() <= 0.5 / 255 + 1e-6
    args = ["--mode", "color", "--corr", "tree", "--iters", "30", "--threshold", "0"]      # (not --quiet: the Result block is read)
    r = subprocess.run([exe] + args + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    out = r.stdout.split("\n")
    k = out.index("Result transform:")
    X = np.array([[float(v) for v in out[k + 1 + i].split()] for i in range(4)])
    rms = CR.rms_spacings(X, d)
    # the same run through the Engine: the driver's own k = 10 normals (both clouds), the files' quantised intensities
    sn, _ = sym.estimate_normals(d["src"], 10)
    tn, _ = sym.estimate_normals(d["tgt"], 10)
    de = dict(d, src_n=sn, tgt_n=tn, src_i=si, tgt_i=ti)
    de["tgt_g"] = sym.intensity_gradient(de["tgt"], tn, ti, 10)
    Xe, rc = _engine_run(sym, de)
    Tref, rcref = CR.color_icp_fp64(de, de["tgt_g"], iters=30, tgt_n=tn, src_i=si, tgt_i=ti)
    print("icp_align --mode color: %.5f spacings; the Engine on its inputs %.5f, rcond %.3g; the fp64 loop on them %.5f, rcond %.3g" % (
        rms, CR.rms_spacings(Xe, d), rc, CR.rms_spacings(Tref, d), rcref))
    assert np.abs(X - Xe).max() < 2e-5, np.abs(X - Xe).max()                 # (the block prints 6 significant digits)
    assert rc >= RCOND_MIN
    assert rms <= BOUND, rms
    # the driver's argument rules
    sym.pcd_write(str(tmp_path / "plain.pcd"), d["src"][:100])
    r = subprocess.run([exe] + args + ["plain.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == sym.ERR_STATE and "colours in both files" in r.stderr
    for bad in (["--color-weight", "1.5"], ["--color-weight", "-1"], ["--color-weight", "x"], ["--scale", "0.05:5"]):
        assert subprocess.run([exe] + args + bad + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True).returncode == 64, bad
    assert subprocess.run([exe, "--mode", "plane", "--color-weight", "0.5", "a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True).returncode == 64
    r = subprocess.run([exe] + args + ["--color-weight", "0.5", "a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
