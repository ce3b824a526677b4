"""GPU Fast Global Registration (symmicp_ctx_fgr, symmicp_ctx_fgr_pass; kernels_fgr.hip) against tests/_fgr_ref.py: the tuple test
bit for bit, one pass's record and weights at every kernel-shape edge, the loop from the device's own trace (schedule, records, chain),
purity, the result against the fp64 method and the truth, degenerate inputs, and the composition in MyICP (Python and C++) and the
driver."""
import os
import subprocess

import numpy as np
import pytest

import _fgr_ref as R
import _global_ref as G
import _record_ref as RR
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
CAT_R = 11.05
CAT_DIST = CAT_R / 4
RESIDENT = 4096           # kFgrResident: the largest set k_fgr_optimize keeps on chip (in LDS); above it every pass streams
OUT16_ULPS = 32           # tests/test_gpu_batch.py's rule for X_{k+1} against the host solve of the device's own record
WEIGHT_ULPS = 4           # l = t t, t = mu / (mu + r2): a division off by one ulp, doubled by the square, plus the square's rounding
E2E_BOUND = 1e-4          # tests/test_gpu_global.py: the project's own bound on a 4x4, both runs reach the same fixed point


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        yield e


def cat_truth():
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    return np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


@pytest.fixture(scope="module")
def catf(eng, cat):
    """the cat pair with its golden normals and the device's own FPFH matches"""
    fs, ft = eng.fpfh(cat["src"], cat["src_n"], CAT_R), eng.fpfh(cat["tgt"], cat["tgt_n"], CAT_R)
    pairs, _ = eng.feature_correspondences(fs, ft)
    return dict(src=cat["src"], tgt=cat["tgt"], pairs=pairs, truth=cat_truth(), max_dist=CAT_DIST, spacing=1.0)


def _bumps(eng, shift=None):
    b = G.bumps_pair(shift=shift)
    fs, ft = eng.fpfh(b["src"], b["src_n"], b["radius"]), eng.fpfh(b["tgt"], b["tgt_n"], b["radius"])
    b["pairs"], _ = eng.feature_correspondences(fs, ft)
    return b


@pytest.fixture(scope="module")
def bumps(eng):
    return _bumps(eng)


@pytest.fixture(scope="module")
def bumps_shifted(eng):
    return _bumps(eng, shift=(1e4, 1e4, 1e4))


# ---- 1. the tuple test, bit for bit ---------------------------------------------------------------------------------------------------
def check_tuples(sym, eng, src, tgt, pairs, max_dist, **kw):
    p, q, _, _ = G.pivoted(src, tgt, pairs)
    want, accepted = R.tuple_set(p, q, kw.get("seed", 0), kw.get("tuple_scale", 0.95), kw.get("max_tuples", 1000), kw.get("tuple_trials", 0))
    r = eng.fgr(src, tgt, pairs, max_dist, iterations=1, check=False, **kw)
    assert r["tuples_accepted"] == accepted, (kw, r["tuples_accepted"], accepted)
    if accepted == 0:
        assert r["status"] == sym.ERR_NO_CONSENSUS and r["set_size"] == 0 and np.array_equal(r["transform"], np.eye(4, dtype=F))
    else:
        assert r["status"] in (sym.OK, sym.ERR_DEGENERATE)
        assert r["set_size"] == len(want) and np.array_equal(r["set"], want), kw
    return r, accepted


def test_tuples_cat_truncated_and_bumps_not(sym, eng, catf, bumps):
    r, acc = check_tuples(sym, eng, catf["src"], catf["tgt"], catf["pairs"], CAT_DIST, seed=1)
    trials = R.default_trials(len(catf["pairs"]))
    print("cat: %d matches, %d of %d trials accepted, M = %d" % (len(catf["pairs"]), acc, trials, r["set_size"]))
    assert acc > 0.9 * trials and r["set_size"] == 3000
    r, acc = check_tuples(sym, eng, bumps["src"], bumps["tgt"], bumps["pairs"], bumps["max_dist"], seed=1)
    print("bumps: %d matches, %d trials accepted, M = %d" % (len(bumps["pairs"]), acc, r["set_size"]))
    assert 0 < acc < 1000 and r["set_size"] == 3 * acc


@pytest.mark.parametrize("kw", [dict(max_tuples=1), dict(max_tuples=7), dict(tuple_trials=1), dict(tuple_trials=255), dict(tuple_trials=256),
                                dict(tuple_trials=257), dict(tuple_trials=65537), dict(tuple_trials=4, seed=3)])
def test_tuples_sizes(sym, eng, catf, kw):
    check_tuples(sym, eng, catf["src"], catf["tgt"], catf["pairs"], CAT_DIST, **dict(dict(seed=2), **kw))


def test_tuples_small_and_extreme_inputs(sym, eng):
    rng = np.random.default_rng(3)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], F)
    ident = lambda n: np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    r, acc = check_tuples(sym, eng, tri, tri + F(0.25), ident(3), 0.1, seed=5)           # m = 3
    assert acc > 0
    # a translated copy: every trial with distinct draws is accepted
    src = rng.random((500, 3)).astype(F)
    tgt = src + np.array([0.5, -1.0, 2.0], F)
    r, acc = check_tuples(sym, eng, src, tgt, ident(500), 0.05, seed=6, tuple_trials=5000)
    c = R.tuple_draws(6, 5000, 500)
    assert acc == int(((c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 0] != c[:, 2])).sum())
    # tuple_scale = 1 on jittered points: no triangle is congruent to the last bit, nothing is accepted
    jit = tgt + (rng.random((500, 3)) * 1e-3).astype(F)
    r, acc = check_tuples(sym, eng, src, jit, ident(500), 0.05, seed=6, tuple_trials=5000, tuple_scale=1.0)
    assert acc == 0 and r["status"] == sym.ERR_NO_CONSENSUS
    with pytest.raises(sym.SymmIcpError) as e:
        eng.fgr(src, jit, ident(500), 0.05, seed=6, tuple_trials=5000, tuple_scale=1.0)
    assert e.value.status == sym.ERR_NO_CONSENSUS


# ---- 2. one pass at every kernel-shape edge -----------------------------------------------------------------------------------------
PASS_M = [1, 2, 3, 63, 64, 65, 1023, 1024, 1025, RESIDENT - 1, RESIDENT, RESIDENT + 1, 3000, 20000]


@pytest.fixture(scope="module")
def passin(catf):
    from symmicp import synth
    p, q, _, _ = G.pivoted(catf["src"], catf["tgt"], catf["pairs"])
    X = synth.rigid4(synth.rotation(30.0, (0.0, 0.0, 1.0)), np.array([1.0, -0.5, 0.25])).astype(F)
    return dict(p=p, q=q, X=X, D2=R.d2_max(p, q), d2=R.delta2(CAT_DIST))


def assert_weights(got, want, tag):
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert np.all(err <= WEIGHT_ULPS * np.spacing(np.abs(want)).astype(np.float64)), (tag, float(err.max()))


@pytest.mark.parametrize("which", ["D2", "d2"])
def test_pass_record_and_weights(eng, passin, which):
    mu = passin[which]
    m = len(passin["p"])
    for M in PASS_M:
        idx = (np.arange(M) * 7) % m                  # (any M from the cat's matches: rows repeat above m, as a set's do)
        p, q = passin["p"][idx], passin["q"][idx]
        S, w = eng.fgr_pass(p, q, passin["X"], mu)
        ref, mag, l = R.pass_record(p, q, passin["X"], mu)
        RR.assert_record(S, ref, mag, RR.TOL_REC, (which, M))
        assert S[37] == M and S[33] == 0 and S[38] == 0 and S[39] == 0
        assert_weights(w, l, (which, M))
        assert 0 < l.min() and l.max() <= 1


# ---- 3. the loop, from the device's own trace -----------------------------------------------------------------------------------------
def check_loop(sym, eng, d, **kw):
    src, tgt, pairs, md = d["src"], d["tgt"], d["pairs"], d["max_dist"]
    r = eng.fgr(src, tgt, pairs, md, want_trace=True, **kw)
    K = kw.get("iterations", 64)
    p, q, cs, ct = G.pivoted(src, tgt, pairs)
    assert r["iterations"] == K and r["X_trace"].shape == (K + 1, 4, 4)
    mus = R.schedule(R.d2_max(p, q), md, K, kw.get("decrease_every", 4), kw.get("division_factor", 1.4))
    assert np.array_equal(bits(r["mu_trace"]), bits(mus)) and bits(r["mu"]) == bits(mus[-1])
    ps, qs = p[r["set"]], q[r["set"]]
    assert np.array_equal(r["X_trace"][0], np.eye(4, dtype=F))
    for k in range(K):
        Xk = r["X_trace"][k]
        ref, mag, l = R.pass_record(ps, qs, Xk, mus[k])
        RR.assert_record(r["sums_trace"][k], ref, mag, RR.TOL_REC, (kw, k))
        st, pb, qb, a, t, rc, Xi = sym.solve(sym.MODE_PLANE, r["sums_trace"][k])
        assert st == sym.OK
        scale = 1.0 + float(np.abs(pb).sum() + np.abs(qb).sum() + np.abs(t).sum())
        Xk64 = Xk.astype(np.float64)
        bound = OUT16_ULPS * 2.0 ** -24 * scale * np.abs(Xk64).sum(0)[None, :] + 4 * 2.0 ** -24 * (np.abs(Xi.astype(np.float64)) @ np.abs(Xk64))
        err = np.abs(r["X_trace"][k + 1].astype(np.float64) - R.mat4_mul32(Xi, Xk).astype(np.float64))
        assert np.all(err <= bound), (kw, k, float(err.max()))
    assert_weights(r["weights"], l, kw)
    assert r["weight_sum"] == r["sums_trace"][K - 1][34]
    # the result: T = T(ct) X T(-cs) in fp64, its fp32 rounding, inliers and RMSE over all pairs
    T = R.compose(r["X_trace"][K], cs, ct)
    assert np.allclose(r["transform64"], T, rtol=1e-13, atol=1e-13) and np.array_equal(r["transform"], r["transform64"].astype(F))
    dd = src[pairs[:, 0]].astype(np.float64) @ r["transform64"][:3, :3].T + r["transform64"][:3, 3] - tgt[pairs[:, 1]]
    r2 = (dd * dd).sum(1)
    inl = r2 <= float(F(md)) ** 2
    edge = np.abs(r2 - float(F(md)) ** 2) < 1e-9 * float(F(md)) ** 2
    assert abs(r["inliers"] - int(inl.sum())) <= int(edge.sum())
    if not edge.any():
        assert r["rmse"] == pytest.approx(np.sqrt(r2[inl].mean()) if inl.any() else 0.0, rel=1e-12)      # (no inlier: 0)
    return r


@pytest.mark.parametrize("kw", [dict(iterations=1), dict(iterations=5, decrease_every=1), dict(),
                                dict(iterations=5, decrease_every=1, division_factor=1e9), dict(iterations=9, decrease_every=4, max_tuples=0)])
def test_loop_from_its_own_trace(sym, eng, bumps, kw):
    d = bumps
    if kw.get("division_factor", 0) > 1e6:
        # the floor in one step.  At the pair's own max_dist that leaves sum l < 6 at X_0 = I (every residual is far above delta: PLANE's
        # solve refuses the record, test_degenerate_inputs has that outcome); a delta of half the clouds' radius keeps the weights up
        p, q, _, _ = G.pivoted(d["src"], d["tgt"], d["pairs"])
        d = dict(bumps, max_dist=float(0.5 * np.sqrt(R.d2_max(p, q))))
    r = check_loop(sym, eng, d, seed=1, **kw)
    if kw.get("division_factor", 0) > 1e6:
        assert (r["mu_trace"] == R.delta2(d["max_dist"])).all()
    if kw.get("max_tuples", 1) == 0:
        assert r["set_size"] == len(bumps["pairs"]) and np.array_equal(r["set"], np.arange(len(bumps["pairs"])))


def test_loop_streamed_set(sym, eng, catf):
    """M = 6000 > the resident limit: every pass streams the set"""
    r = check_loop(sym, eng, catf, seed=1, iterations=6, decrease_every=2, max_tuples=2000)
    assert r["set_size"] == 6000 > RESIDENT


# ---- 4. purity --------------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes(eng, bumps):
    a = eng.fgr(bumps["src"], bumps["tgt"], bumps["pairs"], bumps["max_dist"], seed=2, want_trace=True)
    b = eng.fgr(bumps["src"], bumps["tgt"], bumps["pairs"], bumps["max_dist"], seed=2, want_trace=True)
    for k in ("transform", "transform64", "set", "weights", "X_trace", "sums_trace", "mu_trace"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["iterations"], a["inliers"], a["rmse"], a["weight_sum"], a["tuples_accepted"]) == \
        (b["iterations"], b["inliers"], b["rmse"], b["weight_sum"], b["tuples_accepted"])


def test_a_call_between_two_steps_leaves_the_context_alone(sym, cat, bumps):
    def steps(with_call):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=10) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            out = [e.begin(np.eye(4, dtype=F)), e.step()]
            if with_call:
                assert e.fgr(bumps["src"], bumps["tgt"], bumps["pairs"], bumps["max_dist"], seed=1, iterations=8)["iterations"] == 8
                e.fgr_pass(bumps["src"][:100], bumps["tgt"][:100], np.eye(4), 1.0)
            out += [e.step(), e.step()]
            return out, e.transform(), e.pivot(), e.correspondences()
    (a, Xa, pa, ca), (b, Xb, pb, cb) = steps(False), steps(True)
    for x, y in zip(a, b):
        assert x["sums"].tobytes() == y["sums"].tobytes() and x["increment"].tobytes() == y["increment"].tobytes()
        assert (x["status"], x["iter"], x["diff"], x["rcond"], x["pairs"]) == (y["status"], y["iter"], y["diff"], y["rcond"], y["pairs"])
    assert np.array_equal(Xa, Xb) and np.array_equal(pa, pb) and all(np.array_equal(u, v) for u, v in zip(ca, cb))


# ---- 5. against fp64 and the truth ----------------------------------------------------------------------------------------------------
def check_against_fp64_and_truth(eng, d, seed, name):
    r = eng.fgr(d["src"], d["tgt"], d["pairs"], d["max_dist"], seed=seed)
    ref = R.fgr64(d["src"], d["tgt"], d["pairs"], d["max_dist"], seed=seed)
    assert ref["status"] == R.OK and np.array_equal(r["set"], ref["set"]) and r["tuples_accepted"] == ref["accepted"]
    disp = R.displacement(r["transform64"], ref["T"], d["src"][d["pairs"][:, 0]]) / d["max_dist"]
    rot, rms = G.rotation_error_deg(r["transform"], d["truth"]), G.rms_to_truth(r["transform"], d["truth"], d["src"]) / d["spacing"]
    print("%s seed %d: %d matches, %d tuples, M = %d, %d inliers; displacement to fp64 %.3e of max_dist (bound %.3e); %.4f deg, rms %.4f spacings"
          % (name, seed, len(d["pairs"]), r["tuples_accepted"], r["set_size"], r["inliers"], disp, 4 * R.E, rot, rms))
    assert disp <= 4 * R.E
    return rot, rms


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cat_against_fp64_and_the_truth(eng, catf, seed):
    rot, rms = check_against_fp64_and_truth(eng, catf, seed, "cat")
    assert rot < 0.1 and rms < 0.05                    # tests/test_gpu_global.py's bounds for RANSAC on the cat


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_bumps_against_fp64_and_the_truth(eng, bumps, seed):
    rot, rms = check_against_fp64_and_truth(eng, bumps, seed, "bumps")
    assert rms < 1.0                                    # ... and on the bumps pair: below 1 spacing


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_bumps_shifted_against_fp64_and_the_truth(eng, bumps_shifted, seed):
    rot, rms = check_against_fp64_and_truth(eng, bumps_shifted, seed, "bumps shifted by 1e4")
    assert rms < 1.0


# ---- 6. degenerate inputs: a status, not a hang ---------------------------------------------------------------------------------------
def test_degenerate_inputs(sym, eng):
    ident = lambda n: np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
    line = np.zeros((40, 3), F)
    line[:, 0] = np.arange(40)
    for kw in (dict(), dict(max_tuples=0)):
        r = eng.fgr(line, line, ident(40), 0.5, check=False, want_trace=True, **kw)
        assert r["status"] == sym.ERR_DEGENERATE and r["iterations"] == 0
        assert np.isfinite(r["transform"]).all() and np.array_equal(r["transform"], np.eye(4, dtype=F))
    point = np.tile(np.array([[1.0, 2.0, 3.0]], F), (20, 1))
    r = eng.fgr(point, point, ident(20), 0.5, check=False)
    assert r["status"] == sym.ERR_DEGENERATE and r["iterations"] == 0 and np.isfinite(r["transform"]).all()
    with pytest.raises(sym.SymmIcpError) as e:
        eng.fgr(line, line, ident(40), 0.5)
    assert e.value.status == sym.ERR_DEGENERATE
    # weights that sum to less than 6 (mu at a tiny floor at once, every residual far above it): PLANE's solve refuses the record
    rng = np.random.default_rng(9)
    a, b = rng.random((60, 3)).astype(F), rng.random((60, 3)).astype(F)
    r = eng.fgr(a, b, ident(60), 1e-3, division_factor=1e9, decrease_every=1, max_tuples=0, check=False, want_trace=True)
    assert r["status"] == sym.ERR_DEGENERATE and r["iterations"] == 0 and 0 < r["weight_sum"] < 6 and r["sums_trace"][0][37] == 60
    assert np.array_equal(r["transform"][:3, :3], np.eye(3, dtype=F)) and np.isfinite(r["transform"]).all()
    # m = 3 on a proper triangle succeeds
    from symmicp import synth
    tri = np.array([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0.3]], F)
    T = synth.rigid4(synth.rotation(20.0, (0.1, 0.7, 0.2)), np.array([0.3, -0.2, 0.1]))
    moved = (tri.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(F)
    r = eng.fgr(tri, moved, ident(3), 0.05, seed=1)
    assert r["status"] == sym.OK and r["iterations"] == 64 and r["inliers"] == 3
    assert np.abs(tri.astype(np.float64) @ r["transform64"][:3, :3].T + r["transform64"][:3, 3] - moved).max() < 1e-5
    for bad in (dict(iterations=0), dict(division_factor=1.0), dict(tuple_scale=0.0), dict(max_dist=-1.0), dict(decrease_every=0)):
        assert eng.fgr(tri, moved, ident(3), **dict(dict(max_dist=0.05, check=False), **bad))["status"] == sym.ERR_ARG, bad


# ---- 7. the composition: MyICP (Python and C++) and the driver ----------------------------------------------------------------------
def python_icp(sym, d):
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, verbose=False)
    icp.setMaxCorrespondenceDistance(2 * d["max_dist"])
    icp.setInputSource(d["src"], d["src_n"])
    icp.setInputTarget(d["tgt"], d["tgt_n"])
    return icp


def far_or_failed(sym, status, T, d):
    """started from the identity the engine does NOT solve the case: a status other than OK, or an end more than 10 spacings rms away"""
    rms = G.rms_to_truth(T, d["truth"], d["src"]) / d["spacing"]
    print("   from the identity: status %d, %.1f spacings rms from the truth" % (status, rms))
    return status != sym.OK or rms > 10.0


def test_myicp_fgr_init_python_cpp_and_driver(sym, tmp_path):
    d = G.bumps_pair()
    icp = python_icp(sym, d)
    r0 = icp.align()
    assert far_or_failed(sym, r0["status"], r0["transform"], d)         # else the case shows nothing
    icp.setGlobalInit(fpfh_radius=d["radius"], max_dist=d["max_dist"], seed=1, method="fgr", hypotheses=1)
    ra = icp.align()
    g = icp.globalResult()
    rb = python_icp(sym, d).align(d["truth"])                            # the yardstick: the same engine given the true transform
    assert ra["status"] == rb["status"] == sym.OK and g["status"] == sym.OK and g["method"] == "fgr" and "evaluated" not in g
    diff = float(np.abs(ra["transform"].astype(np.float64) - rb["transform"]).max())
    print("bumps: %d correspondences, %d tuples, M = %d, %d inliers; init %.3f spacings rms from the truth; |T_fgr - T_truth-started| = %.2e"
          % (g["correspondences"], g["tuples_accepted"], g["set_size"], g["inliers"],
             G.rms_to_truth(g["transform"], d["truth"], d["src"]) / d["spacing"], diff))
    assert diff <= E2E_BOUND
    assert np.array_equal(icp.align(d["truth"])["transform"], rb["transform"])      # a caller's guess switches the initialisation off
    icp.setGlobalInit(fpfh_radius=d["radius"], max_dist=d["max_dist"], method="fgr", fgr_division_factor=1.0)
    with pytest.raises(sym.SymmIcpError) as e:                           # a failing initialisation is raised, not replaced by the identity
        icp.align()
    assert e.value.status == sym.ERR_ARG and "FGR" in str(e.value)
    with pytest.raises(ValueError):
        icp.setGlobalInit(fpfh_radius=d["radius"], max_dist=d["max_dist"], method="teaser")

    # the C++ class on the same inputs
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_fgr")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for fname, arr in [("src", d["src"]), ("tgt", d["tgt"]), ("truth", d["truth"]), ("src_n", d["src_n"]), ("tgt_n", d["tgt_n"]),
                       ("params", np.array([d["radius"], d["max_dist"], 64, 1, 0.0, 2 * d["max_dist"], 30]))]:
        np.ascontiguousarray(arr, F).tofile(tmp_path / (fname + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {k: np.fromfile(tmp_path / ("out_%s.f32" % k), F) for k in ("identity", "global", "truth")}
    init = np.fromfile(tmp_path / "init.f32", F)
    assert far_or_failed(sym, int(out["identity"][0]), out["identity"][1:].reshape(4, 4), d)
    assert out["global"][0] == 0 and out["truth"][0] == 0
    Tg, Tt = out["global"][1:].reshape(4, 4), out["truth"][1:].reshape(4, 4)
    assert float(np.abs(Tg.astype(np.float64) - Tt).max()) <= E2E_BOUND
    # the two classes make the same calls: the same bits
    assert np.array_equal(init[:16].reshape(4, 4), g["transform"])
    assert list(init[16:]) == [g["correspondences"], g["tuples_accepted"], g["set_size"], g["iterations"], g["inliers"]]
    assert np.array_equal(Tg, ra["transform"]) and np.array_equal(Tt, rb["transform"])

    # the driver: exit code 0, one line about the initialisation, the written cloud is the source moved to the same fixed point.  It keeps
    # x, y, z of a PCD file alone and estimates the normals towards a viewpoint at the origin, and FPFH matching needs them oriented alike
    # in both clouds (include/myicp.h): where bumps_pair() puts the pair the origin sees the two surfaces from opposite sides (one true
    # match of 452, no estimator can use that).  So the pair is shifted to where the origin looks at both from their front: far out along
    # the bisector of the two mean normals, e_z and R e_z.
    from symmicp import synth
    ez = np.array([0.0, 0.0, 1.0])
    bis = ez + synth.rotation(*G.BUMPS_ROTATION) @ ez
    src0 = d["src"]
    d = G.bumps_pair(shift=-20.0 * bis / np.linalg.norm(bis))
    d["src_n"] = d["tgt_n"] = None
    rb = python_icp(sym, d).align(d["truth"])
    assert rb["status"] == sym.OK
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    a, b, out = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), str(tmp_path / "moved.pcd")
    sym.pcd_write(a, d["src"], binary=True)
    sym.pcd_write(b, d["tgt"], binary=True)
    base = [exe, "--mode", "paper", "--corr", "tree", "--iters", "30", "--max-dist", "%r" % (2 * d["max_dist"]), "--out", out]
    init = ["--init", "fgr", "--fpfh-radius", "%r" % d["radius"], "--fgr-dist", "%r" % d["max_dist"], "--fgr-iters", "64", "--fgr-tuples", "1000",
            "--seed", "1"]
    r = subprocess.run(base + init + [a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("global init:")]
    assert len(lines) == 1 and "correspondences" in lines[0] and "FGR" in lines[0] and "tuples accepted" in lines[0] and "inliers" in lines[0]
    moved, _ = sym.pcd_read(out)
    want = d["src"].astype(np.float64) @ rb["transform"].astype(np.float64)[:3, :3].T + rb["transform"].astype(np.float64)[:3, 3]
    rms = float(np.sqrt(((moved - want) ** 2).sum(1).mean()))
    # the bound of the runs above, as a distance: entries within E2E_BOUND of the truth-started 4x4, in the frame bumps_pair() itself puts
    # the pair in, move every coordinate of a point x of it by less than (|x| + |y| + |z| + 1) E2E_BOUND; a distance holds in any frame
    bound = np.sqrt(3.0) * float((np.abs(src0).sum(1) + 1.0).max()) * E2E_BOUND
    print("icp_align --init fgr: %s\n   rms to the truth-started result %.2e (bound %.2e, spacing %.2e)" % (lines[0], rms, bound, d["spacing"]))
    assert rms <= bound
    os.remove(out)
    r = subprocess.run(base + ["--quiet", a, b], capture_output=True, text=True, timeout=600)
    far = r.returncode != 0
    if not far:
        moved, _ = sym.pcd_read(out)
        far = float(np.sqrt(((moved - want) ** 2).sum(1).mean())) > 10 * d["spacing"]
    assert far
    for bad in (["--init", "fgr"], ["--fgr-dist", "3"], ["--init", "global", "--fpfh-radius", "3", "--ransac-dist", "1", "--fgr-iters", "3"],
                ["--init", "fgr", "--fpfh-radius", "3", "--fgr-dist", "-1"], ["--init", "fgr", "--fpfh-radius", "3", "--ransac-dist", "1"],
                ["--init", "fgr", "--fpfh-radius", "3", "--fgr-dist", "1", "--ransac-iters", "100"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64
