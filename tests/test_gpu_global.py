"""GPU feature matching and RANSAC (symmicp_ctx_feature_nn, symmicp_ctx_feature_correspondences, symmicp_ctx_ransac;
kernels_global.hip) against tests/_global_ref.py: the matching bit for bit, every RANSAC hypothesis against fp64 up to the ones the
reference itself calls unclear, the refit against numpy's Kabsch fit, what the whole is for (two clouds 140 degrees apart), and the
composition in MyICP (Python and C++)."""
import os
import subprocess

import numpy as np
import pytest

import _global_ref as G
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
CAT_R = 11.05
CAT_DIST = CAT_R / 4


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
    """the cat pair with its golden normals, FPFH at r = 11.05 and the mutual correspondences, all from the device"""
    fs, ft = eng.fpfh(cat["src"], cat["src_n"], CAT_R), eng.fpfh(cat["tgt"], cat["tgt_n"], CAT_R)
    pairs, d2 = eng.feature_correspondences(fs, ft)
    return dict(src=cat["src"], tgt=cat["tgt"], fs=fs, ft=ft, pairs=pairs, d2=d2, truth=cat_truth(), max_dist=CAT_DIST, spacing=1.38)


def _bumps(eng, shift=None):
    b = G.bumps_pair(shift=shift)
    b["fs"], b["ft"] = eng.fpfh(b["src"], b["src_n"], b["radius"]), eng.fpfh(b["tgt"], b["tgt_n"], b["radius"])
    b["pairs"], b["d2"] = eng.feature_correspondences(b["fs"], b["ft"])
    return b


@pytest.fixture(scope="module")
def bumps(eng):
    return _bumps(eng)


@pytest.fixture(scope="module")
def c4f(eng):
    from symmicp import synth
    d = synth.c4_surface(50_000)
    return eng.fpfh(d["src"], d["src_n"], 0.0138), eng.fpfh(d["tgt"], d["tgt_n"], 0.0138)


def check_nn(e, fa, fb, ref=None):
    nn, d2, second = e.feature_nn(fa, fb)
    rn, rd, rs = G.feature_nn(fa, fb) if ref is None else ref
    assert np.array_equal(nn, rn)
    assert np.array_equal(bits(d2), bits(rd)) and np.array_equal(bits(second), bits(rs))
    return nn, d2, second


# ---- 1. matching, exact -------------------------------------------------------------------------------------------------------------
def test_nn_cat_in_full(eng, catf):
    nn, d2, second = check_nn(eng, catf["fs"], catf["ft"])
    assert (second >= d2).all() and (nn >= 0).all()
    check_nn(eng, catf["ft"], catf["fs"])


def test_nn_4096_queries_against_c4_surface_50k(eng, c4f):
    fs, ft = c4f
    rows = np.sort(np.random.default_rng(7).choice(len(ft), 4096, replace=False))
    check_nn(eng, ft[rows], fs)


def test_nn_single_candidate_and_single_query(eng, catf):
    fs, ft = catf["fs"], catf["ft"]
    nn, d2, second = check_nn(eng, fs[:300], ft[5:6])
    assert not nn.any() and np.isinf(second).all() and (second > 0).all()
    check_nn(eng, fs[17:18], ft)
    nn, d2, second = check_nn(eng, fs[:1], ft[:1])
    assert list(nn) == [0] and np.isinf(second[0])


def test_nn_duplicate_candidates_lower_row_wins(eng, catf):
    fs, ft = catf["fs"][:500], catf["ft"][:700]
    fb = np.concatenate([ft, ft[:400], ft[100:300]])
    nn, d2, second = check_nn(eng, fs, fb)
    assert (nn < 700).all()
    dup = nn < 400
    assert dup.any() and np.array_equal(bits(second[dup]), bits(d2[dup]))          # the copy is the runner-up, at the same distance


def test_nn_all_zero_histograms(eng):
    za, zb = np.zeros((300, 33), F), np.zeros((513, 33), F)
    nn, d2, second = check_nn(eng, za, zb)
    assert not nn.any() and not d2.any() and not second.any()
    fa = np.zeros((50, 33), F); fa[:, 3] = 100.0
    check_nn(eng, fa, zb)
    check_nn(eng, za, fa)


@pytest.mark.parametrize("na,nb", [(257, 4099), (1, 129), (513, 127), (1023, 1), (255, 128), (700, 1025)])
def test_nn_sizes_that_fit_no_tile(eng, na, nb):
    rng = np.random.default_rng(na * 7919 + nb)
    fa = (rng.random((na, 33)) * 100).astype(F)
    fb = (rng.random((nb, 33)) * 100).astype(F)
    fb[nb // 2] = fb[0]
    check_nn(eng, fa, fb)


def test_nn_split_and_unsplit_candidates_give_the_same_answer(sym, catf, monkeypatch):
    """SYMMICP_FEATURE_NN_SPLITS / _QUERIES (read at symmicp_create) force how the candidates are split over workgroups and how
    many queries a thread holds: every shape gives the bits of the reference"""
    fa, fb = catf["fs"][:1111], catf["ft"]
    ref = G.feature_nn(fa, fb)
    for splits, q in (("1", "1"), ("1", "2"), ("2", "1"), ("7", "2"), ("64", "1"), ("3400", "2"), ("", "")):
        for key, val in (("SYMMICP_FEATURE_NN_SPLITS", splits), ("SYMMICP_FEATURE_NN_QUERIES", q)):
            if val:
                monkeypatch.setenv(key, val)
            else:
                monkeypatch.delenv(key, raising=False)
        with sym.Engine() as e:
            check_nn(e, fa, fb, ref)
            check_nn(e, fa[:1], fb, tuple(x[:1] for x in ref))


def test_nn_refuses_non_finite_features(sym, eng, catf):
    fs, ft = catf["fs"][:100].copy(), catf["ft"][:100].copy()
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            a, b = fs.copy(), ft.copy()
            (a, b)[which][37, 5] = bad
            with pytest.raises(sym.SymmIcpError) as e:
                eng.feature_nn(a, b)
            assert e.value.status == sym.ERR_ARG
            assert eng.feature_correspondences_raw(a, b)[0] == sym.ERR_ARG
    check_nn(eng, fs, ft)                                                          # ... and the context still works


@pytest.mark.parametrize("mutual", [True, False])
@pytest.mark.parametrize("ratio", [0.0, 0.8, 0.95])
def test_correspondences_filters_against_numpy(eng, catf, mutual, ratio):
    pairs, d2 = eng.feature_correspondences(catf["fs"], catf["ft"], mutual=mutual, max_ratio=ratio)
    rp, rd = G.correspondences(catf["fs"], catf["ft"], mutual, ratio)
    assert np.array_equal(pairs, rp) and np.array_equal(bits(d2), bits(rd))
    assert (np.diff(pairs[:, 0]) > 0).all()
    if not mutual and ratio == 0.0:
        assert len(pairs) == len(catf["fs"])


def test_correspondences_cap_protocol(sym, eng, catf):
    fs, ft = catf["fs"], catf["ft"]
    n = len(catf["pairs"])
    st, pairs, d2, count = eng.feature_correspondences_raw(fs, ft, cap=0)             # pairs_out == NULL: the count
    assert st == sym.ERR_SIZE and count == n and pairs is None
    st, pairs, d2, count = eng.feature_correspondences_raw(fs, ft, cap=n - 1)
    assert st == sym.ERR_SIZE and count == n
    st, pairs, d2, count = eng.feature_correspondences_raw(fs, ft, cap=n)
    assert st == 0 and count == n and np.array_equal(pairs, catf["pairs"])


def test_matching_twice_and_on_a_context_holding_clouds_leaves_it_untouched(sym, cat, catf, bumps):
    """align, match and run RANSAC on the same context, align again: source, certificates, correspondences and the following
    alignment are bit-identical (the check of tests/test_gpu_fpfh.py::test_context_untouched)"""
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        r1 = e.align()
        src1, nrm1 = e.source()
        idx1, d21 = e.correspondences()
        cert1 = e.certificates()
        piv1 = e.pivot()
        a = e.feature_nn(catf["fs"], catf["ft"])
        b = e.feature_nn(catf["fs"], catf["ft"])
        pa = e.feature_correspondences(bumps["fs"], bumps["ft"])
        ra = e.ransac(bumps["src"], bumps["tgt"], bumps["pairs"], bumps["max_dist"], hypotheses=65536, seed=3, want_hypotheses=True, check=False)
        rb = e.ransac(bumps["src"], bumps["tgt"], bumps["pairs"], bumps["max_dist"], hypotheses=65536, seed=3, want_hypotheses=True, check=False)
        assert all(np.array_equal(bits(x) if x.dtype == F else x, bits(y) if y.dtype == F else y) for x, y in zip(a, b))
        assert np.array_equal(pa[0], bumps["pairs"]) and np.array_equal(bits(pa[1]), bits(bumps["d2"]))
        for key in ("transform", "transform64", "hyp_status", "hyp_inliers", "inlier_mask"):
            assert np.array_equal(ra[key], rb[key]), key
        assert ra["status"] == rb["status"] and ra["best_hypothesis"] == rb["best_hypothesis"]
        src2, nrm2 = e.source()
        cert2 = e.certificates()
        idx1b, d21b = e.correspondences()
        assert np.array_equal(src1, src2) and np.array_equal(nrm1, nrm2)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(cert1, cert2))
        assert np.array_equal(idx1, idx1b) and np.array_equal(d21, d21b)
        r2 = e.align()
        idx2, d22 = e.correspondences()
        assert np.array_equal(e.pivot(), piv1)
    assert r1["status"] == r2["status"] == 0 and r1["iters"] == r2["iters"]
    assert np.array_equal(r1["transform"], r2["transform"]) and np.array_equal(r1["diffs"], r2["diffs"])
    assert np.array_equal(idx1, idx2) and np.array_equal(d21, d22)
    with sym.Engine() as e2:                                                          # another context: the same bits
        c = e2.feature_nn(catf["fs"], catf["ft"])
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    d = sym.feature_nn(catf["fs"], catf["ft"])                                        # the module-level call creates its own
    assert all(np.array_equal(x, y) for x, y in zip(a, d))


def test_matching_quality_on_the_cat_pair(eng, cat):
    """tests/test_gpu_fpfh.py::test_features_find_the_counterpart_on_the_cat_pair without SciPy: normals estimated on each cloud
    alone (k = 10, viewpoint at the origin), FPFH at r = 11.05, every source row matched to its nearest target row in feature
    space; the share of matches within r of the true counterpart (row i <-> row i) is 0.9885 there.  The exact fp32 rule and the
    fp64 k-d tree may break a handful of near-ties differently: three rows of 3 400 (0.001) are allowed."""
    src, tgt = cat["src"], cat["tgt"]
    f = []
    for x in (src, tgt):
        nrm, _ = eng.estimate_normals(x, 10)
        f.append(eng.fpfh(x, nrm, CAT_R))
    j = eng.feature_nn(f[0], f[1])[0]
    d = np.linalg.norm(tgt[j].astype(np.float64) - tgt.astype(np.float64), axis=1)
    share = float((d <= CAT_R).mean())
    print("within r of the counterpart: %.4f (the very row %.4f)" % (share, float((j == np.arange(len(src))).mean())))
    assert abs(share - 0.9885) <= 0.001


# ---- 2. RANSAC against fp64 ---------------------------------------------------------------------------------------------------------
def ransac_inputs(name, eng, catf, bumps):
    if name == "cat":
        return catf, 4000, (1, 2, 3)
    if name == "cat_shifted":
        d = dict(catf)
        d["src"], d["tgt"] = (catf["src"] + F(1e4)).astype(F), (catf["tgt"] + F(1e4)).astype(F)
        return d, 4000, (1, 2, 3)
    return bumps, 262144, tuple(range(1, 9))


def displacement(hyp32, Rt64, p, q, rows, max_dist):
    """max over the hypotheses `rows` and all correspondence points of |T32 p - T64 p| / max_dist"""
    worst = 0.0
    P = p.astype(np.float64)
    for a in range(0, len(rows), 256):
        h = rows[a:a + 256]
        d = hyp32[h].astype(np.float64) - Rt64[h]
        mv = np.einsum("hij,kj->hki", d[:, :9].reshape(-1, 3, 3), P) + d[:, None, 9:]
        worst = max(worst, float(np.sqrt((mv * mv).sum(2)).max(initial=0.0)))
    return worst / max_dist


@pytest.mark.parametrize("name", ["cat", "cat_shifted", "bumps"])
def test_hypotheses_against_fp64(sym, eng, catf, bumps, name):
    d, H, seeds = ransac_inputs(name, eng, catf, bumps)
    src, tgt, pairs, md = d["src"], d["tgt"], d["pairs"], d["max_dist"]
    worst = 0.0
    for seed in seeds:
        hyp, status, piv = eng.ransac_hypotheses(src, tgt, pairs, md, hypotheses=H, seed=seed)
        p, q, cs, ct = G.pivoted(src, tgt, pairs)
        assert np.array_equal(bits(piv[0]), bits(cs)) and np.array_equal(bits(piv[1]), bits(ct))
        c = G.draws(seed, H, len(pairs))
        ref = G.hypotheses(p, q, c, md)
        unclear = float((~ref["clear"]).mean())
        print("%s seed %d: %d evaluated by fp64, %.3f %% not clear" % (name, seed, (ref["status"] == G.EVALUATED).sum(), 100 * unclear))
        assert unclear < 0.01                                                     # from the reference alone
        assert np.array_equal(status == G.REPEATED, ref["status"] == G.REPEATED)   # the draws are integers: exact
        cl = ref["clear"]
        assert np.array_equal(status[cl], ref["status"][cl])
        both = np.nonzero((status == G.EVALUATED) & (ref["status"] == G.EVALUATED))[0]
        assert len(both) > 0
        assert not hyp[(status != G.EVALUATED) & (status != G.FAR)].any()
        w = displacement(hyp, ref["Rt"], p, q, both, float(F(md)))
        print("   largest displacement device vs fp64 over %d hypotheses x %d points: %.3e of max_dist" % (len(both), len(pairs), w))
        worst = max(worst, w)
        # the counts of the full run lie between the fp64 counts at max_dist (1 -+ DELTA)
        r = eng.ransac(src, tgt, pairs, md, hypotheses=H, seed=seed, refits=0, want_hypotheses=True)
        assert np.array_equal(r["hyp_status"], status)
        inl = r["hyp_inliers"]
        assert not inl[status != G.EVALUATED].any()
        lo = G.inlier_counts(ref["Rt"][both], p, q, float(F(md)) * (1 - G.DELTA))
        hi = G.inlier_counts(ref["Rt"][both], p, q, float(F(md)) * (1 + G.DELTA))
        assert np.all(lo <= inl[both]) and np.all(inl[both] <= hi)
        # the winner: the arg-max of the device's own counts, ties to the lowest h; and a maximum by fp64's lights too
        ev = np.nonzero(status == G.EVALUATED)[0]
        best = int(ev[np.argmax(inl[ev])])
        assert r["best_hypothesis"] == best and r["inliers_ransac"] == inl[best] and r["evaluated"] == len(ev)
        assert best in both and hi[np.searchsorted(both, best)] >= lo.max()
        assert int(r["inlier_mask"].sum()) == r["inliers_ransac"] == r["inliers_final"]
    print("%s: largest displacement %.3e of max_dist (recorded: %.3e, DELTA = %.3e)" % (name, worst, G.MEASURED_DISPLACEMENT, G.DELTA))
    assert worst <= 2 * G.MEASURED_DISPLACEMENT          # half of DELTA: the recorded margin still describes the device


@pytest.mark.parametrize("name", ["cat", "bumps"])
def test_refit_against_numpy_kabsch(eng, catf, bumps, name):
    d, H, seeds = ransac_inputs(name, eng, catf, bumps)
    src, tgt, pairs, md = d["src"], d["tgt"], d["pairs"], d["max_dist"]
    X, Y = src[pairs[:, 0]], tgt[pairs[:, 1]]
    extent = float(np.abs(np.concatenate([X, Y])).max())
    seed = seeds[0]
    prev = None
    for refits in (0, 1, 2):
        r = eng.ransac(src, tgt, pairs, md, hypotheses=H, seed=seed, refits=refits, want_hypotheses=True)
        T = r["transform64"]
        assert np.array_equal(bits(r["transform"]), bits(T.astype(F)))             # the fp32 4x4 is the fp64 result rounded
        assert np.array_equal(T[3], [0, 0, 0, 1])
        assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-5 and np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-5
        if refits == 0:
            # the winner's 12 floats about the pivots, composed into the caller's coordinates in fp64
            hyp, _, piv = eng.ransac_hypotheses(src, tgt, pairs, md, hypotheses=H, seed=seed)
            Rw, tw = hyp[r["best_hypothesis"], :9].astype(np.float64).reshape(3, 3), hyp[r["best_hypothesis"], 9:].astype(np.float64)
            assert np.abs(T[:3, :3] - Rw).max() == 0
            assert np.abs(T[:3, 3] - (tw + piv[1] - Rw @ piv[0].astype(np.float64))).max() <= 1e-12 * max(extent, 1.0)
        else:
            K = G.kabsch(X[prev], Y[prev])
            print("%s refit %d: |R - R_numpy| %.2e, |t - t_numpy| %.2e (extent %.3g)" % (name, refits, np.abs(T[:3, :3] - K[:3, :3]).max(),
                                                                                       np.abs(T[:3, 3] - K[:3, 3]).max(), extent))
            assert np.abs(T[:3, :3] - K[:3, :3]).max() <= 1e-9
            assert np.abs(T[:3, 3] - K[:3, 3]).max() <= 1e-9 * extent
            assert np.array_equal(r["inlier_mask"], G.inlier_mask64(T, X, Y, md))
            res = np.linalg.norm(X[r["inlier_mask"]].astype(np.float64) @ T[:3, :3].T + T[:3, 3] - Y[r["inlier_mask"]], axis=1)
            assert abs(r["rmse_final"] - np.sqrt((res ** 2).mean())) <= 1e-9 * max(extent, 1.0)
        assert r["inliers_final"] == int(r["inlier_mask"].sum())
        prev = r["inlier_mask"]


def test_ransac_argument_errors_and_no_consensus(sym, eng, catf):
    src, tgt, pairs, md = catf["src"], catf["tgt"], catf["pairs"], catf["max_dist"]
    ok = dict(max_dist=md, hypotheses=500, seed=1)
    for bad in (dict(max_dist=0.0), dict(max_dist=float("nan")), dict(max_dist=float("inf")), dict(hypotheses=0), dict(hypotheses=2 ** 24 + 1),
                dict(edge_ratio=1.5), dict(edge_ratio=float("nan")), dict(refits=-1), dict(refits=9)):
        r = eng.ransac(src, tgt, pairs, check=False, **dict(ok, **bad))
        assert r["status"] == sym.ERR_ARG, bad
    for bad_pairs in (pairs[:2], np.array([[0, 0], [1, 1], [len(src), 2]], np.int32), np.array([[0, 0], [1, -1], [2, 2]], np.int32)):
        assert eng.ransac(src, tgt, bad_pairs, check=False, **ok)["status"] == sym.ERR_ARG
    s2 = src.copy(); s2[pairs[5, 0], 1] = np.nan
    assert eng.ransac(s2, tgt, pairs, check=False, **ok)["status"] == sym.ERR_ARG
    # three collinear pairs: every hypothesis is REPEATED or DEGENERATE -> no consensus, said loudly, identity returned
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], F)
    r = eng.ransac(line, line, np.array([[0, 0], [1, 1], [2, 2]], np.int32), 0.1, hypotheses=256, seed=1, want_hypotheses=True, check=False)
    assert r["status"] == sym.ERR_NO_CONSENSUS and r["evaluated"] == 0 and r["best_hypothesis"] == -1
    assert np.array_equal(r["transform"], np.eye(4, dtype=F)) and not r["inlier_mask"].any()
    assert set(np.unique(r["hyp_status"])) <= {G.REPEATED, G.DEGENERATE} and not r["hyp_inliers"].any()
    with pytest.raises(sym.SymmIcpError) as e:
        eng.ransac(line, line, np.array([[0, 0], [1, 1], [2, 2]], np.int32), 0.1, hypotheses=256, seed=1)
    assert e.value.status == sym.ERR_NO_CONSENSUS and "ransac" in str(e.value)
    # edge check off (<= 0): the statuses of the reference without it
    p, q, _, _ = G.pivoted(src, tgt, pairs)
    r = eng.ransac(src, tgt, pairs, md, hypotheses=2000, seed=4, edge_ratio=0.0, want_hypotheses=True)
    ref = G.hypotheses(p, q, G.draws(4, 2000, len(pairs)), md, edge_ratio=0.0)
    assert not (r["hyp_status"] == G.EDGE).any() and np.array_equal(r["hyp_status"][ref["clear"]], ref["status"][ref["clear"]])


# ---- 3. it does what it is for ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_cat_is_registered_from_its_features(eng, catf, seed):
    r = eng.ransac(catf["src"], catf["tgt"], catf["pairs"], CAT_DIST, hypotheses=4000, seed=seed, refits=1)
    rot, rms = G.rotation_error_deg(r["transform"], catf["truth"]), G.rms_to_truth(r["transform"], catf["truth"], catf["src"])
    print("cat seed %d: %d correspondences, %d evaluated, %d -> %d inliers; %.4f deg, rms %.4f" % (
        seed, len(catf["pairs"]), r["evaluated"], r["inliers_ransac"], r["inliers_final"], rot, rms))
    assert rot < 0.1 and rms < 0.05


def check_bumps(eng, b, seed):
    r = eng.ransac(b["src"], b["tgt"], b["pairs"], b["max_dist"], hypotheses=262144, seed=seed, refits=1)
    rms = G.rms_to_truth(r["transform"], b["truth"], b["src"]) / b["spacing"]
    print("bumps seed %d: %d correspondences, %d evaluated, %d -> %d inliers; %.3f deg, rms %.3f spacings" % (
        seed, len(b["pairs"]), r["evaluated"], r["inliers_ransac"], r["inliers_final"], G.rotation_error_deg(r["transform"], b["truth"]), rms))
    assert rms < 1.0
    return r


@pytest.mark.parametrize("seed", list(range(1, 9)))
def test_bumps_140_degrees_apart(eng, bumps, seed):
    check_bumps(eng, bumps, seed)


@pytest.fixture(scope="module")
def bumps_shifted(eng):
    return _bumps(eng, shift=(1e3, -2e3, 5e2))


@pytest.mark.parametrize("seed", list(range(1, 9)))
def test_bumps_far_from_the_origin(eng, bumps_shifted, seed):
    check_bumps(eng, bumps_shifted, seed)


# ---- 4. the composition: MyICP (Python and C++) and the driver --------------------------------------------------------------------
E2E_BOUND = 1e-4          # the project's own bound on a 4x4 (smoke()): both runs reach the same fixed point


def e2e_case(name, cat):
    """-> dict(src, tgt, src_n, tgt_n (None: MyICP estimates them), truth, spacing, radius, max_dist, hypotheses)"""
    from symmicp import synth
    if name == "bumps":
        b = G.bumps_pair()
        return dict(b, hypotheses=262144)
    R2, t2 = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([40.0, -25.0, 60.0])
    tgt = (cat["tgt"].astype(np.float64) @ R2.T + t2).astype(F)
    return dict(src=cat["src"], tgt=tgt, src_n=None, tgt_n=None, truth=synth.rigid4(R2, t2) @ cat_truth(), spacing=1.38, radius=CAT_R,
                max_dist=CAT_DIST, hypotheses=65536)


def python_icp(sym, d):
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, verbose=False)
    icp.setMaxCorrespondenceDistance(2 * d["max_dist"])
    icp.setInputSource(d["src"], d["src_n"])
    icp.setInputTarget(d["tgt"], d["tgt_n"])
    return icp


def far_or_failed(sym, status, T, d):
    """the existing engine started from the identity does NOT solve the case: a status other than OK, or an end more than 10
    spacings rms from the truth"""
    rms = G.rms_to_truth(T, d["truth"], d["src"]) / d["spacing"]
    print("   from the identity: status %d, %.1f spacings rms from the truth" % (status, rms))
    return status != sym.OK or rms > 10.0


@pytest.mark.parametrize("name", ["bumps", "cat140"])
def test_myicp_global_init_python_and_cpp(sym, cat, name, tmp_path):
    d = e2e_case(name, cat)
    icp = python_icp(sym, d)
    r0 = icp.align()
    assert far_or_failed(sym, r0["status"], r0["transform"], d)         # else the case shows nothing
    icp.setGlobalInit(fpfh_radius=d["radius"], max_dist=d["max_dist"], hypotheses=d["hypotheses"], seed=1)
    ra = icp.align()
    g = icp.globalResult()
    rb = python_icp(sym, d).align(d["truth"])                            # the yardstick: the same engine given the true transform
    assert ra["status"] == rb["status"] == sym.OK and g["status"] == sym.OK
    diff = float(np.abs(ra["transform"].astype(np.float64) - rb["transform"]).max())
    print("%s: %d correspondences, %d evaluated, %d -> %d inliers; init %.3f spacings rms from the truth; |T_global - T_truth-started| = %.2e; "
          "end %.4f spacings from the truth" % (name, g["correspondences"], g["evaluated"], g["inliers_ransac"], g["inliers_final"],
                                                G.rms_to_truth(g["transform"], d["truth"], d["src"]) / d["spacing"], diff,
                                                G.rms_to_truth(ra["transform"], d["truth"], d["src"]) / d["spacing"]))
    assert diff <= E2E_BOUND
    assert np.array_equal(icp.getFinalTransformation(), ra["transform"])
    # a caller's guess switches the initialisation off
    assert np.array_equal(icp.align(d["truth"])["transform"], rb["transform"])
    # with voxel levels the initialisation feeds the first level: the same bits as the levels started from its transform by hand
    levels = [(2.0 * d["spacing"], 20, 4 * d["max_dist"]), (0.0, 30, 2 * d["max_dist"])]
    icp.setVoxelLevels(levels)
    rl = icp.align()
    by_hand = python_icp(sym, d)
    by_hand.setVoxelLevels(levels)
    assert rl["status"] == sym.OK and np.array_equal(rl["transform"], by_hand.align(g["transform"])["transform"])
    # a failing initialisation is raised, not replaced by the identity
    icp.setGlobalInit(fpfh_radius=d["radius"], max_dist=d["max_dist"] * 1e-6, hypotheses=1, seed=1)
    with pytest.raises(sym.SymmIcpError) as e:
        icp.align()
    assert e.value.status == sym.ERR_NO_CONSENSUS and "RANSAC" in str(e.value)

    # the C++ class on the same inputs
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_global")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    files = [("src", d["src"]), ("tgt", d["tgt"]), ("truth", d["truth"]),
             ("params", np.array([d["radius"], d["max_dist"], d["hypotheses"], 1, 0.0, 2 * d["max_dist"], 30]))]
    if d["src_n"] is not None:
        files += [("src_n", d["src_n"]), ("tgt_n", d["tgt_n"])]
    for fname, arr in files:
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
    assert list(init[16:]) == [g["correspondences"], g["evaluated"], g["inliers_ransac"], g["inliers_final"], g["best_hypothesis"]]
    assert np.array_equal(Tg, ra["transform"]) and np.array_equal(Tt, rb["transform"])


def test_icp_align_driver_init_global(sym, cat, tmp_path):
    """icp_align --init global on two PCD files 140 degrees apart: exit code 0, one line about the initialisation, and the written
    cloud lies on the target; without --init global the same command does not get there"""
    d = e2e_case("cat140", cat)
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    a, b, out = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), str(tmp_path / "moved.pcd")
    sym.pcd_write(a, d["src"])
    sym.pcd_write(b, d["tgt"])
    base = [exe, "--mode", "paper", "--corr", "tree", "--iters", "30", "--max-dist", "%r" % (2 * d["max_dist"]), "--out", out]
    init = ["--init", "global", "--fpfh-radius", "%r" % d["radius"], "--ransac-dist", "%r" % d["max_dist"], "--ransac-iters", "65536", "--seed", "1"]
    r = subprocess.run(base + init + [a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("global init:")]
    assert len(lines) == 1 and "correspondences" in lines[0] and "hypotheses evaluated" in lines[0] and "inliers" in lines[0]
    moved, _ = sym.pcd_read(out)
    want = d["src"].astype(np.float64) @ d["truth"][:3, :3].T + d["truth"][:3, 3]
    rms = float(np.sqrt(((moved - want) ** 2).sum(1).mean()))
    print("icp_align --init global: rms to the truth %.4f (spacing 1.38)" % rms)
    assert rms < 0.05
    os.remove(out)
    r = subprocess.run(base + ["--quiet", a, b], capture_output=True, text=True, timeout=600)
    far = r.returncode != 0
    if not far:
        moved, _ = sym.pcd_read(out)
        far = float(np.sqrt(((moved - want) ** 2).sum(1).mean())) > 10 * 1.38
    assert far
    for bad in (["--init", "global"], ["--fpfh-radius", "3"], ["--init", "global", "--fpfh-radius", "3", "--ransac-dist", "-1"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64
