"""GPU ISS keypoints (symmicp_ctx_iss_keypoints; kernels_keypoints.hip) against tests/_iss_ref.py: the neighbour counts exactly, the
saliency of every point the reference calls clear against fp64, the non-maximum suppression exactly as a function of the device's own
saliencies, the smallest shapes at which the kernels can go wrong, the cap protocol, and the keypoint stage of the global
initialisation in MyICP (Python and C++)."""
import os
import subprocess

import numpy as np
import pytest

import _fpfh_ref as R
import _global_ref as G
import _iss_ref as I
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
CAT_SPACING = 1.3816
CAT_RS, CAT_RN = 6 * CAT_SPACING, 4 * CAT_SPACING
CAT_R = 11.05                 # the FPFH radius and RANSAC distance tests/test_gpu_global.py uses for cat
CAT_DIST = CAT_R / 4
E2E_BOUND = 1e-4              # tests/test_gpu_global.py's bound on the same comparison


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


@pytest.fixture(scope="module")
def cases(cat, bunny):
    """name -> (xyz, salient radius, non-maximum radius, query rows or None)"""
    from symmicp import synth
    c4 = synth.c4_surface(50_000)["src"]
    rows = np.sort(np.random.default_rng(5).choice(len(c4), 4096, replace=False))
    bs = R.median_spacing(bunny, np.arange(len(bunny)))
    return dict(cat=(cat["src"], CAT_RS, CAT_RN, None), cat_out=(cat["tgt"], CAT_RS, CAT_RN, None), bunny=(bunny, 6 * bs, 4 * bs, None),
                c4=(c4, 0.0138, 0.0092, rows))


def check_saliency(dev, xyz, rs, q=None, **kw):
    """the saliency stage of the device result `dev` on the rows q against the reference; returns the reference"""
    q = np.arange(len(xyz)) if q is None else q
    ref = I.saliency(xyz, rs, queries=q, **kw)
    unclear = 1.0 - float(ref["clear"].mean())
    assert unclear < 0.01                                                  # from the reference alone
    assert np.array_equal(dev["neighbors"][q], ref["k"])
    cl = ref["clear"]
    s = dev["saliency"][q].astype(np.float64)
    l1, l3 = ref["lam"][:, 0], ref["lam"][:, 2]
    flags_agree = np.array_equal(s[cl] > 0, ref["salient"][cl])
    sa = cl & ref["salient"]
    err = np.abs(s[sa] - l3[sa]) - (2.0 ** -23 * l3[sa] + 1e-12 * l1[sa])
    print("   %d rows, %.3f %% not clear, %d salient; worst |s - l3| minus its bound: %.3e" % (len(q), 100 * unclear, int(sa.sum()),
                                                                                           float(err.max(initial=-np.inf))))
    assert flags_agree
    assert (err <= 0).all()
    assert (dev["saliency"] >= 0).all() and np.isfinite(dev["saliency"]).all()
    return ref


def check_nms(dev, xyz, rn, q=None, min_neighbors=5):
    """the keypoint rows are the numpy NMS of the device's OWN saliencies over the exact neighbourhoods; ascending"""
    rows = dev["rows"]
    assert rows.dtype == np.int32 and (np.diff(rows) > 0).all()
    want = I.nms(dev["saliency"], xyz, rn, min_neighbors, queries=q)
    got = rows if q is None else np.intersect1d(rows, q)
    assert np.array_equal(got, want)
    return want


def run(eng, xyz, rs, rn, **kw):
    return eng.iss_keypoints(xyz, rs, rn, return_saliency=True, **kw)


# ---- 1. and 2. the two stages on real clouds -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cat", "cat_out", "bunny", "c4"])
def test_saliency_and_nms_stages(eng, cases, name):
    xyz, rs, rn, q = cases[name]
    dev = run(eng, xyz, rs, rn)
    check_saliency(dev, xyz, rs, q)
    kept = check_nms(dev, xyz, rn, q)
    print("   %s: %d keypoints in all, %d among the checked rows" % (name, len(dev["rows"]), len(kept)))
    assert len(dev["rows"]) > 0


def test_cat_counts_are_the_pinned_ones(eng, cat):
    """tests/test_iss_ref.py pins 91 / 33 / 160 keypoints from the reference alone; no cat point is unclear, so the device must agree"""
    x = cat["src"]
    for (a, b), want in (((6, 4), 91), ((8, 6), 33), ((4, 3), 160)):
        rows_ref, sal = I.keypoints(x, a * CAT_SPACING, b * CAT_SPACING)
        dev = run(eng, x, a * CAT_SPACING, b * CAT_SPACING)
        check_nms(dev, x, b * CAT_SPACING)
        print("   %d / %d spacings: %d keypoints (reference %d)" % (a, b, len(dev["rows"]), len(rows_ref)))
        assert len(rows_ref) == want and sal["clear"].all()
        # A row's verdict depends on comparisons of its own saliency alone, and the device's fp32 saliency is within one ulp of the
        # reference's: the two row sets may differ only at rows that have a neighbour within rn whose saliency is within two ulps
        _, offs, nb, _ = R.radius_sets(x, b * CAT_SPACING)
        seg = np.repeat(np.arange(len(x)), np.diff(offs))
        si, sj = sal["s"].astype(np.float64)[seg], sal["s"].astype(np.float64)[nb]
        near = (si > 0) & (sj > 0) & (np.abs(si - sj) <= 2.0 ** -22 * np.maximum(si, sj))
        assert np.isin(np.setxor1d(dev["rows"], rows_ref), seg[near]).all()
        if not near.any():
            assert len(dev["rows"]) == want


def test_frames_cat_keypoints_survive_the_rigid_motion(eng, cat):
    a = eng.iss_keypoints(cat["src"], CAT_RS, CAT_RN)
    b = eng.iss_keypoints(cat["tgt"], CAT_RS, CAT_RN)
    common = len(np.intersect1d(a, b))
    print("   %d keypoints of cat, %d of cat_out, %d at the same row" % (len(a), len(b), common))
    assert common >= 0.9 * len(a)


# ---- 3. the smallest shapes at which it can go wrong ------------------------------------------------------------------------------
def slab(n, seed):
    x = np.random.default_rng(seed).random((n, 3)).astype(F)
    x[:, 2] *= F(0.3)
    return x


def test_one_point(eng):
    dev = run(eng, np.array([[1.0, 2.0, 3.0]], F), 1.0, 1.0)
    assert len(dev["rows"]) == 0 and list(dev["neighbors"]) == [0] and list(dev["saliency"]) == [0.0]


@pytest.mark.parametrize("n", [5, 6])
def test_n_at_min_neighbors(eng, n):
    """n = min_neighbors: every point has n - 1 < 5 neighbours, nothing is salient; one more and every point has exactly 5"""
    x = slab(n, 11 + n)
    dev = run(eng, x, 10.0, 10.0)
    assert (dev["neighbors"] == n - 1).all()
    ref = check_saliency(dev, x, 10.0)
    check_nms(dev, x, 10.0)
    if n == 5:
        assert not dev["saliency"].any() and len(dev["rows"]) == 0
    else:
        assert ref["salient"].any() and len(dev["rows"]) == 1          # rn covers the cloud: the arg-max alone


@pytest.mark.parametrize("n", [255, 257, 513])
def test_sizes_that_fill_no_block_and_no_leaf(eng, n):
    x = slab(n, n)
    dev = run(eng, x, 0.3, 0.2)
    check_saliency(dev, x, 0.3)
    check_nms(dev, x, 0.2)
    assert 0 < len(dev["rows"]) < n


def test_all_points_equal(eng):
    x = np.tile(np.array([[0.5, -1.25, 3.0]], F), (64, 1))
    dev = run(eng, x, 1.0, 1.0)
    assert (dev["neighbors"] == 63).all() and not dev["saliency"].any() and len(dev["rows"]) == 0


def test_two_points_1e_minus_20_apart(eng):
    x = np.array([[0, 0, 0], [1e-20, 2e-20, 3e-20]], F)
    dev = run(eng, x, 1.0, 1.0, min_neighbors=1)
    assert list(dev["neighbors"]) == [1, 1]                              # d2 underflows towards 0 and is still <= r2
    assert not dev["saliency"].any() and len(dev["rows"]) == 0           # rank one: l3 is 0 up to 1e-13 l1 = 1e-52, which is 0 in fp32


def test_collinear_points(eng):
    t = np.cumsum(np.random.default_rng(1).integers(1, 4, 40)) * 0.25
    x = np.zeros((40, 3), F)
    x[:, 0] = t
    dev = run(eng, x, 3.0, 3.0)
    ref = I.saliency(x, 3.0)
    assert np.array_equal(dev["neighbors"], ref["k"]) and dev["neighbors"].min() >= 5
    assert not dev["saliency"].any() and len(dev["rows"]) == 0           # along an axis every product with y or z is exactly 0
    d = np.stack([t, t, t], 1).astype(F)                                 # along the diagonal: l2 = l3 = 0 up to the promised 1e-13 l1
    dev = run(eng, d, 6.0, 6.0)
    ref = I.saliency(d, 6.0)
    assert np.array_equal(dev["neighbors"], ref["k"])
    assert (dev["saliency"].astype(np.float64) <= 1e-13 * ref["lam"][:, 0]).all()
    check_nms(dev, d, 6.0)


def test_flat_lattice_has_saliency_exactly_zero(eng):
    x = I.lattice(9, 9)
    dev = run(eng, x, I.LATTICE_RS, I.LATTICE_RS)
    assert np.array_equal(dev["neighbors"], I.saliency(x, I.LATTICE_RS)["k"]) and dev["neighbors"][40] == 20
    assert not dev["saliency"].any() and len(dev["rows"]) == 0


def test_lattice_with_one_raised_point(eng):
    x = I.lattice(9, 9, [(4, 4)])
    dev = run(eng, x, I.LATTICE_RS, I.LATTICE_RS)
    check_saliency(dev, x, I.LATTICE_RS)
    check_nms(dev, x, I.LATTICE_RS)
    assert list(dev["rows"]) == [40] and dev["saliency"][40] == F(0.25)   # C is exactly diag(2.65625, 1.7, 0.25) at the apex
    assert int((dev["saliency"] > 0).sum()) == 21


def test_exact_tie_goes_to_the_lowest_row(eng):
    x, a, b = I.double_bump()
    dev = run(eng, x, I.LATTICE_RS, I.LATTICE_RS)
    assert bits(dev["saliency"][a]) == bits(dev["saliency"][b]) == bits(F(0.25))
    assert list(dev["rows"]) == sorted([a, b])                           # out of each other's reach
    dev = run(eng, x, I.LATTICE_RS, 9.0)
    assert list(dev["rows"]) == [min(a, b)]
    check_nms(dev, x, 9.0)
    swapped = x.copy()
    swapped[[a, b]] = swapped[[b, a]]                                    # the other point now holds the lower row (and the other sorted position)
    assert list(eng.iss_keypoints(swapped, I.LATTICE_RS, 9.0)) == [min(a, b)]


def test_extreme_radii_and_gamma_one(eng, cat):
    x = cat["src"]
    dev = run(eng, x, CAT_RS, 1e4)                                       # rn larger than the cloud: the arg-max, lowest row first
    s = dev["saliency"]
    assert list(dev["rows"]) == [int(np.nonzero(s == s.max())[0][0])]
    dev = run(eng, x, 0.01, 0.01)                                        # rs below the spacing: no point has 5 neighbours
    assert dev["neighbors"].max() < 5 and not dev["saliency"].any() and len(dev["rows"]) == 0
    dev = run(eng, x, CAT_RS, CAT_RN, gamma21=1.0, gamma32=1.0)
    ref = check_saliency(dev, x, CAT_RS, gamma21=1.0, gamma32=1.0)
    check_nms(dev, x, CAT_RN)
    assert ref["salient"].sum() >= I.saliency(x, CAT_RS)["salient"].sum()
    dev = run(eng, x, CAT_RS, CAT_RN, min_neighbors=60)                  # the count test of both stages bites
    check_saliency(dev, x, CAT_RS, min_neighbors=60)
    check_nms(dev, x, CAT_RN, min_neighbors=60)


def test_strided_and_column_major_inputs(sym, eng, cat):
    xyz = cat["src"]
    n = len(xyz)
    cfg = sym.iss_config(CAT_RS, CAT_RN)
    st, rows, count, sal, nb = eng.iss_keypoints_raw(xyz, cfg, cap=n)
    assert st == 0 and count > 0
    x4 = np.zeros((n, 4), F); x4[:, :3] = xyz
    cm = np.asfortranarray(xyz).T.copy()
    x6 = np.zeros((n, 6), F); x6[:, 0::2] = xyz
    for buf, strides in ((x4, (n, 4, 1)), (cm, (n, 1, n)), (x6, (n, 6, 2))):
        st, rows2, count2, sal2, nb2 = eng.iss_keypoints_raw(buf, cfg, cap=n, strides=strides)
        assert st == 0 and count2 == count and np.array_equal(rows2, rows)
        assert np.array_equal(bits(sal2), bits(sal)) and np.array_equal(nb2, nb)


def test_cloud_shifted_by_1e4(eng, cat):
    x = (cat["src"] + F(1e4)).astype(F)
    dev = run(eng, x, CAT_RS, CAT_RN)
    assert np.array_equal(dev["neighbors"], I.saliency(x, CAT_RS)["k"])
    check_nms(dev, x, CAT_RN)
    assert len(dev["rows"]) > 0


# ---- 4. protocol ------------------------------------------------------------------------------------------------------------------
def test_cap_protocol(sym, eng, cat):
    x = cat["src"]
    cfg = sym.iss_config(CAT_RS, CAT_RN)
    full = run(eng, x, CAT_RS, CAT_RN)
    k = len(full["rows"])
    st, rows, count, sal, nb = eng.iss_keypoints_raw(x, cfg)                             # rows_out == NULL, cap 0: the count
    assert st == sym.ERR_SIZE and count == k and rows is None
    assert np.array_equal(bits(sal), bits(full["saliency"])) and np.array_equal(nb, full["neighbors"])
    st, rows, count, sal, nb = eng.iss_keypoints_raw(x, cfg, cap=k - 1)
    assert st == sym.ERR_SIZE and count == k and (rows == -1).all()                      # the rows are not written ...
    assert np.array_equal(bits(sal), bits(full["saliency"])) and np.array_equal(nb, full["neighbors"])   # ... the rest is
    st, rows, count, sal, nb = eng.iss_keypoints_raw(x, cfg, cap=k)
    assert st == 0 and count == k and np.array_equal(rows, full["rows"])
    st, rows, count, _, _ = eng.iss_keypoints_raw(x, sym.iss_config(0.01, 0.01))         # no keypoint: the count query succeeds
    assert st == 0 and count == 0
    for bad in (dict(salient_radius=-1.0), dict(non_max_radius=float("nan")), dict(gamma21=0.0), dict(min_neighbors=0)):
        c = sym.iss_config(**dict(dict(salient_radius=CAT_RS, non_max_radius=CAT_RN), **bad))
        assert eng.iss_keypoints_raw(x, c, cap=k)[0] == sym.ERR_ARG
    assert eng.iss_keypoints_raw(x, cfg, cap=k)[0] == 0                                  # ... and the context still works


def test_two_calls_and_two_contexts_give_identical_bits(sym, eng, cases):
    for name in ("cat", "c4"):
        xyz, rs, rn, _ = cases[name]
        a, b = run(eng, xyz, rs, rn), run(eng, xyz, rs, rn)
        with sym.Engine() as e2:
            c = run(e2, xyz, rs, rn)
        d = sym.iss_keypoints(xyz, rs, rn, return_saliency=True)                         # the module-level call creates its own
        for o in (b, c, d):
            assert np.array_equal(a["rows"], o["rows"]) and np.array_equal(bits(a["saliency"]), bits(o["saliency"]))
            assert np.array_equal(a["neighbors"], o["neighbors"])


def test_context_with_clouds_is_left_untouched(sym, cat, cases):
    """two contexts run the same two passes; one of them computes keypoints of other clouds between the passes: every record,
    the certificates and the correspondences are bit-identical"""
    def passes(between):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            out = [e.begin(), e.step()]
            if between:
                for name in ("c4", "cat_out"):
                    xyz, rs, rn, _ = cases[name]
                    e.iss_keypoints(xyz, rs, rn)
            out.append(e.step())
            return out, e.certificates(), e.correspondences(), e.source(), e.pivot()
    (ra, ca, ka, sa, pa), (rb, cb, kb, sb, pb) = passes(True), passes(False)
    for x, y in zip(ra, rb):
        assert x["status"] == y["status"] and x["iter"] == y["iter"] and x["pairs"] == y["pairs"]
        assert np.array_equal(x["sums"].view(np.uint64), y["sums"].view(np.uint64))
        assert np.array_equal(bits(x["increment"]), bits(y["increment"]))
        assert np.array_equal(np.array([x["diff"], x["rcond"]]).view(np.uint64), np.array([y["diff"], y["rcond"]]).view(np.uint64))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ca, cb))
    assert all(np.array_equal(x, y) for x, y in zip(ka, kb)) and all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert np.array_equal(pa, pb)


# ---- 5. the composition: MyICP (Python and C++) and the driver -----------------------------------------------------------------
def cat140(cat):
    """tests/test_gpu_global.py's cat case: the target turned 140 degrees and moved away, normals estimated by MyICP"""
    from symmicp import synth
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    truth0 = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    R2, t2 = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([40.0, -25.0, 60.0])
    tgt = (cat["tgt"].astype(np.float64) @ R2.T + t2).astype(F)
    return dict(src=cat["src"], tgt=tgt, truth=synth.rigid4(R2, t2) @ truth0, spacing=1.38, radius=CAT_R, max_dist=CAT_DIST, hypotheses=65536)


def python_icp(sym, d):
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, verbose=False)
    icp.setMaxCorrespondenceDistance(2 * d["max_dist"])
    icp.setInputSource(d["src"], None)
    icp.setInputTarget(d["tgt"], None)
    return icp


def test_myicp_keypoint_init_python_and_cpp(sym, eng, cat, tmp_path):
    d = cat140(cat)
    base = dict(fpfh_radius=d["radius"], max_dist=d["max_dist"], hypotheses=d["hypotheses"], seed=1)
    icp = python_icp(sym, d)
    icp.setGlobalInit(**base)                                              # iss off: the calls as they were, composed by hand below
    r_off = icp.align()
    g_off = dict(icp.globalResult())
    assert r_off["status"] == sym.OK and g_off["source_keypoints"] == 0 and g_off["target_keypoints"] == 0
    feats = []
    for x in (d["src"], d["tgt"]):
        nrm, _ = eng.estimate_normals(x, 10)
        feats.append(eng.fpfh(x, nrm, d["radius"]))
    pairs, _ = eng.feature_correspondences(feats[0], feats[1])
    by_hand = eng.ransac(d["src"], d["tgt"], pairs, d["max_dist"], hypotheses=d["hypotheses"], seed=1)
    assert g_off["correspondences"] == len(pairs) and np.array_equal(bits(g_off["transform"]), bits(by_hand["transform"]))

    icp.setGlobalInit(iss=True, iss_salient_radius=CAT_RS, iss_non_max_radius=CAT_RN, **base)
    ra = icp.align()
    g = dict(icp.globalResult())
    rb = python_icp(sym, d).align(d["truth"])                              # the yardstick: the same engine given the true transform
    assert ra["status"] == rb["status"] == sym.OK and g["status"] == sym.OK
    ks, kt = eng.iss_keypoints(d["src"], CAT_RS, CAT_RN), eng.iss_keypoints(d["tgt"], CAT_RS, CAT_RN)
    assert (g["source_keypoints"], g["target_keypoints"]) == (len(ks), len(kt))
    assert 3 <= g["correspondences"] <= min(len(ks), len(kt)) and g["source_points"] == len(d["src"])
    diff = float(np.abs(ra["transform"].astype(np.float64) - rb["transform"]).max())
    print("%d and %d keypoints, %d correspondences (%d without keypoints), %d evaluated, %d -> %d inliers; init %.3f spacings rms from the truth; "
          "|T_iss - T_truth-started| = %.2e" % (len(ks), len(kt), g["correspondences"], g_off["correspondences"], g["evaluated"], g["inliers_ransac"],
                                                g["inliers_final"], G.rms_to_truth(g["transform"], d["truth"], d["src"]) / d["spacing"], diff))
    assert diff <= E2E_BOUND
    # fewer than 3 keypoints: raised with the step named, no fall-back to the full cloud
    icp.setGlobalInit(iss=True, iss_salient_radius=0.01, iss_non_max_radius=0.01, **base)
    with pytest.raises(sym.SymmIcpError) as e:
        icp.align()
    assert e.value.status == sym.ERR_NO_CONSENSUS and "ISS keypoints" in str(e.value)

    # the C++ class on the same inputs
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_keypoints")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for fname, arr in (("src", d["src"]), ("tgt", d["tgt"]), ("truth", d["truth"]),
                       ("params", np.array([d["radius"], d["max_dist"], d["hypotheses"], 1, 2 * d["max_dist"], 30, CAT_RS, CAT_RN, 0.01]))):
        np.ascontiguousarray(arr, F).tofile(tmp_path / (fname + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = {k: np.fromfile(tmp_path / ("out_%s.f32" % k), F) for k in ("off", "iss", "truth")}
    init = {k: np.fromfile(tmp_path / ("init_%s.f32" % k), F) for k in ("off", "iss")}
    assert out["off"][0] == 0 and out["iss"][0] == 0 and out["truth"][0] == 0
    Ti, Tt = out["iss"][1:].reshape(4, 4), out["truth"][1:].reshape(4, 4)
    assert float(np.abs(Ti.astype(np.float64) - Tt).max()) <= E2E_BOUND
    # the two classes make the same calls: the same bits, keypoints on or off
    assert np.array_equal(init["iss"][:16].reshape(4, 4), g["transform"]) and np.array_equal(init["off"][:16].reshape(4, 4), g_off["transform"])
    assert list(init["iss"][16:]) == [g["correspondences"], len(ks), len(kt), g["inliers_final"]]
    assert list(init["off"][16:]) == [g_off["correspondences"], 0, 0, g_off["inliers_final"]]
    assert np.array_equal(Ti, ra["transform"]) and np.array_equal(out["off"][1:].reshape(4, 4), r_off["transform"])
    assert np.array_equal(Tt, rb["transform"])


def test_icp_align_driver_init_keypoints(sym, cat, tmp_path):
    d = cat140(cat)
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    a, b, out = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), str(tmp_path / "moved.pcd")
    sym.pcd_write(a, d["src"])
    sym.pcd_write(b, d["tgt"])
    base = [exe, "--mode", "paper", "--corr", "tree", "--iters", "30", "--max-dist", "%r" % (2 * d["max_dist"]), "--out", out]
    init = ["--init", "global", "--fpfh-radius", "%r" % d["radius"], "--ransac-dist", "%r" % d["max_dist"], "--ransac-iters", "65536", "--seed", "1"]
    kp = ["--init-keypoints", "iss", "--iss-radius", "%r" % CAT_RS, "--iss-nms-radius", "%r" % CAT_RN]
    r = subprocess.run(base + init + kp + [a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("global init:")]
    assert len(lines) == 1 and "ISS keypoints" in lines[0] and "correspondences" in lines[0]
    ks, kt = sym.iss_keypoints(d["src"], CAT_RS, CAT_RN), sym.iss_keypoints(d["tgt"], CAT_RS, CAT_RN)
    assert "%d and %d ISS keypoints" % (len(ks), len(kt)) in lines[0]
    moved, _ = sym.pcd_read(out)
    want = d["src"].astype(np.float64) @ d["truth"][:3, :3].T + d["truth"][:3, 3]
    rms = float(np.sqrt(((moved - want) ** 2).sum(1).mean()))
    print("icp_align --init-keypoints iss: rms to the truth %.4f (spacing 1.38)" % rms)
    assert rms < 0.05                                                       # tests/test_gpu_global.py's bound for the same driver
    for bad in (kp, init + ["--init-keypoints", "iss"], init + ["--iss-radius", "3"], init + ["--init-keypoints", "harris"],
                init + kp + ["--iss-min-neighbors", "0"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64
