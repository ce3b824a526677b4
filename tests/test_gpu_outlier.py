"""Statistical and radius outlier removal on the device (symmicp_ctx_statistical_outlier_removal, symmicp_ctx_radius_outlier_removal;
kernels_outlier.hip) against tests/_outlier_ref.py.

The comparison is EXACT: mean_dist as uint64 views, mu / sd / thr and the kept rows equal.  The device's fp64 sqrt, add and divide are
correctly rounded (no fast-math), the k smallest fp32 d2 are a well-defined multiset, and the sum runs in ascending d2 on both sides:
a mismatch is a kernel bug, not a tolerance question."""
import os
import re
import subprocess

import numpy as np
import pytest

import _knn_ref as K
import _outlier_ref as X
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
E2E_BOUND = 1e-4              # tests/test_gpu_global.py's bound on end-point comparisons of two alignments
NOISE_K, NOISE_MUL, NOISE_R, NOISE_MIN = 8, 1.0, 4 * X.CAT_SPACING, 3
TIGHT_R = X.CAT_SPACING       # a radius that takes surface points too (with min_neighbors 1: those whose nearest point is farther)


def b64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


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
def noisy(cat):
    """the noisy pair of the function tests: cat with stray points, and cat moved by a small rigid motion with other stray points"""
    from symmicp import synth
    truth = synth.rigid4(synth.rotation(5.0, (0.3, 0.5, 0.8)), np.array([1.0, -0.5, 0.8]))
    moved = (cat["src"].astype(np.float64) @ truth[:3, :3].T + truth[:3, 3]).astype(F)
    sx, si, so = X.noisy_cat(cat["src"])
    tx, ti, to = X.noisy_cat(moved, seed=11)
    return dict(src=sx, src_injected=si, src_origin=so, tgt=tx, tgt_injected=ti, tgt_origin=to, truth=truth)


def check_exact(eng, xyz, k, std_mul=1.0):
    """the device's whole result against the reference's; returns the device's"""
    dev = eng.remove_statistical_outlier(xyz, k, std_mul, return_stats=True)
    ref = X.statistical(xyz, k, std_mul)
    bad = np.nonzero(b64(dev["mean_dist"]) != b64(ref["mean_dist"]))[0]
    assert len(bad) == 0, (len(bad), bad[:8], dev["mean_dist"][bad[:8]], ref["mean_dist"][bad[:8]])
    assert (dev["mu"], dev["sd"], dev["thr"]) == (ref["mu"], ref["sd"], ref["thr"])
    assert dev["rows"].dtype == np.int32 and np.array_equal(dev["rows"], ref["rows"])
    return dev


# ---- 1. exactness on real clouds ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 8, 16, 17, 20, 50, 64])
def test_cat_is_exact(eng, cat, k):
    dev = check_exact(eng, cat["src"], k, 2.0 if k in (20, 64) else 1.0)
    assert 0 < len(dev["rows"]) < len(cat["src"])


def test_bunny_is_exact(eng, bunny):
    check_exact(eng, bunny, 20, 2.0)


@pytest.mark.parametrize("k", [20, 64])
def test_c4_sampled_rows_are_exact(eng, k):
    """50 000 points on the device; the reference on 4 096 sampled rows (its exact k-NN set of a row costs a pass over the cloud).
    The statistics and the kept rows are the reference's formula over the device's own n values."""
    from symmicp import synth
    x = synth.c4_surface(50_000)["src"]
    q = np.sort(np.random.default_rng(5).choice(len(x), 4096, replace=False))
    dev = eng.remove_statistical_outlier(x, k, 2.0, return_stats=True)
    assert np.array_equal(b64(dev["mean_dist"][q]), b64(X.mean_dist(x, k, q)))
    assert (dev["mu"], dev["sd"], dev["thr"]) == X.statistics(dev["mean_dist"], 2.0)
    assert np.array_equal(dev["rows"], X.kept(dev["mean_dist"], dev["thr"]))


# ---- 2. the smallest shapes ----------------------------------------------------------------------------------------------------------
def test_two_points(eng):
    dev = check_exact(eng, np.array([[0, 0, 0], [3, 4, 0]], F), 1)
    assert list(dev["mean_dist"]) == [5.0, 5.0] and list(dev["rows"]) == [0, 1]


@pytest.mark.parametrize("k", [1, 7, 64])
def test_every_other_point_is_a_neighbour(eng, k):
    check_exact(eng, np.random.default_rng(k).random((k + 1, 3)).astype(F), k)


@pytest.mark.parametrize("n,k", [(257, 8), (257, 40), (9, 8), (9, 3), (129, 64)])
def test_one_past_a_block_and_one_past_a_leaf(eng, n, k):
    """257 = one past a 256-thread block (k <= 32), 129 = one past a 128-thread block (k > 32), 9 = one past a leaf of 8"""
    check_exact(eng, np.random.default_rng(n + k).random((n, 3)).astype(F), k)


@pytest.mark.parametrize("k", [6, 7, 26])
def test_lattice_ties_at_the_kth_distance(eng, k):
    g = np.arange(6, dtype=F)
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    dev = check_exact(eng, x, k)
    if k == 6:
        assert dev["mean_dist"][x.tolist().index([2.0, 2.0, 2.0])] == 1.0          # an inner point: its 6 face neighbours


def test_all_points_identical(eng):
    x = np.tile(np.array([[0.5, -1.25, 3.0]], F), (100, 1))
    dev = check_exact(eng, x, 8)
    assert (dev["mean_dist"] == 0).all() and (dev["mu"], dev["sd"], dev["thr"]) == (0.0, 0.0, 0.0) and len(dev["rows"]) == 100


def test_collinear_points(eng):
    t = np.cumsum(np.random.default_rng(1).integers(1, 4, 100)) * 0.25
    x = np.zeros((100, 3), F)
    x[:, 0], x[:, 1], x[:, 2] = t, 2 * t, -t
    check_exact(eng, x, 8)
    check_exact(eng, x, 33)


def test_one_point_a_thousand_extents_away(eng):
    """its walk has to cross the whole tree (every other point is a neighbour candidate); its m is huge but finite"""
    x = np.random.default_rng(2).random((600, 3)).astype(F)
    x[321] = (1000.0, 1000.0, 1000.0)
    dev = check_exact(eng, x, 20)
    m = dev["mean_dist"]
    assert np.isfinite(m).all() and m[321] > 1700 and 321 not in dev["rows"] and len(dev["rows"]) == 599


def test_duplicated_rows(eng, cat):
    """70 copies of row 0 and k = 64: the copies' nearest 64 are each other at d2 == 0 (excluded by row, not by distance)"""
    x = np.concatenate([cat["src"], np.tile(cat["src"][:1], (70, 1))])
    dev = check_exact(eng, x, 64)
    assert (dev["mean_dist"][len(cat["src"]):] == 0).all() and dev["mean_dist"][0] == 0


def test_strided_and_column_major_inputs(eng, cat):
    xyz = cat["src"]
    n = len(xyz)
    st, rows, count, md, stats = eng.remove_statistical_outlier_raw(xyz, 20, 2.0, cap=n)
    st2, rows_r, count_r, nb = eng.remove_radius_outlier_raw(xyz, NOISE_R, 30, cap=n)
    assert st == 0 and st2 == 0 and 0 < count < n and 0 < count_r < n
    x4 = np.zeros((n, 4), F); x4[:, :3] = xyz
    cm = np.asfortranarray(xyz).T.copy()
    for buf, strides in ((x4, (n, 4, 1)), (cm, (n, 1, n))):
        s, r, c, m, t = eng.remove_statistical_outlier_raw(buf, 20, 2.0, cap=n, strides=strides)
        assert s == 0 and c == count and np.array_equal(r, rows) and np.array_equal(b64(m), b64(md)) and np.array_equal(b64(t), b64(stats))
        s, r, c, q = eng.remove_radius_outlier_raw(buf, NOISE_R, 30, cap=n, strides=strides)
        assert s == 0 and c == count_r and np.array_equal(r, rows_r) and np.array_equal(q, nb)


# ---- 3. the radius filter -----------------------------------------------------------------------------------------------------------
def test_radius_filter_is_the_radius_search_count(sym, eng, cat, bunny):
    import _fpfh_ref as R
    for x, r in ((cat["src"], NOISE_R), (cat["src"], 1.5 * X.CAT_SPACING), (bunny, 3 * R.median_spacing(bunny, np.arange(len(bunny))))):
        st, count = eng.radius_search_raw(x, r)[:2]
        assert st == 0 and count.max() > 1
        for mn in (1, max(1, int(np.median(count))), int(count.max()), int(count.max()) + 1):
            dev = eng.remove_radius_outlier(x, r, mn, return_counts=True)
            assert np.array_equal(dev["neighbors"], count)
            assert dev["rows"].dtype == np.int32 and np.array_equal(dev["rows"], np.nonzero(count >= mn)[0])
        assert len(dev["rows"]) == 0                                 # above every count: nothing is kept, and that is no error
        st, rows, c, nb = eng.remove_radius_outlier_raw(x, r, int(count.max()) + 1)
        assert st == sym.OK and c == 0                               # ... the count query succeeds too
    ref = X.radius(cat["src"], NOISE_R, 30)
    dev = eng.remove_radius_outlier(cat["src"], NOISE_R, 30, return_counts=True)
    assert np.array_equal(dev["neighbors"], ref["neighbors"]) and np.array_equal(dev["rows"], ref["rows"])


# ---- 4. protocol --------------------------------------------------------------------------------------------------------------------
def test_cap_protocol(sym, eng, cat):
    x = cat["src"]
    full = eng.remove_statistical_outlier(x, 20, 2.0, return_stats=True)
    k = len(full["rows"])
    stats = np.array([full["mu"], full["sd"], full["thr"]])
    written = lambda md, st3: np.array_equal(b64(md), b64(full["mean_dist"])) and np.array_equal(b64(st3), b64(stats))
    st, rows, count, md, st3 = eng.remove_statistical_outlier_raw(x, 20, 2.0)             # rows_out == NULL, cap 0: the count
    assert st == sym.ERR_SIZE and count == k and rows is None and written(md, st3)
    st, rows, count, md, st3 = eng.remove_statistical_outlier_raw(x, 20, 2.0, cap=k - 1)
    assert st == sym.ERR_SIZE and count == k and (rows == -1).all() and written(md, st3)  # the rows are not written, the rest is
    st, rows, count, md, st3 = eng.remove_statistical_outlier_raw(x, 20, 2.0, cap=k)
    assert st == 0 and count == k and np.array_equal(rows, full["rows"]) and written(md, st3)
    for bad in (dict(k=0), dict(k=65), dict(std_mul=float("nan"))):
        assert eng.remove_statistical_outlier_raw(x, **dict(dict(k=20, std_mul=2.0), **bad), cap=k)[0] == sym.ERR_ARG

    fr = eng.remove_radius_outlier(x, NOISE_R, 30, return_counts=True)
    k = len(fr["rows"])
    assert 0 < k < len(x)
    st, rows, count, nb = eng.remove_radius_outlier_raw(x, NOISE_R, 30)
    assert st == sym.ERR_SIZE and count == k and rows is None and np.array_equal(nb, fr["neighbors"])
    st, rows, count, nb = eng.remove_radius_outlier_raw(x, NOISE_R, 30, cap=k - 1)
    assert st == sym.ERR_SIZE and count == k and (rows == -1).all() and np.array_equal(nb, fr["neighbors"])
    st, rows, count, nb = eng.remove_radius_outlier_raw(x, NOISE_R, 30, cap=k)
    assert st == 0 and count == k and np.array_equal(rows, fr["rows"])
    assert eng.remove_radius_outlier_raw(x, -1.0, 30, cap=k)[0] == sym.ERR_ARG and eng.remove_radius_outlier_raw(x, NOISE_R, 0, cap=k)[0] == sym.ERR_ARG
    assert eng.remove_radius_outlier_raw(x, NOISE_R, 30, cap=k)[0] == 0                   # ... and the context still works


def test_context_with_clouds_is_left_untouched(sym, cat, noisy):
    """two contexts run the same passes; one of them filters other clouds between two steps: every record, the transform, the pairs
    and index_info are identical, and what the filters return on it is what the one-shot forms return"""
    got = {}

    def passes(between):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            out = [e.begin(), e.step()]
            info = e.index_info()
            if between:
                got["sor"] = e.remove_statistical_outlier(noisy["src"], 50, 1.0, return_stats=True)
                got["ror"] = e.remove_radius_outlier(noisy["tgt"], NOISE_R, NOISE_MIN, return_counts=True)
            after = e.index_info()
            assert sorted(after) == sorted(info) and all(np.array_equal(after[key], info[key]) for key in info)
            out.append(e.step())
            return out, e.certificates(), e.correspondences(), e.source(), e.pivot(), e.transform()
    (ra, ca, ka, sa, pa, ta), (rb, cb, kb, sb, pb, tb) = passes(True), passes(False)
    for x, y in zip(ra, rb):
        assert x["status"] == y["status"] and x["iter"] == y["iter"] and x["pairs"] == y["pairs"]
        assert np.array_equal(x["sums"].view(np.uint64), y["sums"].view(np.uint64))
        assert np.array_equal(x["increment"].view(np.uint32), y["increment"].view(np.uint32))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ca, cb))
    assert all(np.array_equal(x, y) for x, y in zip(ka, kb)) and all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert np.array_equal(pa, pb) and np.array_equal(ta, tb)
    one = sym.remove_statistical_outlier(noisy["src"], 50, 1.0, return_stats=True)
    assert np.array_equal(one["rows"], got["sor"]["rows"]) and np.array_equal(b64(one["mean_dist"]), b64(got["sor"]["mean_dist"]))
    assert (one["mu"], one["sd"], one["thr"]) == (got["sor"]["mu"], got["sor"]["sd"], got["sor"]["thr"])
    one = sym.remove_radius_outlier(noisy["tgt"], NOISE_R, NOISE_MIN, return_counts=True)
    assert np.array_equal(one["rows"], got["ror"]["rows"]) and np.array_equal(one["neighbors"], got["ror"]["neighbors"])


# ---- 5. function ----------------------------------------------------------------------------------------------------------------------
def test_noisy_cat_filters_remove_exactly_the_injected_points(eng, noisy):
    for name in ("src", "tgt"):
        x, injected = noisy[name], noisy[name + "_injected"]
        assert injected.sum() > 50
        for rows in (eng.remove_statistical_outlier(x, NOISE_K, NOISE_MUL), eng.remove_radius_outlier(x, NOISE_R, NOISE_MIN)):
            assert np.array_equal(rows, np.nonzero(~injected)[0])


def test_normals_of_the_filtered_cloud_are_those_of_the_clean_cat(eng, cat, noisy):
    """What the reference supports: a surviving surface row's k = 10 neighbour set can differ from its set in the clean cat only
    where a removed point was a neighbour -- and no surface row's set contained an injected point (asserted).  The kernel sums the
    moments in (d2, row) order, and the shuffle renumbers the rows: where the mapped neighbour SEQUENCES are identical (no tie in d2
    reordered; asserted for more than 99 % of the rows from the reference alone) the normals and curvatures are equal bit for bit."""
    x, origin = noisy["src"], noisy["src_origin"]
    keep = eng.remove_statistical_outlier(x, NOISE_K, NOISE_MUL)
    assert np.array_equal(keep, np.nonzero(origin >= 0)[0])
    o = origin[keep]
    assert not noisy["src_injected"][K.knn(x, 10, keep)[0]].any()
    filtered = x[keep]
    assert np.array_equal(filtered, cat["src"][o])
    same = (o[K.knn(filtered, 10)[0]] == K.knn(cat["src"], 10, o)[0]).all(axis=1)
    assert same.mean() > 0.99
    nf, cf = eng.estimate_normals(filtered, 10)
    nc, cc = eng.estimate_normals(cat["src"], 10)
    assert np.array_equal(nf[same].view(np.uint32), nc[o][same].view(np.uint32))
    assert np.array_equal(cf[same].view(np.uint32), cc[o][same].view(np.uint32))


# ---- 6. MyICP (Python and C++) and the driver -----------------------------------------------------------------------------------------
def new_icp(sym):
    return sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, verbose=False)


def icp_inputs(eng, noisy):
    """normals the caller supplies for the source (the clean rows' estimated normals, a marker on the stray rows) and intensities"""
    s_inj, t_inj = noisy["src_injected"], noisy["tgt_injected"]
    nrm = np.tile(np.array([[0, 0, 1]], F), (len(s_inj), 1))
    nrm[~s_inj] = eng.estimate_normals(noisy["src"][~s_inj], 10)[0]
    return nrm, np.arange(len(s_inj), dtype=F), np.arange(len(t_inj), dtype=F) * F(0.5)


def test_myicp_python(sym, eng, noisy):
    s_inj, t_inj = noisy["src_injected"], noisy["tgt_injected"]
    nrm, si, ti = icp_inputs(eng, noisy)
    icp = new_icp(sym)
    assert icp.outliersRemoved() == (0, 0)
    icp.setInputSource(noisy["src"], nrm, si)
    icp.setInputTarget(noisy["tgt"], None, ti)
    with pytest.raises(sym.SymmIcpError) as e:
        icp.removeStatisticalOutliers(65, 1.0)
    assert e.value.status == sym.ERR_ARG and len(icp.cloud_src) == len(s_inj)
    assert icp.removeStatisticalOutliers(NOISE_K, NOISE_MUL) == sym.OK
    assert icp.outliersRemoved() == (int(s_inj.sum()), int(t_inj.sum()))
    assert np.array_equal(icp.cloud_src, noisy["src"][~s_inj]) and np.array_equal(icp.cloud_tgt, noisy["tgt"][~t_inj])
    assert np.array_equal(icp.normals_src, nrm[~s_inj]) and icp._have_src and icp.normals_tgt is None
    assert np.array_equal(icp.intensity_src, si[~s_inj]) and np.array_equal(icp.intensity_tgt, ti[~t_inj])
    ra = icp.align()
    clean = new_icp(sym)                                                   # the clean pair: the surface rows, supplied the same normals
    clean.setInputSource(noisy["src"][~s_inj], nrm[~s_inj])
    clean.setInputTarget(noisy["tgt"][~t_inj], None)
    rb = clean.align()
    assert ra["status"] == rb["status"] == sym.OK
    diff = float(np.abs(ra["transform"].astype(np.float64) - rb["transform"]).max())
    off = float(np.abs(ra["transform"].astype(np.float64) - noisy["truth"]).max())
    print("|T_filtered - T_clean| = %.2e; |T_filtered - truth| = %.2e" % (diff, off))
    assert diff <= E2E_BOUND
    assert icp.removeRadiusOutliers(NOISE_R, NOISE_MIN) == sym.OK and icp.outliersRemoved() == (0, 0)      # nothing stray is left
    assert icp.removeRadiusOutliers(TIGHT_R, 1) == sym.OK                                      # ... a radius that does remove
    rs, rt = icp.outliersRemoved()
    assert rs > 0 and rt > 0 and len(icp.cloud_src) == int((~s_inj).sum()) - rs == len(icp.normals_src) == len(icp.intensity_src)


def test_myicp_cpp(sym, eng, noisy, tmp_path):
    s_inj, t_inj = noisy["src_injected"], noisy["tgt_injected"]
    nrm, si, ti = icp_inputs(eng, noisy)
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_outlier")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for fname, arr in (("src", noisy["src"]), ("tgt", noisy["tgt"]), ("src_nrm", nrm), ("src_int", si), ("tgt_int", ti),
                       ("params", np.array([NOISE_K, NOISE_MUL, TIGHT_R, 1]))):
        np.ascontiguousarray(arr, F).tofile(tmp_path / (fname + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "sor_src.i32", np.int32), np.nonzero(~s_inj)[0])
    assert np.array_equal(np.fromfile(tmp_path / "sor_tgt.i32", np.int32), np.nonzero(~t_inj)[0])
    assert np.array_equal(np.fromfile(tmp_path / "out_src.f32", F).reshape(-1, 3), noisy["src"][~s_inj])
    assert np.array_equal(np.fromfile(tmp_path / "out_tgt.f32", F).reshape(-1, 3), noisy["tgt"][~t_inj])
    # the two classes make the same calls: the transform of the Python class on the same inputs, and the radius filter's rows
    icp = new_icp(sym)
    icp.setInputSource(noisy["src"], nrm, si)
    icp.setInputTarget(noisy["tgt"], None, ti)
    icp.removeStatisticalOutliers(NOISE_K, NOISE_MUL)
    ra = icp.align()
    out = np.fromfile(tmp_path / "out_T.f32", F)
    assert out[0] == 0 and float(np.abs(out[1:].reshape(4, 4).astype(np.float64) - ra["transform"]).max()) <= E2E_BOUND
    icp.removeRadiusOutliers(TIGHT_R, 1)
    assert np.array_equal(np.fromfile(tmp_path / "ror_src.f32", F).reshape(-1, 3), icp.cloud_src)


def test_icp_align_driver_sor_and_ror(sym, noisy, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    a, b, out = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), str(tmp_path / "moved.pcd")
    sym.pcd_write(a, noisy["src"], binary=True)
    sym.pcd_write(b, noisy["tgt"], binary=True)
    ns, nt = len(noisy["src"]), len(noisy["tgt"])
    clean_s, clean_t = int((~noisy["src_injected"]).sum()), int((~noisy["tgt_injected"]).sum())
    base = [exe, "--mode", "paper", "--corr", "tree", "--iters", "30", "--out", out]
    r = subprocess.run(base + ["--ror", "%r:%d" % (NOISE_R, NOISE_MIN), "--sor", "%d:%g" % (NOISE_K, NOISE_MUL), a, b], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln for ln in r.stdout.splitlines() if "outlier removal:" in ln]
    assert len(lines) == 2 and lines[0].startswith("statistical") and lines[1].startswith("radius")      # the statistical filter first
    counts = [tuple(int(v) for v in re.search(r"source (\d+) -> (\d+), target (\d+) -> (\d+)", ln).groups()) for ln in lines]
    assert counts == [(ns, clean_s, nt, clean_t), (clean_s, clean_s, clean_t, clean_t)]
    moved, _ = sym.pcd_read(out)                                            # the filtered source, aligned
    T = noisy["truth"]
    want = noisy["src"][~noisy["src_injected"]].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    assert moved.shape == want.shape
    rms = float(np.sqrt(((moved - want) ** 2).sum(1).mean()))
    print("icp_align --sor --ror: rms to the truth %.4f (spacing 1.38)" % rms)
    assert rms < 0.05                                                       # tests/test_gpu_global.py's bound for the same driver
    q = subprocess.run(base + ["--quiet", "--sor", "8:1", a, b], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0 and "outlier removal" not in q.stdout
    for bad in (["--sor", "8"], ["--sor", "0:1"], ["--sor", "65:1"], ["--sor", "8:x"], ["--ror", "5"], ["--ror", "0:3"], ["--ror", "5:0"], ["--ror", "-1:3"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64
