"""GPU radius search and FPFH features (symmicp_ctx_radius_search, symmicp_ctx_fpfh; kernels_fpfh.hip) against tests/_fpfh_ref.py:
the neighbourhoods exactly, the SPFH counts against fp64 up to the pairs the reference itself calls ambiguous, the FPFH stage
against fp64 within a derived bound, the edge inputs, what the features are for, determinism, and a context left as it was."""
import ctypes as C
import os

import numpy as np
import pytest

import _fpfh_ref as R
import _knn_ref as K
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F = np.float32


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
def c4m():
    """c4_surface(1M), 4096 sampled rows, and the two radii (about 30 and about 100 neighbours) from its median spacing"""
    from symmicp import synth
    d = synth.c4_surface(1_000_000)
    rows = np.sort(np.random.default_rng(5).choice(1_000_000, 4096, replace=False))
    sp = R.median_spacing(d["src"], rows)
    return dict(xyz=d["src"], nrm=d["src_n"], rows=rows, radii=(R.SPACINGS_30 * sp, R.SPACINGS_100 * sp))


@pytest.fixture(scope="module")
def c4s():
    from symmicp import synth
    return synth.c4_surface(50_000)


@pytest.fixture(scope="module")
def lattice():
    g = np.arange(9, dtype=F) * F(0.25)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def take(offs, rows, d2, q):
    """the CSR lists of the rows q"""
    cnt = np.diff(offs)[q]
    o = np.zeros(len(q) + 1, np.int64)
    np.cumsum(cnt, out=o[1:])
    idx = np.repeat(offs[:-1][q] - o[:-1], cnt) + np.arange(o[-1])
    return o, rows[idx], d2[idx]


def sort_lists(sym, offs, rows, d2):
    from symmicp import _sort_lists
    return _sort_lists(offs, rows, d2) if len(rows) else (rows, d2)


def check_radius(sym, eng, xyz, r, queries=None, dev=None):
    """counts equal, every list equal as a set (both sides in (d2, row) order) and d2 bit-equal"""
    n = len(xyz)
    q = np.arange(n) if queries is None else queries
    count, offs, rows, d2 = eng.radius_search(xyz, r, sort=False) if dev is None else dev
    assert len(count) == n and offs[0] == 0 and offs[-1] == len(rows) == len(d2) and np.array_equal(np.diff(offs), count)
    rc, ro, rr, rd = R.radius_sets(xyz, r, None if queries is None else q)
    assert np.array_equal(count[q], rc)
    o, rows_q, d2_q = take(offs, rows, d2, q)
    rows_q, d2_q = sort_lists(sym, o, rows_q, d2_q)
    assert np.array_equal(o, ro) and np.array_equal(rows_q, rr)
    assert np.array_equal(d2_q.view(np.uint32), rd.view(np.uint32))
    return count, offs, rows, d2


# ---- 1. radius search, exact --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["src", "tgt"])
@pytest.mark.parametrize("r", [2.0, 5.53, 11.05, 40.0])
def test_radius_cat(sym, eng, cat, which, r):
    check_radius(sym, eng, cat[which], r)


@pytest.mark.parametrize("r", [0.004, 0.02])
def test_radius_bunny(sym, eng, bunny, r):
    check_radius(sym, eng, bunny, r)


def test_radius_lattice_with_boundary_ties(sym, eng, lattice):
    count, offs, rows, d2 = check_radius(sym, eng, lattice, 0.75)
    centre = (4 * 9 + 4) * 9 + 4
    assert count[centre] == 122 and (d2[offs[centre]:offs[centre + 1]] == F(0.5625)).sum() == 30


def test_radius_duplicates_isolated_and_single(sym, eng, cat):
    rng = np.random.default_rng(3)
    x = np.concatenate([cat["src"][:600], cat["src"][:150], cat["src"][:50], [[1e4, 1e4, 1e4]]]).astype(F)
    perm = rng.permutation(len(x))
    x = x[perm]
    count, offs, rows, d2 = check_radius(sym, eng, x, 5.53)
    far = int(np.nonzero(perm == len(x) - 1)[0][0])
    assert count[far] == 0
    assert (d2 == 0).sum() >= 2 * 150                 # a duplicate of the point itself, at d2 == 0, is a member
    one = np.array([[1.5, -2.0, 3.0]], F)
    count, offs, rows, d2 = eng.radius_search(one, 1.0)
    assert list(count) == [0] and list(offs) == [0, 0] and len(rows) == 0 and len(d2) == 0
    # the module-level call creates a context of its own
    a = sym.radius_search(x, 5.53)
    b = eng.radius_search(x, 5.53)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_radius_strided_inputs(sym, eng, cat):
    xyz = cat["src"]
    n = len(xyz)
    packed = eng.radius_search(xyz, 5.53, sort=False)
    total = len(packed[2])
    x4 = np.zeros((n, 4), F); x4[:, :3] = xyz                       # 16-byte points
    cm = np.asfortranarray(xyz).T.copy()                            # column-major n x 3
    x6 = np.zeros((n, 6), F); x6[:, 0::2] = xyz                     # the host transpose path
    for buf, strides in ((x4, (n, 4, 1)), (cm, (n, 1, n)), (x6, (n, 6, 2))):
        st, count, offs, rows, d2, tot = eng.radius_search_raw(buf, 5.53, cap=total, strides=strides)
        assert st == 0 and tot == total
        assert np.array_equal(count, packed[0]) and np.array_equal(offs, packed[1])
        assert np.array_equal(rows[:total], packed[2]) and np.array_equal(d2[:total].view(np.uint32), packed[3].view(np.uint32))


def test_radius_c4_surface_1m(sym, eng, c4m):
    for r, lo, hi in zip(c4m["radii"], (20, 80), (40, 120)):
        dev = eng.radius_search(c4m["xyz"], r, sort=False)
        count = check_radius(sym, eng, c4m["xyz"], r, c4m["rows"], dev=dev)[0]
        assert lo <= np.median(count[c4m["rows"]]) <= hi


def test_radius_cap_protocol_and_list_order(sym, eng, cat):
    xyz = cat["src"]
    n = len(xyz)
    rc = R.radius_sets(xyz, 5.53)[0]
    total = int(rc.sum())
    st, count, offs, rows, d2, tot = eng.radius_search_raw(xyz, 5.53)                       # counts only
    assert st == 0 and tot == total and np.array_equal(count, rc) and rows is None
    st, count, offs, rows, d2, tot = eng.radius_search_raw(xyz, 5.53, cap=total - 1)
    assert st == sym.ERR_SIZE and tot == total and np.array_equal(count, rc)
    assert (rows == -1).all() and (d2 == -1.0).all()                                        # the lists are not written
    st, count, offs, rows, d2, tot = eng.radius_search_raw(xyz, 5.53, cap=total)
    assert st == 0 and tot == total and (rows >= 0).all()
    st, _, _, rows_nod2, none, _ = eng.radius_search_raw(xyz, 5.53, cap=total, want_d2=False)   # d2_out == NULL
    assert st == 0 and none is None and np.array_equal(rows_nod2, rows)
    # the order inside the lists is the same on two calls (and on another context)
    st, count2, offs2, rows2, d22, _ = eng.radius_search_raw(xyz, 5.53, cap=total)
    assert np.array_equal(rows, rows2) and np.array_equal(d2.view(np.uint32), d22.view(np.uint32)) and np.array_equal(offs, offs2)
    with sym.Engine() as e2:
        st, _, _, rows3, d23, _ = e2.radius_search_raw(xyz, 5.53, cap=total)
    assert np.array_equal(rows, rows3) and np.array_equal(d2.view(np.uint32), d23.view(np.uint32))


def test_radius_and_fpfh_argument_errors_on_a_context(sym, eng, cat):
    L = sym.lib()
    x = np.ascontiguousarray(cat["src"][:200]); nr = np.ascontiguousarray(cat["src_n"][:200])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert eng.radius_search_raw(x, bad)[0] == sym.ERR_ARG
        with pytest.raises(sym.SymmIcpError) as e:
            eng.fpfh(x, nr, bad)
        assert e.value.status == sym.ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        y = x.copy(); y[17, 1] = bad
        assert eng.radius_search_raw(y, 5.0)[0] == sym.ERR_ARG       # the index build refuses non-finite coordinates
        with pytest.raises(sym.SymmIcpError) as e:
            eng.fpfh(y, nr, 5.0)
        assert e.value.status == sym.ERR_ARG
    assert eng.radius_search_raw(x, 5.0)[0] == 0                     # ... and the context still works


def test_context_untouched(sym, cat, c4s):
    """align, search and compute features of other clouds on the same context, align again: source, certificates,
    correspondences and the following alignment are bit-identical"""
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        r1 = e.align()
        src1, nrm1 = e.source()
        idx1, d21 = e.correspondences()
        cert1 = e.certificates()
        piv1 = e.pivot()
        e.radius_search(c4s["src"], 0.0138)
        e.fpfh(c4s["src"], c4s["src_n"], 0.0138)
        e.fpfh(cat["src"], cat["src_n"], 5.53, want_spfh=True)
        e.radius_search(cat["tgt"], 2.0)
        src2, nrm2 = e.source()
        cert2 = e.certificates()
        idx1b, d21b = e.correspondences()
        assert np.array_equal(src1, src2) and np.array_equal(nrm1, nrm2)
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(cert1, cert2))
        assert np.array_equal(idx1, idx1b) and np.array_equal(d21, d21b)
        r2 = e.align()
        idx2, d22 = e.correspondences()
        assert np.array_equal(e.pivot(), piv1)
    assert r1["status"] == r2["status"] == 0 and r1["iters"] == r2["iters"]
    assert np.array_equal(r1["transform"], r2["transform"]) and np.array_equal(r1["diffs"], r2["diffs"])
    assert np.array_equal(idx1, idx2) and np.array_equal(d21, d22)


# ---- 2. and 3. SPFH counts and the FPFH stage against fp64 -------------------------------------------------------------------------
def device_counts(dev):
    """the integer histograms behind spfh_out, and the check that spfh_out is bit-equal to (100 * c) / k for them"""
    k = dev["count"].astype(np.int64)
    c = np.rint(dev["spfh"].astype(np.float64) * k[:, None] / 100.0).astype(np.int64)
    assert np.array_equal(R.spfh_from_counts(c, k).view(np.uint32), dev["spfh"].view(np.uint32))
    assert (c >= 0).all() and (c[:, :11].sum(1) <= k).all()
    assert np.array_equal(c[:, :11].sum(1), c[:, 11:22].sum(1)) and np.array_equal(c[:, :11].sum(1), c[:, 22:].sum(1))
    return c, k


def check_spfh(xyz, nrm, r, dev, q):
    """sum_b |c_dev[b] - c_ref64[b]| <= 2 * (ambiguous feature values among the point's pairs); at most 1 % of the pairs may be
    ambiguous, asserted from the reference alone before the device is looked at"""
    rc, offs, rows, d2 = R.radius_sets(xyz, r, q)
    i, j, seg = R.pair_index(q, offs, rows)
    f64 = R.pair_features(xyz, nrm, i, j, np.float64)
    amb = R.ambiguous(f64)
    share = float(amb.any(1).mean()) if len(i) else 0.0
    print("r = %g: %d pairs, %.3f %% ambiguous" % (r, len(i), 100 * share))
    assert share <= 0.01
    c64, k64 = R.spfh_counts(xyz, nrm, q, offs, rows, feats=f64)
    c, k = device_counts(dev)
    assert np.array_equal(k[q], k64)
    allow = 2 * np.bincount(seg, amb.sum(1), minlength=len(q))
    diff = np.abs(c[q] - c64).sum(1)
    print("   points that differ from fp64: %d of %d (allowed to: %d)" % ((diff > 0).sum(), len(q), (allow > 0).sum()))
    assert np.all(diff <= allow)
    return offs, rows, d2


def check_fpfh_stage(dev, q, offs, rows, d2):
    """fpfh_out against the fp64 FPFH stage of the device's own SPFH.

    Bound.  With u = 2^-24, k = |N(i)| and all terms non-negative: w = fl(1 / d2) and fl(h * w) carry one rounding each and the
    k - 1 additions of a sum of non-negative terms at most (k - 1) u of the sum, so s[b] is within (k + 1) u of its value,
    relatively; t adds the block's 11 values (10 more roundings): within (k + 11) u; g = fl(100 / t) and fl(s[b] * g) add one
    rounding each.  fpfh[b] = s[b] * 100 / t is therefore within ((k + 1) + (k + 11) + 2) u = (2 k + 14) u of its value, and its
    value is at most 100: |dev - ref| <= 100 (k + 7) 2^-23 in the worst case, inside the bound asserted, 100 (k + 16) 2^-23.
    The sum of a block's 11 outputs: the same roundings, shared: the same bound."""
    ref = R.fpfh_from_spfh(dev["spfh"], offs, rows, d2)
    got = dev["fpfh"][q].astype(np.float64)
    assert np.isfinite(dev["fpfh"]).all()
    bound = 100.0 * (np.diff(offs) + 16) * 2.0 ** -23
    err = np.abs(got - ref)
    print("   FPFH stage: max |dev - ref| / bound = %.3f" % float((err / bound[:, None]).max(initial=0.0)))
    assert np.all(err <= bound[:, None])
    for f in range(3):
        t_ref = ref[:, 11 * f:11 * f + 11].sum(1)
        t = got[:, 11 * f:11 * f + 11].sum(1)
        full = t_ref > 0
        assert np.all(np.abs(t[full] - 100.0) <= bound[full])
        assert not got[~full, 11 * f:11 * f + 11].any()


@pytest.mark.parametrize("r", [5.53, 11.05])
def test_spfh_and_fpfh_cat(eng, cat, r):
    xyz, nrm = cat["src"], cat["src_n"]
    dev = eng.fpfh(xyz, nrm, r, want_spfh=True)
    q = np.arange(len(xyz))
    check_fpfh_stage(dev, q, *check_spfh(xyz, nrm, r, dev, q))


def test_spfh_and_fpfh_c4_surface_50k(eng, c4s):
    xyz, nrm = c4s["src"], c4s["src_n"]
    dev = eng.fpfh(xyz, nrm, 0.0138, want_spfh=True)
    q = np.arange(len(xyz))
    check_fpfh_stage(dev, q, *check_spfh(xyz, nrm, 0.0138, dev, q))


def test_spfh_and_fpfh_c4_surface_1m(eng, c4m):
    for r in c4m["radii"]:
        dev = eng.fpfh(c4m["xyz"], c4m["nrm"], r, want_spfh=True)
        check_fpfh_stage(dev, c4m["rows"], *check_spfh(c4m["xyz"], c4m["nrm"], r, dev, c4m["rows"]))


def test_fpfh_strided_and_free_function(sym, eng, cat):
    xyz, nrm = cat["src"], cat["src_n"]
    n = len(xyz)
    packed = eng.fpfh(xyz, nrm, 5.53, want_spfh=True)
    x4 = np.zeros((n, 4), F); x4[:, :3] = xyz
    n12 = np.zeros((n, 12), F); n12[:, 4:7] = nrm
    a = eng.fpfh_strided(x4, n12.reshape(-1)[4:], 5.53, (n, 4, 1, 12, 1))
    b = eng.fpfh_strided(np.asfortranarray(xyz).T.copy(), np.asfortranarray(nrm).T.copy(), 5.53, (n, 1, n, 1, n))
    c = sym.fpfh(xyz, nrm, 5.53, want_spfh=True)
    for other in (a, b, c):
        for key in ("fpfh", "spfh", "count"):
            assert np.array_equal(other[key], packed[key]), key
    assert np.array_equal(eng.fpfh(xyz, nrm, 5.53), packed["fpfh"])          # spfh_out == count_out == NULL


# ---- 4. edge inputs ---------------------------------------------------------------------------------------------------------------
def test_zero_normals_give_zero_histograms(sym, eng):
    xyz, nrm = sym.pcd_read(os.path.join(GOLDEN, "cat_out.pcd"))
    assert nrm is not None and not nrm.any()                # the file's own normal fields
    dev = eng.fpfh(xyz, nrm, 11.05, want_spfh=True)
    assert not dev["fpfh"].any() and not dev["spfh"].any()
    assert np.array_equal(dev["count"], R.radius_sets(xyz, 11.05)[0])


def test_nan_normals_drop_their_pairs_on_both_sides(eng, cat):
    xyz, nrm = cat["src"], cat["src_n"].copy()
    bad = np.arange(0, len(xyz), 7)
    nrm[bad] = np.nan
    dev = eng.fpfh(xyz, nrm, 5.53, want_spfh=True)
    assert np.isfinite(dev["fpfh"]).all() and np.isfinite(dev["spfh"]).all()
    assert not dev["spfh"][bad].any()                       # every pair of such a row is invalid
    q = np.arange(len(xyz))
    check_fpfh_stage(dev, q, *check_spfh(xyz, nrm, 5.53, dev, q))


def test_duplicates_isolated_points_and_extreme_radii(eng, cat):
    rng = np.random.default_rng(4)
    x = np.concatenate([cat["src"][:900], cat["src"][:200], [[1e4, 1e4, 1e4]]]).astype(F)
    nr = np.concatenate([cat["src_n"][:900], cat["src_n"][:200], [[0, 0, 1]]]).astype(F)
    perm = rng.permutation(len(x))
    x, nr = x[perm], nr[perm]
    q = np.arange(len(x))
    dev = eng.fpfh(x, nr, 5.53, want_spfh=True)
    check_fpfh_stage(dev, q, *check_spfh(x, nr, 5.53, dev, q))
    far = int(np.nonzero(perm == len(x) - 1)[0][0])
    assert dev["count"][far] == 0 and not dev["fpfh"][far].any() and not dev["spfh"][far].any()
    # a radius larger than the cloud: every point is a neighbour of every other
    y, ny = np.ascontiguousarray(cat["src"][:1500]), np.ascontiguousarray(cat["src_n"][:1500])
    dev = eng.fpfh(y, ny, 1e4, want_spfh=True)
    assert (dev["count"] == len(y) - 1).all()
    q = np.arange(len(y))
    check_fpfh_stage(dev, q, *check_spfh(y, ny, 1e4, dev, q))
    # a radius smaller than any spacing
    dev = eng.fpfh(y, ny, 1e-6, want_spfh=True)
    assert not dev["count"].any() and not dev["fpfh"].any() and not dev["spfh"].any()
    one = eng.fpfh(y[:1], ny[:1], 1.0, want_spfh=True)
    assert list(one["count"]) == [0] and not one["fpfh"].any()


def test_overflowing_weights_leave_no_nan_or_inf(eng):
    """two points 1e-20 apart (d2 ~ 1e-40, a positive subnormal: the weight 1 / d2 is not finite in fp32), with and without company"""
    x = np.array([[0, 0, 0], [1e-20, 0, 0]], F)
    nr = np.array([[0, 0, 1], [0, 1, 0]], F)
    dev = eng.fpfh(x, nr, 1.0, want_spfh=True)
    assert list(dev["count"]) == [1, 1]
    assert np.isfinite(dev["fpfh"]).all() and np.isfinite(dev["spfh"]).all() and not dev["fpfh"].any()
    x3 = np.array([[0, 0, 0], [1e-20, 0, 0], [0.5, 0.1, 0], [0.2, 0.4, 0.1]], F)
    n3 = np.array([[0, 0, 1], [0, 1, 0], [0, 0.6, 0.8], [0.6, 0, 0.8]], F)
    dev = eng.fpfh(x3, n3, 1.0, want_spfh=True)
    assert np.isfinite(dev["fpfh"]).all() and np.isfinite(dev["spfh"]).all()
    s = dev["fpfh"].reshape(4, 3, 11).sum(2)
    assert np.all((np.abs(s - 100.0) < 1e-3) | (s == 0.0))
    assert np.all(np.abs(s[2:] - 100.0) < 1e-3)              # the two ordinary points keep their histograms


# ---- 5. it does what it is for --------------------------------------------------------------------------------------------------
def test_features_find_the_counterpart_on_the_cat_pair(eng, cat):
    """cat.pcd and cat_out.pcd (the same cloud moved; row i <-> row i), normals estimated on each cloud alone (k = 10, viewpoint at
    the origin), FPFH at r = 11.05, every source row matched to the target row nearest in feature space: the share of matches within
    r of the true counterpart.  The fp64 numpy pipeline (reference normals, reference FPFH) is run next to it."""
    from scipy.spatial import cKDTree
    r = 11.05
    src, tgt = cat["src"], cat["tgt"]

    def share(fs, ft):
        j = cKDTree(ft).query(fs, 1)[1]
        d = np.linalg.norm(tgt[j].astype(np.float64) - tgt.astype(np.float64), axis=1)
        return float((d <= r).mean()), float((j == np.arange(len(src))).mean())

    dev = []
    for x in (src, tgt):
        nrm, _ = eng.estimate_normals(x, 10)
        dev.append(eng.fpfh(x, nrm, r).astype(np.float64))
    ref = []
    for x in (src, tgt):
        nrm, _ = K.emulate(x, K.knn(x, 10)[0])
        count, offs, rows, d2 = R.radius_sets(x, r)
        c, k = R.spfh_counts(x, nrm, np.arange(len(x)), offs, rows, np.float64)
        ref.append(R.fpfh_from_spfh(np.where(k[:, None] > 0, 100.0 * c / np.maximum(k, 1)[:, None], 0.0), offs, rows, d2))
    s_dev, s_ref = share(*dev), share(*ref)
    print("within r of the counterpart: device %.4f (the very row %.4f), fp64 reference %.4f (%.4f)" % (s_dev + s_ref))
    assert s_ref[0] > 0.9
    assert s_dev[0] >= s_ref[0] - 0.01


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------
def test_fpfh_is_deterministic_and_independent_of_the_context(sym, eng, cat, c4s):
    xyz, nrm = c4s["src"], c4s["src_n"]
    a = eng.fpfh(xyz, nrm, 0.0138, want_spfh=True)
    b = eng.fpfh(xyz, nrm, 0.0138, want_spfh=True)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        c = e.fpfh(xyz, nrm, 0.0138, want_spfh=True)
    with sym.Engine() as e:
        d = e.fpfh(xyz, nrm, 0.0138, want_spfh=True)
    for other in (b, c, d):
        assert np.array_equal(a["fpfh"].view(np.uint32), other["fpfh"].view(np.uint32))
        assert np.array_equal(a["spfh"].view(np.uint32), other["spfh"].view(np.uint32))
        assert np.array_equal(a["count"], other["count"])
