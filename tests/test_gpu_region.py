"""Region-growing segmentation on the device (symmicp_ctx_region_growing; kernels_region.hip) against tests/_region_ref.py.

The comparison is EXACT: labels, region count, sizes, seed and smooth equal.  The neighbourhoods are the exact fp32 sets of the radius
search, the smoothness test is one fp32 expression in a fixed association, a component's representative is its minimum seed row whatever
the order in which the unions arrived, and the border key is a minimum: a mismatch is a kernel bug, not a tolerance question."""
import numpy as np
import pytest

import _cluster_ref as CR
import _region_ref as G

pytestmark = pytest.mark.gpu

F = np.float32
SP = CR.CAT_SPACING
H = 2.0 ** -4                  # the corner's lattice spacing
CAT_SETTINGS = [(3, 15.0, 0.05), (2, 30.0, 0.05), (4, 10.0, 0.02)]      # (spacings, degrees, curvature threshold)


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
def corner():
    return G.corner(12, H)


@pytest.fixture(scope="module")
def cat_ref(cat):
    """the reference on the cat at the pinned setting (3 spacings, 15 degrees, 0.05), computed once"""
    return G.region_growing(cat["src"], cat["src_n"], 3 * SP, G.cos_of(15), cat["golden"]["src_curv"], 0.05)


def same(dev, ref):
    assert dev["labels"].dtype == np.int32 and dev["sizes"].dtype == np.int32 and dev["smooth"].dtype == np.int32
    bad = np.nonzero(dev["labels"] != ref["labels"])[0]
    assert len(bad) == 0, (len(bad), bad[:8], dev["labels"][bad[:8]], ref["labels"][bad[:8]])
    assert dev["regions"] == ref["regions"] and np.array_equal(dev["sizes"], ref["sizes"])
    assert np.array_equal(dev["seed"], ref["seed"]) and np.array_equal(dev["smooth"], ref["smooth"])


def run_cos(sym, eng, x, nr, eps, cos, curv=None, thr=0.05, lo=0, hi=0):
    """the device at an exact smoothness_cos (the raw entry, cap = n) -> the dict of Engine.region_growing(..., return_info=True)"""
    cfg = sym.region_config(eps, curvature_threshold=thr, min_region_size=lo, max_region_size=hi, smoothness_cos=cos)
    st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(x, nr, curv, cfg, cap=len(x))
    assert st == sym.OK
    return dict(labels=labels, regions=regions, sizes=sizes[:regions].copy(), seed=seed.astype(bool), smooth=smooth)


def check_exact(eng, x, nr, eps, deg, curv=None, thr=0.05, lo=0, hi=0):
    """the device's whole result against the reference's; returns the device's"""
    dev = eng.region_growing(x, nr, eps, deg, curv, thr, lo, hi, return_info=True)
    same(dev, G.region_growing(x, nr, eps, G.cos_of(deg), curv, thr, lo, hi))
    return dev


# ---- 1. the answers written down by hand ---------------------------------------------------------------------------------------------
def test_one_point(eng):
    x, nr = np.zeros((1, 3), F), np.array([[0, 0, 1]], F)
    dev = check_exact(eng, x, nr, 1.0, 30.0)
    assert dev["labels"].tolist() == [0] and dev["sizes"].tolist() == [1] and dev["smooth"].tolist() == [0]
    dev = check_exact(eng, x, nr, 1.0, 30.0, np.array([1.0], F))
    assert dev["labels"].tolist() == [-1] and dev["regions"] == 0 and not dev["seed"].any()


def test_two_points_at_the_exact_bound(sym, eng):
    x = CR.line([0.0, 1.0])
    nr = np.array([[1, 0, 0], [0.5, 0.8660254, 0]], F)
    for cos, want in ((F(0.5), [0, 0]), (np.nextafter(F(0.5), F(1)), [0, 1])):
        dev = run_cos(sym, eng, x, nr, 1.5, cos)
        same(dev, G.region_growing(x, nr, 1.5, cos))
        assert dev["labels"].tolist() == want
    # d2 == r2 exactly is a member; just below it is not
    x = np.array([[0, 0, 0], [3, 4, 0]], F)
    nr = np.tile(np.array([[0, 0, 1]], F), (2, 1))
    for eps, want in ((F(5), [0, 0]), (np.nextafter(F(5), F(0)), [0, 1])):
        dev = run_cos(sym, eng, x, nr, eps, F(1))
        same(dev, G.region_growing(x, nr, eps, F(1)))
        assert dev["labels"].tolist() == want


def test_corner_is_one_cluster_and_three_regions(eng, corner):
    """the test that shows the feature: one Euclidean cluster, three regions = the three faces"""
    x, nr, face = corner
    assert eng.cluster_dbscan(x, 1.5 * H, 1, return_info=True)["clusters"] == 1
    dev = check_exact(eng, x, nr, 1.5 * H, 10.0)
    assert dev["regions"] == 3 and dev["sizes"].tolist() == [144, 132, 121] and np.array_equal(dev["labels"], face)
    assert dev["seed"].all() and (dev["labels"] >= 0).all()
    # a caller-made curvature makes the 34 edge rows non-seeds: border rows of the face their normal belongs to
    cv = G.edge_curvature(x, H)
    dev = check_exact(eng, x, nr, 1.5 * H, 10.0, cv)
    assert (~dev["seed"]).sum() == 34 and dev["sizes"].tolist() == [144, 132, 121] and np.array_equal(dev["labels"], face)
    # every row a non-seed: nothing is labelled
    dev = check_exact(eng, x, nr, 1.5 * H, 10.0, np.ones(len(x), F))
    assert (dev["labels"] == -1).all() and dev["regions"] == 0 and len(dev["sizes"]) == 0


@pytest.mark.parametrize("moved,reverse", [(False, False), (False, True), (True, False), (True, True)])
def test_border_row_on_the_edge(eng, moved, reverse):
    """_region_ref.border_case: a bit-equal d2 goes to the lower representative, a nearer seed wins (tests/test_region_ref.py asserts
    which face that is from the reference alone)"""
    x, nr, cv, face, row = G.border_case(moved)
    if reverse:
        x, nr, cv, face, row = x[::-1].copy(), nr[::-1].copy(), cv[::-1].copy(), face[::-1], len(x) - 1 - row
    dev = check_exact(eng, x, nr, 1.5 * H, 50.0, cv)
    other = int(np.nonzero((face == (1 if moved or reverse else 2)) & dev["seed"])[0][0])      # a seed of the face it must NOT join
    joined = int(dev["labels"][row])
    assert dev["regions"] == 3 and joined >= 0 and joined != dev["labels"][other]
    assert check_exact(eng, x, nr, 1.5 * H, 40.0, cv)["labels"][row] == -1


def test_sign_flips_change_nothing(eng, cat, cat_ref):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    sign = np.where(np.random.default_rng(0).random(len(x)) < 0.5, F(-1), F(1))
    a = eng.region_growing(x, nr, 3 * SP, 15.0, cv, return_info=True)
    b = eng.region_growing(x, nr * sign[:, None], 3 * SP, 15.0, cv, return_info=True)
    same(a, cat_ref)
    for key in ("labels", "sizes", "seed", "smooth"):
        assert a[key].tobytes() == b[key].tobytes(), key


# ---- 2. exactness on real clouds -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,deg,thr", CAT_SETTINGS)
def test_cat_is_exact(eng, cat, m, deg, thr):
    dev = check_exact(eng, cat["src"], cat["src_n"], m * SP, deg, cat["golden"]["src_curv"], thr)
    border, unlabelled = int((~dev["seed"] & (dev["labels"] >= 0)).sum()), int((dev["labels"] < 0).sum())
    print("cat at (%g spacings, %g degrees, %g): %d regions, largest %d, %d border rows, %d unlabelled" % (
        m, deg, thr, dev["regions"], dev["sizes"].max(), border, unlabelled))
    if (m, deg, thr) == CAT_SETTINGS[0]:
        assert (dev["regions"], int(dev["sizes"].max()), border, unlabelled) == (321, 1708, 312, 548)      # tests/test_region_ref.py's pins
    assert dev["regions"] > 10 and border > 0 and unlabelled > 0


def test_cat_without_curvature_is_exact(eng, cat):
    dev = check_exact(eng, cat["src"], cat["src_n"], 3 * SP, 15.0)
    assert dev["seed"].all() and (dev["labels"] >= 0).all() and dev["sizes"].sum() == 3400 and dev["regions"] > 100


def test_bunny_is_exact(eng, bunny):
    import _fpfh_ref as R
    nr, cv = eng.estimate_normals(bunny, 10)
    thr = float(np.quantile(cv, 0.9))                                    # (the scan is smooth: a tenth of its rows are made non-seeds)
    dev = check_exact(eng, bunny, nr, 4 * R.median_spacing(bunny, np.arange(len(bunny))), 20.0, cv, thr)
    assert dev["regions"] >= 1 and (~dev["seed"]).sum() >= len(bunny) // 20


def test_row_order_does_not_matter(eng, cat, cat_ref):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    perm = np.random.default_rng(9).permutation(len(x))
    b = check_exact(eng, x[perm], nr[perm], 3 * SP, 15.0, cv[perm])
    back = np.empty(len(x), np.int32)
    back[perm] = b["labels"]
    assert G.partition(back) == G.partition(cat_ref["labels"])
    assert np.array_equal(b["seed"], cat_ref["seed"][perm]) and np.array_equal(b["smooth"], cat_ref["smooth"][perm])
    assert G.numbering_is_by_lowest_seed_row(b["labels"], b["seed"])
    assert sorted(np.unique(b["labels"][b["labels"] >= 0]).tolist()) == list(range(b["regions"]))


def test_strided_inputs(sym, eng, cat, cat_ref):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    n = len(x)
    cfg = sym.region_config(3 * SP, 15.0, 0.05)
    x4 = np.zeros((n, 4), F); x4[:, :3] = x
    n5 = np.zeros((n, 5), F); n5[:, :3] = nr
    c3 = np.full((n, 3), np.nan, F); c3[:, 0] = cv                      # (a NaN the stride skips)
    xcm, ncm = np.asfortranarray(x).T.copy(), np.asfortranarray(nr).T.copy()
    both = np.concatenate([x, nr], 1)                                    # one buffer of x y z nx ny nz records
    for xb, nb, cb, strides in ((x4, n5, c3, (n, 4, 1, 5, 1, 3)), (xcm, ncm, cv, (n, 1, n, 1, n, 1)), (both, both.reshape(-1)[3:], cv, (n, 6, 1, 6, 1, 1))):
        st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(xb, nb, cb, cfg, cap=n, strides=strides)
        assert st == sym.OK
        same(dict(labels=labels, regions=regions, sizes=sizes[:regions], seed=seed.astype(bool), smooth=smooth), cat_ref)


# ---- 3. the identity with Euclidean clustering ---------------------------------------------------------------------------------------
def test_smoothness_zero_is_euclidean_clustering(sym, eng, cat):
    scene = CR.scene(cat["src"])
    rng = np.random.default_rng(2)
    for x, eps, clusters in ((cat["src"], 3 * SP, 8), (scene, 3 * SP, None)):
        nr = rng.standard_normal((len(x), 3)).astype(F)                  # any normals: at smoothness_cos = 0 every edge is smooth
        c = eng.cluster_dbscan(x, eps, 1, return_info=True)
        r = run_cos(sym, eng, x, nr, eps, 0.0)
        assert clusters is None or c["clusters"] == clusters
        assert r["labels"].tobytes() == c["labels"].tobytes() and r["sizes"].tobytes() == c["sizes"].tobytes() and r["regions"] == c["clusters"]
        assert np.array_equal(r["smooth"], c["neighbors"]) and r["seed"].all()


# ---- 4. shapes that stress the union ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_chain_of_slowly_turning_normals(eng, order):
    """4 096 points whose normals turn by 1 degree per link: the ends are far more than 90 degrees apart, and it is ONE region at 2
    degrees; with one link of 5 degrees it is two"""
    n = 4096
    perm = dict(ascending=np.arange(n), descending=np.arange(n)[::-1], shuffled=np.random.default_rng(4).permutation(n))[order]
    x, nr = G.chain(n, 1.0)
    assert G.smooth_dot(nr[0], nr[90]) < 1e-6 and G.smooth_dot(nr[0], nr[1]) > G.cos_of(2)      # 90 links on: orthogonal
    dev = check_exact(eng, x[perm].copy(), nr[perm].copy(), 1.5, 2.0)
    assert dev["regions"] == 1 and not dev["labels"].any() and dev["sizes"].tolist() == [n]
    step = np.ones(n - 1)
    step[1500] = 5.0
    x, nr = G.chain(n, step)
    dev = check_exact(eng, x[perm].copy(), nr[perm].copy(), 1.5, 2.0)
    back = np.empty(n, np.int32)
    back[perm] = dev["labels"]
    assert dev["regions"] == 2 and sorted(dev["sizes"].tolist()) == [1501, n - 1501]
    assert len(set(back[:1501].tolist())) == 1 and len(set(back[1501:].tolist())) == 1 and back[0] != back[-1]


def test_coincident_points_with_interleaved_regions(eng):
    x, nr = G.interleaved(2048)
    dev = check_exact(eng, x, nr, 0.5, 30.0)
    assert dev["regions"] == 2 and dev["sizes"].tolist() == [1024, 1024] and dev["labels"].tolist() == [0, 1] * 1024      # representatives 0 and 1
    assert (dev["smooth"] == 1023).all()


def test_lattice_twice(eng):
    x, nr = G.lattice(64)
    a = check_exact(eng, x, nr, 1.0, 30.0)
    b = eng.region_growing(x, nr, 1.0, 30.0, return_info=True)
    assert a["regions"] == 1 and not a["labels"].any() and a["sizes"].tolist() == [4096]
    for key in ("labels", "sizes", "seed", "smooth"):
        assert a[key].tobytes() == b[key].tobytes(), key


# ---- 5. size filter, cap protocol, optional outputs ----------------------------------------------------------------------------------------
def test_size_filter(eng, cat, cat_ref):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    for lo, hi in ((5, 0), (0, 100), (5, 100), (1708, 1708)):
        dev = check_exact(eng, x, nr, 3 * SP, 15.0, cv, 0.05, lo, hi)
        assert np.array_equal(dev["sizes"], np.bincount(dev["labels"][dev["labels"] >= 0], minlength=dev["regions"]))
        assert np.array_equal(dev["seed"], cat_ref["seed"]) and np.array_equal(dev["smooth"], cat_ref["smooth"])      # before the filter
        assert 0 < dev["regions"] < cat_ref["regions"]
        assert all((lo == 0 or s >= lo) and (hi == 0 or s <= hi) for s in dev["sizes"].tolist())


def test_cap_protocol(sym, eng, cat, cat_ref):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    cfg = sym.region_config(3 * SP, 15.0, 0.05)
    r = cat_ref["regions"]
    written = lambda labels, seed, smooth: np.array_equal(labels, cat_ref["labels"]) and np.array_equal(seed.astype(bool), cat_ref["seed"]) and \
        np.array_equal(smooth, cat_ref["smooth"])
    st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(x, nr, cv, cfg)                 # sizes_out == NULL, cap 0
    assert st == sym.ERR_SIZE and regions == r and sizes is None and written(labels, seed, smooth)
    st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(x, nr, cv, cfg, cap=r - 1)
    assert st == sym.ERR_SIZE and regions == r and (sizes == -1).all() and written(labels, seed, smooth)      # the sizes are not written, the rest is
    st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(x, nr, cv, cfg, cap=r)
    assert st == sym.OK and regions == r and np.array_equal(sizes, cat_ref["sizes"]) and written(labels, seed, smooth)
    # no region at all: the count query succeeds
    st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(x, nr, cv, sym.region_config(3 * SP, 15.0, -1.0))
    assert st == sym.OK and regions == 0 and (labels == -1).all() and not seed.any()
    for bad in (dict(eps=-1.0), dict(smoothness_cos=1.5), dict(curvature_threshold=float("nan")), dict(min_region_size=-1),
                dict(min_region_size=9, max_region_size=8)):
        assert eng.region_growing_raw(x, nr, cv, sym.region_config(**dict(dict(eps=3 * SP), **bad)), cap=r)[0] == sym.ERR_ARG
    with pytest.raises(sym.SymmIcpError) as e:
        eng.region_growing(x, nr, float("nan"))
    assert e.value.status == sym.ERR_ARG
    assert eng.region_growing_raw(x, nr, cv, cfg, cap=r)[0] == sym.OK                                  # ... and the context still works


def test_optional_outputs_and_one_shot_form(sym, eng, cat, cat_ref):
    """seed_out and smooth_out NULL (the count walk is not launched): the same labels and sizes; the one-shot entry gives them too"""
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    cfg = sym.region_config(3 * SP, 15.0, 0.05)
    st, labels, regions, sizes, seed, smooth = eng.region_growing_raw(x, nr, cv, cfg, cap=len(x), want=False)
    assert st == sym.OK and seed is None and smooth is None
    assert labels.tobytes() == cat_ref["labels"].tobytes() and regions == cat_ref["regions"] and np.array_equal(sizes[:regions], cat_ref["sizes"])
    assert np.array_equal(eng.region_growing(x, nr, 3 * SP, 15.0, cv), cat_ref["labels"])
    same(sym.region_growing(x, nr, 3 * SP, 15.0, cv, return_info=True), cat_ref)
    parts = sym.clusters_from_labels(cat_ref["labels"])
    assert len(parts) == cat_ref["regions"] and len(parts[0]) == 1708


# ---- 6. the context is left untouched ---------------------------------------------------------------------------------------------------
def test_context_with_clouds_is_left_untouched(sym, cat, cat_ref, corner):
    """two contexts run the same passes; one of them grows regions on other clouds between two steps: every record, the transform, the
    pairs and index_info are identical, and what the region growing returns on it is the reference's"""
    got = {}

    def passes(between):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            out = [e.begin(), e.step()]
            info = e.index_info()
            if between:
                got["cat"] = e.region_growing(cat["src"], cat["src_n"], 3 * SP, 15.0, cat["golden"]["src_curv"], return_info=True)
                got["corner"] = e.region_growing(corner[0], corner[1], 1.5 * H, 10.0)
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
    same(got["cat"], cat_ref)
    assert np.array_equal(got["corner"], corner[2])


# ---- 7. regions into batch_align ---------------------------------------------------------------------------------------------------------
def test_pack_regions_into_batch_align(sym, eng, corner):
    """the corner and a slightly moved copy of it: both are segmented and packed, face k is aligned to face k in ONE batch of three
    problems, and every problem's result struct is byte-equal to the same problem run alone"""
    from symmicp import synth
    x, nr, face = corner
    motion = synth.rigid4(synth.rotation(1.0, (0.2, -0.4, 0.9)), np.array([0.1, -0.05, 0.08]) * H)
    y = (x.astype(np.float64) @ motion[:3, :3].T + motion[:3, 3]).astype(F)
    ny = (nr.astype(np.float64) @ motion[:3, :3].T).astype(F)
    lx, ly = eng.region_growing(x, nr, 1.5 * H, 10.0), eng.region_growing(y, ny, 1.5 * H, 10.0)
    assert np.array_equal(lx, face) and np.array_equal(ly, face)
    ps, pt = sym.pack_clusters(x, nr, lx), sym.pack_clusters(y, ny, ly)
    assert ps["skipped"] == [] and ps["labels"].tolist() == [0, 1, 2] and ps["ranges"][:, 1].tolist() == [144, 132, 121]
    assert np.array_equal(ps["xyz"], x[ps["rows"]]) and np.array_equal(pt["ranges"], ps["ranges"])
    probs = [(int(ps["ranges"][k, 0]), int(ps["ranges"][k, 1]), int(pt["ranges"][k, 0]), int(pt["ranges"][k, 1])) for k in range(3)]
    cfg = dict(mode=sym.MODE_P2P, max_iters=10)
    whole = eng.batch_align(ps["xyz"], ps["nrm"], pt["xyz"], pt["nrm"], probs, **cfg)
    assert len(whole) == 3
    for k in range(3):
        alone = eng.batch_align(ps["xyz"], ps["nrm"], pt["xyz"], pt["nrm"], [probs[k]], **cfg)
        assert alone[0]["raw"] == whole[k]["raw"], k
        print("face %d (%d points): status %d, diff %.3g -> %.3g" % (k, probs[k][1], whole[k]["status"], whole[k]["diff_initial"], whole[k]["diff_final"]))
