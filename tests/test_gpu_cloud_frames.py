"""The per-point cloud operations far from the origin, in a frame of exact ties and across units of length (tests/_cloud_frames.py has
the frames, fixtures, parameters and measured counts; tests/test_cloud_frames_ref.py asserts the conditions on the CPU):
knn, radius_search, fpfh, remove_statistical_outlier, remove_radius_outlier, cluster_dbscan, orient_normals, segment_plane,
evaluate_registration, ndt_map and voxel_downsample.

a. Frames.  The device's output against the operation's numpy reference at the shifted fp32 coordinates, through the checks of the
   operation's own test file (imported, not restated): bit for bit wherever those are.  In the tie frame the assertions are also shown to
   have bitten, from the device's output: the k-NN lists cut a tie in ascending caller row, the radius lists hold every d2 == r2 pair, a
   duplicate row is its twin's first neighbour at d2 == 0, FPFH stays finite over its 1 / 0 weights.  Every cap (tie counts, the ambiguous
   share) is asserted from the reference before the device's output is looked at.
b. Units.  A run on the cloud x 2^e with every length argument x 2^e against the run in the original unit: _cloud_frames.unit_*, which
   tests/test_cloud_frames_ref.py asserts of the references too.  Every scaling is an exact power of two: zero tolerance."""
import numpy as np
import pytest

import _cloud_frames as CF
import _eval_ref as E
import _fpfh_ref as R
import _frame_cases as FC
import _knn_ref as K
import _outlier_ref as X
import _segplane_ref as S
import test_gpu_cluster as TC
import test_gpu_eval as TE
import test_gpu_fpfh as TF
import test_gpu_ndt_map as TN
import test_gpu_orient as TOR
import test_gpu_outlier as TO
import test_gpu_segplane as TS
import test_gpu_voxel as TV
from test_gpu_fpfh import check_fpfh_stage, check_spfh

pytestmark = pytest.mark.gpu

f32 = np.float32
FRAMES = CF.FRAME_NAMES


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
def base(cat):
    """fixture -> its cloud in its own frame (the pair: a dict), with what rides along"""
    b = dict(cat=cat["src"], pair=CF.cat_pair(cat), scene=CF.scene(cat), floor=CF.floor(cat), ndt=CF.ndt_cloud(),
             nrm=cat["src_n"], signs=CF.random_signs(cat["src_n"]))
    b["eval_cases"] = CF.eval_cases(b["pair"])
    b["ror_min"] = int(np.median(R.radius_sets(b["cat"], CF.ROR_R)[0]))
    return b


@pytest.fixture(scope="module")
def frames(base):
    """(fixture, frame) -> (cloud, offset), and the cat's reference 22-NN lists and d2 matrix per frame, computed once and left unchanged"""
    cache = {}

    def get(fixture, name, what="cloud"):
        key = (fixture, name)
        if key not in cache:
            if fixture == "pair":
                d = CF.pair_frame(base["pair"], name)
                cache[key] = dict(cloud=(d, d["offset"]))
            else:
                cache[key] = dict(cloud=CF.frame(fixture, base[fixture], name))
        slot = cache[key]
        if what == "knn" and "knn" not in slot:
            slot["knn"] = K.knn(slot["cloud"][0], 22)
        if what == "d2" and "d2" not in slot:
            slot["d2"] = CF.d2_matrix(slot["cloud"][0])
        return slot[what]
    return get


# ---- a. far and tie frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", CF.KNN_K)
@pytest.mark.parametrize("name", FRAMES)
def test_knn(sym, eng, frames, name, k):
    x, _ = frames("cat", name)
    if k > CF.KNN_MAX:                                  # the entry's contract is 3 <= k <= 16: a refusal, and the context works on
        with pytest.raises(sym.SymmIcpError) as err:
            eng.knn(x, k)
        assert err.value.status == sym.ERR_ARG
        return
    rr, rd = frames("cat", name, "knn")
    tied = CF.kth_ties(rd, k)
    twins = frames("cat", name, "d2") == 0 if name == "tie" else None
    if name == "tie":
        assert tied.sum() >= CF.MIN_KTH_TIES and (twins.sum(1) > 1).sum() >= CF.MIN_DUPLICATES
    rows, d2 = eng.knn(x, k)
    assert np.array_equal(rows, rr[:, :k]), int((rows != rr[:, :k]).any(1).sum())
    assert np.array_equal(d2.view(np.uint32), rd[:, :k].view(np.uint32))
    if name != "tie":
        return
    # ... and from the device's own lists: a tie at the cut keeps the lowest caller rows, in ascending order
    m = frames("cat", name, "d2")
    for i in np.flatnonzero(tied).tolist():
        at = np.flatnonzero(m[i] == d2[i, k - 1])
        got = rows[i][d2[i] == d2[i, k - 1]]
        assert len(got) < len(at) and np.array_equal(got, at[:len(got)]), (i, got, at)
    # a duplicate row's list begins with the rows at its own place (itself among them), ascending, at d2 == 0
    for i in np.flatnonzero(twins.sum(1) > 1).tolist():
        at = np.flatnonzero(twins[i])[:k]
        assert np.array_equal(rows[i, :len(at)], at) and not d2[i, :len(at)].any(), (i, rows[i], at)


@pytest.mark.parametrize("r", CF.RADII + (CF.FPFH_R,))
@pytest.mark.parametrize("name", FRAMES)
def test_radius_search_sorted_and_unsorted(sym, eng, frames, name, r):
    x, _ = frames("cat", name)
    n = len(x)
    rc, ro, rrows, rd2 = R.radius_sets(x, r)
    r2 = f32(r) * f32(r)
    if name == "tie" and r in CF.RADII:
        assert CF.boundary_pairs((rc, ro, rrows, rd2), r) >= CF.MIN_BOUNDARY_PAIRS
    count, offs, rows, d2 = eng.radius_search(x, r, sort=True)                  # the lists in (d2, row) order: the reference's own
    assert np.array_equal(count, rc) and np.array_equal(offs, ro) and np.array_equal(rows, rrows)
    assert np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    TF.check_radius(sym, eng, x, r, dev=eng.radius_search(x, r, sort=False))    # the lists as the walk left them
    if name != "tie":
        return
    m = frames("cat", name, "d2")
    seg = np.repeat(np.arange(n), count)
    if r in CF.RADII:                                   # every pair at d2 == r2 is in the device's lists
        i, j = np.nonzero(m == r2)
        assert len(i) >= CF.MIN_BOUNDARY_PAIRS
        on = d2 == r2
        assert np.array_equal(np.sort(seg[on] * n + rows[on]), np.sort(i * n + j))
    # a duplicate row is its twin's first neighbour, at d2 == 0
    twins = m == 0
    dup = np.flatnonzero(twins.sum(1) > 1)
    assert len(dup) >= CF.MIN_DUPLICATES
    for i in dup.tolist():
        at = np.flatnonzero(twins[i])
        at = at[at != i]
        assert np.array_equal(rows[offs[i]:offs[i] + len(at)], at) and not d2[offs[i]:offs[i] + len(at)].any(), i


@pytest.mark.parametrize("name", FRAMES)
def test_fpfh(eng, base, frames, name):
    x, _ = frames("cat", name)
    dev = eng.fpfh(x, base["nrm"], CF.FPFH_R, want_spfh=True)
    q = np.arange(len(x))
    offs, rows, d2 = check_spfh(x, base["nrm"], CF.FPFH_R, dev, q)              # (asserts the ambiguous share before it looks at dev)
    check_fpfh_stage(dev, q, offs, rows, d2)
    if name == "tie":                                   # pairs at d2 == 0: the weight 1 / 0 is met, and nothing of it is left
        assert (d2 == 0).sum() >= CF.MIN_DUPLICATES
        assert np.isfinite(dev["fpfh"]).all() and np.isfinite(dev["spfh"]).all()


@pytest.mark.parametrize("k,std_mul", CF.SOR)
@pytest.mark.parametrize("name", FRAMES)
def test_remove_statistical_outlier(eng, frames, name, k, std_mul):
    x, _ = frames("cat", name)
    if name == "tie":
        assert CF.kth_ties(frames("cat", name, "knn")[1], k + 1).sum() >= CF.MIN_KTH_TIES
    dev = TO.check_exact(eng, x, k, std_mul)
    assert 0 < len(dev["rows"]) < len(x)


@pytest.mark.parametrize("name", FRAMES)
def test_remove_radius_outlier(eng, frames, name):
    x, _ = frames("cat", name)
    sets = R.radius_sets(x, CF.ROR_R)
    mn = int(np.median(sets[0]))
    ref = X.radius(x, CF.ROR_R, mn)
    if name == "tie":                                   # pairs at d2 == r2: each is one neighbour more of its row
        assert CF.boundary_pairs(sets, CF.ROR_R) >= CF.MIN_BOUNDARY_PAIRS
    dev = eng.remove_radius_outlier(x, CF.ROR_R, mn, return_counts=True)
    assert np.array_equal(dev["neighbors"], ref["neighbors"])
    assert dev["rows"].dtype == np.int32 and np.array_equal(dev["rows"], ref["rows"]) and 0 < len(dev["rows"]) < len(x)


@pytest.mark.parametrize("min_points", CF.SCENE_MIN_POINTS)
@pytest.mark.parametrize("name", FRAMES + ("tie, eps on the lattice",))
def test_cluster_dbscan(eng, frames, name, min_points):
    eps = CF.TIE_EPS if "," in name else CF.SCENE_EPS
    x, _ = frames("scene", name.split(",")[0])
    dev = TC.check_exact(eng, x, eps, min_points)
    assert dev["clusters"] > 1


@pytest.mark.parametrize("rule", ["viewpoint", "direction"])
@pytest.mark.parametrize("k", CF.ORIENT_K)
@pytest.mark.parametrize("name", FRAMES)
def test_orient_normals(eng, base, frames, name, k, rule):
    x, off = frames("cat", name)
    rr, rd = frames("cat", name, "knn")
    if name == "tie":
        assert CF.kth_ties(rd, k).sum() >= CF.MIN_KTH_TIES
    seed = dict(viewpoint=CF.shifted_point(CF.VIEWPOINT, off)) if rule == "viewpoint" else dict(direction=CF.DIRECTION_RULE)
    TOR.check_exact(eng, x, base["signs"], k, rows=rr[:, :k], **seed)


@pytest.mark.parametrize("name", FRAMES + ("tie, max_dist on the lattice",))
def test_segment_plane(sym, eng, frames, name):
    """through plane_hypotheses (every status and the four floats, in TS.check) and the full result with one refit"""
    md = CF.TIE_MAX_DIST if "," in name else S.MAX_DIST
    x, _ = frames("floor", name.split(",")[0])
    ref = S.segment(x, md, CF.PLANE_H, 0, 1)
    assert ref["status"] == S.OK and S.margin(ref, md) > 1e-6                  # test_floor_scene's condition for equal rows
    if "," in name:
        assert CF.plane_boundary_pairs(x, ref, md) >= CF.MIN_FIXTURE_BOUNDARY
    r, _ = TS.check(sym, eng, x, md, CF.PLANE_H, seed=0, refits=1)
    assert r["status"] == sym.OK and r["inliers_final"] > 1000


@pytest.mark.parametrize("name", FRAMES)
def test_evaluate_registration(eng, frames, name):
    d, off = frames("pair", name)
    for which, Xf, D in CF.eval_cases(d, off):
        full = E.evaluate(d["src"], d["tgt"], Xf, D)
        r = eng.evaluate_registration(d["src"], d["tgt"], Xf, D, want_pairs=True)
        TE.check_pairs(r, full, (name, which, D))
        TE.check_sums(r, full, (name, which, D))
        assert 0 < r["inliers"] and (D == 0.0 or r["inliers"] < len(d["src"]))


@pytest.mark.parametrize("name", FRAMES)
def test_ndt_map(eng, frames, name):
    x, _ = frames("ndt", name)
    ref = TN.check_map(eng.ndt_map(x, CF.NDT_RES), x, CF.NDT_RES, tag=name)
    assert len(ref["key"]) > 10


def test_voxel_downsample_in_the_tie_frame(eng, base, frames):
    x, _ = frames("cat", "tie")
    dev = TV.check(eng, x, CF.VOXEL_LEAF, base["nrm"])
    assert 1 < len(dev["xyz"]) < len(x)


# ---- b. units -------------------------------------------------------------------------------------------------------------------------------
def dev_knn(sym, eng, x, b, e):
    return [eng.knn(x, k) for k in CF.KNN_K if k <= CF.KNN_MAX]


def dev_radius(sym, eng, x, b, e):
    return [eng.radius_search(x, CF.length(r, e), sort=s) for r in CF.RADII + (CF.FPFH_R,) for s in (True, False)]


def dev_fpfh(sym, eng, x, b, e):
    return eng.fpfh(x, b["nrm"], CF.length(CF.FPFH_R, e), want_spfh=True)


def dev_sor(sym, eng, x, b, e):
    return [eng.remove_statistical_outlier(x, k, mul, return_stats=True) for k, mul in CF.SOR]


def dev_ror(sym, eng, x, b, e):
    return eng.remove_radius_outlier(x, CF.length(CF.ROR_R, e), b["ror_min"], return_counts=True)


def dev_cluster(sym, eng, x, b, e):
    return [eng.cluster_dbscan(x, CF.length(eps, e), mp, return_info=True) for eps in (CF.SCENE_EPS, CF.TIE_EPS) for mp in CF.SCENE_MIN_POINTS]


def dev_orient(sym, eng, x, b, e):
    return [eng.orient_normals(x, b["signs"], k, return_info=True, **seed) for k in CF.ORIENT_K
            for seed in (dict(viewpoint=CF.lengths(CF.VIEWPOINT, e)), dict(direction=CF.DIRECTION_RULE))]


def dev_plane(sym, eng, x, b, e):
    out = []
    for md in (S.MAX_DIST, CF.TIE_MAX_DIST):
        hy = eng.plane_hypotheses(x, sym.plane_config(CF.length(md, e), CF.PLANE_H, 0, 1))
        out.append((eng.segment_plane(x, CF.length(md, e), CF.PLANE_H, 0, 1, return_info=True), (hy["hyp_status"], hy["hyp"], hy["pivot"])))
    return out


def dev_eval(sym, eng, d, b, e):
    return [eng.evaluate_registration(d["src"], d["tgt"], FC.scaled_transform(Xf, 2.0 ** e), CF.length(D, e), want_pairs=True)
            for _, Xf, D in b["eval_cases"]]


def dev_ndt(sym, eng, x, b, e):
    return eng.ndt_map(x, CF.length(CF.NDT_RES, e))


def dev_voxel(sym, eng, x, b, e):
    return eng.voxel_downsample(x, CF.length(CF.VOXEL_LEAF, e), b["nrm"])


def each(compare):
    return lambda a, b, e: [compare(u, v, e) for u, v in zip(a, b)]


def plane_units(a, b, e):
    for (ra, ha), (rb, hb) in zip(a, b):
        CF.unit_hypotheses(ha, hb, e)
        CF.unit_segment(ra, rb, e)


# op -> (fixture, the device run, the unit assertion of _cloud_frames)
OPS = {
    "knn": ("cat", dev_knn, each(CF.unit_knn)),
    "radius_search": ("cat", dev_radius, each(CF.unit_radius)),
    "fpfh": ("cat", dev_fpfh, CF.unit_fpfh),
    "remove_statistical_outlier": ("cat", dev_sor, each(CF.unit_sor)),
    "remove_radius_outlier": ("cat", dev_ror, CF.unit_ror),
    "cluster_dbscan": ("scene", dev_cluster, each(CF.unit_cluster)),
    "orient_normals": ("cat", dev_orient, each(CF.unit_orient)),
    "segment_plane": ("floor", dev_plane, plane_units),
    "evaluate_registration": ("pair", dev_eval, each(CF.unit_eval)),
    "ndt_map": ("ndt", dev_ndt, CF.unit_ndt),
    "voxel_downsample": ("cat", dev_voxel, CF.unit_voxel),
}


@pytest.fixture(scope="module")
def original(sym, eng, base):
    """op -> the device's run in the original unit, made once per operation and left unchanged"""
    cache = {}

    def get(op):
        if op not in cache:
            fixture, run, _ = OPS[op]
            cache[op] = run(sym, eng, base[fixture], base, 0)
        return cache[op]
    return get


@pytest.mark.parametrize("e", CF.UNIT_EXPONENTS)
@pytest.mark.parametrize("op", list(OPS))
def test_units(sym, eng, base, original, op, e):
    fixture, run, compare = OPS[op]
    x = FC.scaled(base["pair"], 2.0 ** e) if fixture == "pair" else CF.scaled(base[fixture], e)
    compare(original(op), run(sym, eng, x, base, e), e)
