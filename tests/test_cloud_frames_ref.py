"""CPU: the conditions of the cloud-operation frame tests (tests/_cloud_frames.py), asserted from the numpy references alone, so that
tests/test_gpu_cloud_frames.py cannot pass on vacuous inputs:

  * the far frames hold no duplicate rows; the tie frames hold the duplicates, the ties at the k-th distance and the pairs at d2 == r2
    that the tie rules and the `<=` are decided on (thresholds in _cloud_frames, counts printed and recorded in its docstring);
  * the FPFH reference stays usable: at most 1 % of its pairs are ambiguous in every frame;
  * every reference runs in every frame, and is equivariant under a power-of-two unit exactly as the GPU file asserts of the device:
    the unit assertions are properties of the definitions, not of the kernels."""
import numpy as np
import pytest

import _cloud_frames as CF
import _cluster_ref as CR
import _eval_ref as E
import _fpfh_ref as R
import _frame_cases as FC
import _knn_ref as K
import _ndt_ref as N
import _orient_ref as OR
import _outlier_ref as X
import _segplane_ref as S
import _voxel_ref as V

f32 = np.float32


@pytest.fixture(scope="module")
def base(cat):
    """fixture -> its cloud in its own frame (the pair: a dict)"""
    return dict(cat=cat["src"], pair=CF.cat_pair(cat), scene=CF.scene(cat), floor=CF.floor(cat), ndt=CF.ndt_cloud(),
                nrm=cat["src_n"], signs=CF.random_signs(cat["src_n"]))


# ---- the frames ---------------------------------------------------------------------------------------------------------------------------
def test_far_frames_hold_no_duplicate_rows(base):
    for fixture in ("cat", "scene", "floor", "ndt"):
        for name in CF.FRAME_NAMES[:2]:
            x, _ = CF.frame(fixture, base[fixture], name)
            dup = CF.duplicate_rows(x)
            print("%s at %g extents: %d duplicate rows" % (fixture, CF.OFFSETS[fixture][CF.FRAME_NAMES.index(name)], dup))
            assert dup == 0, (fixture, name)
    for name in CF.FRAME_NAMES[:2]:
        d = CF.pair_frame(base["pair"], name)
        assert CF.duplicate_rows(d["src"]) == 0 and CF.duplicate_rows(d["tgt"]) == 0, name


def cat_counts(x):
    d2 = K.knn(x, 22)[1]
    ties = {k: int(CF.kth_ties(d2, k).sum()) for k in (10, 16, 17, 20, 21)}
    edge = {r: CF.boundary_pairs(R.radius_sets(x, r), r) for r in CF.RADII}
    return CF.duplicate_rows(x), ties, edge


def test_tie_frame_of_the_cat(base):
    """the docstring's first table, and its thresholds at the cat's tie frame"""
    tie = CF.OFFSETS["cat"][2]
    for o in (0.0, 1e3, 1e4, CF.TIE, tie):
        dup, ties, edge = cat_counts(CF.shifted(base["cat"], o)[0])
        print("o = %g: %d duplicate rows; rows tied at the k-th d2 %s; ordered pairs at d2 == r2 %s" % (o, dup, ties, edge))
    assert dup >= CF.MIN_DUPLICATES
    assert all(v >= CF.MIN_KTH_TIES for v in ties.values()), ties
    assert all(v >= CF.MIN_BOUNDARY_PAIRS for v in edge.values()), edge


def test_tie_frame_of_the_pair(base):
    d = CF.pair_frame(base["pair"], "tie")
    dups = CF.duplicate_rows(d["src"]), CF.duplicate_rows(d["tgt"])
    # the evaluation's own tie: a moved source row with two or more target rows at its smallest d2 (the lowest row must win)
    y = E.move(np.eye(4, dtype=f32), d["src"])
    m = K._d2(y, d["tgt"])
    tied = int(((m == m.min(1, keepdims=True)).sum(1) > 1).sum())
    print("the pair at %g extents: %d / %d duplicate rows, %d source rows with tied nearest targets" % (CF.OFFSETS["pair"][2], dups[0], dups[1], tied))
    assert min(dups) >= CF.MIN_DUPLICATES and tied >= CF.MIN_DUPLICATES


def test_tie_frame_of_the_scene(base):
    x, _ = CF.frame("scene", base["scene"], "tie")
    own = CF.boundary_pairs(R.radius_sets(x, CF.SCENE_EPS), CF.SCENE_EPS)
    sets = R.radius_sets(x, CF.TIE_EPS)
    edge = CF.boundary_pairs(sets, CF.TIE_EPS)
    print("the scene at %g extents: %d duplicate rows; pairs at d2 == r2: %d at eps %.4f, %d at eps %g (median %d neighbours)" % (
        CF.OFFSETS["scene"][2], CF.duplicate_rows(x), own, CF.SCENE_EPS, edge, CF.TIE_EPS, np.median(sets[0])))
    assert f32(CF.TIE_EPS) * f32(CF.TIE_EPS) == 9.0 and not (sets[3] % f32(1.0)).any()        # d2 is a whole number there
    assert edge >= CF.MIN_FIXTURE_BOUNDARY


def test_tie_frame_of_the_floor_scene(base):
    x, _ = CF.frame("floor", base["floor"], "tie")
    for md in (S.MAX_DIST, CF.TIE_MAX_DIST):
        ref = S.segment(x, md, CF.PLANE_H, 0, 1)
        edge = CF.plane_boundary_pairs(x, ref, md)
        print("the floor scene at %g extents, max_dist %.4f: %d evaluated, %d -> %d inliers, %d pairs at |offset| == max_dist, margin %.2e" % (
            CF.OFFSETS["floor"][2], md, ref["evaluated"], ref["inliers_ransac"], ref["inliers_final"], edge, S.margin(ref, md)))
        assert ref["status"] == S.OK
    assert edge >= CF.MIN_FIXTURE_BOUNDARY


def test_fpfh_reference_stays_usable_in_every_frame(base):
    for o in (0.0,) + CF.OFFSETS["cat"]:
        x, _ = CF.shifted(base["cat"], o)
        rc, offs, rows, d2 = R.radius_sets(x, CF.FPFH_R)
        i, j, _ = R.pair_index(np.arange(len(x)), offs, rows)
        share = float(R.ambiguous(R.pair_features(x, base["nrm"], i, j, np.float64)).any(1).mean())
        print("o = %g: %d pairs, %.2f %% ambiguous, %d at d2 == 0" % (o, len(i), 100 * share, int((d2 == 0).sum())))
        assert share <= CF.MAX_AMBIGUOUS


# ---- the references: what they are run on, in a frame (off: the frame's offset) or in a unit (e: its exponent) ------------------------------
def view(off, e):
    return CF.shifted_point(CF.VIEWPOINT, off) if off is not None else CF.lengths(CF.VIEWPOINT, e)


def ref_knn(x, b, e, off):
    return K.knn(x, CF.KNN_MAX)


def ref_radius(x, b, e, off):
    return [R.radius_sets(x, CF.length(r, e)) for r in CF.RADII + (CF.FPFH_R,)]


def ref_fpfh(x, b, e, off):
    """the reference's own pipeline: fp32 pair features, the header's SPFH, the fp64 FPFH stage"""
    rc, offs, rows, d2 = R.radius_sets(x, CF.length(CF.FPFH_R, e))
    c, k = R.spfh_counts(x, b["nrm"], np.arange(len(x)), offs, rows, np.float32)
    spfh = R.spfh_from_counts(c, k)
    return dict(count=rc, spfh=spfh, fpfh=R.fpfh_from_spfh(spfh, offs, rows, d2))


def ref_sor(x, b, e, off):
    return [X.statistical(x, k, mul) for k, mul in CF.SOR]


def ref_ror(x, b, e, off):
    count = R.radius_sets(x, CF.length(CF.ROR_R, e))[0]
    return X.radius(x, CF.length(CF.ROR_R, e), int(np.median(count)))


def ref_cluster(x, b, e, off):
    return [CR.cluster(x, CF.length(eps, e), mp) for eps in (CF.SCENE_EPS, CF.TIE_EPS) for mp in CF.SCENE_MIN_POINTS]


def ref_orient(x, b, e, off):
    rows = K.knn(x, CF.KNN_MAX)[0]
    return [OR.orient(x, b["signs"], k, rows=rows[:, :k], **seed) for k in CF.ORIENT_K
            for seed in (dict(viewpoint=view(off, e)), dict(direction=CF.DIRECTION_RULE))]


def ref_plane(x, b, e, off):
    out = []
    for md in (S.MAX_DIST, CF.TIE_MAX_DIST):
        r = S.segment(x, CF.length(md, e), CF.PLANE_H, 0, 1)
        out.append((r, (r["hyp_status"], r["hyp"], r["pivot"])))
    return out


def ref_eval(d, b, e, off):
    cases = b["eval_cases"] if off is None else CF.eval_cases(d, off)
    return [E.evaluate(d["src"], d["tgt"], FC.scaled_transform(Xf, 2.0 ** e), CF.length(D, e)) for _, Xf, D in cases]


def ref_ndt(x, b, e, off):
    return N.build_map(x, CF.length(CF.NDT_RES, e))


def ref_voxel(x, b, e, off):
    return V.voxel_downsample(x, CF.length(CF.VOXEL_LEAF, e), b["nrm"])


def each(compare):
    return lambda a, b, e: [compare(u, v, e) for u, v in zip(a, b)]


def plane_units(a, b, e):
    for (ra, ha), (rb, hb) in zip(a, b):
        CF.unit_hypotheses(ha, hb, e)
        CF.unit_segment(ra, rb, e)


# op -> (fixture, the reference, the unit assertion, what a run must show at least)
OPS = {
    "knn": ("cat", ref_knn, CF.unit_knn, lambda r: np.isfinite(r[1]).all() and (np.diff(r[1], axis=1) >= 0).all()),
    "radius_search": ("cat", ref_radius, each(CF.unit_radius), lambda r: all(len(s[2]) > 0 for s in r)),
    "fpfh": ("cat", ref_fpfh, CF.unit_fpfh, lambda r: np.isfinite(r["fpfh"]).all() and (r["count"] > 0).mean() > 0.9),
    "remove_statistical_outlier": ("cat", ref_sor, each(CF.unit_sor), lambda r: all(0 < len(s["rows"]) < 3400 for s in r)),
    "remove_radius_outlier": ("cat", ref_ror, CF.unit_ror, lambda r: 0 < len(r["rows"]) < 3400),
    "cluster_dbscan": ("scene", ref_cluster, each(CF.unit_cluster), lambda r: all(c["clusters"] > 1 for c in r)),
    "orient_normals": ("cat", ref_orient, each(CF.unit_orient), lambda r: all(o["tree_edges"] == 3400 - o["components"] for o in r)),
    "segment_plane": ("floor", ref_plane, plane_units, lambda r: all(s["status"] == S.OK and s["inliers_final"] > 1000 for s, _ in r)),
    "evaluate_registration": ("pair", ref_eval, each(CF.unit_eval), lambda r: all(v["inliers"] > 0 for v in r)),
    "ndt_map": ("ndt", ref_ndt, CF.unit_ndt, lambda r: len(r["key"]) > 10),
    "voxel_downsample": ("cat", ref_voxel, CF.unit_voxel, lambda r: r["count"].sum() == 3400),
}


@pytest.fixture(scope="module")
def original(base):
    """every reference in the original unit and frame, computed once"""
    base["eval_cases"] = CF.eval_cases(base["pair"])
    return {op: ref(base[fixture], base, 0, None) for op, (fixture, ref, _, _) in OPS.items()}


@pytest.mark.parametrize("op", list(OPS))
def test_reference_runs_in_every_frame(base, original, op):
    fixture, ref, _, shows = OPS[op]
    assert shows(original[op])
    for name in CF.FRAME_NAMES:
        if fixture == "pair":
            d = CF.pair_frame(base["pair"], name)
            x, off = d, d["offset"]
        else:
            x, off = CF.frame(fixture, base[fixture], name)
        assert shows(ref(x, base, 0, off)), (op, name)


@pytest.mark.parametrize("e", CF.UNIT_EXPONENTS)
@pytest.mark.parametrize("op", list(OPS))
def test_reference_is_equivariant_under_a_power_of_two_unit(base, original, op, e):
    fixture, ref, compare, _ = OPS[op]
    x = FC.scaled(base["pair"], 2.0 ** e) if fixture == "pair" else CF.scaled(base[fixture], e)
    compare(original[op], ref(x, base, e, None), e)
