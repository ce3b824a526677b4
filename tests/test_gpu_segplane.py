"""GPU tests of the RANSAC plane segmentation (symmicp_ctx_segment_plane; kernels_plane.hip) against tests/_segplane_ref.py.

The device part -- pivot, status, (n, d), the per-hypothesis inlier counts, the winner -- is EQUAL to the reference; the final rows are
EQUAL too (the scenes keep every row at least 1e-6 max_dist from the fp64 threshold, asserted here per case where it is relied on), and
the plane agrees to 1e-12 (two correct fp64 evaluations of a 3x3 eigenvector differ by a few ulp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import _cluster_ref as CR
import _segplane_ref as S
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
SP = S.SP
CHUNK, BATCH = S.K_CHUNK, S.K_BATCH


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def floor(cat):
    return S.floor_scene(cat["src"])


@pytest.fixture(scope="module")
def wall(cat):
    return S.floor_wall_scene(cat["src"])


def lattice(nx, ny, z=0.0):
    g = np.stack(np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.full((len(g), 1), z)], 1).astype(F)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fiu" else a


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def check(sym, eng, x, max_dist, H, seed=0, refits=1, min_inliers=3, axis=None, deg=0.0, rows_exact=True):
    """one call against the reference -> (result dict, reference dict)"""
    ref = S.segment(x, max_dist, H, seed, refits, min_inliers, axis, deg)
    cfg = sym.plane_config(max_dist, H, seed, refits, min_inliers, axis, deg)
    hy = eng.plane_hypotheses(x, cfg)
    assert same_bits(hy["pivot"], ref["pivot"])
    assert np.array_equal(hy["hyp_status"], ref["hyp_status"])
    assert same_bits(hy["hyp"], ref["hyp"]), int(np.count_nonzero((bits(hy["hyp"]) != bits(ref["hyp"])).reshape(H, -1).any(1)))
    st, r = eng.segment_plane(x, max_dist, H, seed, refits, min_inliers, axis, deg, return_info=True, check=False)
    assert st == ref["status"], (st, ref["status"])
    assert np.array_equal(r["hyp_status"], ref["hyp_status"]) and np.array_equal(r["hyp_inliers"], ref["hyp_inliers"])
    assert (r["best_hypothesis"], r["evaluated"], r["inliers_ransac"]) == (ref["best_hypothesis"], ref["evaluated"], ref["inliers_ransac"])
    if st != sym.OK:
        assert st == sym.ERR_NO_CONSENSUS and r["count"] == 0 and len(r["rows"]) == 0 and not r["plane"].any() and not r["plane32"].any()
        assert r["inliers_final"] == 0
        return r, ref
    if rows_exact:
        assert np.array_equal(r["rows"], ref["rows"]) and r["rows"].dtype == np.int32 and r["inliers_final"] == r["count"] == len(ref["rows"])
    xf = x.astype(np.float64)
    extent = float(np.abs(xf).max()) + 1.0
    assert np.abs(r["plane"][:3] - ref["plane"][:3]).max() <= 1e-12 and abs(r["plane"][3] - ref["plane"][3]) <= 1e-12 * extent
    assert abs(np.linalg.norm(r["plane"][:3]) - 1.0) <= (1e-6 if refits == 0 else 1e-12)
    assert same_bits(r["plane32"], r["plane"].astype(F))
    assert np.abs(r["distance"] - (xf @ r["plane"][:3] + r["plane"][3])).max() <= 1e-9 * extent
    assert abs(r["rmse_final"] - np.sqrt(np.mean(r["distance"][r["rows"]] ** 2))) <= 1e-9 * extent
    return r, ref


# ---- exactness ------------------------------------------------------------------------------------------------------------------------
SQUARE = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.5, 1.25]], F)


def test_three_points(sym, eng):
    r, _ = check(sym, eng, np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F), 0.5, 64)
    assert r["best_hypothesis"] == 1 and r["evaluated"] == 13 and r["rows"].tolist() == [0, 1, 2]


@pytest.mark.parametrize("refits", [0, 1])
def test_a_point_at_exactly_max_dist(sym, eng, refits):
    r, _ = check(sym, eng, SQUARE, 0.25, 64, refits=refits)
    assert r["inliers_ransac"] == 5 and r["rows"].tolist() == [0, 1, 2, 3, 4]
    r, _ = check(sym, eng, SQUARE, np.nextafter(F(0.25), F(0)), 64, refits=refits)
    assert r["inliers_ransac"] == 4 and r["rows"].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("name", ["collinear", "coincident"])
def test_no_plane_no_consensus(sym, eng, name):
    x = CR.line(np.arange(20.0)) if name == "collinear" else np.tile(np.array([[0.5, -1.25, 3.0]], F), (20, 1))
    r, _ = check(sym, eng, x, 0.5, 128, seed=3)
    assert r["status"] == sym.ERR_NO_CONSENSUS and r["evaluated"] == 0 and r["best_hypothesis"] == -1
    with pytest.raises(sym.SymmIcpError) as e:
        sym.segment_plane(x, 0.5, 128, 3)
    assert e.value.status == sym.ERR_NO_CONSENSUS


def test_equal_planes_the_lowest_hypothesis_wins(sym, eng):
    x = np.concatenate([lattice(8, 8, 0.0), lattice(8, 8, 10.0)])
    x = np.ascontiguousarray(x[np.random.default_rng(2).permutation(len(x))])
    r, ref = check(sym, eng, x, 0.25, 64, refits=0)
    assert r["best_hypothesis"] == np.nonzero(ref["hyp_inliers"] == 64)[0][0] and np.count_nonzero(ref["hyp_inliers"] == 64) > 1


def test_min_inliers(sym, eng):
    x = np.concatenate([lattice(8, 8, 0.0), lattice(5, 5, 10.0)])
    assert check(sym, eng, x, 0.25, 64, min_inliers=64)[0]["status"] == sym.OK
    r, _ = check(sym, eng, x, 0.25, 64, min_inliers=65)
    assert r["status"] == sym.ERR_NO_CONSENSUS and r["inliers_ransac"] == 64 and r["best_hypothesis"] >= 0


def test_orientation_rule(sym, eng):
    x = lattice(9, 7, 2.0)
    for seed in range(6):
        r, _ = check(sym, eng, x, 0.25, 16, seed=seed)
        assert r["plane"][2] > 0
        d, _ = check(sym, eng, x, 0.25, 16, seed=seed, axis=(0, 0, -3), deg=10.0)
        assert d["plane"][2] < 0 and np.array_equal(d["rows"], r["rows"])
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    diag = np.stack([g[:, 0], g[:, 0], g[:, 1]], 1).astype(F)
    for seed in range(4):
        r, _ = check(sym, eng, diag, 0.25, 16, seed=seed, refits=0)
        assert r["plane"][0] > 0 and r["plane"][0] == -r["plane"][1]


def test_axis_constraint(sym, eng):
    x = np.concatenate([lattice(8, 8, 0.0), lattice(8, 8, 0.0)[:, [2, 0, 1]]])
    r, ref = check(sym, eng, x, 0.25, 64, seed=1, refits=0, axis=(0, 0, 2), deg=10.0)
    assert np.array_equal(r["plane"], [0, 0, 1, 0]) and (r["hyp_status"] == sym.PLANE_OFF_AXIS).any()
    r, _ = check(sym, eng, x, 0.25, 64, seed=1, refits=0, axis=(-1, 0, 0), deg=10.0)
    assert np.array_equal(r["plane"], [-1, 0, 0, 0])
    check(sym, eng, x, 0.25, 64, seed=1, axis=(0, 1, 0), deg=90.0)                  # 90 degrees: cos_min rounds to a tiny positive number


def test_cat_is_exact(sym, eng, cat):
    for refits in (0, 2):
        r, ref = check(sym, eng, cat["src"], 2 * SP, 512, seed=4, refits=refits, rows_exact=False)
        near = np.abs(np.abs(ref["distance"]) - float(F(2 * SP))) <= 1e-6 * 2 * SP      # rows a tolerance on the plane could flip
        diff = np.setxor1d(r["rows"], ref["rows"])
        assert r["status"] == sym.OK and np.all(near[diff]), (len(diff), int(near.sum()))


def test_bunny_is_exact(sym, eng, bunny):
    """the bunny fixture is one scan line of 93 points, straight to a few parts in a thousand: every sample sits at the sine bound, which
    the device decides in fp32 exactly as the reference does"""
    md = 4 * CR.R.median_spacing(bunny, np.arange(len(bunny)))
    for seed in (0, 4):
        r, ref = check(sym, eng, bunny, md, 512, seed=seed, rows_exact=False)
        assert np.count_nonzero(ref["hyp_status"] == S.DEGENERATE) > 400


def test_cat_offset_by_1e4_is_pivoted(sym, eng, cat):
    x = (cat["src"].astype(np.float64) + np.array([1e4, -2e4, 3e4])).astype(F)
    r, ref = check(sym, eng, x, 2 * SP, 512, seed=4, rows_exact=False)
    assert np.abs(ref["pivot"]).max() > 9e3 and r["inliers_final"] > 100
    assert len(np.setxor1d(r["rows"], ref["rows"])) == 0 or S.margin(ref, 2 * SP) <= 1e-6


def test_floor_scene(sym, eng, floor):
    x, kind = floor
    r, ref = check(sym, eng, x, S.MAX_DIST, 256)
    assert S.margin(ref, S.MAX_DIST) > 1e-6
    assert np.all(np.isin(np.nonzero(kind == S.FLOOR)[0], r["rows"])) and S.angle_deg(r["plane"][:3], S.SCENE_UP) <= 0.05


def test_floor_wall_scene(sym, eng, wall):
    x, kind = wall
    r, ref = check(sym, eng, x, S.MAX_DIST, 256)
    assert S.margin(ref, S.MAX_DIST) > 1e-6 and np.count_nonzero(kind[r["rows"]] == S.WALL) == 6293
    r, ref = check(sym, eng, x, S.MAX_DIST, 256, axis=S.SCENE_UP, deg=10.0)
    assert S.margin(ref, S.MAX_DIST) > 1e-6 and np.count_nonzero(kind[r["rows"]] == S.FLOOR) == 5542
    assert float(r["plane"][:3] @ S.SCENE_UP) > 0 and 200 <= np.count_nonzero(r["hyp_status"] == sym.PLANE_OFF_AXIS) <= 245


# ---- boundaries -----------------------------------------------------------------------------------------------------------------------
def noisy_plane(n, seed):
    """n points of the plane z = 0.2 x - 0.1 y with noise, and a fifth of them lifted off it"""
    rng = np.random.default_rng(seed)
    p = rng.uniform(-10, 10, (n, 3))
    p[:, 2] = 0.2 * p[:, 0] - 0.1 * p[:, 1] + rng.normal(0, 0.02, n)
    p[::5, 2] += rng.uniform(1, 5, len(p[::5]))
    return p.astype(F)


@pytest.mark.parametrize("n", [3, 4, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1])
def test_point_counts_around_the_chunk(sym, eng, n):
    check(sym, eng, noisy_plane(n, n), 0.1, 96, seed=n, rows_exact=False)


@pytest.mark.parametrize("H", [1, 255, 256, 257, 511, 512, 513, 4096])
def test_hypothesis_counts(sym, eng, H):
    check(sym, eng, noisy_plane(700, 5), 0.1, H, seed=2, rows_exact=False)


def test_evaluated_counts_around_a_block(sym, eng):
    """a workgroup of the scoring kernel owns K_BATCH EVALUATED hypotheses, 256 per hypothesis slot of a lane: one less than / equal to /
    one more than a slot's worth, a workgroup's worth and two, by choosing H from the reference's statuses"""
    x = noisy_plane(300, 8)
    st = S.hypotheses(x, 5 * BATCH // 2, 6)["status"]
    ev = np.cumsum(st == S.EVALUATED)
    seen = []
    wants = [255, 256, 257, BATCH - 1, BATCH, BATCH + 1, 2 * BATCH, 2 * BATCH + 1]
    for want in wants:
        H = int(np.nonzero(ev == want)[0][0]) + 1
        r, ref = check(sym, eng, x, 0.1, H, seed=6, rows_exact=False)
        seen.append(ref["evaluated"])
    assert seen == wants


def test_all_but_one_hypothesis_not_evaluated(sym, eng):
    """a long line and one point off it: only a sample of that point and two distinct line points is a plane"""
    x = CR.line(np.arange(40.0))
    x[17] = [17.0, 9.0, 0.0]
    ev = [int((S.hypotheses(x, H, 0)["status"] == S.EVALUATED).sum()) for H in range(1, 200)]
    H = ev.index(1) + 1
    r, ref = check(sym, eng, x, 0.25, H, refits=0)
    assert ref["evaluated"] == 1 and r["status"] == sym.OK and r["inliers_ransac"] == 40 and r["best_hypothesis"] == H - 1


# ---- interface ------------------------------------------------------------------------------------------------------------------------
def test_strided_and_column_major_inputs(sym, eng, floor):
    x = floor[0][:3000]
    n = len(x)
    cfg = sym.plane_config(S.MAX_DIST, 128, 1)
    st, want = eng.segment_plane_raw(x, cfg, cap=n)
    assert st == sym.OK
    padded = np.zeros((n, 4), F)
    padded[:, :3] = x
    for buf, strides in ((padded, (n, 4, 1)), (np.ascontiguousarray(x.T), (n, 1, n))):
        st, got = eng.segment_plane_raw(buf, cfg, cap=n, strides=strides)
        assert st == sym.OK and all(same_bits(np.asarray(got[k]), np.asarray(want[k])) for k in want)
        hy = eng.plane_hypotheses(buf, cfg, strides=strides)
        assert all(same_bits(v, eng.plane_hypotheses(x, cfg)[k]) for k, v in hy.items())


def test_cap_protocol(sym, eng, floor):
    x = floor[0]
    cfg = sym.plane_config(S.MAX_DIST, 256, 0)
    st, full = eng.segment_plane_raw(x, cfg, cap=len(x))
    count = full["count"]
    assert st == sym.OK and count == 5575 and (full["rows"][:count] >= 0).all() and (full["rows"][count:] == -1).all()
    st, r = eng.segment_plane_raw(x, cfg)                                  # the count only: rows_out NULL, cap 0
    assert st == sym.ERR_SIZE and r["count"] == count and r["rows"] is None and same_bits(r["plane"], full["plane"]) and same_bits(r["distance"], full["distance"])
    st, r = eng.segment_plane_raw(x, cfg, cap=count - 1)
    assert st == sym.ERR_SIZE and r["count"] == count and (r["rows"] == -1).all() and same_bits(r["plane32"], full["plane32"])
    st, r = eng.segment_plane_raw(x, cfg, cap=count)
    assert st == sym.OK and np.array_equal(r["rows"], full["rows"][:count])
    st, r = eng.segment_plane_raw(x, cfg, cap=count, want=False)           # without the optional outputs
    assert st == sym.OK and np.array_equal(r["rows"], full["rows"][:count]) and "distance" not in r


# ---- determinism and the context ------------------------------------------------------------------------------------------------------
def test_two_calls_give_equal_bytes(sym, wall):
    x = wall[0]
    outs = []
    for _ in range(2):
        r = sym.segment_plane(x, S.MAX_DIST, 256, 0, axis=S.SCENE_UP, max_angle_deg=10.0, return_info=True)      # a fresh one-shot context each
        outs.append({k: np.asarray(v) for k, v in r.items()})
    with sym.Engine() as e:
        r = e.segment_plane(x, S.MAX_DIST, 256, 0, axis=S.SCENE_UP, max_angle_deg=10.0, return_info=True)
        outs.append({k: np.asarray(v) for k, v in r.items()})
    for o in outs[1:]:
        assert [k for k in o if not same_bits(o[k], outs[0][k])] == []


def test_context_between_two_steps_is_left_untouched(sym, cat, floor):
    """segment_plane on a context stopped between two symmicp_step calls: the steps after it are bit-equal to an undisturbed run's"""
    def run(disturb):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            its = [e.begin()]
            out = None
            for k in range(6):
                if disturb and k in (1, 3):
                    out = e.segment_plane(floor[0], S.MAX_DIST, 256, 0, return_info=True)
                its.append(e.step())
            return its, e.transform(), e.certificates(), out

    a, Xa, ca, _ = run(False)
    b, Xb, cb, out = run(True)
    for p, q in zip(a, b):
        assert [k for k in p if not same_bits(np.asarray(p[k]), np.asarray(q[k]))] == []
    assert same_bits(Xa, Xb) and all(same_bits(u, v) for u, v in zip((ca[0], ca[2], ca[3]), (cb[0], cb[2], cb[3])))
    ref = S.segment(floor[0], S.MAX_DIST, 256, 0, 1)
    assert np.array_equal(out["rows"], ref["rows"]) and np.array_equal(out["hyp_inliers"], ref["hyp_inliers"])


# ---- composition ----------------------------------------------------------------------------------------------------------------------
def test_segment_planes_peels_two_planes(sym, eng, wall):
    x, kind = wall
    planes, labels = eng.segment_planes(x, S.MAX_DIST, 5, 1000, hypotheses=256)
    rp, rl = S.segment_planes(x, S.MAX_DIST, 5, 1000, 256, 0, 1)
    assert len(planes) == 2 and np.array_equal(labels, rl) and np.abs(planes - rp).max() <= 1e-10
    assert np.count_nonzero(kind[labels == 0] == S.WALL) == 6293
    p1, l1 = sym.segment_planes(x, S.MAX_DIST, 1, 1000, hypotheses=256)
    assert len(p1) == 1 and np.array_equal(l1 == 0, labels == 0)


def test_floor_removed_then_clusters_then_batch_align(sym, eng, cat, floor):
    """the pipeline the feature exists for: one cluster with the floor, three without it, packed and aligned in one batch"""
    x, kind = floor
    assert len(sym.euclidean_clusters(x, CR.THREE_EPS)) == 1
    plane, rows = eng.segment_plane(x, S.MAX_DIST, 256)
    keep = np.setdiff1d(np.arange(len(x)), rows)
    objects = np.ascontiguousarray(x[keep])
    labels = eng.cluster_dbscan(objects, CR.THREE_EPS)
    assert labels.max() == 2 and labels.min() == 0
    for k in range(3):
        assert len(np.unique(kind[keep][labels == k])) == 1
    nrm = eng.estimate_normals(objects, 10)[0]
    pk = sym.pack_clusters(objects, nrm, labels)
    assert len(pk["ranges"]) == 3 and pk["skipped"] == []
    # every object against a copy of itself turned by 2 degrees about the plane's normal
    from symmicp import synth
    Rz = synth.rotation(2.0, plane[:3])
    c = pk["xyz"].astype(np.float64).mean(axis=0)
    tgt = ((pk["xyz"].astype(np.float64) - c) @ Rz.T + c).astype(F)
    tgt_n = (pk["nrm"].astype(np.float64) @ Rz.T).astype(F)
    problems = [(int(f), int(m), int(f), int(m)) for f, m in pk["ranges"]]
    rs = eng.batch_align(pk["xyz"], pk["nrm"], tgt, tgt_n, problems, mode=sym.MODE_PAPER, max_iters=30)
    assert len(rs) == 3
    for r in rs:
        assert r["status"] == 0 and r["diff_final"] < r["diff_initial"]          # (each object was moved towards its own copy)


# ---- MyICP (Python and C++) and the driver ----------------------------------------------------------------------------------------------
E2E_BOUND = 1e-4              # tests/test_gpu_outlier.py's bound on end-point comparisons of two alignments
PAIR_H = 256


@pytest.fixture(scope="module")
def pair(cat):
    """the cat pair, each cat standing on a sparse noisy floor of its own (the target's floor moved with the cat), rows shuffled ->
    dict(src, tgt, src_floor, tgt_floor [bool], truth); the reference's answers for both clouds ride along"""
    from symmicp import synth
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    T = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])      # cat.pcd -> cat_out.pcd
    x = cat["src"].astype(np.float64)
    lo, hi = x.min(axis=0), x.max(axis=0)
    gx, gy = np.meshgrid(np.arange(lo[0] - 4 * SP, hi[0] + 4 * SP, 2 * SP), np.arange(lo[1] - 4 * SP, hi[1] + 4 * SP, 2 * SP), indexing="ij")
    lattice_ = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, lo[2])], 1)
    out = dict(truth=T)
    for name, seed, base, M in (("src", 31, cat["src"], np.eye(4)), ("tgt", 32, cat["tgt"], T)):
        f = lattice_.copy()
        f[:, 2] += (synth.uniform01(seed, len(f)) - 0.5) * 0.6 * SP
        f = f @ M[:3, :3].T + M[:3, 3]
        cloud = np.concatenate([base.astype(np.float64), f]).astype(F)
        perm = np.random.default_rng(seed).permutation(len(cloud))
        out[name] = np.ascontiguousarray(cloud[perm])
        out[name + "_floor"] = (np.arange(len(cloud)) >= len(base))[perm]
        ref = S.segment(out[name], S.MAX_DIST, PAIR_H, 0, 1)
        assert ref["status"] == S.OK and S.margin(ref, S.MAX_DIST) > 1e-6 and np.all(out[name + "_floor"][ref["rows"]].sum() == out[name + "_floor"].sum())
        out[name + "_keep"] = np.setdiff1d(np.arange(len(cloud)), ref["rows"])
        out[name + "_plane"] = ref["plane"]
    return out


def new_icp(sym):
    return sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, verbose=False)


def pair_inputs(eng, pair):
    """normals the caller supplies for the source (the kept rows' estimated normals, a marker on the rest) and intensities"""
    ks = pair["src_keep"]
    nrm = np.tile(np.array([[0, 0, 1]], F), (len(pair["src"]), 1))
    nrm[ks] = eng.estimate_normals(pair["src"][ks], 10)[0]
    return nrm, np.arange(len(pair["src"]), dtype=F), np.arange(len(pair["tgt"]), dtype=F) * F(0.5)


def test_myicp_python_remove_plane(sym, eng, pair):
    ks, kt = pair["src_keep"], pair["tgt_keep"]
    nrm, si, ti = pair_inputs(eng, pair)
    icp = new_icp(sym)
    icp.setInputSource(pair["src"], nrm, si)
    icp.setInputTarget(pair["tgt"], None, ti)
    for bad in (dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=S.MAX_DIST, hypotheses=0), dict(max_dist=S.MAX_DIST, min_inliers=-1),
                dict(max_dist=S.MAX_DIST, axis=(0, 0, 1), max_angle_deg=0.0)):
        with pytest.raises(sym.SymmIcpError) as e:
            icp.removePlane(**bad)
        assert e.value.status == sym.ERR_ARG and len(icp.cloud_src) == len(pair["src"]) and len(icp.cloud_tgt) == len(pair["tgt"])
    # no plane of that many points: nothing goes, and that is not an error
    assert icp.removePlane(S.MAX_DIST, PAIR_H, min_inliers=len(pair["src"])) == sym.OK and icp.outliersRemoved() == (0, 0)
    assert not icp.planeRemoved()[0].any() and not icp.planeRemoved()[1].any() and len(icp.cloud_src) == len(pair["src"])
    assert icp.removePlane(S.MAX_DIST, PAIR_H) == sym.OK
    assert icp.outliersRemoved() == (len(pair["src"]) - len(ks), len(pair["tgt"]) - len(kt))
    assert np.array_equal(icp.cloud_src, pair["src"][ks]) and np.array_equal(icp.cloud_tgt, pair["tgt"][kt])
    assert not pair["src_floor"][ks].any() and not pair["tgt_floor"][kt].any()                   # every floor row went
    assert np.array_equal(icp.normals_src, nrm[ks]) and icp._have_src and icp.normals_tgt is None
    assert np.array_equal(icp.intensity_src, si[ks]) and np.array_equal(icp.intensity_tgt, ti[kt])
    for got, want in zip(icp.planeRemoved(), (pair["src_plane"], pair["tgt_plane"])):
        assert np.abs(got - want).max() <= 1e-10 and got[2] > 0.99
    ra = icp.align()
    clean = new_icp(sym)                                                   # the pair without the floor: the kept rows, supplied the same normals
    clean.setInputSource(pair["src"][ks], nrm[ks])
    clean.setInputTarget(pair["tgt"][kt], None)
    rb = clean.align()
    assert ra["status"] == rb["status"] == sym.OK
    diff = float(np.abs(ra["transform"].astype(np.float64) - rb["transform"]).max())
    off = float(np.abs(ra["transform"].astype(np.float64) - pair["truth"]).max())
    print("|T_edited - T_without_floor| = %.2e; |T_edited - truth| = %.2e" % (diff, off))
    assert diff <= E2E_BOUND and off < 1e-2


def test_myicp_cpp_remove_plane(sym, eng, pair, tmp_path):
    ks, kt = pair["src_keep"], pair["tgt_keep"]
    nrm, si, ti = pair_inputs(eng, pair)
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_segplane")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for fname, arr in (("src", pair["src"]), ("tgt", pair["tgt"]), ("src_nrm", nrm), ("src_int", si), ("tgt_int", ti),
                       ("params", np.array([S.MAX_DIST, PAIR_H]))):
        np.ascontiguousarray(arr, F).tofile(tmp_path / (fname + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert np.array_equal(np.fromfile(tmp_path / "keep_src.i32", np.int32), ks) and np.array_equal(np.fromfile(tmp_path / "keep_tgt.i32", np.int32), kt)
    assert np.array_equal(np.fromfile(tmp_path / "out_src.f32", F).reshape(-1, 3), pair["src"][ks])
    assert np.array_equal(np.fromfile(tmp_path / "out_tgt.f32", F).reshape(-1, 3), pair["tgt"][kt])
    planes = np.fromfile(tmp_path / "planes.f64", np.float64).reshape(2, 4)
    assert np.abs(planes - np.stack([pair["src_plane"], pair["tgt_plane"]])).max() <= 1e-10
    # the two classes make the same calls: the transform of the Python class on the same inputs
    icp = new_icp(sym)
    icp.setInputSource(pair["src"], nrm, si)
    icp.setInputTarget(pair["tgt"], None, ti)
    icp.removePlane(S.MAX_DIST, PAIR_H)
    ra = icp.align()
    out = np.fromfile(tmp_path / "out_T.f32", F)
    assert out[0] == 0 and float(np.abs(out[1:].reshape(4, 4).astype(np.float64) - ra["transform"]).max()) <= E2E_BOUND


def test_icp_align_driver_remove_plane(sym, pair, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    a, b, out = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), str(tmp_path / "moved.pcd")
    sym.pcd_write(a, pair["src"], binary=True)
    sym.pcd_write(b, pair["tgt"], binary=True)
    ks, kt = pair["src_keep"], pair["tgt_keep"]
    base = [exe, "--mode", "paper", "--corr", "tree", "--iters", "30", "--out", out]
    for extra in ([], ["--plane-axis", "0,0,2:10"]):
        r = subprocess.run(base + ["--remove-plane", "%r:%d" % (S.MAX_DIST, PAIR_H)] + extra + [a, b], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        lines = [ln for ln in r.stdout.splitlines() if "plane removal:" in ln]
        assert len(lines) == 1
        assert tuple(int(v) for v in re.search(r"source (\d+) -> (\d+), target (\d+) -> (\d+)", lines[0]).groups()) == (
            len(pair["src"]), len(ks), len(pair["tgt"]), len(kt))
        moved, _ = sym.pcd_read(out)                                        # the edited source, aligned: row j is kept row j
        T = pair["truth"]
        want = pair["src"][ks].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
        assert moved.shape == want.shape
        rms = float(np.sqrt(((moved - want) ** 2).sum(1).mean()))
        print("icp_align --remove-plane %s: rms to the truth %.4f (spacing 1.38)" % (" ".join(extra), rms))
        assert rms < 0.05                                                   # tests/test_gpu_outlier.py's bound for the same driver
    q = subprocess.run(base + ["--quiet", "--remove-plane", "%r" % S.MAX_DIST, a, b], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0 and "plane removal" not in q.stdout
    q = subprocess.run(base + ["--remove-plane", "%r:%d:%d" % (S.MAX_DIST, PAIR_H, len(pair["src"]))] + [a, b], capture_output=True, text=True, timeout=600)
    assert q.returncode == 0 and "source %d -> %d, target %d -> %d" % ((len(pair["src"]),) * 2 + (len(pair["tgt"]),) * 2) in q.stdout      # no such plane: nothing goes
    for bad in (["--remove-plane", "0"], ["--remove-plane", "-1:100"], ["--remove-plane", "0.5:0"], ["--remove-plane", "0.5:x"],
                ["--remove-plane", "0.5:100:-1"], ["--remove-plane", "0.5:100:3:4"], ["--remove-plane", "0.5", "--plane-axis", "0,0,1"],
                ["--remove-plane", "0.5", "--plane-axis", "0,0,1:0"], ["--remove-plane", "0.5", "--plane-axis", "0,0,1:91"],
                ["--remove-plane", "0.5", "--plane-axis", "0,0,0:10"], ["--remove-plane", "0.5", "--plane-axis", "0,1:10"], ["--plane-axis", "0,0,1:10"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64, bad
