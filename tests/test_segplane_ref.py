"""CPU tests that pin tests/_segplane_ref.py -- the numpy statement of symmicp_ctx_segment_plane that the GPU tests compare with -- to
answers written down by hand, and that check the conditions the two scenes of the GPU tests rely on from the reference alone."""
import numpy as np
import pytest

import _cluster_ref as CR
import _segplane_ref as S


def lattice(nx, ny, z=0.0):
    g = np.stack(np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij"), -1).reshape(-1, 2)
    return np.concatenate([g, np.full((len(g), 1), z)], 1).astype(np.float32)


TRIANGLE = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
# a unit square at z = 1 and its centre raised by 0.25: the mean's z (1.05) is not an fp32 number, but 1 - c and 1.25 - c are exact
# (both within a factor 2 of c), so the raised point is EXACTLY 0.25 from the square's plane on the device
SQUARE = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1], [0.5, 0.5, 1.25]], np.float32)


def test_three_points_only_the_permutations_are_evaluated():
    hy = S.hypotheses(TRIANGLE, 64, 0)
    perm = np.array([sorted(d) == [0, 1, 2] for d in hy["draws"].tolist()])
    assert np.array_equal(hy["status"] == S.EVALUATED, perm) and np.all(hy["status"][~perm] == S.REPEATED)
    assert np.nonzero(perm)[0].tolist() == EVALUATED_OF_64
    assert np.array_equal(np.abs(hy["hyp"][perm]), np.tile(np.array([[0, 0, 1, 0]], np.float32), (perm.sum(), 1)))
    assert not hy["hyp"][~perm].any()
    r = S.segment(TRIANGLE, 0.5, 64, 0, 1)
    assert r["status"] == S.OK and r["best_hypothesis"] == EVALUATED_OF_64[0] and r["inliers_ransac"] == 3 and r["rows"].tolist() == [0, 1, 2]
    assert np.allclose(r["plane"], [0, 0, 1, 0], atol=1e-15)


# recorded from a pure-Python SplitMix64 of (seed 0, stream 2) at n = 3: the h whose three draws are a permutation of (0, 1, 2)
EVALUATED_OF_64 = [1, 9, 11, 19, 22, 23, 24, 27, 34, 36, 55, 60, 63]


def test_the_draws_are_stream_2_of_the_seed():
    from symmicp import synth
    u = synth.splitmix64(7, 30, stream=2)
    assert not np.array_equal(u, synth.splitmix64(7, 30, stream=0)) and not np.array_equal(u, synth.splitmix64(7, 30, stream=1))
    d = S.draws(1000, 10, 7)
    assert d.shape == (10, 3) and np.array_equal(d.ravel(), [(int(v) >> 32) * 1000 >> 32 for v in u.tolist()])


def test_a_point_at_exactly_max_dist_is_an_inlier():
    hy = S.hypotheses(SQUARE, 64, 0)
    flat = (hy["status"] == S.EVALUATED) & (np.abs(hy["hyp"][:, 2]) == 1)            # samples of three corners
    assert flat.any()
    off = np.abs(S.offsets32(hy["p"], hy["hyp"][np.nonzero(flat)[0][0]]))
    assert off.tolist() == [0, 0, 0, 0, 0.25]                                       # exactly
    inl = S.score(hy["p"], hy["hyp"], hy["status"], 0.25)
    below = S.score(hy["p"], hy["hyp"], hy["status"], np.nextafter(np.float32(0.25), np.float32(0)))
    assert np.all(inl[flat] == 5) and np.all(below[flat] == 4)
    assert np.all(inl[(hy["status"] == S.EVALUATED) & ~flat] == 3)                   # a tilted plane holds its own sample only
    r = S.segment(SQUARE, 0.25, 64, 0, 0)
    assert r["status"] == S.OK and r["inliers_ransac"] == 5 and r["rows"].tolist() == [0, 1, 2, 3, 4] and r["best_hypothesis"] == np.nonzero(flat)[0][0]
    r = S.segment(SQUARE, np.nextafter(np.float32(0.25), np.float32(0)), 64, 0, 0)
    assert r["status"] == S.OK and r["inliers_ransac"] == 4 and r["rows"].tolist() == [0, 1, 2, 3]
    assert np.array_equal(np.abs(r["plane"]), [0, 0, 1, 1]) and r["plane"][2] == 1 and r["plane"][3] == -1      # z = 1, in the caller's frame


@pytest.mark.parametrize("name", ["collinear", "coincident"])
def test_clouds_without_a_plane_have_no_consensus(name):
    x = CR.line(np.arange(20.0)) if name == "collinear" else np.tile(np.array([[0.5, -1.25, 3.0]], np.float32), (20, 1))
    r = S.segment(x, 0.5, 128, 3, 1)
    assert r["status"] == S.NO_CONSENSUS and r["evaluated"] == 0 and r["best_hypothesis"] == -1 and r["count"] == 0 and not r["plane"].any()
    assert np.all((r["hyp_status"] == S.REPEATED) | (r["hyp_status"] == S.DEGENERATE)) and (r["hyp_status"] == S.DEGENERATE).any()
    assert not r["hyp"].any() and not r["hyp_inliers"].any()


def test_equal_planes_the_lowest_hypothesis_wins():
    x = np.concatenate([lattice(8, 8, 0.0), lattice(8, 8, 10.0)])
    x = np.ascontiguousarray(x[np.random.default_rng(2).permutation(len(x))])
    r = S.segment(x, 0.25, 64, 0, 0)
    full = np.nonzero(r["hyp_inliers"] == 64)[0]
    d = r["hyp"][full, 3] * r["hyp"][full, 2]                                      # +5 for the plane z = 0, -5 for z = 10 (pivot z = 5)
    assert r["hyp_inliers"].max() == 64 and set(d.tolist()) == {5.0, -5.0}           # both planes were drawn, with equal counts
    assert r["best_hypothesis"] == full[0] and r["inliers_final"] == 64
    assert np.array_equal(r["plane"], [0, 0, 1, 0 if d[0] > 0 else -10]) and np.all(x[r["rows"], 2] == (0 if d[0] > 0 else 10))


def test_orientation_rule():
    x = lattice(9, 7, 2.0)
    signs = set()
    for seed in range(6):
        r = S.segment(x, 0.25, 16, seed, 1)
        signs.add(float(np.sign(r["hyp"][r["best_hypothesis"], 2])))
        assert r["status"] == S.OK and np.allclose(r["plane"], [0, 0, 1, -2], atol=1e-12) and r["plane"][2] > 0
        down = S.segment(x, 0.25, 16, seed, 1, axis=(0, 0, -3), max_angle_deg=10.0)
        assert np.allclose(down["plane"], [0, 0, -1, 2], atol=1e-12) and np.array_equal(down["rows"], r["rows"])
    assert signs == {1.0, -1.0}                                                     # the winners' own normals pointed both ways
    # equal magnitudes: the lowest axis decides.  The plane x = y through lattice points: n0 == -n1 exactly with refits = 0
    g = np.stack(np.meshgrid(np.arange(6.0), np.arange(5.0), indexing="ij"), -1).reshape(-1, 2)
    diag = np.stack([g[:, 0], g[:, 0], g[:, 1]], 1).astype(np.float32)
    for seed in range(4):
        r = S.segment(diag, 0.25, 16, seed, 0)
        assert r["status"] == S.OK and r["plane"][0] > 0 and r["plane"][0] == -r["plane"][1] and r["plane"][2] == 0


def test_axis_constraint_status():
    x = np.concatenate([lattice(8, 8, 0.0), lattice(8, 8, 0.0)[:, [2, 0, 1]]])       # the planes z = 0 and x = 0
    free = S.hypotheses(x, 64, 1)
    up = S.hypotheses(x, 64, 1, axis=(0, 0, 2), max_angle_deg=10.0)
    was = free["status"] == S.EVALUATED
    assert np.array_equal(up["status"][~was], free["status"][~was]) and np.array_equal(up["hyp"], free["hyp"])      # OFF_AXIS keeps n, d
    cosz = np.abs(free["hyp"][:, 2])
    assert np.array_equal(up["status"][was] == S.OFF_AXIS, cosz[was] < np.float32(np.cos(np.radians(10.0))))
    assert (up["status"] == S.OFF_AXIS).any() and (up["status"] == S.EVALUATED).any()
    r = S.segment(x, 0.25, 64, 1, 0, axis=(0, 0, 2), max_angle_deg=10.0)
    assert np.array_equal(r["plane"], [0, 0, 1, 0]) and r["inliers_final"] == 64 + 8
    r = S.segment(x, 0.25, 64, 1, 0, axis=(-1, 0, 0), max_angle_deg=10.0)
    assert np.array_equal(r["plane"], [-1, 0, 0, 0]) and r["inliers_final"] == 64 + 8


def test_min_inliers_above_the_winner_is_no_consensus():
    x = np.concatenate([lattice(8, 8, 0.0), lattice(5, 5, 10.0)])
    assert S.segment(x, 0.25, 64, 0, 1, min_inliers=64)["status"] == S.OK
    r = S.segment(x, 0.25, 64, 0, 1, min_inliers=65)
    assert r["status"] == S.NO_CONSENSUS and r["inliers_ransac"] == 64 and r["best_hypothesis"] >= 0 and r["count"] == 0 and not r["plane"].any()
    planes, labels = S.segment_planes(x, 0.25, 5, 20, 64, 0, 1)
    assert len(planes) == 2 and np.array_equal(labels, [0] * 64 + [1] * 25)
    assert len(S.segment_planes(x, 0.25, 5, 26, 64, 0, 1)[0]) == 1 and len(S.segment_planes(x, 0.25, 1, 3, 64, 0, 1)[0]) == 1


def test_jacobi_restatement_agrees_with_lapack():
    rng = np.random.default_rng(0)
    for _ in range(20):
        B = rng.standard_normal((3, 3))
        A0 = B @ B.T
        A, V = S.jacobi3(A0)
        lam = np.array([A[0][0], A[1][1], A[2][2]])
        assert np.allclose(np.sort(lam), np.linalg.eigvalsh(A0), rtol=1e-12, atol=1e-13)
        V = np.array(V)
        assert np.allclose(A0 @ V, V * lam, atol=1e-12) and np.allclose(V.T @ V, np.eye(3), atol=1e-13)


# ---- the scenes of tests/test_gpu_segplane.py ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def floor(cat):
    x, kind = S.floor_scene(cat["src"])
    return x, kind, S.segment(x, S.MAX_DIST, 256, 0, 1)


@pytest.fixture(scope="module")
def wall(cat):
    return S.floor_wall_scene(cat["src"])


def test_floor_scene_the_floor_is_found_and_the_objects_come_apart(floor):
    x, kind, r = floor
    assert len(x) == 11492 and np.count_nonzero(kind == S.FLOOR) == 5542
    rows = r["rows"]
    assert r["status"] == S.OK and np.all(np.isin(np.nonzero(kind == S.FLOOR)[0], rows))          # every floor row is an inlier
    assert np.count_nonzero(kind[rows] < S.FLOOR) <= 60
    assert S.angle_deg(r["plane"][:3], S.SCENE_UP) <= 0.05
    assert abs(np.linalg.norm(r["plane"][:3]) - 1) < 1e-15
    assert S.margin(r, S.MAX_DIST) > 1e-6                                                         # a tolerance on the plane cannot flip a row
    assert CR.cluster(x, CR.THREE_EPS)["clusters"] == 1
    keep = np.setdiff1d(np.arange(len(x)), rows)
    after = CR.cluster(x[keep], CR.THREE_EPS)
    assert after["clusters"] == 3
    for k in range(3):
        assert len(np.unique(kind[keep][after["labels"] == k])) == 1


def test_floor_wall_scene_unconstrained_the_wall_wins(wall):
    x, kind = wall
    assert len(x) == 17785 and np.count_nonzero(kind == S.WALL) == 6293
    r = S.segment(x, S.MAX_DIST, 256, 0, 1)
    got = np.bincount(kind[r["rows"]], minlength=5)
    assert r["status"] == S.OK and got[S.WALL] == 6293 and got[:3].sum() == 0 and 100 <= got[S.FLOOR] <= 250
    assert S.angle_deg(r["plane"][:3], S.SCENE_WALL_NORMAL) <= 0.05 and S.margin(r, S.MAX_DIST) > 1e-6


def test_floor_wall_scene_with_the_up_axis_the_floor_wins(wall):
    x, kind = wall
    r = S.segment(x, S.MAX_DIST, 256, 0, 1, axis=S.SCENE_UP, max_angle_deg=10.0)
    got = np.bincount(kind[r["rows"]], minlength=5)
    assert r["status"] == S.OK and got[S.FLOOR] == 5542 and 150 <= got[S.WALL] <= 300 and got[:3].sum() <= 60
    assert 200 <= np.count_nonzero(r["hyp_status"] == S.OFF_AXIS) <= 245
    assert S.angle_deg(r["plane"][:3], S.SCENE_UP) <= 0.05 and float(r["plane"][:3] @ S.SCENE_UP) > 0 and S.margin(r, S.MAX_DIST) > 1e-6


def test_floor_wall_scene_peels_into_two_planes(wall):
    x, kind = wall
    planes, labels = S.segment_planes(x, S.MAX_DIST, 5, 1000, 256, 0, 1)
    assert len(planes) == 2
    first, second = np.bincount(kind[labels == 0], minlength=5), np.bincount(kind[labels == 1], minlength=5)
    assert first[S.WALL] == 6293 and second[S.WALL] == 0 and second[S.FLOOR] >= 5542 - 250 and first[S.FLOOR] + second[S.FLOOR] == 5542
    assert np.count_nonzero(labels < 0) == np.count_nonzero(kind < S.FLOOR) - second[:3].sum()
