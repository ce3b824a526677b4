"""CPU tests of tests/_global_ref.py, the numpy restatement of feature matching and RANSAC that tests/test_gpu_global.py holds the
device to: the matching against a brute force in fp64, hand-worked RANSAC samples, the draws against plain integer arithmetic, the
invariance of the winner's inlier set under a rigid motion, and the numbers of the fp64 reference pipeline (reference FPFH of
tests/_fpfh_ref.py, SciPy k-d tree for the matching) on the two test inputs as regression pins."""
import numpy as np
import pytest

import _global_ref as G
import _knn_ref as K

F = np.float32
CAT_R = 11.05


def cat_truth():
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    return np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


@pytest.fixture(scope="module")
def catref(cat):
    """the cat pair through the fp64 reference pipeline: FPFH at r = 11.05 and the mutual matches"""
    fs, ft = G.reference_fpfh(cat["src"], cat["src_n"], CAT_R), G.reference_fpfh(cat["tgt"], cat["tgt_n"], CAT_R)
    return dict(src=cat["src"], tgt=cat["tgt"], fs=fs, ft=ft, pairs=G.mutual_matches_kdtree(fs, ft), truth=cat_truth(), max_dist=CAT_R / 4)


@pytest.fixture(scope="module")
def bumpsref():
    b = G.bumps_pair()
    b["fs"], b["ft"] = G.reference_fpfh(b["src"], b["src_n"], b["radius"]), G.reference_fpfh(b["tgt"], b["tgt_n"], b["radius"])
    b["pairs"] = G.mutual_matches_kdtree(b["fs"], b["ft"])
    return b


def true_pairs(d):
    x = d["src"][d["pairs"][:, 0]].astype(np.float64) @ d["truth"][:3, :3].T + d["truth"][:3, 3]
    return int((np.linalg.norm(x - d["tgt"][d["pairs"][:, 1]], axis=1) <= d["max_dist"]).sum())


# ---- matching -----------------------------------------------------------------------------------------------------------------------
def test_feature_nn_against_fp64_brute_force(catref):
    fa, fb = catref["fs"][:800].astype(F), catref["ft"].astype(F)
    nn, d2, second = G.feature_nn(fa, fb)
    D = ((fa.astype(np.float64)[:, None, :] - fb.astype(np.float64)[None, :, :]) ** 2).sum(2)
    rows = np.arange(len(fa))
    o = np.argsort(D, axis=1, kind="stable")[:, :2]
    # fp32 sums of 33 non-negative terms: within 34 roundings of the exact value
    tol = 34 * 2.0 ** -24
    assert np.all(np.abs(d2 - D[rows, nn]) <= tol * D[rows, nn])
    assert np.all(np.abs(second - D[rows, o[:, 1]]) <= tol * D[rows, o[:, 1]] + 1e-30)
    gap = D[rows, o[:, 1]] - D[rows, o[:, 0]] > 2 * tol * D[rows, o[:, 1]]
    assert gap.mean() > 0.99 and np.array_equal(nn[gap], o[gap, 0])
    assert np.all(D[rows, nn] <= D[rows, o[:, 0]] * (1 + 2 * tol))               # ... and elsewhere a tie within rounding
    # chunking does not matter
    a = G.feature_nn(fa, fb, budget=1 << 12)
    assert all(np.array_equal(x, y) for x, y in zip(a, (nn, d2, second)))


def test_feature_nn_ties_duplicates_and_single_rows():
    rng = np.random.default_rng(1)
    fa, fb = (rng.random((40, 33)) * 100).astype(F), (rng.random((30, 33)) * 100).astype(F)
    fb2 = np.concatenate([fb, fb[:10]])
    nn, d2, second = G.feature_nn(fa, fb2)
    assert (nn < 30).all()
    dup = nn < 10
    assert np.array_equal(second[dup], d2[dup])
    nn, d2, second = G.feature_nn(fa, fb[:1])
    assert not nn.any() and np.isinf(second).all()
    nn, d2, second = G.feature_nn(np.zeros((5, 33), F), np.zeros((7, 33), F))
    assert not nn.any() and not d2.any() and not second.any()
    exact = G.feature_nn(fb, fb)
    assert np.array_equal(exact[0], np.arange(30)) and not exact[1].any() and (exact[2] > 0).all()


def test_correspondence_filters():
    rng = np.random.default_rng(2)
    fb = (rng.random((50, 33)) * 100).astype(F)
    fa = fb[rng.permutation(50)[:35]] + (rng.random((35, 33)) * 0.01).astype(F)
    one_way, _ = G.correspondences(fa, fb, mutual=False)
    assert len(one_way) == 35 and np.array_equal(one_way[:, 0], np.arange(35))
    mutual, d2 = G.correspondences(fa, fb, mutual=True)
    assert len(mutual) == 35                                                     # every query has its own twin
    fa2 = np.concatenate([fa, fa[:5] + F(0.5)])                                  # five worse copies compete for the same rows
    mutual2, _ = G.correspondences(fa2, fb, mutual=True)
    assert len(mutual2) == 35 and (mutual2[:, 0] < 35).all()
    strict, _ = G.correspondences(fa2, fb, mutual=False, max_ratio=1e-3)
    loose, _ = G.correspondences(fa2, fb, mutual=False, max_ratio=0.999)
    assert len(strict) <= 35 < len(loose) <= 40
    nn, dd, sec = G.feature_nn(fa2, fb)
    assert np.array_equal(loose[:, 0], np.nonzero(dd <= F(0.999) * F(0.999) * sec)[0])


# ---- RANSAC -------------------------------------------------------------------------------------------------------------------------
def test_draws_restate_splitmix64_in_plain_integers():
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    for seed, m in ((1, 3196), (8, 705), (0, 3), (2 ** 63 + 12345, 2 ** 31 - 1)):
        base = mix((seed * 0x9E3779B97F4A7C15 + 0x2545F4914F6CDD1D) & M)
        c = G.draws(seed, 50, m)
        want = [((mix((base + (i + 1) * 0x9E3779B97F4A7C15) & M) >> 32) * m) >> 32 for i in range(150)]
        assert c.reshape(-1).tolist() == want and c.min() >= 0 and c.max() < m


def test_a_known_triangle_pair_gives_a_known_transform():
    from symmicp import synth
    R = synth.rotation(70.0, (1.0, -2.0, 0.5))
    t = np.array([0.3, -1.2, 2.0])
    p = np.array([[0, 0, 0], [1, 0, 0], [0.2, 0.9, 0], [0.4, 0.3, 0.8], [-0.5, 0.2, 0.1]], np.float64)
    q = p @ R.T + t
    hy = G.hypotheses(p, q, np.array([[0, 1, 2], [3, 1, 4], [2, 4, 0]]), 0.01)
    assert list(hy["status"]) == [G.EVALUATED] * 3 and hy["clear"].all()
    for k in range(3):
        assert np.abs(hy["Rt"][k, :9].reshape(3, 3) - R).max() < 1e-12 and np.abs(hy["Rt"][k, 9:] - t).max() < 1e-12
    assert np.array_equal(G.inlier_counts(hy["Rt"], p, q, 0.01), [5, 5, 5])
    # by hand: the unit right triangle against itself turned a quarter about z and lifted by 3
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    q = np.array([[0, 0, 3], [0, 1, 3], [-1, 0, 3]], np.float64)
    hy = G.hypotheses(p, q, np.array([[0, 1, 2]]), 0.5)
    assert np.allclose(hy["Rt"][0], [0, -1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 3], atol=1e-15)


def test_every_status_is_reached_by_a_constructed_sample():
    p = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0.5, 0, 0], [0, 0.6, 0]], np.float64)
    q = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [0.5, 0, 0], [0.3, 1.0, 0]], np.float64)
    q[:, 0] += 5.0
    c = np.array([[0, 1, 1],          # a repeated draw
                  [0, 1, 5],          # |p0 - p5| = 0.6 against |q0 - q5| = 1.04: the edges disagree
                  [0, 1, 3],          # collinear
                  [0, 1, 2]])         # fine
    hy = G.hypotheses(p, q, c, 0.1)
    assert list(hy["status"]) == [G.REPEATED, G.EDGE, G.DEGENERATE, G.EVALUATED]
    assert list(hy["clear"]) == [False, True, False, True]      # the collinear sample has no frame: the quantities of the later check are not numbers
    # far: triangles that pass the edge test (ratio 0.9) and are not congruent; the sample pairs miss by more than max_dist
    q2 = q.copy()
    q2[2] = [5.0, 1.08, 0]
    hy = G.hypotheses(p, q2, np.array([[0, 1, 2]]), 0.01)
    assert list(hy["status"]) == [G.FAR]
    assert list(G.hypotheses(p, q2, np.array([[0, 1, 2]]), 0.2)["status"]) == [G.EVALUATED]
    # the edge check switched off lets the unequal triangle through to the later checks
    assert G.hypotheses(p, q, c[1:2], 0.1, edge_ratio=0.0)["status"][0] in (G.FAR, G.EVALUATED)
    # a threshold met within 1e-4 is not clear
    q3 = q.copy()
    q3[2] = [5.0, 1.0 / 0.9 * (1 + 2e-5), 0]
    assert not G.hypotheses(p, q3, np.array([[0, 1, 2]]), 10.0)["clear"][0]


def test_kabsch_is_a_proper_rotation_and_exact_on_exact_data():
    from symmicp import synth
    rng = np.random.default_rng(3)
    X = rng.standard_normal((40, 3))
    R, t = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([0.7, -0.4, 1.1])
    T = G.kabsch(X, X @ R.T + t)
    assert np.abs(T[:3, :3] - R).max() < 1e-13 and np.abs(T[:3, 3] - t).max() < 1e-13
    Y = X.copy(); Y[:, 2] *= -1                                    # a mirror image: the best PROPER rotation, not the reflection
    T = G.kabsch(X, Y)
    assert abs(np.linalg.det(T[:3, :3]) - 1.0) < 1e-12


def test_winner_inlier_set_is_invariant_under_a_rigid_motion(catref):
    """the same pairs and draws with both centred clouds turned by one rotation (in fp64, no rounding of the moved clouds; the pivots take up any translation): same
    statuses up to the unclear ones, same winner, same inlier set"""
    from symmicp import synth
    d = catref
    M = synth.rotation(77.0, (0.2, -0.9, 0.4))
    a = G.ransac(d["src"], d["tgt"], d["pairs"], d["max_dist"], 4000, 2, refits=0)
    p, q, _, _ = G.pivoted(d["src"], d["tgt"], d["pairs"])
    pm, qm = p.astype(np.float64) @ M.T, q.astype(np.float64) @ M.T                 # pivots move along: the motion of the centred sets
    c = G.draws(2, 4000, len(d["pairs"]))
    hy = G.hypotheses(pm, qm, c, d["max_dist"])
    cl = a["clear"] & hy["clear"]
    assert cl.mean() > 0.99 and np.array_equal(hy["status"][cl], a["status"][cl])
    ev = np.nonzero(hy["status"] == G.EVALUATED)[0]
    inl = np.zeros(4000, np.int64)
    inl[ev] = G.inlier_counts(hy["Rt"][ev], pm, qm, float(F(d["max_dist"])))
    best = int(np.argmax(inl))
    assert best == a["best"] and inl[best] == a["inliers"][a["best"]]
    mask = G.residuals(hy["Rt"][best:best + 1], pm, qm)[0] <= float(F(d["max_dist"]))
    assert np.array_equal(mask, a["mask"])


# ---- the numbers of the reference pipeline (regression pins) ---------------------------------------------------------------------------
def test_reference_numbers_on_the_cat_pair(catref):
    d = catref
    assert len(d["src"]) == 3400 and len(d["pairs"]) == 3196 and true_pairs(d) == 3180
    for seed in (1, 2, 3):
        w = G.ransac(d["src"], d["tgt"], d["pairs"], d["max_dist"], 4000, seed, refits=0)
        r1 = G.ransac(d["src"], d["tgt"], d["pairs"], d["max_dist"], 4000, seed, refits=1)
        r2 = G.ransac(d["src"], d["tgt"], d["pairs"], d["max_dist"], 4000, seed, refits=2)
        rot = [G.rotation_error_deg(x["T"], d["truth"]) for x in (w, r1, r2)]
        rms = [G.rms_to_truth(x["T"], d["truth"], d["src"]) for x in (w, r1, r2)]
        print("cat seed %d: %d evaluated, winner %d inliers; %.2f deg %.3f -> %.3f deg %.4f -> %.3f deg %.4f; %.2f %% not clear" % (
            seed, w["evaluated"], w["inliers"][w["best"]], rot[0], rms[0], rot[1], rms[1], rot[2], rms[2], 100 * (~w["clear"]).mean()))
        assert 3958 <= w["evaluated"] <= 3974 and 3183 <= w["inliers"][w["best"]] <= 3184
        assert 2.0 <= rot[0] <= 2.7 and 0.76 <= rms[0] <= 0.95
        assert rot[1] <= 0.06 and 0.016 <= rms[1] <= 0.024
        assert rot[2] <= 0.05 and rms[2] <= 0.017
        assert (~w["clear"]).mean() <= 0.0016


def test_reference_numbers_on_the_bumps_pair(bumpsref):
    d = bumpsref
    sp = d["spacing"]
    assert abs(sp - 5.92e-3) < 0.005e-3 and len(d["pairs"]) == 705 and true_pairs(d) == 46
    for seed in range(1, 9):
        w = G.ransac(d["src"], d["tgt"], d["pairs"], d["max_dist"], 262144, seed, refits=0)
        r1 = G.ransac(d["src"], d["tgt"], d["pairs"], d["max_dist"], 262144, seed, refits=1)
        rot = [G.rotation_error_deg(x["T"], d["truth"]) for x in (w, r1)]
        rms = [G.rms_to_truth(x["T"], d["truth"], d["src"]) / sp for x in (w, r1)]
        print("bumps seed %d: %d evaluated, winner %d inliers (runner-up %d); %.2f deg %.2f -> %.2f deg %.2f spacings; %.2f %% not clear" % (
            seed, w["evaluated"], w["inliers"][w["best"]], w["runner_up"], rot[0], rms[0], rot[1], rms[1], 100 * (~w["clear"]).mean()))
        assert 493 <= w["evaluated"] <= 591 and 48 <= w["inliers"][w["best"]] <= 51 and 46 <= w["runner_up"] <= 49
        assert 0.29 <= rot[0] <= 0.66 and 0.58 <= rms[0] <= 1.11
        assert 0.13 <= rot[1] <= 0.34 and 0.34 <= rms[1] <= 0.73
        assert (~w["clear"]).mean() <= 0.0050


def test_reference_numbers_on_cat_moved_by_a_further_140_degrees(cat):
    """normals estimated on each cloud alone (k = 10, viewpoint at the origin): the two clouds disagree on the orientation of a
    fifth of their normals, and the matching still carries RANSAC"""
    from symmicp import synth
    R2, t2 = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([40.0, -25.0, 60.0])
    src = cat["src"]
    tgt = (cat["tgt"].astype(np.float64) @ R2.T + t2).astype(F)
    truth = synth.rigid4(R2, t2) @ cat_truth()
    sn, tn = K.emulate(src, K.knn(src, 10)[0])[0], K.emulate(tgt, K.knn(tgt, 10)[0])[0]
    flipped = float((((sn.astype(np.float64) @ truth[:3, :3].T) * tn).sum(1) < 0).mean())
    assert 0.17 <= flipped <= 0.21
    d = dict(src=src, tgt=tgt, truth=truth, max_dist=CAT_R / 4,
             pairs=G.mutual_matches_kdtree(G.reference_fpfh(src, sn, CAT_R), G.reference_fpfh(tgt, tn, CAT_R)))
    assert len(d["pairs"]) == 1483 and true_pairs(d) == 1326
    for seed in (1, 2, 3):
        r = G.ransac(src, tgt, d["pairs"], d["max_dist"], 65536, seed)
        rot, rms = G.rotation_error_deg(r["T"], truth), G.rms_to_truth(r["T"], truth, src)
        print("cat + 140 deg, seed %d: %d evaluated, %d inliers; %.3f deg, rms %.4f" % (seed, r["evaluated"], r["inliers"][r["best"]], rot, rms))
        assert 0.04 <= rot <= 0.08 and 0.03 <= rms <= 0.06
