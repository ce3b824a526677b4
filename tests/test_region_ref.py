"""CPU tests of the region-growing reference (tests/_region_ref.py): answers written down by hand, the properties the header promises
(sign blindness, the identity with Euclidean clustering, independence of the row order), and the exact counts of the cat at the
non-trivial setting of tests/test_gpu_region.py.  The device is compared against this reference there; here the reference is pinned."""
import numpy as np
import pytest

import _cluster_ref as CR
import _region_ref as G

F = np.float32
H = 2.0 ** -4                  # the corner's lattice spacing
SP = CR.CAT_SPACING


@pytest.fixture(scope="module")
def corner():
    return G.corner(12, H)


def test_cos_of_is_the_stated_conversion():
    assert G.cos_of(30).dtype == np.float32 and G.cos_of(30) == F(0.8660254) and G.cos_of(0) == F(1) and G.cos_of(60) == F(0.5)
    assert G.cos_of(90) >= 0 and G.cos_of(90) < 1e-7


def test_one_point():
    x, nr = np.zeros((1, 3), F), np.array([[0, 0, 1]], F)
    r = G.region_growing(x, nr, 1.0, G.cos_of(30))
    assert r["labels"].tolist() == [0] and r["regions"] == 1 and r["sizes"].tolist() == [1] and r["smooth"].tolist() == [0] and r["seed"].all()
    r = G.region_growing(x, nr, 1.0, G.cos_of(30), np.array([1.0], F), 0.05)
    assert r["labels"].tolist() == [-1] and r["regions"] == 0 and len(r["sizes"]) == 0 and not r["seed"].any()


def test_two_points_at_the_exact_bound():
    """n_i . n_j is exactly 0.5 in fp32: one region at smoothness_cos = 0.5, two at the next float above it"""
    x = CR.line([0.0, 1.0])
    nr = np.array([[1, 0, 0], [0.5, 0.8660254, 0]], F)
    assert G.smooth_dot(nr[0], nr[1]) == F(0.5)
    r = G.region_growing(x, nr, 1.5, F(0.5))
    assert r["labels"].tolist() == [0, 0] and r["smooth"].tolist() == [1, 1]
    r = G.region_growing(x, nr, 1.5, np.nextafter(F(0.5), F(1)))
    assert r["labels"].tolist() == [0, 1] and r["smooth"].tolist() == [0, 0] and r["sizes"].tolist() == [1, 1]
    assert G.region_growing(x, nr, 0.5, F(0.5))["labels"].tolist() == [0, 1]          # smooth normals, out of range


def test_d2_equal_to_r2_is_a_member():
    x = np.array([[0, 0, 0], [3, 4, 0]], F)
    nr = np.tile(np.array([[0, 0, 1]], F), (2, 1))
    assert G.region_growing(x, nr, 5.0, F(1))["labels"].tolist() == [0, 0]
    assert G.region_growing(x, nr, np.nextafter(F(5), F(0)), F(1))["labels"].tolist() == [0, 1]


def test_corner_is_one_cluster_and_three_regions(corner):
    """the test that shows the feature: Euclidean clustering cannot split the corner, region growing gives its three faces"""
    x, nr, face = corner
    assert len(x) == 397 and np.bincount(face).tolist() == [144, 132, 121]
    assert CR.cluster(x, 1.5 * H, 1)["clusters"] == 1
    r = G.region_growing(x, nr, 1.5 * H, G.cos_of(10))
    assert r["regions"] == 3 and r["sizes"].tolist() == [144, 132, 121] and np.array_equal(r["labels"], face)
    assert r["seed"].all() and (r["labels"] >= 0).all()                                # no border rows, nothing unlabelled
    assert r["smooth"].min() >= 3 and r["smooth"].max() == 8


def test_corner_with_non_seed_edges(corner):
    """a caller-made curvature turns the 34 rows on the cube's edges into non-seeds: each joins the face its normal belongs to"""
    x, nr, face = corner
    cv = G.edge_curvature(x, H)
    r = G.region_growing(x, nr, 1.5 * H, G.cos_of(10), cv, 0.05)
    assert (~r["seed"]).sum() == 34 and np.array_equal(r["seed"], cv == 0)
    assert r["regions"] == 3 and r["sizes"].tolist() == [144, 132, 121] and np.array_equal(r["labels"], face)
    # the threshold is compared as curv <= threshold: at 0.1 the edges are seeds again, at -1 nothing is
    assert G.region_growing(x, nr, 1.5 * H, G.cos_of(10), cv, F(0.1))["seed"].all()
    assert (G.region_growing(x, nr, 1.5 * H, G.cos_of(10), cv, -1.0)["labels"] == -1).all()


def face_of_label(labels, face, skip):
    """{label: the face of its rows}, the row `skip` left out; every label's rows lie in one face"""
    rest = np.arange(len(labels)) != skip
    out = {}
    for l in np.unique(labels[rest]).tolist():
        f = np.unique(face[rest][labels[rest] == l])
        assert len(f) == 1 and l >= 0
        out[l] = int(f[0])
    return out


@pytest.mark.parametrize("moved,reverse,want", [(False, False, 1), (False, True, 2), (True, False, 2), (True, True, 2)])
def test_border_row_on_the_edge(moved, reverse, want):
    """the hand-built border row (see _region_ref.border_case): a bit-equal d2 goes to the lower representative, a nearer seed wins"""
    x, nr, cv, face, row = G.border_case(moved)
    if reverse:
        x, nr, cv, face, row = x[::-1].copy(), nr[::-1].copy(), cv[::-1].copy(), face[::-1], len(x) - 1 - row
    r = G.region_growing(x, nr, 1.5 * H, G.cos_of(50), cv, 0.05)
    assert r["regions"] == 3 and (~r["seed"]).sum() == 1 and not r["seed"][row]
    faces = face_of_label(r["labels"], face, row)
    assert sorted(faces.values()) == [0, 1, 2] and faces[int(r["labels"][row])] == want
    if not moved:
        # the tie is real: a seed of each face at the same d2 bits, and the face it joined has the lower representative
        d2 = ((x.astype(F) - x[row]) ** 2).sum(1)
        near = np.nonzero((d2 == F(H * H)) & r["seed"])[0]
        assert {int(face[j]) for j in near} == {1, 2}
        reps = {faces[l]: int(np.nonzero(r["labels"] == l)[0].min()) for l in faces}
        assert reps[want] < reps[3 - want]
    # at 40 degrees the row's normal is smooth with nobody: it stays unlabelled
    assert G.region_growing(x, nr, 1.5 * H, G.cos_of(40), cv, 0.05)["labels"][row] == -1


def test_every_row_a_non_seed(corner):
    x, nr, _ = corner
    r = G.region_growing(x, nr, 1.5 * H, G.cos_of(10), np.ones(len(x), F), 0.05)
    assert (r["labels"] == -1).all() and r["regions"] == 0 and len(r["sizes"]) == 0 and not r["seed"].any() and r["smooth"].min() >= 3


def test_sign_flips_change_nothing(cat):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    sign = np.where(np.random.default_rng(0).random(len(x)) < 0.5, F(-1), F(1))
    a = G.region_growing(x, nr, 3 * SP, G.cos_of(15), cv, 0.05)
    b = G.region_growing(x, nr * sign[:, None], 3 * SP, G.cos_of(15), cv, 0.05)
    for key in ("labels", "sizes", "seed", "smooth", "root"):
        assert np.array_equal(a[key], b[key]), key


def test_identity_with_euclidean_clustering(cat, corner):
    """smoothness_cos = 0 and no curvature: the labels of _cluster_ref.cluster(., eps, 1), label for label"""
    for x, nr, eps, clusters in ((cat["src"], cat["src_n"], 3 * SP, 8), (corner[0], corner[1], 1.5 * H, 1)):
        r, c = G.region_growing(x, nr, eps, 0.0), CR.cluster(x, eps, 1)
        assert c["clusters"] == clusters and r["regions"] == clusters
        assert np.array_equal(r["labels"], c["labels"]) and np.array_equal(r["sizes"], c["sizes"]) and np.array_equal(r["smooth"], c["neighbors"])


def test_row_order_does_not_matter(cat):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    perm = np.random.default_rng(9).permutation(len(x))
    a = G.region_growing(x, nr, 3 * SP, G.cos_of(15), cv, 0.05)
    b = G.region_growing(x[perm], nr[perm], 3 * SP, G.cos_of(15), cv[perm], 0.05)
    # no border row of this setting ties between two regions (a tie goes by the representative, which the row order moves)
    back = np.empty(len(x), np.int32)
    back[perm] = b["labels"]
    assert G.partition(back) == G.partition(a["labels"])
    assert np.array_equal(b["seed"], a["seed"][perm]) and np.array_equal(b["smooth"], a["smooth"][perm])
    for r in (a, b):
        assert G.numbering_is_by_lowest_seed_row(r["labels"], r["seed"])
        assert sorted(np.unique(r["labels"][r["labels"] >= 0]).tolist()) == list(range(r["regions"]))


def test_cat_counts_are_pinned(cat):
    """the cat with the golden normals and curvature at (3 spacings, 15 degrees, 0.05): a setting with many regions, border rows and
    unlabelled rows at once"""
    r = G.region_growing(cat["src"], cat["src_n"], 3 * SP, G.cos_of(15), cat["golden"]["src_curv"], 0.05)
    lab = r["labels"]
    border, unlabelled = int((~r["seed"] & (lab >= 0)).sum()), int((lab < 0).sum())
    assert (r["regions"], int(r["sizes"].max()), border, unlabelled) == (321, 1708, 312, 548)
    assert r["regions"] >= 100 and border >= 200 and unlabelled >= 200
    assert int(r["sizes"].sum()) + unlabelled == 3400


def test_size_filter(cat):
    x, nr, cv = cat["src"], cat["src_n"], cat["golden"]["src_curv"]
    full = G.region_growing(x, nr, 3 * SP, G.cos_of(15), cv, 0.05)
    for lo, hi in ((5, 0), (0, 100), (5, 100)):
        r = G.region_growing(x, nr, 3 * SP, G.cos_of(15), cv, 0.05, lo, hi)
        keep = np.ones(full["regions"], bool)
        keep &= (full["sizes"] >= lo) if lo else True
        keep &= (full["sizes"] <= hi) if hi else True
        assert 0 < r["regions"] == keep.sum() < full["regions"] and np.array_equal(r["sizes"], full["sizes"][keep])
        assert np.array_equal(r["labels"] >= 0, (full["labels"] >= 0) & np.append(keep, False)[full["labels"]])
        assert np.array_equal(r["root"], full["root"]) and np.array_equal(r["seed"], full["seed"])
