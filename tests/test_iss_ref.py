"""CPU tests of the numpy restatement of the ISS keypoints (tests/_iss_ref.py): against an O(n^2) brute force written with loops,
on hand-worked clouds whose answers are known exactly, and pinned on the golden cat pair (what tests/test_gpu_iss.py relies on)."""
import os

import numpy as np
import pytest

import _iss_ref as I
from conftest import GOLDEN

F = np.float32
CAT_SPACING = 1.3816          # median nearest-neighbour distance of cat.pcd


def brute(xyz, rs, rn, g21, g32, min_nb):
    """the header, with loops: -> (k, s, keypoint rows)"""
    x = np.ascontiguousarray(xyz, F)
    n = len(x)

    def nbrs(i, r):
        r2 = F(r) * F(r)
        out = []
        for j in range(n):
            d = x[j] - x[i]
            d2 = F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
            if j != i and d2 <= r2:
                out.append(j)
        return out

    k, s = np.zeros(n, np.int64), np.zeros(n, F)
    for i in range(n):
        nb = nbrs(i, rs)
        k[i] = len(nb)
        if k[i] < min_nb:
            continue
        S = np.zeros((3, 3))
        for j in nb:
            e = (x[j] - x[i]).astype(np.float64)
            S += np.outer(e, e)
        l3, l2, l1 = np.linalg.eigvalsh(S / k[i])
        if l2 < float(F(g21)) * l1 and l3 < float(F(g32)) * l2 and F(l3) > 0:
            s[i] = F(l3)
    keep = []
    for i in range(n):
        nb = nbrs(i, rn)
        if s[i] > 0 and len(nb) >= min_nb and not any(s[j] > s[i] or (s[j] == s[i] and j < i) for j in nb):
            keep.append(i)
    return k, s, np.array(keep, np.int32)


@pytest.mark.parametrize("seed,n,rs,rn,g21,g32,min_nb", [(1, 220, 0.25, 0.2, 0.975, 0.975, 5), (2, 150, 0.3, 0.45, 0.8, 0.6, 3),
                                                          (3, 90, 0.5, 0.3, 1.0, 1.0, 1)])
def test_restatement_against_brute_force(seed, n, rs, rn, g21, g32, min_nb):
    rng = np.random.default_rng(seed)
    x = rng.random((n, 3)).astype(F)
    x[:, 2] *= F(0.3)                                     # a slab: a spread of eigenvalue ratios
    x[n // 2] = x[0]                                      # a duplicate point is a neighbour of its twin
    k, s, rows = brute(x, rs, rn, g21, g32, min_nb)
    got_rows, sal = I.keypoints(x, rs, rn, g21, g32, min_nb)
    assert np.array_equal(sal["k"], k)
    # the sums run in another order: a few 1e-16 l1, far below the margin of every clear point
    cl = sal["clear"]
    assert cl.mean() > 0.99
    assert np.array_equal(sal["s"][cl] > 0, s[cl] > 0)
    assert np.allclose(sal["s"][cl], s[cl], rtol=2.0 ** -22, atol=0)
    assert 0 < len(rows) < n
    assert np.array_equal(I.nms(s, x, rn, min_nb), rows)                 # NMS is a pure function of s
    if np.array_equal(sal["s"], s):
        assert np.array_equal(got_rows, rows)
    for brute_sets in (True, False):                                     # the k-d tree proposals and the brute neighbourhoods agree
        assert np.array_equal(I.nms(s, x, rn, min_nb, brute=brute_sets), rows)


def test_planar_lattice_has_no_keypoint():
    x = I.lattice(9, 9)
    rows, sal = I.keypoints(x, I.LATTICE_RS, I.LATTICE_RS)
    assert sal["k"][40] == 20 and sal["k"].min() >= 5
    assert (sal["lam"][:, 2] == 0).all() and not sal["salient"].any() and not sal["s"].any() and len(rows) == 0
    assert sal["clear"].all()


def test_straight_line_has_no_keypoint():
    x = np.zeros((40, 3), F)
    x[:, 0] = np.cumsum(np.random.default_rng(1).integers(1, 4, 40)) * 0.25
    rows, sal = I.keypoints(x, 3.0, 3.0)
    assert sal["k"].min() >= 5
    assert (sal["lam"][:, 1:] == 0).all() and not sal["s"].any() and len(rows) == 0


def test_single_bump_has_its_keypoint_at_the_apex():
    """the apex sees its 20 neighbours all 0.5 below it: C = diag(mean dx^2, mean dy^2, 0.25) exactly, l3 = h^2; a neighbour of the apex
    sees one point 0.5 above the plane: l3 about h^2 / k.  Every point with s > 0 lies within the radius of the apex and loses to it."""
    x = I.lattice(9, 9, [(4, 4)])
    rows, sal = I.keypoints(x, I.LATTICE_RS, I.LATTICE_RS)
    assert list(rows) == [40]
    assert sal["k"][40] == 20 and np.array_equal(sal["lam"][40], [2.65625, 1.7, 0.25]) and sal["s"][40] == F(0.25)
    others = np.setdiff1d(np.nonzero(sal["s"])[0], [40])
    assert len(others) == 20 and (sal["s"][others] < 0.02).all()
    assert sal["clear"].all()
    # with gamma21 = 1 on a SQUARE neighbourhood l1 == l2 exactly: the strict test fails, nothing is salient at the apex
    sq = x.copy()
    sq[:, 1] = (sq[:, 1] / F(I.LATTICE_DY)).astype(F)
    assert I.saliency(sq, 2.5, 1.0, 1.0)["s"][40] == 0


def test_exact_tie_goes_to_the_lowest_row():
    x, a, b = I.double_bump()
    sal = I.saliency(x, I.LATTICE_RS)
    assert sal["s"][a] == sal["s"][b] == F(0.25)                          # translated neighbourhoods: the same bits
    assert list(I.nms(sal["s"], x, I.LATTICE_RS)) == sorted([a, b])       # out of each other's reach: both stay
    assert list(I.nms(sal["s"], x, 9.0)) == [min(a, b)]                   # within reach: the lower row alone
    swapped = x.copy()
    swapped[[a, b]] = swapped[[b, a]]                                     # (the two points trade rows: still the lower ROW)
    assert list(I.keypoints(swapped, I.LATTICE_RS, 9.0)[0]) == [min(a, b)]


# ---- pins on the golden pair: (salient radius, non-maximum radius) in spacings -> keypoints of cat, of cat_out, common rows ----------
CAT_PINS = {(6, 4): (91, 91, 91), (8, 6): (33, 33, 33), (4, 3): (160, 160, 160)}


@pytest.fixture(scope="module")
def cats(oracle):
    return [oracle.pcd_read(os.path.join(GOLDEN, f))[0] for f in ("cat.pcd", "cat_out.pcd")]


@pytest.mark.parametrize("radii", sorted(CAT_PINS))
def test_pins_on_the_cat_pair(cats, radii):
    rs, rn = radii[0] * CAT_SPACING, radii[1] * CAT_SPACING
    got = []
    for x in cats:
        rows, sal = I.keypoints(x, rs, rn)
        assert sal["clear"].mean() > 0.99
        assert (np.diff(rows) > 0).all()
        got.append(rows)
    assert (len(got[0]), len(got[1]), len(np.intersect1d(got[0], got[1]))) == CAT_PINS[radii]
