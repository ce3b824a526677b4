"""CPU tests of tests/_fpfh_ref.py, the numpy reference of the radius search and the FPFH features, against itself: the radius
sets against an O(n^2) brute force, hand-worked histograms, invariance under a rigid motion, and the margins its header records."""
import os

import numpy as np
import pytest

import _fpfh_ref as R
from conftest import GOLDEN


def _brute_sets(xyz, r):
    """independent O(n^2) statement of N(i): the full fp32 distance matrix"""
    x = np.ascontiguousarray(xyz, np.float32)
    dx = x[:, None, 0] - x[None, :, 0]
    dy = x[:, None, 1] - x[None, :, 1]
    dz = x[:, None, 2] - x[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    member = d2 <= np.float32(r) * np.float32(r)
    np.fill_diagonal(member, False)
    return member, d2


def _check_sets(xyz, r, **kw):
    member, d2 = _brute_sets(xyz, r)
    count, offs, rows, dd = R.radius_sets(xyz, r, **kw)
    assert np.array_equal(count, member.sum(1))
    for i in range(len(xyz)):
        rr, di = rows[offs[i]:offs[i + 1]], dd[offs[i]:offs[i + 1]]
        assert np.array_equal(np.sort(rr), np.nonzero(member[i])[0])
        assert np.array_equal(di.view(np.uint32), d2[i, rr].view(np.uint32))
        key = (di.view(np.uint32).astype(np.int64) << 32) | rr
        assert np.all(np.diff(key) > 0)                     # ascending (d2, row)
    return count


@pytest.mark.parametrize("r", [2.0, 5.53, 11.05])
def test_radius_sets_match_brute_force_on_cat(cat, r):
    for brute in (True, False):         # the chunked path and the cKDTree path
        _check_sets(cat["src"], r, brute=brute)


def test_radius_sets_keep_boundary_ties_on_a_lattice():
    """integer lattice, spacing 0.25, radius exactly 3 spacings: the 30 members at d2 == r2 ((3,0,0) and (2,2,1) and their images)
    are in; an interior point has the 123 - 1 lattice points of the closed ball"""
    g = np.arange(9, dtype=np.float32) * np.float32(0.25)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for brute in (True, False):
        count = _check_sets(xyz, 0.75, brute=brute)
        centre = (4 * 9 + 4) * 9 + 4
        assert count[centre] == 122
    _, offs, rows, d2 = R.radius_sets(xyz, 0.75, [centre])
    assert (d2 == np.float32(0.5625)).sum() == 30
    # a subset of query rows gives the same lists as the full run
    c_all, o_all, r_all, d_all = R.radius_sets(xyz, 0.75)
    assert np.array_equal(rows, r_all[o_all[centre]:o_all[centre + 1]])


def _fpfh64(xyz, nrm, r):
    n = len(xyz)
    count, offs, rows, d2 = R.radius_sets(xyz, r)
    c, k = R.spfh_counts(xyz, nrm, np.arange(n), offs, rows, np.float64)
    with np.errstate(all="ignore"):
        spfh = np.where(k[:, None] > 0, 100.0 * c / k[:, None], 0.0)
    return R.fpfh_from_spfh(spfh, offs, rows, d2), spfh, count


def test_two_points_with_perpendicular_normals_by_hand():
    """p0 = 0, n0 = z; p1 = x, n1 = y.  Pair (0, 1): d = x, a1 = a2 = 0 (no swap), A = z, B = y, f3 = 0, v = x cross z = -y, vn = 1,
    w = z cross (-y) = x, f2 = v.B = -1, f1 = atan2(x.y, z.y) = atan2(0, 0) = 0: bins floor(5.5) = 5, 0, 5.  Pair (1, 0) gives the
    same by symmetry (v = -z, w = -x, f2 = -1, f1 = 0).  One neighbour each: SPFH = 100 in bins 5, 11 + 0, 22 + 5; the FPFH of a
    point is its only neighbour's SPFH scaled to 100 per block: the same."""
    xyz = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0, 1], [0, 1, 0]], np.float32)
    want = np.zeros(33)
    want[[5, 11, 27]] = 100.0
    for dt in (np.float32, np.float64):
        f = R.pair_features(xyz, nrm, [0, 1], [1, 0], dt)
        assert f["valid"].all() and not f["swap"].any()
        assert np.array_equal(f["f1"], [0, 0]) and np.array_equal(f["f2"], [-1, -1]) and np.array_equal(f["f3"], [0, 0])
        assert np.array_equal(f["f4"], [1, 1]) and np.array_equal(f["vn"], [1, 1])
        assert np.array_equal(f["b1"], [5, 5]) and np.array_equal(f["b2"], [0, 0]) and np.array_equal(f["b3"], [5, 5])
    fp, spfh, count = _fpfh64(xyz, nrm, 1.5)
    assert np.array_equal(count, [1, 1])
    assert np.array_equal(spfh, np.stack([want, want])) and np.array_equal(fp, np.stack([want, want]))
    c, k = R.spfh_counts(xyz, nrm, [0, 1], *R.radius_sets(xyz, 1.5)[1:3], dtype=np.float32)
    assert np.array_equal(R.spfh_from_counts(c, k), np.stack([want, want]).astype(np.float32))


def test_swap_puts_the_frame_on_the_better_normal():
    """p0 = 0, n0 = (0, 0.6, 0.8); p1 = x, n1 = (0.8, 0.6, 0): a1 = 0 < a2 = 0.8 -> the frame moves to point 1: A = n1, B = n0, d = -x,
    f3 = -0.8; seen from point 1 (d = -x, a1 = -0.8, a2 = 0) there is no swap and f3 = -0.8 again: the pair is symmetric"""
    xyz = np.array([[0, 0, 0], [1, 0, 0]], np.float32)
    nrm = np.array([[0, 0.6, 0.8], [0.8, 0.6, 0]], np.float32)
    f = R.pair_features(xyz, nrm, [0, 1], [1, 0], np.float64)
    assert list(f["swap"]) == [True, False]
    np.testing.assert_allclose(f["f3"], [-0.8, -0.8], rtol=1e-7)
    np.testing.assert_allclose(f["f1"][0], f["f1"][1], rtol=1e-12)
    np.testing.assert_allclose(f["f2"][0], f["f2"][1], rtol=1e-12)


def test_three_points_on_a_line_with_zero_normals_are_all_zero():
    xyz = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], np.float32)
    nrm = np.zeros((3, 3), np.float32)
    fp, spfh, count = _fpfh64(xyz, nrm, 1.5)
    assert np.array_equal(count, [1, 2, 1])
    assert not spfh.any() and not fp.any()
    # ... and with normals along the line (v = d x A = 0: no frame)
    fp, spfh, _ = _fpfh64(xyz, np.tile(np.float32([1, 0, 0]), (3, 1)), 1.5)
    assert not spfh.any() and not fp.any()


def test_overflowing_weights_give_zero_blocks_not_nan():
    """two points 1e-20 apart: d2 ~ 1e-40 is a positive fp32 subnormal whose reciprocal is not finite in fp32; in fp64 it is, so the
    fp64 reference of a GIVEN spfh is computed from the fp32 weight rule's point of view by the caller -- here: the rule itself"""
    spfh = np.zeros((2, 33), np.float32)
    spfh[:, [5, 11, 27]] = 100.0
    offs = np.array([0, 1, 2], np.int64)
    rows = np.array([1, 0], np.int32)
    out = R.fpfh_from_spfh(spfh, offs, rows, np.array([np.inf, np.nan], np.float32))      # (what a non-finite block sum looks like)
    assert not out.any()
    out = R.fpfh_from_spfh(spfh, offs, rows, np.array([0.0, 0.0], np.float32))            # duplicates: d2 == 0 is skipped
    assert not out.any()


@pytest.mark.parametrize("r", [5.53, 11.05])
def test_fpfh_is_invariant_under_a_rigid_motion(cat, r):
    """fp64 FPFH of cat.pcd and of the same cloud moved by Rz(45 deg), (2.5, 0, 0) with the normals rotated along: max L1 distance over
    the points 9.6e-4 at r = 5.53 and 6.3e-4 at r = 11.05 (the moved points are rounded to fp32, which moves a few pairs over a bin edge)"""
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    Rz = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    xyz, nrm = cat["src"], cat["src_n"]
    moved = (xyz.astype(np.float64) @ Rz.T + np.array([2.5, 0, 0])).astype(np.float32)
    nrm_m = (nrm.astype(np.float64) @ Rz.T).astype(np.float32)
    a, _, ka = _fpfh64(xyz, nrm, r)
    b, _, kb = _fpfh64(moved, nrm_m, r)
    l1 = np.abs(a - b).sum(1).max()
    print("r = %g: max L1 %.3g, neighbour counts that differ: %d" % (r, l1, int((ka != kb).sum())))
    assert l1 < 0.01


def _cases(cat):
    from symmicp import synth
    yield "cat 5.53", cat["src"], cat["src_n"], 5.53, None
    yield "cat 11.05", cat["src"], cat["src_n"], 11.05, None
    c4 = synth.c4_surface(50_000)
    yield "c4_surface(50k) 0.0138", c4["src"], c4["src_n"], 0.0138, None
    c1 = synth.c4_surface(1_000_000)
    rows = np.sort(np.random.default_rng(5).choice(1_000_000, 4096, replace=False))
    sp = R.median_spacing(c1["src"], rows)
    yield "c4_surface(1M) ~30", c1["src"], c1["src_n"], R.SPACINGS_30 * sp, rows
    yield "c4_surface(1M) ~100", c1["src"], c1["src_n"], R.SPACINGS_100 * sp, rows


def test_margins_are_four_times_the_measured_error_and_few_pairs_are_ambiguous(cat):
    """the header of _fpfh_ref.py: on every cloud of the GPU test of the SPFH counts the fp32 restatement stays within a quarter of
    M_EDGE / M_SWAP of fp64, no bin differs outside the ambiguous pairs, and fewer than 1 % of the pairs are ambiguous"""
    for name, xyz, nrm, r, rows in _cases(cat):
        q = np.arange(len(xyz)) if rows is None else rows
        count, offs, rr, _ = R.radius_sets(xyz, r, q)
        m = R.measure_margins(xyz, nrm, q, offs, rr)
        print(name, "median neighbours %d" % np.median(count), m)
        assert 4 * m["edge_err"] <= R.M_EDGE and 4 * m["swap_err"] <= R.M_SWAP, (name, m)
        assert m["amb_share"] < 0.01, (name, m)
        if "1M" in name:
            assert (20 <= np.median(count) <= 40) if "30" in name else (80 <= np.median(count) <= 120)
        # fp32 against fp64 under the GPU test's own rule
        i, j, seg = R.pair_index(q, offs, rr)
        f64 = R.pair_features(xyz, nrm, i, j, np.float64)
        c64, _ = R.spfh_counts(xyz, nrm, q, offs, rr, feats=f64)
        c32, _ = R.spfh_counts(xyz, nrm, q, offs, rr, np.float32)
        allow = 2 * np.bincount(seg, R.ambiguous(f64).sum(1), minlength=len(q))
        assert np.all(np.abs(c32 - c64).sum(1) <= allow), name
