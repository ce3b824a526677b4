"""CPU tests of the numpy restatement of registration evaluation (tests/_eval_ref.py): the two routes to the information matrix agree,
the matrix is symmetric and positive semidefinite, and the definition gives the recorded values on the golden cat pair and on the
partial-overlap surface pair."""
import math
import os

import numpy as np
import pytest

import _eval_ref as E
import _trim_ref as TR
from conftest import GOLDEN

f32 = np.float32


@pytest.fixture(scope="module")
def cat_pair(oracle):
    src, _ = oracle.pcd_read(os.path.join(GOLDEN, "cat.pcd"))
    tgt, _ = oracle.pcd_read(os.path.join(GOLDEN, "cat_out.pcd"))
    c, s = math.cos(math.pi / 4), math.sin(math.pi / 4)
    return src, tgt, np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


@pytest.fixture(scope="module")
def overlap():
    return TR.partial_overlap(20000, 0xC4)


def test_move_and_nearest_follow_the_definition():
    rng = np.random.default_rng(1)
    src, tgt = rng.random((37, 3)).astype(f32), rng.integers(0, 3, (29, 3)).astype(f32)      # a lattice target: exact ties
    X = E.random_rigid(rng)
    y = E.move(X, src)
    for i in (0, 17, 36):
        for r in range(3):
            want = f32(f32(f32(X[r, 0] * src[i, 0]) + f32(X[r, 1] * src[i, 1])) + f32(X[r, 2] * src[i, 2])) + X[r, 3]
            assert y[i, r] == f32(want)
    rows, d2 = E.nearest(y, tgt, chunk=5)
    for i in range(len(y)):
        d = y[i] - tgt
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        best = min((dd[j], j) for j in range(len(tgt)))
        assert (d2[i], rows[i]) == best


def test_gate_and_outputs():
    rng = np.random.default_rng(2)
    src, tgt = rng.random((50, 3)).astype(f32), rng.random((40, 3)).astype(f32)
    full = E.evaluate(src, tgt, None, 0.0)
    assert full["inliers"] == 50 and full["fitness"] == 1.0 and (full["nn"] >= 0).all()
    d = float(np.sqrt(np.median(full["d2_all"])))
    r = E.evaluate(src, tgt, None, d)
    keep = full["d2_all"] <= f32(f32(d) * f32(d))
    assert r["inliers"] == int(keep.sum()) and 0 < r["inliers"] < 50
    assert (r["nn"][~keep] == -1).all() and np.isinf(r["d2"][~keep]).all() and (r["nn"][keep] == full["nn_all"][keep]).all()
    assert r["rmse"] == math.sqrt(r["mean_d2"]) and r["mean_d2"] == r["sum_d2"] / r["inliers"]
    none = E.evaluate(src, tgt, None, 1e-6)
    assert none["inliers"] == 0 and none["rmse"] == 0.0 and none["mean_d2"] == 0.0 and not none["information"].any()


def test_the_two_information_routes_agree():
    rng = np.random.default_rng(3)
    for n, scale, off in ((1, 1.0, 0.0), (7, 1.0, 0.0), (500, 30.0, 100.0), (2000, 0.01, -3.0)):
        q = (rng.normal(size=(n, 3)) * scale + off).astype(f32).astype(np.float64)
        pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
        s = [math.fsum(q[:, a]) for a in range(3)]
        S = [math.fsum(q[:, a] * q[:, b]) for a, b in pairs]
        A, B = E.information_from_sums(n, s, S), E.information_explicit(q)
        mag = np.abs(B).max()
        # the closed form adds two correctly rounded sums where the explicit one rounds once: one more rounding per entry
        assert np.abs(A - B).max() <= 4 * np.finfo(np.float64).eps * mag, (n, np.abs(A - B).max(), mag)
        assert (A == A.T).all()
        w = np.linalg.eigvalsh(A)
        assert w.min() >= -1e-12 * max(w.max(), 1.0), w
        assert A[3, 3] == A[4, 4] == A[5, 5] == n


def test_information_of_the_evaluation_is_symmetric_psd(cat_pair):
    src, tgt, T = cat_pair
    r = E.evaluate(src, tgt, T, 0.5)
    L = r["information"]
    assert (L == L.T).all()
    w = np.linalg.eigvalsh(L)
    assert w.min() >= -1e-12 * w.max() and w.max() > 0


def test_cat_pair_at_the_truth(cat_pair):
    src, tgt, T = cat_pair
    r = E.evaluate(src, tgt, T, 0.5)
    assert len(src) == 3400 and r["fitness"] == 1.0 and r["inliers"] == 3400
    assert (r["nn"] == np.arange(3400)).all()
    assert abs(math.sqrt(float(r["d2"].max())) - 9.54e-7) < 0.005e-7


def test_cat_pair_at_the_identity(cat_pair):
    src, tgt, _ = cat_pair
    assert E.evaluate(src, tgt, None, 1.0)["inliers"] == 92


def test_partial_overlap_fitness(overlap):
    d = overlap
    at_truth = E.evaluate(d["src"], d["tgt"], d["truth"], 2 * d["spacing"])
    at_identity = E.evaluate(d["src"], d["tgt"], None, 2 * d["spacing"])
    assert round(at_truth["fitness"], 4) == 0.5835
    assert round(at_identity["fitness"], 4) == 0.2052
