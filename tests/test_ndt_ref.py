"""CPU tests of the numpy restatement of SYMMICP_MODE_NDT (tests/_ndt_ref.py) on its own: the map, the weight and the restated loop
behave as the mode's definition says, before any of it is compared with the device (tests/test_gpu_ndt_map.py, tests/test_gpu_ndt.py)."""
import math

import numpy as np
import pytest

import _ndt_ref as R

F = np.float32


@pytest.fixture(scope="module")
def c4():
    from symmicp import synth
    d = synth.c4_surface(4000)
    pivot = d["tgt"].astype(np.float64).mean(0).astype(F)
    nmap = R.with_factors(R.build_map(d["tgt"], 0.1))
    return dict(d, pivot=pivot, map=nmap)


def test_map_of_the_surface_pair(c4):
    m = c4["map"]
    assert len(m["key"]) == 207                                  # of 279 occupied voxels
    assert np.all(np.diff(m["key"].astype(np.int64)) > 0)
    assert np.all(m["count"] >= 6)
    # the factors give M back, and M inverts the inflated covariance
    assert np.allclose(R.M_of(m["axes"], m["inv_eig"]), m["M"], rtol=0, atol=1e-6 * np.abs(m["M"]).max())
    assert np.all(np.diff(m["lam"], axis=1) >= 0) and np.all(m["lam"][:, 0] >= 0.01 * m["lam"][:, 2] * (1 - 1e-6))


@pytest.mark.parametrize("neighbors,first_items", [(7, 18498), (1, 3533)])
def test_restated_loop_converges(c4, neighbors, first_items):
    """12 passes end closer to the truth than they start; the first pass's item count is the prototype's"""
    X, log = R.loop(c4["map"], c4["src"], c4["pivot"], 12, neighbors)
    assert log[0][0] == first_items
    r0, t0 = R.pose_error(np.eye(4), c4["truth"])
    r1, t1 = R.pose_error(X, c4["truth"])
    assert r1 < r0 and t1 < t0, (r0, t0, r1, t1)
    assert r1 < 0.2 and t1 < 2e-3, (r1, t1)
    assert log[-1][1] > log[0][1]                               # sum of the weights: the score went up


def test_weight_is_exp_to_a_few_ulp_and_monotone():
    x = -np.random.default_rng(20261020).uniform(0.0, 64.0, 200000).astype(F)
    x = np.sort(np.concatenate([x, F([0.0, -0.0, np.nextafter(F(-64), F(0))])]))
    w = R.weight(x)
    e = np.exp(x.astype(np.float64))
    assert np.max(np.abs(w.astype(np.float64) - e) / e) <= 2.0 ** -22
    assert np.all(np.diff(w) >= 0)
    edge = R.weight(F([-64.0, -1e30, -np.inf, np.nan, 1.0, np.inf, 0.0, -0.0]))
    assert np.array_equal(edge, F([0, 0, 0, 0, 1, 1, 1, 1]))


def test_gauss_constants():
    d1, d2 = R.gauss(0.55)
    assert abs(d1 - (-2.217225244)) < 1e-9 and abs(d2 - 0.433123004) < 1e-8
    # the definition, term by term
    c1, c2 = 10 * 0.45, 0.55
    d3 = -math.log(c2)
    assert d1 == -math.log(c1 + c2) - d3
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(R.NdtError):
            R.gauss(bad)


def test_items_of_one_point_by_hand():
    """a 3 x 1 x 1 row of voxels, the middle one empty: the own cell and the face neighbours of a point, cell by cell"""
    rng = np.random.default_rng(3)
    a = rng.uniform(0.0, 1.0, (8, 3)).astype(F)
    b = a + F([2.0, 0.0, 0.0])
    nmap = R.with_factors(R.build_map(np.concatenate([a, b]), 1.0))
    assert list(nmap["key"]) == [0, 2] and list(nmap["grid"]) == [0, 0, 0, 3, 1, 1]
    y = F([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5], [0.5, 1.5, 0.5]])
    pt, row, own = R.items(nmap, y, 7)
    assert list(own) == [0, -1, 1, -1, -1]
    assert sorted(zip(pt.tolist(), row.tolist())) == [(0, 0), (1, 0), (1, 1), (2, 1), (3, 1), (4, 0)]
    pt, row, _ = R.items(nmap, y, 1)
    assert sorted(zip(pt.tolist(), row.tolist())) == [(0, 0), (2, 1)]


def test_grid_refuses_cells_at_2_to_the_23():
    x = F([[0, 0, 0], [1, 1, 1], [8388608.0, 0, 0]])
    with pytest.raises(R.NdtError):
        R.grid(x, 1.0)
    R.grid(x, 2.0)
