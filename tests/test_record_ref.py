"""CPU tests of the numpy pass record (_record_ref.py) that the GPU record tests compare against: the oracle's own record
(symmicp_oracle.c orc_reduce40) for QUIRKS, PAPER and P2P, the PLANE record of _plane_ref.py, the pair gates at their bounds."""
import numpy as np
import pytest

import _record_ref as R
from _plane_ref import plane_record


def pair_data(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pn = rng.standard_normal((n, 3))
    pn = (pn / np.linalg.norm(pn, axis=1, keepdims=True)).astype(np.float32)
    qn = rng.standard_normal((n, 3))
    qn = (qn / np.linalg.norm(qn, axis=1, keepdims=True)).astype(np.float32)
    idx = rng.permutation(n).astype(np.int32)
    q = np.empty_like(p)
    q[idx] = (p + 0.05 * rng.standard_normal((n, 3))).astype(np.float32)      # row i pairs with a target row near it
    idx[::11] = -1
    return p, pn, q, qn, idx


@pytest.mark.parametrize("mode", [R.MODE_QUIRKS, R.MODE_PAPER, R.MODE_P2P])
@pytest.mark.parametrize("gates", [(0.0, -2.0), (0.05, -2.0), (0.0, 0.0), (0.08, 0.2)])
def test_record_matches_oracle_reduce40(oracle, mode, gates):
    p, pn, q, qn, idx = pair_data(3001, 5)
    mcd, mnd = gates
    M2 = R.f32_max_d2(mcd)
    pivot = np.float32([0.1, -0.2, 0.05])
    S, M, kept = R.record(mode, p, pn, q, qn, idx, pivot, 0, 1.0, M2, mnd)
    ref = oracle.reduce40(p, pn, q, qn, idx=idx, pivot=None if mode == R.MODE_QUIRKS else pivot, max_d2=float(M2), min_ndot=mnd,
                          p2p=(mode == R.MODE_P2P))
    R.assert_record(ref, S, M, R.TOL_EXACT, "oracle")
    assert ref[34] == kept
    if mcd > 0 or mnd > -1:
        assert 0 < kept < (idx >= 0).sum()


@pytest.mark.parametrize("loss", [0, 1])
def test_plane_record_matches_plane_ref(loss):
    p, pn, q, qn, idx = pair_data(2000, 6)
    pivot = np.float32([0.3, 0.0, -0.1])
    M2 = R.f32_max_d2(0.06)
    S, M, kept = R.record(R.MODE_PLANE, p, pn, q, qn, idx, pivot, loss, 0.02, M2, 0.1)
    has = idx >= 0
    pp, ppn, j = p[has], pn[has], idx[has]
    keep = ~(R.dist2(pp, q[j]) > M2) & ~(R.ndot(ppn, qn[j]) < np.float32(0.1))
    ref, mag = plane_record(pp[keep], q[j[keep]], qn[j[keep]], pivot, loss, 0.02)
    assert kept == keep.sum() and 0 < kept < has.sum()
    R.assert_record(S, ref, mag, R.TOL_EXACT, "plane")
    # the fp64 rows of the solve tests agree to fp32 rounding
    ref64, _ = plane_record(pp[keep], q[j[keep]], qn[j[keep]], pivot, loss, 0.02, dtype=np.float64)
    assert np.abs(ref64[:37] - S[:37]).max() <= 1e-5 * mag[:37].max()


@pytest.mark.parametrize("mode", [R.MODE_PAPER, R.MODE_P2P, R.MODE_PLANE])
def test_weighted_record_with_unit_weights_is_the_unweighted_record(mode):
    p, pn, q, qn, idx = pair_data(1500, 7)
    S0, M0, k0 = R.record(mode, p, pn, q, qn, idx, (0, 0, 0), 0, 1.0, R.f32_max_d2(0.07), 0.0)
    S1, M1, k1 = R.record(mode, p, pn, q, qn, idx, (0, 0, 0), 1, 1e30, R.f32_max_d2(0.07), 0.0)
    assert k0 == k1 and S1[37] == k1 == S0[34] and S0[37] == 0
    assert np.array_equal(S0[:37], S1[:37])
    # a scale that bites: weights in (0, 1], their sum below the count
    S2, _, _ = R.record(mode, p, pn, q, qn, idx, (0, 0, 0), 1, 1e-3, R.f32_max_d2(0.07), 0.0)
    assert 0 < S2[34] < S2[37] == k0


def test_gates_keep_pairs_at_their_bounds():
    """d2 == max_d2 and ndot == min_ndot are kept, one ulp beyond is dropped; max_d2 is the fp32 square of the fp32 distance"""
    m = np.float32(0.1875)                              # 3/16: the square 9/256 is exact
    M2 = R.f32_max_d2(m)
    assert M2 == np.float32(9 / 256)
    p = np.zeros((4, 3), np.float32)
    q = np.zeros((4, 3), np.float32)
    q[0, 0] = m
    q[1, 0] = np.nextafter(m, np.float32(1))
    q[2, 0] = np.nextafter(m, np.float32(0))
    n1 = np.tile(np.float32([0, 0, 1]), (4, 1))
    keep = R.gate(p, n1, q, n1, M2)
    assert keep.tolist() == [True, False, True, True]
    n2 = n1.copy()
    n2[:3, 2] = [0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nextafter(np.float32(0.5), np.float32(1))]
    assert R.gate(p, n1, p, n2, 0.0, 0.5).tolist() == [True, False, True, True]
    # the engine squares the fp32 distance in fp32: not always the fp32 rounding of the double square
    ms = [0.1 + k * 1e-6 for k in range(2000)]
    assert any(R.f32_max_d2(x) != np.float32(x * x) for x in ms)
    assert all(R.f32_max_d2(x) == np.float32(np.float32(x) * np.float32(x)) for x in ms)


def test_xf_rows_and_moved_follow_the_mode():
    X = np.eye(4, dtype=np.float32)
    X[:3, 3] = [1, 2, 3]
    v = np.float32([[1, 0, 0]])
    p, pn = R.moved(X, v, v, R.MODE_QUIRKS)
    assert np.array_equal(pn, [[2, 2, 3]])            # QUIRKS: the normals take the translation
    p, pn = R.moved(X, v, v, R.MODE_PAPER)
    assert np.array_equal(p, [[2, 2, 3]]) and np.array_equal(pn, v)
