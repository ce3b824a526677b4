"""CPU tests of the colored-ICP references (tests/_color_ref.py) on the textured ridge pair (symmicp.synth.ridge_textured): they pin
the inputs of the GPU tests, so that a GPU failure cannot be blamed on them.

  * geometry alone does not fix the pose: the geometric-only 6x6 normal matrix is singular (rcond < 1e-9);
  * the fp64 colored-ICP loop (lambda = 0.968, gradient from k = 10 neighbours, 30 iterations, exact neighbours) ends below 0.01
    sample spacings from the truth -- measured 0.00251, from a start 9.0 spacings away -- with rcond >= 0.05 (measured 0.081);
  * the gradient's 3x3 system stays well conditioned: below 100 on every point (measured 27.3, median 2), and the gradient is tangent;
  * the COLOR record at lambda = 1 is PLANE's record bit for bit, at lambda = 0 the photometric rows alone, and the gates and the
    trim fraction act on the pair before its rows."""
import numpy as np
import pytest

import _color_ref as CR
import _record_ref as R

f32 = np.float32


@pytest.fixture(scope="module")
def pair():
    from symmicp import synth
    return synth.ridge_textured()


@pytest.fixture(scope="module")
def grad(pair):
    rows = CR.knn_rows(pair["tgt"], 10)
    g, degenerate, cond = CR.gradient(pair["tgt"], pair["tgt_n"], pair["tgt_i"], rows, want_cond=True)
    return dict(rows=rows, g=g, degenerate=degenerate, cond=cond)


def test_fixture_pair_is_what_the_issue_defines(pair):
    from symmicp import synth
    d = pair
    n = 20000
    assert d["src"].shape == d["tgt"].shape == d["src_n"].shape == d["tgt_n"].shape == (n, 3)
    assert d["src_i"].shape == d["tgt_i"].shape == (n,)
    assert all(d[k].dtype == np.float32 for k in ("src", "src_n", "src_i", "tgt", "tgt_n", "tgt_i"))
    assert d["spacing"] == np.sqrt(1.0 / n)
    u, v = synth.uniform01(0xC7, n, 0), synth.uniform01(0xC7, n, 1)
    assert np.array_equal(d["src"][:, 0], u.astype(f32)) and np.array_equal(d["src"][:, 1], (v - 0.03).astype(f32))
    assert np.array_equal(d["src"][:, 2], (0.05 * np.sin(10 * np.pi * u + 1.0)).astype(f32))
    tex = 0.5 + 0.2 * np.sin(2 * np.pi * (2 * u + 0.3)) * np.cos(3 * np.pi * v) + 0.15 * np.sin(2 * np.pi * (3 * v + u))
    assert np.array_equal(d["src_i"], tex.astype(f32))
    assert 0.0 < d["src_i"].min() and d["src_i"].max() < 1.0               # (an rgb field can carry it)
    assert np.abs(d["src_n"][:, 1]).max() == 0.0                           # constant along v: the ridge
    M = synth.rigid4(synth.rotation(3.0, (2, -1, 4)), np.array([0.004, 0.003, -0.002]))
    S = np.eye(4)
    S[1, 3] = 0.03
    assert np.allclose(d["truth"], M @ S, atol=0, rtol=0)
    # the target is the other sampling of the same textured surface, moved
    ut, vt = synth.uniform01(0xC8, n, 0), synth.uniform01(0xC8, n, 1)
    pt = np.stack([ut, vt, 0.05 * np.sin(10 * np.pi * ut + 1.0)], 1)
    assert np.array_equal(d["tgt"], (pt @ M[:3, :3].T + M[:3, 3]).astype(f32))
    assert abs(CR.rms_spacings(np.eye(4), d) - 9.0) < 0.01                 # the start: 9.00 spacings from the truth


def test_geometry_alone_is_singular(pair):
    rc = CR.geometric_rcond(pair)
    print("geometric-only rcond", rc)
    assert rc < 1e-9


def test_gradient_is_well_conditioned_and_tangent(pair, grad):
    print("gradient condition: max %.3g median %.3g; degenerate rows %d" % (grad["cond"].max(), np.median(grad["cond"]), grad["degenerate"].sum()))
    assert grad["degenerate"].sum() == 0
    assert grad["cond"].max() < 100.0
    gn = np.abs((grad["g"] * pair["tgt_n"].astype(np.float64)).sum(1))
    assert gn.max() < 1e-6 * np.abs(grad["g"]).max()
    # and it is the texture's gradient: against the analytic one on the tangent plane, within the k = 10 stencil's error
    assert np.isfinite(grad["g"]).all() and 2.0 < np.abs(grad["g"]).max() < 10.0


def test_knn_rows_are_the_exact_sets(pair):
    """the neighbour sets the reference gradient uses, against brute force on a sample of rows"""
    x = pair["tgt"]
    rows = CR.knn_rows(x, 10)
    for i in (0, 1, 777, 19999):
        d2 = R.dist2(np.repeat(x[i:i + 1], len(x), 0), x)
        order = np.lexsort((np.arange(len(x)), d2))[:10]
        assert np.array_equal(rows[i], order), i
        assert rows[i][0] == i


def test_color_loop_converges_where_geometry_cannot(pair, grad):
    T, rc = CR.color_icp_fp64(pair, grad["g"].astype(f32), lam=0.968, iters=30)
    rms = CR.rms_spacings(T, pair)
    print("COLOR fp64 loop: %.5f spacings, smallest rcond %.3g" % (rms, rc))
    assert rms < 0.01
    assert rc >= 0.05


def _random_pairs(rng, n=500):
    p = (rng.normal(size=(n, 3)) + 5.0).astype(f32)
    q = (p + rng.normal(scale=0.05, size=(n, 3))).astype(f32)
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(f32)
    pn, qn = unit(rng.normal(size=(n, 3))), unit(rng.normal(size=(n, 3)))
    g = rng.normal(scale=3.0, size=(n, 3)).astype(f32)
    ip, iq = rng.uniform(size=n).astype(f32), rng.uniform(size=n).astype(f32)
    return p, pn, ip, q, qn, g, iq


@pytest.mark.parametrize("loss", [0, 1])
def test_record_at_lambda_1_is_planes_and_at_0_the_photometric_rows(loss):
    p, pn, ip, q, qn, g, iq = _random_pairs(np.random.default_rng(1))
    pivot = q.mean(0)
    S1, _, kept = CR.color_record(p, pn, ip, q, qn, g, iq, None, pivot, lam=1.0, loss=loss, scale=0.05)
    Sp, _, n = R.record(R.MODE_PLANE, p, pn, q, qn, None, pivot, loss, 0.05)
    assert kept.sum() == n == len(p)
    assert np.array_equal(S1, Sp)
    S0, _, _ = CR.color_record(p, pn, ip, q, qn, g, iq, None, pivot, lam=0.0, loss=0)
    # the photometric rows alone: PLANE's form with n = g and the intensity difference added to c
    P, Q = p - pivot, q - pivot
    V = np.concatenate([np.cross(P.astype(np.float64), g.astype(np.float64)), g.astype(np.float64)], 1)
    c = ((P - Q).astype(np.float64) * g).sum(1) + (iq.astype(np.float64) - ip)
    A = V.T @ V
    assert np.allclose(S0[:21], A[np.triu_indices(6)], rtol=1e-5, atol=1e-5 * np.abs(A).max())
    assert np.allclose(S0[21:27], V.T @ c, rtol=1e-5, atol=1e-5 * np.abs(V.T @ c).max())
    assert np.isclose(S0[35], (c * c).sum(), rtol=1e-5)
    assert np.array_equal(S0[27:35], Sp[27:35]) or loss                  # once per pair, as PLANE


def test_gates_and_trimming_act_before_the_rows():
    p, pn, ip, q, qn, g, iq = _random_pairs(np.random.default_rng(2))
    pivot = q.mean(0)
    idx = np.arange(len(p))
    idx[::7] = -1
    d2 = R.dist2(p, q)
    md = float(np.sqrt(np.median(d2)))
    S, M, kept = CR.color_record(p, pn, ip, q, qn, g, iq, idx, pivot, max_d2=R.f32_max_d2(md), min_ndot=0.0, rho=0.6)
    want = (idx >= 0) & ~(d2 > R.f32_max_d2(md)) & ~(R.ndot(pn, qn) < f32(0.0))
    assert (kept & ~want).sum() == 0 and 0 < kept.sum() < want.sum()
    k = int(np.ceil(float(f32(0.6)) * want.sum()))
    tau = np.sort(d2[want])[k - 1]
    assert np.array_equal(kept, want & (d2 <= tau))
    S2, _, _ = CR.color_record(p[kept], pn[kept], ip[kept], q, qn, g, iq, idx[kept], pivot)
    assert np.array_equal(S, S2) and S[34] == kept.sum()
    assert (M[:37] >= np.abs(S[:37]) * (1 - 1e-12)).all()
