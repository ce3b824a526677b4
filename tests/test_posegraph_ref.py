"""CPU tests of the numpy restatement of the pose-graph optimiser (tests/_posegraph_ref.py): the definitions of include/symmicp.h hold
together -- the error vanishes at a consistent graph, the cost does not depend on the world frame, the stated Jacobians are the
derivatives of the error, the residual is the one the evaluation's information matrix weighs, and the loop with the line process
converges and tells a false closure from a true one."""
import numpy as np
import pytest

import _posegraph_ref as R


def test_error_vanishes_at_a_consistent_graph():
    rng = np.random.default_rng(1)
    truth, edges = R.make_graph(rng, 6, R.ring_pairs(6) + [(0, 3, 1), (4, 1, 1)])
    a = R.assemble(truth, edges, 0, 1.0)
    assert np.abs(a["e"]).max() < 1e-14 and a["cost"] < 1e-24
    assert np.abs(a["g"]).max() < 1e-11 and np.array_equal(a["l"], np.ones(len(edges)))


def test_log_and_exp_are_inverse_and_continuous_across_the_series():
    rng = np.random.default_rng(2)
    for size in (0.0, 1e-9, 9.9e-5, 1.01e-4, 1e-2, 1.0, 3.0, np.pi - 1e-5, np.pi - 1e-9):
        w = rng.normal(size=3)
        w *= size / np.linalg.norm(w)
        back = R.log_rot(R.exp_rot(w))
        assert np.abs(back - w).max() <= 1e-12 * max(size, 1e-3) + (2e-7 if size > 3.1 else 0.0), (size, back, w)
    Rm = R.exp_rot(np.array([0.3, -0.2, 0.5]))
    assert np.abs(Rm.T @ Rm - np.eye(3)).max() < 1e-15


def test_cost_is_invariant_under_a_common_left_multiplication():
    rng = np.random.default_rng(3)
    truth, edges = R.make_graph(rng, 7, R.ring_pairs(7) + [(2, 5, 1)], noise=0.05)
    poses = R.perturb(rng, truth, 0, 0.1)
    G = R.random_pose(rng, 2.0, 5.0)
    F, F2 = R.cost(poses, edges, 3.0), R.cost(np.stack([G @ X for X in poses]), edges, 3.0)
    assert F > 0 and abs(F - F2) <= 1e-12 * F


def test_stated_jacobians_are_the_derivatives_of_the_error():
    """J_s = Ad(T) and J_t = -I against central differences of e at a consistent edge (|dJ| ~ 1e-9 at h = 1e-6: h^2 truncation plus
    1e-16 / h rounding)"""
    rng = np.random.default_rng(4)
    worst = 0.0
    for _ in range(5):
        Xs, Xt = R.random_pose(rng, 1.0, 2.0), R.random_pose(rng, 1.0, 2.0)
        T = R.relative(Xs, Xt)
        h = 1e-6
        Js, Jt = np.zeros((6, 6)), np.zeros((6, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Js[:, k] = (R.edge_error(Xs @ R.exp_pose(d), Xt, T) - R.edge_error(Xs @ R.exp_pose(-d), Xt, T)) / (2 * h)
            Jt[:, k] = (R.edge_error(Xs, Xt @ R.exp_pose(d), T) - R.edge_error(Xs, Xt @ R.exp_pose(-d), T)) / (2 * h)
        worst = max(worst, np.abs(Js - R.adjoint(T)).max(), np.abs(Jt + np.eye(6)).max())
    print("max |J_fd - J| = %.2e" % worst)
    assert worst < 1e-7


@pytest.fixture(scope="module")
def sym():
    import os
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()
    return symmicp


def test_residual_is_the_one_the_information_matrix_weighs(sym):
    """e^T L e / sum |E q - q|^2 -> 1 for a small E, L = symmicp_information_from_sums of the points q (1.000224 at 1e-2, 1.000024 at 1e-3
    with this seed: the ratio departs from 1 by O(|e|), so the bounds are 2 |e|)"""
    rng = np.random.default_rng(5)
    q = rng.uniform(-1.0, 1.0, (200, 3))
    S = q.T @ q
    L = sym.information_from_sums(len(q), q.sum(0), [S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2]])
    for size, tol in ((1e-2, 2e-2), (1e-3, 2e-3)):
        E = R.random_pose(rng, size, size)
        e = np.concatenate([R.log_rot(E[:3, :3]), E[:3, 3]])
        moved = q @ E[:3, :3].T + E[:3, 3]
        ratio = (e @ L @ e) / ((moved - q) ** 2).sum()
        print("size %g: ratio %.6f" % (size, ratio))
        assert abs(ratio - 1.0) < tol, (size, ratio)


def eight_ring(rng):
    """a noisy ring of 8, one true closure (2 -> 6) and one false one (1 -> 5: the true T turned by 30 degrees)"""
    truth, edges = R.make_graph(rng, 8, [(i, i + 1, 0) for i in range(7)] + [(7, 0, 0), (2, 6, 1), (1, 5, 1)], noise=0.01)
    s, t, unc, T, L = edges[9]
    wrong = np.eye(4)
    wrong[:3, :3] = R.exp_rot(np.array([0.0, 0.0, np.radians(30.0)]))
    edges[9] = (s, t, unc, R.relative(truth[s], truth[t]) @ wrong, L)
    return truth, edges


def test_reference_loop_converges_and_prunes_the_false_closure():
    rng = np.random.default_rng(6)
    truth, edges = eight_ring(rng)
    start = R.perturb(rng, truth, 0, 0.05)
    r = R.optimize(start, edges, ref=0, max_dist=0.05)
    print("iterations %d accepted %d reason %d cost %.4g -> %.4g l_true %.4f l_false %.3g" % (
        r["iterations"], r["accepted"], r["stop_reason"], r["cost_initial"], r["cost_final"], r["weights"][8], r["weights"][9]))
    assert r["iterations"] < 30 and r["stop_reason"] in (2, 3) and r["cost_final"] < r["cost_initial"]
    assert r["weights"][9] < 0.25 and r["pruned"][9] and r["weights"][8] > 0.9 and not r["pruned"][8]
    assert np.array_equal(r["poses"][0], start[0])
    for i in range(8):
        D = R.inv_rigid(truth[i]) @ r["poses"][i]                      # (start[0] is truth[0]: the frames agree)
        assert np.abs(D - np.eye(4)).max() < 0.05, (i, D)
    # the PCG of the device's design solves the same systems: the same run to the same poses
    r2 = R.optimize(start, edges, ref=0, max_dist=0.05, solver=lambda H, g, lam, ref: R.solve_pcg(H, g, lam, ref)[0])
    assert r2["iterations"] == r["iterations"] and np.abs(r2["poses"] - r["poses"]).max() < 1e-8
