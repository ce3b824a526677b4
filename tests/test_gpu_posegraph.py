"""GPU pose-graph optimisation (symmicp_ctx_posegraph_optimize, symmicp_ctx_posegraph_pass; kernels_posegraph.hip) against the fp64
numpy restatement in tests/_posegraph_ref.py: one launch of the iteration kernel on graphs at every shape edge of the kernel (a single
edge, fewer nodes than a wave, a chain across a wave, a gather longer than a wave, the caps), the Levenberg-Marquardt loop on rings
(consistent, noisy, with a false closure), reproducibility, purity, and the whole of multiway registration on four noisy copies of the
cat.

Tolerances.  None is taken from the device.  `python tests/_posegraph_ref.py cap` prints what they are 100 x of:
  e, c, l, cost, g, hdiag   the spread between the reference and the same formulas in another association and the reverse summation
                            order, relative to the largest entry of each array: 5.59e-15 at worst (the cap graph) -> FIELD_TOL.
  delta                     per graph, the larger of (the reference's block-Jacobi PCG with the device's stop rule against the dense
                            solve) and (the dense solve of the other order's H and g against it), relative to the largest |delta|:
                            DELTA_SPREAD below -> 100 x per graph.
  final poses, cost, l      the reference loop run with the PCG and with the other order against its dense run, on the three rings:
                            max |dX| 4.44e-16, cost 1.11e-15 relative, weights 6.66e-16 -> POSE_TOL, COST_TOL, WEIGHT_TOL."""
import time

import numpy as np
import pytest

import _posegraph_ref as R

pytestmark = pytest.mark.gpu

FIELD_TOL = 100 * 5.59e-15
DELTA_SPREAD = dict(pair=3.40e-15, ring3=1.25e-15, seven=1.79e-14, chain65=1.21e-07, star130=1.25e-12, n100=1.66e-09, cap=3.46e-10)
POSE_TOL = 100 * 4.44e-16          # absolute; the rings' poses are O(1)
COST_TOL = 100 * 1.11e-15          # relative
WEIGHT_TOL = 100 * 6.66e-16        # absolute; l <= 1
# The consistent ring stops on max |d| <= min_increment = 1e-9: the last step was below 1e-9, and the error a Gauss-Newton step leaves at
# a consistent graph (where the linearisation is exact) is below the step it took.
TRUTH_TOL = 1e-9
# The pruned closure keeps a weight l < 1e-3 (asserted); it pulls with l L e, |e| = 30 degrees = 0.52, against odometry of the same
# information: a displacement of about l |e| < 5.2e-4, and both runs stop within 1e-6 of their cost.  Bound: 1e-3.
FALSE_EDGE_TOL = 1e-3


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        yield e


@pytest.fixture(scope="module")
def graphs():
    return R.pass_graphs()


def probe(eng, name, poses, edges, ref):
    """the pass probe of one graph against the reference: every field, then delta against the dense solve"""
    n, m = len(poses), len(edges)
    a = R.assemble(poses, edges, ref, R.PASS_MU)
    lam = R.PASS_LAMBDA_REL * max(a["hdiag"][i][k, k] for i in range(n) for k in range(6))
    t0 = time.perf_counter()
    r = eng.posegraph_pass(poses, edges, ref, R.PASS_MU, lam, cg_max_iterations=R.PASS_CG_MAX.get(name, 0))
    dt = time.perf_counter() - t0
    dd = R.solve_dense(a["H"], a["g"], lam, ref)
    err = {k: R.relerr(r[k], a[k]) for k in ("e", "c", "l", "g", "hdiag")}
    err["cost"] = abs(r["cost"] - a["cost"]) / a["cost"]
    err["delta"] = R.relerr(r["delta"], dd)
    ft = R.cost(R.retract(poses, dd, ref), edges, R.PASS_MU)
    err["cost_trial"] = abs(r["cost_trial"] - ft) / ft
    print("%s: n %d m %d  %.1f ms  cg %d iterations, residual %.2e  errors %s" % (
        name, n, m, 1e3 * dt, r["cg_iterations"], r["cg_residual"], " ".join("%s %.2e" % kv for kv in err.items())))
    assert r["status"] == 0 and not r["accepted"] and r["lam"] == lam
    for k in ("e", "c", "l", "g", "hdiag", "cost"):
        assert err[k] <= FIELD_TOL, (name, k, err[k])
    assert not r["g"][ref].any() and not r["hdiag"][ref].any() and not r["delta"][ref].any()
    assert np.array_equal(r["l"][[not e[2] for e in edges]], np.ones(sum(1 for e in edges if not e[2])))
    assert r["hdiag_max"] == r["hdiag"][:, range(6), range(6)].max() and r["grad_max"] == np.abs(r["g"]).max()
    assert r["delta_max"] == np.abs(r["delta"]).max()
    tol = 100 * DELTA_SPREAD[name]
    assert err["delta"] <= tol, (name, err["delta"], tol)
    # the trial cost is F at X Exp(delta): as close to the dense solve's as delta is, through F's slope (|dF| <= |g| |d delta| 6 n)
    assert err["cost_trial"] <= FIELD_TOL + tol * np.abs(a["g"]).max() * np.abs(dd).max() * 6 * n / ft, (name, err["cost_trial"])
    assert 0 < r["cg_iterations"] <= (R.PASS_CG_MAX.get(name, 0) or 6 * (n - 1)) and r["cg_residual"] <= 1e-10
    uncertain = np.array([bool(e[2]) for e in edges])
    if uncertain.any():
        assert r["l"][uncertain].min() < 0.9 and (r["l"][uncertain] > 0).all()      # the line process is exercised
    return r


@pytest.mark.parametrize("name", ["pair", "ring3", "seven", "chain65", "star130", "n100"])
def test_pass_probe_matches_the_reference(eng, graphs, name):
    probe(eng, name, *graphs[name])


def test_pass_probe_at_the_caps(eng):
    """n = 1024, m = 16384: a chain plus random closures, once, the probe only"""
    poses, edges, ref = R.pass_graphs(with_cap=True)["cap"]
    assert len(poses) == 1024 and len(edges) == 16384
    probe(eng, "cap", poses, edges, ref)


def run(eng, start, edges, **kw):
    return eng.posegraph_optimize(start, edges, R.RING_MAX_DIST, want_trace=True, **kw)


@pytest.fixture(scope="module")
def rings():
    return R.ring_cases()


def test_consistent_ring_comes_back_to_the_truth(eng, rings):
    start, edges, truth = rings["consistent"]
    r = run(eng, start, edges)
    ref = R.optimize(start, edges, max_dist=R.RING_MAX_DIST)
    print("consistent: %d iterations (reference %d), reason %d, cost %.3g -> %.3g" % (
        r["iterations"], ref["iterations"], r["stop_reason"], r["cost_initial"], r["cost_final"]))
    assert r["status"] == 0 and r["stop_reason"] == 3 and r["iterations"] == ref["iterations"]
    assert r["poses"][0].tobytes() == np.ascontiguousarray(start[0]).tobytes()          # the reference node, bit for bit
    worst = max(np.abs(R.inv_rigid(r["poses"][0]) @ r["poses"][i] - R.inv_rigid(truth[0]) @ truth[i]).max() for i in range(len(truth)))
    assert worst <= TRUTH_TOL, worst
    assert np.abs(r["poses"] - ref["poses"]).max() <= POSE_TOL
    assert not r["pruned"].any() and r["pruned_count"] == 0 and (r["weights"] > 1 - 1e-12).all()
    assert (r["poses"][:, 3] == (0, 0, 0, 1)).all()


def test_noisy_ring_matches_the_reference_run(eng, rings):
    start, edges, _ = rings["noisy"]
    t0 = time.perf_counter()
    r = run(eng, start, edges)
    dt = time.perf_counter() - t0
    ref = R.optimize(start, edges, max_dist=R.RING_MAX_DIST)
    print("noisy: %.1f ms, %d iterations (%d accepted; reference %d, %d), %d cg iterations, cost %.6g -> %.6g (reference %.6g), max |dX| %.2e, max |dl| %.2e" % (
        1e3 * dt, r["iterations"], r["accepted_steps"], ref["iterations"], ref["accepted"], r["cg_iterations"], r["cost_initial"], r["cost_final"],
        ref["cost_final"], np.abs(r["poses"] - ref["poses"]).max(), np.abs(r["weights"] - ref["weights"]).max()))
    assert r["status"] == 0 and r["cost_final"] <= r["cost_initial"]
    assert (r["iterations"], r["accepted_steps"], r["stop_reason"]) == (ref["iterations"], ref["accepted"], ref["stop_reason"])
    assert r["mu"] == ref["mu"] == R.derive_mu(edges, R.RING_MAX_DIST)
    assert abs(r["cost_initial"] - ref["cost_initial"]) <= FIELD_TOL * ref["cost_initial"]
    assert abs(r["cost_final"] - ref["cost_final"]) <= COST_TOL * ref["cost_final"]
    assert np.abs(r["poses"] - ref["poses"]).max() <= POSE_TOL
    assert np.abs(r["weights"] - ref["weights"]).max() <= WEIGHT_TOL
    # the trace is the loop: costs chain through the accepted steps, lambda follows the control rule
    tr = r["trace"]
    assert len(tr) == r["iterations"] and tr[0]["lam"] == 1e-5 * tr[0]["hdiag_max"] and tr[0]["cost"] == r["cost_initial"]
    lam, nu = tr[0]["lam"], 2.0
    for k, t in enumerate(tr):
        assert t["lam"] == lam and t["accepted"] == (t["cost_trial"] < t["cost"]) and t["status"] == 0
        if t["accepted"]:
            rho = (t["cost"] - t["cost_trial"]) / t["model_decrease"]
            lam, nu = lam * max(1.0 / 3.0, 1.0 - (2.0 * rho - 1.0) ** 3), 2.0
        else:
            lam, nu = lam * nu, 2.0 * nu
        if k + 1 < len(tr):
            nxt = tr[k + 1]["cost"]
            assert abs(nxt - (t["cost_trial"] if t["accepted"] else t["cost"])) <= FIELD_TOL * max(nxt, 1e-300)
    assert r["lambda_final"] == lam and r["grad_max"] == tr[-1]["grad_max"]


def test_false_closure_is_pruned_and_leaves_the_poses_alone(eng, rings):
    start, edges, _ = rings["false"]
    clean = rings["noisy"][1]
    assert len(edges) == len(clean) + 1 and edges[-1][2] == 1
    r = run(eng, start, edges)
    ref = R.optimize(start, edges, max_dist=R.RING_MAX_DIST)
    # the same mu for the run without the edge, so that the only difference is the edge
    rc = run(eng, start, clean, line_process_weight=r["mu"])
    print("false closure: l %.3g (reference %.3g); true closures %s; max |dX| to the run without it %.2e" % (
        r["weights"][-1], ref["weights"][-1], r["weights"][[7, 8]], np.abs(r["poses"] - rc["poses"]).max()))
    assert r["status"] == 0 and r["pruned"][-1] and r["pruned_count"] == 1 and r["weights"][-1] < 1e-3 < 0.25
    assert not r["pruned"][:-1].any() and (r["weights"][[7, 8]] > 0.9).all()            # the true closures are kept
    assert np.abs(r["poses"] - rc["poses"]).max() <= FALSE_EDGE_TOL
    assert np.abs(r["poses"] - ref["poses"]).max() <= POSE_TOL and np.abs(r["weights"] - ref["weights"]).max() <= WEIGHT_TOL


def test_two_runs_give_identical_bytes(eng, sym, rings, graphs):
    start, edges, _ = rings["false"]
    a, b = run(eng, start, edges), run(eng, start, edges)
    c = sym.posegraph_optimize(start, edges, R.RING_MAX_DIST, want_trace=True)        # a context of its own
    for x in (b, c):
        assert a["poses"].tobytes() == x["poses"].tobytes() and a["weights"].tobytes() == x["weights"].tobytes()
        assert a["trace"] == x["trace"] and a["cost_final"] == x["cost_final"] and a["lambda_final"] == x["lambda_final"]
    poses, gedges, ref = graphs["n100"]
    p, q = (eng.posegraph_pass(poses, gedges, ref, R.PASS_MU, 0.5) for _ in range(2))
    for k in ("e", "c", "l", "g", "hdiag", "delta"):
        assert p[k].tobytes() == q[k].tobytes(), k
    assert (p["cost"], p["cost_trial"], p["cg_iterations"], p["cg_residual"]) == (q["cost"], q["cost_trial"], q["cg_iterations"], q["cg_residual"])


def test_the_context_is_unchanged_around_the_call(sym, cat, rings):
    start, edges, _ = rings["noisy"]
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=12) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        before = e.align()
        x0 = e.transform()
        r = e.posegraph_optimize(start, edges, R.RING_MAX_DIST)
        assert r["status"] == 0 and np.array_equal(e.transform(), x0)
        after = e.align()
    assert before["status"] == after["status"] == 0 and before["iters"] == after["iters"]
    assert before["transform"].tobytes() == after["transform"].tobytes() and before["diffs"].tobytes() == after["diffs"].tobytes()


def test_degenerate_block_is_reported(eng, sym, rings):
    """every information matrix zero: H = 0, lambda_0 = 0, no node block is positive definite: SYMMICP_ERR_DEGENERATE after one
    launch, with the poses the call was given"""
    start, edges, _ = rings["consistent"]
    dead = [(s, t, u, T, np.zeros((6, 6))) for s, t, u, T, L in edges]
    r = eng.posegraph_optimize(start, dead, R.RING_MAX_DIST, line_process_weight=1.0, check=False)
    assert r["status"] == sym.ERR_DEGENERATE and r["iterations"] == 1 and r["stop_reason"] == 0
    assert np.array_equal(r["poses"][:, :3], start[:, :3])
    with pytest.raises(sym.SymmIcpError) as e:
        eng.posegraph_optimize(start, dead, R.RING_MAX_DIST, line_process_weight=1.0)
    assert e.value.status == sym.ERR_DEGENERATE


def test_multiway_registration_of_four_noisy_cats(sym, cat):
    """four moved copies of the cat, each with its own Gaussian noise (sigma 0.05, a thirtieth of the 1.5 point spacing): odometry
    1 -> 0, 2 -> 1, 3 -> 2 and the closure 3 -> 0 by build_pose_graph; the device's poses against the reference loop on the same edges.
    The tolerance is the reference's own spread on THESE edges, computed here as for the rings (PCG and other order against the dense
    run), times 100, and not below 100 ulps of the largest pose entry."""
    rng = np.random.default_rng(31)
    world, wn = cat["src"].astype(np.float64), cat["src_n"].astype(np.float64)
    truth = [np.eye(4)] + [R.random_pose(rng, np.radians(4.0), 1.0) for _ in range(3)]
    clouds, normals = [], []
    for X in truth:
        Xi = R.inv_rigid(X)                                   # world = X p: the cloud in its node's frame
        clouds.append((world @ Xi[:3, :3].T + Xi[:3, 3] + rng.normal(0.0, 0.05, world.shape)).astype(np.float32))
        normals.append((wn @ Xi[:3, :3].T).astype(np.float32))
    pairs = [(1, 0, 0, None), (2, 1, 0, None), (3, 2, 0, None), (3, 0, 1, None)]
    max_dist = 0.5
    t0 = time.perf_counter()
    edges, start = sym.build_pose_graph(clouds, normals, pairs, max_dist, mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30)
    t1 = time.perf_counter()
    r = sym.posegraph_optimize(start, edges, max_dist)
    t2 = time.perf_counter()
    ref = R.optimize(start, edges, max_dist=max_dist)
    pcg = lambda H, g, lam, node: R.solve_pcg(H, g, lam, node)[0]
    spread = max(np.abs(R.optimize(start, edges, max_dist=max_dist, solver=pcg)["poses"] - ref["poses"]).max(),
                 np.abs(R.optimize(start, edges, max_dist=max_dist, variant=1)["poses"] - ref["poses"]).max())
    tol = 100 * max(spread, np.finfo(np.float64).eps * np.abs(ref["poses"]).max())
    err = np.abs(r["poses"] - ref["poses"]).max()
    off = max(np.abs(r["poses"][i] - truth[i]).max() for i in range(4))
    print("cats: pairs %.2f s, optimiser %.1f ms; %d iterations (reference %d), closure l %.4f (reference %.4f), max |dX| %.2e (tolerance %.2e), %.3g from the truth" % (
        t1 - t0, 1e3 * (t2 - t1), r["iterations"], ref["iterations"], r["weights"][3], ref["weights"][3], err, tol, off))
    assert [e[:3] for e in edges] == [(1, 0, 0), (2, 1, 0), (3, 2, 0), (3, 0, 1)]
    assert r["status"] == 0 and r["iterations"] == ref["iterations"] and err <= tol, (err, tol)
    assert not r["pruned"].any() and r["weights"][3] > 0.25 and abs(r["weights"][3] - ref["weights"][3]) <= 100 * max(spread, 1e-15)
    assert off < 0.05                                         # within the noise's sigma of the truth
    m = sym.multiway_registration(clouds, normals, pairs, max_dist, engine_kwargs=dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30))
    assert m["poses"].tobytes() == r["poses"].tobytes() and len(m["edges"]) == 4
