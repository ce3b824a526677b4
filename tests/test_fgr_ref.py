"""CPU tests of tests/_fgr_ref.py, the numpy restatement of Fast Global Registration that tests/test_gpu_fgr.py holds the device to:
the draws against plain integer arithmetic, a hand-worked tuple and a hand-worked pass, the library's host solve on a restated record,
and the numbers of the fp64 method on the matches of the fp64 reference pipeline (reference FPFH of tests/_fpfh_ref.py, SciPy k-d tree
for the matching: the fixtures tests/test_global_ref.py pins) as regression pins.

These tests check the reference itself, so all but one of them would pass without the library's FGR entry points: only
test_restatement_defaults_are_the_librarys touches the new API (tests/test_fgr_abi.py and tests/test_gpu_fgr.py are the ones that hold
the feature).

Measured with the defaults (64 iterations, mu / 1.4 every 4, tuple_scale 0.95, 1000 tuples, min(100 m, 2^24) trials); the errors are
those of fgr64(), E is the largest displacement between fgr32()'s and fgr64()'s final transforms over the paired source points, as a
fraction of max_dist:

    input (matches)                 seed  accepted trials  M      rotation error  RMS to truth     E
    cat (3 196)                     1     314 161          3 000  0.0466 deg      0.0196           2.39e-6
                                    2     314 182          3 000  0.0268          0.0110           1.47e-6
                                    3     314 124          3 000  0.0327          0.0127           3.44e-6
    bumps (705)                     1     322              966    0.1452          0.2436 spacings  1.69e-5
                                    2     373              1 119  0.0566          0.2857           1.25e-5
                                    3     376              1 128  0.2374          0.3713           2.18e-5
                                    4     364              1 092  0.1183          0.2239           2.94e-5
    bumps shifted by 1e4 (786)      1     529              1 587  0.1384          0.3638           3.38e-5
                                    2     528              1 584  0.2252          0.3605           1.85e-5
                                    3     524              1 572  0.2254          0.2592           2.83e-5
                                    4     518              1 554  0.2699          0.2823           3.32e-5

    The worst E is 3.38e-5; _fgr_ref.E = 4e-5 is that value rounded up, with room for another BLAS or numpy build.  No seed was
    dropped: on every one of them the two precisions end in the same basin.
For comparison DESIGN.md records 0.32 - 0.77 spacings for RANSAC with one refit on the bumps pair."""
import numpy as np
import pytest

import _fgr_ref as R
import _global_ref as G

F = np.float32
CAT_R = 11.05

# (seed, accepted trials, M, rotation error in degrees, RMS to truth in spacings) of fgr64()
PINS = {
    "cat": [(1, 314161, 3000, 0.0466, 0.0196), (2, 314182, 3000, 0.0268, 0.0110), (3, 314124, 3000, 0.0327, 0.0127)],
    "bumps": [(1, 322, 966, 0.1452, 0.2436), (2, 373, 1119, 0.0566, 0.2857), (3, 376, 1128, 0.2374, 0.3713), (4, 364, 1092, 0.1183, 0.2239)],
    "bumps_shifted": [(1, 529, 1587, 0.1384, 0.3638), (2, 528, 1584, 0.2252, 0.3605), (3, 524, 1572, 0.2254, 0.2592),
                      (4, 518, 1554, 0.2699, 0.2823)],
}
PIN_REL = 0.02          # the pinned errors are rounded to four decimals; a different BLAS moves the fp64 method far less than this


def cat_truth():
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    return np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def _bumps(shift=None):
    b = G.bumps_pair(shift=shift)
    fs, ft = G.reference_fpfh(b["src"], b["src_n"], b["radius"]), G.reference_fpfh(b["tgt"], b["tgt_n"], b["radius"])
    b["pairs"] = G.mutual_matches_kdtree(fs, ft)
    return b


@pytest.fixture(scope="module")
def inputs(cat):
    """the three inputs through the fp64 reference pipeline -> {name: dict(src, tgt, pairs, truth, max_dist, spacing)}"""
    fs, ft = G.reference_fpfh(cat["src"], cat["src_n"], CAT_R), G.reference_fpfh(cat["tgt"], cat["tgt_n"], CAT_R)
    out = dict(cat=dict(src=cat["src"], tgt=cat["tgt"], pairs=G.mutual_matches_kdtree(fs, ft), truth=cat_truth(), max_dist=CAT_R / 4, spacing=1.0))
    out["bumps"] = _bumps()
    out["bumps_shifted"] = _bumps((1e4, 1e4, 1e4))
    return out


# ---- tuple test ------------------------------------------------------------------------------------------------------------------
def _mix64(z):
    M = (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
    return z ^ (z >> 31)


def test_draws_against_plain_integer_arithmetic():
    M = (1 << 64) - 1
    for seed, m in ((0, 3), (1, 705), (12345678901234567, 3196), (2 ** 64 - 1, 2 ** 31 - 1)):
        base = _mix64((seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D) & M)
        want = [[((_mix64((base + (3 * t + j + 1) * 0x9E3779B97F4A7C15) & M) >> 32) * m) >> 32 for j in range(3)] for t in range(50)]
        got = R.tuple_draws(seed, 50, m)
        assert got.tolist() == want and got.min() >= 0 and got.max() < m
    # stream 1 is not RANSAC's stream 0
    assert not np.array_equal(R.tuple_draws(1, 50, 705), G.draws(1, 50, 705))
    assert R.default_trials(705) == 70500 and R.default_trials(10 ** 6) == 2 ** 24


def test_hand_worked_tuple():
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], F)
    P = tri[None]
    # edges 1, 2, 1 against the same scaled by s^2: accepted iff s^2 >= 0.95^2 and 1 / s^2 >= 0.95^2
    assert not R.edge_fails32(P, F(0.96) * P, 0.95)[0] and R.edge_fails32(P, F(0.94) * P, 0.95)[0]
    assert not R.edge_fails32(P, P / F(0.96), 0.95)[0] and R.edge_fails32(P, P / F(0.94), 0.95)[0]
    assert not R.edge_fails32(P, P, 1.0)[0]                                  # a congruent triangle passes at scale 1
    far = tri.copy(); far[2] = (0, 1.2, 0)                                  # one edge 1 -> 1.2: 1 < 0.9025 x 1.44
    assert R.edge_fails32(P, far[None], 0.95)[0]
    # m = 3: exactly the trials whose draws are a permutation are accepted, in trial order
    c = R.tuple_draws(5, 300, 3)
    perm = np.array([len(set(r)) == 3 for r in c.tolist()])
    sel, acc = R.tuple_set(tri, tri, seed=5)
    assert acc == perm.sum() > 0 and sel.tolist() == c[perm].reshape(-1).tolist()
    sel, acc2 = R.tuple_set(tri, tri, seed=5, max_tuples=2)
    assert acc2 == acc and sel.tolist() == c[perm][:2].reshape(-1).tolist()
    sel, acc = R.tuple_set(tri, tri, max_tuples=0)
    assert acc == 0 and sel.tolist() == [0, 1, 2]


def test_restatement_defaults_are_the_librarys():
    """the defaults of fgr() here, of symmicp.fgr() and of symmicp_fgr_config_default are one set"""
    import ctypes as C
    import inspect
    import symmicp as sym
    cfg = sym.FgrConfig()
    sym.lib().symmicp_fgr_config_default(C.byref(cfg))
    lib_defaults = dict(iterations=cfg.iterations, decrease_every=cfg.decrease_every, division_factor=cfg.division_factor,
                        tuple_scale=cfg.tuple_scale, max_tuples=cfg.max_tuples, tuple_trials=cfg.tuple_trials, seed=cfg.seed)
    for f in (R.fgr, sym.fgr, sym.Engine.fgr):
        d = {k: v.default for k, v in inspect.signature(f).parameters.items() if k in lib_defaults}
        assert set(d) == set(lib_defaults), f
        for k, v in d.items():
            assert F(v) == F(lib_defaults[k]), (f, k, v, lib_defaults[k])
    assert (R.OK, R.ERR_DEGENERATE, R.ERR_NO_CONSENSUS) == (sym.OK, sym.ERR_DEGENERATE, sym.ERR_NO_CONSENSUS)


# ---- schedule and pass ---------------------------------------------------------------------------------------------------------------
def test_schedule():
    mu = R.schedule(F(100.0), 1.0, iterations=12, decrease_every=4, division_factor=2.0)
    assert mu.tolist() == [50.0] * 4 + [25.0] * 4 + [12.5] * 4
    mu = R.schedule(F(100.0), 3.0, iterations=5, decrease_every=1, division_factor=1e6)
    assert mu.tolist() == [9.0] * 5                                          # the floor in one step
    mu = R.schedule(F(0.5), 1.0, iterations=3)
    assert mu.tolist() == [0.5] * 3                                          # D2 below delta^2: mu stays
    assert R.d2_max(np.array([[3, 0, 0]], F), np.array([[0, 4, 1]], F)) == F(17.0)


def test_hand_worked_pass():
    p, q = np.array([[1, 2, 3]], F), np.array([[1, 2, 2]], F)
    for dtype in (np.float32, np.float64):
        S, Mg, l = R.pass_record(p, q, np.eye(4), 1.0, dtype)
        assert l[0] == 0.25                                                  # d = (0, 0, 1), r2 = 1, t = 1 / 2
        J = np.array([[0, 3, -2, 1, 0, 0], [-3, 0, 1, 0, 1, 0], [2, -1, 0, 0, 0, 1]], np.float64)
        A, b = 0.25 * J.T @ J, 0.25 * J.T @ np.array([0, 0, 1.0])
        assert S[:21].tolist() == [A[r, c] for r in range(6) for c in range(r, 6)]
        assert S[0] == 3.25 and S[21:27].tolist() == b.tolist() == [0.5, -0.25, 0, 0, 0, 0.25]
        assert S[27:33].tolist() == [0.25, 0.5, 0.75, 0.25, 0.5, 0.5]
        assert S[33:40].tolist() == [0, 0.25, 0.25, 1, 1, 0, 0]
        assert np.array_equal(Mg[:38], np.abs(S[:38]))
    # the transform is applied to p alone
    X = np.eye(4); X[2, 3] = -1.0
    S, _, l = R.pass_record(p, q, X, 1.0)
    assert l[0] == 1.0 and S[35] == 0 and S[27:30].tolist() == [1, 2, 2]


def test_plane_solve_recovers_a_rigid_motion_from_the_restated_record():
    import symmicp as sym
    rng = np.random.default_rng(7)
    p = (rng.random((200, 3)) * 2 - 1).astype(F)
    from symmicp import synth
    Rm, t = synth.rotation(3.0, (0.2, -0.5, 0.8)), np.array([0.05, -0.02, 0.03])
    q = (p.astype(np.float64) @ Rm.T + t).astype(F)
    X = np.eye(4, dtype=F)
    for _ in range(5):
        S, _, _ = R.pass_record(p, q, X, 1.0, weights=np.ones(len(p), F))
        assert S[34] == 200 and S[37] == 200
        st, *_, Xi = sym.solve(sym.MODE_PLANE, S)
        assert st == sym.OK
        X = R.mat4_mul32(Xi, X)
    assert np.abs(X[:3, :3] - Rm).max() < 2e-6 and np.abs(X[:3, 3] - t).max() < 2e-6
    # ... and the fp64 solve of this module agrees with it
    X64 = np.eye(4)
    for _ in range(5):
        X64 = R.solve64(R.pass_record(p, q, X64, 1.0, np.float64, weights=np.ones(len(p)))[0]) @ X64
    assert np.abs(X64 - X).max() < 2e-6
    # degenerate records come back as such: too few, collinear
    assert R.solve64(R.pass_record(p[:5], q[:5], np.eye(4), 1.0, np.float64, weights=np.ones(5))[0]) is None
    line = np.zeros((50, 3), F); line[:, 0] = np.linspace(-1, 1, 50)
    S, _, _ = R.pass_record(line, line, np.eye(4), 1.0, weights=np.ones(50, F))
    assert R.solve64(S) is None and sym.solve(sym.MODE_PLANE, S)[0] == sym.ERR_DEGENERATE


# ---- the method ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cat", "bumps", "bumps_shifted"])
def test_pins_of_the_fp64_method_and_E(inputs, name):
    d = inputs[name]
    worst = 0.0
    for seed, accepted, M, rot, rms in PINS[name]:
        r64 = R.fgr64(d["src"], d["tgt"], d["pairs"], d["max_dist"], seed=seed)
        assert r64["status"] == R.OK and r64["iterations"] == 64
        assert (r64["accepted"], len(r64["set"])) == (accepted, M), (seed, r64["accepted"], len(r64["set"]))
        got = (G.rotation_error_deg(r64["T"], d["truth"]), G.rms_to_truth(r64["T"], d["truth"], d["src"]) / d["spacing"])
        print(name, seed, "rotation error %.4f deg, RMS %.4f spacings" % got)
        assert abs(got[0] - rot) <= PIN_REL * rot + 5e-5 and abs(got[1] - rms) <= PIN_REL * rms + 5e-5, (seed, got)
        r32 = R.fgr32(d["src"], d["tgt"], d["pairs"], d["max_dist"], seed=seed)
        assert r32["status"] == R.OK and np.array_equal(r32["set"], r64["set"]) and np.array_equal(r32["mu_trace"], r64["mu_trace"])
        e = R.displacement(r32["T"], r64["T"], d["src"][d["pairs"][:, 0]]) / d["max_dist"]
        print(name, seed, "E %.3e" % e)
        worst = max(worst, e)
    assert worst <= R.E, worst
    # the schedule: sixteen divisions by 1.4 (a factor of 218) in 64 iterations, never below its floor
    mu = r64["mu_trace"]
    assert (np.diff(mu) <= 0).all() and len(np.unique(mu)) == 16 and mu[-1] > R.delta2(d["max_dist"])


def test_tuple_test_matters_on_the_hard_pair(inputs):
    """6.5 % of the bumps pair's matches are true; the tuple test raises that before the loop sees them"""
    d = inputs["bumps"]
    x = d["src"][d["pairs"][:, 0]].astype(np.float64) @ d["truth"][:3, :3].T + d["truth"][:3, 3]
    true = np.linalg.norm(x - d["tgt"][d["pairs"][:, 1]], axis=1) <= d["max_dist"]
    assert 0.05 < true.mean() < 0.08
    sel, _ = R.tuple_set(*G.pivoted(d["src"], d["tgt"], d["pairs"])[:2], seed=1)
    assert true[sel].mean() > 0.25
    on = R.fgr64(d["src"], d["tgt"], d["pairs"], d["max_dist"], seed=1)
    off = R.fgr64(d["src"], d["tgt"], d["pairs"], d["max_dist"], max_tuples=0)
    rms = [G.rms_to_truth(r["T"], d["truth"], d["src"]) / d["spacing"] for r in (on, off)]
    assert rms[0] < rms[1] < 1.0
