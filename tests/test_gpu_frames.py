"""GPU tests: registration in other coordinate frames (run with -m gpu on a real MI355X).

(a) units: the same problem in clouds scaled by a power of two s must run the same passes bit for bit -- the same pairs,
    squared distances times s^2, every slot of the 40-double record times s^dim (tests/_frames.py), the same rotations and
    translations times s, the same stop and the same index shape.  The PAPER solve equilibrates its 6 x 6 system, so its
    conditioning checks do not depend on the unit either: the device-driven loop keeps running at 2^12.
(b) offsets: clouds far from the origin (coarsely quantised fp32, many exact ties): pairs and distances bit-exact against the
    oracle's brute-force NN on the positions the engine reports, the record against orc_reduce40, the final transform
    against oracle.align.
(c) shapes the grid fits badly: slabs, needles, far-apart clusters, negative coordinates, a target of one repeated point.
(d) all of the above under every forced search regime, in child processes (the switches are read once per process).
"""
import os
import sys

import numpy as np
import pytest

from _frames import scale_record

pytestmark = pytest.mark.gpu

TOL_SUM = 1e-11       # relative, on the fp64 reduction record (different summation order)
TOL_T = 1e-4          # final transforms, normalised units: rotation absolute, translation / extent


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


_DATA = {}


def _data(name, cat=None):
    if name not in _DATA:
        from symmicp import synth
        if name == "cat":
            _DATA[name] = dict(src=cat["src"], src_n=cat["src_n"], tgt=cat["tgt"], tgt_n=cat["tgt_n"])
        elif name == "c4":
            _DATA[name] = synth.c4_surface(100_000)
        elif name == "c4_8k":
            _DATA[name] = synth.c4_surface(8000)
        elif name == "c5":
            _DATA[name] = synth.c5_scan(64 * 1500)
    return _DATA[name]


# ----------------------------------------------------------------------------------------------
# (a) power-of-two units
# ----------------------------------------------------------------------------------------------
# settings that carry a length: scaled with the clouds (diff_threshold: the stop rule compares sum |p - q| with it)
_LENGTHS = ("max_corr_dist", "eps_translation", "diff_threshold")
_REGIME_STATS = ("grid_level", "tree_levels", "pass_blocks", "passes", "packet_fallbacks", "loop_straggler_passes")


def _cfg(cfg, s):
    out = dict(cfg)
    out.setdefault("diff_threshold", 1.0)
    for k in _LENGTHS:
        if k in out:
            out[k] = float(np.float32(out[k]) * np.float32(s))
    return out


def _engine(sym, d, s, cfg, loss):
    f = np.float32(s)
    e = sym.Engine(**_cfg(cfg, s))
    e.set_target(d["tgt"] * f, d["tgt_n"])                 # exact: a power of two
    e.set_source(d["src"] * f, d["src_n"])
    if loss is not None:
        e.set_robust_loss(loss[0], float(np.float32(loss[1]) * f))
    return e


def _run_passes(sym, d, s, cfg, loss, n):
    passes = []
    with _engine(sym, d, s, cfg, loss) as e:
        it = e.begin()
        for _ in range(n):
            idx, d2 = e.correspondences()
            passes.append(dict(it, idx=idx, d2=d2, X=e.transform().copy()))
            if it["status"] != 0:
                break
            it = e.step(check=False)
        passes.append(dict(it, idx=None, d2=None, X=e.transform().copy()))
        st = e.stats()
    return passes, st


def _run_align(sym, d, s, cfg, loss):
    with _engine(sym, d, s, cfg, loss) as e:
        r = e.align()
        st = e.stats()
    return r, st


def _assert_transform_scaled(X0, X, s, what):
    f = np.float32(s)
    assert np.array_equal(X[:3, :3], X0[:3, :3]), (what, X, X0)
    assert np.array_equal(X[:3, 3], X0[:3, 3] * f), (what, X[:3, 3], X0[:3, 3] * f)
    assert np.array_equal(X[3], X0[3]), what


def _assert_passes_scaled(p0, p1, s, p2p, quirks=False):
    f = np.float32(s)
    assert len(p0) == len(p1)
    # QUIRKS moves the normals by the translation too (myicp.cpp:137): from the second pass on its rows mix units, and only the
    # first pass and the first increment are unit-free (one step is driven); PAPER and P2P are unit-free on every pass
    for k, (a, b) in enumerate(zip(p0, p1)):
        assert a["status"] == b["status"] and a["iter"] == b["iter"], (k, a["status"], b["status"])
        if a["idx"] is not None:
            assert np.array_equal(a["idx"], b["idx"]), (k, int((a["idx"] != b["idx"]).sum()))
            assert np.array_equal(a["d2"] * (f * f), b["d2"]), k
        assert np.float32(a["diff"]) * f == np.float32(b["diff"]), k
        if not (quirks and k > 0):
            assert np.array_equal(scale_record(a["sums"], s, p2p), b["sums"]), (k, np.flatnonzero(scale_record(a["sums"], s, p2p) != b["sums"]))
        assert a["rcond"] == b["rcond"], (k, a["rcond"], b["rcond"])
        assert a["pairs"] == b["pairs"], k
        _assert_transform_scaled(a["X"], b["X"], s, k)
        _assert_transform_scaled(a["increment"], b["increment"], s, k)


# name, cloud, mode, corr, config, robust loss (name, scale in the unscaled frame), passes driven one by one
_UNIT_CASES = {
    "cat-paper-tree": ("cat", "MODE_PAPER", "CORR_TREE", dict(max_iters=30), None, 8),
    "cat-quirks-identity": ("cat", "MODE_QUIRKS", "CORR_IDENTITY", dict(), None, 1),      # (see _assert_passes_scaled)
    "cat-p2p-tree": ("cat", "MODE_P2P", "CORR_TREE", dict(max_iters=30), None, 8),
    "cat-paper-tree-huber": ("cat", "MODE_PAPER", "CORR_TREE",
                             dict(max_iters=30, max_corr_dist=40.0, eps_rotation=1e-5, eps_translation=1e-3), ("huber", 2.0), 8),
    "c4-paper-tree": ("c4", "MODE_PAPER", "CORR_TREE", dict(max_iters=30, fixed_iters=1), None, 6),
    "c5-paper-tree": ("c5", "MODE_PAPER", "CORR_TREE", dict(max_iters=30), None, 6),
}
_UNIT_PARAMS = [(c, k) for c in _UNIT_CASES for k in (-12, -6, 6, 12) + ((14,) if c.startswith("cat") else ())]
_UNSCALED = {}


def _case(sym, cat, name):
    cloud, mode, corr, cfg, loss, n = _UNIT_CASES[name]
    cfg = dict(cfg, mode=getattr(sym, mode), corr=getattr(sym, corr))
    return _data(cloud, cat), cfg, loss, n, mode == "MODE_P2P", mode == "MODE_QUIRKS"


@pytest.mark.parametrize("name,k", _UNIT_PARAMS, ids=["%s-2^%d" % p for p in _UNIT_PARAMS])
def test_power_of_two_units_run_the_same_passes(sym, cat, name, k):
    d, cfg, loss, n, p2p, quirks = _case(sym, cat, name)
    s = 2.0 ** k
    if name not in _UNSCALED:
        a0 = [_run_align(sym, d, 1.0, cfg, loss) for _ in range(2)]       # twice: LOOP_SLOW hand-backs depend on timing
        _UNSCALED[name] = (_run_passes(sym, d, 1.0, cfg, loss, n), a0)
    (p0, st0), a0 = _UNSCALED[name]
    p1, st1 = _run_passes(sym, d, s, cfg, loss, n)
    _assert_passes_scaled(p0, p1, s, p2p, quirks)
    for key in _REGIME_STATS:
        assert st0[key] == st1[key], (key, st0[key], st1[key])
    assert st0["kernel_launches"][7] == st1["kernel_launches"][7]            # passes repaired after skipping the walk
    if quirks:
        return
    r1, sa1 = _run_align(sym, d, s, cfg, loss)
    for r0, sa0 in a0:
        assert r0["status"] == r1["status"] == 0 and r0["iters"] == r1["iters"], (r0["status"], r1["status"], r0["iters"], r1["iters"])
        _assert_transform_scaled(r0["transform"], r1["transform"], s, "align")
        f = np.float32(s)
        assert np.float32(r0["diff_initial"]) * f == np.float32(r1["diff_initial"])
        assert np.float32(r0["diff_final"]) * f == np.float32(r1["diff_final"])
        assert np.array_equal(r0["diffs"] * f, r1["diffs"])
        assert (sa0["grid_level"], sa0["tree_levels"]) == (sa1["grid_level"], sa1["tree_levels"])
    # the device-driven loop must not hand its solves back to the host because of the unit
    lp0 = min(sa0["loop_passes"] for _, sa0 in a0)
    assert sa1["loop_passes"] >= lp0, (sa1["loop_passes"], lp0, sa1["passes"])
    if name.startswith("c4"):
        assert lp0 > 0
        print("%s 2^%d: loop_passes / passes = %d / %d (unscaled %d / %d)"
              % (name, k, sa1["loop_passes"], sa1["passes"], lp0, a0[0][1]["passes"]))


# ----------------------------------------------------------------------------------------------
# (b) frames far from the origin
# ----------------------------------------------------------------------------------------------
def _nudge(src, k):
    """a guess that turns the source by k/2 degrees about its centre and moves it by k/100 of its extent"""
    from symmicp import synth
    c = src.astype(np.float64).mean(0)
    R = synth.rotation(0.5 * k, (0.2, 1.0, -0.4))
    return synth.rigid4(R, c - R @ c + 0.01 * k * np.ptp(src, 0)).astype(np.float32)


def _check_passes_against_oracle(sym, oracle, e, src, src_n, tgt, tgt_n, mode, apply_mode, n, records=True):
    """drive n passes; after each: pairs + distances bit-exact against oracle.nn_brute on the positions the engine used,
    the record against orc_reduce40 at TOL_SUM.  A solve flagged degenerate (legitimately: QUIRKS far from the origin) does not
    end the run: the next pass starts again from a guess.  Returns the number of passes that followed a solve."""
    it = e.begin()
    solved = 0
    for done in range(n):
        idx, d2 = e.correspondences()
        X = e.transform()
        if apply_mode == sym.APPLY_INCREMENTAL:
            p, pn = e.source()
        else:
            p = oracle.apply(X, src, True)
            pn = oracle.apply(X, src_n, mode == sym.MODE_QUIRKS)       # QUIRKS moves normals by the translation (myicp.cpp:137)
        ri, rd = oracle.nn_brute(p, tgt)
        assert np.array_equal(idx, ri), (done, int((idx != ri).sum()))
        assert np.array_equal(d2, rd), (done, int((d2 != rd).sum()))
        if records:
            S = oracle.reduce40(p, pn, tgt, tgt_n, idx=idx, pivot=None if mode == sym.MODE_QUIRKS else e.pivot(),
                                p2p=(mode == sym.MODE_P2P))
            g = np.asarray(it["sums"], np.float64)
            assert np.abs(g - S).max() <= TOL_SUM * np.abs(S).max(), (done, np.abs(g - S).max() / np.abs(S).max())
        it = e.step(check=False)
        if it["status"] != 0:
            it = e.begin(_nudge(src, done + 1))
        else:
            solved += 1
    return solved


def _centred_transform(X, o):
    """X (x -> R x + t) written for coordinates about o: translation R o + t - o, in fp64"""
    X = np.asarray(X, np.float64)
    return X[:3, :3], X[:3, 3] + X[:3, :3] @ o - o


_OFFSET_PARAMS = [(c, o, m, a) for c in ("cat", "c4_8k") for o in (1e2, 1e3, 1e4)
                  for m in ("MODE_PAPER", "MODE_QUIRKS") for a in ("APPLY_INCREMENTAL", "APPLY_CUMULATIVE")]


@pytest.mark.parametrize("cloud,o,mode,apply_mode", _OFFSET_PARAMS, ids=["%s-%g-%s-%s" % (c, o, m[5:].lower(), a[6:].lower())
                                                                        for c, o, m, a in _OFFSET_PARAMS])
def test_offset_frames_stay_exact(sym, oracle, cat, cloud, o, mode, apply_mode):
    d = _data(cloud, cat)
    mode, apply_mode = getattr(sym, mode), getattr(sym, apply_mode)
    lo = np.minimum(d["src"].min(0), d["tgt"].min(0)).astype(np.float64)
    hi = np.maximum(d["src"].max(0), d["tgt"].max(0)).astype(np.float64)
    E = float(np.max(hi - lo))
    off = o * E * np.array([1.0, -0.7, 0.3])
    src = (d["src"].astype(np.float64) + off).astype(np.float32)
    tgt = (d["tgt"].astype(np.float64) + off).astype(np.float32)
    n = 8
    with sym.Engine(mode=mode, corr=sym.CORR_TREE, apply=apply_mode, max_iters=n, fixed_iters=1) as e:
        e.set_target(tgt, d["tgt_n"])
        e.set_source(src, d["src_n"])
        solved = _check_passes_against_oracle(sym, oracle, e, src, d["src_n"], tgt, d["tgt_n"], mode, apply_mode, n)
        X = e.transform()
    if mode == sym.MODE_QUIRKS:
        # the reference's arithmetic sums about the origin, un-centred: far from it the conditioning of its solves grows as
        # (offset / extent)^2, and two exact implementations part after a few increments.  Its passes are what is checked here.
        return
    assert solved == n
    ro = oracle.align(src, d["src_n"], tgt, d["tgt_n"], mode=mode, corr=oracle.CORR_BRUTE, apply_mode=apply_mode,
                      max_iters=n, fixed_iters=True)
    assert ro["status"] == 0 and ro["iters"] == n
    # the translation of a transform far from the origin carries (I - R) o: compare it in the frame centred at the offset.  The
    # clouds themselves are only resolved to an fp32 ulp of the offset: where 8 of those exceed TOL_T of the extent, they are the bar
    # (increments that differ in their last bits round the moved points apart by that much, and the pairs follow)
    tol = max(TOL_T, 8.0 * float(np.spacing(np.float32(np.abs(off).max()))) / E)
    R, t = _centred_transform(X, off)
    Ro, to = _centred_transform(ro["transform"], off)
    assert np.abs(R - Ro).max() < tol, (np.abs(R - Ro).max(), tol)
    assert np.abs(t - to).max() / E < tol, (np.abs(t - to).max() / E, tol)


# ----------------------------------------------------------------------------------------------
# (c) shapes the grid fits badly
# ----------------------------------------------------------------------------------------------
def _shape(kind):
    rng = np.random.default_rng(sum(map(ord, kind)))
    n = 12000
    if kind == "slab":
        p = rng.random((n, 3)) * np.array([10.0, 7.0, 1e-5])
    elif kind == "needle":
        p = np.stack([rng.random(n) * 100.0, 1e-3 * rng.standard_normal(n), 1e-3 * rng.standard_normal(n)], 1)
    elif kind == "clusters":                                   # two clusters 1e4 times their own size apart
        p = rng.random((n, 3)) * 1e-3
        p[n // 2:] += np.array([10.0, 3.0, -2.0])
    elif kind == "negative":
        from symmicp import synth
        p = synth.c4_surface(n)["src"].astype(np.float64) - np.array([5.0, 7.0, 3.0])
    else:                                                      # one point repeated 5000 times + an outlier
        q = np.concatenate([np.tile([[0.3, -0.2, 0.7]], (5000, 1)), [[4.0, 1.0, -2.0]]])
        qn = np.tile(np.float32([[0, 0, 1]]), (len(q), 1))
        p = np.array([0.3, -0.2, 0.7]) + 0.05 * rng.standard_normal((2000, 3))
        p[::97] = np.array([4.0, 1.0, -2.0]) + 0.05 * rng.standard_normal((len(p[::97]), 3))
        pn = rng.standard_normal(p.shape)
        pn /= np.linalg.norm(pn, axis=1, keepdims=True)
        return p.astype(np.float32), pn.astype(np.float32), q.astype(np.float32), qn
    nr = rng.standard_normal((n, 3))
    nr /= np.linalg.norm(nr, axis=1, keepdims=True)
    from symmicp import synth
    R = synth.rotation(2.0, (0.3, -1.0, 0.5))
    ext = p.max(0) - p.min(0)
    q = (p - p.mean(0)) @ R.T + p.mean(0) + 0.01 * ext * np.array([1.0, -0.5, 0.25])
    # the target (what the grid and the tree index) is the shape itself; the source a slightly moved copy of it
    return q.astype(np.float32), (nr @ R.T).astype(np.float32), p.astype(np.float32), nr.astype(np.float32)


@pytest.mark.parametrize("kind", ["slab", "needle", "clusters", "negative", "one_point"])
@pytest.mark.parametrize("apply_mode", ["APPLY_INCREMENTAL", "APPLY_CUMULATIVE"])
def test_badly_fitting_shapes_stay_exact(sym, oracle, kind, apply_mode):
    src, sn, tgt, tn = _shape(kind)
    if kind == "negative":
        assert (src < 0).all() and (tgt < 0).all()
    apply_mode = getattr(sym, apply_mode)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, apply=apply_mode, max_iters=8, fixed_iters=1) as e:
        e.set_target(tgt, tn)
        e.set_source(src, sn)
        solved = _check_passes_against_oracle(sym, oracle, e, src, sn, tgt, tn, sym.MODE_PAPER, apply_mode, 8)
        assert solved == 8 or kind == "one_point", solved             # one repeated point: the solve may be flagged degenerate
        # guesses that move the queries by whole extents: every pass searches afresh
        for G in (np.diag([1.0, 1.0, 1.0, 1.0]), np.array([[0, -1, 0, 0.5], [1, 0, 0, -0.25], [0, 0, 1, 0.125], [0, 0, 0, 1.0]])):
            e.begin(G.astype(np.float32))
            idx, d2 = e.correspondences()
            ri, rd = oracle.nn_brute(src, tgt, X=G.astype(np.float32))
            assert np.array_equal(idx, ri) and np.array_equal(d2, rd), int((idx != ri).sum())


# ----------------------------------------------------------------------------------------------
# (d) every forced search regime
# ----------------------------------------------------------------------------------------------
_FORCED = {
    "first-pass-packet": dict(SYMMICP_FIRST_PASS="packet"),
    "first-pass-walk": dict(SYMMICP_FIRST_PASS="walk"),
    "packet-waves-1": dict(SYMMICP_PACKET_WAVES="1"),
    "packet-waves-4": dict(SYMMICP_PACKET_WAVES="4"),
    "cells-queries-128": dict(SYMMICP_CELLS_QUERIES="128"),
    "cells-queries-256": dict(SYMMICP_CELLS_QUERIES="256"),
    "optimistic-budget-walk": dict(SYMMICP_OPTIMISTIC="1", SYMMICP_BUDGET_WALK="1"),
}


@pytest.mark.parametrize("regime", list(_FORCED))
def test_frames_under_forced_regimes_in_a_subprocess(sym, regime):
    """The regime switches are read once per process: rerun (a)-(c) of this module in a child under each of them."""
    import subprocess
    env = dict(os.environ, **_FORCED[regime])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "not forced_regimes"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout
