"""CPU tests of the point-to-plane mode (SYMMICP_MODE_PLANE): the host solve against an independent fp64 restatement, exact answers,
power-of-two units, degenerate scenes, and the argument rules that need no device."""
import os
import subprocess

import numpy as np
import pytest

from _frames import scale_record
from _plane_ref import angle_axis, plane_record, plane_solve, rot_err
from conftest import ROOT


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def _random_pairs(rng, n=500, offset=10.0, noise=0.1):
    q = (rng.normal(size=(n, 3)) * 3 + offset).astype(np.float32)
    nq = rng.normal(size=(n, 3))
    nq = (nq / np.linalg.norm(nq, axis=1, keepdims=True)).astype(np.float32)
    p = (q + rng.normal(size=(n, 3)) * noise).astype(np.float32)
    return p, q, nq


def test_enum_and_names(sym):
    import re
    assert sym.MODE_PLANE == 3
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    assert re.search(r"SYMMICP_MODE_PLANE = 3\b", hdr)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("weighted", [False, True])
def test_solve_matches_fp64_restatement(sym, seed, weighted):
    """symmicp.solve(MODE_PLANE) on a record of random well-posed pairs = the fp64 restatement, to 1e-6 relative (fp32 outputs)"""
    rng = np.random.default_rng(seed)
    p, q, nq = _random_pairs(rng, offset=10.0 * seed)
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    loss, scale = (3, 0.05) if weighted else (0, 1.0)              # Cauchy at half the noise: the weights bite
    S, _ = plane_record(p, q, nq, pv, loss, scale, dtype=np.float64)
    w = None
    if weighted:
        from _plane_ref import plane_terms
        T, c = plane_terms(p, q, nq, pv, loss, scale, dtype=np.float64)
        w = T[:, 34]
        assert 0.1 * len(w) < w.sum() < 0.9 * len(w)
    st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_PLANE, S, pv)
    ref = plane_solve(p, q, nq, pv, w)
    assert st == 0 and 0.0 < rc <= 1.0, (st, rc)
    rel = lambda x, y: float(np.abs(np.asarray(x, np.float64) - y).max() / np.abs(y).max())   # noqa: E731
    assert rel(a, ref["a"]) < 1e-6 and rel(t, ref["t"]) < 1e-6, (a, ref["a"], t, ref["t"])
    assert rel(pb, ref["pbar"]) < 1e-6 and rel(qb, ref["qbar"]) < 1e-6
    # (the 4x4 is composed in fp32 about pbar: its translation carries the rounding of T(pbar + t) R T(-pbar), a few ulps of |pbar|)
    bar = 1e-6 * max(1.0, np.abs(ref["X"]).max()) + 8 * np.finfo(np.float32).eps * np.abs(ref["pbar"]).max()
    assert np.abs(X - ref["X"]).max() < bar, (X, ref["X"])


def test_pure_translation_in_one_step(sym, cat):
    """exact pairs q = p + t0: one solve returns the identity rotation and t0, to fp32 rounding"""
    q, nq = cat["src"], cat["src_n"]
    t0 = np.array([0.3, -0.2, 0.15], np.float32)
    p = q - t0
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    st, _, _, a, _, _, X = sym.solve(sym.MODE_PLANE, plane_record(p, q, nq, pv)[0], pv)
    assert st == 0
    assert np.abs(X[:3, :3] - np.eye(3)).max() < 1e-6
    assert np.abs(X[:3, 3] - t0).max() < 8 * np.finfo(np.float32).eps * np.abs(q).max(), X[:3, 3]
    assert np.abs(a).max() < 1e-7


def test_small_rotation_error_is_second_order(sym, cat):
    """exact pairs under a rotation by theta (and a translation): one linearised solve is off by O(theta^2)"""
    q, nq = cat["src"], cat["src_n"]
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    c0 = q.astype(np.float64).mean(0)
    ax = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    tt = np.array([0.2, -0.1, 0.3])
    errs = []
    for th in (0.04, 0.02, 0.01):
        R = angle_axis(ax * th)
        p = ((q.astype(np.float64) - tt - c0) @ R + c0).astype(np.float32)        # q = R (p - c0) + c0 + tt
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = c0 + tt - R @ c0
        st, _, _, _, _, _, X = sym.solve(sym.MODE_PLANE, plane_record(p, q, nq, pv)[0], pv)
        assert st == 0
        ang, dt = rot_err(X, T)
        assert ang < 0.5 * th * th and dt < 5.0 * th * th, (th, ang, dt)     # (cat's extent is ~200: the lever arm of dt)
        errs.append(ang)
    assert errs[0] / errs[1] > 3.0 and errs[1] / errs[2] > 3.0, errs        # halving theta quarters the error


def test_power_of_two_units_solve_to_the_same_bits(sym, oracle, cat):
    """the cat pair's PLANE record scaled slot by slot by its unit exponent: status 0, the same rotation, a, rc bit for bit, and t,
    the translation, pbar, qbar exactly 2^k times larger"""
    src, tgt, tn = cat["src"], cat["tgt"], cat["tgt_n"]
    pv = tgt.astype(np.float64).mean(0).astype(np.float32)
    S, _ = plane_record(src, tgt, tn, pv)
    st0, pb0, qb0, a0, t0, rc0, X0 = sym.solve(sym.MODE_PLANE, S, pv)
    assert st0 == 0
    for k in (-14, -8, 0, 8, 14):
        s = np.float32(2.0 ** k)
        st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_PLANE, scale_record(S, float(s)), pv * s)
        assert st == 0, (k, st, rc)
        assert np.array_equal(X[:3, :3], X0[:3, :3]) and np.array_equal(X[:3, 3], X0[:3, 3] * s), k
        assert np.array_equal(a, a0) and np.array_equal(t, t0 * s) and rc == rc0, k
        assert np.array_equal(pb, pb0 * s) and np.array_equal(qb, qb0 * s), k


def test_degenerate_scenes(sym, bunny):
    """a single plane (rank 3) and the collinear bunny with one normal direction: DEGENERATE in every unit, no NaN status"""
    rng = np.random.default_rng(3)
    pl = np.zeros((400, 3), np.float32)
    pl[:, :2] = rng.uniform(-5, 5, (400, 2))
    n = np.tile(np.array([[0, 0, 1]], np.float32), (400, 1))
    scenes = [(pl + np.float32(0.01), pl, n)]
    nb = np.tile(np.array([[0, 0, 1]], np.float32), (len(bunny), 1))
    scenes.append((bunny, bunny + np.array([0.01, 0.02, 0.0], np.float32), nb))
    for p, q, nq in scenes:
        pv = q.astype(np.float64).mean(0).astype(np.float32)
        S, _ = plane_record(p, q, nq, pv)
        for k in (-14, -8, 0, 8, 14):
            s = np.float32(2.0 ** k)
            st, _, _, _, _, rc, _ = sym.solve(sym.MODE_PLANE, scale_record(S, float(s)), pv * s)
            assert st == sym.ERR_DEGENERATE and np.isfinite(rc), (k, st, rc)
    # fewer than 6 pairs
    p, q, nq = _random_pairs(np.random.default_rng(0), n=5)
    assert sym.solve(sym.MODE_PLANE, plane_record(p, q, nq, q.mean(0))[0], q.mean(0))[0] == sym.ERR_DEGENERATE


def test_config_range_checked_before_the_device(sym):
    """symmicp_create validates the config before it looks for a device: mode 3 passes the check, mode 4 does not"""
    import ctypes as C
    L = sym.lib()
    for mode, bad in ((sym.MODE_PLANE, False), (4, True), (-1, True)):
        cfg = sym.default_config(mode=mode)
        h = C.c_void_p()
        st = L.symmicp_create(C.byref(cfg), C.byref(h))
        if st == 0:
            L.symmicp_destroy(h)
        assert (st == sym.ERR_ARG) == bad, (mode, st)
    assert sym.solve(4, np.zeros(40))[0] == sym.ERR_ARG


def test_robust_loss_in_plane_mode(sym):
    m = sym.MyICP(mode=sym.MODE_PLANE, verbose=False)
    m.setRobustLoss("huber", 0.5)
    assert m._loss == (sym.LOSS_HUBER, 0.5)
    # the weighted record solves like any other (slot 34 = sum w, slot 37 = pairs)
    p, q, nq = _random_pairs(np.random.default_rng(9))
    pv = q.mean(0).astype(np.float32)
    S, _ = plane_record(p, q, nq, pv, loss=1, scale=0.05)
    assert S[37] == len(p) and S[34] < len(p)
    assert sym.solve(sym.MODE_PLANE, S, pv)[0] == 0


def _driver():
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    return exe


@pytest.mark.parametrize("args,usage", [
    (["--mode", "plane"], False),
    (["--mode", "plane", "--loss", "huber", "--loss-scale", "0.5"], False),
    (["--mode", "plane", "--loss", "huber"], True),                  # no scale
    (["--mode", "planes"], True),
    (["--mode", "p2p"], True),                                      # (not offered by the driver)
])
def test_driver_mode_plane_usage(tmp_path, args, usage):
    """--mode plane passes the driver's argument checks (the missing files then fail with ERR_IO before any device work)"""
    r = subprocess.run([_driver()] + args + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    if usage:
        assert r.returncode == 64 and "usage:" in r.stderr and "plane" in r.stderr, (r.returncode, r.stderr)
    else:
        assert r.returncode == 4, (r.returncode, r.stderr)
