"""CPU tests of the plane-to-plane mode (SYMMICP_MODE_GICP): the closed form of the record against the explicit inverse of the
covariances, the host solve against an independent fp64 restatement, exact answers, power-of-two units, and the argument rules that
need no device (the context's epsilon setter needs one: test_gpu_gicp.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from _frames import scale_record
from _gicp_ref import (FP64_C, direct_record, fp64_excess, gicp_direct, gicp_pass_record, gicp_record, gicp_solve, gicp_terms,
                       swapped_matrices, unpack_upper)
from _plane_ref import angle_axis, rot_err
from conftest import ROOT


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _random_pairs(rng, n=500, offset=10.0, noise=0.1):
    """fp32 points; normals unit in fp64 (the closed form is the inverse for unit normals: fp32-rounded ones are off by ~1e-7,
    which the ~1 / eps weight along the normals would carry into the solve)"""
    q = (rng.normal(size=(n, 3)) * 3 + offset).astype(np.float32)
    p = (q + rng.normal(size=(n, 3)) * noise).astype(np.float32)
    nq = _unit(rng, n)
    npn = nq + rng.normal(size=(n, 3)) * 0.2
    npn = npn / np.linalg.norm(npn, axis=1, keepdims=True)
    return p, npn, q, nq


# ---- the enum and the argument rules ----------------------------------------------------------------------------------------
def test_enum_and_names(sym):
    assert sym.MODE_GICP == 5
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    assert re.search(r"SYMMICP_MODE_GICP = 5\b", hdr)
    assert not re.search(r"SYMMICP_MODE_\w+ = 4\b", hdr)                # 4 stays unassigned
    for fn in ("symmicp_set_gicp_epsilon", "symmicp_get_gicp_epsilon"):
        assert fn in sym.EXPORTS and hasattr(sym.lib(), fn)


def test_create_accepts_mode_5_and_refuses_4(sym):
    """symmicp_create validates the config before it looks for a device: 5 passes the check, 4 and -1 do not (nor in symmicp_solve)"""
    L = sym.lib()
    for mode, bad in ((sym.MODE_GICP, False), (4, True), (-1, True), (6, True)):
        cfg = sym.default_config(mode=mode)
        h = C.c_void_p()
        st = L.symmicp_create(C.byref(cfg), C.byref(h))
        if st == 0:
            L.symmicp_destroy(h)
        assert (st == sym.ERR_ARG) == bad, (mode, st)
    S, _ = gicp_record(*_random_pairs(np.random.default_rng(0)), pivot=(10.0, 10.0, 10.0))
    for mode in (4, -1, 6):
        assert sym.solve(mode, S)[0] == sym.ERR_ARG, mode
    assert sym.solve(sym.MODE_GICP, S, np.full(3, 10.0, np.float32))[0] == 0


def test_header_states_the_epsilon_rule():
    """the setter's comment names the fp32 rule it enforces, and the driver's help line the range"""
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    i = hdr.index("int symmicp_set_gicp_epsilon")
    doc = hdr[hdr.rindex("/*", 0, i):i]
    assert "1.0f - eps != 1.0f" in doc and "2^-25" in doc, doc
    drv = open(os.path.join(ROOT, "examples", "icp_align.cpp")).read()
    assert "1.0f - gicp_eps == 1.0f" in drv and "2^-25 < E <= 1" in drv


def test_epsilon_entry_points_refuse_a_null_context(sym):
    L = sym.lib()
    ep = C.c_float(0)
    assert L.symmicp_set_gicp_epsilon(None, C.c_float(0.5)) == sym.ERR_ARG
    assert L.symmicp_get_gicp_epsilon(None, C.byref(ep)) == sym.ERR_ARG


# ---- the closed form against the explicit inverse -----------------------------------------------------------------------------
def _normal_cases(rng, n=64):
    a = _unit(rng, n)
    perp = np.cross(a, _unit(rng, n))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    # nearly parallel: cs = 1 - 1e-7, i.e. an angle of sqrt(2e-7)
    th = np.sqrt(2e-7)
    near = np.cos(th) * a + np.sin(th) * perp
    return {"random": (a, _unit(rng, n)), "nearly_parallel": (a, near), "parallel": (a, a.copy()), "anti_parallel": (a, -a),
            "orthogonal": (a, perp)}


@pytest.mark.parametrize("eps", [1e-6, 1e-3, 0.5, 1.0])
@pytest.mark.parametrize("case", ["random", "nearly_parallel", "parallel", "anti_parallel", "orthogonal"])
def test_closed_form_matches_explicit_inverse(eps, case):
    """the fp64 terms summed into slots 0..26 and 35 = H, g and sum d^T M d from (C_p + C_q)^-1, to 1e-14 / eps relative (Sigma's
    condition number is about 1 / eps: its explicit inverse is only that accurate)"""
    rng = np.random.default_rng(sum(map(ord, case)))
    a, b = _normal_cases(rng)[case]
    n = len(a)
    q = rng.normal(size=(n, 3)) * 3 + 5.0
    p = q + rng.normal(size=(n, 3)) * 0.3
    pv = np.array([4.0, 5.0, 6.0])
    S, _ = gicp_record(p, a, q, b, pv, eps, dtype=np.float64)
    H, g, e = gicp_direct(p, a, q, b, pv, eps)
    bar = 1e-14 / eps
    Hr = unpack_upper(S)
    assert np.abs(Hr - H).max() <= bar * np.abs(H).max(), (case, eps, np.abs(Hr - H).max() / np.abs(H).max())
    assert np.abs(S[21:27] - g).max() <= bar * np.abs(g).max(), (case, eps)
    assert abs(S[35] - e) <= bar * abs(e), (case, eps, S[35], e)


def test_zero_normals_are_half_identity():
    """M = 1/2 I: the record is that of point-to-point rows at weight 1/2, whatever eps"""
    rng = np.random.default_rng(5)
    q = rng.normal(size=(50, 3)) * 2
    p = q + rng.normal(size=(50, 3)) * 0.1
    z = np.zeros((50, 3))
    for eps in (1e-3, 1.0):
        S, _ = gicp_record(p, z, q, z, (0.0, 0.0, 0.0), eps, dtype=np.float64)
        H = np.zeros((6, 6))
        g = np.zeros(6)
        for i in range(50):
            J = np.concatenate([-np.array([[0, -p[i, 2], p[i, 1]], [p[i, 2], 0, -p[i, 0]], [-p[i, 1], p[i, 0], 0]]), np.eye(3)], 1)
            H += 0.5 * J.T @ J
            g += 0.5 * J.T @ (p[i] - q[i])
        assert np.abs(unpack_upper(S) - H).max() <= 1e-13 * np.abs(H).max()
        assert np.abs(S[21:27] - g).max() <= 1e-13 * np.abs(g).max()
        assert abs(S[35] - 0.5 * ((p - q) ** 2).sum()) <= 1e-13 * S[35]


def test_epsilon_one_does_not_read_the_normals():
    """at eps = 1 the covariances are I: the fp32 record of the kernel's expressions does not depend on the normals, to the bit"""
    rng = np.random.default_rng(11)
    p, npn, q, nq = _random_pairs(rng)
    npn, nq = npn.astype(np.float32), nq.astype(np.float32)
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    S0, _ = gicp_record(p, npn, q, nq, pv, 1.0)
    S1, _ = gicp_record(p, np.zeros_like(npn), q, np.zeros_like(nq), pv, 1.0)
    S2, _ = gicp_record(p, -nq, q, npn * np.float32(3), pv, 1.0)
    assert np.array_equal(S0, S1) and np.array_equal(S0, S2)
    S3, _ = gicp_record(p, npn, q, nq, pv, 1e-3)
    assert not np.array_equal(S0, S3)


# ---- the fp32 record against the fp64 definition --------------------------------------------------------------------------------
# the smallest eps the engine accepts: the float above 2^-25 (at 2^-25 and below, 1.0f - eps == 1.0f)
EPS_MIN = float(np.nextafter(np.float32(2.0 ** -25), np.float32(1)))


def _bar_case(cat, case):
    """-> (p, pn, q, qn, pairs, pivot): the first pass of the cat pair at 15 degrees (identity pairs or nearest neighbours), or the
    200k surface pair at its true pose with its nearest neighbours (the data of test_gpu_gicp.py's fp64 checks)"""
    import _record_ref as R
    from symmicp import synth
    if case == "c4_truth":
        d = synth.c4_surface(200000)
        p, pn = R.moved(d["truth"], d["src"], d["src_n"], R.MODE_GICP)
    else:
        d = synth.perturbed(cat["src"], cat["src_n"])
        p, pn = d["src"], d["src_n"]
    idx = np.arange(len(p)) if case == "cat15_identity" else R.nn_ref(p, d["tgt"])[0]
    pv = d["tgt"].astype(np.float64).mean(0).astype(np.float32)
    return p, pn, d["tgt"], d["tgt_n"], idx, pv


@pytest.mark.parametrize("case", ["cat15_identity", "cat15_nn", "c4_truth"])
def test_fp32_record_meets_the_fp64_bar(cat, case):
    """the kernels' record (restated in fp32) against gicp_direct's np.linalg.inv(C_p + C_q) on the same fp32 data: within
    FP64_C x 2^-24 / eps of each slot's magnitude.  Two mutants of the closed form -- gamma_u and gamma_v swapped, the axis rows at
    weight 1 instead of 1/2 -- miss that bar by 10x at least: a mistake the kernel and its restatement shared would fail here"""
    p, pn, q, qn, idx, pv = _bar_case(cat, case)
    eps = 1e-3
    S, M, _ = gicp_pass_record(p, pn, q, qn, idx, pv, eps)
    D = direct_record(p, pn, q[idx], qn[idx], pv, eps)
    assert fp64_excess(S, M, D, eps) <= FP64_C, fp64_excess(S, M, D, eps)
    Dswap = direct_record(p, pn, q[idx], qn[idx], pv, eps, M=swapped_matrices(pn, qn[idx], eps))
    assert fp64_excess(Dswap, M, D, eps) >= 10 * FP64_C, fp64_excess(Dswap, M, D, eps)
    S1, _, _ = gicp_pass_record(p, pn, q, qn, idx, pv, 1.0)          # eps = 1: the axis rows alone
    assert fp64_excess(S + S1, M, D, eps) >= 10 * FP64_C, fp64_excess(S + S1, M, D, eps)


@pytest.mark.parametrize("eps", [1.0, 1e-3, 1e-5, EPS_MIN])
def test_edge_pairs_are_finite_in_fp32(eps):
    """the closed form at its edges (test_gpu_gicp.py's hand-placed pairs) in the kernels' fp32: every record finite, and equal
    normals keep lambda_u = 2 - fl32(1 - eps) 2 > 0 down to the smallest accepted eps"""
    from _gicp_ref import gicp_k
    k = gicp_k(eps)
    assert k < np.float32(1) and np.float32(2) - k * np.float32(2) > 0
    a = np.float32([[0, 0, 1], [0.6, 0.8, 0], [0.6, 0.8, 0], [1, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, 0], [0.6000001, 0.8, 0]])
    b = np.float32([[0, 0, 1], [0.6, 0.8, 0], [-0.6, -0.8, 0], [0, 1, 0], [0, 1, 0], [0, 0, 0], [0, 0, 0], [0.6, 0.8000001, 0]])
    p = np.float32(np.arange(24).reshape(8, 3) * 0.25)
    q = p + np.float32([0.01, -0.02, 0.03])
    T, r = gicp_terms(p, a, q, b, np.zeros(3, np.float32), eps)
    assert np.isfinite(T).all() and np.isfinite(r).all()


def test_eps_at_the_fp32_edge():
    """2^-25 is the largest eps that 1.0f - eps rounds away; 1e-8 is below it; the next float up survives"""
    f = np.float32
    assert f(1) - f(2.0 ** -25) == f(1) and f(1) - f(1e-8) == f(1)
    assert f(1) - f(EPS_MIN) == np.nextafter(f(1), f(0))


# ---- the host solve --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("weighted", [False, True])
def test_solve_matches_fp64_restatement(sym, seed, weighted):
    """symmicp.solve(MODE_GICP) on a record of random well-posed pairs = the fp64 restatement, to 1e-6 relative (fp32 outputs)"""
    rng = np.random.default_rng(seed)
    p, npn, q, nq = _random_pairs(rng, offset=10.0 * seed)
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    loss, scale = (3, 0.5) if weighted else (0, 1.0)               # Cauchy at about the median residual: the weights bite
    S, _ = gicp_record(p, npn, q, nq, pv, 1e-3, loss, scale, dtype=np.float64)
    w = None
    if weighted:
        T, _ = gicp_terms(p, npn, q, nq, pv, 1e-3, loss, scale, dtype=np.float64)
        w = T[:, 34]
        assert 0.1 * len(w) < w.sum() < 0.9 * len(w)
    st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_GICP, S, pv)
    ref = gicp_solve(p, npn, q, nq, pv, 1e-3, w)
    assert st == 0 and 0.0 < rc <= 1.0, (st, rc)
    rel = lambda x, y: float(np.abs(np.asarray(x, np.float64) - y).max() / np.abs(y).max())   # noqa: E731
    assert rel(a, ref["a"]) < 1e-6 and rel(t, ref["t"]) < 1e-6, (a, ref["a"], t, ref["t"])
    assert rel(pb, ref["pbar"]) < 1e-6 and rel(qb, ref["qbar"]) < 1e-6
    bar = 1e-6 * max(1.0, np.abs(ref["X"]).max()) + 8 * np.finfo(np.float32).eps * np.abs(ref["pbar"]).max()
    assert np.abs(X - ref["X"]).max() < bar, (X, ref["X"])
    # the same record through PLANE's solve: GICP's is PLANE's
    assert np.array_equal(sym.solve(sym.MODE_PLANE, S, pv)[6], X)


def test_pure_translation_in_one_step(sym, cat):
    """exact pairs q = p + t0 with the same normals: one solve returns the identity rotation and t0, to fp32 rounding"""
    q, nq = cat["src"], cat["src_n"]
    t0 = np.array([0.3, -0.2, 0.15], np.float32)
    p = q - t0
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    st, _, _, a, _, _, X = sym.solve(sym.MODE_GICP, gicp_record(p, nq, q, nq, pv)[0], pv)
    assert st == 0
    assert np.abs(X[:3, :3] - np.eye(3)).max() < 1e-6
    assert np.abs(X[:3, 3] - t0).max() < 8 * np.finfo(np.float32).eps * np.abs(q).max(), X[:3, 3]
    assert np.abs(a).max() < 1e-7


def test_small_rotation_error_is_second_order(sym, cat):
    """exact pairs under a rotation by theta (and a translation), normals moved with the points: one linearised solve is off by
    O(theta^2)"""
    q, nq = cat["src"], cat["src_n"]
    pv = q.astype(np.float64).mean(0).astype(np.float32)
    c0 = q.astype(np.float64).mean(0)
    ax = np.array([0.3, 0.5, 0.8]) / np.linalg.norm([0.3, 0.5, 0.8])
    tt = np.array([0.2, -0.1, 0.3])
    errs = []
    for th in (0.04, 0.02, 0.01):
        R = angle_axis(ax * th)
        p = ((q.astype(np.float64) - tt - c0) @ R + c0).astype(np.float32)        # q = R (p - c0) + c0 + tt
        pn = (nq.astype(np.float64) @ R).astype(np.float32)                     # nq = R pn
        T = np.eye(4)
        T[:3, :3] = R
        T[:3, 3] = c0 + tt - R @ c0
        st, _, _, _, _, _, X = sym.solve(sym.MODE_GICP, gicp_record(p, pn, q, nq, pv)[0], pv)
        assert st == 0
        ang, dt = rot_err(X, T)
        assert ang < 0.5 * th * th and dt < 5.0 * th * th, (th, ang, dt)
        errs.append(ang)
    assert errs[0] / errs[1] > 3.0 and errs[1] / errs[2] > 3.0, errs        # halving theta quarters the error


def test_power_of_two_units_solve_to_the_same_bits(sym, cat):
    """the cat pair's GICP record scaled slot by slot by its unit exponent: status 0, the same rotation, a, rc bit for bit, and t,
    the translation, pbar, qbar exactly 2^k times larger"""
    src, sn, tgt, tn = cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"]
    pv = tgt.astype(np.float64).mean(0).astype(np.float32)
    S, _ = gicp_record(src, sn, tgt, tn, pv)
    st0, pb0, qb0, a0, t0, rc0, X0 = sym.solve(sym.MODE_GICP, S, pv)
    assert st0 == 0
    for k in (-14, -8, 0, 8, 14):
        s = np.float32(2.0 ** k)
        st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_GICP, scale_record(S, float(s)), pv * s)
        assert st == 0, (k, st, rc)
        assert np.array_equal(X[:3, :3], X0[:3, :3]) and np.array_equal(X[:3, 3], X0[:3, 3] * s), k
        assert np.array_equal(a, a0) and np.array_equal(t, t0 * s) and rc == rc0, k
        assert np.array_equal(pb, pb0 * s) and np.array_equal(qb, qb0 * s), k


def test_scaled_clouds_give_scaled_records(cat):
    """the kernel's expressions on clouds scaled by 2^k: every slot scales by its unit exponent exactly (the normals, gu and gv do
    not change), so the solve above sees the same bits"""
    src, sn, tgt, tn = cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"]
    pv = tgt.astype(np.float64).mean(0).astype(np.float32)
    S, _ = gicp_record(src, sn, tgt, tn, pv)
    for k in (-8, 8):
        s = np.float32(2.0 ** k)
        Sk, _ = gicp_record(src * s, sn, tgt * s, tn, pv * s)
        assert np.array_equal(Sk, scale_record(S, float(s))), k


# ---- the command-line driver -------------------------------------------------------------------------------------------------
def _driver():
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    return exe


@pytest.mark.parametrize("args,usage", [
    (["--mode", "gicp"], False),
    (["--mode", "gicp", "--gicp-epsilon", "0.01"], False),
    (["--mode", "gicp", "--gicp-epsilon", "1"], False),
    (["--gicp-epsilon", "1e-6", "--mode", "gicp"], False),
    (["--mode", "gicp", "--loss", "huber", "--loss-scale", "0.5"], False),
    (["--mode", "gicp", "--gicp-epsilon", "0"], True),
    (["--mode", "gicp", "--gicp-epsilon", "-0.1"], True),
    (["--mode", "gicp", "--gicp-epsilon", "1.5"], True),
    (["--mode", "gicp", "--gicp-epsilon", "nan"], True),
    (["--mode", "gicp", "--gicp-epsilon", "inf"], True),
    (["--mode", "gicp", "--gicp-epsilon", "x"], True),
    (["--mode", "gicp", "--gicp-epsilon"], True),                    # no value
    (["--mode", "paper", "--gicp-epsilon", "0.01"], True),           # only with --mode gicp
    (["--gicp-epsilon", "0.01"], True),
    (["--mode", "gicps"], True),
    (["--mode", "gicp", "--gicp-epsilon", "2.98023259e-08"], False),   # the float above 2^-25: fl32(1 - eps) < 1
    (["--mode", "gicp", "--gicp-epsilon", "2.98023224e-08"], True),    # 2^-25: 1.0f - eps == 1.0f
    (["--mode", "gicp", "--gicp-epsilon", "1e-8"], True),
])
def test_driver_mode_gicp_usage(tmp_path, args, usage):
    """--mode gicp and --gicp-epsilon pass the driver's argument checks (the missing files then fail with ERR_IO before any device
    work); bad values are usage errors"""
    r = subprocess.run([_driver()] + args + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    if usage:
        assert r.returncode == 64, (args, r.returncode, r.stderr)
        if args[-1] != "--gicp-epsilon":
            assert "usage:" in r.stderr and "gicp" in r.stderr and "plane" in r.stderr, r.stderr
    else:
        assert r.returncode == 4, (args, r.returncode, r.stderr)
