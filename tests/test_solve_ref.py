"""The solve of one record (icp-symm_amd/csrc/solve_core.h) against an exact reference (_solve_ref.py, mpmath at 50 digits), on real
records, synthetic Grams with a prescribed spectrum down to 1e-18, and edge records.  CPU only:

  * the host solve (symmicp.solve, exact_rc = true): its status follows the exact eigenvalue ratio across the threshold, its rcond is
    that ratio, its solution is within the forward-error bound of the exact one;
  * the device's form of the same code (exact_rc = false, the conditioning estimate of the device-driven loop) compiled on the host
    with g++ -ffp-contract=off: it accepts nothing the host rejects, its estimate is a lower bound of the exact ratio, and it solves
    to the host's bits.  The Kahan-type record is the named regression case: the old estimate (the Cholesky pivot ratio, an UPPER
    bound) passed it at 2.4e-4 where the exact ratio is 1.4e-16."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _solve_ref as R
from _record_ref import MODE_QUIRKS, MODE_PAPER, MODE_PLANE
from conftest import ROOT

MODES = (MODE_PAPER, MODE_PLANE, MODE_QUIRKS)
U = 2.0 ** -53
BAND = 4.0          # status is only asserted for exact ratios outside [thr / BAND, thr * BAND]
C_FWD = 8.0         # forward error: |y - y*| <= C_FWD n u / rc |y*| + 2^-24 |y*| (+ forming error, real records) in the equilibrated unknowns


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def records(cat):
    """(name, mode, record, pivot, exact reference) for every generated record"""
    out = []
    z = np.zeros(3, np.float32)
    for nm, S in R.synthetic_records():
        for m in MODES:
            out.append((nm, m, S, z))
    for nm, m, S, pv in R.real_records(cat):
        out.append((nm, m, S, pv))
    for nm, S in R.edge_records():
        for m in MODES:
            out.append((nm, m, S, z))
    return out


@pytest.fixture(scope="module")
def host(sym, records):
    return [sym.solve(m, S, pv) for _, m, S, pv, in records]


@pytest.fixture(scope="module")
def exact(records, host):
    return [R.reference(m, S, a_solved=h[3] if m == MODE_QUIRKS else None) for (_, m, S, _), h in zip(records, host)]


def test_host_status_follows_the_exact_ratio(records, host, exact):
    checked = 0
    for (nm, m, S, _), h, ex in zip(records, host, exact):
        st = h[0]
        if not ex["ok_exact"]:
            assert st == 3, (nm, m, st)                                # non-finite record, or too few pairs: degenerate
            continue
        if m == MODE_QUIRKS and ex["x"] is not None and np.all(np.abs(ex["x"][:3]) < 2.0 ** -150):
            assert st == 3, (nm, st)                                   # a = 0 in fp32: the axis is 0/0 (func.cpp:96), as the reference
            continue
        if ex["x"] is not None and not np.all(np.abs(ex["x"]) <= np.finfo(np.float32).max):
            assert st == 3, (nm, m, st)                                # (float) x overflows: the increment is not finite
            continue
        thr = R.HOST_THRESH[m]
        if ex["rc"] > thr * BAND:
            assert st == 0, (nm, m, ex["rc"], h[5])
            checked += 1
        elif ex["rc"] < thr / BAND:
            assert st == 3, (nm, m, ex["rc"], h[5])
            checked += 1
    assert checked > 300


def test_host_rcond_is_the_exact_ratio(records, host, exact):
    """the Jacobi sweep's ratio within 1e-6 relative where the exact ratio exceeds 1e-10 (its eigenvalues are off by O(u) lambda_max:
    O(u / rc) relative on lambda_min, 1e-6 at rc = 1e-10), plus the fp32 rounding of rcond"""
    n = 0
    for (nm, m, S, _), h, ex in zip(records, host, exact):
        if not ex["ok_exact"] or not ex["rc"] > 1e-10 or h[0] != 0:
            continue
        rel = abs(h[5] - ex["rc"]) / ex["rc"]
        assert rel <= 1e-6 + 2.0 ** -24, (nm, m, h[5], ex["rc"], rel)
        n += 1
    assert n > 100


def test_host_solution_is_within_the_forward_error_bound(records, host, exact):
    """every accepted record: |y - y*| <= (C_FWD n u / rc + 2^-24) |y*| in the equilibrated unknowns y = x / D (the bound of a backward-
    stable Cholesky solve, the fp32 rounding of a and t on top); real records add the rounding of forming the system in fp64 from
    un-centred sums, C_FWD n u cond * |A| / |A| -- bounded here through the record's largest slot over the centred diagonal"""
    n = 0
    for (nm, m, S, _), h, ex in zip(records, host, exact):
        if h[0] != 0 or ex["x"] is None:
            continue
        x = np.concatenate([h[3], h[4]]).astype(np.float64)
        xs = ex["x"]
        D = ex.get("D", np.ones(6))
        y, ys = x / D, xs / D
        dim = 6 if m != MODE_QUIRKS else 3
        form = 0.0
        if m != MODE_QUIRKS and nm.startswith(("cat", "c4", "c5")):
            form = float(np.abs(S[:35]).max()) * float(np.max(D) ** 2)       # |terms| of the fp64 centring over the equilibrated scale
        bound = (C_FWD * dim * U * (1.0 + form) / ex["rc"] + 2.0 ** -24) * np.linalg.norm(ys) + 2.0 ** -147 / np.min(D)     # (fp32 underflow)
        assert np.linalg.norm(y - ys) <= bound, (nm, m, y, ys, ex["rc"])
        n += 1
    assert n > 100


# ---- the device form (exact_rc = false) on the host ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gate_driver(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the gate driver")
    d = tmp_path_factory.mktemp("gate")
    exe = str(d / "solve_gate")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "icp-symm_amd", "csrc"), os.path.join(ROOT, "tests", "cpp", "solve_gate.cpp"), "-o", exe])
    return exe


def run_gate(exe, items):
    """items: (mode, record, pivot) -> [(host, device)] with each = (status, rcond, pbar qbar a t as uint32 bits [12])"""
    lines = [str(len(items))]
    for m, S, pv in items:
        lines.append(" ".join([str(m)] + [float(v).hex() for v in np.asarray(pv, np.float32)] + [float(v).hex() for v in np.asarray(S, np.float64)]))
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    res = []
    for i in range(len(items)):
        pair = []
        for ln in out[2 * i:2 * i + 2]:
            f = ln.split()
            rc = np.array([int(f[1], 16)], np.uint32).view(np.float32)[0]
            pair.append((int(f[0]), float(rc), np.array([int(v, 16) for v in f[2:]], np.uint32)))
        res.append(pair)
    return res


def test_device_gate_implies_host_ok(gate_driver, records, exact):
    res = run_gate(gate_driver, [(m, S, pv) for _, m, S, pv in records])
    accepted = 0
    for (nm, m, S, _), ex, ((hs, hrc, hb), (ds, drc, db)) in zip(records, exact, res):
        if ds == 0:
            assert hs == 0, (nm, m, "device accepts what the host flags", drc, hrc, ex["rc"])
            accepted += 1
        if ex["ok_exact"] and np.isfinite(ex["rc"]):
            assert drc <= ex["rc"] * (1 + 1e-9), (nm, m, "not a lower bound", drc, ex["rc"])
            if drc > R.LOOP_GATE:
                assert ex["rc"] > R.LOOP_GATE, (nm, m)
        # the same factorisation and substitutions whichever estimate: a, t, pbar, qbar to the bit
        assert np.array_equal(hb, db), (nm, m)
    assert accepted > 200


def test_kahan_record_is_refused_by_both_forms(gate_driver):
    """the named regression case: exact ratio 1.4e-16; the Cholesky pivot ratio 2.4e-4 (the old device estimate) would have passed
    the loop's 1e-6 gate and applied a turn of ~90 degrees"""
    S = R.kahan_record()
    ex = R.reference(MODE_PAPER, S)
    assert ex["rc"] < 1e-15 and ex["piv"] > 1e-4 and ex["lb"] <= ex["rc"]
    for m in (MODE_PAPER, MODE_PLANE):
        (hs, hrc, _), (ds, drc, _) = run_gate(gate_driver, [(m, S, np.zeros(3, np.float32))])[0]
        assert hs == 3 and ds == 3, (m, hs, ds, hrc, drc)
        assert drc <= R.LOOP_GATE


def test_lower_bound_is_within_n2_of_the_exact_ratio(records, exact):
    """the bound's other side (exact arithmetic): lambda_min / lambda_max / n^2 <= 1 / (tr A ||L^-1||_F^2) <= lambda_min / lambda_max"""
    for (nm, m, S, _), ex in zip(records, exact):
        if not ex["ok_exact"] or not ex["lb"] > 0:
            continue
        n = 3 if m == MODE_QUIRKS else 6
        assert ex["rc"] / n ** 2 * (1 - 1e-12) <= ex["lb"] <= ex["rc"] * (1 + 1e-12), (nm, m, ex)


def test_mat4_mul_replay_is_associative_as_written():
    """the replay's order matters: a product whose terms cancel only in one association (catches a swapped operand order)"""
    A = np.eye(4, dtype=np.float32)
    A[0, :] = [1.0, 1e8, -1e8, 1.0]
    B = np.eye(4, dtype=np.float32)
    B[:, 0] = [1.0, 1.0, 1.0, 1.0]
    C = R.mat4_mul(A, B)
    assert C[0, 0] == np.float32(np.float32(np.float32(1.0 + 1e8) - 1e8) + 1.0)
