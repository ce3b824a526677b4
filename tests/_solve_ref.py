"""Exact reference of the solve a record feeds (icp-symm_amd/csrc/solve_core.h), and the records to feed it.  Used by test_solve_ref.py
(host solve, and the gate of the device form compiled on the host) and test_gpu_solve.py (the device's own solve).

From the fp64 slots of a record the systems are built as solve_centred / solve_quirks build them, in mpmath at 50 digits:
  PAPER   s = pbar + qbar, d = pbar - qbar, K n = s x n;  A = [[MtM - MNK^T - K NM + K NtN K^T, MtN - K NtN], [.., NtN]],
          b = (Mtc - MtN d - K Ntc + K NtN d, Ntc - NtN d);  PLANE the same with s = pbar, d = 0;
          both equilibrated D A D, D = diag(2^-floor(e/2)) from the diagonal's binary exponent (pow2_equilibrator): x = -D (DAD)^-1 D b.
  QUIRKS  MtM a = -(Mtc + MtN t0), t0 = qbar - pbar in fp32 as the solve forms it; NtN t = -(Ntc + MtN^T a) with the solve's fp32 a.
The exact figures: solution x*, lambda_min / lambda_max (`rc`), the Cholesky pivot ratio (the device's old estimate) and the lower
bound 1 / (tr A ||L^-1||_F^2) the device uses now.

mat4_mul is replayed in numpy fp32 with the kernel's association (unfused products and sums), so it matches bit for bit."""
import mpmath
import numpy as np

from _record_ref import MODE_QUIRKS, MODE_PAPER, MODE_PLANE, NSUM, record

mp = mpmath.mp
mp.dps = 50
f32 = np.float32

HOST_THRESH = {MODE_PAPER: 1e-12, MODE_PLANE: 1e-12, MODE_QUIRKS: 1e-10}      # status OK iff the host's Jacobi ratio is above
DEVICE_THRESH = {MODE_PAPER: 1e-11, MODE_PLANE: 1e-11, MODE_QUIRKS: 1e-9}     # ... and the device's lower bound above these
LOOP_GATE = 1e-6                                                              # k_reduce_solve hands back a bound at or below this


def pow2_equilibrator(d):
    d = float(d)
    if not (d > 0.0 and d < float("inf")):
        return 1.0
    _, e = np.frexp(d)
    e = int(e)
    return float(np.ldexp(1.0, -((e - (e & 1)) // 2)))


def _blocks(S):
    S = [mpmath.mpf(float(v)) for v in np.asarray(S, np.float64)]
    G = mpmath.matrix(6, 6)
    k = 0
    for r in range(6):
        for c in range(r, 6):
            G[r, c] = G[c, r] = S[k]
            k += 1
    return S, G


def _figures(A):
    """(rc, pivot ratio, lower bound) of symmetric A (mpmath), exactly"""
    n = A.rows
    w = mpmath.eigsy(A, eigvals_only=True)
    aw = [abs(x) for x in w]
    rc = min(aw) / max(aw) if max(aw) > 0 else mpmath.mpf(0)
    if min(w) <= 0:
        return float(rc), 0.0, 0.0
    L = mpmath.matrix(n, n)
    for j in range(n):
        dj = A[j, j] - sum(L[j, k] ** 2 for k in range(j))
        L[j, j] = mpmath.sqrt(dj)
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - sum(L[i, k] * L[j, k] for k in range(j))) / L[j, j]
    piv = [L[i, i] ** 2 for i in range(n)]
    Li = mpmath.inverse(L)
    fro = sum(Li[i, j] ** 2 for i in range(n) for j in range(n))
    tr = sum(A[i, i] for i in range(n))
    return float(rc), float(min(piv) / max(piv)), float(1 / (tr * fro))


def centred(mode, S):
    """-> dict(A, b, D): the equilibrated system DAD y = -D b of PAPER / PLANE (mpmath), x = D y"""
    Sv, G = _blocks(S)
    cnt = Sv[34]
    pb = [Sv[27 + k] / cnt for k in range(3)]
    qb = [Sv[30 + k] / cnt for k in range(3)]
    if mode == MODE_PAPER:
        s = [pb[k] + qb[k] for k in range(3)]
        d = [pb[k] - qb[k] for k in range(3)]
    else:
        s, d = pb, [mpmath.mpf(0)] * 3
    K = mpmath.matrix([[0, -s[2], s[1]], [s[2], 0, -s[0]], [-s[1], s[0], 0]])
    MtM, NtN, MtN = G[0:3, 0:3], G[3:6, 3:6], G[0:3, 3:6]
    Mtc = mpmath.matrix(Sv[21:24])
    Ntc = mpmath.matrix(Sv[24:27])
    dv = mpmath.matrix(d)
    A = mpmath.matrix(6, 6)
    A11 = MtM - MtN * K.T - K * MtN.T + K * NtN * K.T
    A12 = MtN - K * NtN
    for r in range(3):
        for c in range(3):
            A[r, c] = A11[r, c]
            A[r, c + 3] = A[c + 3, r] = A12[r, c]
            A[r + 3, c + 3] = NtN[r, c]
    b1 = Mtc - MtN * dv - K * Ntc + K * NtN * dv
    b2 = Ntc - NtN * dv
    b = mpmath.matrix([b1[0], b1[1], b1[2], b2[0], b2[1], b2[2]])
    D = [pow2_equilibrator(A[i, i]) for i in range(6)]
    for i in range(6):
        for j in range(6):
            A[i, j] *= D[i] * D[j]
        b[i] *= D[i]
    return dict(A=A, b=b, D=D)


def reference(mode, S, a_solved=None):
    """exact figures of record S: dict(rc, piv, lb, x [6] or None (a then t), ok_exact (finite and cnt large enough))
    QUIRKS: rc, piv, lb are the minimum over its two 3 x 3 systems; the t system is solved from a_solved (the fp32 a the solve
    produced; the exact a* when None)."""
    S = np.asarray(S, np.float64)
    used = np.r_[0:30] if mode == MODE_PLANE else np.r_[0:33]      # (PLANE's increment does not read the target centroid; cnt = inf is 0 centroids)
    if not np.all(np.isfinite(S[used])):
        return dict(rc=float("nan"), piv=float("nan"), lb=float("nan"), x=None, ok_exact=False)
    cnt = S[34]
    if mode == MODE_QUIRKS:
        if not cnt > 0:
            return dict(rc=0.0, piv=0.0, lb=0.0, x=None, ok_exact=False)
        Sv, G = _blocks(S)
        pb = (S[27:30] / cnt).astype(f32)
        qb = (S[30:33] / cnt).astype(f32)
        t0 = (qb - pb).astype(f32)
        MtM, NtN, MtN = G[0:3, 0:3], G[3:6, 3:6], G[0:3, 3:6]
        f1, f2 = _figures(MtM), _figures(NtN)
        rhs = -(mpmath.matrix(Sv[21:24]) + MtN * mpmath.matrix([mpmath.mpf(float(v)) for v in t0]))
        x = None
        if f1[0] > 0 and f2[0] > 0:
            a = mpmath.lu_solve(MtM, rhs)
            av = [float(v) for v in a] if a_solved is None else [float(v) for v in np.asarray(a_solved, f32)]
            rhs2 = -(mpmath.matrix(Sv[24:27]) + MtN.T * mpmath.matrix(av))
            t = mpmath.lu_solve(NtN, rhs2)
            x = np.array([float(v) for v in a] + [float(v) for v in t])
        return dict(rc=min(f1[0], f2[0]), piv=min(f1[1], f2[1]), lb=min(f1[2], f2[2]), x=x, ok_exact=True)
    if not cnt >= 6:
        return dict(rc=0.0, piv=0.0, lb=0.0, x=None, ok_exact=False)
    sy = centred(mode, S)
    rc, piv, lb = _figures(sy["A"])
    x = None
    if rc > 0:
        y = mpmath.lu_solve(sy["A"], -sy["b"])
        x = np.array([float(y[i] * sy["D"][i]) for i in range(6)])
    return dict(rc=rc, piv=piv, lb=lb, x=x, ok_exact=True, D=np.array(sy["D"]))


def mat4_mul(A, B):
    """solve::mat4_mul in fp32: C[r][c] = ((A[r][0] B[0][c] + A[r][1] B[1][c]) + A[r][2] B[2][c]) + A[r][3] B[3][c]"""
    A = np.asarray(A, f32).reshape(4, 4)
    B = np.asarray(B, f32).reshape(4, 4)
    C = np.empty((4, 4), f32)
    with np.errstate(all="ignore"):
        for r in range(4):
            for c in range(4):
                s = A[r, 0] * B[0, c]
                s = f32(s + A[r, 1] * B[1, c])
                s = f32(s + A[r, 2] * B[2, c])
                s = f32(s + A[r, 3] * B[3, c])
                C[r, c] = s
    return C


# ---- records -----------------------------------------------------------------------------------------------------------------
def _pack_gram(G, mtc, ntc, cnt=100.0, sp=(0, 0, 0), sq=(0, 0, 0), diff=1.0):
    S = np.zeros(NSUM)
    k = 0
    for r in range(6):
        for c in range(r, 6):
            S[k] = G[r, c]
            k += 1
    S[21:24] = mtc
    S[24:27] = ntc
    S[27:30] = sp
    S[30:33] = sq
    S[33] = diff
    S[34] = cnt
    return S


def kahan_record():
    """the named regression case: L unit lower triangular with -30 below the diagonal, Gram L L^T, centroid sums 0, cnt 100,
    Mtc = 0.01 (1,2,3), Ntc = -0.02 (1,2,3).  Exact rc 1.4e-16; the Cholesky pivot ratio 2.4e-4 passed the device's old gate."""
    L = np.eye(6) + np.tril(np.full((6, 6), -30.0), -1)
    return _pack_gram(L @ L.T, 0.01 * np.array([1, 2, 3.0]), -0.02 * np.array([1, 2, 3.0]))


def _haar(rng, n):
    Q, R = np.linalg.qr(rng.standard_normal((n, n)))
    return Q * np.sign(np.diag(R))


def synthetic_records(seed=20261015):
    """centred Grams with a prescribed spectrum: rc from 1e-1 to 1e-18 on a log grid, eigenvectors Haar-random, axis-aligned
    (a permutation) or Kahan-type (the orthogonal factor of a Kahan matrix), diagonal magnitudes spread by 2^[-12, 12] so that the
    equilibration matters.  -> list of (name, record)"""
    rng = np.random.default_rng(seed)
    out = []
    for e in np.arange(-1.0, -18.5, -0.5):
        rc = 10.0 ** e
        for kind in ("haar", "axis", "kahan"):
            if kind == "haar":
                Q = _haar(rng, 6)
            elif kind == "axis":
                Q = np.eye(6)[rng.permutation(6)]
            else:
                c = 0.3
                Kh = np.diag(np.sqrt(1 - c * c) ** np.arange(6)) @ (np.eye(6) - c * np.triu(np.ones((6, 6)), 1))
                Q, _ = np.linalg.qr(Kh.T)
            lam = np.exp(np.linspace(0.0, np.log(rc), 6))[rng.permutation(6)]
            G = (Q * lam) @ Q.T
            G = 0.5 * (G + G.T)
            sc = 2.0 ** rng.integers(-12, 13, 6)
            G = G * np.outer(sc, sc)
            b = rng.standard_normal(6) * sc
            out.append(("syn_%s_%.1f" % (kind, e), _pack_gram(G, b[:3], b[3:])))
    out.append(("kahan", kahan_record()))
    return out


def real_records(cat):
    """records of real passes -> list of (name, mode, record, pivot): the cat pair (identity pairing) on its first pass and on a
    converged one (source moved by the truth), PAPER / PLANE / QUIRKS, Huber-weighted, offsets 1e3 and 1e4, units 2^-14 and 2^14;
    and small C4 / C5 pairs paired by their exact nearest neighbours"""
    from symmicp import synth
    from _record_ref import nn_ref, xf_rows
    out = []
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    T = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)
    src, sn, tgt, tn = cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"]
    moved_src, moved_n = xf_rows(T, src, 1.0), xf_rows(T, sn, 0.0)
    pairs = [("cat", src, sn, tgt, tn)]
    cases = []
    for nm, p, pn, q, qn in pairs:
        for stage, P, PN in (("first", p, pn), ("conv", moved_src, moved_n)):
            for off in (0.0, 1e3, 1e4):
                for k in (0, -14, 14):
                    u = f32(2.0 ** k)
                    o = f32(off)
                    cases.append(("%s_%s_off%g_u%d" % (nm, stage, off, k), P * u + o, PN, q * u + o, qn))
    d4 = synth.c4_surface(4096)
    d5 = synth.c5_scan(64 * 64)
    for nm, d in (("c4", d4), ("c5", d5)):
        idx, _ = nn_ref(d["src"], d["tgt"])
        cases.append((nm + "_first", d["src"], d["src_n"], d["tgt"][idx], d["tgt_n"][idx]))
    for nm, p, pn, q, qn in cases:
        pivot = q.astype(np.float64).mean(0).astype(f32)
        for mode in (MODE_PAPER, MODE_PLANE, MODE_QUIRKS):
            if mode == MODE_QUIRKS and ("_off" in nm and "_off0_" not in nm):
                continue                                      # (QUIRKS sums about the origin: offsets only ruin its conditioning)
            pv = np.zeros(3, f32) if mode == MODE_QUIRKS else pivot
            S, _, _ = record(mode, p, pn, q, qn, pivot=pv)
            out.append(("%s_m%d" % (nm, mode), mode, S, pv))
            if mode == MODE_PAPER and "_u0" in nm:
                S, _, _ = record(mode, p, pn, q, qn, pivot=pv, loss=1, scale=0.05 * float(np.abs(p - q).max() + 1e-3))
                Sw = S.copy()
                out.append(("%s_m%d_huber" % (nm, mode), mode, Sw, pv))
    return out


def edge_records(seed=7):
    """-> list of (name, record): counts 0, 5, 6; an all-zero Gram; rhs = 0; NaN / inf in one slot at a time; slots near 1e300"""
    rng = np.random.default_rng(seed)
    Q = _haar(rng, 6)
    G = (Q * np.array([1, 0.5, 0.3, 0.2, 0.1, 0.05])) @ Q.T
    base = _pack_gram(G, rng.standard_normal(3), rng.standard_normal(3))
    out = []
    for cnt in (0.0, 5.0, 6.0):
        S = base.copy(); S[34] = cnt
        out.append(("cnt%d" % cnt, S))
    S = base.copy(); S[:21] = 0.0
    out.append(("zero_gram", S))
    S = base.copy(); S[21:27] = 0.0
    out.append(("rhs0", S))
    for slot in (0, 5, 11, 20, 22, 25, 28, 31, 34):
        for v in (np.nan, np.inf):
            S = base.copy(); S[slot] = v
            out.append(("slot%d_%s" % (slot, v), S))
    S = base.copy(); S[21:27] *= 1e300
    out.append(("rhs_1e300", S))
    S = base.copy(); S[:21] *= 1e300
    out.append(("gram_1e300", S))
    S = base.copy(); S[:21] *= 1e-300
    out.append(("gram_1e-300", S))
    return out
