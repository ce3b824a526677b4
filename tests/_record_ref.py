"""The fp64 reduction record of one pass (include/symmicp.h, symmicp_sums), rebuilt in numpy from the pass's own inputs.  Shared by
the record tests of every mode: test_gpu_robust.py, test_gpu_plane.py (through _plane_ref), test_gpu_pass_matrix.py and _fuzz_nn.py.

Per-pair terms repeat the kernels' fp32 expressions (acc_pair / acc_plane in icp-symm_amd/csrc/kernels_pass.hip, and acc_gicp
through _gicp_ref.gicp_terms, built with -ffp-contract=off: every product and sum rounded on its own, in the kernels' association),
are carried to fp64 exactly and summed there.  So a record agrees with the pass up to the order of the fp64 summation: a slot is
compared at c x (sum of its terms' magnitudes) -- c = TOL_EXACT for the unweighted records, whose fp64 terms are exact products of fp32 values, and c = TOL_REC for the
weighted ones, whose w * v_r * v_s rounds once more in a different place -- and the pair count (slot 37, or 34 unweighted) exactly.

The two pair gates are applied as every kernel applies them (and the oracle, symmicp_oracle.c reduce_range): a pair is dropped when
d2 > max_d2 or when the moved source normal . target normal < min_ndot; a pair AT either bound is kept.  max_d2 is the fp32 square
of the fp32 max_corr_dist (engine_loop.cpp fill_pass_args): f32_max_d2."""
import numpy as np

NSUM = 40
TOL_EXACT = 1e-12      # unweighted records: fp64 sums of exact terms, only the order differs
TOL_REC = 1e-6         # weighted records

MODE_QUIRKS, MODE_PAPER, MODE_P2P, MODE_PLANE, MODE_GICP = 0, 1, 2, 3, 5       # symmicp_mode
f32 = np.float32


def np_weight(loss, scale, r):
    """robust_loss.h in fp32 (0 = none)"""
    r = np.asarray(r, f32)
    one = f32(1)
    with np.errstate(divide="ignore", over="ignore"):
        u = r / f32(scale)
        au = np.abs(u)
        u2 = u * u
        if loss == 1:
            return np.where(au <= one, one, one / au).astype(f32)
        if loss == 2:
            t = one - u2
            return np.where(au < one, t * t, f32(0)).astype(f32)
        if loss == 3:
            return (one / (one + u2)).astype(f32)
        if loss == 4:
            t = one + u2
            return (one / (t * t)).astype(f32)
    return np.ones_like(r)


def xf_rows(X, v, w):
    """xf_row of device_common.h on every row of v: ((m0 x + m1 y) + m2 z) + m3 w in fp32, unfused"""
    X = np.asarray(X, f32).reshape(4, 4)
    v = np.asarray(v, f32)
    out = np.empty_like(v)
    for r in range(3):
        out[:, r] = ((X[r, 0] * v[:, 0] + X[r, 1] * v[:, 1]) + X[r, 2] * v[:, 2]) + X[r, 3] * f32(w)
    return out


def moved(X, src, src_n, mode):
    """the source as a pass moves it from the original rows (cumulative apply): points with the translation, normals without it
    (PAPER, P2P, PLANE, GICP) -- except in QUIRKS, whose normals take the translation too (myicp.cpp:137, nrm_w = 1)"""
    return xf_rows(X, src, 1.0), xf_rows(X, src_n, 1.0 if mode == MODE_QUIRKS else 0.0)


def f32_max_d2(max_corr_dist):
    """the bound the kernels compare d2 with: max_corr_dist squared in fp32 (0 = no distance gate)"""
    m = f32(max_corr_dist)
    return f32(m * m) if m > 0 else f32(0)


def dist2(p, q):
    """dist2 of device_common.h: (dx dx + dy dy) + dz dz in fp32"""
    R = np.asarray(p, f32) - np.asarray(q, f32)
    return (R[:, 0] * R[:, 0] + R[:, 1] * R[:, 1]) + R[:, 2] * R[:, 2]


def ndot(pn, qn):
    pn, qn = np.asarray(pn, f32), np.asarray(qn, f32)
    return (pn[:, 0] * qn[:, 0] + pn[:, 1] * qn[:, 1]) + pn[:, 2] * qn[:, 2]


def gate(p, pn, q, qn, max_d2=0.0, min_ndot=-2.0):
    """the pairs the gates keep (bool [n])"""
    keep = np.ones(len(p), bool)
    md2 = f32(max_d2)
    if md2 > 0:
        keep &= ~(dist2(p, q) > md2)
    mn = f32(min_ndot)
    if mn > f32(-1):
        keep &= ~(ndot(pn, qn) < mn)
    return keep


def record_terms(p, pn, q, qn, pivot, loss, scale, p2p=False):
    """per-pair terms [n, 38] of the PAPER / QUIRKS (pivot 0, normals as moved) / P2P record and the residuals r, as acc_pair forms
    them"""
    pv = np.asarray(pivot, f32)
    d2 = dist2(p, q)                                                 # (the pair's distance is taken before the pivot comes off)
    dist = np.sqrt(d2)
    P = np.asarray(p, f32) - pv
    Q = np.asarray(q, f32) - pv
    D = P - Q
    n = len(P)
    T = np.zeros((n, 38))
    if p2p:
        r = dist
        w = np_weight(loss, scale, r).astype(np.float64) if loss else np.ones(n)
        P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
        for a in range(3):
            for b in range(3):
                T[:, 3 * a + b] = w * P64[:, a] * Q64[:, b]
        T[:, 27:30] = w[:, None] * P64
        T[:, 30:33] = w[:, None] * Q64
    else:
        N = np.asarray(pn, f32) + np.asarray(qn, f32)
        S = P + Q
        m0 = S[:, 1] * N[:, 2] - S[:, 2] * N[:, 1]
        m1 = S[:, 2] * N[:, 0] - S[:, 0] * N[:, 2]
        m2 = S[:, 0] * N[:, 1] - S[:, 1] * N[:, 0]
        c = (D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1]) + D[:, 2] * N[:, 2]
        r = c
        w = np_weight(loss, scale, r).astype(np.float64) if loss else np.ones(n)
        V = np.stack([m0, m1, m2, N[:, 0], N[:, 1], N[:, 2]], 1).astype(np.float64)
        k = 0
        for a in range(6):
            for b in range(a, 6):
                T[:, k] = w * V[:, a] * V[:, b]
                k += 1
        cd = c.astype(np.float64)
        T[:, 21:27] = V * (w * cd)[:, None]
        T[:, 27:30] = w[:, None] * P.astype(np.float64)
        T[:, 30:33] = w[:, None] * Q.astype(np.float64)
        T[:, 35] = w * cd * cd
    T[:, 33] = dist
    T[:, 34] = w
    T[:, 36] = d2
    T[:, 37] = 1.0 if loss else 0.0
    return T, r


def plane_terms(p, q, nq, pivot, loss=0, scale=1.0, dtype=np.float32):
    """per-pair terms [n, 38] of the PLANE record (acc_plane) and the residuals r = c.  dtype float32: the kernels' rows (fp32,
    unfused, their association); float64: the same rows in fp64 (an exact-as-possible record for the solve tests)."""
    f = dtype
    pv = np.asarray(pivot, f)
    d2 = dist2(p, q)
    P = np.asarray(p, f) - pv
    Q = np.asarray(q, f) - pv
    N = np.asarray(nq, f)
    D = P - Q
    m0 = P[:, 1] * N[:, 2] - P[:, 2] * N[:, 1]
    m1 = P[:, 2] * N[:, 0] - P[:, 0] * N[:, 2]
    m2 = P[:, 0] * N[:, 1] - P[:, 1] * N[:, 0]
    c = (D[:, 0] * N[:, 0] + D[:, 1] * N[:, 1]) + D[:, 2] * N[:, 2]
    n = len(P)
    w = np_weight(loss, scale, c).astype(np.float64) if loss else np.ones(n)
    V = np.stack([m0, m1, m2, N[:, 0], N[:, 1], N[:, 2]], 1).astype(np.float64)
    T = np.zeros((n, 38))
    k = 0
    for a in range(6):
        for b in range(a, 6):
            T[:, k] = w * V[:, a] * V[:, b]
            k += 1
    cd = c.astype(np.float64)
    T[:, 21:27] = V * (w * cd)[:, None]
    T[:, 27:30] = w[:, None] * P.astype(np.float64)
    T[:, 30:33] = w[:, None] * Q.astype(np.float64)
    T[:, 33] = np.sqrt(d2)
    T[:, 34] = w
    T[:, 35] = w * cd * cd
    T[:, 36] = d2
    T[:, 37] = 1.0 if loss else 0.0
    return T, c


def pass_terms(mode, p, pn, q, qn, pivot, loss=0, scale=1.0, eps=1e-3):
    """the terms of any mode's record: QUIRKS sums about the origin (the kernels get a zero pivot); eps: GICP's covariance eps"""
    if mode == MODE_PLANE:
        return plane_terms(p, q, qn, pivot, loss, scale)
    if mode == MODE_GICP:
        from _gicp_ref import gicp_terms          # (imported here: _gicp_ref imports this module)
        return gicp_terms(p, pn, q, qn, pivot, eps, loss, scale)
    pv = np.zeros(3, f32) if mode == MODE_QUIRKS else pivot
    return record_terms(p, pn, q, qn, pv, loss, scale, p2p=(mode == MODE_P2P))


def record(mode, p, pn, q, qn, idx=None, pivot=(0.0, 0.0, 0.0), loss=0, scale=1.0, max_d2=0.0, min_ndot=-2.0, eps=1e-3):
    """-> (record [40], sum of |terms| [40], number of pairs the gates kept) of the pass whose moved source is (p, pn), target
    (q, qn) and pairs idx (row i -> target row idx[i]; -1: no pair; None: identity pairing)"""
    p, pn = np.asarray(p, f32), np.asarray(pn, f32)
    q, qn = np.asarray(q, f32), np.asarray(qn, f32)
    if idx is None:
        idx = np.arange(len(p))
    idx = np.asarray(idx, np.int64)
    has = idx >= 0
    p, pn, j = p[has], pn[has], idx[has]
    keep = gate(p, pn, q[j], qn[j], max_d2, min_ndot)
    T, _ = pass_terms(mode, p[keep], pn[keep], q[j[keep]], qn[j[keep]], pivot, loss, scale, eps)
    S = np.zeros(NSUM)
    M = np.zeros(NSUM)
    S[:38] = T.sum(0)
    M[:38] = np.abs(T).sum(0)
    return S, M, int(keep.sum())


def assert_record(gpu, ref, mag, c, tag="", slot_c=None):
    """every slot 0..36 within c x (sum of its terms' magnitudes) -- slot_c: {slot: c} where a slot needs its own bar -- and the
    pair count exactly: slot 37 of a weighted record, slot 34 of an unweighted one (the weights' sum of a weighted one is held to c)"""
    gpu = np.asarray(gpu, np.float64)
    ref = np.asarray(ref, np.float64)
    bar = np.full(37, float(c))
    for k, v in (slot_c or {}).items():
        bar[k] = v
    err = np.abs(gpu[:37] - ref[:37])
    bad = np.nonzero(err > bar * np.asarray(mag[:37]))[0]
    assert bad.size == 0, (tag, [(int(k), gpu[k], ref[k], mag[k]) for k in bad[:6]])
    assert gpu[37] == ref[37], (tag, gpu[37], ref[37])
    if ref[37] == 0:
        assert gpu[34] == ref[34], (tag, gpu[34], ref[34])


def nn_ref(p, q):
    """exact nearest neighbours of the moved source rows p in q: (row, fp32 d2), ties to the lowest row.  The oracle's brute force
    (the dist2 expression above) for small clouds; for large ones a k-d tree proposes 16 candidates in fp64, the fp32 dist2 of each is
    evaluated as the kernels do and the smallest (d2, row) wins.  A row whose 16th candidate is not clearly farther than the winner
    (a tie or near-tie could lie beyond the candidates) goes to the brute force."""
    from oracle import oracle
    p, q = np.asarray(p, f32), np.asarray(q, f32)
    if len(p) * len(q) <= 4e10:
        return oracle.nn_brute(p, q)
    from scipy.spatial import cKDTree
    k = min(16, len(q))
    dist, cand = cKDTree(q.astype(np.float64)).query(p.astype(np.float64), k=k)
    cand = cand.reshape(len(p), k)
    dist = dist.reshape(len(p), k)
    d2c = np.stack([dist2(p, q[cand[:, c]]) for c in range(k)], 1)
    best = np.empty(len(p), np.int64)
    for c in range(k):
        if c == 0:
            best[:] = cand[:, 0]
            bd = d2c[:, 0].copy()
            continue
        better = (d2c[:, c] < bd) | ((d2c[:, c] == bd) & (cand[:, c] < best))
        best[better] = cand[better, c]
        bd[better] = d2c[better, c]
    unsure = dist[:, -1] <= np.sqrt(bd.astype(np.float64)) * (1 + 1e-4) + 1e-30
    if k == len(q):
        unsure[:] = False
    if unsure.any():
        ri, rd = oracle.nn_brute(p[unsure], q)
        best[unsure] = ri
        bd[unsure] = rd
    return best.astype(np.int32), bd.astype(f32)
