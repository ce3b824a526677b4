"""Plain numpy references for the radius search and the FPFH features (kernels_fpfh.hip; include/symmicp.h defines the arithmetic).

radius_sets()     the exact neighbourhoods N(i) = {j != i : d2(i, j) <= r2} of the query rows, r2 = fl32(r * r), d2 the kernels' fp32
                  (dx*dx + dy*dy) + dz*dz, as CSR lists ordered by (d2, row).  Brute force up to BRUTE_MAX points; above it a cKDTree
                  proposes every point within r * (1 + 1e-5) and the fp32 rule decides (the fp32 d2 and r2 are within a few 2^-24
                  relative of the exact squares, so no member can lie beyond the proposal radius).
pair_features()   PCL's computePairFeatures for the pairs (i[k], j[k]): in np.float32 every operation in the header's association
                  (numpy's float32 ufuncs round every operation and fuse nothing), in np.float64 the same formulas.
spfh_counts()     the integer histograms c_i[b] of the query rows and their neighbour counts.
spfh_from_counts() (100 * c) / k in fp32, the header's SPFH.
fpfh_from_spfh()  the FPFH stage in fp64 from a GIVEN spfh (the device's, in the tests): weights 1 / d2 over the neighbours with
                  d2 > 0, each 11-bin block scaled to sum 100, or 0 when its sum is not a positive finite number.
ambiguous()       which feature values of which pairs a correct fp32 implementation may bin differently from fp64.

Margins of ambiguous().  A device that follows the header differs from the fp32 restatement here only in atan2f (a few ulp) and in
nothing else (sqrtf and / are correctly rounded on both sides), so its distance from fp64 is that of the restatement plus those few
ulp: each margin is 4 x the largest error the restatement shows against fp64 on the clouds of tests/test_gpu_fpfh.py, measured by
measure_margins() below (python tests/_fpfh_ref.py 1m prints the table; the 1M surface's radii are 6.4 and 11.7 median spacings):

    cloud (radius; median neighbours)          pairs      max |x32 - x64| * (vn / f4)   max error of a1, a2   swaps that differ   bins that differ
    cat (5.53; 22)                             90 158     1.64e-5                       1.87e-7               0                   0
    cat (11.05; 102)                           360 882    2.60e-5                       2.01e-7               0                   0
    c4_surface(50 000) (0.0138; 17)            882 292    0.11e-5                       0.87e-7               2                   0
    c4_surface(1M), 4096 rows (0.003887; 27)   117 138    0.12e-5                       0.73e-7               3                   0
    c4_surface(1M), 4096 rows (0.007106; 89)   387 852    0.12e-5                       0.83e-7               3                   0
    (cat_out with the golden normals, 11.05: 6.17e-5 and 2.09e-7 -- not a cloud of the SPFH test, so it does not set the margins)

    M_EDGE = 4 x 2.60e-5 = 1.05e-4 (bin coordinate, after multiplying by the conditioning vn / f4 = |d^ x A| of v)
    M_SWAP = 4 x 2.01e-7 -> 1e-6   (| |a1| - |a2| |: below it the two precisions may pick different frames, which moves all three features)
With these margins 0.37 % / 0.23 % / 0.07 % / 0.35 % / 0.14 % of the pairs above are ambiguous in some feature (the tests require < 1 %).
tests/test_fpfh_ref.py measures the errors again and asserts that they stay below a quarter of the margins.

Every function evaluates a subset of query rows, so that 1M-point clouds can be checked on a few thousand rows.
"""
import numpy as np

BRUTE_MAX = 8192
M_EDGE = 1.05e-4
M_SWAP = 1e-6
M_VN = 1e-5          # vn / f4 below this: the validity test vn > 0 and the direction of v are marginal
TINY = 1e-12

PI32 = np.float32(3.14159274)
INV_2PI32 = np.float32(0.159154937)


def _d2_32(q, p):
    """fp32 (dx*dx + dy*dy) + dz*dz of the rows of q [m,3] against the rows of p [m,3] (or broadcastable)"""
    dx = q[..., 0] - p[..., 0]
    dy = q[..., 1] - p[..., 1]
    dz = q[..., 2] - p[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _csr(lists_rows, lists_d2):
    count = np.array([len(r) for r in lists_rows], np.int32)
    offs = np.zeros(len(count) + 1, np.int64)
    np.cumsum(count, out=offs[1:])
    rows = np.concatenate(lists_rows).astype(np.int32) if len(lists_rows) else np.zeros(0, np.int32)
    d2 = np.concatenate(lists_d2).astype(np.float32) if len(lists_d2) else np.zeros(0, np.float32)
    return count, offs, rows, d2


def radius_sets(xyz, r, queries=None, brute=None):
    """-> (count [m] int32, offsets [m + 1] int64, rows [total] int32, d2 [total] f32) of the rows `queries` (default: all); every
    list in ascending (d2, row).  brute=True forces the O(n m) path (the reference's own check)."""
    xyz = np.ascontiguousarray(xyz, np.float32)
    n = xyz.shape[0]
    qi = np.arange(n) if queries is None else np.asarray(queries)
    r2 = np.float32(r) * np.float32(r)
    if brute is None:
        brute = n <= BRUTE_MAX
    out_r, out_d = [], []
    if brute:
        m = max(1, (1 << 22) // n)
        for a in range(0, len(qi), m):
            q = qi[a:a + m]
            with np.errstate(over="ignore"):
                d2 = _d2_32(xyz[q][:, None, :], xyz[None, :, :])
            member = d2 <= r2
            member[np.arange(len(q)), q] = False
            for k in range(len(q)):
                j = np.nonzero(member[k])[0]
                o = np.lexsort((j, d2[k, j]))
                out_r.append(j[o])
                out_d.append(d2[k, j][o])
        return _csr(out_r, out_d)
    from scipy.spatial import cKDTree
    x64 = xyz.astype(np.float64)
    cand = cKDTree(x64).query_ball_point(x64[qi], float(np.float32(r)) * (1 + 1e-5) + 1e-300)
    for k, q in enumerate(qi):
        j = np.asarray(cand[k], np.int64)
        d2 = _d2_32(xyz[q][None, :], xyz[j])
        keep = (d2 <= r2) & (j != q)
        j, d2 = j[keep], d2[keep]
        o = np.lexsort((j, d2))
        out_r.append(j[o])
        out_d.append(d2[o])
    return _csr(out_r, out_d)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def pair_features(xyz, nrm, i, j, dtype=np.float32):
    """the pair features of row i[k] with its neighbour j[k] -> dict of arrays [len(i)]: f1 f2 f3 f4 vn a1 a2 (dtype), x1 x2 x3 (the
    bin coordinates before floor and clamp), swap, valid (bool), b1 b2 b3 (int, 0..10; meaningless where not valid).
    d2 is ALWAYS the kernels' fp32 distance of the fp32 points (the neighbourhoods are defined by it; f4 > 0 is decided on it),
    widened to dtype; everything after it is computed in dtype."""
    T = np.dtype(dtype).type
    x32 = np.ascontiguousarray(xyz, np.float32)
    i, j = np.asarray(i), np.asarray(j)
    with np.errstate(all="ignore"):
        d2 = _d2_32(x32[j], x32[i]).astype(T) if T is np.float32 else None
        p, q = x32[i].astype(T), x32[j].astype(T)
        n, m = np.asarray(nrm, np.float32)[i].astype(T), np.asarray(nrm, np.float32)[j].astype(T)
        d = [q[:, c] - p[:, c] for c in range(3)]
        if d2 is None:
            d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
            d2 = np.where(_d2_32(x32[j], x32[i]) > 0, d2, 0.0)      # (fp32 underflow of d2 decides f4 > 0 on both sides)
        nn = [n[:, c] for c in range(3)]
        mm = [m[:, c] for c in range(3)]
        f4 = np.sqrt(d2)
        a1 = _dot(nn, d) / f4
        a2 = _dot(mm, d) / f4
        swap = np.abs(a1) < np.abs(a2)
        A = [np.where(swap, mm[c], nn[c]) for c in range(3)]
        B = [np.where(swap, nn[c], mm[c]) for c in range(3)]
        d = [np.where(swap, -d[c], d[c]) for c in range(3)]
        f3 = np.where(swap, -a2, a1)
        v = _cross(d, A)
        vn = np.sqrt(_dot(v, v))
        v = [v[c] / vn for c in range(3)]
        w = _cross(A, v)
        f2 = _dot(v, B)
        f1 = np.arctan2(_dot(w, B), _dot(A, B))
        valid = (f4 > 0) & (vn > 0) & np.isfinite(f1) & np.isfinite(f2) & np.isfinite(f3)
        if T is np.float32:
            x1 = (T(11) * (f1 + PI32)) * INV_2PI32
        else:
            x1 = 11.0 * (f1 + np.pi) / (2.0 * np.pi)
        x2 = (T(11) * (f2 + T(1))) * T(0.5)
        x3 = (T(11) * (f3 + T(1))) * T(0.5)
        bins = [np.clip(np.floor(np.where(valid, x, 0)), 0, 10).astype(np.int64) for x in (x1, x2, x3)]
    return dict(f1=f1, f2=f2, f3=f3, f4=f4, vn=vn, a1=a1, a2=a2, x1=x1, x2=x2, x3=x3, swap=swap, valid=valid,
                b1=bins[0], b2=bins[1], b3=bins[2])


def pair_index(queries, offs, rows):
    """the (i, j, list number) of every pair of CSR lists that belong to the rows `queries`"""
    seg = np.repeat(np.arange(len(offs) - 1), np.diff(offs))
    return np.asarray(queries)[seg], rows.astype(np.int64), seg


def spfh_counts(xyz, nrm, queries, offs, rows, dtype=np.float64, feats=None):
    """-> (c [m,33] int64, k [m] int64): valid pairs per bin and neighbours per query row; `feats`: pair_features already evaluated"""
    i, j, seg = pair_index(queries, offs, rows)
    f = pair_features(xyz, nrm, i, j, dtype) if feats is None else feats
    c = np.zeros((len(offs) - 1, 33), np.int64)
    ok = f["valid"]
    for base, key in ((0, "b1"), (11, "b2"), (22, "b3")):
        np.add.at(c, (seg[ok], base + f[key][ok]), 1)
    return c, np.diff(offs).astype(np.int64)


def spfh_from_counts(c, k):
    """the header's fp32 SPFH: (100.0f * (float)c) / (float)k, zeros where k == 0"""
    kf = k.astype(np.float32)[:, None]
    with np.errstate(all="ignore"):
        s = (np.float32(100.0) * c.astype(np.float32)) / kf
    return np.where(kf > 0, s, np.float32(0)).astype(np.float32)


def fpfh_from_spfh(spfh, offs, rows, d2):
    """fp64 FPFH of the rows whose CSR lists are given, from spfh [n,33] of the WHOLE cloud (indexed by `rows`) -> [m,33] f64"""
    m = len(offs) - 1
    seg = np.repeat(np.arange(m), np.diff(offs))
    use = d2 > 0
    with np.errstate(all="ignore"):
        w = 1.0 / d2[use].astype(np.float64)
        s = np.zeros((m, 33))
        np.add.at(s, seg[use], spfh[rows[use]].astype(np.float64) * w[:, None])
        out = np.zeros((m, 33))
        for f in range(3):
            blk = s[:, 11 * f:11 * f + 11]
            t = blk.sum(1)
            ok = (t > 0) & np.isfinite(t)
            out[ok, 11 * f:11 * f + 11] = blk[ok] * (100.0 / t[ok])[:, None]
    return out


def ambiguous(f64, m_edge=M_EDGE, m_swap=M_SWAP):
    """f64: pair_features(..., np.float64).  -> bool [pairs, 3]: feature values a correct fp32 implementation may put in another bin
    (or drop / keep differently) than fp64 does:
      * its bin coordinate lies within m_edge / max(vn / f4, TINY) of an integer (dividing by |d^ x A| is the conditioning of v);
      * in all three features at once: | |a1| - |a2| | < m_swap (the swap flips the frame), or validity is marginal
        (vn / f4 < M_VN while f4 > 0, or a feature that is finite but beyond fp32's range)."""
    with np.errstate(all="ignore"):
        cond = np.maximum(f64["vn"] / f64["f4"], TINY)
        cond = np.where(np.isfinite(cond), cond, TINY)
        amb = np.zeros((len(cond), 3), bool)
        for c, key in enumerate(("x1", "x2", "x3")):
            x = f64[key]
            amb[:, c] = np.abs(x - np.rint(x)) < m_edge / cond
        whole = np.abs(np.abs(f64["a1"]) - np.abs(f64["a2"])) < m_swap
        whole |= (f64["f4"] > 0) & (f64["vn"] / f64["f4"] < M_VN)
        big = np.zeros(len(cond), bool)
        for key in ("f1", "f2", "f3", "vn"):
            big |= np.isfinite(f64[key]) & (np.abs(f64[key]) > 1e37)
        whole |= big
        amb |= whole[:, None]
    # a pair that is invalid for a reason both precisions agree on (f4 == 0, NaN normals, vn == 0 exactly) is not ambiguous
    dead = ~f64["valid"] & ~whole
    amb[dead] = False
    return amb


def median_spacing(xyz, rows):
    """median distance of the rows `rows` to their nearest other point (fp64 cKDTree)"""
    from scipy.spatial import cKDTree
    x64 = np.asarray(xyz, np.float64)
    return float(np.median(cKDTree(x64).query(x64[rows], 2)[0][:, 1]))


# radius in median spacings that gives about 30 / about 100 neighbours on a smooth surface sampled uniformly at random
# (pi r^2 rho neighbours, and the median nearest-neighbour distance of a planar Poisson process is sqrt(ln 2 / (pi rho)):
# r = spacing * sqrt(k / ln 2), 6.6 and 12.0; rounded down a little because c4_surface is not flat)
SPACINGS_30, SPACINGS_100 = 6.4, 11.7


def measure_margins(xyz, nrm, queries, offs, rows):
    """the fp32 restatement against fp64 on the given lists -> dict(pairs, edge_err, swap_err, swap_flips, bin_flips, amb_share)"""
    i, j, _ = pair_index(queries, offs, rows)
    a = pair_features(xyz, nrm, i, j, np.float32)
    b = pair_features(xyz, nrm, i, j, np.float64)
    both = a["valid"] & b["valid"] & (a["swap"] == b["swap"])
    with np.errstate(all="ignore"):
        cond = b["vn"] / b["f4"]
        e = 0.0
        for key in ("x1", "x2", "x3"):
            dx = np.abs(a[key].astype(np.float64) - b[key])
            if key == "x1":
                dx = np.minimum(dx, np.abs(dx - 11.0))          # atan2's branch cut: 0 and 11 are the same edge
            dx = dx[both] * cond[both]
            e = max(e, float(dx.max()) if len(dx) else 0.0)
        fin = np.isfinite(a["a1"]) & np.isfinite(b["a1"]) & np.isfinite(a["a2"]) & np.isfinite(b["a2"])
        se = max(float(np.abs(a["a1"].astype(np.float64) - b["a1"])[fin].max(initial=0.0)),
                 float(np.abs(a["a2"].astype(np.float64) - b["a2"])[fin].max(initial=0.0)))
    flips = sum(int(((a[k] != b[k]) & both).sum()) for k in ("b1", "b2", "b3"))
    amb = ambiguous(b)
    return dict(pairs=len(i), edge_err=e, swap_err=se, swap_flips=int((a["swap"] != b["swap"])[a["valid"] | b["valid"]].sum()),
                bin_flips=flips, valid_flips=int((a["valid"] != b["valid"]).sum()), amb_share=float(amb.any(1).mean()) if len(i) else 0.0)


if __name__ == "__main__":
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "icp-symm_amd", "py"))
    sys.path.insert(0, os.path.dirname(here))
    from oracle import oracle as O
    from symmicp import synth
    g = np.load(os.path.join(here, "golden", "cat_golden.npz"))
    cat, _ = O.pcd_read(os.path.join(here, "golden", "cat.pcd"))
    cat_out, _ = O.pcd_read(os.path.join(here, "golden", "cat_out.pcd"))
    c4 = synth.c4_surface(50_000)
    cases = [("cat 5.53", cat, g["src_n"], 5.53, None), ("cat 11.05", cat, g["src_n"], 11.05, None),
             ("cat_out 11.05", cat_out, g["tgt_n"], 11.05, None), ("c4 50k 0.0138", c4["src"], c4["src_n"], 0.0138, None)]
    if "1m" in sys.argv[1:]:
        c1 = synth.c4_surface(1_000_000)
        rows = np.sort(np.random.default_rng(5).choice(1_000_000, 4096, replace=False))
        sp = median_spacing(c1["src"], rows)
        cases += [("c4 1M ~30", c1["src"], c1["src_n"], SPACINGS_30 * sp, rows), ("c4 1M ~100", c1["src"], c1["src_n"], SPACINGS_100 * sp, rows)]
    for name, x, nr, r, rows in cases:
        q = np.arange(len(x)) if rows is None else rows
        cnt, offs, rr, dd = radius_sets(x, r, q)
        print(name, "median neighbours %d" % np.median(cnt), measure_margins(x, nr, q, offs, rr), flush=True)
