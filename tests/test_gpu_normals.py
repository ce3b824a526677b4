"""GPU tests: the k-NN PCA normals pre-step (k_normals_knn, MyICP::estimateNormals) held exactly, for every point.

For each input the neighbour sets the kernel walks to (symmicp_ctx_knn) must equal the brute-force reference of tests/_knn_ref.py
bit for bit, rows and fp32 d2.  The normals and curvatures must equal, bit for bit, tests/_knn_ref.emulate: the kernel's own fp64
arithmetic (moments in set order, cyclic Jacobi capped at 12 sweeps, flip, curvature) replayed in numpy on the reference sets.
With 64 sweeps that emulation is the oracle's orc_normals_knn (tests/test_knn_ref.py checks it on the CPU).  Where the oracle is
cheap it is called directly, and the device must equal it on every point except where the two caps give different bits: a few
neighbourhoods with a repeated smallest eigenvalue (7 points of the cubic tie lattice at k = 10, 192 of cat with every point twice
at k = 3), where the Jacobi never meets its absolute stop and the cap decides.  Besides, independent of the emulation, against numpy eigh of the reference covariance C (see _bars):
  |n| within 4e-7 of 1; Rayleigh quotient n^T C n - lam0 <= 1e-12 tr C; angle to the eigenvector <= 4e-7 + 1e-14 tr / (lam1 - lam0);
  curvature within 2 fp32 ulps (+ 4 fp64 eps, eigh's own accuracy) of lam0 / tr where lam1 - lam0 > 1e-9 tr;
  (vp - p) . n >= 0 wherever the reference normal is not within 1e-6 of perpendicular to vp - p.
"""
import numpy as np
import pytest

import _knn_ref as R

pytestmark = pytest.mark.gpu

KS = (3, 4, 9, 10, 15, 16)
VP_UP = (0.5, 0.5, 2.0)


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine() as e:
        yield e


def _bars(xyz, nrm, curv, rows, vp, centres=None):
    p = np.asarray(xyz, np.float32)[np.arange(len(rows)) if centres is None else centres].astype(np.float64)
    _, C = R.moments(xyz, rows)
    lam, vec = R.eig(C)
    tr = np.trace(C, axis1=1, axis2=2)
    n = nrm.astype(np.float64)
    ln = np.linalg.norm(n, axis=1)
    assert np.isfinite(n).all() and np.isfinite(curv).all()
    assert np.abs(ln - 1).max() <= 4e-7, np.abs(ln - 1).max()
    u = n / ln[:, None]
    rq = np.einsum("ni,nij,nj->n", u, C, u)
    assert (rq - lam[:, 0] <= 1e-12 * tr).all(), (rq - lam[:, 0] - 1e-12 * tr).max()
    v0 = vec[:, :, 0]
    ang = np.arctan2(np.linalg.norm(np.cross(u, v0), axis=1), np.abs(np.einsum("ni,ni->n", u, v0)))
    with np.errstate(divide="ignore", invalid="ignore"):
        bar = 4e-7 + 1e-14 * tr / (lam[:, 1] - lam[:, 0])
    bar[~(lam[:, 1] > lam[:, 0])] = np.inf
    assert (ang <= bar).all(), (ang - bar).max()
    sep = lam[:, 1] - lam[:, 0] > 1e-9 * tr
    with np.errstate(all="ignore"):
        ref = np.where(tr > 0, np.maximum(lam[:, 0], 0) / tr, 0.0)
    tol = 2 * np.spacing(ref.astype(np.float32)).astype(np.float64) + 4 * np.finfo(np.float64).eps
    assert (np.abs(curv.astype(np.float64) - ref)[sep] <= tol[sep]).all()
    w = np.asarray(vp, np.float32).astype(np.float64) - p
    clear = np.abs(np.einsum("ni,ni->n", w, v0)) > 1e-6 * np.linalg.norm(w, axis=1)
    assert (np.einsum("ni,ni->n", w, n)[clear] >= 0).all()


def check(eng, xyz, k, vp=(0.0, 0.0, 0.0), oracle=None):
    """every point of one cloud: sets, bars, emulation bits, and the oracle's bits when given -> (rows, nrm, curv)"""
    xyz = np.ascontiguousarray(xyz, np.float32)
    rows, d2 = eng.knn(xyz, k)
    rr, rd = R.knn(xyz, k)
    bad = ~((rows == rr).all(1) & (d2.view(np.uint32) == rd.view(np.uint32)).all(1))
    assert not bad.any(), (k, int(bad.sum()), np.flatnonzero(bad)[:5], rows[bad][:2], rr[bad][:2])
    nrm, curv = eng.estimate_normals(xyz, k, vp)
    _bars(xyz, nrm, curv, rr, vp)
    en, ec = R.emulate(xyz, rr, vp, sweeps=12)
    bad = ~((nrm == en).all(1) & (curv == ec))
    assert not bad.any(), (k, int(bad.sum()), np.flatnonzero(bad)[:5])
    if oracle is not None:
        # the oracle runs the Jacobi for up to 64 sweeps: where that changes the bits (only neighbourhoods with a repeated smallest
        # eigenvalue, whose rotations never meet the 1e-300 stop; test_knn_ref.py lists them) the device may differ from it
        on, oc = oracle.normals_knn(xyz, k, viewpoint=vp)
        e64 = R.emulate(xyz, rr, vp, sweeps=64)
        capped = ~((en == e64[0]).all(1) & (ec == e64[1]))
        bad = ~((nrm == on).all(1) & (curv == oc)) & ~capped
        assert not bad.any(), (k, int(bad.sum()), np.flatnonzero(bad)[:5])
        if capped.any():
            lam = np.linalg.eigvalsh(R.moments(xyz, rr[capped])[1])
            assert (lam[:, 1] - lam[:, 0] <= 1e-12 * lam.sum(1)).all()
        print("normals vs oracle: n=%d k=%d differ=%d capped=%d" % (len(xyz), k, int((~((nrm == on).all(1) & (curv == oc))).sum()), int(capped.sum())))
    return rows, nrm, curv


# ---- fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_cat_both_clouds(eng, oracle, cat, k):
    for xyz in (cat["src"], cat["tgt"]):
        check(eng, xyz, k, oracle=oracle)


def test_collinear_bunny(eng, oracle, bunny):
    for k in KS:
        rows, nrm, curv = check(eng, bunny, k, oracle=oracle)
        line = R.eig(R.moments(bunny, rows)[1])[1][:, :, 2]          # each neighbourhood's own line: the cloud bends a little
        assert np.abs(np.einsum("ni,ni->n", nrm.astype(np.float64), line)).max() <= 1e-6
        assert np.abs(curv).max() <= 1e-6


# ---- synthetic clouds -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload,n", [("c3", 20000), ("c4", 40000), ("c5", 30000)])
def test_synthetic(eng, oracle, workload, n):
    from symmicp import synth
    d = dict(c3=synth.c3_uniform, c4=synth.c4_surface, c5=synth.c5_scan)[workload](n)
    for k in KS:
        check(eng, d["src"], k, VP_UP, oracle=oracle if k == 10 else None)


# ---- exact ties -------------------------------------------------------------------------------------------------------------
def _shuffled(g, seed):
    return g[np.random.default_rng(seed).permutation(len(g))]


def test_cubic_tie_lattice(eng, oracle):
    g = np.stack(np.meshgrid(*[np.arange(16)] * 3, indexing="ij"), -1).reshape(-1, 3).astype(np.float32) * np.float32(0.125)
    xyz = _shuffled(g, 1)
    for k in KS:                                      # 7 = self + the 6 face neighbours: 10 and 16 cut the 12-point edge shell
        check(eng, xyz, k, VP_UP, oracle=oracle if k in (10, 16) else None)


def test_planar_tie_lattice(eng, oracle):
    g = np.stack(np.meshgrid(np.arange(64), np.arange(64), indexing="ij"), -1).reshape(-1, 2)
    xyz = _shuffled(np.concatenate([g, np.full((len(g), 1), 3)], 1).astype(np.float32) * np.float32(0.125), 2)
    for k in (7,) + KS:                               # 5 = self + 4 edge neighbours: 7 cuts the 4-point diagonal shell
        check(eng, xyz, k, VP_UP, oracle=oracle if k == 7 else None)


# ---- duplicates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["interleaved", "blocks"])
def test_cat_every_point_twice(eng, oracle, cat, layout):
    x = cat["src"]
    xyz = np.repeat(x, 2, axis=0) if layout == "interleaved" else np.concatenate([x, x])
    for k in KS:
        check(eng, xyz, k, oracle=oracle if k in (3, 10, 16) else None)


def test_coincident_cluster_has_zero_covariance(eng, oracle):
    rng = np.random.default_rng(5)
    cloud = rng.random((3000, 3), dtype=np.float32)
    at = np.float32([0.25, 0.5, 0.75])
    xyz = np.concatenate([cloud[:1000], np.tile(at, (20, 1)), cloud[1000:]])
    for k in KS:
        rows, nrm, curv = check(eng, xyz, k, VP_UP, oracle=oracle)
        c = slice(1000, 1020)
        assert (rows[c] >= 1000).all() and (rows[c] < 1020).all()            # every neighbour is a copy: covariance exactly 0
        assert (curv[c] == 0).all() and np.isfinite(nrm[c]).all()
        assert np.array_equal(np.linalg.norm(nrm[c], axis=1), np.ones(20, np.float32))


# ---- tiny clouds and the tree's leaf / fan sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 10, 16])
def test_tiny_clouds(eng, oracle, k):
    rng = np.random.default_rng(k)
    for n in sorted({k, k + 1, 2 * k, 2 * k + 1, 2 * k + 2, 8, 9, 63, 64, 65, 512, 513, 4096, 4097}):
        if n < k:
            continue
        check(eng, rng.random((n, 3), dtype=np.float32), k, VP_UP, oracle=oracle)


# ---- frames -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("times", [1e3, 1e4])
def test_cat_far_from_the_origin(eng, oracle, cat, times):
    x = cat["src"]
    off = np.float32(times * float((x.max(0) - x.min(0)).max()))
    xyz = x + np.float32([1.0, -0.5, 0.25]) * off
    vp = tuple(float(v) for v in (xyz.mean(0) + np.float32([0, 0, 2]) * off))
    for k in (3, 10, 16):
        check(eng, xyz, k, vp, oracle=oracle)


@pytest.mark.parametrize("e2", [-14, 14])
def test_power_of_two_units(eng, cat, e2):
    s = np.float32(2.0 ** e2)
    for xyz in (cat["src"], cat["tgt"]):
        for k in (3, 10, 16):
            rows0, nrm0, curv0 = check(eng, xyz, k, VP_UP)
            rows1, nrm1, curv1 = check(eng, xyz * s, k, tuple(float(v * s) for v in VP_UP))
            assert np.array_equal(rows0, rows1)
            assert np.array_equal(nrm0.view(np.uint32), nrm1.view(np.uint32))
            assert np.array_equal(curv0.view(np.uint32), curv1.view(np.uint32))


def test_viewpoints(eng, oracle, cat):
    x = cat["tgt"]
    for vp in ((0.0, 0.0, 0.0), VP_UP, tuple(float(v) for v in x.mean(0))):
        check(eng, x, 10, vp, oracle=oracle)


# ---- the bench size ---------------------------------------------------------------------------------------------------------
def test_c4_1m_sample(eng):
    from symmicp import synth
    xyz = synth.c4_surface(1_000_000)["src"]
    rows, d2 = eng.knn(xyz, 10)
    nrm, curv = eng.estimate_normals(xyz, 10, VP_UP)
    sub = np.random.default_rng(7).choice(len(xyz), 20000, replace=False)
    rr, rd = R.knn(xyz, 10, queries=sub)
    assert np.array_equal(rows[sub], rr) and np.array_equal(d2[sub].view(np.uint32), rd.view(np.uint32))
    _bars(xyz, nrm[sub], curv[sub], rr, VP_UP, centres=sub)
    en, ec = R.emulate(xyz, rr, VP_UP, sweeps=12, centres=sub)
    assert np.array_equal(nrm[sub], en) and np.array_equal(curv[sub], ec)


# ---- the context path -------------------------------------------------------------------------------------------------------
def test_engine_matches_the_one_shot_entry(sym, eng, cat):
    for k in (3, 10, 16):
        a = sym.estimate_normals(cat["src"], k, viewpoint=VP_UP)
        b = eng.estimate_normals(cat["src"], k, VP_UP)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    # viewpoint NULL is the origin
    a = eng.estimate_normals_strided(cat["src"], 3, 1, len(cat["src"]), 10, None)
    b = eng.estimate_normals(cat["src"], 10, (0.0, 0.0, 0.0))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_strided_input_matches_packed(eng, cat):
    x = cat["tgt"]
    n = len(x)
    want = eng.estimate_normals(x, 10, VP_UP)
    pt = np.full((n, 4), np.nan, np.float32)              # pcl::PointXYZ in the shim: x y z pad
    pt[:, :3] = x
    pn = np.full((n, 12), np.nan, np.float32)             # pcl::PointNormal: x y z pad, normal, curvature ...
    pn[:, :3] = x
    cm = np.ascontiguousarray(x.T)                        # column-major: row_stride 1, col_stride n
    for buf, rs, cs in ((pt, 4, 1), (pn, 12, 1), (cm, 1, n)):
        got = eng.estimate_normals_strided(buf, rs, cs, n, 10, VP_UP)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (rs, cs)


def _run(sym, d, est=None, steps=(3, 5)):
    """c4 PAPER/TREE engine: begin, steps[0] steps, `est` (a callable on the engine), steps[1] steps -> everything observable"""
    out = []
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        its = [e.begin()]
        its += [e.step() for _ in range(steps[0])]
        if est is not None:
            est(e)
        its += [e.step() for _ in range(steps[1])]
        out = dict(sums=np.stack([i["sums"] for i in its]), diffs=np.array([i["diff"] for i in its]),
                   inc=np.stack([i["increment"] for i in its]), X=e.transform(), corr=e.correspondences(), cert=e.certificates())
    return out


def _same(a, b):
    assert np.array_equal(a["sums"], b["sums"]) and np.array_equal(a["diffs"], b["diffs"]) and np.array_equal(a["inc"], b["inc"])
    assert np.array_equal(a["X"], b["X"])
    for u, v in zip(a["corr"] + a["cert"], b["corr"] + b["cert"]):
        assert np.array_equal(u, v)


def test_estimate_mid_alignment_leaves_the_alignment_alone(sym, eng):
    from symmicp import synth
    d = synth.c4_surface(200_000)
    big = synth.c4_surface(400_000)["src"]
    small = synth.c3_uniform(100_000)["src"]
    seen = {}

    def est(e):
        seen["big"] = e.estimate_normals(big, 10, VP_UP)
        seen["small"] = e.estimate_normals(small, 16, VP_UP)
        seen["knn"] = e.knn(small, 16)

    _same(_run(sym, d, est), _run(sym, d))
    ref_big = eng.estimate_normals(big, 10, VP_UP)
    ref_small = eng.estimate_normals(small, 16, VP_UP)
    assert np.array_equal(seen["big"][0], ref_big[0]) and np.array_equal(seen["big"][1], ref_big[1])
    assert np.array_equal(seen["small"][0], ref_small[0]) and np.array_equal(seen["small"][1], ref_small[1])
    assert np.array_equal(seen["knn"][0], eng.knn(small, 16)[0])


def test_estimate_on_a_fresh_context_then_align(sym):
    from symmicp import synth
    d = synth.c4_surface(200_000)
    pre = synth.c4_surface(50_000)["src"]
    res = []
    for first in (True, False):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1) as e:
            if first:
                e.estimate_normals(pre, 10)                # no keep-arena yet: the estimate creates it
            e.set_target(d["tgt"], d["tgt_n"])
            e.set_source(d["src"], d["src_n"])
            r = e.align()
            res.append((r, e.correspondences()))
    (a, ca), (b, cb) = res
    assert a["status"] == b["status"] == 0 and a["iters"] == b["iters"]
    assert np.array_equal(a["transform"], b["transform"]) and np.array_equal(a["diffs"], b["diffs"])
    assert np.array_equal(ca[0], cb[0]) and np.array_equal(ca[1], cb[1])


def test_argument_errors_leave_outputs_alone(sym, eng, cat):
    import ctypes as C
    L = sym.lib()
    x = np.ascontiguousarray(cat["src"][:40])
    n = len(x)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                # noqa: E731
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))                # noqa: E731
    for nn, k in ((n, 2), (n, 17), (n, n + 1), (0, 3), (10, 11)):
        nrm = np.full((n, 3), 7, np.float32)
        curv = np.full(n, 7, np.float32)
        rows = np.full((n, 17), 7, np.int32)
        d2 = np.full((n, 17), 7, np.float32)
        assert L.symmicp_estimate_normals(-1, fp(x), 3, 1, nn, k, None, fp(nrm), fp(curv)) == sym.ERR_ARG
        assert L.symmicp_ctx_estimate_normals(eng._h, fp(x), 3, 1, nn, k, None, fp(nrm), fp(curv)) == sym.ERR_ARG
        assert L.symmicp_ctx_knn(eng._h, fp(x), 3, 1, nn, k, ip(rows), fp(d2)) == sym.ERR_ARG
        assert (nrm == 7).all() and (curv == 7).all() and (rows == 7).all() and (d2 == 7).all()
    nrm = np.full((n, 3), 7, np.float32)
    rows = np.full((n, 10), 7, np.int32)
    d2 = np.full((n, 10), 7, np.float32)
    assert L.symmicp_estimate_normals(-1, None, 3, 1, n, 10, None, fp(nrm), None) == sym.ERR_ARG
    assert L.symmicp_estimate_normals(-1, fp(x), 3, 1, n, 10, None, None, None) == sym.ERR_ARG
    assert L.symmicp_ctx_estimate_normals(eng._h, fp(x), 3, 1, n, 10, None, None, None) == sym.ERR_ARG
    assert L.symmicp_ctx_estimate_normals(None, fp(x), 3, 1, n, 10, None, fp(nrm), None) == sym.ERR_ARG
    assert L.symmicp_ctx_knn(eng._h, fp(x), 3, 1, n, 10, None, fp(d2)) == sym.ERR_ARG
    assert L.symmicp_ctx_knn(eng._h, fp(x), 3, 1, n, 10, ip(rows), None) == sym.ERR_ARG
    assert L.symmicp_ctx_knn(eng._h, None, 3, 1, n, 10, ip(rows), fp(d2)) == sym.ERR_ARG
    assert L.symmicp_ctx_knn(None, fp(x), 3, 1, n, 10, ip(rows), fp(d2)) == sym.ERR_ARG
    assert (nrm == 7).all() and (rows == 7).all() and (d2 == 7).all()
    # the context still works afterwards
    check(eng, x, 10)
