"""GPU voxel-grid downsampling (symmicp_ctx_voxel_downsample, kernels_voxel.hip) against tests/_voxel_ref.py, bit for bit in
xyz, nrm, count and voxel_of; the argument errors; strided inputs; a context left exactly as it was."""
import ctypes as C
import os

import numpy as np
import pytest

import _voxel_ref as V
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

F = np.float32


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
def c4():
    from symmicp import synth
    return synth.c4_surface(1_000_000)


def bits_equal(dev, ref):
    assert len(dev["xyz"]) == len(ref["xyz"])
    assert np.array_equal(dev["xyz"].view(np.uint32), ref["xyz"].view(np.uint32))
    assert np.array_equal(dev["count"], ref["count"])
    assert np.array_equal(dev["voxel_of"], ref["voxel_of"])
    assert (dev["nrm"] is None) == (ref["nrm"] is None)
    if ref["nrm"] is not None:
        assert np.array_equal(dev["nrm"].view(np.uint32), ref["nrm"].view(np.uint32))


def check(eng, xyz, leaf, nrm=None, min_points=1):
    dev = eng.voxel_downsample(xyz, leaf, nrm, min_points)
    ref = V.voxel_downsample(xyz, leaf, nrm, min_points)
    bits_equal(dev, ref)
    return dev


@pytest.mark.parametrize("leaf", [1.0, 3.0, 8.0, 40.0])
def test_cat_pair_with_normals(eng, cat, sym, leaf):
    check(eng, cat["src"], leaf, cat["src_n"])
    tgt, tn = sym.pcd_read(os.path.join(GOLDEN, "cat_out.pcd"))
    assert tn is not None and not tn.any()                  # cat_out.pcd's normal fields are all zero
    r = check(eng, tgt, leaf, tn)
    assert not r["nrm"].any()                               # ... and stay zero
    check(eng, cat["tgt"], leaf, cat["tgt_n"], min_points=3)


@pytest.mark.parametrize("leaf,min_points", [(0.002, 1), (0.005, 3), (0.01, 10)])
def test_bunny(eng, bunny, leaf, min_points):
    check(eng, bunny, leaf, None, min_points)
    n = np.tile(np.array([[0.6, 0.0, 0.8]], F), (len(bunny), 1))
    n[::3] = [0.0, 1.0, 0.0]
    check(eng, bunny, leaf, n, min_points)


@pytest.mark.parametrize("leaf,ppv", [(0.0019, 2), (0.0043, 8), (0.0116, 50)])
def test_c4_surface_1m(eng, c4, leaf, ppv):
    r = check(eng, c4["src"], leaf, c4["src_n"])
    mean = len(c4["src"]) / len(r["xyz"])
    assert 0.5 * ppv < mean < 2.0 * ppv, mean
    check(eng, c4["tgt"], leaf, c4["tgt_n"], min_points=3)


def test_c4_min_points(eng, c4):
    for mp in (1, 3, 10):
        r = check(eng, c4["src"][:200_000], 0.005, c4["src_n"][:200_000], mp)
        assert (r["voxel_of"] < 0).any() == (mp > 1)


def test_uniform_cube(eng, sym):
    from symmicp import synth
    xyz = synth.c3_uniform(100_000)["src"]
    for leaf, mp in ((0.05, 1), (0.1, 3), (0.013, 1)):
        check(eng, xyz, leaf, None, mp)


def test_lattice_on_voxel_faces(eng):
    leaf = 0.125
    g = np.arange(-20, 21, dtype=F) * F(leaf)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    xyz = np.concatenate([xyz, xyz + F(leaf / 2)])
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=xyz.shape).astype(F)
    r = check(eng, xyz, leaf, nrm)
    assert len(r["xyz"]) == 41 ** 3 and r["count"].max() == 2
    check(eng, xyz, 0.25, nrm, 5)


def test_large_offset(eng):
    rng = np.random.default_rng(12)
    xyz = (rng.uniform(0, 0.05, (50_000, 3)) + 1e4).astype(F)
    for leaf in (0.003, 0.0073, 0.01):
        check(eng, xyz, leaf)


def test_single_point(eng):
    xyz = np.array([[1.5, -2.25, 3.0]], F)
    r = check(eng, xyz, 0.1, np.array([[0.0, 0.0, 2.0]], F))
    assert np.array_equal(r["xyz"], xyz) and np.array_equal(r["nrm"], [[0, 0, 1]]) and r["count"][0] == 1
    st, res, m = eng.voxel_downsample_raw(xyz, 0.1, min_points=2)
    assert st == 0 and m == 0 and len(res["xyz"]) == 0 and res["voxel_of"][0] == -1


def test_one_heavy_voxel(eng):
    # the serial worst case: 200k points in one voxel, summed by one thread
    rng = np.random.default_rng(13)
    xyz = rng.uniform(0, 1, (200_000, 3)).astype(F)
    nrm = rng.normal(size=xyz.shape).astype(F)
    r = check(eng, xyz, 2.0, nrm)
    assert len(r["xyz"]) == 1 and r["count"][0] == 200_000


def test_strided_inputs_match_packed(eng, cat):
    xyz, nrm = cat["src"], cat["src_n"]
    n = len(xyz)
    packed = eng.voxel_downsample(xyz, 3.0, nrm, 2)
    # pcl::PointXYZ-like records of 4 floats (xyz) and PointNormal-like records of 12 (normals at offset 4)
    x4 = np.zeros((n, 4), F); x4[:, :3] = xyz
    n12 = np.zeros((n, 12), F); n12[:, 4:7] = nrm
    st, r4, _ = eng.voxel_downsample_raw(x4, 3.0, n12.reshape(-1)[4:], 2, strides=(n, 4, 1, 12, 1))
    assert st == 0
    bits_equal(r4, packed)
    # column-major N x 3 (Eigen)
    st, rc, _ = eng.voxel_downsample_raw(np.asfortranarray(xyz).T.copy(), 3.0, np.asfortranarray(nrm).T.copy(), 2, strides=(n, 1, n, 1, n))
    assert st == 0
    bits_equal(rc, packed)
    # a generic stride (the host transpose path): rows of 6 floats, columns 2 apart
    x6 = np.zeros((n, 6), F); x6[:, 0::2] = xyz
    st, r5, _ = eng.voxel_downsample_raw(x6, 3.0, nrm, 2, strides=(n, 6, 2, 3, 1))
    assert st == 0
    bits_equal(r5, packed)


def test_free_function_matches_ctx(sym, eng, cat):
    a = sym.voxel_downsample(cat["src"], 5.0, cat["src_n"], 2)
    bits_equal(a, eng.voxel_downsample(cat["src"], 5.0, cat["src_n"], 2))


def test_size_error_reports_the_count(eng, cat):
    ref = V.voxel_downsample(cat["src"], 4.0)
    m = len(ref["xyz"])
    st, res, n_out = eng.voxel_downsample_raw(cat["src"], 4.0, cap=m - 1)
    assert st == 2 and res is None and n_out == m          # SYMMICP_ERR_SIZE
    st, res, n_out = eng.voxel_downsample_raw(cat["src"], 4.0, cap=m)
    assert st == 0 and n_out == m
    bits_equal(dict(res, nrm=None), ref)


def test_argument_errors(sym, eng):
    L = sym.lib()
    xyz = np.random.default_rng(14).uniform(0, 1, (100, 3)).astype(F)
    nrm = np.ones((100, 3), F)
    out = np.zeros((100, 3), F)
    nout = np.zeros((100, 3), F)
    m = C.c_size_t(0)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))

    def call(x=xyz, n_pts=100, leaf=0.1, mp=1, xo=out, nr=None, no=None, nout_p=True, h=eng._h):
        return L.symmicp_ctx_voxel_downsample(h, None if x is None else fp(x), 3, 1, None if nr is None else fp(nr), 3, 1, n_pts, leaf, mp,
                                              None if xo is None else fp(xo), None if no is None else fp(no), None, None, 100,
                                              C.byref(m) if nout_p else None)

    assert call() == 0
    assert call(x=None) == 1
    assert call(xo=None) == 1
    assert call(nout_p=False) == 1
    assert call(n_pts=0) == 1
    assert call(n_pts=2 ** 31) == 1
    for leaf in (0.0, -0.5, float("inf"), float("nan")):
        assert call(leaf=leaf) == 1
    assert call(mp=0) == 1 and call(mp=-3) == 1
    assert call(no=nout) == 1                               # nrm_out without nrm
    assert call(nr=nrm, no=nout) == 0
    assert call(h=None) == 1
    for bad in (np.nan, np.inf, -np.inf):
        x = xyz.copy(); x[17, 2] = bad
        assert call(x=x) == 1
    assert call(leaf=1e-12) == 1                            # floorf(max * inv) beyond int32
    big = np.zeros((100, 3), F); big[1] = 1.0
    assert call(x=big, leaf=1.0 / 2000) == 1                # 2001^3 voxels > 2^32
    assert call(x=big, leaf=1.0 / 1000) == 0                # 1001^3 < 2^32
    # the free function refuses the same arguments before it creates a context
    assert L.symmicp_voxel_downsample(-1, fp(xyz), 3, 1, None, 3, 1, 100, 0.0, 1, fp(out), None, None, None, 100, C.byref(m)) == 1
    assert L.symmicp_voxel_downsample(-1, fp(xyz), 3, 1, None, 3, 1, 100, 0.1, 1, fp(out), fp(nout), None, None, 100, C.byref(m)) == 1


def test_context_untouched(sym, cat):
    """align, downsample other clouds on the same context, align again: identical results, source and correspondences"""
    from symmicp import synth
    d = synth.c4_surface(200_000)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:   # (source() needs it)
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        r1 = e.align()
        src1, nrm1 = e.source()
        idx1, d21 = e.correspondences()
        piv1 = e.pivot()
        e.voxel_downsample(d["src"], 0.003, d["src_n"], 2)
        e.voxel_downsample(cat["src"], 2.0, cat["src_n"])
        src2, nrm2 = e.source()
        assert np.array_equal(src1, src2) and np.array_equal(nrm1, nrm2)
        r2 = e.align()
        idx2, d22 = e.correspondences()
        assert np.array_equal(e.pivot(), piv1)
    assert r1["status"] == r2["status"] == 0 and r1["iters"] == r2["iters"]
    assert np.array_equal(r1["transform"], r2["transform"]) and np.array_equal(r1["diffs"], r2["diffs"])
    assert np.array_equal(idx1, idx2) and np.array_equal(d21, d22)
