"""tests/_voxel_ref.py (the numpy reference the GPU voxel downsample is held to bit for bit) against a plain per-point loop:
every point's voxel from float32 scalar ops, a dict of row lists, sums one float32 add at a time in row order.  CPU only."""
import numpy as np
import pytest

import _voxel_ref as V

F = np.float32


def loop_ref(xyz, leaf, nrm=None, min_points=1):
    xyz = np.asarray(xyz, F)
    inv = F(1) / F(leaf)
    cells = [tuple(int(np.floor(F(p[k]) * inv)) for k in range(3)) for p in xyz]
    lo = [min(c[k] for c in cells) for k in range(3)]
    hi = [max(c[k] for c in cells) for k in range(3)]
    nx, ny = hi[0] - lo[0] + 1, hi[1] - lo[1] + 1
    vox = {}
    for i, c in enumerate(cells):
        key = (c[0] - lo[0]) + nx * ((c[1] - lo[1]) + ny * (c[2] - lo[2]))
        vox.setdefault(key, []).append(i)
    out_xyz, out_nrm, out_cnt = [], [], []
    voxel_of = np.full(len(xyz), -1, np.int32)
    for key in sorted(vox):
        members = vox[key]
        if len(members) < min_points:
            continue
        for i in members:
            voxel_of[i] = len(out_xyz)
        s = [F(0), F(0), F(0)]
        for i in members:
            s = [F(s[k] + xyz[i, k]) for k in range(3)]
        out_xyz.append([F(s[k] / F(len(members))) for k in range(3)])
        out_cnt.append(len(members))
        if nrm is not None:
            t = [F(0), F(0), F(0)]
            for i in members:
                t = [F(t[k] + F(nrm[i, k])) for k in range(3)]
            l2 = F(F(F(t[0] * t[0]) + F(t[1] * t[1])) + F(t[2] * t[2]))
            if l2 > 0:
                ln = F(np.sqrt(l2))
                out_nrm.append([F(t[k] / ln) for k in range(3)])
            else:
                out_nrm.append([F(0), F(0), F(0)])
    return dict(xyz=np.array(out_xyz, F).reshape(-1, 3), nrm=None if nrm is None else np.array(out_nrm, F).reshape(-1, 3),
                count=np.array(out_cnt, np.int32), voxel_of=voxel_of)


def same(a, b):
    for k in ("xyz", "count", "voxel_of"):
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    assert (a["nrm"] is None) == (b["nrm"] is None)
    if a["nrm"] is not None:
        assert np.array_equal(a["nrm"].view(np.uint32), b["nrm"].view(np.uint32))


def unit(v):
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def cloud(seed, n, lo, hi):
    rng = np.random.default_rng(seed)
    return rng.uniform(lo, hi, (n, 3)).astype(F), unit(rng.normal(size=(n, 3)))


@pytest.mark.parametrize("leaf,min_points", [(0.25, 1), (0.5, 1), (0.5, 3), (0.1, 2), (1.7, 10)])
def test_negative_coordinates(leaf, min_points):
    xyz, nrm = cloud(1, 600, -2.0, 1.0)
    same(V.voxel_downsample(xyz, leaf, nrm, min_points), loop_ref(xyz, leaf, nrm, min_points))


def test_points_on_voxel_faces():
    # x = k * leaf exactly, and a lattice of them: the floor decides which side a face point falls on
    leaf = 0.25
    g = np.arange(-4, 5, dtype=F) * F(leaf)
    xyz = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3).astype(F)
    xyz = np.concatenate([xyz, xyz + F(0.0625)])
    rng = np.random.default_rng(2)
    nrm = unit(rng.normal(size=xyz.shape))
    r = V.voxel_downsample(xyz, leaf, nrm)
    same(r, loop_ref(xyz, leaf, nrm))
    assert r["count"].max() == 2 and len(r["count"]) == 9 ** 3


def test_leaf_larger_than_the_cloud():
    xyz, nrm = cloud(3, 300, 0.1, 0.4)
    r = V.voxel_downsample(xyz, 10.0, nrm)
    same(r, loop_ref(xyz, 10.0, nrm))
    assert len(r["xyz"]) == 1 and r["count"][0] == 300 and np.all(r["voxel_of"] == 0)


def test_large_offset():
    # coordinates around 1e4 with a fine leaf: the float32 rounding of x * inv decides the voxel (not the exact quotient)
    xyz, nrm = cloud(4, 800, 0.0, 0.05)
    xyz = (xyz + F(10000.0)).astype(F)
    for leaf in (0.003, 0.01, 0.0073):
        same(V.voxel_downsample(xyz, leaf, nrm), loop_ref(xyz, leaf, nrm))
    inv = F(1) / F(0.003)
    exact = np.floor(xyz.astype(np.float64) / 0.003)
    assert np.any(np.floor(xyz * inv) != exact)        # the case is real: fp32 and exact cells differ somewhere


def test_min_points_and_dropped_rows():
    xyz, nrm = cloud(5, 500, 0.0, 1.0)
    for mp in (1, 2, 3, 5, 10, 1000):
        r = V.voxel_downsample(xyz, 0.2, nrm, mp)
        same(r, loop_ref(xyz, 0.2, nrm, mp))
        assert np.all(r["count"] >= mp)
        assert np.array_equal(np.bincount(r["voxel_of"][r["voxel_of"] >= 0], minlength=len(r["count"])), r["count"])


def test_x_fastest_order():
    leaf = 1.0
    pts = np.array([[0.5, 0.5, 1.5], [1.5, 0.5, 0.5], [0.5, 1.5, 0.5], [0.5, 0.5, 0.5], [1.5, 1.5, 1.5]], F)
    r = V.voxel_downsample(pts, leaf)
    # keys: x + 2 (y + 2 z): (0,0,0) 0, (1,0,0) 1, (0,1,0) 2, (0,0,1) 4, (1,1,1) 7
    assert np.array_equal(r["xyz"], pts[[3, 1, 2, 0, 4]])
    assert np.array_equal(r["voxel_of"], [3, 1, 2, 0, 4])
    same(r, loop_ref(pts, leaf))


def test_zero_normals_and_cancelling_normals():
    xyz = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [1.1, 0.1, 0.1], [1.2, 0.1, 0.1], [2.5, 0.5, 0.5]], F)
    nrm = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1], [0, 0, -1], [0, 3, 4]], F)
    r = V.voxel_downsample(xyz, 1.0, nrm)
    same(r, loop_ref(xyz, 1.0, nrm))
    assert np.array_equal(r["nrm"], np.array([[0, 0, 0], [0, 0, 0], [0, 0.6, 0.8]], F))


def test_sequential_sum_is_not_pairwise():
    # one heavy voxel: the reference's sum is the left-to-right float32 one, which differs from np.sum's pairwise order here
    rng = np.random.default_rng(6)
    xyz = (rng.uniform(0, 1, (50000, 3)) * [1, 1e-3, 1e3]).astype(F)
    r = V.voxel_downsample(xyz, 2000.0)
    acc = np.add.accumulate(xyz, axis=0, dtype=F)[-1]
    assert np.array_equal(r["xyz"][0], acc / F(len(xyz)))
    pairwise = np.array([np.ascontiguousarray(xyz[:, k]).sum(dtype=F) for k in range(3)], F)    # (contiguous: numpy sums pairwise)
    assert not np.array_equal(r["xyz"][0], pairwise / F(len(xyz)))


def test_mixed_voxel_sizes_match_the_loop():
    rng = np.random.default_rng(7)
    xyz = np.concatenate([rng.normal(0, 0.02, (400, 3)), rng.uniform(-1, 1, (300, 3))]).astype(F)
    nrm = unit(rng.normal(size=xyz.shape))
    for leaf, mp in ((0.05, 1), (0.3, 4), (0.011, 1)):
        same(V.voxel_downsample(xyz, leaf, nrm, mp), loop_ref(xyz, leaf, nrm, mp))


def test_grid_errors():
    xyz, _ = cloud(8, 10, 0.0, 1.0)
    for leaf in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(V.GridError):
            V.voxel_downsample(xyz, leaf)
    with pytest.raises(V.GridError):
        V.voxel_downsample(xyz, 1e-12)                 # int32 overflow of the cell index
    big = np.array([[0, 0, 0], [1, 1, 1]], F)
    with pytest.raises(V.GridError):
        V.voxel_downsample(big, 1.0 / 2000)            # 2001^3 > 2^32 voxels, every index fits an int
    bad = xyz.copy()
    bad[3, 1] = np.nan
    with pytest.raises(V.GridError):
        V.voxel_downsample(bad, 0.1)
    with pytest.raises(V.GridError):
        V.voxel_downsample(xyz, 0.1, min_points=0)
