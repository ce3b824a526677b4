"""GPU tests of the NDT voxel map (symmicp_ctx_ndt_map, symmicp_ndt_map, symmicp_get_ndt_map; kernels_ndt.hip) against tests/_ndt_ref.py:
key, count and grid exactly, the mean's bits, the covariance's fp64 bits, the inverse covariance M rebuilt from the device's factors within
1e-6 x max|M_ref| (three axes and three o, each rounded to fp32, give <= 4.2e-7), the axes orthonormal to 1e-6, o ordered by ascending
lambda.  Sizes are the small ones at which the build can go wrong, not a workload."""
import numpy as np
import pytest

import _ndt_ref as R

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


def check_map(dev, xyz, resolution, min_points=6, eig_ratio=0.01, tag=""):
    ref = R.build_map(xyz, resolution, min_points, eig_ratio)
    assert np.array_equal(dev["grid"], ref["grid"]), (tag, dev["grid"], ref["grid"])
    assert np.array_equal(dev["key"], ref["key"]), tag
    assert np.array_equal(dev["count"], ref["count"]), tag
    assert np.array_equal(dev["mean"].view(np.uint32), ref["mean"].view(np.uint32)), tag
    assert np.array_equal(dev["cov"].view(np.uint64), ref["cov"].view(np.uint64)), tag
    m = len(ref["key"])
    if m == 0:
        return ref
    M = R.M_of(dev["axes"], dev["inv_eig"])
    bar = 1e-6 * np.abs(ref["M"]).reshape(m, -1).max(1)
    err = np.abs(M - ref["M"]).reshape(m, -1).max(1)
    assert np.all(err <= bar), (tag, int(np.argmax(err / bar)), float((err / bar).max()))
    A = dev["axes"].astype(np.float64)
    gram = np.einsum("vri,vsi->vrs", A, A)
    assert np.abs(gram - np.eye(3)).max() <= 1e-6, tag
    assert np.all(np.diff(dev["inv_eig"], axis=1) <= 0), tag                  # ascending lambda: descending o
    # the device's o against the reference's inflated eigenvalues
    assert np.allclose(dev["inv_eig"], (1.0 / ref["lam"]).astype(F), rtol=1e-6, atol=0), tag
    return ref


def test_seeded_cube_on_both_sides_of_zero(sym, eng):
    rng = np.random.default_rng(20261020)
    x = (rng.random((2000, 3)) - 0.5).astype(F)
    dev = eng.ndt_map(x, 0.25)
    ref = check_map(dev, x, 0.25, tag="cube")
    assert len(ref["key"]) == 64 and ref["grid"].tolist() == [-2, -2, -2, 4, 4, 4]
    # a shuffled input gives the reference of the shuffled rows (sums run in caller row order)
    p = rng.permutation(len(x))
    check_map(eng.ndt_map(x[p], 0.25), x[p], 0.25, tag="shuffled")
    # the one-shot entry is the same map
    one = sym.ndt_map(x, 0.25)
    for k in ("key", "count", "mean", "cov", "axes", "inv_eig", "grid"):
        assert np.array_equal(one[k], dev[k]), k
    # other parameters
    check_map(eng.ndt_map(x, 0.25, min_points=40, eig_ratio=0.2), x, 0.25, 40, 0.2, tag="min_points 40")
    check_map(eng.ndt_map(x, 0.0625, min_points=3), x, 0.0625, 3, tag="fine")


def crafted_cloud(min_points=6):
    """resolution 0.5 (a power of two): one voxel per case along x, cells 0, 2, 4, ... on y = z = 0"""
    rng = np.random.default_rng(11)
    parts = []
    cell = lambda i: F([0.5 * 2 * i, 0.0, 0.0])
    parts.append(cell(0) + rng.uniform(0.05, 0.45, (min_points - 1, 3)).astype(F))              # one point short: dropped
    parts.append(cell(1) + rng.uniform(0.05, 0.45, (min_points, 3)).astype(F))                  # exactly min_points: kept
    parts.append(np.repeat(cell(2)[None] + F([0.25, 0.125, 0.375]), 9, axis=0))                 # coincident: lambda_max = 0, dropped
    t = np.linspace(0.05, 0.45, 7).astype(F)
    parts.append(cell(3) + np.stack([t, t, t], 1))                                              # collinear: kept, two equal inflated o
    uv = rng.uniform(0.05, 0.45, (12, 2)).astype(F)
    parts.append(cell(4) + np.stack([uv[:, 0], uv[:, 1], F(0.25) * np.ones(12, F)], 1))         # coplanar (z constant)
    face = cell(5) + rng.uniform(0.05, 0.45, (8, 3)).astype(F)
    face[0] = cell(5) + F([0.0, 0.25, 0.25])                                                    # exactly on the lower face of cell 10: it
    parts.append(face)                                                                          # belongs to cell 10, not to cell 9
    return np.concatenate(parts).astype(F)


def test_crafted_voxels(eng):
    x = crafted_cloud()
    dev = eng.ndt_map(x, 0.5)
    ref = check_map(dev, x, 0.5, tag="crafted")
    assert dev["key"].tolist() == [2, 6, 8, 10] and dev["count"].tolist() == [6, 7, 12, 8]
    line = dev["inv_eig"][1]
    assert line[0] == line[1] and line[0] > line[2] * 99.0                                      # both raised to 0.01 lambda_max
    plane = dev["inv_eig"][2]
    assert plane[0] > plane[1] * 1.5 and abs(abs(dev["axes"][2][0][2]) - 1.0) < 1e-6            # the flat direction is z
    assert len(ref["key"]) == 4
    # every voxel dropped: an empty map, not an error
    e = eng.ndt_map(x[:5], 0.5)
    assert len(e["key"]) == 0 and e["grid"].tolist() == [0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("n", [1, 5, 6, 63, 64, 65, 257, 2049])
def test_single_voxel_clouds(eng, n):
    x = (np.random.default_rng(n).random((n, 3)) * 0.9 + 3.0).astype(F)
    dev = eng.ndt_map(x, 1.0)
    ref = check_map(dev, x, 1.0, tag="n=%d" % n)
    assert len(ref["key"]) == (1 if n >= 6 else 0)
    if n >= 6:
        assert dev["count"].tolist() == [n] and dev["grid"].tolist() == [3, 3, 3, 1, 1, 1]


def test_row_stride_4_and_the_cap_protocol(sym, eng):
    rng = np.random.default_rng(5)
    x = (rng.random((1500, 3)) - 0.25).astype(F)
    wide = np.full((1500, 4), np.nan, F)
    wide[:, :3] = x
    cfg = sym.ndt_config(0.25)
    st, dev, m = eng.ndt_map_raw(wide, cfg, strides=(1500, 4, 1))
    assert st == sym.OK
    ref = check_map(dev, x, 0.25, tag="stride 4")
    assert m == len(ref["key"]) and m > 8
    # m always; SYMMICP_ERR_SIZE when it does not fit, OK when it just fits; every output may be NULL
    st, r, m1 = eng.ndt_map_raw(x, cfg, cap=m - 1)
    assert st == sym.ERR_SIZE and r is None and m1 == m
    st, r, m1 = eng.ndt_map_raw(x, cfg, cap=m)
    assert st == sym.OK and m1 == m and np.array_equal(r["key"], ref["key"])
    st, r, m1 = eng.ndt_map_raw(x, cfg, cap=0, want=False)
    assert st == sym.ERR_SIZE and m1 == m
    st, r, m1 = eng.ndt_map_raw(x, cfg, cap=m, want=False)
    assert st == sym.OK and m1 == m


def test_ctx_form_leaves_a_tree_context_as_it_was(sym):
    from symmicp import synth
    d = synth.c4_surface(3000)
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=4, fixed_iters=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.begin()
        e.step()
        X0, idx0, ix0 = e.transform().copy(), e.correspondences(), e.index_arrays()
        dev = e.ndt_map(d["tgt"], 0.1)
        check_map(dev, d["tgt"], 0.1, tag="on a TREE context")
        assert np.array_equal(e.transform(), X0)
        idx1 = e.correspondences()
        assert np.array_equal(idx0[0], idx1[0]) and np.array_equal(idx0[1], idx1[1])
        ix1 = e.index_arrays()
        for k in ("tq", "tn", "boxes", "ctop", "cells", "onodes"):
            assert np.array_equal(ix0[k].view(np.uint32), ix1[k].view(np.uint32)), k
        it = e.step()                                   # the loop goes on from where it was
        assert it["iter"] == 2
        with pytest.raises(sym.SymmIcpError) as err:    # a TREE context holds no NDT map
            e.get_ndt_map()
        assert err.value.status == sym.ERR_STATE
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=4, fixed_iters=1) as f:
        f.set_target(d["tgt"], d["tgt_n"])
        f.set_source(d["src"], d["src_n"])
        f.begin()
        f.step()
        assert np.array_equal(f.step()["sums"], it["sums"])


def test_set_ndt_on_a_live_context_equals_a_fresh_set_target(sym):
    from symmicp import synth
    d = synth.c4_surface(4000)
    keys = ("key", "count", "mean", "cov", "axes", "inv_eig", "grid")
    with sym.Engine(mode=sym.MODE_NDT) as e:
        e.set_ndt(resolution=0.2)
        e.set_target(d["tgt"], None)
        first = e.get_ndt_map()
        check_map(first, d["tgt"], 0.2, tag="set_target 0.2")
        e.set_source(d["src"], None)
        e.begin()
        e.set_ndt(resolution=0.1, neighbors=1)
        with pytest.raises(sym.SymmIcpError) as err:    # the loop state was reset, as after set_target
            e.step()
        assert err.value.status == sym.ERR_STATE
        rebuilt = e.get_ndt_map()
        assert e.get_ndt()["neighbors"] == 1 and e.get_ndt()["resolution"] == F(0.1)
        # a refused setter leaves configuration and map as they were
        for bad in (dict(resolution=0.0), dict(min_points=2), dict(eig_ratio=0.0), dict(outlier_ratio=1.0), dict(neighbors=3),
                    dict(resolution=1e-9)):                    # (the last: cells beyond 2^23 on this target)
            with pytest.raises(sym.SymmIcpError) as err:
                e.set_ndt(**dict(dict(resolution=0.1, neighbors=1), **bad))
            assert err.value.status == sym.ERR_ARG, bad
        assert e.get_ndt()["neighbors"] == 1 and e.get_ndt()["resolution"] == F(0.1)
        again = e.get_ndt_map()
        for k in keys:
            assert np.array_equal(again[k], rebuilt[k]), k
        r0 = e.begin()
    with sym.Engine(mode=sym.MODE_NDT) as f:
        f.set_ndt(resolution=0.1, neighbors=1)
        f.set_target(d["tgt"], None)
        fresh = f.get_ndt_map()
        f.set_source(d["src"], None)
        r1 = f.begin()
    check_map(fresh, d["tgt"], 0.1, tag="set_target 0.1")
    for k in keys:
        assert np.array_equal(rebuilt[k], fresh[k]), k
    assert np.array_equal(r0["sums"], r1["sums"])
