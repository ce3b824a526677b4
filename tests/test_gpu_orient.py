"""Consistent normal orientation on the device (symmicp_ctx_orient_normals; kernels_orient.hip) against tests/_orient_ref.py.

The comparison is EXACT: nrm_out bits, flip, component, the sorted tree and every count equal.  The neighbour sets are the exact fp32
sets of the k-NN walk, the edge order is strict and total, so the minimum spanning forest is unique and so is every parity on it: a
mismatch is a kernel bug, not a tolerance question."""
import os
import subprocess

import numpy as np
import pytest

import _knn_ref as K
import _orient_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
CAT_R = 11.05


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
def catn(cat):
    """the cat with its unoriented normals under random signs, and its 16-NN sets (the first k of them are the k-NN sets)"""
    sign = np.where(np.random.default_rng(5).random(len(cat["src"])) < 0.5, -1.0, 1.0).astype(F)
    return dict(xyz=cat["src"], nrm=cat["src_n"] * sign[:, None], rows=K.knn(cat["src"], 16)[0])


COUNTS = ("graph_edges", "tree_edges", "components", "largest_component", "flipped", "rounds")


def same(dev, ref):
    assert dev["normals"].dtype == F and dev["component"].dtype == np.int32 and dev["tree"].dtype == np.int32
    assert {k: dev[k] for k in COUNTS} == {k: ref[k] for k in COUNTS}
    bad = np.nonzero(dev["flip"] != ref["flip"])[0]
    assert len(bad) == 0, (len(bad), bad[:8])
    assert np.array_equal(dev["normals"].view(np.uint32), ref["normals"].view(np.uint32))
    assert np.array_equal(dev["component"], ref["component"])
    assert np.array_equal(dev["tree"], ref["tree"])
    n = len(dev["flip"])
    assert dev["rounds"] <= int(np.ceil(np.log2(n))) + 1


def check_exact(eng, xyz, nrm, k, rows=None, **seed):
    dev = eng.orient_normals(xyz, nrm, k, return_info=True, **seed)
    same(dev, R.orient(xyz, nrm, k, rows=rows, **seed))
    return dev


def unit(v):
    return (v / np.linalg.norm(v, axis=1)[:, None]).astype(F)


# ---- 1. the smallest shapes and ties ------------------------------------------------------------------------------------------------
def test_smallest_shapes(eng):
    rng = np.random.default_rng(1)
    for n, k in ((3, 3), (17, 16), (4, 3), (5, 4)):
        check_exact(eng, rng.random((n, 3)).astype(F) + F(1.0), unit(rng.normal(size=(n, 3))), k)


def test_copies_of_one_point(eng):
    """64 copies: every d2 and every weight ties; a row beyond the first k is not in its own neighbour set"""
    xyz = np.tile(np.array([[1.5, -2.0, 3.0]], F), (64, 1))
    sign = np.where(np.random.default_rng(2).random(64) < 0.5, -1.0, 1.0).astype(F)
    for k in (3, 16):
        dev = check_exact(eng, xyz, np.array([[0.6, 0.0, 0.8]], F) * sign[:, None], k)
        assert dev["components"] == 1 and len(np.unique(dev["normals"].view(np.uint32), axis=0)) == 1


def test_planar_grid_all_weights_tie(eng):
    """32 x 32 grid, one normal under random signs: every w is 0 and the forest is the row tie-break's"""
    gx, gy = np.meshgrid(np.arange(32, dtype=F), np.arange(32, dtype=F), indexing="ij")
    xyz = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 7, F)], 1)
    sign = np.where(np.random.default_rng(3).random(len(xyz)) < 0.5, -1.0, 1.0).astype(F)
    for k in (5, 9):
        dev = check_exact(eng, xyz, np.array([[0, 0, 1]], F) * sign[:, None], k)
        assert dev["components"] == 1 and (dev["normals"][:, 2] == -1).all()
    zero = np.zeros_like(xyz)                                # zero normals are allowed: every w is 1, nothing is flipped but by the seed
    check_exact(eng, xyz, zero, 5)


def test_separate_components_have_a_seed_each(eng):
    """two blobs farther apart than any k-NN edge, and 5 stray points off them (3 near the one, 2 near the other: their nearest
    neighbours are each other and their blob)"""
    rng = np.random.default_rng(4)
    a, b = rng.normal(size=(120, 3)), rng.normal(size=(90, 3))
    stray = np.concatenate([rng.normal(size=(3, 3)) * 3 + [100, 15, 0], rng.normal(size=(2, 3)) * 3 + [-100, -15, 0]])
    xyz = np.concatenate([a + [100, 0, 0], stray, b - [100, 0, 0]]).astype(F)
    nrm = unit(rng.normal(size=(len(xyz), 3)))
    for seed in (dict(), dict(viewpoint=(100.0, 0.5, 0.0)), dict(direction=(0.0, 0.0, 1.0)), dict(direction=(-1.0, 2.0, 0.5))):
        dev = check_exact(eng, xyz, nrm, 6, **seed)
        assert dev["components"] == 2 and dev["largest_component"] == 123
    # Euclidean-separate groups of exactly k + 1 points are components of their own
    xyz = np.concatenate([rng.random((7, 3)) + 50 * i for i in range(6)]).astype(F)
    dev = check_exact(eng, xyz, unit(rng.normal(size=(42, 3))), 6)
    assert dev["components"] == 6 and dev["largest_component"] == 7


# ---- 2. the cat ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_edges(eng, catn, n):
    check_exact(eng, catn["xyz"][:n], catn["nrm"][:n], 8)


@pytest.mark.parametrize("k", [6, 10, 16])
def test_cat_is_exact(eng, catn, k):
    dev = check_exact(eng, catn["xyz"], catn["nrm"], k, rows=catn["rows"][:, :k])
    assert k == 6 or dev["components"] == {10: 4, 16: 1}[k]


@pytest.mark.parametrize("seed", [dict(viewpoint=(0.0, 0.0, 0.0)), dict(viewpoint=(1.0, 2.0, 3.0)), dict(viewpoint=(500.0, -300.0, 80.0)),
                                  dict(direction=(0.0, 0.0, 1.0)), dict(direction=(0.3, -0.5, -0.8))])
def test_seed_rules_inside_and_outside_the_box(eng, catn, seed):
    xyz = catn["xyz"]
    if seed.get("viewpoint") == (1.0, 2.0, 3.0):            # a viewpoint inside the bounding box: its centre
        seed = dict(viewpoint=tuple(float(v) for v in (xyz.min(0) + xyz.max(0)) / 2))
    check_exact(eng, xyz, catn["nrm"], 10, rows=catn["rows"][:, :10], **seed)


def test_two_calls_give_the_same_bytes_and_signs_do_not_matter(sym, eng, catn):
    a = eng.orient_normals(catn["xyz"], catn["nrm"], 16, return_info=True)
    b = eng.orient_normals(catn["xyz"], catn["nrm"], 16, return_info=True)
    c = sym.orient_normals(catn["xyz"], -catn["nrm"], 16, return_info=True)                 # the one-shot form, every sign inverted
    for key in a:
        assert np.array_equal(a[key], b[key]), key
    assert np.array_equal(a["normals"].view(np.uint32), c["normals"].view(np.uint32)) and np.array_equal(a["tree"], c["tree"])
    assert np.array_equal(a["flip"], ~c["flip"])
    d = eng.orient_normals(catn["xyz"], a["normals"], 16, return_info=True)                 # idempotent
    assert d["flipped"] == 0 and np.array_equal(a["normals"].view(np.uint32), d["normals"].view(np.uint32))
    assert np.array_equal(eng.orient_normals(catn["xyz"], catn["nrm"], 16).view(np.uint32), a["normals"].view(np.uint32))


def test_strided_inputs_and_optional_outputs(sym, eng, catn):
    xyz, nrm, n = catn["xyz"][:500], catn["nrm"][:500], 500
    ref = eng.orient_normals(xyz, nrm, 8, return_info=True)
    wide = np.zeros((n, 8), F)
    wide[:, :3], wide[:, 4:7] = xyz, nrm
    cfg = sym.orient_config(8)
    st, out, flip, comp, tree, res = eng.orient_normals_raw(wide, wide.ravel()[4:], cfg, strides=(n, 8, 1, 8, 1))
    assert st == sym.OK and np.array_equal(out.view(np.uint32), ref["normals"].view(np.uint32)) and np.array_equal(comp, ref["component"])
    assert len(tree) == res.tree_edges == ref["tree_edges"] and res.rounds == ref["rounds"]
    cm_x, cm_n = np.ascontiguousarray(xyz.T), np.ascontiguousarray(nrm.T)                    # column-major
    st, out, _, _, _, _ = eng.orient_normals_raw(cm_x, cm_n, cfg, strides=(n, 1, n, 1, n), want=False)
    assert st == sym.OK and np.array_equal(out.view(np.uint32), ref["normals"].view(np.uint32))


# ---- 3. many rounds, many workgroups --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def surface():
    """65 536 rows of a bumpy sheet in random row order, unit normals under random signs"""
    rng = np.random.default_rng(6)
    u, v = rng.random(65536) * 40, rng.random(65536) * 40
    z = 2.0 * np.sin(0.4 * u) * np.cos(0.3 * v)
    xyz = np.stack([u, v, z], 1).astype(F)
    nrm = unit(np.stack([-0.8 * np.cos(0.4 * u) * np.cos(0.3 * v), 0.6 * np.sin(0.4 * u) * np.sin(0.3 * v), np.ones_like(u)], 1))
    sign = np.where(rng.random(len(xyz)) < 0.5, -1.0, 1.0).astype(F)
    return xyz, nrm * sign[:, None]


def test_surface_of_65536_rows(eng, surface):
    xyz, nrm = surface
    dev = check_exact(eng, xyz, nrm, 8, viewpoint=(20.0, 20.0, 50.0))
    print("65 536 rows, k = 8: %d graph edges, %d components, %d rounds" % (dev["graph_edges"], dev["components"], dev["rounds"]))
    big = dev["component"] == np.bincount(dev["component"]).argmax()
    assert big.mean() > 0.9 and (dev["normals"][big, 2] > 0).all()            # the sheet faces the viewpoint above it


# ---- 4. the context is left untouched -----------------------------------------------------------------------------------------------------
def test_context_with_clouds_is_left_untouched(sym, cat, catn):
    """two contexts run the same passes; one of them orients another cloud's normals between two steps: every record, the transform,
    the pairs and index_info are identical, and what the orientation returns on it is the reference's"""
    got = {}

    def passes(between):
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            out = [e.begin(), e.step()]
            info = e.index_info()
            if between:
                got["a"] = e.orient_normals(catn["xyz"], catn["nrm"], 10, return_info=True)
                got["b"] = e.orient_normals(catn["xyz"][:300], catn["nrm"][:300], 5)
                with pytest.raises(sym.SymmIcpError) as err:                                 # and a failing call
                    e.orient_normals(catn["xyz"][:300], catn["nrm"][:300], 17)
                assert err.value.status == sym.ERR_ARG
            after = e.index_info()
            assert sorted(after) == sorted(info) and all(np.array_equal(after[key], info[key]) for key in info)
            out.append(e.step())
            return out, e.certificates(), e.correspondences(), e.source(), e.pivot(), e.transform()
    (ra, ca, ka, sa, pa, ta), (rb, cb, kb, sb, pb, tb) = passes(True), passes(False)
    for x, y in zip(ra, rb):
        assert x["status"] == y["status"] and x["iter"] == y["iter"] and x["pairs"] == y["pairs"]
        assert np.array_equal(x["sums"].view(np.uint64), y["sums"].view(np.uint64))
        assert np.array_equal(x["increment"].view(np.uint32), y["increment"].view(np.uint32))
    assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(ca, cb))
    assert all(np.array_equal(x, y) for x, y in zip(ka, kb)) and all(np.array_equal(x, y) for x, y in zip(sa, sb))
    assert np.array_equal(pa, pb) and np.array_equal(ta, tb)
    same(got["a"], R.orient(catn["xyz"], catn["nrm"], 10, rows=catn["rows"][:, :10]))
    assert np.array_equal(got["b"].view(np.uint32), R.orient(catn["xyz"][:300], catn["nrm"][:300], 5)["normals"].view(np.uint32))


# ---- 5. function: MyICP (Python and C++) and the driver -----------------------------------------------------------------------------------
E2E_BOUND = 1e-4          # tests/test_gpu_global.py's bound on the same comparison: both runs reach the same fixed point
CAT_DIST = CAT_R / 4


@pytest.fixture(scope="module")
def cat140(cat):
    """tests/test_gpu_global.py's pair: the cat and its target moved by a further 140 degrees; MyICP estimates the normals"""
    from symmicp import synth
    R2, t2 = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([40.0, -25.0, 60.0])
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    truth = synth.rigid4(R2, t2) @ np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    return dict(src=cat["src"], tgt=(cat["tgt"].astype(np.float64) @ R2.T + t2).astype(F), truth=truth)


def python_icp(sym, d, iters=30):
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=iters, verbose=False)
    icp.setMaxCorrespondenceDistance(2 * CAT_DIST)
    icp.setInputSource(d["src"], None)
    icp.setInputTarget(d["tgt"], None)
    return icp


def test_oriented_normals_agree_across_the_pair(eng, cat140):
    """the numbers of tests/test_orient_ref.py on the device: 0.1876 of the rows disagree before, none after at k = 16"""
    sn, tn = eng.estimate_normals(cat140["src"], 10)[0], eng.estimate_normals(cat140["tgt"], 10)[0]
    R3 = cat140["truth"][:3, :3]
    before = R.disagreement(sn, tn, R3)
    after = R.disagreement(eng.orient_normals(cat140["src"], sn, 16), eng.orient_normals(cat140["tgt"], tn, 16), R3)
    print("cat + 140 deg on the device: disagreement %.4f before, %.4f after" % (before, after))
    assert 0.17 <= before <= 0.21 and after == 0.0


def test_myicp_global_init_with_oriented_normals(sym, cat140):
    """MyICP with GlobalInit orient_k = 16 ends where the same engine ends from the true transform"""
    d = cat140
    icp = python_icp(sym, d)
    icp.setGlobalInit(fpfh_radius=CAT_R, max_dist=CAT_DIST, hypotheses=65536, seed=1, orient_k=16)
    ra = icp.align()
    g = icp.globalResult()
    rb = python_icp(sym, d).align(d["truth"])
    assert ra["status"] == rb["status"] == sym.OK and g["status"] == sym.OK
    diff = float(np.abs(ra["transform"].astype(np.float64) - rb["transform"]).max())
    print("cat + 140 deg, orient_k = 16: %d correspondences, %d -> %d inliers; |T_global - T_truth-started| = %.2e" % (
        g["correspondences"], g["inliers_ransac"], g["inliers_final"], diff))
    assert diff <= E2E_BOUND
    for bad in (2, 17):
        icp.setGlobalInit(fpfh_radius=CAT_R, max_dist=CAT_DIST, hypotheses=4000, seed=1, orient_k=bad)
        with pytest.raises(sym.SymmIcpError) as e:
            icp.align()
        assert e.value.status == sym.ERR_ARG


def test_myicp_python_set_orient_normals(sym, eng, cat140):
    d = cat140
    plain = eng.estimate_normals(d["src"], 10)[0]
    want = eng.orient_normals(d["src"], plain, 16)
    icp = python_icp(sym, d, iters=2)
    icp.setOrientNormals(16)
    assert icp.align()["status"] == sym.OK
    assert np.array_equal(icp.normals_src.view(np.uint32), want.view(np.uint32)) and not np.array_equal(want, plain)
    icp = python_icp(sym, d, iters=2)                       # supplied normals are left alone
    icp.setOrientNormals(16)
    icp.setInputSource(d["src"], plain)
    assert icp.align()["status"] == sym.OK and np.array_equal(icp.normals_src, plain)
    assert np.array_equal(icp.normals_tgt.view(np.uint32), eng.orient_normals(d["tgt"], eng.estimate_normals(d["tgt"], 10)[0], 16).view(np.uint32))
    icp = python_icp(sym, d, iters=2)
    icp.setOrientNormals(17)
    with pytest.raises(sym.SymmIcpError) as e:
        icp.align()
    assert e.value.status == sym.ERR_ARG


def test_myicp_cpp(sym, eng, cat140, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_orient")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for fname in ("src", "tgt"):
        np.ascontiguousarray(cat140[fname], F).tofile(tmp_path / (fname + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "myicp_orient: ok" in r.stdout, r.stdout + r.stderr
    # the two classes make the same calls: the same bits as the Python entries
    for fname in ("src", "tgt"):
        want = eng.orient_normals(cat140[fname], eng.estimate_normals(cat140[fname], 10)[0], 16)
        assert np.array_equal(np.fromfile(tmp_path / (fname + "_nrm.f32"), F).reshape(-1, 3).view(np.uint32), want.view(np.uint32))


def test_icp_align_driver_orient_normals(sym, cat140, tmp_path):
    d = cat140
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    a, b, out = str(tmp_path / "a.pcd"), str(tmp_path / "b.pcd"), str(tmp_path / "moved.pcd")
    sym.pcd_write(a, d["src"])
    sym.pcd_write(b, d["tgt"])
    base = [exe, "--mode", "paper", "--corr", "tree", "--iters", "30", "--max-dist", "%r" % (2 * CAT_DIST), "--out", out, "--quiet"]
    init = ["--init", "global", "--fpfh-radius", "%r" % CAT_R, "--ransac-dist", "%r" % CAT_DIST, "--ransac-iters", "65536", "--seed", "1"]
    r = subprocess.run(base + init + ["--orient-normals", "16", a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    moved, _ = sym.pcd_read(out)
    want = d["src"].astype(np.float64) @ d["truth"][:3, :3].T + d["truth"][:3, 3]
    rms = float(np.sqrt(((moved - want) ** 2).sum(1).mean()))
    print("icp_align --init global --orient-normals 16: rms to the truth %.4f (spacing 1.38)" % rms)
    assert rms < 0.05                                                       # tests/test_gpu_global.py's bound for the same driver
    for bad in (["--orient-normals", "2"], ["--orient-normals", "17"], ["--orient-normals", "x"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64
