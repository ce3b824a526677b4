"""CPU tests of the orientation reference (tests/_orient_ref.py) and of the host side of orient_core.h:
  * the numbers of the issue on the cat + 140 degrees pair of test_global_ref.py: the two clouds disagree on 0.1876 of their normals
    before, on none after at k = 16 (one component each); at k = 10 each cloud has four components of 3282 / 66 / 32 / 20 rows;
  * a sphere with random input signs and a viewpoint outside: every output normal points outward;
  * negating a random half of the input normals leaves the output bit-identical;
  * the tree has n - components edges, is acyclic, and scipy's forest is Kruskal's; the round count is within ceil(log2 n);
  * tests/cpp/orient_core.cpp: the host Boruvka of orient_core.h against Kruskal, trees and parities, and the walk guard, built with
    g++ (and once more under -fsanitize=address,undefined where the toolchain links it)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _knn_ref as K
import _orient_ref as R

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def pair(cat):
    """the cat and its target moved by a further 140 degrees, normals of each cloud alone (k = 10, viewpoint at the origin), and the
    16-NN sets both orientations below start from"""
    from symmicp import synth
    R2, t2 = synth.rotation(140.0, (0.3, 0.5, 0.8)), np.array([40.0, -25.0, 60.0])
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    truth = synth.rigid4(R2, t2) @ np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    src = cat["src"]
    tgt = (cat["tgt"].astype(np.float64) @ R2.T + t2).astype(F)
    rs, rt = K.knn(src, 16)[0], K.knn(tgt, 16)[0]
    # (the first 10 of the 16 nearest in (d2, row) order are the 10 nearest)
    sn, tn = K.emulate(src, rs[:, :10])[0], K.emulate(tgt, rt[:, :10])[0]
    return dict(src=src, tgt=tgt, sn=sn, tn=tn, rs=rs, rt=rt, truth=truth)


def test_cat_pair_agrees_after_orientation_at_k16(pair):
    before = R.disagreement(pair["sn"], pair["tn"], pair["truth"][:3, :3])
    a, b = R.orient(pair["src"], pair["sn"], 16, rows=pair["rs"]), R.orient(pair["tgt"], pair["tn"], 16, rows=pair["rt"])
    after = R.disagreement(a["normals"], b["normals"], pair["truth"][:3, :3])
    print("cat + 140 deg: disagreement %.4f before, %.4f after at k = 16; components %d / %d, rounds %d / %d, flipped %d / %d" % (
        before, after, a["components"], b["components"], a["rounds"], b["rounds"], a["flipped"], b["flipped"]))
    assert round(before, 4) == 0.1876
    assert after == 0.0
    assert a["components"] == b["components"] == 1 and a["largest_component"] == len(pair["src"])


def test_cat_pair_components_at_k10(pair):
    for xyz, nrm, rows in ((pair["src"], pair["sn"], pair["rs"]), (pair["tgt"], pair["tn"], pair["rt"])):
        r = R.orient(xyz, nrm, 10, rows=rows[:, :10])
        sizes = sorted(np.bincount(r["component"])[np.unique(r["component"])].tolist(), reverse=True)
        assert sizes == [3282, 66, 32, 20] and r["components"] == 4 and r["largest_component"] == 3282
    a, b = R.orient(pair["src"], pair["sn"], 10, rows=pair["rs"][:, :10]), R.orient(pair["tgt"], pair["tn"], 10, rows=pair["rt"][:, :10])
    after = R.disagreement(a["normals"], b["normals"], pair["truth"][:3, :3])
    print("cat + 140 deg at k = 10: disagreement %.4f after" % after)
    assert 0.0 < after <= 0.025            # the small components are seeded on their own


def sphere(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    centre = np.array([3.0, -2.0, 10.0])
    return (centre + 2.0 * v).astype(F), v.astype(F), centre


def test_sphere_points_outward_from_random_signs():
    xyz, out, centre = sphere(1500, 1)
    sign = np.where(np.random.default_rng(2).random(len(xyz)) < 0.5, -1.0, 1.0).astype(F)
    # a viewpoint outside: the closest point faces it, so its normal is flipped towards it = outward
    r = R.orient(xyz, out * sign[:, None], 8, viewpoint=(0.0, 0.0, 0.0))
    assert r["components"] == 1
    assert ((r["normals"].astype(np.float64) * (xyz - centre)).sum(1) > 0).all()
    assert np.array_equal(r["flip"], sign < 0) and r["flipped"] == int((sign < 0).sum())
    # Open3D's rule: the top of the sphere along +z points up
    r = R.orient(xyz, out * sign[:, None], 8, direction=(0.0, 0.0, 1.0))
    assert ((r["normals"].astype(np.float64) * (xyz - centre)).sum(1) > 0).all()
    # a viewpoint inside turns every normal towards it: inward (what remains the caller's part)
    r = R.orient(xyz, out * sign[:, None], 8, viewpoint=tuple(centre))
    assert ((r["normals"].astype(np.float64) * (xyz - centre)).sum(1) < 0).all()


def test_output_does_not_depend_on_input_signs(pair):
    xyz, nrm = pair["src"], pair["sn"]
    r0 = R.orient(xyz, nrm, 16, rows=pair["rs"])
    half = np.random.default_rng(3).random(len(xyz)) < 0.5
    neg = nrm.copy()
    neg[half] = -neg[half]
    r1 = R.orient(xyz, neg, 16, rows=pair["rs"])
    assert np.array_equal(r0["normals"].view(np.uint32), r1["normals"].view(np.uint32))
    assert np.array_equal(r0["tree"], r1["tree"]) and np.array_equal(r0["flip"] ^ half, r1["flip"])
    # idempotent
    r2 = R.orient(xyz, r0["normals"], 16, rows=pair["rs"])
    assert np.array_equal(r0["normals"].view(np.uint32), r2["normals"].view(np.uint32)) and r2["flipped"] == 0


def test_tree_is_a_spanning_forest_and_scipy_agrees_with_kruskal(pair):
    for k in (6, 10, 16):
        g = R.graph(pair["src"], pair["sn"], k, pair["rs"][:, :k])
        t = R.forest(g)
        assert np.array_equal(t, R.kruskal(g))
        count, chosen = R.rounds(g)
        assert np.array_equal(chosen, t)                    # Boruvka's rounds choose exactly the forest's edges
        r = R.orient(pair["src"], pair["sn"], k, rows=pair["rs"][:, :k])
        n = len(pair["src"])
        assert len(r["tree"]) == r["tree_edges"] == n - r["components"] and r["rounds"] == count <= int(np.ceil(np.log2(n)))
        # acyclic: a union-find over the tree's edges never meets an edge inside one set
        parent = list(range(n))

        def find(x):
            while parent[x] != x:
                x = parent[x]
            return x

        for a, b in r["tree"].tolist():
            a, b = find(a), find(b)
            assert a != b
            parent[a] = b
        assert (r["tree"][:, 0] < r["tree"][:, 1]).all()
        assert len(np.unique(r["component"])) == r["components"] and (r["component"] <= np.arange(n)).all()


def test_ties_everywhere_and_duplicates():
    # a planar grid with identical normals under random signs: every w is 0, the forest is the row tie-break's; all agree afterwards
    gx, gy = np.meshgrid(np.arange(12, dtype=F), np.arange(12, dtype=F), indexing="ij")
    xyz = np.stack([gx.ravel(), gy.ravel(), np.full(gx.size, 5, F)], 1)
    sign = np.where(np.random.default_rng(4).random(len(xyz)) < 0.5, -1.0, 1.0).astype(F)
    nrm = np.array([[0, 0, 1]], F) * sign[:, None]
    r = R.orient(xyz, nrm, 5)
    assert r["components"] == 1 and (r["normals"] == np.array([0, 0, -1], F)).all()          # the origin is below the grid
    g = R.graph(xyz, nrm, 5)
    assert not g["wbits"].any() and np.array_equal(R.forest(g), R.kruskal(g))
    # 40 copies of one point: a row beyond the first k is not in its own set, which then has k members
    xyz = np.tile(np.array([[1, 2, 3]], F), (40, 1))
    rows = K.knn(xyz, 4)[0]
    assert (rows == np.arange(4)).all()
    r = R.orient(xyz, np.tile(np.array([[0, 1, 0]], F), (40, 1)), 4)
    assert r["components"] == 1 and r["graph_edges"] == 6 + 36 * 4 and r["flipped"] == 40     # (0, 1, 0) at (1, 2, 3) faces away


def test_boruvka_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the orient_core driver")
    src = os.path.join(ROOT, "tests", "cpp", "orient_core.cpp")
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "icp-symm_amd", "csrc"), src]
    exe = str(tmp_path / "orient_core")
    subprocess.check_call(base + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "orient_core: ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.count(" ok\n") == 13
    # the same program under the sanitizers (a stand-alone program with its own main), where the toolchain can link them
    san = str(tmp_path / "orient_core_san")
    r = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], capture_output=True, text=True)
    if r.returncode == 0:
        out = subprocess.run([san], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "orient_core: ok" in out.stdout, out.stdout + out.stderr
    else:
        print("no sanitizer runtime to link against: the plain build only")
