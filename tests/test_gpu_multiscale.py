"""Coarse-to-fine alignment (MyICP.setVoxelLevels in C++ and Python, icp_align --scale): the same bits as the composition written
by hand through the C-ABI (downsample, set, align with a guess), parity with a CPU pipeline (tests/_voxel_ref.py + the oracle),
and a pose where one level fails and the levels converge."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _voxel_ref as V
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

TOL_T = 1e-4          # the C4 parity bar (tests/test_gpu_parity.py)
CAT_LEVELS = [(8.0, 10, 16.0), (4.0, 10, 8.0), (0.0, 10, 0.0)]
C4_LEVELS = [(0.02, 10, 0.05), (0.01, 10, 0.02), (0.0, 10, 0.0)]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def _truth_cat():
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    return np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])


def _rot(deg, axis):
    a = np.asarray(axis, float)
    a /= np.linalg.norm(a)
    th = np.radians(deg)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def by_hand(sym, src, sn, tgt, tn, levels, guess=None, mode=None):
    """the composition through the C-ABI alone: downsample both clouds, set them, align from the previous transform"""
    out = []
    with sym.Engine(mode=sym.MODE_PAPER if mode is None else mode, corr=sym.CORR_TREE) as e:
        X = guess
        for leaf, iters, dist in levels:
            if leaf > 0:
                a, b = e.voxel_downsample(src, leaf, sn), e.voxel_downsample(tgt, leaf, tn)
                s_, sn_, t_, tn_ = a["xyz"], a["nrm"], b["xyz"], b["nrm"]
            else:
                s_, sn_, t_, tn_ = src, sn, tgt, tn
            e.set_config(max_iters=iters, max_corr_dist=dist)
            e.set_target(t_, tn_)
            e.set_source(s_, sn_)
            r = e.align(X)
            assert r["status"] == 0, r
            out.append(r)
            X = r["transform"]
    return out


def cpu_pipeline(oracle, src, sn, tgt, tn, levels, guess=None, corr=None):
    """_voxel_ref downsampling, then oracle.align(PAPER, exact NN, guess, max_corr_dist) per level"""
    X = guess
    for leaf, iters, dist in levels:
        if leaf > 0:
            a, b = V.voxel_downsample(src, leaf, sn), V.voxel_downsample(tgt, leaf, tn)
            s_, sn_, t_, tn_ = a["xyz"], a["nrm"], b["xyz"], b["nrm"]
        else:
            s_, sn_, t_, tn_ = src, sn, tgt, tn
        r = oracle.align(s_, sn_, t_, tn_, mode=oracle.MODE_PAPER, corr=oracle.CORR_BRUTE if corr is None else corr, max_iters=iters,
                         max_corr_dist=dist, guess=X)
        assert r["status"] == 0
        X = r["transform"]
    return X


def python_myicp(sym, src, sn, tgt, tn, levels, guess=None):
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, verbose=False)
    icp.setInputSource(src, sn)
    icp.setInputTarget(tgt, tn)
    icp.setVoxelLevels(levels)
    r = icp.align(guess)
    assert r["status"] == 0
    return icp


def test_cpp_and_python_myicp_equal_the_composition_by_hand(sym, cat, tmp_path):
    G = np.eye(4, dtype=np.float32)
    c, s = np.cos(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0))
    G[:2, :2] = [[c, -s], [s, c]]
    G[0, 3] = 1.5
    hand = by_hand(sym, cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], CAT_LEVELS, G)
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_voxel")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for name, arr in (("src", cat["src"]), ("src_n", cat["src_n"]), ("tgt", cat["tgt"]), ("tgt_n", cat["tgt_n"]), ("guess", G),
                      ("levels", np.array(CAT_LEVELS, np.float32))):
        np.ascontiguousarray(arr, np.float32).tofile(tmp_path / (name + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    T = np.fromfile(tmp_path / "out.f32", np.float32).reshape(4, 4)
    per = np.fromfile(tmp_path / "levels_out.f32", np.float32).reshape(-1, 4, 4)
    iters = np.fromfile(tmp_path / "iters.f32", np.float32)
    assert np.array_equal(T.view(np.uint32), hand[-1]["transform"].view(np.uint32))
    for k, h in enumerate(hand):
        assert np.array_equal(per[k], h["transform"]) and iters[k] == h["iters"]
    icp = python_myicp(sym, cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], CAT_LEVELS, G)
    assert np.array_equal(icp.getFinalTransformation().view(np.uint32), T.view(np.uint32))
    assert [x["iters"] for x in icp.levelResults()] == [h["iters"] for h in hand]
    # without levels the C++ object is the single-level align it always was
    plain = np.fromfile(tmp_path / "out_plain.f32", np.float32).reshape(4, 4)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        assert np.array_equal(plain, e.align(G)["transform"])
    assert np.abs(T - _truth_cat()).max() < TOL_T


def test_cat_levels_match_the_cpu_pipeline(sym, cat, oracle):
    icp = python_myicp(sym, cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], CAT_LEVELS)
    X = cpu_pipeline(oracle, cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], CAT_LEVELS)
    T = icp.getFinalTransformation()
    assert np.abs(T - X).max() < TOL_T
    assert np.abs(T - _truth_cat()).max() < TOL_T


def test_c4_levels_match_the_cpu_pipeline(sym, oracle):
    from symmicp import synth
    d = synth.c4_surface(100_000)
    icp = python_myicp(sym, d["src"], d["src_n"], d["tgt"], d["tgt_n"], C4_LEVELS)
    counts = [len(V.voxel_downsample(d["src"], leaf)["xyz"]) for leaf, _, _ in C4_LEVELS[:2]]
    assert counts[0] < counts[1] < len(d["src"])
    X = cpu_pipeline(oracle, d["src"], d["src_n"], d["tgt"], d["tgt_n"], C4_LEVELS, corr=oracle.CORR_GRID)
    T = icp.getFinalTransformation()
    assert np.abs(T - X).max() < TOL_T
    assert np.abs(T - d["truth"]).max() < 5e-4


def test_driver_scale_prints_what_python_myicp_prints(sym, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    shutil.copy(os.path.join(GOLDEN, "cat.pcd"), tmp_path / "cat.pcd")
    shutil.copy(os.path.join(GOLDEN, "cat_out.pcd"), tmp_path / "cat_out.pcd")
    args = ["--mode", "paper", "--corr", "tree", "--scale", "8:10:16", "--scale", "4:10:8", "--scale", "0:10"]
    r = subprocess.run([exe] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    out = r.stdout.split("\n")
    heads = [l for l in out if l.startswith("level ")]
    assert len(heads) == 3 and heads[0].startswith("level 1/3: leaf 8, source 3400 -> ") and heads[2].startswith("level 3/3: leaf 0, source 3400 -> 3400")
    assert out.index(heads[2]) < out.index("iters#1")                  # coarse levels are quiet: iteration lines of the last only
    assert sum(1 for l in out if l == "Result transform:") == 1
    # the Python mirror in a process of its own (its C stdout is the library's): the same text, line for line
    script = ("import sys; sys.path[:0] = [%r, %r]\n"
              "import symmicp\n"
              "icp = symmicp.MyICP(mode=symmicp.MODE_PAPER, corr=symmicp.CORR_TREE)\n"
              "icp.LoadCloud('cat.pcd', 'cat_out.pcd')\n"
              "icp.setVoxelLevels([(8, 10, 16), (4, 10, 8), (0, 10, 0)])\n"
              "icp.RegisterSymm()\n") % (ROOT, os.path.join(ROOT, "icp-symm_amd", "py"))
    p = subprocess.run([sys.executable, "-c", script], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    py = [l for l in p.stdout.split("\n") if not l.startswith("/opt/") and "amdgpu.ids" not in l]
    k1, k2 = out.index("Result transform:"), py.index("Result transform:")
    assert out[k1:k1 + 13] == py[k2:k2 + 13]
    assert [l for l in py if l.startswith("level ")] == heads
    T = np.array([[float(v) for v in out[k1 + 1 + i].split()] for i in range(4)])
    assert np.abs(T - _truth_cat()).max() < 1e-3
    # --scale needs nearest-neighbour pairs, and a well-formed LEAF:ITERS[:MAXDIST]
    assert subprocess.run([exe, "--scale", "8:10"], cwd=tmp_path, capture_output=True).returncode == 64
    assert subprocess.run([exe, "--corr", "tree", "--scale", "8"], cwd=tmp_path, capture_output=True).returncode == 64
    assert subprocess.run([exe, "--corr", "tree", "--scale", "8:x"], cwd=tmp_path, capture_output=True).returncode == 64


def test_identity_pairing_with_levels_is_refused(sym, cat):
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_IDENTITY, verbose=False)
    icp.setInputSource(cat["src"], cat["src_n"])
    icp.setInputTarget(cat["tgt"], cat["tgt_n"])
    icp.setVoxelLevels(CAT_LEVELS)
    with pytest.raises(sym.SymmIcpError) as ei:
        icp.align()
    assert ei.value.status == sym.ERR_ARG


@pytest.mark.parametrize("deg,axis", [(45.0, (0, 0, 1)), (75.0, (1, 1, 1))])
def test_levels_widen_the_convergence_basin(sym, cat, oracle, deg, axis):
    """cat_out turned by a further `deg` about its centroid: single-scale PAPER with the same 30-iteration budget ends far from
    the truth (on the CPU oracle and on the GPU), the three levels end at it"""
    R = _rot(deg, axis)
    ctr = cat["tgt"].mean(0).astype(np.float64)
    tgt = ((cat["tgt"] - ctr) @ R.T + ctr).astype(np.float32)
    tn = (cat["tgt_n"] @ R.T).astype(np.float32)
    A = np.eye(4)
    A[:3, :3] = R
    A[:3, 3] = ctr - R @ ctr
    truth = A @ _truth_cat()
    budget = sum(it for _, it, _ in CAT_LEVELS)
    ro = oracle.align(cat["src"], cat["src_n"], tgt, tn, mode=oracle.MODE_PAPER, corr=oracle.CORR_BRUTE, max_iters=budget)
    assert np.abs(ro["transform"] - truth).max() > 1e-2
    assert np.abs(cpu_pipeline(oracle, cat["src"], cat["src_n"], tgt, tn, CAT_LEVELS) - truth).max() < 1e-3
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=budget) as e:
        e.set_target(tgt, tn)
        e.set_source(cat["src"], cat["src_n"])
        single = e.align()["transform"]
    assert np.abs(single - truth).max() > 1e-2
    icp = python_myicp(sym, cat["src"], cat["src_n"], tgt, tn, CAT_LEVELS)
    assert np.abs(icp.getFinalTransformation() - truth).max() < 1e-3
