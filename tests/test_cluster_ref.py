"""CPU tests of the clustering reference (tests/_cluster_ref.py) and of the union-find of the kernels on the host (cluster_core.h):
  * the reference against answers written down by hand on the smallest shapes, and on the shapes that stress the union;
  * the reference against scikit-learn's DBSCAN: core set, labels on core rows and noise set EQUAL; border rows are left out of that
    comparison (the header's border rule is a deliberate departure) and the number of differing ones is printed;
  * tests/cpp/cluster_core.cpp: the host instantiation of find / unite over edge lists in adversarial orders, built with g++ (and once
    more under -fsanitize=address,undefined where the toolchain links it)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _cluster_ref as CR
from conftest import ROOT

SP = CR.CAT_SPACING


@pytest.fixture(scope="module")
def scene(cat):
    return CR.scene(cat["src"])


@pytest.mark.parametrize("case", CR.small_cases(), ids=lambda c: c[0])
def test_reference_on_hand_built_answers(case):
    name, x, eps, mp, want = case
    r = CR.cluster(x, eps, mp)
    assert np.array_equal(r["labels"], want), (r["labels"], r["neighbors"])
    c = int(want.max()) + 1
    assert r["clusters"] == c and np.array_equal(r["sizes"], np.bincount(want[want >= 0], minlength=c))
    assert np.array_equal(r["core"], r["neighbors"] + 1 >= mp)
    assert CR.numbering_is_by_lowest_core_row(r["labels"], r["core"])


def test_border_point_details():
    x, want = CR.border_case(tie=True, b_first=False)
    r = CR.cluster(x, 1.0, 4)
    assert r["core"].tolist() == [False, True, True, True, True, True, True, True, True, False, False]
    assert r["neighbors"][10] == 2 and r["root"][10] == 1 and r["root"][9] == 5      # A's representative is its lowest CORE row, 1


@pytest.mark.parametrize("case", CR.stress_cases(), ids=lambda c: c[0])
def test_reference_on_the_stress_shapes(case):
    name, x, eps = case
    r = CR.cluster(x, eps, 1)
    assert r["clusters"] == 1 and not r["labels"].any() and (r["root"] == 0).all() and r["sizes"].tolist() == [len(x)]


def test_cat_cluster_counts(cat):
    got = [CR.cluster(cat["src"], m * SP, 1)["clusters"] for m in (1, 1.5, 2, 3, 6)]
    assert got == [2067, 823, 201, 8, 1]
    for m, mp in ((2, 5), (2, 10), (1.5, 6), (1.5, 8)):
        r = CR.cluster(cat["src"], m * SP, mp)
        border, noise = int((~r["core"] & (r["labels"] >= 0)).sum()), int((r["labels"] < 0).sum())
        assert 30 <= r["clusters"] <= 50 and 400 <= border <= 560 and 800 <= noise <= 2601, (m, mp, r["clusters"], border, noise)


def test_size_filter_and_renumbering(scene):
    full = CR.cluster(scene, 2 * SP, 5)
    r = CR.cluster(scene, 2 * SP, 5, 10, 300)
    keep = (full["sizes"] >= 10) & (full["sizes"] <= 300)
    assert 0 < keep.sum() < len(keep) and r["clusters"] == keep.sum() and np.array_equal(r["sizes"], full["sizes"][keep])
    assert np.array_equal(r["core"], full["core"]) and np.array_equal(r["neighbors"], full["neighbors"])      # before the filter
    renum = np.append(np.where(keep, np.cumsum(keep) - 1, -1), -1)
    assert np.array_equal(r["labels"], renum[full["labels"]])
    assert np.array_equal(CR.cluster(scene, 2 * SP, 5, 0, 300)["sizes"], full["sizes"][full["sizes"] <= 300])


def test_row_order_does_not_matter(scene):
    """the partition of a permuted cloud is the partition of the cloud (no border row of these settings sits at a bit-equal distance
    from two clusters: the GPU test relies on that) and the labels follow the numbering the header prescribes"""
    perm = np.random.default_rng(9).permutation(len(scene))
    for eps, mp in ((3 * SP, 1), (2 * SP, 5)):
        a, b = CR.cluster(scene, eps, mp), CR.cluster(scene[perm], eps, mp)
        back = np.empty(len(scene), np.int32)
        back[perm] = b["labels"]                                  # row i of the permuted cloud is row perm[i]
        assert CR.partition(back) == CR.partition(a["labels"])
        assert CR.numbering_is_by_lowest_core_row(b["labels"], b["core"]) and np.array_equal(b["core"], a["core"][perm])


@pytest.mark.parametrize("which,eps,mp", [("cat", 2 * SP, 5), ("cat", 1.5 * SP, 8), ("cat", 3 * SP, 1), ("scene", 2 * SP, 5), ("scene", 1.5 * SP, 6),
                                          ("scene", 2 * SP, 10), ("scene", 3 * SP, 1)])
def test_reference_against_sklearn(cat, scene, which, eps, mp):
    sk = pytest.importorskip("sklearn.cluster")
    x = cat["src"] if which == "cat" else scene
    r = CR.cluster(x, eps, mp)
    # float64 distances of float32 points, compared with the fp32 r: no pair of these clouds lies within rounding of the radius
    fit = sk.DBSCAN(eps=float(np.float32(eps)), min_samples=mp, algorithm="brute").fit(x.astype(np.float64))
    core = np.zeros(len(x), bool)
    core[fit.core_sample_indices_] = True
    assert np.array_equal(core, r["core"])
    assert np.array_equal(fit.labels_[core], r["labels"][core])
    assert np.array_equal(fit.labels_ < 0, r["labels"] < 0)
    border = ~core & (r["labels"] >= 0)
    print("%s eps %.4f min_points %d: %d clusters, %d border rows, %d of them labelled differently by scikit-learn" % (
        which, eps, mp, r["clusters"], int(border.sum()), int((fit.labels_ != r["labels"])[border].sum())))


def test_union_find_on_the_host(tmp_path):
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the union-find driver")
    src = os.path.join(ROOT, "tests", "cpp", "cluster_core.cpp")
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "icp-symm_amd", "csrc"), src]
    exe = str(tmp_path / "cluster_core")
    subprocess.check_call(base + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "cluster_core: ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.count(" ok\n") == 16
    lost = [int(ln.split("lost swaps")[1].split()[0]) for ln in out.stdout.splitlines() if ln.startswith("meddled")]
    assert len(lost) == 5 and sum(lost) > 100              # the retry path of unite() ran
    # the same program under the sanitizers (a stand-alone program with its own main), where the toolchain can link them
    san = str(tmp_path / "cluster_core_san")
    r = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], capture_output=True, text=True)
    if r.returncode == 0:
        out = subprocess.run([san], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "cluster_core: ok" in out.stdout, out.stdout + out.stderr
    else:
        print("no sanitizer runtime to link against: the plain build only")
