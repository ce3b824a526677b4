"""CPU tests of tests/_knn_ref.py, the reference the GPU normals tests (test_gpu_normals.py) hold k_normals_knn to.

Its neighbour sets fed through its emulation of the kernel's arithmetic with the oracle's 64-sweep cap must reproduce
orc_normals_knn bit for bit (sets, moments, Jacobi, flip and curvature all agree, or some point would differ).  The device's
12-sweep cap gives the same bits on these inputs except on neighbourhoods with a repeated smallest eigenvalue (7 points of the
cubic lattice at k = 10, 192 of cat with every point twice at k = 3), where the cap decides.  The k-d tree path must agree with brute force.
"""
import numpy as np
import pytest

import _knn_ref as R

KS = (3, 4, 9, 10, 15, 16)


def _lattice(dims, seed):
    g = np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, len(dims))
    if g.shape[1] == 2:
        g = np.concatenate([g, np.full((len(g), 1), 3)], 1)
    return (g.astype(np.float32) * np.float32(0.125))[np.random.default_rng(seed).permutation(len(g))]


def _clouds(cat, bunny):
    rng = np.random.default_rng(5)
    cloud = rng.random((3000, 3), dtype=np.float32)
    return dict(cat_src=cat["src"], cat_tgt=cat["tgt"], bunny=bunny, cubic=_lattice((16, 16, 16), 1), planar=_lattice((64, 64), 2),
                cat_twice=np.repeat(cat["src"], 2, axis=0),
                cluster=np.concatenate([cloud[:1000], np.tile(np.float32([0.25, 0.5, 0.75]), (20, 1)), cloud[1000:]]))


@pytest.mark.parametrize("name", ["cat_src", "cat_tgt", "bunny", "cubic", "planar", "cat_twice", "cluster"])
def test_reference_reproduces_the_oracle(oracle, cat, bunny, name):
    xyz = _clouds(cat, bunny)[name]
    for k in KS + (7,):
        if name in ("cat_twice", "cubic") and k not in (3, 10, 16):
            continue
        vp = (0.5, 0.5, 2.0)
        rows, d2 = R.knn(xyz, k)
        assert (d2[:, :-1] <= d2[:, 1:]).all() and (rows[:, 0] >= 0).all()
        on, oc = oracle.normals_knn(xyz, k, viewpoint=vp)
        en, ec = R.emulate(xyz, rows, vp, sweeps=64)
        assert np.array_equal(on.view(np.uint32), en.view(np.uint32)) and np.array_equal(oc.view(np.uint32), ec.view(np.uint32)), (k, name)
        # the device stops the Jacobi after 12 sweeps: the same bits, except on neighbourhoods whose two smallest eigenvalues are
        # equal (cubic lattice at k = 10, a point and its copy plus one more at k = 3) -- there the absolute 1e-300 stop is never met
        # and the rotations go on until the cap
        dn, dc = R.emulate(xyz, rows, vp, sweeps=12)
        diff = ~((dn == en).all(1) & (dc == ec))
        if diff.any():
            lam = np.linalg.eigvalsh(R.moments(xyz, rows[diff])[1])
            assert (lam[:, 1] - lam[:, 0] <= 1e-12 * lam.sum(1)).all()


def test_tie_lattice_sets_are_the_lowest_rows(cat):
    """on the cubic lattice k = 10 cuts through the 12-point edge shell: the set must take the shell's lowest rows"""
    xyz = _lattice((16, 16, 16), 1)
    rows, d2 = R.knn(xyz, 10)
    full = ((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(-1)
    for i in range(0, len(xyz), 97):
        order = np.lexsort((np.arange(len(xyz)), full[i]))[:10]
        assert np.array_equal(rows[i], order)
    assert (d2[:, -1] == d2[:, -2]).any()


def test_kdtree_path_matches_brute_force():
    from symmicp import synth
    for xyz in (synth.c4_surface(20000)["src"], synth.c3_uniform(20000)["src"], synth.c5_scan(20000)["src"]):
        sub = np.random.default_rng(3).choice(len(xyz), 1500, replace=False)
        for k in (3, 16):
            a = R.knn(xyz, k, queries=sub)
            b = R._brute(xyz, k, sub)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_emulation_is_unit_free_under_powers_of_two(cat):
    for xyz in (cat["src"], _lattice((64, 64), 2)):
        for k in (3, 10, 16):
            rows, _ = R.knn(xyz, k)
            a = R.emulate(xyz, rows, (0.5, 0.5, 2.0))
            for e2 in (-14, 14):
                s = np.float32(2.0 ** e2)
                b = R.emulate(xyz * s, rows, (0.5 * float(s), 0.5 * float(s), 2.0 * float(s)))
                assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
