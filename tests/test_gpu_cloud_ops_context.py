"""The cloud operations that run on a caller's context (estimate_normals, knn, radius_search, fpfh, iss_keypoints, intensity_gradient,
voxel_downsample) leave that context as it was: they build a scratch index behind the target's arrays in the keep-arena and have to
give every byte of it back, on the success path and on every failing one.  Each test aligns the cat pair on a TREE context, takes
a snapshot (source, correspondences, certificates, pivot, the target index and its arrays), runs operations, and asks for the
snapshot and the next alignment to be bit-identical to those of a twin context that never ran an operation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F = np.float32
R_RADIUS, R_FPFH, R_ISS, LEAF = 2.0, 5.53, (8.29, 5.53), 2.0      # in units of the cat's point spacing (about 1.4): a few, ~50, ~100 neighbours


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def engine(sym):
    return sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=20, apply=sym.APPLY_INCREMENTAL)      # (source() needs INCREMENTAL)


def load(e, cat, swap=False):
    a, b = ("src", "tgt") if swap else ("tgt", "src")
    e.set_target(cat[a], cat[a + "_n"])
    e.set_source(cat[b], cat[b + "_n"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind in "fiu" else a


def snapshot(e):
    """everything of the context an operation could disturb, by name"""
    out = dict(zip(("src", "src_n", "corr", "corr_d2", "cert", "hood", "hood_T", "winner"), [*e.source(), *e.correspondences(), *e.certificates()]))
    out["pivot"] = e.pivot()
    ix = e.index_arrays()      # index_info's scalars and the index's arrays themselves (they live in the keep-arena)
    out.update(("ix." + k, np.asarray(v)) for k, v in ix.items())
    return out


def differing(a, b, skip=()):
    """names of the entries that are not bit-identical"""
    if isinstance(a, (tuple, list)):
        a, b = dict(enumerate(a)), dict(enumerate(b))
    assert a.keys() == b.keys()
    return [k for k in a if k not in skip and not (a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])))]


# set_source does not clear the 8 member words of a pair's neighbourhood certificate (their validity is a bit of the pair's certificate):
# for a pair that never got one they are whatever the allocation held, so two contexts agree on them only by accident.  One context's
# own snapshots compare in full.
HOOD = ("hood",)


def same_result(r, q):
    return (r["status"] == q["status"] == 0 and r["iters"] == q["iters"] and np.array_equal(bits(r["transform"]), bits(q["transform"]))
            and np.array_equal(bits(r["diffs"]), bits(q["diffs"])))


@pytest.fixture(scope="module")
def twin(sym, cat):
    """the context that never runs an operation: first alignment, its snapshot, the alignment after it, its snapshot; the same for
    the swapped pair on a fresh context"""
    with engine(sym) as e:
        load(e, cat)
        r1 = e.align()
        s1 = snapshot(e)
        r2 = e.align()
        s2 = snapshot(e)
    with engine(sym) as e:
        load(e, cat, swap=True)
        rs = e.align()
        ss = snapshot(e)
    return dict(r1=r1, s1=s1, r2=r2, s2=s2, r_swap=rs, s_swap=ss)


@pytest.fixture(scope="module")
def intensity(cat):
    x = cat["src"].astype(np.float64)
    return (np.sin(0.05 * x[:, 0]) + 0.5 * np.cos(0.07 * x[:, 1]) + 0.01 * x[:, 2]).astype(F)


@pytest.fixture(scope="module")
def bad(cat):
    """the source with one NaN coordinate: refused by the index build, after the cloud is already staged in the keep-arena"""
    b = cat["src"].copy()
    b[17, 1] = np.nan
    return b


def aligned(sym, cat, twin):
    e = engine(sym)
    load(e, cat)
    assert same_result(e.align(), twin["r1"])
    s = snapshot(e)
    assert differing(s, twin["s1"], HOOD) == []
    return e, s


def status_of(sym, call):
    try:
        call()
    except sym.SymmIcpError as err:
        return err.status
    return sym.OK


def run_failures(sym, e, cat, bad, check):
    """every failing call, then the same call with valid arguments; check() after each"""
    src, nrm = cat["src"], cat["src_n"]
    # the outputs do not fit: returns from the middle of the body, the scratch index built
    st, _, _, _, _, total = e.radius_search_raw(src, R_RADIUS)
    assert st == sym.OK and total > 1
    assert e.radius_search_raw(src, R_RADIUS, cap=total - 1)[0] == sym.ERR_SIZE
    check()
    assert e.radius_search_raw(src, R_RADIUS, cap=total)[0] == sym.OK
    check()
    cfg = sym.iss_config(*R_ISS)
    st, _, count, _, _ = e.iss_keypoints_raw(src, cfg, cap=len(src))
    assert st == sym.OK and count > 1
    assert e.iss_keypoints_raw(src, cfg, cap=count - 1)[0] == sym.ERR_SIZE
    check()
    st, rows, count2, _, _ = e.iss_keypoints_raw(src, cfg, cap=count)
    assert st == sym.OK and count2 == count and (rows[:count] >= 0).all()
    check()
    st, _, m = e.voxel_downsample_raw(src, LEAF, nrm)
    assert st == sym.OK and m > 1
    st, r, m2 = e.voxel_downsample_raw(src, LEAF, nrm, cap=m - 1)
    assert st == sym.ERR_SIZE and r is None and m2 == m
    check()
    assert e.voxel_downsample_raw(src, LEAF, nrm, cap=m)[0] == sym.OK
    check()
    # a non-finite coordinate: fails inside the index build, on the set-up's own release
    assert e.radius_search_raw(bad, R_RADIUS)[0] == sym.ERR_ARG
    check()
    assert e.radius_search_raw(src, R_RADIUS)[0] == sym.OK
    check()
    assert status_of(sym, lambda: e.fpfh(bad, nrm, R_FPFH)) == sym.ERR_ARG
    check()
    assert np.isfinite(e.fpfh(src, nrm, R_FPFH)).all()
    check()
    assert status_of(sym, lambda: e.knn(bad, 10)) == sym.ERR_ARG
    check()
    assert (e.knn(src, 10)[0] >= 0).all()
    check()


def test_success_paths_leave_the_context(sym, cat, twin, intensity):
    """estimate_normals, its strided form, knn and intensity_gradient: no other test runs them between two alignments"""
    src, nrm, n = cat["src"], cat["src_n"], len(cat["src"])
    e, s = aligned(sym, cat, twin)
    with e:
        n1, c1 = e.estimate_normals(src, 10)
        assert differing(snapshot(e), s) == []
        padded = np.zeros((n, 4), F)      # PointXYZ records: x y z and a pad word
        padded[:, :3] = src
        n2, c2 = e.estimate_normals_strided(padded, 4, 1, n, 10)
        assert differing(snapshot(e), s) == []
        n3, c3 = e.estimate_normals_strided(np.ascontiguousarray(src.T), 1, n, n, 10)      # column-major
        assert differing(snapshot(e), s) == []
        assert differing([n1, c1], [n2, c2]) == [] and differing([n1, c1], [n3, c3]) == [] and np.isfinite(n1).all()
        rows, d2 = e.knn(cat["tgt"], 7)
        assert differing(snapshot(e), s) == []
        assert rows.min() >= 0 and rows.max() < len(cat["tgt"]) and (np.diff(d2, axis=1) >= 0).all()
        g = e.intensity_gradient(src, nrm, intensity, 10)
        assert differing(snapshot(e), s) == []
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        assert same_result(e.align(), twin["r2"])
        assert differing(snapshot(e), twin["s2"], HOOD) == []


def test_failure_paths_leave_the_context(sym, cat, twin, bad):
    """ERR_SIZE from the middle of three bodies, ERR_ARG from the index build of three more: after each the snapshot is unchanged
    and the same call with valid arguments succeeds; the alignment after them is the twin's"""
    e, s = aligned(sym, cat, twin)
    with e:
        def check():
            assert differing(snapshot(e), s) == []
        run_failures(sym, e, cat, bad, check)
        assert same_result(e.align(), twin["r2"])
        assert differing(snapshot(e), twin["s2"], HOOD) == []


def test_keep_arena_is_still_the_targets(sym, cat, twin, bad):
    """after the failures a new target goes into the same keep-arena: the swapped pair aligns as on a fresh context"""
    e, _ = aligned(sym, cat, twin)
    with e:
        run_failures(sym, e, cat, bad, lambda: None)
        load(e, cat, swap=True)
        assert same_result(e.align(), twin["r_swap"])
        assert differing(snapshot(e), twin["s_swap"], HOOD) == []


# ---- the reverse index beside the target's store ---------------------------------------------------------------------------------
# symmicp_evaluate on a context without a tree index, the reverse probe and the reciprocal passes build an index with a store of its own
# while the context holds a target in its store: the target's arrays, the scratch index of a cloud operation and that index must not meet.

@pytest.mark.parametrize("corr", ["BRUTE", "IDENTITY"])
def test_evaluate_on_a_context_without_a_tree_index(sym, cat, corr):
    """BRUTE and IDENTITY contexts get a scratch reverse index over the target they hold: the alignment and the correspondences after it
    are those of a context that never evaluated; after a cloud operation the swapped pair aligns as on a fresh context"""
    kw = dict(mode=sym.MODE_PAPER, corr=getattr(sym, "CORR_" + corr), max_iters=20, apply=sym.APPLY_INCREMENTAL)

    def state(e):
        return [*e.correspondences(), *e.source(), e.pivot()]

    with sym.Engine(**kw) as e, sym.Engine(**kw) as t, sym.Engine(**kw) as fresh:
        load(e, cat)
        load(t, cat)
        assert same_result(e.align(), t.align())
        X = e.transform()
        ev = e.evaluate(X, R_RADIUS, want_pairs=True)
        one_shot = sym.evaluate_registration(cat["src"], cat["tgt"], X, R_RADIUS, want_pairs=True)
        assert ev["inliers"] == one_shot["inliers"] > 0 and differing([ev["nn"], ev["d2"]], [one_shot["nn"], one_shot["d2"]]) == []
        assert differing(state(e), state(t)) == []
        assert same_result(e.align(), t.align())
        assert differing(state(e), state(t)) == []
        rows, d2 = e.knn(cat["tgt"], 7)
        assert rows.min() >= 0 and rows.max() < len(cat["tgt"]) and (np.diff(d2, axis=1) >= 0).all()
        assert differing(state(e), state(t)) == []
        load(e, cat, swap=True)
        load(fresh, cat, swap=True)
        assert same_result(e.align(), fresh.align())
        assert differing(state(e), state(fresh)) == []
        assert e.evaluate(None, R_RADIUS)["inliers"] == fresh.evaluate(None, R_RADIUS)["inliers"]


def test_failure_inside_the_reverse_build(sym, cat, bad):
    """the reverse probe over a database with one NaN coordinate is refused by the index build, in the probe's own store: the context's
    target index, its source index and the last pass's states stay as they were, and the next pass is the twin's"""
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=6, fixed_iters=1)

    def state(e):
        info = e.reciprocal_info()
        out = dict(zip(("corr", "corr_d2"), e.correspondences()))
        out.update(("ix." + k, np.asarray(v)) for k, v in e.index_arrays().items())
        return out, (e.rejection_state(), e.reciprocal_state(), info["index_valid"], info["index_builds"])

    with sym.Engine(**kw) as e, sym.Engine(**kw) as t:
        for x in (e, t):
            load(x, cat)
            x.set_reciprocal(True)
        assert np.array_equal(e.begin()["sums"], t.begin()["sums"])
        arrays, scalars = state(e)
        assert scalars[2:] == (True, 1)
        q = cat["tgt"][:70]
        assert status_of(sym, lambda: e.reverse_nn_probe(bad, q)) == sym.ERR_ARG
        arrays1, scalars1 = state(e)
        assert differing(arrays1, arrays) == [] and scalars1 == scalars
        assert np.array_equal(e.step()["sums"], t.step()["sums"]) and e.reciprocal_state() == t.reciprocal_state()
        lab, d2 = e.reverse_nn_probe(cat["src"], q)
        assert lab.min() >= 0 and lab.max() < len(cat["src"]) and np.isfinite(d2).all()
        assert np.array_equal(e.step()["sums"], t.step()["sums"]) and e.reciprocal_info()["index_builds"] == 1


def test_target_scratch_and_reverse_index_on_one_context(sym, cat):
    """a reciprocal alignment (the source index in its own store), knn (a scratch index behind the target's arrays) and evaluate (the
    target's own index): the next alignment and the snapshot are the twin's, and the source index was built once"""
    e, t = engine(sym), engine(sym)
    with e, t:
        for x in (e, t):
            load(x, cat)
            x.set_reciprocal(True)
        assert same_result(e.align(), t.align())
        s = snapshot(e)
        assert differing(s, snapshot(t), HOOD) == []
        rows, _ = e.knn(cat["tgt"], 7)
        assert rows.min() >= 0 and rows.max() < len(cat["tgt"])
        ev = e.evaluate(None, R_RADIUS)
        assert 0 < ev["inliers"] <= len(cat["src"])
        assert differing(snapshot(e), s) == []
        assert same_result(e.align(), t.align())
        assert differing(snapshot(e), snapshot(t), HOOD) == []
        assert e.reciprocal_state() == t.reciprocal_state()
        assert e.reciprocal_info() == t.reciprocal_info() and e.reciprocal_info()["index_builds"] == 1


def test_no_target_yet(sym, cat, twin):
    """on a context without a target the operation sizes the keep-arena itself; the target set afterwards reuses it"""
    src = cat["src"]
    with engine(sym) as e:
        knn0 = e.knn(src, 10)
        rad0 = e.radius_search(src, R_RADIUS)
        load(e, cat)
        assert same_result(e.align(), twin["r1"])
        assert differing(snapshot(e), twin["s1"], HOOD) == []
        # the same two on the context that now holds clouds
        assert differing(knn0, e.knn(src, 10)) == []
        assert differing(rad0, e.radius_search(src, R_RADIUS)) == []
        assert differing(snapshot(e), twin["s1"], HOOD) == []
    with engine(sym) as e:      # radius_search first: the other entry's keep.cap == 0 branch
        rad1 = e.radius_search(src, R_RADIUS)
        knn1 = e.knn(src, 10)
        assert differing(rad0, rad1) == [] and differing(knn0, knn1) == []
        load(e, cat)
        assert same_result(e.align(), twin["r1"])
