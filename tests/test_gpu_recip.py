"""Reciprocal correspondences on the GPU (run with -m gpu on a real MI355X): symmicp_set_reciprocal, the reverse search behind it, and
what it is for.

  1. the reverse search alone (symmicp_ctx_reverse_nn_probe) against the numpy restatement, labels and d2 bits exact;
  2. every pass of a reciprocal context against the restatement (tests/_recip_ref.py): n_c, n_u, n_r, kept, tau's bits, the record, the
     pair count and the reported pairs -- modes x pairings x quantile rules, with a Huber loss, with both gates, COLOR, both source
     orders, both apply modes, ragged sizes; on every one of them the kept set lies inside one-to-one's;
  3. behaviour and lifetime: one-to-one on top changes nothing, off is bit for bit a context that never heard of it, the source index
     survives set_target and the read-only entries and is rebuilt by set_source, setters act at the next pass, align stays in the host
     loop, the refusals;
  4. the partial-overlap pair through Engine, MyICP (Python and C++) and the command-line driver.
The pairs of a pass come from a twin context without rejection driven by the same transforms (its pairs and distances are held to the
oracle's brute force by test_gpu_pass_matrix.py)."""
import math
import os
import subprocess

import numpy as np
import pytest

import _recip_ref as RR
import _record_ref as R
import _reject_ref as J
import _trim_ref as T
from conftest import ROOT

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def surf():
    return T.partial_overlap(20000, 0xC4)


def mode_code(sym, mode):
    return {"paper": sym.MODE_PAPER, "p2p": sym.MODE_P2P, "plane": sym.MODE_PLANE, "gicp": sym.MODE_GICP}[mode]


def corr_code(sym, corr):
    return {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[corr]


def tau_bits(x):
    return int(f32(x).view(np.uint32))


def rigid(rng, t_scale):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(0.2, 2.5)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    X = np.eye(4)
    X[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    X[:3, 3] = rng.normal(size=3) * t_scale
    return X.astype(f32)


# ---- 1. the reverse search --------------------------------------------------------------------------------------------------------
DB_SIZES = [1, 2, 8, 9, 63, 64, 65, 1000, 20011]      # a single leaf, the leaf size, one over, ..., a tree of several levels
Q_SIZES = [1, 63, 64, 65, 4099]


def probe_cloud(kind, n, rng):
    """-> (db, labels or None).  cube: random points; lattice: an integer lattice in shuffled order with permuted labels, ties everywhere;
    coincident: 40 copies of one point (a leaf of more than 8 duplicates) among random ones"""
    if kind == "cube":
        return rng.uniform(-1, 1, (n, 3)).astype(f32), None
    if kind == "lattice":
        m = int(math.ceil(n ** (1.0 / 3.0)))
        g = np.stack(np.meshgrid(np.arange(m), np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 3).astype(f32)
        return g[rng.permutation(len(g))[:n]], (rng.permutation(n) * 2 + 5).astype(np.int32)
    db = rng.uniform(-1, 1, (n, 3)).astype(f32)
    db[rng.permutation(n)[:40]] = db[0]
    return db, rng.permutation(n).astype(np.int32)


def probe_queries(db, n_q, rng, lattice):
    """in the db's frame: db points themselves, points 10 extents outside the box, and points about the box (on half-integers for the
    lattice: exact ties)"""
    lo, hi = db.min(0), db.max(0)
    ext = max(float((hi - lo).max()), 1.0)
    on = db[rng.integers(0, len(db), n_q)]
    if lattice:
        inside = (rng.integers(-2, 2 * int(ext) + 4, (n_q, 3)) * 0.5).astype(f32)
    else:
        inside = rng.uniform(lo - 0.3 * ext, hi + 0.3 * ext, (n_q, 3)).astype(f32)
    far = (lo + (hi - lo) * rng.uniform(0, 1, (n_q, 3)) + 10 * ext * np.sign(rng.normal(size=(n_q, 3)))).astype(f32)
    pick = rng.integers(0, 5, n_q)
    q = np.where((pick == 0)[:, None], on, np.where((pick == 1)[:, None], far, inside)).astype(f32)
    return q, pick == 0


@pytest.mark.parametrize("kind", ["cube", "lattice", "coincident"])
@pytest.mark.parametrize("n_db", DB_SIZES)
def test_reverse_nn_probe_equals_the_restatement(sym, n_db, kind):
    rng = np.random.default_rng(n_db * 7 + len(kind))
    db, labels = probe_cloud(kind, n_db, rng)
    ext = max(float((db.max(0) - db.min(0)).max()), 1.0)
    shift = np.eye(4, dtype=f32)
    shift[:3, 3] = [100 * ext, -100 * ext, 100 * ext]
    if kind == "cube":
        # every query count with every kind of transform
        cases = [(X, n_q) for n_q in Q_SIZES for X in (None, rigid(rng, 1.0), shift)]
    else:
        cases = [(None, 1), (None, 4099), (rigid(rng, 1.0), 63), (rigid(rng, 1.0), 64), (shift, 65), (shift, 4099), (rigid(rng, 1.0), 4099)]
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        for X, n_q in cases:
            qs, on_db = probe_queries(db, n_q, rng, kind == "lattice")
            q = qs if X is None else R.xf_rows(X, qs, 1.0)              # into the frame the probe carries them back from
            lab, d2 = e.reverse_nn_probe(db, q, labels, X)
            y = q if X is None else RR.back_project(RR.inverse_rigid(X), q)
            want, wd2 = RR.back(db, labels, y)
            t = (kind, n_db, n_q, X is not None)
            assert np.array_equal(lab, want), (t, int((lab != want).sum()))
            assert np.array_equal(d2.view(np.uint32), wd2.view(np.uint32)), t
            if X is None:
                assert (d2[on_db] == 0).all(), t
                if kind == "cube":
                    assert np.array_equal(db[lab[on_db]], qs[on_db]), t
            if kind == "coincident" and X is None and n_db >= 40:
                # a query on the pile: the lowest label of the pile
                pile = np.flatnonzero((db == db[0]).all(1))
                one = e.reverse_nn_probe(db, db[:1], labels, None)
                assert len(pile) >= 40 and one[0][0] == labels[pile].min() and one[1][0] == 0


def test_reverse_nn_probe_leaves_the_context_alone_and_refuses_bad_arguments(sym, cat):
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=6, fixed_iters=1)
    with sym.Engine(**kw) as e, sym.Engine(**kw) as t:
        for x in (e, t):
            x.set_target(cat["tgt"], cat["tgt_n"])
            x.set_source(cat["src"], cat["src_n"])
            x.set_reciprocal(True)
        a, b = e.begin(), t.begin()
        assert np.array_equal(a["sums"], b["sums"])
        before = (e.correspondences(), e.rejection_state(), e.reciprocal_state(), e.get_reciprocal(), str(e.index_info()))
        lab, d2 = e.reverse_nn_probe(cat["tgt"][:500], cat["src"][:70])
        want = RR.back(cat["tgt"][:500], None, cat["src"][:70])
        assert np.array_equal(lab, want[0]) and np.array_equal(d2, want[1])
        after = (e.correspondences(), e.rejection_state(), e.reciprocal_state(), e.get_reciprocal(), str(e.index_info()))
        assert all(np.array_equal(u, v) for u, v in zip(before[0], after[0])) and before[1:] == after[1:]
        assert np.array_equal(e.step()["sums"], t.step()["sums"]) and e.reciprocal_state() == t.reciprocal_state()
        db, q = cat["tgt"][:8], cat["src"][:3]
        for call in (lambda: e.reverse_nn_probe(db[:0], q), lambda: e.reverse_nn_probe(db, q[:0]),
                     lambda: e.reverse_nn_probe(db, q, np.array([0, 1, 2, 3, -4, 5, 6, 7], np.int32))):
            with pytest.raises(sym.SymmIcpError) as x:
                call()
            assert x.value.status == sym.ERR_ARG


# ---- 2. every pass ----------------------------------------------------------------------------------------------------------------
RULES = {"alone": dict(), "median2": dict(factor=2.0), "rho0.7": dict(rho=0.7)}


def apply_rules(e, rule, one_to_one=False):
    e.set_reciprocal(True)
    if one_to_one:
        e.set_one_to_one(True)
    if rule.get("factor", 0.0) > 0:
        e.set_median_factor(rule["factor"])
    if rule.get("rho", 1.0) < 1:
        e.set_trim_fraction(rule["rho"])


def check_passes(sym, d, mode, corr, rule, loss=False, mcd=0.0, mnd=-2.0, steps=3, tag="", sort_source=None, apply=None, one_to_one=False, bite=True):
    """begin and `steps` steps of a reciprocal context against the numpy restatement -> (passes checked, [kept mask per pass])"""
    m = mode_code(sym, mode)
    src, src_n, tgt, tgt_n = d["src"], d["src_n"], d["tgt"], d["tgt_n"]
    kw = dict(mode=m, corr=corr_code(sym, corr), max_iters=steps + 2, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=mnd)
    if sort_source is not None:
        kw["sort_source"] = sort_source
    incremental = apply == "incremental"
    if apply is not None:
        kw["apply"] = sym.APPLY_INCREMENTAL if incremental else sym.APPLY_CUMULATIVE
    max_d2 = R.f32_max_d2(mcd)
    factor, rho = rule.get("factor", 0.0), rule.get("rho", 1.0)
    ref_kw = dict(factor=factor, rho=rho, max_d2=max_d2, min_ndot=mnd)
    masks = []
    with sym.Engine(**kw) as e, sym.Engine(**kw) as twin, sym.Engine(**kw) as o2o:
        for x in (e, twin, o2o):
            x.set_target(tgt, tgt_n)
            x.set_source(src, src_n)
        apply_rules(e, rule, one_to_one)
        o2o.set_one_to_one(True)
        assert (e.get_reciprocal(), e.one_to_one(), e.median_factor(), e.trim_fraction()) == (True, one_to_one, f32(factor), f32(rho))
        code, scale = 0, 1.0
        if loss:
            # a Huber scale that bites: the median |r| of the first pass's kept pairs, from the numpy rows
            twin.begin()
            idx0 = twin.correspondences()[0]
            p0, pn0 = R.moved(np.eye(4), src, src_n, m)
            k0 = RR.recip_pass(p0, pn0, tgt, tgt_n, idx0, src, np.eye(4), **ref_kw)["kept"]
            res = R.pass_terms(m, p0[k0], pn0[k0], tgt[idx0[k0]], tgt_n[idx0[k0]], np.zeros(3, f32))[1]
            scale = float(np.median(np.abs(res)))
            assert scale > 0
            code = sym.LOSS_HUBER
            e.set_robust_loss("huber", scale)
        it = e.begin()
        done = 0
        for k in range(steps + 1):
            t = "%s pass %d" % (tag, k)
            X = e.transform()
            if incremental:
                # the pass pairs the written-back cloud: its positions from the device, its pairs by the oracle's brute force
                p, pn = e.source()
                idx, d2 = R.nn_ref(p, tgt)
            else:
                twin.begin(guess=X)
                idx, d2 = twin.correspondences()
                p, pn = R.moved(X, src, src_n, m)
            ref = RR.recip_pass(p, pn, tgt, tgt_n, idx, src, X, **ref_kw)
            has = idx >= 0
            assert np.array_equal(d2[has], ref["d2"][has]), t
            nc, npop, kept, tau = e.rejection_state()
            nu, nr = e.reciprocal_state()
            print("%s: n_c %d n_u %d n_r %d kept %d tau %g" % (t, nc, nu, nr, kept, tau))
            assert (nc, nu, nr, kept) == (ref["n_c"], ref["n_u"], ref["n_r"], ref["n_kept"]), (t, nc, nu, nr, kept, ref["n_c"], ref["n_u"], ref["n_r"], ref["n_kept"])
            assert npop == nr, (t, npop, nr)                       # (the select's population)
            assert tau_bits(tau) == tau_bits(ref["tau"]), (t, tau, ref["tau"])
            if rho < 1:
                ts = e.trim_state()
                assert ts[:2] == (nr, kept) and tau_bits(ts[2]) == tau_bits(tau), (t, ts)
            S, M, n_kept = T.trimmed_record(m, p, pn, tgt, tgt_n, idx, ref["kept"], e.pivot(), code, scale)
            assert n_kept == kept
            R.assert_record(it["sums"], S, M, R.TOL_REC if code else R.TOL_EXACT, t)
            assert it["pairs"] == kept, (t, it["pairs"], kept)
            ie, _ = e.correspondences()
            assert np.array_equal(ie, np.where(ref["kept"], idx, -1)), (t, int((ie != np.where(ref["kept"], idx, -1)).sum()))
            # inside one-to-one's kept set of the same pass, on the device
            if not incremental:
                o2o.begin(guess=X)
                io = o2o.correspondences()[0]
                assert o2o.rejection_state()[1] == nu, t
                assert not ((ie >= 0) & (io < 0)).any(), t
            if k == 0 and bite:
                assert 0 < nr < nu <= nc, (t, nr, nu, nc)
                if factor > 0 or rho < 1:
                    assert 0 < kept < nr, (t, kept, nr)
                if mcd > 0 or mnd > -1:
                    assert ref["n_c"] < int(has.sum()), "the gates dropped nothing"
            masks.append(ref["kept"])
            done += 1
            if k == steps:
                break
            it = e.step(check=False)
            if it["status"] != 0:
                break
    return done, masks


GRID = [(m, c, r) for m in ("paper", "p2p", "plane", "gicp") for c in ("brute", "tree") for r in RULES]


@pytest.mark.parametrize("mode,corr,rule", GRID, ids=["%s-%s-%s" % g for g in GRID])
def test_every_pass(sym, cat, surf, mode, corr, rule):
    for name, d in (("cat", cat), ("surface", surf)):
        assert check_passes(sym, d, mode, corr, RULES[rule], tag=name)[0] == 4, name


@pytest.mark.parametrize("mode", ["paper", "plane"])
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_every_pass_with_a_huber_loss(sym, cat, surf, mode, corr):
    for name, d in (("cat", cat), ("surface", surf)):
        assert check_passes(sym, d, mode, corr, RULES["median2"], loss=True, tag=name)[0] == 4, name


@pytest.mark.parametrize("mode", ["paper", "p2p", "plane", "gicp"])
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_every_pass_with_both_gates(sym, cat, surf, mode, corr):
    """a gated pair claims nothing: a distance gate at the 0.8 quantile of the first pass's distances, and every third source normal
    reversed under min_normal_dot = 0 (trimming's recipe)"""
    for name, d0 in (("cat", cat), ("surface", surf)):
        d = dict(d0, src_n=d0["src_n"].copy())
        d["src_n"][::3] *= -1
        d2_0 = R.nn_ref(d["src"], d["tgt"])[1]
        mcd = float(np.sqrt(np.quantile(d2_0, 0.8)))
        assert check_passes(sym, d, mode, corr, RULES["median2"], False, mcd, 0.0, tag=name)[0] >= 2, name


@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_both_source_orders_keep_the_same_set(sym, cat, surf, corr):
    for name, d in (("cat", cat), ("surface", surf)):
        a = check_passes(sym, d, "plane", corr, RULES["alone"], tag=name + " sorted", sort_source=1)
        b = check_passes(sym, d, "plane", corr, RULES["alone"], tag=name + " unsorted", sort_source=0)
        assert a[0] == b[0] == 4
        assert np.array_equal(a[1][0], b[1][0])      # (later passes: the transforms may differ in the last bits of the sums' order)


@pytest.mark.parametrize("corr", ["brute", "tree"])
@pytest.mark.parametrize("apply", ["incremental", "cumulative"])
def test_both_apply_modes(sym, cat, corr, apply):
    """the reverse side never sees the written-back copy: the original source through the inverse of the cumulative transform"""
    assert check_passes(sym, cat, "paper", corr, RULES["median2"], tag=apply, apply=apply)[0] == 4


@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_one_to_one_on_top_changes_nothing(sym, cat, corr):
    assert check_passes(sym, cat, "plane", corr, RULES["median2"], tag="with one-to-one", one_to_one=True)[0] == 4
    its = []
    for on in (False, True):
        with sym.Engine(mode=sym.MODE_PLANE, corr=corr_code(sym, corr), max_iters=6, fixed_iters=1) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            e.set_reciprocal(True)
            e.set_one_to_one(on)
            its.append([e.begin()] + [e.step() for _ in range(3)] + [e.reciprocal_state(), e.rejection_state()[:3]])
    for a, b in zip(its[0][:4], its[1][:4]):
        assert np.asarray(a["sums"]).tobytes() == np.asarray(b["sums"]).tobytes()
    assert its[0][4:] == its[1][4:]


@pytest.mark.parametrize("n_s", [1, 255, 257, 2999])
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_ragged_sizes(sym, cat, corr, n_s):
    d = dict(src=cat["src"][:n_s], src_n=cat["src_n"][:n_s], tgt=cat["tgt"], tgt_n=cat["tgt_n"])
    # (one source point: it wins its target and is its own reverse neighbour -- nothing can bite)
    done = check_passes(sym, d, "paper", corr, RULES["median2"], tag="n_s=%d" % n_s, bite=n_s > 1)[0]
    assert done >= (1 if n_s == 1 else 4)
    # ... and a target smaller than the source
    d = dict(src=cat["src"], src_n=cat["src_n"], tgt=cat["tgt"][:1001], tgt_n=cat["tgt_n"][:1001])
    assert check_passes(sym, d, "paper", corr, RULES["alone"], tag="n_t=1001")[0] == 4


def test_color_mode(sym, oracle):
    """COLOR on its own fixture: the record of the kept set through the colour restatement"""
    import _color_ref as CR
    from symmicp import synth
    d = dict(synth.ridge_textured())
    d["tgt_g"] = sym.intensity_gradient(d["tgt"], d["tgt_n"], d["tgt_i"], 10)
    with sym.Engine(mode=sym.MODE_COLOR, corr=sym.CORR_TREE, max_iters=30, host_loop=1) as e:
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_target_intensity(d["tgt_i"], d["tgt_g"])
        e.set_source_intensity(d["src_i"])
        e.set_reciprocal(True)
        e.set_median_factor(2.0)
        it = e.begin()
        for k in range(3):
            X = e.transform()
            p, pn = oracle.apply(X, d["src"], True), oracle.apply(X, d["src_n"], False)
            pairs, rd = oracle.nn_brute(p, d["tgt"])
            ref = RR.recip_pass(p, pn, d["tgt"], d["tgt_n"], pairs, d["src"], X, factor=2.0)
            nc, npop, kept, tau = e.rejection_state()
            assert (nc, npop, kept, tau_bits(tau)) == (ref["n_c"], ref["n_r"], ref["n_kept"], tau_bits(ref["tau"])), k
            assert e.reciprocal_state() == (ref["n_u"], ref["n_r"]), k
            if k == 0:
                assert 0 < kept < npop < ref["n_u"] <= nc
            want = np.where(ref["kept"], pairs, -1)
            assert np.array_equal(e.correspondences()[0], want), k
            S, M, kept_mask = CR.color_record(p, pn, d["src_i"], d["tgt"], d["tgt_n"], d["tgt_g"], d["tgt_i"], want, e.pivot(), CR.LAMBDA_DEFAULT)
            assert np.array_equal(kept_mask, ref["kept"])
            gpu = np.asarray(it["sums"], np.float64)
            err = np.abs(gpu[:37] - S[:37])
            bad = np.nonzero(err > 1e-9 * np.maximum(M[:37], 1e-300))[0]           # (test_gpu_color.py's comparison)
            assert bad.size == 0, (k, [(int(b), gpu[b], S[b]) for b in bad[:6]])
            assert gpu[37] == S[37] and it["pairs"] == kept == int(ref["kept"].sum()), k
            it = e.step()


# ---- 3. behaviour and lifetime ------------------------------------------------------------------------------------------------------
def _align_with_log(sym, d, set_off, **kw):
    with sym.Engine(**kw) as e:
        if set_off:
            e.set_reciprocal(0)
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_loop_log(True)
        r = e.align()
        for call in (e.rejection_state, e.trim_state, e.reciprocal_state):
            with pytest.raises(sym.SymmIcpError) as x:
                call()
            assert x.value.status == sym.ERR_STATE
        # ... and nothing was allocated for it: no source index, no claim table
        assert e.reciprocal_info() == dict(index_valid=False, index_bytes=0, index_builds=0, table_words=0)
        return r, e.loop_log(), e.stats()


def test_off_is_bit_identical(sym, cat):
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1)
    ra, la, sa = _align_with_log(sym, cat, True, **kw)
    rb, lb, sb = _align_with_log(sym, cat, False, **kw)
    assert ra["status"] == rb["status"] == 0
    assert sa["loop_passes"] == sb["loop_passes"] > 0 and sa["passes"] == sb["passes"]
    assert ra["iters"] == rb["iters"] and ra["transform"].tobytes() == rb["transform"].tobytes()
    assert ra["diffs"].tobytes() == rb["diffs"].tobytes() and f32(ra["diff_final"]) == f32(rb["diff_final"])
    assert len(la) == len(lb) > 0
    for x, y in zip(la, lb):
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k
    # ... so are single passes, and a one-to-one context is what it was: switched on and off again, nothing stays behind
    recs = []
    for toggled in (True, False):
        with sym.Engine(**dict(kw, max_iters=4)) as e:
            e.set_target(cat["tgt"], cat["tgt_n"])
            e.set_source(cat["src"], cat["src_n"])
            e.set_one_to_one(True)
            if toggled:
                e.set_reciprocal(True)
                e.set_reciprocal(False)
            recs.append([e.begin()["sums"].copy()] + [e.step()["sums"].copy() for _ in range(2)] + [e.rejection_state()])
            with pytest.raises(sym.SymmIcpError):
                e.reciprocal_state()
            # (the claim table is the target's size, without the tail a reciprocal pass adds, and there is no source index)
            assert e.reciprocal_info() == dict(index_valid=False, index_bytes=0, index_builds=0, table_words=len(cat["tgt"]))
    for a, b in zip(*recs):
        assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def test_the_source_index_survives_the_target_and_the_read_only_entries(sym, cat, surf):
    kw = dict(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=8, fixed_iters=1)
    with sym.Engine(**kw) as e, sym.Engine(**kw) as t:
        for x in (e, t):
            x.set_target(cat["tgt"], cat["tgt_n"])
            x.set_source(cat["src"], cat["src_n"])
            x.set_reciprocal(True)
        assert e.reciprocal_info()["index_builds"] == 0 and not e.reciprocal_info()["index_valid"]      # (built by the first pass, not by the setter)
        assert np.array_equal(e.begin()["sums"], t.begin()["sums"])
        info0 = e.reciprocal_info()
        assert info0["index_valid"] and info0["index_builds"] == 1 and info0["index_bytes"] > 16 * len(cat["src"])
        assert info0["table_words"] > len(cat["tgt"])
        # everything that rewinds the target's arena, between two steps
        e.knn(surf["tgt"][:5000], 10)
        e.radius_search(surf["src"][:3000], 3.0 * surf["spacing"])
        e.fpfh(surf["tgt"][:3000], surf["tgt_n"][:3000], 5.0 * surf["spacing"])
        e.estimate_normals(surf["src"][:4000], 10)
        a, b = e.step(), t.step()
        assert np.array_equal(a["sums"], b["sums"]) and e.reciprocal_state() == t.reciprocal_state()
        assert e.reciprocal_info() == info0                          # not rebuilt
        # a new target (a larger one: the arena is reallocated), the same source: the index is still the source's
        X = e.transform()
        big = np.concatenate([cat["tgt"], cat["tgt"] + f32(1e-3)]), np.concatenate([cat["tgt_n"], cat["tgt_n"]])
        for x in (e, t):
            x.set_target(*big)
        t.set_source(cat["src"], cat["src_n"])                       # (the twin builds its index afresh)
        a, b = e.begin(guess=X), t.begin(guess=X)
        assert np.array_equal(a["sums"], b["sums"]) and e.reciprocal_state() == t.reciprocal_state()
        assert np.array_equal(e.correspondences()[0], t.correspondences()[0])
        for _ in range(2):
            e.step()
        info1 = e.reciprocal_info()
        assert info1["index_valid"] and info1["index_builds"] == 1 and info1["index_bytes"] == info0["index_bytes"]
        assert t.reciprocal_info()["index_builds"] == 2
        # a new source rebuilds it: the results are those of a context that never saw the old one
        half = cat["src"][::2] + f32(0.01), cat["src_n"][::2]
        e.set_source(*half)
        assert not e.reciprocal_info()["index_valid"] and e.reciprocal_info()["index_builds"] == 1
        with sym.Engine(**kw) as fresh:
            fresh.set_target(*big)
            fresh.set_source(*half)
            fresh.set_reciprocal(True)
            a, b = e.begin(), fresh.begin()
            assert np.array_equal(a["sums"], b["sums"]) and e.reciprocal_state() == fresh.reciprocal_state()
            p, pn = R.moved(np.eye(4), half[0], half[1], sym.MODE_PLANE)
            ref = RR.recip_pass(p, pn, big[0], big[1], R.nn_ref(p, big[0])[0], half[0], np.eye(4))
            assert e.reciprocal_state() == (ref["n_u"], ref["n_r"])
            assert np.array_equal(e.step()["sums"], fresh.step()["sums"])
            assert e.reciprocal_info()["index_builds"] == 2 and e.reciprocal_info()["index_valid"]      # once per set_source
            assert e.reciprocal_info()["index_bytes"] == info0["index_bytes"]                        # (the arena is reused: the new source is smaller)
            # switched off: the index stays (the next reciprocal pass finds it), and nothing more is built
            e.set_reciprocal(False)
            e.step()
            e.set_reciprocal(True)
            e.step()
            assert e.reciprocal_info()["index_builds"] == 2


def test_setters_act_at_the_next_pass_and_align_is_the_host_loop(sym, cat):
    n = len(cat["src"])
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=12, fixed_iters=1)
    with sym.Engine(**kw) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        assert e.get_reciprocal() is False
        it = e.begin()
        assert it["pairs"] == n
        with pytest.raises(sym.SymmIcpError) as x:
            e.reciprocal_state()
        assert x.value.status == sym.ERR_STATE
        e.set_reciprocal(True)
        with pytest.raises(sym.SymmIcpError):
            e.reciprocal_state()                                 # (nothing happens before the next pass)
        it = e.step()
        nu, nr = e.reciprocal_state()
        nc, npop, kept, tau = e.rejection_state()
        assert nc == n and 0 < nr == npop == kept == it["pairs"] < nu < n and np.isposinf(tau)
        assert int((e.correspondences()[0] >= 0).sum()) == nr
        e.set_reciprocal(False)
        assert e.reciprocal_state() == (nu, nr)
        it = e.step()
        assert it["pairs"] == n
        for call in (e.reciprocal_state, e.rejection_state):
            with pytest.raises(sym.SymmIcpError) as x:
                call()
            assert x.value.status == sym.ERR_STATE
    with sym.Engine(**kw) as e, sym.Engine(**kw) as s:
        for x in (e, s):
            x.set_target(cat["tgt"], cat["tgt_n"])
            x.set_source(cat["src"], cat["src_n"])
            x.set_reciprocal(True)
        e.set_loop_log(True)
        r = e.align()
        assert r["status"] == 0 and r["iters"] == 12
        assert e.stats()["loop_passes"] == 0 and len(e.loop_log()) == 0
        its = [s.begin()] + [s.step() for _ in range(12)]
        assert np.array_equal(r["diffs"], np.array([it["diff"] for it in its[:12]], f32))
        assert r["transform"].tobytes() == s.transform().tobytes()
        assert e.reciprocal_state() == s.reciprocal_state()


def _refused(sym, call, status):
    with pytest.raises(sym.SymmIcpError) as x:
        call()
    assert x.value.status == status, x.value


def test_refusals(sym, cat):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_reciprocal(True)
        _refused(sym, lambda: e.set_config(mode=sym.MODE_QUIRKS), sym.ERR_ARG)
        e.cfg.mode = sym.MODE_PAPER
        _refused(sym, lambda: e.set_config(corr=sym.CORR_IDENTITY), sym.ERR_ARG)
        e.cfg.corr = sym.CORR_TREE
        assert e.get_reciprocal() is True
        _refused(sym, e.reciprocal_state, sym.ERR_STATE)          # no pass yet
        _refused(sym, lambda: e.comm_init_rank(2, 1, None), sym.ERR_STATE)
        _refused(sym, lambda: e.comm_init_shm(2, 0, "symmicp_recip_test_%d" % os.getpid()), sym.ERR_STATE)
        assert e.local_count() == 0
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        _refused(sym, e.reciprocal_state, sym.ERR_STATE)
        e.begin()
        assert e.reciprocal_state()[0] > 0
    with sym.Engine(mode=sym.MODE_QUIRKS, corr=sym.CORR_TREE) as e:
        _refused(sym, lambda: e.set_reciprocal(True), sym.ERR_ARG)
        assert e.get_reciprocal() is False
        e.set_reciprocal(False)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_IDENTITY) as e:
        _refused(sym, lambda: e.set_reciprocal(True), sym.ERR_ARG)
        assert e.get_reciprocal() is False
        e.set_reciprocal(False)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.comm_init_rank(2, 0, None)
        _refused(sym, lambda: e.set_reciprocal(True), sym.ERR_STATE)
        assert e.get_reciprocal() is False
        e.set_reciprocal(False)


# ---- 4. what it is for ----------------------------------------------------------------------------------------------------------------
# The bound is the project's bound for this pair (tests/test_gpu_trim.py): 0.1 sample spacings.  The fp64 reference loop ends at 0.00455
# (reciprocal) and 0.00369 (with the median factor 2) (tests/test_recip_ref.py), over 20 times below it, and the unrejected loop ends 400
# times above it, so a rule that rejects nothing cannot pass.  Measured on an MI355X: Engine 0.00455 and 0.00369, both MyICP classes 0.00455
# (also with two voxel levels), the driver with its own normals 0.00503; no rejection 42.536.
BOUND = 0.1


def test_partial_overlap_through_engine(sym, surf):
    out = {}
    for name in ("plain", "reciprocal", "reciprocal+median2"):
        with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1) as e:
            e.set_target(surf["tgt"], surf["tgt_n"])
            e.set_source(surf["src"], surf["src_n"])
            if name != "plain":
                e.set_reciprocal(True)
            if name.endswith("median2"):
                e.set_median_factor(2.0)
            r = e.align()
            assert r["iters"] == 30
            out[name] = T.rms_spacings(r["transform"], surf)
            if name != "plain":
                assert r["status"] == 0 and e.stats()["loop_passes"] == 0
    print("rms from the truth in spacings: %s" % ", ".join("%s %.5f" % kv for kv in out.items()))
    assert out["plain"] > 10.0, out
    assert out["reciprocal"] <= BOUND and out["reciprocal+median2"] <= BOUND, out


def levels_for(surf):
    return [(2.0 * surf["spacing"], 15, 0.0), (0.0, 30, 0.0)]


@pytest.mark.parametrize("levels", [False, True])
def test_partial_overlap_through_python_myicp(sym, surf, levels):
    icp = sym.MyICP(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1, verbose=False)
    icp.setInputSource(surf["src"], surf["src_n"])
    icp.setInputTarget(surf["tgt"], surf["tgt_n"])
    icp.setReciprocalCorrespondences(True)
    if levels:
        icp.setVoxelLevels(levels_for(surf))
    r = icp.align()
    assert r["status"] == 0
    rms = T.rms_spacings(icp.getFinalTransformation(), surf)
    print("MyICP reciprocal%s: %.5f spacings" % (" with two levels" if levels else "", rms))
    assert rms <= BOUND, rms


def test_partial_overlap_through_cpp_myicp(sym, surf, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_recip")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for name, arr in (("src", surf["src"]), ("src_n", surf["src_n"]), ("tgt", surf["tgt"]), ("tgt_n", surf["tgt_n"]),
                      ("levels", np.array(levels_for(surf), f32))):
        np.ascontiguousarray(arr, f32).tofile(tmp_path / (name + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rms = {k: T.rms_spacings(np.fromfile(tmp_path / ("out_%s.f32" % k), f32).reshape(4, 4), surf) for k in ("plain", "recip", "median", "levels")}
    print("C++ MyICP: %s" % rms)
    assert rms["plain"] > 10.0, rms
    for k in ("recip", "median", "levels"):
        assert rms[k] <= BOUND, rms


def test_partial_overlap_through_the_driver(sym, surf, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    sym.pcd_write(str(tmp_path / "a.pcd"), surf["src"], None, binary=True)
    sym.pcd_write(str(tmp_path / "b.pcd"), surf["tgt"], None, binary=True)
    args = ["--mode", "plane", "--corr", "tree", "--iters", "30", "--threshold", "0"]
    rms = {}
    for name, extra in (("plain", []), ("reciprocal", ["--reciprocal"])):
        r = subprocess.run([exe] + args + extra + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")
        k = out.index("Result transform:")
        X = np.array([[float(v) for v in out[k + 1 + i].split()] for i in range(4)])
        rms[name] = T.rms_spacings(X, surf)
    print("icp_align: %s" % rms)
    assert rms["plain"] > 10.0 and rms["reciprocal"] <= BOUND, rms
    for bad in (["--mode", "quirks", "--corr", "tree", "--reciprocal"], ["--mode", "plane", "--corr", "identity", "--reciprocal"]):
        assert subprocess.run([exe] + bad + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True).returncode == 64, bad
