"""Trimmed ICP on the GPU (run with -m gpu on a real MI355X): symmicp_set_trim_fraction, the exact radix select behind it, and what
it is for.

  1. the select alone (symmicp_ctx_select_probe) against np.partition, exactly;
  2. every pass of a trimmed context against the numpy restatement (tests/_trim_ref.py): trim state (n_c, kept, tau's bits), the
     record, the pair count and the reported pairs -- modes x pairings x fractions, with a Huber loss, with both gates, ragged sizes;
  3. the zero threshold (tau = 0 keeps the pairs at distance 0 only, not all of them);
  4. off means off: fraction 1 is bit for bit a context that never heard of trimming, a fraction below 1 stays in the host loop;
  5. the refusals;
  6. the partial-overlap pair through Engine, MyICP (Python and C++), the command-line driver and a two-level run.
The pairs of a pass come from a twin context without trimming driven by the same transforms (its pairs and distances are held to
the oracle's brute force by test_gpu_pass_matrix.py)."""
import math
import os
import subprocess

import numpy as np
import pytest

import _record_ref as R
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
    return {"quirks": sym.MODE_QUIRKS, "paper": sym.MODE_PAPER, "p2p": sym.MODE_P2P, "plane": sym.MODE_PLANE, "gicp": sym.MODE_GICP}[mode]


def corr_code(sym, corr):
    return {"identity": sym.CORR_IDENTITY, "brute": sym.CORR_BRUTE, "tree": sym.CORR_TREE}[corr]


# ---- 1. the select ----------------------------------------------------------------------------------------------------------------
SELECT_SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4097, 1_000_003, 8_388_608]
DISTS = ["full", "equal", "two", "ascending", "descending", "top22", "d2bits"]


def select_keys(dist, n, rng):
    if dist == "full":
        return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if dist == "equal":
        return np.full(n, 0x3F800000, np.uint32)
    if dist == "two":
        return np.where(rng.random(n) < 0.3, np.uint32(0x00000007), np.uint32(0xFFFFFFFF)).astype(np.uint32)
    if dist in ("ascending", "descending"):
        a = (np.arange(n, dtype=np.uint64) * np.uint64(max(1, (2 ** 32 - 1) // n))).astype(np.uint32)
        return a if dist == "ascending" else a[::-1].copy()
    if dist == "top22":
        return (np.uint32(0xABCDE400) | rng.integers(0, 1024, n, dtype=np.uint64).astype(np.uint32)).astype(np.uint32)
    # fp32 squared distances as a pass sees them: a smooth bulk, exact zeros and denormals among them
    d2 = (rng.random(n) ** 2).astype(f32) * f32(0.01)
    d2[rng.random(n) < 0.05] = 0.0
    sub = rng.random(n) < 0.05
    d2[sub] = (rng.integers(1, 2 ** 23, int(sub.sum()), dtype=np.uint64).astype(np.uint32)).view(f32)      # denormals
    assert (d2 >= 0).all()
    return d2.view(np.uint32).copy()


def select_ranks(n):
    return sorted({1, n, min(n, 2), max(1, n // 2), max(1, n // 3 + 1), max(1, (7 * n) // 8), max(1, n - 1)})


@pytest.mark.parametrize("n", SELECT_SIZES)
def test_select_probe_equals_partition(sym, cat, n):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        e.set_trim_fraction(0.5)
        it0 = e.begin()
        before = (e.correspondences(), e.certificates(), e.index_info(), e.trim_state(), e.trim_fraction())
        for di, dist in enumerate(DISTS):
            keys = select_keys(dist, n, np.random.default_rng(1000 * di + n % 997))
            srt = np.sort(keys) if n <= 4097 else None
            for k in select_ranks(n):
                kth, nle = e.select_probe(keys, k)
                want = int(srt[k - 1]) if srt is not None else int(np.partition(keys, k - 1)[k - 1])
                assert kth == want, (dist, n, k, hex(kth), hex(want))
                assert nle == int((keys <= np.uint32(want)).sum()), (dist, n, k, nle)
        after = (e.correspondences(), e.certificates(), e.index_info(), e.trim_state(), e.trim_fraction())
        for a, b in zip(before[:2], after[:2]):
            assert all(np.array_equal(u, v) for u, v in zip(a, b))
        assert str(before[2]) == str(after[2]) and before[3] == after[3] and before[4] == after[4] == 0.5
        # ... and the alignment goes on as one that was never probed
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as t:
            t.set_target(cat["tgt"], cat["tgt_n"])
            t.set_source(cat["src"], cat["src_n"])
            t.set_trim_fraction(0.5)
            assert np.array_equal(t.begin()["sums"], it0["sums"])
            assert np.array_equal(t.step()["sums"], e.step()["sums"])


def test_select_probe_refuses_bad_ranks(sym):
    with sym.Engine() as e:
        keys = np.arange(10, dtype=np.uint32)
        for k in (0, 11):
            with pytest.raises(sym.SymmIcpError) as x:
                e.select_probe(keys, k)
            assert x.value.status == sym.ERR_ARG
        with pytest.raises(sym.SymmIcpError):
            e.select_probe(keys[:0], 1)


# ---- 2. every pass ----------------------------------------------------------------------------------------------------------------
def check_passes(sym, d, mode, corr, rho, loss=False, mcd=0.0, mnd=-2.0, steps=3, tag=""):
    """begin and `steps` steps of a trimmed context against the numpy restatement; -> the number of passes checked"""
    m = mode_code(sym, mode)
    src, src_n, tgt, tgt_n = d["src"], d["src_n"], d["tgt"], d["tgt_n"]
    kw = dict(mode=m, corr=corr_code(sym, corr), max_iters=steps + 2, fixed_iters=1, max_corr_dist=mcd, min_normal_dot=mnd)
    max_d2 = R.f32_max_d2(mcd)
    identity = corr == "identity"
    with sym.Engine(**kw) as e, sym.Engine(**kw) as twin:
        for x in (e, twin):
            x.set_target(tgt, tgt_n)
            x.set_source(src, src_n)
        e.set_trim_fraction(rho)
        assert e.trim_fraction() == f32(rho)
        code, scale = 0, 1.0
        if loss:
            # a Huber scale that bites: the median |r| of the first pass's kept pairs, from the numpy rows
            twin.begin()
            idx0 = None if identity else twin.correspondences()[0]
            p0, pn0 = R.moved(np.eye(4), src, src_n, m)
            r0 = T.trim_pass(p0, pn0, tgt, tgt_n, idx0, rho, max_d2, mnd)
            j0 = np.arange(len(src)) if identity else idx0
            k0 = r0["kept"]
            res = R.pass_terms(m, p0[k0], pn0[k0], tgt[j0[k0]], tgt_n[j0[k0]], np.zeros(3, f32))[1]
            scale = float(np.median(np.abs(res)))
            assert scale > 0
            code = sym.LOSS_HUBER
            e.set_robust_loss("huber", scale)
        it = e.begin()
        done = 0
        for k in range(steps + 1):
            t = "%s pass %d" % (tag, k)
            X = e.transform()
            twin.begin(guess=X)
            idx, d2 = twin.correspondences()
            p, pn = R.moved(X, src, src_n, m)
            if identity:
                assert np.array_equal(idx, np.arange(len(src)))
            ref = T.trim_pass(p, pn, tgt, tgt_n, idx, rho, max_d2, mnd)
            has = idx >= 0
            assert np.array_equal(d2[has], ref["d2"][has]), t
            nc, kept, tau = e.trim_state()
            assert (nc, kept) == (ref["n_c"], int(ref["kept"].sum())), (t, nc, kept, ref["n_c"], int(ref["kept"].sum()))
            assert f32(tau).view(np.uint32) == f32(ref["tau"]).view(np.uint32), (t, tau, ref["tau"])
            assert kept >= ref["k"] >= 1
            S, M, n_kept = T.trimmed_record(m, p, pn, tgt, tgt_n, idx, ref["kept"], e.pivot(), code, scale)
            assert n_kept == kept
            R.assert_record(it["sums"], S, M, R.TOL_REC if code else R.TOL_EXACT, t)
            assert it["pairs"] == kept, (t, it["pairs"], kept)
            if code and k == 0:
                assert 0.0 < S[34] < kept
            ie, _ = e.correspondences()
            assert np.array_equal(ie, np.where(ref["kept"], idx, -1)), (t, int((ie != np.where(ref["kept"], idx, -1)).sum()))
            if k == 0:
                assert 0 < kept < len(src) or len(src) == 1
                if mcd > 0 or mnd > -1:
                    assert ref["n_c"] < int(has.sum()), "the gates dropped nothing"
            done += 1
            if k == steps:
                break
            it = e.step(check=False)
            if it["status"] != 0:
                break
        return done


GRID = [(m, c, r) for m in ("paper", "p2p", "plane", "gicp") for c in ("identity", "brute", "tree") for r in (0.25, 0.5, 0.9)]


@pytest.mark.parametrize("mode,corr,rho", GRID, ids=["%s-%s-%g" % g for g in GRID])
@pytest.mark.parametrize("loss", ["none", "huber"])
def test_every_pass(sym, cat, surf, mode, corr, rho, loss):
    for name, d in (("cat", cat), ("surface", surf)):
        assert check_passes(sym, d, mode, corr, rho, loss == "huber", tag=name) == 4, name


@pytest.mark.parametrize("mode", ["paper", "p2p", "plane", "gicp"])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_every_pass_with_both_gates(sym, cat, surf, mode, corr):
    """the candidates are the gated pairs: a distance gate at the 0.8 quantile of the first pass's distances, and every third source
    normal reversed under min_normal_dot = 0"""
    for name, d0 in (("cat", cat), ("surface", surf)):
        d = dict(d0, src_n=d0["src_n"].copy())
        d["src_n"][::3] *= -1
        d2_0 = R.dist2(d["src"], d["tgt"]) if corr == "identity" else R.nn_ref(d["src"], d["tgt"])[1]
        mcd = float(np.sqrt(np.quantile(d2_0, 0.8)))
        assert check_passes(sym, d, mode, corr, 0.5, False, mcd, 0.0, tag=name) >= 2, name


@pytest.mark.parametrize("n_s", [1, 255, 257])
@pytest.mark.parametrize("corr", ["identity", "brute", "tree"])
def test_ragged_sizes(sym, cat, corr, n_s):
    n_t = n_s if corr == "identity" else len(cat["tgt"])
    d = dict(src=cat["src"][:n_s], src_n=cat["src_n"][:n_s], tgt=cat["tgt"][:n_t], tgt_n=cat["tgt_n"][:n_t])
    done = check_passes(sym, d, "paper", corr, 0.5, tag="n_s=%d" % n_s)
    assert done >= (1 if n_s == 1 else 4)         # (one pair solves nothing: the step after the first pass is degenerate)


# ---- 3. zero threshold ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1000, 1002])
def test_zero_threshold_keeps_the_coincident_half_only(sym, n):
    rng = np.random.default_rng(5)
    tgt = rng.random((n, 3)).astype(f32)
    nrm = rng.normal(size=(n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    src = tgt.copy()
    src[n // 2:, 0] += f32(1.0)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_IDENTITY, max_iters=3, fixed_iters=1) as e:
        e.set_target(tgt, nrm)
        e.set_source(src, nrm)
        e.set_trim_fraction(0.5)
        it = e.begin()
        nc, kept, tau = e.trim_state()
        assert (nc, kept) == (n, n // 2) and f32(tau).view(np.uint32) == 0
        first = np.arange(n) < n // 2
        S, M, cnt = T.trimmed_record(sym.MODE_PAPER, src, nrm, tgt, nrm, None, first, e.pivot())
        assert cnt == n // 2 and it["pairs"] == n // 2 and it["sums"][36] == 0.0 and it["sums"][33] == 0.0
        R.assert_record(it["sums"], S, M, R.TOL_EXACT, "zero threshold")
        assert np.array_equal(e.correspondences()[0], np.where(first, np.arange(n), -1))


# ---- 4. off means off ---------------------------------------------------------------------------------------------------------------
def _align_with_log(sym, d, set_one, **kw):
    with sym.Engine(**kw) as e:
        if set_one:
            e.set_trim_fraction(1.0)
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_loop_log(True)
        r = e.align()
        with pytest.raises(sym.SymmIcpError) as x:
            e.trim_state()
        assert x.value.status == sym.ERR_STATE
        return r, e.loop_log(), e.stats()


@pytest.mark.parametrize("data", ["cat", "cube100k"])
def test_fraction_one_is_bit_identical(sym, cat, data):
    from symmicp import synth
    d = cat if data == "cat" else synth.c3_uniform(100_000)
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1)
    ra, la, sa = _align_with_log(sym, d, True, **kw)
    rb, lb, sb = _align_with_log(sym, d, False, **kw)
    assert ra["status"] == rb["status"] == 0
    assert sa["loop_passes"] > 0 and sb["loop_passes"] > 0
    assert sa["loop_passes"] == sb["loop_passes"] and sa["passes"] == sb["passes"]
    assert ra["iters"] == rb["iters"] and ra["transform"].tobytes() == rb["transform"].tobytes()
    assert ra["diffs"].tobytes() == rb["diffs"].tobytes() and f32(ra["diff_final"]) == f32(rb["diff_final"])
    assert len(la) == len(lb) > 0
    for x, y in zip(la, lb):
        assert x.keys() == y.keys()
        for k in x:
            assert np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes(), k


def test_trimmed_align_is_the_host_loop(sym, cat):
    kw = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=12, fixed_iters=1)
    with sym.Engine(**kw) as e, sym.Engine(**kw) as s:
        for x in (e, s):
            x.set_target(cat["tgt"], cat["tgt_n"])
            x.set_source(cat["src"], cat["src_n"])
            x.set_trim_fraction(0.5)
        r = e.align()
        assert r["status"] == 0 and r["iters"] == 12
        assert e.stats()["loop_passes"] == 0
        its = [s.begin()] + [s.step() for _ in range(12)]
        assert np.array_equal(r["diffs"], np.array([it["diff"] for it in its[:12]], f32))
        assert f32(r["diff_final"]) == f32(its[12]["diff"])
        assert r["transform"].tobytes() == s.transform().tobytes()
        assert e.trim_state() == s.trim_state()


def test_fraction_changes_at_the_next_pass(sym, cat):
    n = len(cat["src"])
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=10, fixed_iters=1) as e:
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        e.set_trim_fraction(0.5)
        it = e.begin()
        nc, kept, _ = e.trim_state()
        assert nc == n and T.trim_k(0.5, n) <= kept == it["pairs"] < T.trim_k(0.5, n) + 8
        e.set_trim_fraction(0.25)
        assert e.trim_state()[1] == kept                      # (nothing happens before the next pass)
        it = e.step()
        nc, kept, _ = e.trim_state()
        assert nc == n and T.trim_k(0.25, n) <= kept == it["pairs"] < T.trim_k(0.25, n) + 8
        e.set_trim_fraction(1.0)
        it = e.step()
        assert it["pairs"] == n
        with pytest.raises(sym.SymmIcpError) as x:
            e.trim_state()
        assert x.value.status == sym.ERR_STATE
        assert (e.correspondences()[0] >= 0).all()
        e.set_trim_fraction(0.5)
        it = e.step()
        assert e.trim_state()[1] == it["pairs"] < n


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------------
def _refused(sym, call, status):
    with pytest.raises(sym.SymmIcpError) as x:
        call()
    assert x.value.status == status, x.value


def test_refusals(sym, cat):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_IDENTITY) as e:
        assert e.trim_fraction() == 1.0
        e.set_trim_fraction(0.75)
        for bad in (0.0, -0.5, 1.5, float("nan"), float("inf"), -float("inf")):
            _refused(sym, lambda: e.set_trim_fraction(bad), sym.ERR_ARG)
            assert e.trim_fraction() == 0.75
        # a trimming context cannot become QUIRKS ...
        _refused(sym, lambda: e.set_config(mode=sym.MODE_QUIRKS), sym.ERR_ARG)
        e.cfg.mode = sym.MODE_PAPER
        _refused(sym, e.trim_state, sym.ERR_STATE)               # no pass yet
        e.set_target(cat["tgt"], cat["tgt_n"])
        e.set_source(cat["src"], cat["src_n"])
        _refused(sym, e.trim_state, sym.ERR_STATE)
        e.begin()
        assert e.trim_state()[0] == len(cat["src"])
        e.set_trim_fraction(1.0)
        e.begin()
        _refused(sym, e.trim_state, sym.ERR_STATE)               # that pass was not trimmed
    # ... and a QUIRKS context takes no fraction below 1
    with sym.Engine(mode=sym.MODE_QUIRKS, corr=sym.CORR_IDENTITY) as e:
        _refused(sym, lambda: e.set_trim_fraction(0.5), sym.ERR_ARG)
        assert e.trim_fraction() == 1.0
        e.set_trim_fraction(1.0)
    # sharded contexts: both orders
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.comm_init_rank(2, 0, None)
        _refused(sym, lambda: e.set_trim_fraction(0.5), sym.ERR_STATE)
        assert e.trim_fraction() == 1.0
        e.set_trim_fraction(1.0)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        e.set_trim_fraction(0.5)
        _refused(sym, lambda: e.comm_init_rank(2, 1, None), sym.ERR_STATE)
        _refused(sym, lambda: e.comm_init_shm(2, 0, "symmicp_trim_test_%d" % os.getpid()), sym.ERR_STATE)
        assert e.local_count() == 0 and e.trim_fraction() == 0.5


# ---- 6. what it is for --------------------------------------------------------------------------------------------------------------
# The bound: the fp64 reference alone ends 0.006 spacings from the truth (tests/test_trim_ref.py); 0.1 leaves fp32 some 16x that,
# and sits 400x below where the untrimmed loop ends, so a trim that does not trim cannot pass.
BOUND = 0.1


def test_partial_overlap_through_engine(sym, surf):
    out = {}
    for rho in (1.0, 0.5):
        with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1) as e:
            e.set_target(surf["tgt"], surf["tgt_n"])
            e.set_source(surf["src"], surf["src_n"])
            if rho < 1:
                e.set_trim_fraction(rho)
            r = e.align()
            assert r["iters"] == 30
            out[rho] = T.rms_spacings(r["transform"], surf)
            if rho < 1:
                assert r["status"] == 0 and e.stats()["loop_passes"] == 0
    print("rms from the truth in spacings: untrimmed %.3f, rho = 0.5 %.5f" % (out[1.0], out[0.5]))
    assert out[1.0] > 10.0, out
    assert out[0.5] <= BOUND, out


def _myicp(sym, surf, levels=None):
    icp = sym.MyICP(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=30, fixed_iters=1, verbose=False)
    icp.setInputSource(surf["src"], surf["src_n"])
    icp.setInputTarget(surf["tgt"], surf["tgt_n"])
    icp.setTrimFraction(0.5)
    if levels:
        icp.setVoxelLevels(levels)
    r = icp.align()
    assert r["status"] == 0
    return T.rms_spacings(icp.getFinalTransformation(), surf)


def levels_for(surf):
    return [(2.0 * surf["spacing"], 15, 0.0), (0.0, 30, 0.0)]


def test_partial_overlap_through_python_myicp(sym, surf):
    rms = _myicp(sym, surf)
    print("MyICP.setTrimFraction(0.5): %.5f spacings" % rms)
    assert rms <= BOUND, rms


def test_partial_overlap_through_two_voxel_levels(sym, surf):
    rms = _myicp(sym, surf, levels_for(surf))
    print("two voxel levels, trimmed: %.5f spacings" % rms)
    assert rms <= BOUND, rms


def test_partial_overlap_through_cpp_myicp(sym, surf, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_trim")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for name, arr in (("src", surf["src"]), ("src_n", surf["src_n"]), ("tgt", surf["tgt"]), ("tgt_n", surf["tgt_n"]),
                      ("levels", np.array(levels_for(surf), f32))):
        np.ascontiguousarray(arr, f32).tofile(tmp_path / (name + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rms = {k: T.rms_spacings(np.fromfile(tmp_path / ("out_%s.f32" % k), f32).reshape(4, 4), surf) for k in ("plain", "trim", "levels")}
    print("C++ MyICP: %s" % rms)
    assert rms["plain"] > 10.0, rms
    assert rms["trim"] <= BOUND and rms["levels"] <= BOUND, rms


def test_partial_overlap_through_the_driver(sym, surf, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    sym.pcd_write(str(tmp_path / "a.pcd"), surf["src"], None, binary=True)
    sym.pcd_write(str(tmp_path / "b.pcd"), surf["tgt"], None, binary=True)
    args = ["--mode", "plane", "--corr", "tree", "--iters", "30", "--threshold", "0"]
    rms = {}
    for name, extra in (("plain", []), ("trim", ["--trim", "0.5"])):
        r = subprocess.run([exe] + args + extra + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out = r.stdout.split("\n")
        k = out.index("Result transform:")
        X = np.array([[float(v) for v in out[k + 1 + i].split()] for i in range(4)])
        rms[name] = T.rms_spacings(X, surf)
    print("icp_align: %s" % rms)
    assert rms["plain"] > 10.0 and rms["trim"] <= BOUND, rms
    # --trim needs a fraction in (0, 1] and a mode other than quirks
    for bad in (["--trim", "0"], ["--trim", "1.5"], ["--trim", "x"], ["--mode", "quirks", "--trim", "0.5"]):
        assert subprocess.run([exe, "--corr", "tree"] + bad + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True).returncode == 64, bad
