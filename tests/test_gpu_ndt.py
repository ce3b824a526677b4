"""GPU tests of SYMMICP_MODE_NDT's pass and loop (k_pass_ndt, engine_loop.cpp) on synth.c4_surface(4000) at resolution 0.1, for the
neighbourhoods 7 and 1.  The restatement (tests/_ndt_ref.py) is fed the map the device itself reports through symmicp_get_ndt_map, so the
pass is judged apart from the last bits of the map's Jacobi (tests/test_gpu_ndt_map.py judges those).  Records are held to
_record_ref.assert_record at TOL_REC, the bar of the weighted records, and the item count exactly."""
import os
import subprocess

import numpy as np
import pytest

import _ndt_ref as R
from _record_ref import TOL_REC, assert_record, f32_max_d2, xf_rows
from conftest import ROOT

pytestmark = pytest.mark.gpu

F = np.float32
RES = 0.1
END_ROT, END_TRANS = 0.2, 2e-3      # about twice the restatement's own ends (0.0904 deg / 8.4e-4 and 0.0584 deg / 5.0e-4): the objective
#                                     jumps when a point crosses a cell face, and the restatement's end moved by 0.011 deg between starts
NEIGHBORS = (7, 1)


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def c4():
    from symmicp import synth
    return synth.c4_surface(4000)


def device_map(e):
    m = e.get_ndt_map()
    m["inv"] = F(1) / F(e.get_ndt()["resolution"])
    return m


def ndt_engine(sym, c4, neighbors, src=None, resolution=RES, **cfg):
    e = sym.Engine(mode=sym.MODE_NDT, **cfg)
    e.set_ndt(resolution=resolution, neighbors=neighbors)
    e.set_target(c4["tgt"], None)
    e.set_source(c4["src"] if src is None else src, None)
    return e


@pytest.fixture(scope="module")
def maps(sym, c4):
    """the device's map of the target (it does not depend on the neighbourhood) and the pivot, read once and left unchanged"""
    with ndt_engine(sym, c4, 7) as e:
        return dict(map=device_map(e), pivot=e.pivot().copy())


def check_record(sums, maps, X, src, neighbors, tag, max_corr_dist=0.0):
    S, M, cnt = R.record(maps["map"], X, src, maps["pivot"], neighbors, max_corr_dist=max_corr_dist)
    S[37] = cnt
    assert_record(sums, S, M, TOL_REC, tag)
    assert sums[37] == cnt, (tag, sums[37], cnt)
    return S, cnt


@pytest.mark.parametrize("neighbors", NEIGHBORS)
def test_begin_record_for_three_guesses(sym, c4, maps, neighbors):
    far = np.eye(4, dtype=F)
    far[0, 3] = 10.0
    with ndt_engine(sym, c4, neighbors) as e:
        assert np.array_equal(e.pivot(), maps["pivot"])
        with pytest.raises(sym.SymmIcpError) as err:          # no pass yet
            e.ndt_state()
        assert err.value.status == sym.ERR_STATE
        for name, X in (("identity", np.eye(4, dtype=F)), ("truth", c4["truth"].astype(F))):
            it = e.begin(X)
            S, cnt = check_record(it["sums"], maps, X, c4["src"], neighbors, "%s/%d" % (name, neighbors))
            assert it["pairs"] == cnt and cnt > 3000
            score, items = e.ndt_state()
            assert items == cnt and score == -R.gauss(float(F(0.55)))[0] * it["sums"][34]
        assert e.begin(None)["sums"][37] == (18498 if neighbors == 7 else 3533)      # the restatement's first-pass items (tests/test_ndt_ref.py)
        # a guess that moves every point out of the map: an empty record is no error, the step on it is degenerate
        it = e.begin(far)
        assert not np.any(it["sums"]) and it["pairs"] == 0
        assert e.ndt_state() == (0.0, 0)
        st = e.step(check=False)
        assert st["status"] == sym.ERR_DEGENERATE
        assert e.begin(None)["sums"][37] > 0                  # the context still works


@pytest.mark.parametrize("neighbors", NEIGHBORS)
@pytest.mark.parametrize("sort_source", [0, 1])
def test_source_subsets(sym, c4, maps, neighbors, sort_source):
    """ragged sizes: one lane, a wave less and more than full, a block less and more than full, many blocks with a ragged tail"""
    X = c4["truth"].astype(F)
    with sym.Engine(mode=sym.MODE_NDT, sort_source=sort_source) as e:
        e.set_ndt(resolution=RES, neighbors=neighbors)
        e.set_target(c4["tgt"], None)
        for n in (1, 63, 65, 255, 257, 3997):
            src = c4["src"][7:7 + n] if n < 3997 else c4["src"][:n]
            e.set_source(src, None)
            for name, G in (("identity", None), ("truth", X)):
                it = e.begin(G)
                check_record(it["sums"], maps, np.eye(4, dtype=F) if G is None else G, src, neighbors, "n=%d %s sort=%d" % (n, name, sort_source))


@pytest.mark.parametrize("neighbors", NEIGHBORS)
def test_max_corr_dist_keeps_an_item_at_the_bound(sym, c4, maps, neighbors):
    X = np.eye(4, dtype=F)
    y = xf_rows(X, c4["src"], 1.0)
    pt, row, _ = R.items(maps["map"], y, neighbors)
    _, _, _, d2, _ = R.item_terms(maps["map"], y, pt, row, maps["pivot"], R.pass_h())
    # a bound m near 0.05 whose fp32 square IS an item's d2: that item sits at the bound and is kept (the gate drops d2 > max_d2 only)
    m = None
    for k in np.argsort(np.abs(np.sqrt(d2.astype(np.float64)) - 0.05)):
        c = F(np.sqrt(np.float64(d2[k])))
        for cand in (c, np.nextafter(c, F(0)), np.nextafter(c, F(1))):
            if f32_max_d2(cand) == d2[k]:
                m = cand
                break
        if m is not None:
            break
    assert m is not None and abs(float(m) - 0.05) < 5e-3
    n_at = int(np.sum(d2 == f32_max_d2(m)))
    n_below = int(np.sum(d2 < f32_max_d2(m)))
    assert n_at >= 1 and n_below + n_at < len(d2)
    with ndt_engine(sym, c4, neighbors, max_corr_dist=float(m)) as e:
        it = e.begin(None)
        _, cnt = check_record(it["sums"], maps, X, c4["src"], neighbors, "gate/%d" % neighbors, max_corr_dist=float(m))
        assert cnt == n_below + n_at
    with ndt_engine(sym, c4, neighbors, max_corr_dist=0.05) as e:
        it = e.begin(None)
        check_record(it["sums"], maps, X, c4["src"], neighbors, "gate 0.05/%d" % neighbors, max_corr_dist=0.05)


@pytest.fixture(scope="module")
def stepped(sym, c4, maps):
    """per neighbourhood: 30 steps by hand -- every pass's record, increment and transform -- run once and shared"""
    out = {}
    for nb in NEIGHBORS:
        with ndt_engine(sym, c4, nb, max_iters=30, fixed_iters=1) as e:
            its = [e.begin(None)]
            Xs = [e.transform().copy()]
            for _ in range(30):
                its.append(e.step())
                Xs.append(e.transform().copy())
            out[nb] = dict(its=its, Xs=Xs, corr=e.correspondences())
    return out


@pytest.mark.parametrize("neighbors", NEIGHBORS)
def test_every_step_of_the_loop(sym, c4, maps, stepped, neighbors):
    its, Xs = stepped[neighbors]["its"], stepped[neighbors]["Xs"]
    for k in range(1, 13):
        check_record(its[k]["sums"], maps, Xs[k], c4["src"], neighbors, "step %d/%d" % (k, neighbors))
        st, _, _, _, _, rc, Xi = sym.solve(sym.MODE_NDT, its[k - 1]["sums"], maps["pivot"])
        assert st == sym.OK
        assert np.array_equal(its[k]["increment"], Xi), k
        assert its[k]["iter"] == k and its[k]["rcond"] == F(rc)
    assert its[12]["sums"][34] > its[0]["sums"][34]                       # the last pass's sum of weights exceeds the first's
    rot, tr = R.pose_error(Xs[30], c4["truth"])
    assert rot < END_ROT and tr < END_TRANS, (rot, tr)
    print("NDT end state, neighbors %d: %.4f deg, %.2e; sum w %.1f -> %.1f" % (neighbors, rot, tr, its[0]["sums"][34], its[30]["sums"][34]))


@pytest.mark.parametrize("neighbors", NEIGHBORS)
def test_align_equals_the_stepped_run_and_repeats(sym, c4, stepped, neighbors):
    runs = []
    for _ in range(2):
        with ndt_engine(sym, c4, neighbors, max_iters=30, fixed_iters=1) as e:
            r = e.align(None, check=True)
            assert r["iters"] == 30
            runs.append((r["transform"].copy(), e.begin(r["transform"])["sums"].copy()))
    assert np.array_equal(runs[0][0], stepped[neighbors]["Xs"][30])
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])      # two runs: identical bits


@pytest.mark.parametrize("neighbors", NEIGHBORS)
def test_correspondences(sym, c4, maps, stepped, neighbors):
    idx, d2 = stepped[neighbors]["corr"]
    ridx, rd2 = R.correspondences(maps["map"], stepped[neighbors]["Xs"][30], c4["src"], maps["pivot"])
    assert np.array_equal(idx, ridx) and np.array_equal(d2.view(np.uint32), rd2.view(np.uint32))
    assert (idx < 0).any() and (idx >= 0).sum() > 3000 and np.all(d2[idx < 0] == 0)
    # sort_source off: the same answer
    with ndt_engine(sym, c4, neighbors, sort_source=0) as e:
        e.begin(stepped[neighbors]["Xs"][30])
        i2, q2 = e.correspondences()
    assert np.array_equal(i2, ridx) and np.array_equal(q2.view(np.uint32), rd2.view(np.uint32))


@pytest.mark.parametrize("neighbors", NEIGHBORS)
def test_units_scale_out(sym, c4, neighbors):
    """the cloud x 4 at resolution 0.4 (exact in fp32): the same items, the same weights -- d2 of the Gauss constants carries no unit"""
    with ndt_engine(sym, c4, neighbors) as e:
        a = e.begin(None)["sums"]
    big = dict(tgt=c4["tgt"] * F(4), src=c4["src"] * F(4))
    with ndt_engine(sym, big, neighbors, resolution=0.4) as e:
        b = e.begin(None)["sums"]
    assert a[37] == b[37]
    assert abs(a[34] - b[34]) <= TOL_REC * a[34]


def _expect(sym, status, fn, *args, **kw):
    with pytest.raises(sym.SymmIcpError) as err:
        fn(*args, **kw)
    assert err.value.status == status, (fn.__name__, args, kw, err.value.status)


def test_refusals_leave_the_context_working(sym, c4, maps):
    setters = (("set_robust_loss", ("huber", 0.01), ("none",)), ("set_trim_fraction", (0.5,), (1.0,)), ("set_one_to_one", (True,), (False,)),
               ("set_median_factor", (2.0,), (0.0,)), ("set_reciprocal", (True,), (False,)))
    with ndt_engine(sym, c4, 7) as e:
        ref = e.begin(None)["sums"]
        for name, on, off in setters:
            _expect(sym, sym.ERR_ARG, getattr(e, name), *on)
            getattr(e, name)(*off)                                         # switching it off is no error
            assert np.array_equal(e.begin(None)["sums"], ref), name
        for kw, back in ((dict(min_normal_dot=0.5), dict(min_normal_dot=-2.0)), (dict(apply=sym.APPLY_INCREMENTAL), dict(apply=sym.APPLY_DEFAULT))):
            _expect(sym, sym.ERR_ARG, e.set_config, **kw)
            e.set_config(**back)
            assert np.array_equal(e.begin(None)["sums"], ref), kw
        # out of NDT while a target is set
        _expect(sym, sym.ERR_STATE, e.set_config, mode=sym.MODE_PLANE)
        e.set_config(mode=sym.MODE_NDT)
        _expect(sym, sym.ERR_STATE, e.comm_init_rank, 2, 0, None)          # (after set_source: refused anyway)
        assert np.array_equal(e.begin(None)["sums"], ref)
        with pytest.raises(sym.SymmIcpError):
            e.source()                                                     # the moved source exists with the incremental apply only
        assert np.array_equal(e.begin(None)["sums"], ref)
    # the other way round: the option first, then the mode
    for name, on, off in setters:
        with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE) as e:
            getattr(e, name)(*on)
            _expect(sym, sym.ERR_ARG, e.set_config, mode=sym.MODE_NDT)
            e.set_config(mode=sym.MODE_PLANE)
            getattr(e, name)(*off)
            e.set_config(mode=sym.MODE_NDT)
            e.set_ndt(resolution=RES)
            e.set_target(c4["tgt"], None)
            e.set_source(c4["src"], None)
            assert np.array_equal(e.begin(None)["sums"], ref), name
    # sharding, both ways round
    with sym.Engine(mode=sym.MODE_NDT) as e:
        _expect(sym, sym.ERR_STATE, e.comm_init_rank, 2, 0, None)
        e.set_ndt(resolution=RES)
        e.set_target(c4["tgt"], None)
        e.set_source(c4["src"], None)
        assert np.array_equal(e.begin(None)["sums"], ref)
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE) as e:
        e.comm_init_rank(2, 0, None)
        _expect(sym, sym.ERR_STATE, e.set_config, mode=sym.MODE_NDT)
        e.set_config(mode=sym.MODE_PLANE)
    # into NDT while a target is set
    with sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE, max_iters=2, fixed_iters=1) as e:
        e.set_target(c4["tgt"], c4["tgt_n"])
        _expect(sym, sym.ERR_STATE, e.set_config, mode=sym.MODE_NDT)
        e.set_config(mode=sym.MODE_PLANE)
        e.set_source(c4["src"], None)
        assert e.align(None, check=True)["iters"] == 2
        _expect(sym, sym.ERR_ARG, e.set_target, c4["tgt"], None)           # normals stay required outside NDT
    # the batched entry has no NDT form
    probs = [(0, 100, 0, 100)]
    _expect(sym, sym.ERR_ARG, sym.batch_align, c4["src"][:100], None, c4["tgt"][:100], c4["tgt_n"][:100], probs, mode=sym.MODE_NDT)
    with sym.Engine(mode=sym.MODE_NDT) as e:
        st, _ = e.batch_align_raw(c4["src"][:100], None, c4["tgt"][:100], c4["tgt_n"][:100], probs, None, sym.batch_config(mode=sym.MODE_NDT))[:2]
        assert st == sym.ERR_ARG
        e.set_ndt(resolution=RES)
        e.set_target(c4["tgt"], None)
        e.set_source(c4["src"], None)
        assert np.array_equal(e.begin(None)["sums"], ref)


def test_evaluate_on_an_ndt_context(sym, c4):
    """symmicp_evaluate builds a temporary index, as on every non-TREE context: the result is the one-shot entry's"""
    with ndt_engine(sym, c4, 7, max_iters=5, fixed_iters=1) as e:
        r = e.align(None, check=True)
        ev = e.evaluate(r["transform"], max_dist=0.05)
        again = e.begin(r["transform"])["sums"]
    one = sym.evaluate_registration(c4["src"], c4["tgt"], r["transform"], max_dist=0.05)
    assert ev["raw"] == one["raw"] and ev["inliers"] > 3000
    assert again[37] > 0


# ---- coarse-to-fine, MyICP (Python and C++), the command line ---------------------------------------------------------------------------
LEVELS = ((0.4, 10), (0.2, 10), (0.1, 10))


def far_start(c4):
    """12 degrees about (1, -2, 3) and t = (0.08, -0.06, 0.04) in front of the truth"""
    from symmicp import synth
    D = synth.rigid4(synth.rotation(12.0, (1, -2, 3)), np.array([0.08, -0.06, 0.04]))
    return (c4["truth"] @ D).astype(F)


@pytest.fixture(scope="module")
def by_hand(sym, c4):
    """the levels as the calls they stand for: set_ndt, then an alignment from the level before -- once, shared"""
    X = far_start(c4)
    per = []
    with sym.Engine(mode=sym.MODE_NDT, verbose=0) as e:
        e.set_ndt(resolution=LEVELS[0][0])
        e.set_target(c4["tgt"], None)
        e.set_source(c4["src"], None)
        for k, (res, iters) in enumerate(LEVELS):
            if k:
                e.set_ndt(resolution=res)
            e.set_config(max_iters=iters)
            r = e.align(X, check=True)
            X = r["transform"]
            per.append(r)
    return per


def test_python_myicp_levels_equal_the_hand_made_sequence(sym, c4, by_hand):
    icp = sym.MyICP(mode=sym.MODE_NDT, verbose=False)
    icp.setInputSource(c4["src"])
    icp.setInputTarget(c4["tgt"])
    icp.setNdt(LEVELS[0][0])
    icp.setNdtLevels(LEVELS)
    r = icp.align(far_start(c4))
    assert r["status"] == sym.OK and len(icp.level_results) == 3
    for a, b in zip(icp.level_results, by_hand):
        assert a["iters"] == b["iters"] == 10 and np.array_equal(a["transform"], b["transform"])
    assert np.array_equal(icp.getFinalTransformation(), by_hand[-1]["transform"])
    assert icp.normals_src is None and icp.normals_tgt is None            # both normals pre-steps were skipped
    rot0, tr0 = R.pose_error(far_start(c4), c4["truth"])
    rot, tr = R.pose_error(icp.getFinalTransformation(), c4["truth"])
    assert abs(rot0 - 12.0) < 1e-3 and rot < END_ROT and tr < END_TRANS, (rot, tr)
    print("NDT levels from 12 deg: %.4f deg, %.2e" % (rot, tr))
    # a single level at 0.1 from the same start does not get there (what the levels are for)
    icp.setNdtLevels([])
    icp.setNdt(0.1)
    icp._cfg["max_iters"] = 20
    one = icp.align(far_start(c4))
    assert R.pose_error(one["transform"], c4["truth"])[0] > 2.0
    # what the mode refuses
    icp.setVoxelLevels([(0.05, 5, 0.0)])
    with pytest.raises(sym.SymmIcpError) as err:
        icp.align()
    assert err.value.status == sym.ERR_ARG
    icp.setVoxelLevels([])
    icp.setRobustLoss("huber", 0.01)
    with pytest.raises(sym.SymmIcpError) as err:
        icp.align()
    assert err.value.status == sym.ERR_ARG


def test_cpp_myicp_levels_equal_the_hand_made_sequence(sym, c4, by_hand, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "test_myicp_ndt")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    for fname, arr in (("src", c4["src"]), ("tgt", c4["tgt"]), ("guess", far_start(c4)), ("levels", np.array(LEVELS))):
        np.ascontiguousarray(arr, F).tofile(tmp_path / (fname + ".f32"))
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    out = np.fromfile(tmp_path / "out.f32", F).reshape(4, 4)
    per = np.fromfile(tmp_path / "levels_out.f32", F).reshape(3, 4, 4)
    assert np.array_equal(np.fromfile(tmp_path / "iters.f32", F), F([10, 10, 10]))
    for k in range(3):
        assert np.array_equal(per[k], by_hand[k]["transform"]), k
    assert np.array_equal(out, by_hand[-1]["transform"])
    # the single alignment it ran last: neighbours 1, resolution 0.1, 12 fixed-length iterations from the identity
    with ndt_engine(sym, c4, 1, max_iters=12, diff_threshold=0.0) as e:
        ref = e.align(None, check=True)
    assert np.array_equal(np.fromfile(tmp_path / "out_single.f32", F).reshape(4, 4), ref["transform"])


def test_command_line(sym, c4, by_hand, tmp_path):
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    a, b, out = str(tmp_path / "src.pcd"), str(tmp_path / "tgt.pcd"), str(tmp_path / "out.pcd")
    sym.pcd_write(a, c4["src"], None, binary=True)
    sym.pcd_write(b, c4["tgt"], None, binary=True)
    base = [exe, "--mode", "ndt"]
    r = subprocess.run(base + ["--ndt-resolution", "0.1", "--iters", "12", "--threshold", "0", "--out", out, a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "iters#12" in r.stdout and "Result transform:" in r.stdout
    with ndt_engine(sym, c4, 7, max_iters=12, diff_threshold=0.0) as e:
        ref = e.align(None, check=True)
    moved, _ = sym.pcd_read(out)
    X = ref["transform"].astype(np.float64)
    assert np.abs(moved - (c4["src"].astype(np.float64) @ X[:3, :3].T + X[:3, 3])).max() < 1e-5
    lv = []
    for res, it in LEVELS:
        lv += ["--ndt-level", "%g:%d" % (res, it)]
    r = subprocess.run(base + ["--ndt-neighbors", "1", "--ndt-min-points", "8"] + lv + [a, b], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "NDT level 3/3: resolution 0.1, 10 iterations" in r.stdout
    for bad in (["--ndt-resolution", "0"], ["--ndt-resolution", "x"], ["--ndt-resolution", "0.1", "--ndt-neighbors", "3"],
                ["--ndt-resolution", "0.1", "--ndt-min-points", "2"], ["--ndt-level", "0.1"], ["--ndt-level", "0:5"], [],
                ["--ndt-resolution", "0.1", "--trim", "0.5"], ["--ndt-resolution", "0.1", "--scale", "0.05:5"],
                ["--ndt-resolution", "0.1", "--loss", "huber", "--loss-scale", "0.1"]):
        assert subprocess.run(base + bad + [a, b], capture_output=True, text=True, timeout=60).returncode == 64, bad
    assert subprocess.run([exe, "--mode", "plane", "--ndt-resolution", "0.1", a, b], capture_output=True, text=True, timeout=60).returncode == 64
