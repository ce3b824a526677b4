"""What the device does with a record: its solve (solve_core.h compiled for gfx950), its conditioning gate, the composition and the
stop rules of the device-driven loop (k_reduce_solve), checked against the host solve (symmicp.solve), the exact reference
(_solve_ref.py) and an fp32 replay of mat4_mul.

  * probe (symmicp_ctx_solve_probe, one thread per record) with the host's exact conditioning: status, pbar, qbar, a, t and rcond are
    the host's bits -- they come only from fp64 +, *, /, sqrt, frexp and ldexp, correctly rounded on both sides; out16 within
    OUT16_ULPS (ocml's sinf / cosf / atanf are within 2 ulp, sqrtf is correctly rounded; glibc's within 1: 3 ulp apart on sin, cos
    and the angle, carried through two rotations and the translations' sums of three products);
  * probe with the device's lower bound: the same a, t bits, and it accepts nothing the host rejects (the Kahan record included);
  * one solve-only launch of k_reduce_solve (symmicp_ctx_loop_solve): its increment is the probe's, X = mat4_mul(increment, X_in) to
    the bit, Xapply follows the apply mode, and the stop rules hold at their edges;
  * in situ: the log of device-driven passes (symmicp_set_loop_log) of real alignments, replayed."""
import numpy as np
import pytest

import _solve_ref as R
from _record_ref import MODE_QUIRKS, MODE_PAPER, MODE_PLANE

pytestmark = pytest.mark.gpu

MODES = (MODE_PAPER, MODE_PLANE, MODE_QUIRKS)
OUT16_ULPS = 32          # per entry, in units of 2^-24 x (1 + |pbar| + |qbar| + |t|) (the translations' scale)
f32 = np.float32


@pytest.fixture(scope="module")
def sym():
    import symmicp
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine() as e:
        yield e


@pytest.fixture(scope="module")
def records(cat):
    z = np.zeros(3, f32)
    out = [(nm, m, S, z) for nm, S in R.synthetic_records() for m in MODES]
    out += [(nm, m, S, pv) for nm, m, S, pv in R.real_records(cat)]
    out += [(nm, m, S, z) for nm, S in R.edge_records() for m in MODES]
    return out


def bits(x):
    return np.ascontiguousarray(np.asarray(x, f32)).view(np.uint32)


def same_bits(a, b):
    """bit-equal, every NaN counted equal to any NaN (payloads are not part of the contract)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(np.where(na, 0, a)), bits(np.where(nb, 0, b)))


def out16_close(X, Y, pb, qb, t):
    scale = 1.0 + float(np.nansum(np.abs(pb)) + np.nansum(np.abs(qb)) + np.nansum(np.abs(t)))      # (PLANE leaves qbar out of the increment)
    return np.all(np.abs(np.asarray(X, np.float64) - np.asarray(Y, np.float64)) <= OUT16_ULPS * 2.0 ** -24 * scale)


def probe_all(eng, records, exact_rc):
    res = []
    for m in MODES:
        for pv_key in set(tuple(pv) for _, mm, _, pv in records if mm == m):
            sel = [i for i, (_, mm, _, pv) in enumerate(records) if mm == m and tuple(pv) == pv_key]
            o = eng.solve_probe(m, np.stack([records[i][2] for i in sel]), exact_rc, pivot=np.array(pv_key, f32))
            for j, i in enumerate(sel):
                res.append((i, {k: v[j] for k, v in o.items()}))
    res.sort(key=lambda r: r[0])
    return [r for _, r in res]


@pytest.fixture(scope="module")
def probes(sym, eng, records):
    host = [sym.solve(m, S, pv) for _, m, S, pv in records]
    return host, probe_all(eng, records, True), probe_all(eng, records, False)


# ---- 1. the device's solve against the host's -------------------------------------------------------------------------------
def test_probe_exact_form_matches_host_bits(records, probes):
    host, ex, _ = probes
    n_ok = 0
    for (nm, m, S, _), h, p in zip(records, host, ex):
        st, pb, qb, a, t, rc, X = h
        assert p["status"] == st, (nm, m, p["status"], st)
        for k, v in (("pbar", pb), ("qbar", qb), ("a", a), ("t", t), ("rcond", np.float32(rc))):
            assert same_bits(p[k], v), (nm, m, k, p[k], v)
        if st == 0:
            assert out16_close(p["out16"], X, pb, qb, t), (nm, m, p["out16"] - X)
            n_ok += 1
    assert n_ok > 200


def test_probe_bound_form_solves_to_the_same_bits(records, probes):
    _, ex, lb = probes
    for (nm, m, _, _), p, q in zip(records, ex, lb):
        for k in ("pbar", "qbar", "a", "t"):
            assert same_bits(p[k], q[k]), (nm, m, k)
        if p["status"] == 0 and q["status"] == 0:
            assert same_bits(p["out16"], q["out16"]), (nm, m)


def test_device_gate_implies_host_ok(records, probes):
    """device accepts => host OK; on the parent commit the Kahan record failed here (pivot ratio 2.4e-4 against an exact 1.4e-16)"""
    host, _, lb = probes
    acc = 0
    for (nm, m, S, _), h, q in zip(records, host, lb):
        if q["status"] == 0:
            assert h[0] == 0, (nm, m, "device accepts what the host flags", q["rcond"], h[5])
            acc += 1
        if q["status"] == 0 and q["rcond"] > R.LOOP_GATE:
            ex = R.reference(m, S, a_solved=h[3] if m == MODE_QUIRKS else None)
            assert ex["rc"] > R.LOOP_GATE and q["rcond"] <= ex["rc"], (nm, m, q["rcond"], ex["rc"])
    assert acc > 200
    k = [i for i, r in enumerate(records) if r[0] == "kahan" and r[1] in (MODE_PAPER, MODE_PLANE)]
    assert k and all(lb[i]["status"] == 3 and lb[i]["rcond"] <= R.LOOP_GATE for i in k), [(lb[i]["status"], lb[i]["rcond"]) for i in k]


# ---- 2. one solve-only launch of k_reduce_solve -----------------------------------------------------------------------------
def rigid(seed):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    if np.linalg.det(Q) < 0:
        Q[:, 0] = -Q[:, 0]
    X = np.eye(4, dtype=f32)
    X[:3, :3] = Q
    X[:3, 3] = rng.standard_normal(3) * 3
    return X


@pytest.fixture(scope="module")
def loop_cases(records, probes):
    """accepted records of every mode with a bound above the loop's gate: real passes and a few synthetic ones"""
    _, _, lb = probes
    out = []
    for i, ((nm, m, S, pv), q) in enumerate(zip(records, lb)):
        if q["status"] == 0 and q["rcond"] > R.LOOP_GATE and (nm.startswith(("cat_first_off0_u0", "cat_conv_off0_u0", "c4", "c5", "syn_haar_-1.0", "syn_kahan_-2.0"))):
            out.append((nm, m, S, pv, q))
    assert {m for _, m, _, _, _ in out} == set(MODES)
    return out


@pytest.mark.parametrize("incremental", [0, 1])
def test_loop_solve_composes_the_probe_increment(eng, loop_cases, incremental):
    for j, (nm, m, S, pv, q) in enumerate(loop_cases):
        X_in = rigid(j)
        o = eng.loop_solve(m, S, X_in=X_in, pivot=pv, diff_threshold=0.0, max_iters=10, iters=3, incremental=incremental)
        assert (o["stop"], o["reason"], o["iters"], o["small_step"]) == (0, 0, 3, 0), (nm, m, o)
        assert o["ring_status"] == 0 and o["ring_solved"] == 1
        assert same_bits(o["ring_increment"], q["out16"]), (nm, m)
        assert same_bits(o["ring_rcond"], q["rcond"]), (nm, m)
        Xn = R.mat4_mul(q["out16"], X_in)
        assert same_bits(o["X"], Xn) and same_bits(o["ring_X"], Xn), (nm, m)
        assert same_bits(o["Xapply"], (q["out16"] if incremental else Xn)[:3]), (nm, m, incremental)
        p = eng.solve_probe(m, S[None], False, pivot=pv, X_in=X_in[None])
        assert same_bits(p["X_out"][0], Xn)


def test_loop_solve_hands_the_kahan_record_back(eng):
    for m in (MODE_PAPER, MODE_PLANE):
        X_in = rigid(5)
        o = eng.loop_solve(m, R.kahan_record(), X_in=X_in, diff_threshold=0.0, max_iters=10, iters=2)
        assert (o["stop"], o["reason"], o["iters"]) == (1, 3, 2), o                   # LOOP_HOST_SOLVE
        assert o["ring_solved"] == -1 and np.isnan(o["ring_increment"]).all()        # nothing written
        assert same_bits(o["X"], X_in)


def test_loop_solve_gate_follows_the_bound(eng, records, probes):
    """LOOP_HOST_SOLVE exactly where the probe's status or bound says: the synthetic spectrum sweep crosses the 1e-6 gate"""
    _, _, lb = probes
    n = {0: 0, 3: 0}
    for (nm, m, S, pv), q in zip(records, lb):
        if not nm.startswith("syn_haar"):
            continue
        o = eng.loop_solve(m, S, pivot=pv, diff_threshold=0.0, max_iters=10, iters=0)
        go = q["status"] == 0 and q["rcond"] > R.LOOP_GATE
        assert o["reason"] == (0 if go else 3), (nm, m, q["status"], q["rcond"], o)
        n[o["reason"]] += 1
    assert n[0] > 10 and n[3] > 10, n


def _case(loop_cases, mode=MODE_PAPER):
    return next(c for c in loop_cases if c[1] == mode and c[0].startswith("cat_conv"))


def test_stop_rule_diff_at_threshold(eng, loop_cases):
    """myicp.cpp:123: go on while diff > threshold (float compare of the record's slot 33)"""
    nm, m, S, pv, q = _case(loop_cases)
    d = f32(S[33])
    for thr, go in ((np.nextafter(d, f32(-np.inf)), True), (d, False), (np.nextafter(d, f32(np.inf)), False)):
        o = eng.loop_solve(m, S, pivot=pv, diff_threshold=float(thr), max_iters=10, iters=1)
        assert o["reason"] == (0 if go else 1) and o["stop"] == (0 if go else 1), (thr, d, o)
        o = eng.loop_solve(m, S, pivot=pv, diff_threshold=float(thr), fixed_iters=1, max_iters=10, iters=1)
        assert o["reason"] == 0, (thr, o)                                         # fixed_iters: the diff does not stop it


def test_stop_rule_max_iters(eng, loop_cases):
    nm, m, S, pv, q = _case(loop_cases)
    for it, go in ((8, True), (9, True), (10, False), (11, False)):
        for fixed in (0, 1):
            o = eng.loop_solve(m, S, pivot=pv, diff_threshold=0.0, fixed_iters=fixed, max_iters=10, iters=it)
            assert o["reason"] == (0 if go else 1), (it, fixed, o)


def test_stop_rule_small_step(eng, loop_cases):
    """the increment rule: angle acos((tr - 1) / 2) and translation norm (fp64 from the fp32 increment) below eps_rotation and
    eps_translation sets small_step; a small_step carried in stops the next call (LOOP_DONE); fixed_iters disables the rule"""
    for nm, m, S, pv, q in loop_cases[:6]:
        Xi = q["out16"].astype(np.float64)
        ang = np.arccos(np.clip((Xi[0, 0] + Xi[1, 1] + Xi[2, 2] - 1.0) * 0.5, -1.0, 1.0))
        tn = np.sqrt(Xi[0, 3] ** 2 + Xi[1, 3] ** 2 + Xi[2, 3] ** 2)
        if not (ang > 1e-30 and tn > 1e-30):
            continue
        up_r, up_t = f32(ang), f32(tn)
        up_r = up_r if up_r > ang else np.nextafter(up_r, f32(np.inf))
        up_t = up_t if up_t > tn else np.nextafter(up_t, f32(np.inf))
        dn_r, dn_t = np.nextafter(up_r, f32(0)), np.nextafter(up_t, f32(0))
        for er, et, small in ((up_r, up_t, 1), (dn_r, up_t, 0), (up_r, dn_t, 0), (np.nextafter(up_r, f32(np.inf)), up_t, 1)):
            o = eng.loop_solve(m, S, pivot=pv, diff_threshold=0.0, max_iters=10, iters=1, eps_rotation=float(er), eps_translation=float(et))
            assert o["reason"] == 0 and o["small_step"] == small, (nm, m, er, et, ang, tn, o)
            o2 = eng.loop_solve(m, S, pivot=pv, diff_threshold=0.0, max_iters=10, iters=2, small_step=o["small_step"],
                                eps_rotation=float(er), eps_translation=float(et))
            assert o2["reason"] == (1 if small else 0), (nm, m, o2)
            o3 = eng.loop_solve(m, S, pivot=pv, diff_threshold=0.0, fixed_iters=1, max_iters=10, iters=1, eps_rotation=float(er), eps_translation=float(et))
            assert o3["small_step"] == 0


# ---- 3. in situ: the log of device-driven passes ----------------------------------------------------------------------------
def _runs():
    return ["cat_paper_cum", "cat_paper_inc", "cat_plane_cum", "cat_plane_inc", "cat_quirks_cum", "cat_quirks_inc",
            "c4_paper", "c4_paper_huber", "c5_stragglers"]


@pytest.fixture(scope="module")
def c4_200k():
    from symmicp import synth
    return synth.c4_surface(200000)


@pytest.mark.parametrize("case", _runs())
def test_logged_device_passes_replay(sym, cat, c4_200k, case):
    from symmicp import synth
    kw = {}
    loss = None
    if case.startswith("cat"):
        d = dict(src=cat["src"], src_n=cat["src_n"], tgt=cat["tgt"], tgt_n=cat["tgt_n"])
        mode = {"paper": sym.MODE_PAPER, "plane": sym.MODE_PLANE, "quirks": sym.MODE_QUIRKS}[case.split("_")[1]]
        kw.update(mode=mode, corr=sym.CORR_IDENTITY, max_iters=12, fixed_iters=1,
                  apply=sym.APPLY_INCREMENTAL if case.endswith("inc") else sym.APPLY_CUMULATIVE)
    elif case.startswith("c4"):
        d = c4_200k
        kw.update(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=25, diff_threshold=0.0, eps_rotation=2e-7, eps_translation=2e-7)
        if case.endswith("huber"):
            loss = ("huber", 0.01)
    else:
        d = synth.c5_scan(64 * 16384)
        kw.update(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=40, fixed_iters=1)
    mode = kw["mode"]
    with sym.Engine(**kw) as e:
        if loss:
            e.set_robust_loss(*loss)
        e.set_target(d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        e.set_loop_log(True)
        r = e.align()
        log = e.loop_log()
        st = e.stats()
        pivot = np.zeros(3, f32) if mode == sym.MODE_QUIRKS else e.pivot()
    assert r["status"] == 0
    assert st["loop_passes"] > 0 and log
    batches = sorted({x["batch"] for x in log})
    assert sum(len([x for x in log if x["batch"] == b]) - 1 for b in batches) == st["loop_passes"]
    solved = 0
    for b in batches:
        ent = [x for x in log if x["batch"] == b]
        for k, x in enumerate(ent):
            if x["solved"]:
                hst, pb, qb, a, t, rc, X = sym.solve(mode, x["sums"], pivot)
                assert hst == 0, (case, x["iter"])
                assert out16_close(x["increment"], X, pb, qb, t), (case, x["iter"], x["increment"] - X)
                assert x["rcond"] > R.LOOP_GATE
                if k > 0:
                    assert same_bits(x["X"], R.mat4_mul(x["increment"], ent[k - 1]["X"])), (case, x["iter"])
                solved += 1
        # why the batch stopped, replayed on its last entry
        last = ent[-1]
        if not last["solved"]:
            it = last["iter"]
            diff = f32(last["sums"][33])
            go = (kw.get("fixed_iters", 0) or diff > f32(kw.get("diff_threshold", 1.0))) and it < kw["max_iters"]
            small = False
            if len(ent) >= 2 and ent[-2]["solved"] and kw.get("eps_rotation", 0) > 0 and not kw.get("fixed_iters", 0):
                Xi = ent[-2]["increment"].astype(np.float64)
                ang = np.arccos(np.clip((Xi[0, 0] + Xi[1, 1] + Xi[2, 2] - 1.0) * 0.5, -1, 1))
                tn = np.sqrt((Xi[:3, 3] ** 2).sum())
                small = ang < f32(kw["eps_rotation"]) and tn < f32(kw["eps_translation"])
            if last["reason"] == sym.LOOP_DONE:
                assert small or not go, (case, it, diff)
            elif last["reason"] == sym.LOOP_HOST_SOLVE:
                assert go and not small, (case, it)                  # the rule let it go on; the gate sent it back
    assert solved > 0
