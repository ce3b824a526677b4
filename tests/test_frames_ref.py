"""CPU: what the GPU frame tests of the rejectors and of colored ICP assert, proved first on the numpy restatements, and what their
fixtures carry (tests/_frame_cases.py).  No GPU.

  1. units: for s = 2^-10 and 2^10 the restatements of a trimmed, a rejecting, a reciprocal and a COLOR pass, run on clouds x s with
     the length settings x s (max_corr_dist, the Huber scale; COLOR: the intensities too), return the same nearest neighbours, the
     same candidate, population and kept sets, tau with the bits of fl32(tau s^2) and a record equal to _frames.scale_record bit for bit
     (COLOR's record has PLANE's shape: the non-P2P dims).  The fp64 gradient is homogeneous: g(s x, n, s I) has g(x, n, I)'s bits,
     g(s x, n, I) is g / s exactly, and the degenerate rows are the same.
  2. range: the smallest non-zero and the largest candidate d2 of each fixture stay normal and finite fp32 under both units.
  3. the shifted fixtures: every (fixture, offset, rejection) the GPU tests run bites on its first pass, and the exact ties in d2 it
     carries are counted.  Measured (first pass, candidates that share their d2 bits with another / members of the select's population
     at its rank, largest over the rejections / targets claimed at equal smallest d2):
         cat      1e2: 0 / 1 / 0      1e3: 6 / 1 / 0      1e4: 477 / 1 / 1      3e5: 3372 / 51 / 200
         surface  1e2: 0 / 1 / 0      1e3: 76 / 1 / 0     3e5: 7932 / 303 / 575
     So at 1e2 extents there is no tie to assert (a d2 is the sum of three squares of some 1e3 quanta each: millions of values for
     thousands of candidates), at 1e3 and 1e4 there are ties among the candidates but no select of a first pass meets one at its
     rank and one claim in all (the cat's at 1e4) is decided by the row.  Those offsets are kept and held to what is true of them; the two frames of _frame_cases.TIE_OFFSETS are the ones in which
     `kept = k0 - rank + bins[j]` and the claim's row tie-break decide, and that is asserted of them here."""
import numpy as np
import pytest

import _color_ref as CR
import _frame_cases as F
import _record_ref as R
import _reject_ref as J
import _trim_ref as T
from _frames import scale_record

f32 = np.float32
MODES = {"paper": R.MODE_PAPER, "p2p": R.MODE_P2P, "plane": R.MODE_PLANE}


@pytest.fixture(scope="module")
def pairs(cat):
    return {"cat": dict(src=cat["src"], src_n=cat["src_n"], tgt=cat["tgt"], tgt_n=cat["tgt_n"]), "surface": F.surface()}


@pytest.fixture(scope="module")
def ridge():
    d = F.ridge_ragged()
    rows = CR.knn_rows(d["tgt"], 10)
    return dict(d, rows=rows, tgt_g=CR.gradient(d["tgt"], d["tgt_n"], d["tgt_i"], rows)[0].astype(f32))


def tau_bits(x):
    return int(f32(x).view(np.uint32))


# ---- 1. units ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", F.SCALE_EXPONENTS)
@pytest.mark.parametrize("name", ["cat", "surface"])
def test_restatements_scale_with_the_unit(pairs, name, k):
    s = 2.0 ** k
    f = f32(s)
    d0 = pairs[name]
    g0 = F.flipped(d0)
    mcd = f32(F.gate_distance(g0))
    checked = 0
    for X0 in (np.eye(4, dtype=f32), F.nudge(d0)):
        X1 = F.scaled_transform(X0, s)
        for gated, a in ((False, d0), (True, g0)):
            b = F.scaled(a, s)
            gates0 = dict(max_d2=R.f32_max_d2(mcd), min_ndot=F.MIN_NDOT) if gated else {}
            gates1 = dict(max_d2=R.f32_max_d2(mcd * f), min_ndot=F.MIN_NDOT) if gated else {}
            i0 = R.nn_ref(R.xf_rows(X0, a["src"], 1.0), a["tgt"])[0]
            i1 = R.nn_ref(R.xf_rows(X1, b["src"], 1.0), b["tgt"])[0]
            assert np.array_equal(i0, i1)
            pivot = a["tgt"].mean(0).astype(f32)
            for rej in (F.GATED.values() if gated else F.REJECTIONS):
                for mname, mode in MODES.items():
                    t = (name, k, rej, mname, gated)
                    r0 = F.ref_pass(a, rej, X0, mode=mode, idx=i0, **gates0)
                    r1 = F.ref_pass(b, rej, X1, mode=mode, idx=i1, **gates1)
                    for key in ("cand", "pop", "kept"):
                        assert np.array_equal(r0[key], r1[key]), (t, key)
                    assert (r0["n_c"], r0["n_kept"], r0["k"]) == (r1["n_c"], r1["n_kept"], r1["k"]), t
                    assert np.array_equal(r0["d2"] * (f * f), r1["d2"]), t
                    assert tau_bits(r1["tau"]) == tau_bits(f32(r0["tau"]) * (f * f)), (t, r0["tau"], r1["tau"])
                    assert 0 < r0["n_kept"] < len(a["src"]), t
                    code, h = (1, F.huber_scale(mode, r0, a)) if gated else (0, 1.0)
                    S0, _, n0 = T.trimmed_record(mode, r0["p"], r0["pn"], a["tgt"], a["tgt_n"], i0, r0["kept"], pivot, code, h)
                    S1, _, n1 = T.trimmed_record(mode, r1["p"], r1["pn"], b["tgt"], b["tgt_n"], i1, r1["kept"], pivot * f, code,
                                                 float(f32(h) * f))
                    assert n0 == n1 == r0["n_kept"], t
                    want = scale_record(S0, s, mname == "p2p")
                    assert np.array_equal(want, S1), (t, np.flatnonzero(want != S1))
                    if code:
                        assert 0.0 < S0[34] < n0, t                    # the weights bite
                    checked += 1
    assert checked == 2 * (6 + 3) * 3


@pytest.mark.parametrize("k", F.SCALE_EXPONENTS)
def test_color_restatement_scales_with_the_unit(ridge, k):
    s = 2.0 ** k
    f = f32(s)
    d = ridge
    # the gradient, in fp64
    for x, n, it, rows in ((d["tgt"], d["tgt_n"], d["tgt_i"], d["rows"]),):
        g0, deg0 = CR.gradient(x, n, it, rows)
        g1, deg1 = CR.gradient(x * f, n, it * f, rows)
        g2, deg2 = CR.gradient(x * f, n, it, rows)
        assert np.array_equal(g0, g1) and np.array_equal(g0 / s, g2)
        assert np.array_equal(deg0, deg1) and np.array_equal(deg0, deg2)
    # the record: plain, and with a Huber loss, both gates and a trim fraction
    b = F.scaled(d, s, intensities=True)
    X0 = F.nudge(d, 1.0, 0.002)
    X1 = F.scaled_transform(X0, s)
    pivot = d["tgt"].mean(0).astype(f32)
    p0, pn0 = R.moved(X0, d["src"], d["src_n"], R.MODE_PLANE)
    p1, pn1 = R.moved(X1, b["src"], b["src_n"], R.MODE_PLANE)
    i0, d20 = R.nn_ref(p0, d["tgt"])
    i1, _ = R.nn_ref(p1, b["tgt"])
    assert np.array_equal(i0, i1)
    md = f32(np.sqrt(np.median(d20.astype(np.float64))))
    mn = float(np.median(R.ndot(pn0, d["tgt_n"][i0])))
    hs = f32(2e-3)
    for v0, v1 in ((dict(), dict()),
                   (dict(loss=1, scale=float(hs), max_d2=R.f32_max_d2(md), min_ndot=mn, rho=0.6),
                    dict(loss=1, scale=float(hs * f), max_d2=R.f32_max_d2(md * f), min_ndot=mn, rho=0.6))):
        S0, _, k0 = CR.color_record(p0, pn0, d["src_i"], d["tgt"], d["tgt_n"], d["tgt_g"], d["tgt_i"], i0, pivot, **v0)
        S1, _, k1 = CR.color_record(p1, pn1, b["src_i"], b["tgt"], b["tgt_n"], d["tgt_g"], b["tgt_i"], i1, pivot * f, **v1)
        assert np.array_equal(k0, k1) and (not v0 or 0 < k0.sum() < len(k0))
        want = scale_record(S0, s)
        assert np.array_equal(want, S1), (k, bool(v0), np.flatnonzero(want != S1))
        if v0:
            assert 0.0 < S0[34] < 0.95 * k0.sum()


# ---- 2. range ---------------------------------------------------------------------------------------------------------------------
def test_scaled_distances_stay_normal_and_finite(pairs, ridge):
    tiny, big = float(np.finfo(f32).tiny), float(np.finfo(f32).max)
    for name, d in list(pairs.items()) + [("ridge", ridge)]:
        d2 = R.nn_ref(d["src"], d["tgt"])[1].astype(np.float64)
        lo, hi = d2[d2 > 0].min(), d2.max()
        for k in F.SCALE_EXPONENTS:
            print("%s 2^%d: candidate d2 in [%.3g, %.3g]" % (name, k, lo * 4.0 ** k, hi * 4.0 ** k))
            assert lo * 4.0 ** k >= tiny and hi * 4.0 ** k < big, (name, k)
            assert np.array_equal((d2.astype(f32) * f32(4.0 ** k)).astype(np.float64), d2 * 4.0 ** k)      # no bit is lost


# ---- 3. the shifted fixtures -------------------------------------------------------------------------------------------------------
def assert_bites(name, r, n_src, t):
    family, kw = F.REJECTIONS[name]
    selects = kw.get("factor", 0.0) > 0 or kw.get("rho", 1.0) < 1
    if family == "trim":
        assert 0 < r["n_kept"] < n_src, t
    elif family == "reject":
        if kw.get("one_to_one"):
            assert 0 < r["n_u"] < r["n_c"], t
        if selects:
            assert 0 < r["n_kept"] < r["n_u"], t
    else:
        assert 0 < r["n_r"] < r["n_u"] <= r["n_c"], t
        if selects:
            assert 0 < r["n_kept"] < r["n_r"], t
    return selects


FRAMES = [(n, o) for n in F.OFFSETS for o in F.OFFSETS[n] + (F.TIE_OFFSETS[n],)]


@pytest.mark.parametrize("name,o", FRAMES, ids=["%s-%g" % f for f in FRAMES])
def test_shifted_fixtures_bite_and_carry_their_ties(pairs, name, o):
    d = F.shifted(pairs[name], o)
    tie_frame = o == F.TIE_OFFSETS[name]
    idx = R.nn_ref(d["src"], d["tgt"])[0]
    for rej, (family, kw) in F.REJECTIONS.items():
        r = F.ref_pass(d, rej, idx=idx)
        ti = F.ties(r)
        t = (name, o, rej)
        print("%s at %g extents, %s: n_c %d, population %d, kept %d; candidates sharing a d2 %d, at the select's rank %d, targets "
              "claimed at equal d2 %d" % (name, o, rej, r["n_c"], int(r["pop"].sum()), r["n_kept"], ti["cand"], ti["at_rank"], ti["claims"]))
        selects = assert_bites(rej, r, len(d["src"]), t)
        if o >= 1e3:
            assert ti["cand"] >= 1, t               # (at 1e2 extents there is none: see the module's docstring)
        if tie_frame:
            assert ti["cand"] >= 100, t
            if selects:
                assert ti["at_rank"] > 1, t
                if kw.get("rho", 1.0) < 1:
                    assert r["n_kept"] > r["k"], t                            # the select's last bin holds more than the rank needs
            if family != "trim":
                assert ti["claims"] >= 10, t                                  # the caller's row decides claims
    if tie_frame:
        return
    # one Huber + gates case per family: the gates drop pairs, the rejector still bites
    g = F.flipped(d)
    mcd = F.gate_distance(g)
    for family, rej in F.GATED.items():
        r = F.ref_pass(g, rej, max_d2=R.f32_max_d2(mcd), min_ndot=F.MIN_NDOT, idx=idx)
        t = (name, o, rej, "gated")
        assert 0 < r["n_c"] < int((idx >= 0).sum()), t
        assert_bites(rej, r, len(d["src"]), t)
        assert F.huber_scale(R.MODE_PAPER, r, g) > 0, t


def test_one_to_one_winners_at_a_tie_are_the_lowest_rows(pairs):
    """the restatement's own tie-break in the tie frames, by the definition: among the candidates of a target at its smallest d2 bits
    the lowest caller row wins"""
    for name, d0 in pairs.items():
        d = F.shifted(d0, F.TIE_OFFSETS[name])
        r = F.ref_pass(d, "one-to-one")
        bits, seen = J.bits(r["d2"]), 0
        for j in np.unique(r["idx"][r["cand"]]):
            rows = np.flatnonzero(r["cand"] & (r["idx"] == j))
            low = rows[bits[rows] == bits[rows].min()]
            assert np.flatnonzero(r["uniq"] & (r["idx"] == j)).tolist() == [low.min()]
            seen += len(low) > 1
        assert seen == F.ties(r)["claims"] >= 10
