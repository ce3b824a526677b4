"""The fixtures, frames and rejections of the rejector and COLOR frame tests (test_frames_ref.py on the CPU, test_gpu_reject_frames.py
and test_gpu_color_frames.py on the GPU), and what the numpy restatements say of a first pass in them.

Frames: a power-of-two unit s (clouds x s: exact), and an offset o extents from the origin -- test_gpu_frames.py's construction:
off = o E (1, -0.7, 0.3) with E the largest extent of the pair's bounding box, added in fp64 and rounded to fp32, normals untouched.
Fixtures: the cat pair, the partial-overlap surface cut to 8000 points, and COLOR's ragged ridge pair (6001 / 5003 points)."""
import numpy as np

import _recip_ref as RR
import _record_ref as R
import _reject_ref as J
import _trim_ref as T
from _frames import scale_record

f32 = np.float32

SCALE_EXPONENTS = (-10, 10)
SURFACE_N = 8000
OFFSETS = {"cat": (1e2, 1e3, 1e4), "surface": (1e2, 1e3)}
# Measured by test_frames_ref.py: at 1e2 extents no two candidates of a first pass share a d2 (three squared differences of ~1e3
# quanta each leave millions of values), at 1e3 a handful do, at 1e4 a seventh of the cat's; no select of a first pass meets a tie at
# its rank and one target in all is claimed at equal d2.  The frames below are the nearest at which every select does and dozens of
# claims are: the clouds are quantised to a few hundredths of their extent there.
TIE_OFFSETS = {"cat": 3e5, "surface": 3e5}

# the six rejections: which restatement (and which check_passes) they belong to, and that one's arguments
REJECTIONS = {
    "rho0.7": ("trim", dict(rho=0.7)),
    "median2": ("reject", dict(factor=2.0)),
    "one-to-one": ("reject", dict(one_to_one=True)),
    "one-to-one+median2": ("reject", dict(one_to_one=True, factor=2.0)),
    "reciprocal": ("recip", dict()),
    "reciprocal+rho0.7": ("recip", dict(rho=0.7)),
}
# one Huber + gates case per family
GATED = {"trim": "rho0.7", "reject": "one-to-one+median2", "recip": "reciprocal+rho0.7"}
GATE_QUANTILE = 0.8           # the distance gate: this quantile of the first pass's distances (the existing gate tests' recipe)
MIN_NDOT = 0.0                # ... with every third source normal reversed


def surface():
    return T.partial_overlap(SURFACE_N, 0xC4)


def ridge_ragged():
    """test_gpu_color.py's ragged pair, without the gradient"""
    from symmicp import synth
    d = synth.ridge_textured(6001, seed=0xD1)
    return dict(d, src=d["src"][:5003], src_n=d["src_n"][:5003], src_i=d["src_i"][:5003])


def extent(d):
    lo = np.minimum(d["src"].min(0), d["tgt"].min(0)).astype(np.float64)
    hi = np.maximum(d["src"].max(0), d["tgt"].max(0)).astype(np.float64)
    return float(np.max(hi - lo))


def offset_of(d, o):
    return o * extent(d) * np.array([1.0, -0.7, 0.3])


def shifted(d, o):
    """the pair o extents from the origin; a truth, if the pair has one, is rewritten for the new frame"""
    off = offset_of(d, o)
    out = dict(d, src=(d["src"].astype(np.float64) + off).astype(f32), tgt=(d["tgt"].astype(np.float64) + off).astype(f32), offset=off)
    if "truth" in d:
        Tt = np.array(d["truth"], np.float64)
        Tt[:3, 3] = Tt[:3, 3] + off - Tt[:3, :3] @ off
        out["truth"] = Tt
    return out


def scaled(d, s, intensities=False):
    f = f32(s)
    out = dict(d, src=d["src"] * f, tgt=d["tgt"] * f)
    if intensities:
        out.update(src_i=d["src_i"] * f, tgt_i=d["tgt_i"] * f)
    return out


def flipped(d):
    """every third source normal reversed: min_normal_dot = 0 then drops a third of the pairs"""
    out = dict(d, src_n=d["src_n"].copy())
    out["src_n"][::3] *= -1
    return out


def gate_distance(d):
    return float(np.sqrt(np.quantile(R.nn_ref(d["src"], d["tgt"])[1], GATE_QUANTILE)))


def nudge(d, deg=2.0, frac=0.01):
    """a rigid transform about the source's centre: deg degrees, frac of the extent (fp32 4x4)"""
    from symmicp import synth
    c = d["src"].astype(np.float64).mean(0)
    Rm = synth.rotation(deg, (0.2, 1.0, -0.4))
    return synth.rigid4(Rm, c - Rm @ c + frac * extent(d) * np.array([1.0, -0.5, 0.25])).astype(f32)


def scaled_transform(X, s):
    X = np.array(X, f32).reshape(4, 4)
    X[:3, 3] *= f32(s)
    return X


def ref_pass(d, name, X=None, max_d2=0.0, min_ndot=-2.0, mode=R.MODE_PAPER, idx=None):
    """the restatement's pass of rejection `name` at transform X (identity), exact fp32 nearest neighbours by the oracle's brute force
    (or idx, if they are at hand) -> the restatement's dict, plus p, pn, idx, pop = the select's population (mask) and k = the
    select's rank in it (0: no select)"""
    X = np.eye(4, dtype=f32) if X is None else np.asarray(X, f32)
    family, kw = REJECTIONS[name]
    p, pn = R.moved(X, d["src"], d["src_n"], mode)
    if idx is None:
        idx = R.nn_ref(p, d["tgt"])[0]
    if family == "trim":
        r = T.trim_pass(p, pn, d["tgt"], d["tgt_n"], idx, kw["rho"], max_d2, min_ndot)
        r = dict(r, n_kept=int(r["kept"].sum()), pop=r["cand"])
    elif family == "reject":
        r = J.reject_pass(p, pn, d["tgt"], d["tgt_n"], idx, max_d2=max_d2, min_ndot=min_ndot, **kw)
        r = dict(r, pop=r["uniq"])
    else:
        r = RR.recip_pass(p, pn, d["tgt"], d["tgt_n"], idx, d["src"], X, max_d2=max_d2, min_ndot=min_ndot, **kw)
        r = dict(r, pop=r["recip"])
    rho = 0.5 if kw.get("factor", 0.0) > 0 else kw.get("rho", 1.0)
    r["k"] = T.trim_k(rho, int(r["pop"].sum())) if rho < 1 else 0
    return dict(r, p=p, pn=pn, idx=idx)


def ties(r):
    """what a pass carries of exact ties in d2 -> dict(cand = candidates whose d2 bits another candidate shares, at_rank = members of
    the select's population at the select's order statistic (1: no tie there; 0: no select), claims = targets whose smallest d2
    bits two or more candidates hold, so that the caller's row decides the claim)"""
    bits = J.bits(r["d2"])
    c = np.flatnonzero(r["cand"])
    _, cnt = np.unique(bits[c], return_counts=True)
    out = dict(cand=int(cnt[cnt > 1].sum()), at_rank=0, claims=0)
    if r["k"]:
        b = np.sort(bits[r["pop"]])
        out["at_rank"] = int((b == b[r["k"] - 1]).sum())
    if len(c):
        j = r["idx"][c]
        order = np.lexsort((bits[c], j))
        js, bs = j[order], bits[c][order]
        first = np.ones(len(js), bool)
        first[1:] = js[1:] != js[:-1]
        start = np.flatnonzero(first)
        lo = np.repeat(bs[start], np.diff(np.append(start, len(js))))
        out["claims"] = int((np.add.reduceat((bs == lo).astype(np.int64), start) > 1).sum())
    return out


def huber_scale(mode, r, d):
    """the median |residual| of a pass's kept pairs (r: ref_pass's dict), as fp32: a Huber scale that bites"""
    k = r["kept"]
    res = R.pass_terms(mode, r["p"][k], r["pn"][k], d["tgt"][r["idx"][k]], d["tgt_n"][r["idx"][k]], np.zeros(3, f32))[1]
    return float(f32(np.median(np.abs(res))))


# ---- what the GPU files assert of a run under a unit ------------------------------------------------------------------------------
def tau_bits(x):
    return int(f32(x).view(np.uint32))


def states(sym, e):
    """(status, values) of the three state getters after a pass"""
    out = []
    for get in (e.trim_state, e.rejection_state, e.reciprocal_state):
        try:
            out.append((0, tuple(get())))
        except sym.SymmIcpError as x:
            out.append((x.status, None))
    return out


def assert_transform_scaled(X0, X, s, what):
    f = f32(s)
    assert np.array_equal(X[:3, :3], X0[:3, :3]), (what, X, X0)
    assert np.array_equal(X[:3, 3], X0[:3, 3] * f), (what, X[:3, 3], X0[:3, 3] * f)
    assert np.array_equal(X[3], X0[3]), what


def assert_passes_scaled(p0, p1, s, p2p, rejects=True):
    """the passes p1 of a run in clouds x s against the passes p0 of the unscaled run, bit for bit (a pass: the step's dict plus idx, d2,
    X and states; COLOR's record has the non-P2P dims; rejects: the context reports rejected rows as -1)"""
    f = f32(s)
    assert len(p0) == len(p1) == 4                      # begin + 3 steps
    for k, (a, b) in enumerate(zip(p0, p1)):
        assert a["status"] == b["status"] == 0 and a["iter"] == b["iter"], (k, a["status"], b["status"])
        assert np.array_equal(a["idx"], b["idx"]), (k, int((a["idx"] != b["idx"]).sum()))
        if rejects:
            assert (a["idx"] < 0).any() and a["pairs"] == int((a["idx"] >= 0).sum()), k           # rejected rows are among them
        assert np.array_equal(a["d2"] * (f * f), b["d2"]), k
        want = scale_record(a["sums"], s, p2p)
        assert np.array_equal(want, b["sums"]), (k, np.flatnonzero(want != b["sums"]))
        assert a["pairs"] == b["pairs"] > 0, k
        assert f32(a["diff"]) * f == f32(b["diff"]), k
        assert [st for st, _ in a["states"]] == [st for st, _ in b["states"]], k
        for (_, u), (_, v) in zip(a["states"], b["states"]):
            if u is None:
                continue
            if len(u) == 2:                                     # reciprocal_state: counts only
                assert u == v, (k, u, v)
            else:
                assert u[:-1] == v[:-1], (k, u, v)              # every count
                assert tau_bits(v[-1]) == tau_bits(f32(u[-1]) * (f * f)), (k, u, v)
        assert_transform_scaled(a["X"], b["X"], s, k)
        assert_transform_scaled(a["increment"], b["increment"], s, k)
