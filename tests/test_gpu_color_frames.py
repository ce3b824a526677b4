"""Colored ICP in other coordinate frames (run with -m gpu on a real MI355X).  acc_color adds a geometric row in PLANE's units and a
photometric row with k = p x g and c_C = d . g + (I_q - I_p): the record scales by one power of the unit s per slot only if the
intensities are scaled with the lengths, for then the gradient g keeps its bits (tests/test_frames_ref.py proves both on the numpy
restatement).  On the ragged ridge pair (6001 / 5003 points) and its identity twin cut to 2003 rows:

  * the gradient is homogeneous: g(s x, n, s I) has the bits of g(x, n, I), g(s x, n, I) is g(x, n, I) / s exactly, the degenerate
    rows (exact zeros) are the same -- k = 3, 10, 16, s = 2^-10 and 2^10, also on test_gpu_color.py's degenerate cloud;
  * the gradient 1e2 and 1e3 extents from the origin stays at test_gpu_color.py's bar, 2^-22 |g_ref|_inf against the fp64 restatement
    fed the device's k-NN rows (the kernel forms its differences in fp64 from the fp32 inputs: the offset costs nothing);
  * begin + 3 steps in clouds and intensities x s (HUBER_SCALE and max_corr_dist x s too) run the same passes bit for bit
    (_frame_cases.assert_passes_scaled, the non-P2P record dims), the gradient recomputed on the device being the unscaled one;
  * every pass 1e2 and 1e3 extents from the origin against the numpy COLOR record at test_gpu_color.py's bars (_run_record_matrix)."""
import numpy as np
import pytest

import _frame_cases as F
import _record_ref as R
from test_gpu_color import HUBER_SCALE, VARIANTS, _check_gradient, _degenerate_cloud, _engine, _identity_twin, _run_record_matrix, _with_gradient

pytestmark = pytest.mark.gpu
f32 = np.float32
OFFSETS = (1e2, 1e3)


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def ragged(sym):
    return _with_gradient(sym, F.ridge_ragged())


@pytest.fixture(scope="module")
def twin(sym, ragged):
    return _identity_twin(sym, ragged, 2003)


# ---- the gradient -----------------------------------------------------------------------------------------------------------------
_G0 = {}


@pytest.mark.parametrize("e", F.SCALE_EXPONENTS)
@pytest.mark.parametrize("k", [3, 10, 16])
@pytest.mark.parametrize("cloud", ["ragged target", "degenerate"])
def test_gradient_is_homogeneous(sym, ragged, cloud, k, e):
    x, n, it = (ragged["tgt"], ragged["tgt_n"], ragged["tgt_i"]) if cloud == "ragged target" else _degenerate_cloud()
    if (cloud, k) not in _G0:
        _G0[(cloud, k)] = sym.intensity_gradient(x, n, it, k)
    g0 = _G0[(cloud, k)]
    f = f32(2.0 ** e)
    g1 = sym.intensity_gradient(x * f, n, it * f, k)
    g2 = sym.intensity_gradient(x * f, n, it, k)
    assert g0.tobytes() == g1.tobytes(), int((g0 != g1).any(1).sum())
    assert np.array_equal(g2, g0 / f), int((g2 != g0 / f).any(1).sum())
    zero = (g0 == 0).all(1)
    assert np.array_equal(zero, (g1 == 0).all(1)) and np.array_equal(zero, (g2 == 0).all(1))
    if cloud == "degenerate":
        assert zero[100:140].all() and zero[300] and not zero[400:].all()       # collinear, zero normal
        assert k > 10 or zero[200:212].all()                                     # twelve copies of one point: duplicates only up to k = 11
    else:
        assert k != 10 or (not zero.any() and np.array_equal(g0, ragged["tgt_g"]))
    print("%s k=%d 2^%d: %d rows, %d degenerate" % (cloud, k, e, len(x), int(zero.sum())))


@pytest.mark.parametrize("o", OFFSETS)
def test_gradient_far_from_the_origin(sym, ragged, cat, o):
    d = F.shifted(ragged, o)
    _check_gradient(sym, d["tgt"], d["tgt_n"], d["tgt_i"], 10, "ragged target at %g extents" % o)
    c = F.shifted(cat, o)
    rng = np.random.default_rng(3)
    it = (0.5 + 0.01 * cat["src"][:, 0] + 0.1 * rng.uniform(size=len(cat["src"]))).astype(f32)      # (test_gpu_color.py's intensity for the cat)
    _check_gradient(sym, c["src"], c["src_n"], it, 10, "cat at %g extents" % o)


# ---- passes under units -------------------------------------------------------------------------------------------------------------
def gates_of(oracle, d, corr):
    """_run_record_matrix's bounds: the median pair distance of the first pass, the median normal dot"""
    j = np.arange(len(d["src"])) if corr == "identity" else oracle.nn_brute(d["src"], d["tgt"])[0]
    return (float(np.sqrt(np.median(R.dist2(d["src"], d["tgt"][j]).astype(np.float64)))), float(np.median(R.ndot(d["src_n"], d["tgt_n"][j]))))


def run_passes(sym, d, s, corr, variant, gates):
    f = f32(s)
    v = VARIANTS[variant]
    ds = F.scaled(d, s, intensities=True)
    g = sym.intensity_gradient(ds["tgt"], ds["tgt_n"], ds["tgt_i"], 10)
    assert g.tobytes() == d["tgt_g"].tobytes()                     # the device's gradient of the scaled target is the unscaled one
    kw = dict(max_corr_dist=float(f32(gates[0]) * f), min_normal_dot=gates[1]) if v.get("gates") else {}
    passes = []
    with _engine(sym, dict(ds, tgt_g=g), corr, host_loop=1, fixed_iters=1, **kw) as e:
        if "loss" in v:
            e.set_robust_loss(v["loss"], float(f32(HUBER_SCALE) * f))
        if "trim" in v:
            e.set_trim_fraction(v["trim"])
        it = e.begin()
        for k in range(4):
            idx, d2 = e.correspondences()
            passes.append(dict(it, idx=idx, d2=d2, X=e.transform().copy(), states=F.states(sym, e)))
            if k == 3 or it["status"] != 0:
                break
            it = e.step(check=False)
    return passes


UNIT_PARAMS = [(c, v, e) for c in ("identity", "brute", "tree") for v in ("plain", "all") for e in F.SCALE_EXPONENTS]
_UNSCALED = {}


@pytest.mark.parametrize("corr,variant,e", UNIT_PARAMS, ids=["%s-%s-2^%d" % p for p in UNIT_PARAMS])
def test_power_of_two_units_run_the_same_passes(sym, oracle, ragged, twin, corr, variant, e):
    d = twin if corr == "identity" else ragged
    if (corr, variant) not in _UNSCALED:
        gates = gates_of(oracle, d, corr)
        _UNSCALED[(corr, variant)] = (gates, run_passes(sym, d, 1.0, corr, variant, gates))
    gates, p0 = _UNSCALED[(corr, variant)]
    p1 = run_passes(sym, d, 2.0 ** e, corr, variant, gates)
    F.assert_passes_scaled(p0, p1, 2.0 ** e, False, rejects=variant == "all")
    if variant == "all":
        # the gates, the trim and the weights bite
        nc, kept, _ = p0[0]["states"][0][1]
        assert 0 < kept < nc < len(d["src"]) and 0.0 < p0[0]["sums"][34] < 0.95 * p0[0]["sums"][37] and p0[0]["sums"][37] == kept
    else:
        assert p0[0]["pairs"] == len(d["src"]) and [st for st, _ in p0[0]["states"]] == [sym.ERR_STATE] * 3


# ---- passes at offsets ----------------------------------------------------------------------------------------------------------------
_SHIFTED = {}


@pytest.mark.parametrize("o", OFFSETS)
@pytest.mark.parametrize("variant", ["plain", "all"])
@pytest.mark.parametrize("corr", ["brute", "tree"])
def test_passes_far_from_the_origin_match_the_numpy_record(sym, oracle, ragged, corr, variant, o):
    if o not in _SHIFTED:
        _SHIFTED[o] = _with_gradient(sym, F.shifted(ragged, o))
    _run_record_matrix(sym, oracle, _SHIFTED[o], corr, variant)
