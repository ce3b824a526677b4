"""CPU tests of the robust loss (symmicp_set_robust_loss): the host copy of the device weight formula, the public names,
and the command-line driver's argument checks.  No compute calls (there is no GPU here)."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()
    return symmicp


def np_weight(loss, scale, r):
    """the table of include/symmicp.h in fp32 numpy"""
    with np.errstate(divide="ignore"):
        return _np_weight(loss, scale, r)


def _np_weight(loss, scale, r):
    r = np.asarray(r, np.float32)
    u = r / np.float32(scale)
    au = np.abs(u)
    u2 = u * u
    one = np.float32(1)
    if loss == 1:
        return np.where(au <= one, one, one / au).astype(np.float32)
    if loss == 2:
        t = one - u2
        return np.where(au < one, t * t, np.float32(0)).astype(np.float32)
    if loss == 3:
        return (one / (one + u2)).astype(np.float32)
    if loss == 4:
        t = one + u2
        return (one / (t * t)).astype(np.float32)
    return np.ones_like(r)


LOSSES = ["huber", "tukey", "cauchy", "geman_mcclure"]


@pytest.mark.parametrize("name", LOSSES)
@pytest.mark.parametrize("scale", [1.0, 0.037, 250.0])
def test_weight_matches_formula(sym, name, scale):
    code = sym.loss_code(name)
    r = np.linspace(0.0, 10.0 * scale, 401, dtype=np.float32)
    r = np.concatenate([r, -r, np.float32([scale, -scale, 0.0])])
    w = sym.robust_weight(code, scale, r)
    ref = np_weight(code, scale, r)
    assert w.dtype == np.float32 and w.shape == r.shape
    np.testing.assert_allclose(w, ref, rtol=2e-7, atol=0)
    # u = 1 exactly and r = 0
    at1 = {"huber": 1.0, "tukey": 0.0, "cauchy": 0.5, "geman_mcclure": 0.25}[name]
    assert sym.robust_weight(name, scale, scale) == at1
    assert sym.robust_weight(name, scale, -scale) == at1
    assert sym.robust_weight(name, scale, 0.0) == 1.0
    # weights never grow with the residual
    wp = sym.robust_weight(code, scale, np.linspace(0.0, 10.0 * scale, 401, dtype=np.float32))
    assert np.all(np.diff(wp) <= 0) and np.all(wp >= 0) and np.all(wp <= 1)


def test_weight_bad_arguments_give_nan(sym):
    for loss, scale in [(5, 1.0), (-1, 1.0), (99, 1.0), (sym.LOSS_HUBER, 0.0), (sym.LOSS_TUKEY, -1.0),
                        (sym.LOSS_CAUCHY, float("nan")), (sym.LOSS_GEMAN_MCCLURE, float("inf"))]:
        assert np.isnan(sym.robust_weight(loss, scale, 0.5)), (loss, scale)
    # NONE ignores the scale: every pair at full weight
    assert sym.robust_weight(sym.LOSS_NONE, 0.0, 123.0) == 1.0
    assert sym.robust_weight("none", float("nan"), 1.0) == 1.0


def test_loss_names_and_enum(sym):
    assert (sym.LOSS_NONE, sym.LOSS_HUBER, sym.LOSS_TUKEY, sym.LOSS_CAUCHY, sym.LOSS_GEMAN_MCCLURE) == (0, 1, 2, 3, 4)
    for k, name in enumerate(["none"] + LOSSES):
        assert sym.loss_code(name) == k and sym.loss_code(name.upper()) == k and sym.loss_code(k) == k
    with pytest.raises(ValueError):
        sym.loss_code("l1")
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for k, name in enumerate(["NONE", "HUBER", "TUKEY", "CAUCHY", "GEMAN_MCCLURE"]):
        assert re.search(r"SYMMICP_LOSS_%s = %d\b" % (name, k), hdr), name
    for fn in ("symmicp_set_robust_loss", "symmicp_get_robust_loss", "symmicp_robust_weight"):
        assert fn in sym.EXPORTS and hasattr(sym.lib(), fn)
    m = sym.MyICP(mode=sym.MODE_PAPER)
    m.setRobustLoss("tukey", 2.0)
    assert m._loss == (sym.LOSS_TUKEY, 2.0)


def _driver():
    exe = os.path.join(ROOT, "icp-symm_amd", "bin", "icp_align")
    assert os.path.exists(exe), "run __graft_entry__.build()"
    return exe


@pytest.mark.parametrize("args", [
    ["--mode", "quirks", "--loss", "huber", "--loss-scale", "1"],
    ["--loss", "huber", "--loss-scale", "1"],                         # the default mode is quirks
    ["--mode", "paper", "--loss", "huber"],                           # no scale
    ["--mode", "paper", "--loss", "huber", "--loss-scale", "0"],
    ["--mode", "paper", "--loss", "huber", "--loss-scale", "nan"],
    ["--mode", "paper", "--loss", "huber", "--loss-scale", "x"],
    ["--mode", "paper", "--loss", "l1", "--loss-scale", "1"],
])
def test_driver_loss_usage_errors(tmp_path, args):
    """argument checks come before any file or device is touched: exit 64 (usage)"""
    r = subprocess.run([_driver()] + args + ["a.pcd", "b.pcd"], cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 64, (r.returncode, r.stderr)
    assert "usage:" in r.stderr and "--loss" in r.stderr
