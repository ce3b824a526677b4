"""CPU tests of the C boundary of SYMMICP_MODE_NDT: the exports and the Python surface, the weight against its numpy restatement bit for
bit, the Gauss constants, the default configuration, and the host-side refusals of symmicp_ndt_map -- all before a device is needed."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import _ndt_ref as R
from conftest import ROOT

F = np.float32
NEW = ["symmicp_ndt_config_default", "symmicp_set_ndt", "symmicp_get_ndt", "symmicp_ndt_gauss", "symmicp_ndt_weight", "symmicp_get_ndt_state",
       "symmicp_ctx_ndt_map", "symmicp_ndt_map", "symmicp_get_ndt_map"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


def test_enum_exports_and_python_surface(sym):
    assert sym.MODE_NDT == 9
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    assert re.search(r"SYMMICP_MODE_NDT = 9\b", hdr)
    assert not re.search(r"SYMMICP_MODE_\w+ = (4|6|8)\b", hdr)              # those stay unassigned
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS)
    for n in NEW:
        assert "%s(" % n in hdr, n
    for name in ("ndt_map", "ndt_weight", "ndt_gauss"):
        assert callable(getattr(sym, name)), name
    for name in ("set_ndt", "get_ndt", "ndt_map", "get_ndt_map", "ndt_state"):
        assert callable(getattr(sym.Engine, name)), name
    # the header says why the weight does not depend on the unit of length
    i = hdr.index("Gauss constants.")
    assert "resolution^3" in hdr[i:i + 1200] and "unit of length" in hdr[i:i + 1200]


def test_create_and_solve_accept_the_mode_before_they_look_for_a_device(sym):
    L = sym.lib()
    for kw, bad in ((dict(mode=sym.MODE_NDT), False), (dict(mode=4), True), (dict(mode=6), True), (dict(mode=8), True), (dict(mode=10), True),
                    (dict(mode=sym.MODE_NDT, min_normal_dot=0.5), True), (dict(mode=sym.MODE_NDT, apply=sym.APPLY_INCREMENTAL), True)):
        cfg = sym.default_config(**kw)
        h = C.c_void_p()
        st = L.symmicp_create(C.byref(cfg), C.byref(h))
        if st == 0:
            L.symmicp_destroy(h)
        assert (st == sym.ERR_ARG) == bad, (kw, st)
    # the mode's solve is PLANE's, bit for bit
    rng = np.random.default_rng(4)
    S = np.zeros(40)
    A = rng.normal(size=(50, 6))
    G = A.T @ A
    k = 0
    for a in range(6):
        for b in range(a, 6):
            S[k] = G[a, b]
            k += 1
    S[21:27] = rng.normal(size=6) * 0.01
    S[27:33] = rng.normal(size=6)
    S[34] = 50.0
    a = sym.solve(sym.MODE_PLANE, S, np.zeros(3, F))
    b = sym.solve(sym.MODE_NDT, S, np.zeros(3, F))
    assert a[0] == b[0] == 0
    for x, y in zip(a[1:], b[1:]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    assert sym.solve(sym.MODE_NDT, np.zeros(40))[0] == sym.ERR_DEGENERATE
    assert sym.solve(4, S)[0] == sym.solve(10, S)[0] == sym.ERR_ARG


def test_weight_equals_the_restatement_bit_for_bit(sym):
    rng = np.random.default_rng(20261020)
    x = np.concatenate([-rng.uniform(0.0, 64.0, 90000), -rng.uniform(0.0, 1.0, 10000)]).astype(F)
    edges = F([0.0, -0.0, -64.0, np.nextafter(F(-64), F(0)), -1e30, np.nan, 1.0])
    x = np.concatenate([x, edges])
    L = sym.lib()
    got = np.array([L.symmicp_ndt_weight(C.c_float(float(v))) for v in x], F)
    ref = R.weight(x)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert list(got[-7:]) == [1.0, 1.0, 0.0, got[-4], 0.0, 0.0, 1.0] and got[-4] > 0
    # within 2^-22 relative of exp where it is not cut off (4 ulp against the 1.37 ulp the restatement measures)
    live = x > F(-64)
    xl = np.minimum(x[live], F(0)).astype(np.float64)
    e = np.array([math.exp(v) for v in xl])
    assert np.max(np.abs(got[live].astype(np.float64) - e) / e) <= 2.0 ** -22
    assert sym.ndt_weight(-1.0) == got.dtype.type(L.symmicp_ndt_weight(C.c_float(-1.0)))


def test_gauss_constants(sym):
    d1, d2 = sym.ndt_gauss(0.55)
    r1, r2 = R.gauss(0.55)
    assert abs(d1 - r1) <= 1e-12 and abs(d2 - r2) <= 1e-12
    assert abs(d1 - (-2.217225244)) < 1e-9 and abs(d2 - 0.433123004) < 1e-8
    L = sym.lib()
    a, b = C.c_double(7.0), C.c_double(7.0)
    for bad in (0.0, 1.0, -0.5, 2.0, float("nan")):
        assert L.symmicp_ndt_gauss(C.c_double(bad), C.byref(a), C.byref(b)) == sym.ERR_ARG
    assert L.symmicp_ndt_gauss(C.c_double(0.55), None, C.byref(b)) == sym.ERR_ARG
    assert a.value == 7.0 and b.value == 7.0


def test_default_configuration_and_struct_size(sym):
    cfg = sym.NdtConfig()
    sym.lib().symmicp_ndt_config_default(C.byref(cfg))
    assert C.sizeof(sym.NdtConfig) == 24 and cfg.struct_size == 24
    assert (cfg.resolution, cfg.min_points, cfg.neighbors) == (1.0, 6, 7)
    assert cfg.eig_ratio == F(0.01) and cfg.outlier_ratio == F(0.55)
    sym.lib().symmicp_ndt_config_default(None)
    x = np.random.default_rng(0).random((32, 3)).astype(F)
    cfg.struct_size = 20
    m = C.c_size_t(99)
    st = sym.lib().symmicp_ndt_map(-1, x.ctypes.data_as(C.POINTER(C.c_float)), 3, 1, 32, C.byref(cfg), None, None, None, None, None, None, None, 32,
                                   C.byref(m))
    assert st == sym.ERR_ARG and m.value == 99
    assert sym.lib().symmicp_set_ndt(None, C.byref(cfg)) == sym.ERR_ARG and sym.lib().symmicp_get_ndt(None, C.byref(cfg)) == sym.ERR_ARG
    assert sym.lib().symmicp_get_ndt_state(None, None, None) == sym.ERR_ARG


def test_map_argument_errors_need_no_device(sym):
    L = sym.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    x = np.random.default_rng(0).random((32, 3)).astype(F)
    n = len(x)
    key, m = np.zeros(n, np.uint32), C.c_size_t(0)

    def call(xyz=x, xr=3, xc=1, n_=n, cfg=None, m_=m, ctx=False, **kw):
        c = sym.ndt_config(**dict(dict(resolution=0.25), **kw)) if cfg is None else cfg
        head = (None,) if ctx else (-1,)
        fn = L.symmicp_ctx_ndt_map if ctx else L.symmicp_ndt_map
        return fn(*head, None if xyz is None else fp(xyz), xr, xc, n_, None if c is False else C.byref(c), key.ctypes.data_as(C.POINTER(C.c_uint32)),
                  None, None, None, None, None, None, n, None if m_ is None else C.byref(m_))

    assert call(xyz=None) == sym.ERR_ARG and call(cfg=False) == sym.ERR_ARG and call(m_=None) == sym.ERR_ARG
    assert call(n_=0) == sym.ERR_ARG and call(n_=2 ** 31) == sym.ERR_ARG
    assert call(ctx=True) == sym.ERR_ARG
    for v in (0.0, -1.0, np.inf, np.nan):
        assert call(resolution=v) == sym.ERR_ARG, v
    for v in (2, 0, -1):
        assert call(min_points=v) == sym.ERR_ARG, v
    for v in (0.0, -0.1, 1.5, np.nan):
        assert call(eig_ratio=v) == sym.ERR_ARG, v
    for v in (0.0, 1.0, -0.1, np.nan):
        assert call(outlier_ratio=v) == sym.ERR_ARG, v
    for v in (0, 2, 6, 27, -7):
        assert call(neighbors=v) == sym.ERR_ARG, v
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[5, 2] = v
        assert call(xyz=y) == sym.ERR_ARG
    # the grid's refusals: a cell coordinate at 2^23, more than 2^32 cells
    y = x.copy()
    y[3, 0] = 8388608.0
    assert call(xyz=y, resolution=1.0) == sym.ERR_ARG
    y[3] = (4000.0, 4000.0, 4000.0)
    assert call(xyz=y, resolution=1.0) == sym.ERR_ARG                        # 4001^3 cells
    assert call(xyz=y, resolution=4.0) in (sym.OK, sym.ERR_HIP)              # 1001^3: with a device this call runs
    # strides: a bad value the strides skip is not read
    wide = np.zeros((n, 5), F)
    wide[:, :3] = x
    wide[3, 4] = np.nan
    assert call(xyz=wide, xr=5) in (sym.OK, sym.ERR_HIP)
    wide[3, 1] = np.nan
    assert call(xyz=wide, xr=5) == sym.ERR_ARG


def test_map_fails_loudly_without_gpu(sym):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((64, 3)).astype(F)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.ndt_map(x, 0.25)
    assert e.value.status == sym.ERR_HIP
