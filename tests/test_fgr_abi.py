"""CPU tests of the C boundary of Fast Global Registration: the header still compiles as pedantic C99, the library exports the new entry
points, the structs have the sizes the bindings assume, and every argument error that is decided before a device is needed comes back
as SYMMICP_ERR_ARG; with valid arguments and no device the calls fail loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_fgr", "symmicp_fgr", "symmicp_ctx_fgr_pass"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def test_library_exports_the_new_entry_points(sym):
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW + ["symmicp_fgr_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS) and "symmicp_fgr_config_default" in sym.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_fgr_config_default(" in hdr
    assert "SYMMICP_ERR_NO_CONSENSUS = 8" in hdr and sym.ERR_NO_CONSENSUS == 8
    assert sym.lib().symmicp_version() == 100                      # additive: the version stays
    for name in ("FgrConfig", "FgrResult", "fgr_config", "fgr"):
        assert hasattr(sym, name), name
    assert hasattr(sym.Engine, "fgr") and hasattr(sym.Engine, "fgr_pass")


def test_struct_sizes_and_defaults(sym):
    assert C.sizeof(sym.FgrConfig) == 40 and C.sizeof(sym.FgrResult) == 40 + 16 * 8
    cfg = sym.FgrConfig()
    sym.lib().symmicp_fgr_config_default(C.byref(cfg))
    assert cfg.struct_size == 40 and cfg.iterations == 64 and cfg.decrease_every == 4 and cfg.max_tuples == 1000
    assert cfg.tuple_trials == 0 and cfg.seed == 0 and cfg.max_dist == 0.0
    assert cfg.division_factor == np.float32(1.4) and cfg.tuple_scale == np.float32(0.95)
    sym.lib().symmicp_fgr_config_default(None)                     # tolerated
    c2 = sym.fgr_config(0.5, iterations=7, decrease_every=2, division_factor=2.0, tuple_scale=0.9, max_tuples=11, tuple_trials=13, seed=2 ** 63 + 5)
    assert (c2.struct_size, c2.max_dist, c2.iterations, c2.decrease_every, c2.division_factor, c2.max_tuples, c2.tuple_trials, c2.seed) == \
        (40, 0.5, 7, 2, 2.0, 11, 13, 2 ** 63 + 5)


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets status codes, not crashes"""
    src = tmp_path / "fgr_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, T[16], w[3000], X[16] = {1.f}, trX[65 * 16], trM[64];
    double sums[40], trS[64 * 40];
    int32_t pairs[6] = {0, 0, 1, 1, 2, 2}, set[3000];
    symmicp_fgr_config cfg;
    symmicp_fgr_result res;
    int a, b, c;
    symmicp_fgr_config_default(&cfg);
    cfg.max_dist = -1.0f;                                                           /* refused */
    a = symmicp_fgr(-1, xyz, 3, 1, 3, xyz, 3, 1, 3, pairs, 3, &cfg, T, &res, set, w, trX, trS, trM);
    b = symmicp_ctx_fgr(NULL, xyz, 3, 1, 3, xyz, 3, 1, 3, pairs, 3, &cfg, T, &res, set, w, trX, trS, trM);
    c = symmicp_ctx_fgr_pass(NULL, xyz, xyz, 3, X, 1.0f, sums, w);
    printf("status %d %d %d sizes %d %d defaults %d %d %u\n", a, b, c, (int)sizeof(cfg), (int)sizeof(res), (int)cfg.iterations,
           (int)cfg.decrease_every, (unsigned)cfg.max_tuples);
    return 0;
}
''')
    exe = tmp_path / "fgr_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 sizes 40 168 defaults 64 4 1000" in r.stdout


def _fgr_args(sym, **kw):
    rng = np.random.default_rng(4)
    src, tgt = rng.random((10, 3)).astype(np.float32), rng.random((12, 3)).astype(np.float32)
    pairs = np.stack([np.arange(6), np.arange(6) + 3], 1).astype(np.int32)
    cfg = sym.fgr_config(0.1, seed=1)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return src, tgt, pairs, cfg


def test_fgr_argument_errors_need_no_device(sym):
    L = sym.lib()
    T, res = np.zeros(16, np.float32), sym.FgrResult()

    def call(src, tgt, pairs, cfg, ns=None, nt=None, m=None, T=T, res=res, f=L.symmicp_fgr, head=(-1,)):
        return f(*head, None if src is None else fp(src), 3, 1, len(src) if ns is None else ns, None if tgt is None else fp(tgt), 3, 1,
                 len(tgt) if nt is None else nt, None if pairs is None else ip(pairs), len(pairs) if m is None else m,
                 None if cfg is None else C.byref(cfg), None if T is None else fp(T), None if res is None else C.byref(res), None, None,
                 None, None, None)

    src, tgt, pairs, cfg = _fgr_args(sym)
    assert call(src, tgt, pairs, cfg, ns=0) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, nt=0) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, ns=2 ** 31) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, nt=2 ** 31) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, m=2) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, m=2 ** 31) == sym.ERR_ARG
    assert call(src, tgt, pairs, None) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, T=None) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, res=None) == sym.ERR_ARG
    for name in ("src", "tgt", "pairs"):
        a = dict(src=src, tgt=tgt, pairs=pairs)
        a[name] = None
        assert call(a["src"], a["tgt"], a["pairs"], cfg, ns=10, nt=12, m=6) == sym.ERR_ARG, name
    for bad in (dict(struct_size=36), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=float("inf")), dict(max_dist=float("nan")),
                dict(iterations=0), dict(iterations=1025), dict(iterations=-3), dict(decrease_every=0), dict(decrease_every=-1),
                dict(division_factor=1.0), dict(division_factor=0.5), dict(division_factor=float("inf")), dict(division_factor=float("nan")),
                dict(tuple_scale=0.0), dict(tuple_scale=-0.5), dict(tuple_scale=1.0001), dict(tuple_scale=float("nan")),
                dict(max_tuples=2 ** 18 + 1), dict(tuple_trials=2 ** 24 + 1)):
        assert call(*_fgr_args(sym, **bad)) == sym.ERR_ARG, bad
    for row, col, val in ((0, 0, -1), (5, 0, 10), (3, 1, 12), (2, 1, -7)):
        p = pairs.copy()
        p[row, col] = val
        assert call(src, tgt, p, cfg) == sym.ERR_ARG                   # a row outside its cloud
    s = src.copy(); s[pairs[4, 0], 2] = np.nan
    assert call(s, tgt, pairs, cfg) == sym.ERR_ARG                     # a paired point that is not finite
    t = tgt.copy(); t[pairs[1, 1], 0] = np.inf
    assert call(src, t, pairs, cfg) == sym.ERR_ARG
    # with the tuple test off the set is the pairs themselves: at most 2^20 of them
    big = np.zeros((2 ** 20 + 1, 2), np.int32)
    assert call(src, tgt, big, _fgr_args(sym, max_tuples=0)[3]) == sym.ERR_ARG
    # the context forms with no context
    assert call(src, tgt, pairs, cfg, f=L.symmicp_ctx_fgr, head=(None,)) == sym.ERR_ARG
    sums = np.zeros(40)
    assert L.symmicp_ctx_fgr_pass(None, fp(src), fp(src), 10, fp(np.eye(4, dtype=np.float32)), 1.0, dp(sums), None) == sym.ERR_ARG
    with pytest.raises(ValueError):
        sym.fgr(src, tgt, pairs[:, :1], 0.1)


def test_fgr_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    src, tgt, pairs, cfg = _fgr_args(sym)
    T, res = np.full(16, -7, np.float32), sym.FgrResult()
    st = sym.lib().symmicp_fgr(-1, fp(src), 3, 1, 10, fp(tgt), 3, 1, 12, ip(pairs), 6, C.byref(cfg), fp(T), C.byref(res), None, None, None, None, None)
    assert st == sym.ERR_HIP and (T == -7).all()
    with pytest.raises(sym.SymmIcpError) as e:
        sym.fgr(src, tgt, pairs, 0.1)
    assert e.value.status == sym.ERR_HIP
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, verbose=False)
    icp.setInputSource(src, src)
    icp.setInputTarget(tgt, tgt)
    icp.setGlobalInit(fpfh_radius=0.5, max_dist=0.1, method="fgr")
    with pytest.raises(sym.SymmIcpError) as e:
        icp.align()
    assert e.value.status == sym.ERR_HIP
