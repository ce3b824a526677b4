"""CPU tests of the C boundary of feature matching and RANSAC: the header still compiles as pedantic C99, the library exports the new
entry points, the structs have the sizes the bindings assume, and every argument error that is decided before a device is needed
comes back as SYMMICP_ERR_ARG; with valid arguments and no device the calls fail loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_feature_nn", "symmicp_feature_nn", "symmicp_ctx_feature_correspondences", "symmicp_feature_correspondences",
       "symmicp_ctx_ransac", "symmicp_ransac", "symmicp_ctx_ransac_hypotheses"]


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
up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))


def test_library_exports_the_new_entry_points(sym):
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW + ["symmicp_ransac_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS) and "symmicp_ransac_config_default" in sym.EXPORTS
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "SYMMICP_ERR_NO_CONSENSUS = 8" in hdr and sym.ERR_NO_CONSENSUS == 8
    assert sym.lib().symmicp_version() == 100                      # additive: the version stays


def test_struct_sizes_and_defaults(sym):
    assert C.sizeof(sym.RansacConfig) == 32 and C.sizeof(sym.RansacResult) == 24 + 16 * 8
    cfg = sym.RansacConfig()
    sym.lib().symmicp_ransac_config_default(C.byref(cfg))
    assert cfg.struct_size == 32 and cfg.hypotheses == 100000 and cfg.seed == 0 and cfg.max_dist == 0.0
    assert abs(cfg.edge_ratio - 0.9) < 1e-7 and cfg.refits == 1
    sym.lib().symmicp_ransac_config_default(None)                  # tolerated


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets status codes, not crashes"""
    src = tmp_path / "global_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float fa[66], fb[66], d2[2], second[2], xyz[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, T[16], hyp[12 * 4], piv[6];
    int32_t nn[2], pairs[6] = {0, 0, 1, 1, 2, 2}, inl[4];
    uint8_t mask[3], status[4];
    size_t count = 0;
    symmicp_ransac_config cfg;
    symmicp_ransac_result res;
    int a, b, c, d, e, f, g, i;
    for (i = 0; i < 66; i++) { fa[i] = (float)i; fb[i] = (float)(66 - i); }
    symmicp_ransac_config_default(&cfg);
    cfg.hypotheses = 4;
    cfg.max_dist = -1.0f;                                                           /* refused */
    a = symmicp_feature_nn(-1, fa, 0, fb, 2, nn, d2, second);
    b = symmicp_ctx_feature_nn(NULL, fa, 2, fb, 2, nn, d2, second);
    c = symmicp_feature_correspondences(-1, fa, 2, fb, 2, 1, 0.0f, pairs, d2, 2, NULL);
    d = symmicp_ctx_feature_correspondences(NULL, fa, 2, fb, 2, 1, 0.0f, pairs, d2, 2, &count);
    e = symmicp_ransac(-1, xyz, 3, 1, 3, xyz, 3, 1, 3, pairs, 3, &cfg, T, &res, mask, status, inl);
    f = symmicp_ctx_ransac(NULL, xyz, 3, 1, 3, xyz, 3, 1, 3, pairs, 3, &cfg, T, &res, mask, status, inl);
    g = symmicp_ctx_ransac_hypotheses(NULL, xyz, 3, 1, 3, xyz, 3, 1, 3, pairs, 3, &cfg, hyp, status, piv);
    printf("status %d %d %d %d %d %d %d sizes %d %d codes %d %d\n", a, b, c, d, e, f, g, (int)sizeof(cfg), (int)sizeof(res),
           (int)SYMMICP_ERR_NO_CONSENSUS, SYMMICP_RANSAC_FAR);
    return 0;
}
''')
    exe = tmp_path / "global_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 1 1 1 sizes 32 152 codes 8 4" in r.stdout


def _features(n, seed):
    return (np.random.default_rng(seed).random((n, 33)) * 100).astype(np.float32)


def test_feature_nn_argument_errors_need_no_device(sym):
    L = sym.lib()
    fa, fb = _features(8, 0), _features(5, 1)
    nn, d2, sec = np.zeros(8, np.int32), np.zeros(8, np.float32), np.zeros(8, np.float32)
    f = L.symmicp_feature_nn
    assert f(-1, None, 8, fp(fb), 5, ip(nn), fp(d2), fp(sec)) == sym.ERR_ARG
    assert f(-1, fp(fa), 8, None, 5, ip(nn), fp(d2), fp(sec)) == sym.ERR_ARG
    assert f(-1, fp(fa), 8, fp(fb), 5, None, fp(d2), fp(sec)) == sym.ERR_ARG
    for na, nb in ((0, 5), (8, 0), (2 ** 31, 5), (8, 2 ** 31)):
        assert f(-1, fp(fa), na, fp(fb), nb, ip(nn), fp(d2), fp(sec)) == sym.ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for which in (0, 1):
            a, b = fa.copy(), fb.copy()
            (a, b)[which][3, 32] = bad
            assert f(-1, fp(a), 8, fp(b), 5, ip(nn), fp(d2), fp(sec)) == sym.ERR_ARG
    assert L.symmicp_ctx_feature_nn(None, fp(fa), 8, fp(fb), 5, ip(nn), fp(d2), fp(sec)) == sym.ERR_ARG
    with pytest.raises(ValueError):
        sym.feature_nn(fa[:, :32], fb)


def test_feature_correspondences_argument_errors_need_no_device(sym):
    L = sym.lib()
    fa, fb = _features(8, 2), _features(5, 3)
    pairs, d2, cnt = np.zeros((8, 2), np.int32), np.zeros(8, np.float32), C.c_size_t(0)
    f = L.symmicp_feature_correspondences
    t = C.byref(cnt)
    assert f(-1, fp(fa), 8, fp(fb), 5, 1, 0.0, ip(pairs), fp(d2), 8, None) == sym.ERR_ARG
    assert f(-1, fp(fa), 8, fp(fb), 5, 1, 0.0, None, fp(d2), 8, t) == sym.ERR_ARG               # no pairs_out, yet cap > 0
    assert f(-1, fp(fa), 8, fp(fb), 5, 1, float("nan"), ip(pairs), fp(d2), 8, t) == sym.ERR_ARG
    assert f(-1, None, 8, fp(fb), 5, 1, 0.0, ip(pairs), fp(d2), 8, t) == sym.ERR_ARG
    assert f(-1, fp(fa), 8, None, 5, 0, 0.0, ip(pairs), fp(d2), 8, t) == sym.ERR_ARG
    assert f(-1, fp(fa), 0, fp(fb), 5, 1, 0.0, ip(pairs), fp(d2), 8, t) == sym.ERR_ARG
    assert f(-1, fp(fa), 8, fp(fb), 2 ** 31, 1, 0.0, ip(pairs), fp(d2), 8, t) == sym.ERR_ARG
    a = fa.copy(); a[0, 0] = np.inf
    assert f(-1, fp(a), 8, fp(fb), 5, 1, 0.0, ip(pairs), fp(d2), 8, t) == sym.ERR_ARG
    assert L.symmicp_ctx_feature_correspondences(None, fp(fa), 8, fp(fb), 5, 1, 0.0, ip(pairs), fp(d2), 8, t) == sym.ERR_ARG


def _ransac_args(sym, **kw):
    rng = np.random.default_rng(4)
    src, tgt = rng.random((10, 3)).astype(np.float32), rng.random((12, 3)).astype(np.float32)
    pairs = np.stack([np.arange(6), np.arange(6) + 3], 1).astype(np.int32)
    cfg = sym.ransac_config(0.1, hypotheses=64, seed=1)
    for k, v in kw.items():
        setattr(cfg, k, v)
    return src, tgt, pairs, cfg


def test_ransac_argument_errors_need_no_device(sym):
    L = sym.lib()
    T, res = np.zeros(16, np.float32), sym.RansacResult()
    mask, status, inl = np.zeros(6, np.uint8), np.zeros(64, np.uint8), np.zeros(64, np.int32)

    def call(src, tgt, pairs, cfg, ns=None, nt=None, m=None, T=T, res=res, f=L.symmicp_ransac, head=(-1,)):
        return f(*head, None if src is None else fp(src), 3, 1, len(src) if ns is None else ns, None if tgt is None else fp(tgt), 3, 1,
                 len(tgt) if nt is None else nt, None if pairs is None else ip(pairs), len(pairs) if m is None else m,
                 None if cfg is None else C.byref(cfg), None if T is None else fp(T), None if res is None else C.byref(res), up(mask),
                 up(status), ip(inl))

    src, tgt, pairs, cfg = _ransac_args(sym)
    assert call(src, tgt, pairs, cfg, ns=0) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, nt=0) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, ns=2 ** 31) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, m=2) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, m=2 ** 31) == sym.ERR_ARG
    assert call(src, tgt, pairs, None) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, T=None) == sym.ERR_ARG
    assert call(src, tgt, pairs, cfg, res=None) == sym.ERR_ARG
    for name in ("src", "tgt", "pairs"):
        a = dict(src=src, tgt=tgt, pairs=pairs)
        n = len(a[name])
        a[name] = None
        assert call(a["src"], a["tgt"], a["pairs"], cfg, ns=10, nt=12, m=6) == sym.ERR_ARG, (name, n)
    for bad in (dict(struct_size=28), dict(hypotheses=0), dict(hypotheses=2 ** 24 + 1), dict(max_dist=0.0), dict(max_dist=-1.0),
                dict(max_dist=float("inf")), dict(max_dist=float("nan")), dict(edge_ratio=1.0001), dict(edge_ratio=float("nan")),
                dict(refits=-1), dict(refits=9)):
        assert call(*_ransac_args(sym, **bad)) == sym.ERR_ARG, bad
    for row, col, val in ((0, 0, -1), (5, 0, 10), (3, 1, 12), (2, 1, -7)):
        p = pairs.copy()
        p[row, col] = val
        assert call(src, tgt, p, cfg) == sym.ERR_ARG                   # a row outside its cloud
    s = src.copy(); s[pairs[4, 0], 2] = np.nan
    assert call(s, tgt, pairs, cfg) == sym.ERR_ARG                     # a paired point that is not finite
    t = tgt.copy(); t[pairs[1, 1], 0] = np.inf
    assert call(src, t, pairs, cfg) == sym.ERR_ARG
    # the context forms with no context
    assert call(src, tgt, pairs, cfg, f=L.symmicp_ctx_ransac, head=(None,)) == sym.ERR_ARG
    hyp, piv = np.zeros((64, 12), np.float32), np.zeros(6, np.float32)
    assert L.symmicp_ctx_ransac_hypotheses(None, fp(src), 3, 1, 10, fp(tgt), 3, 1, 12, ip(pairs), 6, C.byref(cfg), fp(hyp), up(status),
                                           fp(piv)) == sym.ERR_ARG
    with pytest.raises(ValueError):
        sym.ransac(src, tgt, pairs[:, :1], 0.1)


def test_global_registration_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = sym.lib()
    fa, fb = _features(8, 5), _features(5, 6)
    nn = np.full(8, -7, np.int32)
    assert L.symmicp_feature_nn(-1, fp(fa), 8, fp(fb), 5, ip(nn), None, None) == sym.ERR_HIP
    assert (nn == -7).all()
    with pytest.raises(sym.SymmIcpError) as e:
        sym.feature_nn(fa, fb)
    assert e.value.status == sym.ERR_HIP
    with pytest.raises(sym.SymmIcpError) as e:
        sym.feature_correspondences(fa, fb)
    assert e.value.status == sym.ERR_HIP
    src, tgt, pairs, cfg = _ransac_args(sym)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.ransac(src, tgt, pairs, 0.1, hypotheses=64)
    assert e.value.status == sym.ERR_HIP
    icp = sym.MyICP(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, verbose=False)
    icp.setInputSource(src, src)
    icp.setInputTarget(tgt, tgt)
    icp.setGlobalInit(fpfh_radius=0.5, max_dist=0.1)
    with pytest.raises(sym.SymmIcpError) as e:
        icp.align()
    assert e.value.status == sym.ERR_HIP
