"""CPU tests of the C boundary of the batched alignment: the header still compiles as pedantic C99, the library exports the entry
points, the structs have the declared sizes and defaults, and every argument error is returned before a device is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_batch_align", "symmicp_batch_align"]
f32 = np.float32


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


def test_library_exports_the_new_entry_points(sym):
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW + ["symmicp_batch_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + ["symmicp_batch_config_default"]) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_batch_config_default(symmicp_batch_config *cfg);" in hdr
    assert "#define SYMMICP_BATCH_MAX_POINTS 4096" in hdr and sym.BATCH_MAX_POINTS == 4096


def test_struct_sizes_and_defaults(sym):
    assert C.sizeof(sym.BatchProblem) == 16 and C.sizeof(sym.BatchConfig) == 48 and C.sizeof(sym.BatchResult) == 680
    assert sym.BatchResult.pairs.offset == 352 and sym.BatchResult.sums.offset == 360 and sym.BatchResult.transform.offset == 32
    cfg = sym.BatchConfig()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    sym.lib().symmicp_batch_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.mode, cfg.max_iters, cfg.fixed_iters) == (48, sym.MODE_PAPER, 10, 0)
    assert (cfg.diff_threshold, cfg.max_corr_dist, cfg.min_normal_dot, cfg.eps_rotation, cfg.eps_translation) == (1.0, 0.0, -2.0, 0.0, 0.0)
    assert list(cfg.reserved) == [0, 0, 0]
    sym.lib().symmicp_batch_config_default(None)          # tolerated
    c2 = sym.batch_config(mode=sym.MODE_PLANE, max_iters=3)
    assert (c2.struct_size, c2.mode, c2.max_iters, c2.diff_threshold) == (48, sym.MODE_PLANE, 3, 1.0)
    with pytest.raises(AttributeError):
        sym.batch_config(trim_fraction=0.5)


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that fills the structs and calls the entry points compiles without a warning, links, and gets status codes"""
    src = tmp_path / "batch_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f}, nrm[6] = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f};
    symmicp_batch_problem pb = {0u, 2u, 0u, 3u};                    /* the target range leaves its pool */
    symmicp_batch_config cfg;
    symmicp_batch_result out;
    int a, b, c, d;
    symmicp_batch_config_default(&cfg);
    a = symmicp_batch_align(-1, xyz, nrm, 2, xyz, nrm, 2, &pb, NULL, 1, &cfg, &out, NULL, NULL);
    pb.tgt_count = 2u;
    cfg.struct_size = 8;
    b = symmicp_batch_align(-1, xyz, nrm, 2, xyz, nrm, 2, &pb, NULL, 1, &cfg, &out, NULL, NULL);
    cfg.struct_size = (uint32_t)sizeof cfg;
    c = symmicp_ctx_batch_align(NULL, xyz, nrm, 2, xyz, nrm, 2, &pb, NULL, 1, &cfg, &out, NULL, NULL);
    pb.src_count = SYMMICP_BATCH_MAX_POINTS + 1;
    d = symmicp_batch_align(-1, xyz, nrm, 2, xyz, nrm, 2, &pb, NULL, 1, &cfg, &out, NULL, NULL);
    printf("status %d %d %d %d sizes %d %d %d mode %d iters %d\n", a, b, c, d, (int)sizeof pb, (int)sizeof cfg, (int)sizeof out,
           (int)cfg.mode, (int)cfg.max_iters);
    return 0;
}
''')
    exe = tmp_path / "batch_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 2 sizes 16 48 680 mode 1 iters 10" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    rng = np.random.default_rng(0)
    n = 32
    sx, tx = rng.random((n, 3)).astype(f32), rng.random((n, 3)).astype(f32)
    sn = np.tile(np.array([[0, 0, 1]], f32), (n, 1))
    tn = sn.copy()
    out = (sym.BatchResult * 4)()
    C.memset(out, 0, C.sizeof(out))

    def call(src=sx, srcn=sn, ns=n, tgt=tx, tgtn=tn, nt=n, problems=((0, n, 0, n),), B=None, cfg=None, guess=None, res=out, **kw):
        probs, nb = (None, 0) if problems is None else sym.batch_problems(problems)
        c = sym.batch_config(**kw) if cfg is None else cfg
        return L.symmicp_batch_align(-1, fp(src), fp(srcn), ns, fp(tgt), fp(tgtn), nt, probs, fp(guess), nb if B is None else B,
                                     None if c is False else C.byref(c), res, None, None)

    ARG, SIZE = sym.ERR_ARG, sym.ERR_SIZE
    # NULL pools, problems, cfg, out
    assert call(src=None) == ARG and call(tgt=None) == ARG and call(tgtn=None) == ARG
    assert call(problems=None, B=1) == ARG and call(cfg=False) == ARG and call(res=None) == ARG
    # struct_size, mode
    bad = sym.batch_config()
    bad.struct_size = 44
    assert call(cfg=bad) == ARG
    for mode in (sym.MODE_QUIRKS, sym.MODE_GICP, sym.MODE_COLOR, 4, 6, -1, 8):
        assert call(mode=mode) == ARG, mode
    # B
    assert call(B=0) == ARG and call(B=2 ** 20 + 1) == ARG
    # counts, ranges
    assert call(problems=((0, 0, 0, n),)) == ARG and call(problems=((0, n, 0, 0),)) == ARG
    assert call(problems=((0, n, 0, n), (1, n, 0, n))) == ARG and call(problems=((0, n, n, 1),)) == ARG
    assert call(problems=((2 ** 32 - 1, 2, 0, n),)) == ARG                    # first + count does not wrap
    assert call(problems=((0, 4097, 0, n),)) == SIZE and call(problems=((0, n, 0, 4097),)) == SIZE
    assert call(problems=((0, n, 0, n), (0, 5000, 0, n))) == SIZE
    # max_iters, thresholds
    assert call(max_iters=-1) == ARG and call(max_iters=1001) == ARG
    for key in ("diff_threshold", "max_corr_dist", "min_normal_dot", "eps_rotation", "eps_translation"):
        for v in (float("nan"), float("inf"), float("-inf")):
            assert call(**{key: v}) == ARG, (key, v)
    # NULL source normals: PLANE only, and not with the normal gate
    assert call(srcn=None) == ARG and call(srcn=None, mode=sym.MODE_P2P) == ARG
    assert call(srcn=None, mode=sym.MODE_PLANE, min_normal_dot=0.5) == ARG
    # a non-finite coordinate in a row some problem uses -- and only there
    for v in (np.nan, np.inf, -np.inf):
        for which in ("src", "tgt", "srcn", "tgtn"):
            arrs = dict(src=sx.copy(), tgt=tx.copy(), srcn=sn.copy(), tgtn=tn.copy())
            arrs[which][7, 1] = v
            assert call(**arrs) == ARG, (which, v)
            assert call(problems=((8, n - 8, 8, n - 8), (0, 7, 0, 7)), **arrs) in (sym.OK, sym.ERR_HIP), (which, v)      # row 7 is not used
            assert call(problems=((8, n - 8, 8, n - 8), (0, 8, 0, 8)), **arrs) == ARG, (which, v)
    assert L.symmicp_ctx_batch_align(None, fp(sx), fp(sn), n, fp(tx), fp(tn), n, sym.batch_problems(((0, n, 0, n),))[0], None, 1,
                                     C.byref(sym.batch_config()), out, None, None) == ARG
    # the outputs were never touched
    assert bytes(out) == bytes(C.sizeof(out))


def test_size_error_names_the_limit(sym):
    """through a context the message is readable: without a device there is none, so this reads the library's text"""
    blob = open(sym.LIB_PATH, "rb").read()
    assert b"SYMMICP_BATCH_MAX_POINTS = " in blob


def test_batch_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((16, 3)).astype(f32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.batch_align(x, x, x, x, [(0, 16, 0, 16)])
    assert e.value.status == sym.ERR_HIP


def test_myicp_multistart_refusals_need_no_device(sym):
    """MyICP.alignMultiStart returns the batch call's error for a mode outside the three, for clouds above the limit and for no
    guesses: decided before any device, no fallback to a loop of align calls"""
    x = np.random.default_rng(0).random((16, 3)).astype(f32)
    big = np.random.default_rng(1).random((sym.BATCH_MAX_POINTS + 1, 3)).astype(f32)
    for mode, src, guesses, want in ((sym.MODE_QUIRKS, x, np.eye(4, dtype=f32)[None], sym.ERR_ARG),
                                     (sym.MODE_GICP, x, np.eye(4, dtype=f32)[None], sym.ERR_ARG),
                                     (sym.MODE_PAPER, big, np.eye(4, dtype=f32)[None], sym.ERR_SIZE),
                                     (sym.MODE_PAPER, x, np.zeros((0, 4, 4), f32), sym.ERR_ARG)):
        m = sym.MyICP(mode=mode, verbose=False)
        m.setInputSource(src, src)
        m.setInputTarget(x, x)
        with pytest.raises(sym.SymmIcpError) as e:
            m.alignMultiStart(guesses)
        assert e.value.status == want, (mode, len(src), len(guesses))
        assert m.multiStartResults() == [] and np.array_equal(m.getFinalTransformation(), np.eye(4, dtype=f32))
