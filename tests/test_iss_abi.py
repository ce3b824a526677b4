"""CPU tests of the C boundary of the ISS keypoints: the header still compiles as pedantic C99, the library exports the entry points,
the configuration struct has the declared size and defaults, and every argument error is returned before a device is needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_iss_keypoints", "symmicp_iss_keypoints"]


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
    missing = [n for n in NEW + ["symmicp_iss_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + ["symmicp_iss_config_default"]) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_iss_config_default(symmicp_iss_config *cfg);" in hdr


def test_config_size_and_defaults(sym):
    assert C.sizeof(sym.IssConfig) == 28
    cfg = sym.IssConfig()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    sym.lib().symmicp_iss_config_default(C.byref(cfg))
    assert cfg.struct_size == 28 and cfg.salient_radius == 0.0 and cfg.non_max_radius == 0.0 and cfg.reserved == 0
    assert cfg.gamma21 == np.float32(0.975) and cfg.gamma32 == np.float32(0.975) and cfg.min_neighbors == 5
    sym.lib().symmicp_iss_config_default(None)          # tolerated
    c2 = sym.iss_config(3.0, 2.0)
    assert (c2.struct_size, c2.salient_radius, c2.non_max_radius, c2.min_neighbors) == (28, 3.0, 2.0, 5)


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that fills the struct and calls the entry points compiles without a warning, links, and gets status codes"""
    src = tmp_path / "iss_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f}, sal[2];
    int32_t rows[2], nb[2];
    size_t count = 0;
    symmicp_iss_config cfg;
    int a, b, c;
    symmicp_iss_config_default(&cfg);
    a = symmicp_iss_keypoints(-1, xyz, 3, 1, 2, &cfg, rows, 2, &count, sal, nb);         /* the radii are still 0 */
    cfg.salient_radius = 1.5f; cfg.non_max_radius = 1.5f; cfg.struct_size = 8;
    b = symmicp_iss_keypoints(-1, xyz, 3, 1, 2, &cfg, rows, 2, &count, sal, nb);
    cfg.struct_size = (uint32_t)sizeof cfg;
    c = symmicp_ctx_iss_keypoints(NULL, xyz, 3, 1, 2, &cfg, rows, 2, &count, sal, nb);
    printf("status %d %d %d size %d gammas %g %g k %d\n", a, b, c, (int)sizeof cfg, cfg.gamma21, cfg.gamma32, (int)cfg.min_neighbors);
    return 0;
}
''')
    exe = tmp_path / "iss_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 size 28 gammas 0.975 0.975 k 5" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    n = len(x)
    rows, sal, nb, count = np.zeros(n, np.int32), np.zeros(n, np.float32), np.zeros(n, np.int32), C.c_size_t(0)
    t = C.byref(count)
    f = L.symmicp_iss_keypoints
    ok = lambda **kw: sym.iss_config(**dict(dict(salient_radius=0.5, non_max_radius=0.4), **kw))
    cfg = C.byref(ok())
    assert f(-1, None, 3, 1, n, cfg, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, n, None, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, n, cfg, ip(rows), n, None, fp(sal), ip(nb)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, n, cfg, None, n, t, fp(sal), ip(nb)) == sym.ERR_ARG                  # NULL rows_out with cap > 0
    assert f(-1, fp(x), 3, 1, 0, cfg, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, 2 ** 31, cfg, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    bad = ok()
    bad.struct_size = 24
    assert f(-1, fp(x), 3, 1, n, C.byref(bad), ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    for key in ("salient_radius", "non_max_radius"):
        for v in (0.0, -1.0, float("inf"), float("-inf"), float("nan")):
            assert f(-1, fp(x), 3, 1, n, C.byref(ok(**{key: v})), ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG, (key, v)
    for key in ("gamma21", "gamma32"):
        for v in (0.0, -0.5, 1.0000001, 2.0, float("inf"), float("nan")):
            assert f(-1, fp(x), 3, 1, n, C.byref(ok(**{key: v})), ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG, (key, v)
    for v in (0, -3):
        assert f(-1, fp(x), 3, 1, n, C.byref(ok(min_neighbors=v)), ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 1] = v
        assert f(-1, fp(y), 3, 1, n, cfg, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    # strided reading: the bad value sits in a column the strides skip / reach
    wide = np.zeros((n, 5), np.float32)
    wide[:, :3] = x
    wide[3, 4] = np.nan
    rows2, count2 = np.zeros(n, np.int32), C.c_size_t(0)          # (with a device this call runs)
    assert f(-1, fp(wide), 5, 1, n, cfg, ip(rows2), n, C.byref(count2), None, None) in (sym.OK, sym.ERR_HIP)
    wide[3, 2] = np.nan
    assert f(-1, fp(wide), 5, 1, n, cfg, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    assert L.symmicp_ctx_iss_keypoints(None, fp(x), 3, 1, n, cfg, ip(rows), n, t, fp(sal), ip(nb)) == sym.ERR_ARG
    # the outputs were never touched
    assert not rows.any() and not sal.any() and not nb.any() and count.value == 0


def test_iss_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.iss_keypoints(x, 0.5, 0.4)
    assert e.value.status == sym.ERR_HIP
