"""CPU tests of the C boundary of the radius search and the FPFH features: the header still compiles as pedantic C99, the library
exports the four entry points, and the argument errors that are decided before a device is needed come back as SYMMICP_ERR_ARG."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_radius_search", "symmicp_radius_search", "symmicp_ctx_fpfh", "symmicp_fpfh"]


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
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the four entry points compiles without a warning, links, and gets status codes, not crashes"""
    src = tmp_path / "fpfh_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f}, nrm[6] = {0.f, 0.f, 1.f, 0.f, 1.f, 0.f}, fpfh[66], spfh[66], d2[2];
    int32_t count[2], rows[2];
    int64_t offs[3];
    size_t total = 0;
    int a, b, c, d;
    a = symmicp_radius_search(-1, xyz, 3, 1, 2, -1.0f, count, offs, rows, d2, 2, &total);
    b = symmicp_fpfh(-1, xyz, 3, 1, NULL, 3, 1, 2, 1.5f, fpfh, spfh, count);
    c = symmicp_ctx_radius_search(NULL, xyz, 3, 1, 2, 1.5f, count, offs, rows, d2, 2, &total);
    d = symmicp_ctx_fpfh(NULL, xyz, 3, 1, nrm, 3, 1, 2, 1.5f, fpfh, spfh, count);
    printf("status %d %d %d %d\n", a, b, c, d);
    return 0;
}
''')
    exe = tmp_path / "fpfh_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1" in r.stdout


def _args(n=16):
    rng = np.random.default_rng(0)
    x = rng.random((n, 3)).astype(np.float32)
    nr = rng.standard_normal((n, 3)).astype(np.float32)
    return x, nr


def test_radius_search_argument_errors_need_no_device(sym):
    L = sym.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    lp = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    x, _ = _args()
    n = len(x)
    count, offs, rows, d2, total = np.zeros(n, np.int32), np.zeros(n + 1, np.int64), np.zeros(64, np.int32), np.zeros(64, np.float32), C.c_size_t(0)
    t = C.byref(total)
    f = L.symmicp_radius_search
    assert f(-1, None, 3, 1, n, 0.5, ip(count), lp(offs), ip(rows), fp(d2), 64, t) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, n, 0.5, None, lp(offs), ip(rows), fp(d2), 64, t) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, n, 0.5, ip(count), lp(offs), ip(rows), fp(d2), 64, None) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, n, 0.5, ip(count), None, ip(rows), fp(d2), 64, t) == sym.ERR_ARG        # rows_out without offsets_out
    assert f(-1, fp(x), 3, 1, 0, 0.5, ip(count), lp(offs), ip(rows), fp(d2), 64, t) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, 2 ** 31, 0.5, ip(count), lp(offs), ip(rows), fp(d2), 64, t) == sym.ERR_ARG
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert f(-1, fp(x), 3, 1, n, bad, ip(count), lp(offs), ip(rows), fp(d2), 64, t) == sym.ERR_ARG
    assert L.symmicp_ctx_radius_search(None, fp(x), 3, 1, n, 0.5, ip(count), lp(offs), ip(rows), fp(d2), 64, t) == sym.ERR_ARG


def test_fpfh_argument_errors_need_no_device(sym):
    L = sym.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x, nr = _args()
    n = len(x)
    out, sp, count = np.zeros((n, 33), np.float32), np.zeros((n, 33), np.float32), np.zeros(n, np.int32)
    f = L.symmicp_fpfh
    assert f(-1, None, 3, 1, fp(nr), 3, 1, n, 0.5, fp(out), fp(sp), ip(count)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, None, 3, 1, n, 0.5, fp(out), fp(sp), ip(count)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, fp(nr), 3, 1, n, 0.5, None, fp(sp), ip(count)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, fp(nr), 3, 1, 0, 0.5, fp(out), fp(sp), ip(count)) == sym.ERR_ARG
    assert f(-1, fp(x), 3, 1, fp(nr), 3, 1, 2 ** 31, 0.5, fp(out), fp(sp), ip(count)) == sym.ERR_ARG
    for bad in (0.0, -2.0, float("inf"), float("-inf"), float("nan")):
        assert f(-1, fp(x), 3, 1, fp(nr), 3, 1, n, bad, fp(out), fp(sp), ip(count)) == sym.ERR_ARG
    assert L.symmicp_ctx_fpfh(None, fp(x), 3, 1, fp(nr), 3, 1, n, 0.5, fp(out), fp(sp), ip(count)) == sym.ERR_ARG
    with pytest.raises(ValueError):
        sym.fpfh(x, nr[:-1], 0.5)


def test_fpfh_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    L = sym.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    x, nr = _args()
    out = np.full((len(x), 33), -1.0, np.float32)
    assert L.symmicp_fpfh(-1, fp(x), 3, 1, fp(nr), 3, 1, len(x), 0.5, fp(out), None, None) == sym.ERR_HIP
    assert (out == -1.0).all()
    with pytest.raises(sym.SymmIcpError) as e:
        sym.fpfh(x, nr, 0.5)
    assert e.value.status == sym.ERR_HIP
    with pytest.raises(sym.SymmIcpError) as e:
        sym.radius_search(x, 0.5)
    assert e.value.status == sym.ERR_HIP
