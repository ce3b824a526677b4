"""CPU tests of the C boundary of the one-to-one and median-distance rejectors (symmicp_set_one_to_one / _get_one_to_one /
_set_median_factor / _get_median_factor / _get_rejection_state / symmicp_ctx_unique_probe): the library exports them, the header
declares them and still compiles as pedantic C99, symmicp.EXPORTS lists them, and a NULL context is SYMMICP_ERR_ARG."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_set_one_to_one", "symmicp_get_one_to_one", "symmicp_set_median_factor", "symmicp_get_median_factor",
       "symmicp_get_rejection_state", "symmicp_ctx_unique_probe"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


def test_library_exports_the_rejector_entry_points(sym):
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    for name in ("set_one_to_one", "one_to_one", "set_median_factor", "median_factor", "rejection_state", "unique_probe"):
        assert callable(getattr(sym.Engine, name))
    assert callable(sym.MyICP.setOneToOne) and callable(sym.MyICP.setMedianFactor)
    cls = open(os.path.join(ROOT, "include", "myicp.h")).read()
    assert "void setOneToOne(bool" in cls and "void setMedianFactor(float" in cls


def test_header_with_the_rejector_declarations_is_pedantic_c99(sym, tmp_path):
    src = tmp_path / "reject_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    int32_t rows[4] = {0, 0, -1, 1};
    uint32_t d2[4] = {3, 1, 2, 0};
    uint8_t win[4] = {9, 9, 9, 9};
    uint64_t nc = 0, nu = 0, kept = 0;
    float f = 0.0f, tau = 0.0f;
    int on = 0, a, b, c, d, e, g;
    a = symmicp_set_one_to_one(NULL, 1);
    b = symmicp_get_one_to_one(NULL, &on);
    c = symmicp_set_median_factor(NULL, 2.0f);
    d = symmicp_get_median_factor(NULL, &f);
    e = symmicp_get_rejection_state(NULL, &nc, &nu, &kept, &tau);
    g = symmicp_ctx_unique_probe(NULL, rows, d2, 4, 2, win);
    printf("status %d %d %d %d %d %d version %d\n", a, b, c, d, e, g, symmicp_version());
    return 0;
}
''')
    exe = tmp_path / "reject_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 1 1 version 100" in r.stdout
    assert sym.ERR_ARG == 1


def test_null_context_is_an_argument_error(sym):
    L = sym.lib()
    rows = np.array([0, 0, -1, 1], np.int32)
    d2 = np.array([3, 1, 2, 0], np.uint32)
    win = np.full(4, 7, np.uint8)
    nc, nu, kept = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    f, on = C.c_float(7), C.c_int(7)
    assert L.symmicp_set_one_to_one(None, 1) == sym.ERR_ARG
    assert L.symmicp_get_one_to_one(None, C.byref(on)) == sym.ERR_ARG
    assert L.symmicp_set_median_factor(None, 2.0) == sym.ERR_ARG
    assert L.symmicp_get_median_factor(None, C.byref(f)) == sym.ERR_ARG
    assert L.symmicp_get_rejection_state(None, C.byref(nc), C.byref(nu), C.byref(kept), C.byref(f)) == sym.ERR_ARG
    assert L.symmicp_ctx_unique_probe(None, rows.ctypes.data_as(C.POINTER(C.c_int32)), d2.ctypes.data_as(C.POINTER(C.c_uint32)), 4, 2,
                                      win.ctypes.data_as(C.POINTER(C.c_uint8))) == sym.ERR_ARG
    assert (on.value, nc.value, nu.value, kept.value, f.value) == (7, 7, 7, 7, 7.0)
    assert (win == 7).all() and rows.tolist() == [0, 0, -1, 1] and d2.tolist() == [3, 1, 2, 0]

