"""CPU tests of the C boundary of trimmed ICP (symmicp_set_trim_fraction / _get_trim_fraction / _get_trim_state /
symmicp_ctx_select_probe): the library exports them, the header declares them and still compiles as pedantic C99, symmicp.EXPORTS
lists them, and a NULL context is SYMMICP_ERR_ARG."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_set_trim_fraction", "symmicp_get_trim_fraction", "symmicp_get_trim_state", "symmicp_ctx_select_probe"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


def test_library_exports_the_trim_entry_points(sym):
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    for name in ("set_trim_fraction", "trim_fraction", "trim_state", "select_probe"):
        assert callable(getattr(sym.Engine, name))
    assert callable(sym.MyICP.setTrimFraction)


def test_header_with_the_trim_declarations_is_pedantic_c99(sym, tmp_path):
    src = tmp_path / "trim_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    uint32_t keys[4] = {3, 1, 2, 0}, kth = 0;
    uint64_t nc = 0, kept = 0, nle = 0;
    float f = 0.0f, tau = 0.0f;
    int a, b, c, d;
    a = symmicp_set_trim_fraction(NULL, 0.5f);
    b = symmicp_get_trim_fraction(NULL, &f);
    c = symmicp_get_trim_state(NULL, &nc, &kept, &tau);
    d = symmicp_ctx_select_probe(NULL, keys, 4, 2, &kth, &nle);
    printf("status %d %d %d %d version %d\n", a, b, c, d, symmicp_version());
    return 0;
}
''')
    exe = tmp_path / "trim_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 version 100" in r.stdout


def test_null_context_is_an_argument_error(sym):
    L = sym.lib()
    k = np.arange(8, dtype=np.uint32)
    kth, nle, nc, kept = C.c_uint32(7), C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    f = C.c_float(7)
    assert L.symmicp_set_trim_fraction(None, 0.5) == sym.ERR_ARG
    assert L.symmicp_get_trim_fraction(None, C.byref(f)) == sym.ERR_ARG
    assert L.symmicp_get_trim_state(None, C.byref(nc), C.byref(kept), C.byref(f)) == sym.ERR_ARG
    assert L.symmicp_ctx_select_probe(None, k.ctypes.data_as(C.POINTER(C.c_uint32)), 8, 3, C.byref(kth), C.byref(nle)) == sym.ERR_ARG
    assert (kth.value, nle.value, nc.value, kept.value, f.value) == (7, 7, 7, 7, 7.0)
    assert (k == np.arange(8)).all()


def test_entries_fail_loudly_without_gpu(sym):
    """no device: a context cannot be made (SYMMICP_ERR_HIP), so nothing trims or selects on the host instead"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sym.SymmIcpError) as e:
        sym.Engine(mode=sym.MODE_PLANE, corr=sym.CORR_TREE)
    assert e.value.status == sym.ERR_HIP
