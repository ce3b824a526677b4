"""CPU tests of the C boundary of the index test entries (symmicp_ctx_index_info / _index_arrays / _source_share / _radix_sort_probe /
_scan_probe): the header still compiles as pedantic C99, the library exports them and symmicp.EXPORTS lists them, the argument
errors that are decided before a device is needed come back as SYMMICP_ERR_ARG, and without a device nothing pretends to work."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_index_info", "symmicp_ctx_index_arrays", "symmicp_ctx_source_share", "symmicp_ctx_radix_sort_probe",
       "symmicp_ctx_scan_probe"]


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
    assert L.symmicp_version() == 100


def test_info_struct_matches_the_binding(sym, tmp_path):
    """sizeof and the offset of the last field, as a C compiler lays the struct out"""
    src = tmp_path / "info_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "symmicp.h"\nint main(void) { printf("%d %d %d\\n", '
                   '(int)sizeof(symmicp_index_info), (int)offsetof(symmicp_index_info, level_hist), (int)offsetof(symmicp_index_info, olevel_off)); return 0; }\n')
    exe = tmp_path / "info_size"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(sym.IndexInfo), sym.IndexInfo.level_hist.offset, sym.IndexInfo.olevel_off.offset]


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the five entries compiles without a warning, links, and gets status codes, not crashes"""
    src = tmp_path / "index_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    symmicp_index_info info;
    uint32_t keys[4] = {3, 1, 2, 0}, vals[4] = {0, 1, 2, 3};
    size_t nl = 0, np = 0;
    int32_t so = 0, ck = 0;
    int a, b, c, d, e;
    info.struct_size = (int32_t)sizeof(info);
    a = symmicp_ctx_index_info(NULL, &info);
    b = symmicp_ctx_index_arrays(NULL, NULL, NULL, NULL, NULL, NULL, NULL);
    c = symmicp_ctx_source_share(NULL, &nl, &np, &so, &ck, NULL, NULL);
    d = symmicp_ctx_radix_sort_probe(NULL, keys, vals, 4, 30);
    e = symmicp_ctx_scan_probe(NULL, keys, 4);
    printf("status %d %d %d %d %d version %d\n", a, b, c, d, e, symmicp_version());
    return 0;
}
''')
    exe = tmp_path / "index_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 1 version 100" in r.stdout


def test_null_context_is_an_argument_error(sym):
    L = sym.lib()
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    k, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32)
    info = sym.IndexInfo()
    info.struct_size = C.sizeof(sym.IndexInfo)
    assert L.symmicp_ctx_index_info(None, C.byref(info)) == sym.ERR_ARG
    assert L.symmicp_ctx_index_arrays(None, None, None, None, None, None, None) == sym.ERR_ARG
    assert L.symmicp_ctx_source_share(None, None, None, None, None, None, None) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(None, u(k), u(v), 8, 30) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(None, u(k), u(v), 0, 30) == sym.ERR_ARG
    assert L.symmicp_ctx_scan_probe(None, u(k), 8) == sym.ERR_ARG
    assert (k == np.arange(8)).all() and (v == np.arange(8)).all()


def test_entries_fail_loudly_without_gpu(sym):
    """no device: a context cannot be made (SYMMICP_ERR_HIP), so no probe can run on the host instead"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sym.SymmIcpError) as e:
        sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE)
    assert e.value.status == sym.ERR_HIP
    for name in ("index_info", "index_arrays", "source_share", "radix_sort_probe", "scan_probe"):
        assert callable(getattr(sym.Engine, name))
