"""CPU tests of the C boundary of the outlier filters: the header still compiles as pedantic C99, the library exports the entry points,
and every argument error is returned before a device is needed, with the outputs untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_statistical_outlier_removal", "symmicp_statistical_outlier_removal", "symmicp_ctx_radius_outlier_removal",
       "symmicp_radius_outlier_removal"]


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
    for name in ("remove_statistical_outlier", "remove_radius_outlier"):
        assert callable(getattr(sym, name)) and callable(getattr(sym.Engine, name)) and callable(getattr(sym.Engine, name + "_raw"))
    for name in ("removeStatisticalOutliers", "removeRadiusOutliers", "outliersRemoved"):
        assert callable(getattr(sym.MyICP, name))
        assert name in open(os.path.join(ROOT, "include", "myicp.h")).read()


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the four entry points compiles without a warning, links, and gets SYMMICP_ERR_ARG from each"""
    src = tmp_path / "outlier_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f};
    int32_t rows[2], nb[2];
    double md[2], stats[3];
    size_t count = 0;
    int a, b, c, d;
    a = symmicp_statistical_outlier_removal(-1, xyz, 3, 1, 2, 2, 1.0f, rows, 2, &count, md, stats);     /* k > n - 1 */
    b = symmicp_ctx_statistical_outlier_removal(NULL, xyz, 3, 1, 2, 1, 1.0f, rows, 2, &count, md, stats);
    c = symmicp_radius_outlier_removal(-1, xyz, 3, 1, 2, 0.0f, 1, rows, 2, &count, nb);                 /* radius 0 */
    d = symmicp_ctx_radius_outlier_removal(NULL, xyz, 3, 1, 2, 1.5f, 1, rows, 2, &count, nb);
    printf("status %d %d %d %d count %d\n", a, b, c, d, (int)count);
    return 0;
}
''')
    exe = tmp_path / "outlier_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 count 0" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    assert sym.ERR_ARG == 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    n = len(x)
    rows, md, st3, nb, count = np.zeros(n, np.int32), np.zeros(n), np.zeros(3), np.zeros(n, np.int32), C.c_size_t(0)
    t = C.byref(count)
    inf, nan = float("inf"), float("nan")

    def sor(xyz=x, xr=3, xc=1, n_=n, k=4, mul=1.0, rows_=rows, cap=n, cnt=t):
        return L.symmicp_statistical_outlier_removal(-1, None if xyz is None else fp(xyz), xr, xc, n_, k, mul, None if rows_ is None else ip(rows_),
                                                     cap, cnt, dp(md), dp(st3))

    def ror(xyz=x, xr=3, xc=1, n_=n, radius=0.5, mn=2, rows_=rows, cap=n, cnt=t):
        return L.symmicp_radius_outlier_removal(-1, None if xyz is None else fp(xyz), xr, xc, n_, radius, mn, None if rows_ is None else ip(rows_),
                                                cap, cnt, ip(nb))

    for f in (sor, ror):
        assert f(xyz=None) == sym.ERR_ARG
        assert f(cnt=None) == sym.ERR_ARG
        assert f(rows_=None) == sym.ERR_ARG                      # NULL rows_out with cap > 0
        assert f(n_=0) == sym.ERR_ARG
        assert f(n_=2 ** 31) == sym.ERR_ARG
        for v in (np.nan, np.inf, -np.inf):
            y = x.copy()
            y[7, 1] = v
            assert f(xyz=y) == sym.ERR_ARG
    for k in (0, -1, 65, 1000, n):                                # k outside 1 .. 64, or above n - 1 = 15
        assert sor(k=k) == sym.ERR_ARG, k
    assert sor(xyz=x[:1], n_=1, k=1) == sym.ERR_ARG               # one point has no neighbour
    for v in (inf, -inf, nan):
        assert sor(mul=v) == sym.ERR_ARG
    for v in (0.0, -1.0, inf, -inf, nan):
        assert ror(radius=v) == sym.ERR_ARG, v
    for v in (0, -3):
        assert ror(mn=v) == sym.ERR_ARG
    # strided reading: the bad value sits in a column the strides skip / reach
    wide = np.zeros((n, 5), np.float32)
    wide[:, :3] = x
    wide[3, 4] = np.nan
    rows2, count2 = np.zeros(n, np.int32), C.c_size_t(0)          # (with a device these calls run)
    assert sor(xyz=wide, xr=5, rows_=rows2, cnt=C.byref(count2)) in (sym.OK, sym.ERR_HIP)
    assert ror(xyz=wide, xr=5, rows_=rows2, cnt=C.byref(count2)) in (sym.OK, sym.ERR_HIP)
    wide[3, 2] = np.nan
    assert sor(xyz=wide, xr=5) == sym.ERR_ARG and ror(xyz=wide, xr=5) == sym.ERR_ARG
    assert L.symmicp_ctx_statistical_outlier_removal(None, fp(x), 3, 1, n, 4, 1.0, ip(rows), n, t, dp(md), dp(st3)) == sym.ERR_ARG
    assert L.symmicp_ctx_radius_outlier_removal(None, fp(x), 3, 1, n, 0.5, 2, ip(rows), n, t, ip(nb)) == sym.ERR_ARG
    # the outputs were never touched
    assert not rows.any() and not md.any() and not st3.any() and not nb.any() and count.value == 0


def test_filters_fail_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.remove_statistical_outlier(x, 4, 1.0)
    assert e.value.status == sym.ERR_HIP
    with pytest.raises(sym.SymmIcpError) as e:
        sym.remove_radius_outlier(x, 0.5, 2)
    assert e.value.status == sym.ERR_HIP
