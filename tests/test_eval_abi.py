"""CPU tests of the C boundary of registration evaluation: the library exports the entry points, symmicp_evaluation has the size of
its ctypes mirror, symmicp_information_from_sums is the reference's closed form bit for bit, every argument error of
symmicp_evaluate_registration is returned before a device is needed, and the header still compiles as pedantic C99."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _eval_ref as E
from conftest import ROOT

NEW = ["symmicp_information_from_sums", "symmicp_evaluate_registration", "symmicp_ctx_evaluate_registration", "symmicp_evaluate"]


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
    assert "} symmicp_evaluation;" in hdr


def test_struct_size_matches_the_mirror(sym, tmp_path):
    assert C.sizeof(sym.Evaluation) == 8 * (1 + 3 + 1 + 3 + 6 + 36) == 400
    src = tmp_path / "eval_size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "symmicp.h"\nint main(void) { printf("%d %d %d\\n", (int)sizeof(symmicp_evaluation), '
                   '(int)offsetof(symmicp_evaluation, sum_q), (int)offsetof(symmicp_evaluation, information)); return 0; }\n')
    exe = tmp_path / "eval_size"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(v) for v in out] == [C.sizeof(sym.Evaluation), sym.Evaluation.sum_q.offset, sym.Evaluation.information.offset]


def test_information_from_sums_is_the_reference_bit_for_bit(sym):
    rng = np.random.default_rng(5)
    for _ in range(200):
        n = int(rng.integers(0, 1 << 40))
        s = rng.normal(size=3) * 10.0 ** rng.integers(-5, 8)
        S = rng.normal(size=6) * 10.0 ** rng.integers(-5, 12)
        got, want = sym.information_from_sums(n, s, S), E.information_from_sums(n, s, S)
        assert got.shape == (6, 6) and got.dtype == np.float64
        assert got.tobytes() == want.tobytes()
    z = sym.information_from_sums(0, np.zeros(3), np.zeros(6))
    assert z.tobytes() == E.information_from_sums(0, np.zeros(3), np.zeros(6)).tobytes()
    dp = C.POINTER(C.c_double)
    buf = np.zeros(36)
    assert sym.lib().symmicp_information_from_sums(1, None, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp)) == sym.ERR_ARG
    assert sym.lib().symmicp_information_from_sums(1, buf.ctypes.data_as(dp), None, buf.ctypes.data_as(dp)) == sym.ERR_ARG
    assert sym.lib().symmicp_information_from_sums(1, buf.ctypes.data_as(dp), buf.ctypes.data_as(dp), None) == sym.ERR_ARG


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    fp = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rng = np.random.default_rng(0)
    s, t = rng.random((16, 3)).astype(np.float32), rng.random((12, 3)).astype(np.float32)
    ns, nt = len(s), len(t)
    X = np.tile(np.eye(4, dtype=np.float32).reshape(1, 16), (3, 1))
    out = (sym.Evaluation * 4)()
    nn, d2 = np.zeros((3, ns), np.int32), np.zeros((3, ns), np.float32)
    f = L.symmicp_evaluate_registration

    def call(src=s, ns_=ns, tgt=t, nt_=nt, X_=X, K=3, dist=0.5, out_=out):
        return f(-1, fp(src), 3, 1, ns_, fp(tgt), 3, 1, nt_, fp(X_), K, dist, out_, ip(nn), fp(d2))

    assert call(src=None) == sym.ERR_ARG
    assert call(tgt=None) == sym.ERR_ARG
    assert call(out_=None) == sym.ERR_ARG
    for bad in (0, 2 ** 31):
        assert call(ns_=bad) == sym.ERR_ARG
        assert call(nt_=bad) == sym.ERR_ARG
    for K in (0, 4097, 2 ** 40):
        assert call(K=K) == sym.ERR_ARG
    for K in (0, 2, 3):
        assert call(X_=None, K=K) == sym.ERR_ARG                  # NULL X16 means K == 1
    for v in (np.nan, np.inf, -np.inf):
        for k, e in ((0, 0), (1, 7), (2, 11)):                     # any X_k, any entry of the top three rows
            Y = X.copy()
            Y[k, e] = v
            assert call(X_=Y) == sym.ERR_ARG, (v, k, e)
        assert call(dist=v) == sym.ERR_ARG
        y = s.copy()
        y[7, 1] = v
        assert call(src=y) == sym.ERR_ARG
        y = t.copy()
        y[11, 2] = v
        assert call(tgt=y) == sym.ERR_ARG
    # the bottom row is ignored: a non-finite entry there is no argument error (with a device this call runs)
    Y = X.copy()
    Y[1, 13] = np.nan
    assert call(X_=Y) in (sym.OK, sym.ERR_HIP)
    # strided reading: the bad value sits in a column the strides skip / reach
    wide = np.zeros((ns, 5), np.float32)
    wide[:, :3] = s
    wide[3, 4] = np.nan
    assert f(-1, fp(wide), 5, 1, ns, fp(t), 3, 1, nt, fp(X), 3, 0.5, out, None, None) in (sym.OK, sym.ERR_HIP)
    wide[3, 2] = np.nan
    assert f(-1, fp(wide), 5, 1, ns, fp(t), 3, 1, nt, fp(X), 3, 0.5, out, None, None) == sym.ERR_ARG
    # the context forms refuse a NULL context the same way
    assert L.symmicp_ctx_evaluate_registration(None, fp(s), 3, 1, ns, fp(t), 3, 1, nt, fp(X), 3, 0.5, out, None, None) == sym.ERR_ARG
    assert L.symmicp_evaluate(None, fp(X), 3, 0.5, out, None, None) == sym.ERR_ARG
    import torch
    if not torch.cuda.is_available():
        assert not nn.any() and not d2.any()                       # the outputs were never touched
        with pytest.raises(sym.SymmIcpError) as e:                 # valid arguments and no device: no CPU fallback
            sym.evaluate_registration(s, t, X.reshape(3, 4, 4), 0.5)
        assert e.value.status == sym.ERR_HIP


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets status codes and the closed form"""
    src = tmp_path / "eval_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float s[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f}, t[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f}, d2[2];
    float X[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    double q[3] = {1.0, 2.0, 3.0}, qq[6] = {1.0, 2.0, 3.0, 4.0, 6.0, 9.0}, L[36];
    int32_t nn[2];
    symmicp_evaluation e;
    int a, b, c, d;
    a = symmicp_evaluate_registration(-1, s, 3, 1, 2, t, 3, 1, 2, X, 0, 0.5f, &e, nn, d2);       /* K == 0 */
    b = symmicp_ctx_evaluate_registration(NULL, s, 3, 1, 2, t, 3, 1, 2, X, 1, 0.5f, &e, nn, d2);
    c = symmicp_evaluate(NULL, X, 1, 0.5f, &e, nn, d2);
    d = symmicp_information_from_sums(1, q, qq, L);
    printf("status %d %d %d %d size %d L %g %g %g %g %g\n", a, b, c, d, (int)sizeof e, L[0], L[1], L[4], L[19], L[35]);
    return 0;
}
''')
    exe = tmp_path / "eval_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 0 size 400 L 13 -2 -3 3 1" in r.stdout
