"""The C-ABI of reciprocal correspondences without a GPU: the new symbols resolve, symmicp_inverse_rigid is the numpy restatement bit for
bit, and the header still compiles as pedantic C99."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

import _recip_ref as RR
from conftest import ROOT

f32 = np.float32
NEW = ["symmicp_set_reciprocal", "symmicp_get_reciprocal", "symmicp_get_reciprocal_state", "symmicp_inverse_rigid", "symmicp_ctx_reverse_nn_probe",
       "symmicp_ctx_reciprocal_info"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


def test_the_new_symbols_resolve(sym):
    L = ctypes.CDLL(sym.LIB_PATH)
    assert [n for n in NEW if not hasattr(L, n)] == []
    assert set(NEW) <= set(sym.EXPORTS)
    for name in ("set_reciprocal", "get_reciprocal", "reciprocal_state", "reverse_nn_probe", "reciprocal_info"):
        assert callable(getattr(sym.Engine, name))
    assert callable(sym.MyICP.setReciprocalCorrespondences) and callable(sym.inverse_rigid)


def rigid(rng, scale):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    th = rng.uniform(-math.pi, math.pi)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    X = np.eye(4)
    X[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    X[:3, 3] = rng.normal(size=3) * scale
    return X.astype(f32)


def test_inverse_rigid_equals_the_restatement_bit_for_bit(sym):
    rng = np.random.default_rng(11)
    c = math.cos(math.pi / 4)
    cat = np.array([[c, -c, 0, 2.5], [c, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], f32)      # the cat fixture's Rz(45 deg) + (2.5, 0, 0)
    skew = np.eye(4, dtype=f32)
    skew[:3] = rng.normal(size=(3, 4)).astype(f32) * f32(3)                                # not rigid: the rule is the arithmetic
    skew[3] = [7, -8, 9, 10]                                                                # (the bottom row is ignored)
    cases = [np.eye(4, dtype=f32), cat, skew] + [rigid(rng, s) for s in (0.0, 1.0, 1.0, 100.0, 1e4, 1e-3)]
    for X in cases:
        got = sym.inverse_rigid(X)
        want = RR.inverse_rigid(X)
        assert got.dtype == f32 and got.shape == (3, 4)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (X, got, want)
    assert np.array_equal(sym.inverse_rigid(np.eye(4)), np.eye(4, dtype=f32)[:3])
    m = sym.inverse_rigid(cat)
    assert np.array_equal(m[:, :3], cat[:3, :3].T) and m[0, 3] == f32(-(float(f32(c)) * 2.5)) and m[1, 3] == f32(float(f32(c)) * 2.5) and m[2, 3] == 0
    # for a rigid X it inverts to rounding
    X = cases[4].astype(np.float64)
    M = np.eye(4)
    M[:3] = sym.inverse_rigid(cases[4])
    assert np.abs(M @ X - np.eye(4)).max() < 1e-6
    L = sym.lib()
    out = (ctypes.c_float * 12)()
    assert L.symmicp_inverse_rigid(None, out) == sym.ERR_ARG
    assert L.symmicp_inverse_rigid((ctypes.c_float * 16)(), None) == sym.ERR_ARG


def test_header_compiles_as_pedantic_c99(sym, tmp_path):
    src = tmp_path / "recip.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float X[16], m[12];
    int k, on = 7;
    uint64_t a = 0, b = 0;
    for (k = 0; k < 16; k++) X[k] = (k % 5 == 0) ? 1.f : 0.f;
    X[3] = 2.f;
    if (symmicp_inverse_rigid(X, m) != SYMMICP_OK || m[0] != 1.f || m[3] != -2.f || m[7] != 0.f) return 2;
    if (symmicp_set_reciprocal(NULL, 1) != SYMMICP_ERR_ARG || symmicp_get_reciprocal(NULL, &on) != SYMMICP_ERR_ARG) return 3;
    if (symmicp_get_reciprocal_state(NULL, &a, &b) != SYMMICP_ERR_ARG) return 4;
    if (symmicp_ctx_reciprocal_info(NULL, &on, &a, &b, &a) != SYMMICP_ERR_ARG) return 6;
    if (symmicp_ctx_reverse_nn_probe(NULL, X, NULL, 1, X, 1, NULL, &on, m) != SYMMICP_ERR_ARG) return 5;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "recip_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
