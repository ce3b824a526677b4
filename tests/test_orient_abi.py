"""CPU tests of the C boundary of the normal orientation: the header still compiles as pedantic C99, the library exports the entry
points, the config default and the struct sizes are what the header says, and every argument error of the header is returned before a
device is needed, with the outputs untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_orient_normals", "symmicp_orient_normals"]


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
    missing = [n for n in NEW + ["symmicp_orient_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + ["symmicp_orient_config_default"]) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_orient_config_default(" in hdr
    assert "SYMMICP_ERR_INTERNAL = 9" in hdr and sym.ERR_INTERNAL == 9
    assert "SYMMICP_ORIENT_VIEWPOINT = 0, SYMMICP_ORIENT_DIRECTION = 1" in hdr and (sym.ORIENT_VIEWPOINT, sym.ORIENT_DIRECTION) == (0, 1)
    assert callable(sym.orient_normals) and callable(sym.orient_config)
    assert callable(sym.Engine.orient_normals) and callable(sym.Engine.orient_normals_raw)
    myicp = open(os.path.join(ROOT, "include", "myicp.h")).read()
    assert callable(sym.MyICP.setOrientNormals) and "setOrientNormals" in myicp and "orient_k" in myicp


def test_config_default_and_struct_sizes(sym):
    assert C.sizeof(sym.OrientConfig) == 24 and C.sizeof(sym.OrientResult) == 48
    cfg = sym.OrientConfig()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    sym.lib().symmicp_orient_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.k, cfg.seed_rule, list(cfg.ref)) == (24, 16, sym.ORIENT_VIEWPOINT, [0.0, 0.0, 0.0])
    sym.lib().symmicp_orient_config_default(None)                  # tolerated
    cfg = sym.orient_config(7, viewpoint=(1, 2, 3))
    assert (cfg.struct_size, cfg.k, cfg.seed_rule, list(cfg.ref)) == (24, 7, sym.ORIENT_VIEWPOINT, [1.0, 2.0, 3.0])
    cfg = sym.orient_config(5, direction=(0, 0, 1))
    assert (cfg.k, cfg.seed_rule, list(cfg.ref)) == (5, sym.ORIENT_DIRECTION, [0.0, 0.0, 1.0])
    with pytest.raises(ValueError):
        sym.orient_config(5, viewpoint=(0, 0, 0), direction=(0, 0, 1))


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets SYMMICP_ERR_ARG from each"""
    src = tmp_path / "orient_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f}, nrm[9] = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 0.f, 0.f, -1.f}, out[9] = {7.f};
    uint8_t flip[3] = {9, 9, 9};
    int32_t comp[3] = {7, 7, 7}, tree[4];
    size_t count = 5;
    symmicp_orient_config cfg;
    symmicp_orient_result res;
    int a, b, c;
    symmicp_orient_config_default(&cfg);
    a = symmicp_orient_normals(-1, xyz, 3, 1, nrm, 3, 1, 3, &cfg, out, flip, comp, tree, &count, &res);            /* k 16 > n */
    cfg.k = 3;
    b = symmicp_ctx_orient_normals(NULL, xyz, 3, 1, nrm, 3, 1, 3, &cfg, out, flip, comp, tree, &count, &res);
    cfg.seed_rule = SYMMICP_ORIENT_DIRECTION;
    c = symmicp_orient_normals(-1, xyz, 3, 1, nrm, 3, 1, 3, &cfg, out, flip, comp, tree, &count, &res);            /* zero direction */
    printf("status %d %d %d size %d %d default %d count %d out %d flip %d comp %d\n", a, b, c, (int)sizeof(cfg), (int)sizeof(res),
           (int)cfg.struct_size, (int)count, (int)out[0], (int)flip[0], (int)comp[0]);
    return 0;
}
''')
    exe = tmp_path / "orient_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 size 24 48 default 24 count 5 out 7 flip 9 comp 7" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    assert sym.ERR_ARG == 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rng = np.random.default_rng(0)
    x, nr = rng.random((20, 3)).astype(np.float32), rng.normal(size=(20, 3)).astype(np.float32)
    n = len(x)
    out, flip, comp, tree = np.zeros((n, 3), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros((n, 2), np.int32)
    count, res = C.c_size_t(0), sym.OrientResult()
    inf, nan = float("inf"), float("nan")

    def run(xyz=x, xr=3, nrm=nr, nrs=3, n_=n, k=6, viewpoint=None, direction=None, out_=out, tree_=tree, cnt=C.byref(count), struct_size=None,
            seed_rule=None, no_cfg=False, one_shot=True):
        c = sym.orient_config(k, viewpoint, direction)
        if struct_size is not None:
            c.struct_size = struct_size
        if seed_rule is not None:
            c.seed_rule = seed_rule
        fn, head = (L.symmicp_orient_normals, -1) if one_shot else (L.symmicp_ctx_orient_normals, None)
        return fn(head, None if xyz is None else fp(xyz), xr, 1, None if nrm is None else fp(nrm), nrs, 1, n_, None if no_cfg else C.byref(c),
                  None if out_ is None else fp(out_), flip.ctypes.data_as(C.POINTER(C.c_uint8)), ip(comp), None if tree_ is None else ip(tree_), cnt,
                  C.byref(res))

    assert run(xyz=None) == sym.ERR_ARG
    assert run(nrm=None) == sym.ERR_ARG
    assert run(no_cfg=True) == sym.ERR_ARG
    assert run(out_=None) == sym.ERR_ARG
    assert run(cnt=None) == sym.ERR_ARG                            # tree_out without tree_count
    assert run(n_=0) == sym.ERR_ARG
    assert run(n_=2 ** 31) == sym.ERR_ARG
    for v in (0, 20, 28):
        assert run(struct_size=v) == sym.ERR_ARG
    for v in (-1, 0, 2, 17, 21, 2 ** 31 - 1):
        assert run(k=v) == sym.ERR_ARG, v
    assert run(k=6, n_=5) == sym.ERR_ARG                           # k above n
    for v in (-1, 2, 7):
        assert run(seed_rule=v) == sym.ERR_ARG, v
    for v in (inf, -inf, nan):
        assert run(viewpoint=(0.0, v, 0.0)) == sym.ERR_ARG
        assert run(direction=(0.0, 1.0, v)) == sym.ERR_ARG
    assert run(direction=(0.0, 0.0, 0.0)) == sym.ERR_ARG
    assert run(direction=(0.0, -0.0, 0.0)) == sym.ERR_ARG
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 1] = v
        assert run(xyz=y) == sym.ERR_ARG
        y = nr.copy()
        y[19, 2] = v
        assert run(nrm=y) == sym.ERR_ARG
    # strided reading: the bad value sits in a column the strides skip / reach
    wide = np.zeros((n, 5), np.float32)
    wide[:, :3] = nr
    wide[3, 4] = np.nan
    out2, count2 = np.zeros((n, 3), np.float32), C.c_size_t(0)                                      # (with a device these calls run)
    assert run(nrm=wide, nrs=5, out_=out2, cnt=C.byref(count2), tree_=None) in (sym.OK, sym.ERR_HIP)
    assert run(k=3, out_=out2, cnt=None, tree_=None) in (sym.OK, sym.ERR_HIP)                       # no tree: no count needed
    assert run(direction=(0.0, 0.0, -1e-30), out_=out2, cnt=C.byref(count2), tree_=None) in (sym.OK, sym.ERR_HIP)
    wide[3, 2] = np.nan
    assert run(nrm=wide, nrs=5) == sym.ERR_ARG
    assert run(one_shot=False) == sym.ERR_ARG                      # a NULL context
    # the outputs were never touched
    assert not out.any() and not flip.any() and not comp.any() and not tree.any() and count.value == 0 and res.rounds == 0


def test_orient_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((20, 3)).astype(np.float32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.orient_normals(x, x, 6)
    assert e.value.status == sym.ERR_HIP
