"""CPU tests of the C boundary of the region-growing entry: the header still compiles as pedantic C99, the library exports the entry
points, the config default and the struct size are what the header says, every argument error is returned before a device is needed
with the outputs untouched, and region_cos is the stated conversion."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_region_growing", "symmicp_region_growing"]


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
    missing = [n for n in NEW + ["symmicp_region_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + ["symmicp_region_config_default"]) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_region_config_default(" in hdr
    for name in ("region_growing", "region_config", "region_cos", "pack_clusters", "clusters_from_labels"):
        assert callable(getattr(sym, name))
    assert callable(sym.Engine.region_growing) and callable(sym.Engine.region_growing_raw)


def test_config_default_and_struct_size(sym):
    assert C.sizeof(sym.RegionConfig) == 24
    cfg = sym.RegionConfig()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    sym.lib().symmicp_region_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.eps, cfg.min_region_size, cfg.max_region_size) == (24, 0.0, 0, 0)
    assert cfg.smoothness_cos == np.float32(0.8660254) and cfg.curvature_threshold == np.float32(0.05)
    sym.lib().symmicp_region_config_default(None)                  # tolerated
    cfg = sym.region_config(0.5, 10.0, 0.25, 3, 90)
    assert (cfg.struct_size, cfg.min_region_size, cfg.max_region_size) == (24, 3, 90) and cfg.eps == np.float32(0.5)
    assert cfg.smoothness_cos == sym.region_cos(10.0) and cfg.curvature_threshold == np.float32(0.25)
    assert sym.region_config(0.5, smoothness_cos=0.0).smoothness_cos == 0.0
    assert sym.region_config(0.5).smoothness_cos == np.float32(0.8660254)          # 30 degrees through region_cos = the C default


def test_region_cos(sym):
    for deg in (0, 2, 10, 15, 30, 45, 50, 60, 89.5, 90):
        v = sym.region_cos(deg)
        assert type(v) is np.float32 and v == np.float32(np.cos(np.deg2rad(np.float64(deg))))
    assert sym.region_cos(0) == 1 and sym.region_cos(60) == np.float32(0.5) and 0 <= sym.region_cos(90) < 1e-7


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets SYMMICP_ERR_ARG from each"""
    src = tmp_path / "region_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f}, nrm[6] = {0.f, 0.f, 1.f, 0.f, 0.f, 1.f}, curv[2] = {0.f, 0.f};
    int32_t labels[2] = {7, 7}, sizes[2], smooth[2];
    uint8_t seed[2];
    size_t regions = 0;
    symmicp_region_config cfg;
    int a, b, c;
    symmicp_region_config_default(&cfg);
    a = symmicp_region_growing(-1, xyz, 3, 1, nrm, 3, 1, curv, 1, 2, &cfg, labels, &regions, sizes, 2, seed, smooth);       /* eps 0 */
    cfg.eps = 1.5f;
    b = symmicp_ctx_region_growing(NULL, xyz, 3, 1, nrm, 3, 1, NULL, 0, 2, &cfg, labels, &regions, sizes, 2, seed, smooth);
    cfg.smoothness_cos = 1.5f;
    c = symmicp_region_growing(-1, xyz, 3, 1, nrm, 3, 1, NULL, 0, 2, &cfg, labels, &regions, sizes, 2, NULL, NULL);
    printf("status %d %d %d size %d default %d regions %d labels %d %d\n", a, b, c, (int)sizeof(cfg), (int)cfg.struct_size, (int)regions,
           (int)labels[0], (int)labels[1]);
    return 0;
}
''')
    exe = tmp_path / "region_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 size 24 default 24 regions 0 labels 7 7" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    assert sym.ERR_ARG == 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    rng = np.random.default_rng(0)
    x = rng.random((16, 3)).astype(np.float32)
    nr = rng.standard_normal((16, 3)).astype(np.float32)
    cv = rng.random(16).astype(np.float32)
    n = len(x)
    labels, sizes, smooth, seed, regions = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), C.c_size_t(0)
    t = C.byref(regions)
    inf, nan = float("inf"), float("nan")
    good = dict(eps=0.5, smoothness_cos=0.9, curvature_threshold=0.5, min_region_size=0, max_region_size=0)

    def run(xyz=x, xr=3, xc=1, nrm=nr, nrs=3, ncs=1, curv=cv, cs=1, n_=n, cfg=good, labels_=labels, cnt=t, sizes_=sizes, cap=n, struct_size=None,
            no_cfg=False):
        c = sym.region_config(**cfg)
        if struct_size is not None:
            c.struct_size = struct_size
        return L.symmicp_region_growing(-1, None if xyz is None else fp(xyz), xr, xc, None if nrm is None else fp(nrm), nrs, ncs,
                                        None if curv is None else fp(curv), cs, n_, None if no_cfg else C.byref(c),
                                        None if labels_ is None else ip(labels_), cnt, None if sizes_ is None else ip(sizes_), cap,
                                        seed.ctypes.data_as(C.POINTER(C.c_uint8)), ip(smooth))

    assert run(xyz=None) == sym.ERR_ARG
    assert run(nrm=None) == sym.ERR_ARG
    assert run(no_cfg=True) == sym.ERR_ARG
    assert run(labels_=None) == sym.ERR_ARG
    assert run(cnt=None) == sym.ERR_ARG
    assert run(sizes_=None) == sym.ERR_ARG                         # NULL sizes_out with cap > 0
    assert run(n_=0) == sym.ERR_ARG
    assert run(n_=2 ** 31) == sym.ERR_ARG
    for v in (0, 20, 28):
        assert run(struct_size=v) == sym.ERR_ARG
    for v in (0.0, -1.0, inf, -inf, nan):
        assert run(cfg=dict(good, eps=v)) == sym.ERR_ARG, v
    for v in (-1e-6, 1.0000001, -1.0, 2.0, inf, -inf, nan):
        assert run(cfg=dict(good, smoothness_cos=v)) == sym.ERR_ARG, v
    assert run(cfg=dict(good, curvature_threshold=nan)) == sym.ERR_ARG
    assert run(cfg=dict(good, min_region_size=-1)) == sym.ERR_ARG
    assert run(cfg=dict(good, max_region_size=-1)) == sym.ERR_ARG
    assert run(cfg=dict(good, min_region_size=5, max_region_size=4)) == sym.ERR_ARG
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 1] = v
        assert run(xyz=y) == sym.ERR_ARG
        m = nr.copy()
        m[5, 2] = v
        assert run(nrm=m) == sym.ERR_ARG
    k = cv.copy()
    k[9] = np.nan
    assert run(curv=k) == sym.ERR_ARG
    # strided reading: the bad value sits where the strides skip / reach it
    wide = np.zeros((n, 5), np.float32)
    wide[:, :3] = x
    wide[3, 4] = np.nan
    wn = np.zeros((n, 4), np.float32)
    wn[:, :3] = nr
    wn[2, 3] = np.inf
    k2 = np.zeros(2 * n, np.float32)
    k2[1::2] = np.nan
    labels2, sizes2, count2 = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_size_t(0)          # (with a device these calls run)
    ok = dict(labels_=labels2, sizes_=sizes2, cnt=C.byref(count2))
    assert run(xyz=wide, xr=5, nrm=wn, nrs=4, curv=k2, cs=2, **ok) in (sym.OK, sym.ERR_HIP)
    for cfg in (dict(good, min_region_size=5, max_region_size=5), dict(good, curvature_threshold=inf), dict(good, curvature_threshold=-inf),
                dict(good, smoothness_cos=0.0), dict(good, smoothness_cos=1.0)):
        assert run(cfg=cfg, **ok) in (sym.OK, sym.ERR_HIP)
    kinf = cv.copy()
    kinf[3], kinf[4] = np.inf, -np.inf                              # an infinite curvature is a value, not an error
    assert run(curv=kinf, **ok) in (sym.OK, sym.ERR_HIP)
    assert run(curv=None, cs=0, **ok) in (sym.OK, sym.ERR_HIP)
    wide[3, 2] = np.nan
    assert run(xyz=wide, xr=5) == sym.ERR_ARG
    wn[2, 1] = np.inf
    assert run(nrm=wn, nrs=4) == sym.ERR_ARG
    assert run(curv=k2, cs=1) == sym.ERR_ARG
    c = sym.region_config(**good)
    assert L.symmicp_ctx_region_growing(None, fp(x), 3, 1, fp(nr), 3, 1, None, 0, n, C.byref(c), ip(labels), t, ip(sizes), n, None, None) == sym.ERR_ARG
    # the outputs were never touched
    assert not labels.any() and not sizes.any() and not smooth.any() and not seed.any() and regions.value == 0


def test_region_growing_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    nr = np.tile(np.array([[0, 0, 1]], np.float32), (16, 1))
    with pytest.raises(sym.SymmIcpError) as e:
        sym.region_growing(x, nr, 0.5)
    assert e.value.status == sym.ERR_HIP
