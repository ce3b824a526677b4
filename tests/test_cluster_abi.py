"""CPU tests of the C boundary of the clustering entry: the header still compiles as pedantic C99, the library exports the entry points,
the config default and the struct size are what the header says, and every argument error is returned before a device is needed, with
the outputs untouched."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_cluster", "symmicp_cluster"]


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
    missing = [n for n in NEW + ["symmicp_cluster_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + ["symmicp_cluster_config_default"]) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_cluster_config_default(" in hdr
    for name in ("cluster_dbscan", "euclidean_clusters", "pack_clusters", "clusters_from_labels"):
        assert callable(getattr(sym, name))
    assert callable(sym.Engine.cluster_dbscan) and callable(sym.Engine.cluster_dbscan_raw)
    assert callable(sym.MyICP.removeSmallClusters) and "removeSmallClusters" in open(os.path.join(ROOT, "include", "myicp.h")).read()


def test_config_default_and_struct_size(sym):
    assert C.sizeof(sym.ClusterConfig) == 24
    cfg = sym.ClusterConfig()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    sym.lib().symmicp_cluster_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.eps, cfg.min_points, cfg.min_cluster_size, cfg.max_cluster_size, cfg.reserved) == (24, 0.0, 1, 0, 0, 0)
    sym.lib().symmicp_cluster_config_default(None)                  # tolerated
    cfg = sym.cluster_config(0.5, 7, 3, 90)
    assert (cfg.struct_size, cfg.min_points, cfg.min_cluster_size, cfg.max_cluster_size) == (24, 7, 3, 90) and cfg.eps == np.float32(0.5)


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets SYMMICP_ERR_ARG from each"""
    src = tmp_path / "cluster_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[6] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f};
    int32_t labels[2] = {7, 7}, sizes[2], nb[2];
    uint8_t core[2];
    size_t clusters = 0;
    symmicp_cluster_config cfg;
    int a, b, c;
    symmicp_cluster_config_default(&cfg);
    a = symmicp_cluster(-1, xyz, 3, 1, 2, &cfg, labels, &clusters, sizes, 2, core, nb);            /* eps 0 */
    cfg.eps = 1.5f;
    b = symmicp_ctx_cluster(NULL, xyz, 3, 1, 2, &cfg, labels, &clusters, sizes, 2, core, nb);
    cfg.min_points = 0;
    c = symmicp_cluster(-1, xyz, 3, 1, 2, &cfg, labels, &clusters, sizes, 2, core, nb);
    printf("status %d %d %d size %d default %d clusters %d labels %d %d\n", a, b, c, (int)sizeof(cfg), (int)cfg.struct_size, (int)clusters,
           (int)labels[0], (int)labels[1]);
    return 0;
}
''')
    exe = tmp_path / "cluster_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 size 24 default 24 clusters 0 labels 7 7" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    assert sym.ERR_ARG == 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    n = len(x)
    labels, sizes, nb, core, clusters = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint8), C.c_size_t(0)
    t = C.byref(clusters)
    inf, nan = float("inf"), float("nan")
    good = dict(eps=0.5, min_points=2, min_cluster_size=0, max_cluster_size=0)

    def run(xyz=x, xr=3, xc=1, n_=n, cfg=good, labels_=labels, cnt=t, sizes_=sizes, cap=n, struct_size=None, no_cfg=False):
        c = sym.cluster_config(**cfg)
        if struct_size is not None:
            c.struct_size = struct_size
        return L.symmicp_cluster(-1, None if xyz is None else fp(xyz), xr, xc, n_, None if no_cfg else C.byref(c), None if labels_ is None else ip(labels_),
                                 cnt, None if sizes_ is None else ip(sizes_), cap, core.ctypes.data_as(C.POINTER(C.c_uint8)), ip(nb))

    assert run(xyz=None) == sym.ERR_ARG
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
    for v in (0, -1, -2 ** 31):
        assert run(cfg=dict(good, min_points=v)) == sym.ERR_ARG, v
    assert run(cfg=dict(good, min_cluster_size=-1)) == sym.ERR_ARG
    assert run(cfg=dict(good, max_cluster_size=-1)) == sym.ERR_ARG
    assert run(cfg=dict(good, min_cluster_size=5, max_cluster_size=4)) == sym.ERR_ARG
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 1] = v
        assert run(xyz=y) == sym.ERR_ARG
    # strided reading: the bad value sits in a column the strides skip / reach
    wide = np.zeros((n, 5), np.float32)
    wide[:, :3] = x
    wide[3, 4] = np.nan
    labels2, sizes2, count2 = np.zeros(n, np.int32), np.zeros(n, np.int32), C.c_size_t(0)          # (with a device these calls run)
    assert run(xyz=wide, xr=5, labels_=labels2, sizes_=sizes2, cnt=C.byref(count2)) in (sym.OK, sym.ERR_HIP)
    assert run(cfg=dict(good, min_cluster_size=5, max_cluster_size=5), labels_=labels2, sizes_=sizes2, cnt=C.byref(count2)) in (sym.OK, sym.ERR_HIP)
    wide[3, 2] = np.nan
    assert run(xyz=wide, xr=5) == sym.ERR_ARG
    c = sym.cluster_config(**good)
    assert L.symmicp_ctx_cluster(None, fp(x), 3, 1, n, C.byref(c), ip(labels), t, ip(sizes), n, None, None) == sym.ERR_ARG
    # the outputs were never touched
    assert not labels.any() and not sizes.any() and not nb.any() and not core.any() and clusters.value == 0


def test_python_helpers_on_given_labels(sym):
    """clusters_from_labels and pack_clusters are host functions of the labels"""
    labels = np.array([2, -1, 0, 2, 1, 0, 2, -1, 1, 3], np.int32)
    parts = sym.clusters_from_labels(labels)
    assert [p.tolist() for p in parts] == [[0, 3, 6], [2, 5], [4, 8], [9]]      # largest first, ties by label; rows ascending
    assert all(p.dtype == np.int32 for p in parts) and sym.clusters_from_labels(np.full(4, -1)) == []
    x = np.arange(30, dtype=np.float32).reshape(10, 3)
    p = sym.pack_clusters(x, -x, labels)
    assert p["rows"].tolist() == [2, 5, 4, 8, 0, 3, 6, 9] and p["ranges"].tolist() == [[0, 2], [2, 2], [4, 3], [7, 1]]
    assert p["labels"].tolist() == [0, 1, 2, 3] and p["skipped"] == []
    assert np.array_equal(p["xyz"], x[p["rows"]]) and np.array_equal(p["nrm"], -x[p["rows"]])
    big = np.zeros(sym.BATCH_MAX_POINTS + 3, np.int32)
    big[-2:] = 1
    q = sym.pack_clusters(np.zeros((len(big), 3), np.float32), None, big)
    assert q["skipped"] == [(0, sym.BATCH_MAX_POINTS + 1)] and q["labels"].tolist() == [1] and q["ranges"].tolist() == [[0, 2]] and q["nrm"] is None


def test_cluster_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.cluster_dbscan(x, 0.5, 2)
    assert e.value.status == sym.ERR_HIP
    with pytest.raises(sym.SymmIcpError) as e:
        sym.euclidean_clusters(x, 0.5)
    assert e.value.status == sym.ERR_HIP
