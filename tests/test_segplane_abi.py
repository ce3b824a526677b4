"""CPU tests of the C boundary of the plane segmentation: the header still compiles as pedantic C99, the library exports the entry points,
the config default and the struct sizes are what the header says, every argument error is returned before a device is needed, with
the outputs untouched, and plane_core.h computes on the host what tests/cpp/plane_core.cpp writes down."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NEW = ["symmicp_ctx_segment_plane", "symmicp_segment_plane", "symmicp_ctx_plane_hypotheses"]


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
    missing = [n for n in NEW + ["symmicp_plane_config_default"] if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + ["symmicp_plane_config_default"]) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_plane_config_default(" in hdr
    for name in ("segment_plane", "segment_planes", "plane_config"):
        assert callable(getattr(sym, name))
    assert callable(sym.Engine.segment_plane) and callable(sym.Engine.segment_plane_raw) and callable(sym.Engine.segment_planes)
    myicp_h = open(os.path.join(ROOT, "include", "myicp.h")).read()
    assert callable(sym.MyICP.removePlane) and callable(sym.MyICP.planeRemoved) and "removePlane" in myicp_h and "planeRemoved" in myicp_h
    assert (sym.PLANE_EVALUATED, sym.PLANE_REPEATED, sym.PLANE_DEGENERATE, sym.PLANE_OFF_AXIS) == (0, 1, 2, 3)
    for k, name in enumerate(("EVALUATED", "REPEATED", "DEGENERATE", "OFF_AXIS")):
        assert "#define SYMMICP_PLANE_%s %d\n" % (name, k) in hdr
    assert sym.lib().symmicp_version() == 100


def test_config_default_and_struct_sizes(sym):
    assert C.sizeof(sym.PlaneConfig) == 48 and C.sizeof(sym.PlaneResult) == 56
    cfg = sym.PlaneConfig()
    C.memset(C.byref(cfg), 0xFF, C.sizeof(cfg))
    sym.lib().symmicp_plane_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.hypotheses, cfg.seed, cfg.max_dist, cfg.min_inliers, cfg.refits, list(cfg.axis), cfg.max_angle_deg, cfg.reserved) == (
        48, 1000, 0, 0.0, 3, 1, [0.0, 0.0, 0.0], 0.0, 0)
    sym.lib().symmicp_plane_config_default(None)                  # tolerated
    cfg = sym.plane_config(0.5, 77, 9, 2, 40, (0, 0, 2), 15.0)
    assert (cfg.struct_size, cfg.hypotheses, cfg.seed, cfg.min_inliers, cfg.refits, list(cfg.axis), cfg.max_angle_deg) == (48, 77, 9, 40, 2, [0.0, 0.0, 2.0], 15.0)
    assert cfg.max_dist == np.float32(0.5)


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets SYMMICP_ERR_ARG from each"""
    src = tmp_path / "plane_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float xyz[9] = {0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float plane[4] = {7.f, 7.f, 7.f, 7.f}, hyp[4], pivot[3];
    int32_t rows[3] = {7, 7, 7}, inl[1];
    uint8_t status[1];
    double dist[3];
    size_t count = 9;
    symmicp_plane_config cfg;
    symmicp_plane_result res;
    int a, b, c, d;
    symmicp_plane_config_default(&cfg);
    res.best_hypothesis = 5;
    cfg.hypotheses = 1;
    a = symmicp_segment_plane(-1, xyz, 3, 1, 3, &cfg, plane, &res, rows, 3, &count, dist, status, inl);            /* max_dist 0 */
    cfg.max_dist = 0.5f;
    b = symmicp_ctx_segment_plane(NULL, xyz, 3, 1, 3, &cfg, plane, &res, rows, 3, &count, dist, status, inl);
    c = symmicp_ctx_plane_hypotheses(NULL, xyz, 3, 1, 3, &cfg, hyp, status, pivot);
    cfg.refits = 9;
    d = symmicp_segment_plane(-1, xyz, 3, 1, 3, &cfg, plane, &res, rows, 3, &count, dist, status, inl);
    printf("status %d %d %d %d size %d %d default %d count %d rows %d plane %g best %d macros %d%d%d%d\n", a, b, c, d, (int)sizeof(cfg), (int)sizeof(res),
           (int)cfg.struct_size, (int)count, (int)rows[0], (double)plane[0], (int)res.best_hypothesis, SYMMICP_PLANE_EVALUATED,
           SYMMICP_PLANE_REPEATED, SYMMICP_PLANE_DEGENERATE, SYMMICP_PLANE_OFF_AXIS);
    return 0;
}
''')
    exe = tmp_path / "plane_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 size 48 56 default 48 count 9 rows 7 plane 7 best 5 macros 0123" in r.stdout


def test_argument_errors_need_no_device(sym):
    L = sym.lib()
    assert sym.ERR_ARG == 1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    n, H = len(x), 8
    plane, rows, dist = np.zeros(4, np.float32), np.zeros(n, np.int32), np.zeros(n, np.float64)
    status, inl, count, res = np.zeros(H, np.uint8), np.zeros(H, np.int32), C.c_size_t(0), sym.PlaneResult()
    t = C.byref(count)
    inf, nan = float("inf"), float("nan")
    good = dict(max_dist=0.1, hypotheses=H, seed=0, refits=1, min_inliers=3, axis=None, max_angle_deg=0.0)

    def run(xyz=x, xr=3, xc=1, n_=n, cfg=good, plane_=plane, res_=res, rows_=rows, cap=n, cnt=t, struct_size=None, no_cfg=False):
        c = sym.plane_config(**cfg)
        if struct_size is not None:
            c.struct_size = struct_size
        return L.symmicp_segment_plane(-1, None if xyz is None else fp(xyz), xr, xc, n_, None if no_cfg else C.byref(c),
                                       None if plane_ is None else fp(plane_), None if res_ is None else C.byref(res_),
                                       None if rows_ is None else ip(rows_), cap, cnt, dist.ctypes.data_as(C.POINTER(C.c_double)),
                                       status.ctypes.data_as(C.POINTER(C.c_uint8)), ip(inl))

    assert run(xyz=None) == sym.ERR_ARG
    assert run(no_cfg=True) == sym.ERR_ARG
    assert run(plane_=None) == sym.ERR_ARG
    assert run(res_=None) == sym.ERR_ARG
    assert run(cnt=None) == sym.ERR_ARG
    assert run(rows_=None) == sym.ERR_ARG                          # NULL rows_out with cap > 0
    for v in (0, 1, 2, 2 ** 31):
        assert run(n_=v, cfg=dict(good, min_inliers=0)) == sym.ERR_ARG, v
    for v in (0, 44, 52):
        assert run(struct_size=v) == sym.ERR_ARG
    for v in (0, 2 ** 24 + 1):
        assert run(cfg=dict(good, hypotheses=v)) == sym.ERR_ARG, v
    for v in (0.0, -1.0, inf, -inf, nan):
        assert run(cfg=dict(good, max_dist=v)) == sym.ERR_ARG, v
    for v in (-1, n + 1, -2 ** 31):
        assert run(cfg=dict(good, min_inliers=v)) == sym.ERR_ARG, v
    for v in (-1, 9):
        assert run(cfg=dict(good, refits=v)) == sym.ERR_ARG, v
    for v in ((nan, 0, 0), (0, inf, 0), (0, 0, -inf)):
        assert run(cfg=dict(good, axis=v, max_angle_deg=10.0)) == sym.ERR_ARG, v
    for v in (0.0, -5.0, 90.5, nan, inf):
        assert run(cfg=dict(good, axis=(0, 0, 1), max_angle_deg=v)) == sym.ERR_ARG, v
    for v in (np.nan, np.inf, -np.inf):
        y = x.copy()
        y[7, 1] = v
        assert run(xyz=y) == sym.ERR_ARG
    # strided reading: the bad value sits in a column the strides skip / reach
    wide = np.zeros((n, 5), np.float32)
    wide[:, :3] = x
    wide[3, 4] = np.nan
    plane2, rows2, count2, res2 = np.zeros(4, np.float32), np.zeros(n, np.int32), C.c_size_t(0), sym.PlaneResult()      # (with a device these calls run)
    ok = (sym.OK, sym.ERR_HIP, sym.ERR_NO_CONSENSUS)
    assert run(xyz=wide, xr=5, plane_=plane2, res_=res2, rows_=rows2, cnt=C.byref(count2)) in ok
    assert run(cfg=dict(good, max_angle_deg=-1.0), plane_=plane2, res_=res2, rows_=rows2, cnt=C.byref(count2)) in ok      # no axis: the angle is not read
    assert run(cfg=dict(good, axis=(0, 0, 1), max_angle_deg=90.0), plane_=plane2, res_=res2, rows_=rows2, cnt=C.byref(count2)) in ok
    assert run(cfg=dict(good, min_inliers=n), plane_=plane2, res_=res2, rows_=rows2, cnt=C.byref(count2)) in ok
    wide[3, 2] = np.nan
    assert run(xyz=wide, xr=5) == sym.ERR_ARG
    c = sym.plane_config(**good)
    assert L.symmicp_ctx_segment_plane(None, fp(x), 3, 1, n, C.byref(c), fp(plane), C.byref(res), ip(rows), n, t, None, None, None) == sym.ERR_ARG
    assert L.symmicp_ctx_plane_hypotheses(None, fp(x), 3, 1, n, C.byref(c), fp(plane), None, None) == sym.ERR_ARG
    # the outputs were never touched
    assert not plane.any() and not rows.any() and not dist.any() and not status.any() and not inl.any() and count.value == 0
    assert (res.best_hypothesis, res.evaluated, res.inliers_ransac, res.inliers_final, res.rmse_final, list(res.plane)) == (0, 0, 0, 0, 0.0, [0.0] * 4)


def test_segment_plane_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    x = np.random.default_rng(0).random((16, 3)).astype(np.float32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.segment_plane(x, 0.1, 16)
    assert e.value.status == sym.ERR_HIP
    with pytest.raises(sym.SymmIcpError) as e:
        sym.segment_planes(x, 0.1, 2, 3, 16)
    assert e.value.status == sym.ERR_HIP


def test_plane_core_on_the_host(tmp_path):
    """tests/cpp/plane_core.cpp: the host instantiation of plane_core.h, unfused as the library is built; and the same stand-alone
    program once more under the sanitizers where the toolchain links them"""
    if not shutil.which("g++"):
        pytest.fail("g++ is needed to build the plane_core driver")
    rocm = os.environ.get("ROCM_PATH") or os.environ.get("ROCM") or "/opt/rocm"       # (plane_core.h includes the HIP headers: host side only here)
    src = os.path.join(ROOT, "tests", "cpp", "plane_core.cpp")
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fno-fast-math",
            "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "icp-symm_amd", "csrc"),
            "-isystem", os.path.join(rocm, "include"), src]
    exe = str(tmp_path / "plane_core")
    subprocess.check_call(base + ["-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "plane_core: ok" in out.stdout, out.stdout + out.stderr
    assert out.stdout.count(" ok\n") == 4
    san = str(tmp_path / "plane_core_san")
    r = subprocess.run(base + ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", san], capture_output=True, text=True)
    if r.returncode == 0:
        out = subprocess.run([san], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0 and "plane_core: ok" in out.stdout, out.stdout + out.stderr
    else:
        print("no sanitizer runtime to link against: the plain build only")
