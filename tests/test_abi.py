"""CPU tests of the drop-in boundary: the C-ABI library builds for gfx950, loads, and exports every
symbol include/symmicp.h declares.  No compute calls (there is no GPU here)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, GOLDEN


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    # load through the package (torch's HIP runtime first): a bare dlopen here would map a second HIP runtime into the process,
    # and every GPU test that runs after this module in the same process would find no device
    symmicp.lib()
    return symmicp


def test_header_symbols_are_exported(sym):
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    declared = sorted(set(re.findall(r"\b(symmicp_[a-z0-9_]+)\s*\(", hdr)))
    assert len(declared) >= 25
    L = ctypes.CDLL(sym.LIB_PATH)
    missing = [n for n in declared if not hasattr(L, n)]
    assert not missing, missing
    assert sorted(sym.EXPORTS) == declared


def test_struct_sizes_match_header(sym):
    cfg = sym.default_config()
    assert cfg.struct_size == ctypes.sizeof(sym.Config) == 64
    assert cfg.max_iters == 10 and cfg.diff_threshold == 1.0          # myicp.cpp:6
    assert cfg.mode == sym.MODE_QUIRKS and cfg.corr == sym.CORR_IDENTITY
    assert ctypes.sizeof(sym.Sums) == 8 * sym.NSUM
    assert sym.lib().symmicp_version() >= 100


def test_create_fails_loudly_without_gpu(sym):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sym.SymmIcpError) as e:
        sym.Engine()
    assert e.value.status == sym.ERR_HIP     # no CPU fallback


def test_code_object_is_gfx950_only(sym):
    blob = open(sym.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for other in (b"gfx90a", b"gfx942", b"sm_"):
        assert other not in blob


def test_host_solve_matches_oracle(sym, oracle, cat):
    """symmicp_solve is pure host code (func.cpp:76-102 after the reduction) -> testable on CPU."""
    S = oracle.reduce40(cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"])
    st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_QUIRKS, S)
    st2, pb2, qb2, a2, t2, rc2 = oracle.solve_quirks_gram(S)
    assert st == st2 == 0
    np.testing.assert_allclose(a, a2, rtol=2e-6)
    np.testing.assert_allclose(t, t2, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(X, oracle.compose(pb2, qb2, a2, t2, paper=False), rtol=1e-5, atol=1e-5)
    pivot = cat["tgt"].astype(np.float64).mean(0).astype(np.float32)
    S = oracle.reduce40(cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], pivot=pivot)
    st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_PAPER, S, pivot)
    st2, pb2, qb2, a2, t2, rc2 = oracle.solve_paper(S, pivot)
    assert st == st2 == 0
    np.testing.assert_allclose(a, a2, rtol=2e-6, atol=1e-8)
    np.testing.assert_allclose(X, oracle.compose(pb2, qb2, a2, t2, paper=True), rtol=1e-5, atol=1e-5)
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    T = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert np.abs(X - T).max() < 1e-4     # PAPER + identity pairing: exact in one step


def test_host_solve_flags_degenerate(sym):
    S = np.zeros(sym.NSUM)
    S[34] = 100.0
    for mode in (sym.MODE_QUIRKS, sym.MODE_PAPER):
        st = sym.solve(mode, S)[0]
        assert st == sym.ERR_DEGENERATE


def test_pcd_io_roundtrip(sym, oracle, tmp_path):
    xyz, nrm = sym.pcd_read(os.path.join(GOLDEN, "cat.pcd"))
    xyz_o, _ = oracle.pcd_read(os.path.join(GOLDEN, "cat.pcd"))
    assert nrm is None and np.array_equal(xyz, xyz_o)
    xyz2, nrm2 = sym.pcd_read(os.path.join(GOLDEN, "cat_out.pcd"))
    xyz2_o, _ = oracle.pcd_read(os.path.join(GOLDEN, "cat_out.pcd"))
    assert nrm2 is not None and np.array_equal(xyz2, xyz2_o)
    rng = np.random.default_rng(0)
    n = rng.standard_normal((100, 3)).astype(np.float32)
    for binary in (False, True):
        p = str(tmp_path / ("t%d.pcd" % binary))
        sym.pcd_write(p, xyz[:100], n, binary=binary)
        a, b = sym.pcd_read(p)
        assert np.array_equal(a, xyz[:100]) and np.array_equal(b, n)
        a2, b2 = oracle.pcd_read(p)
        assert np.array_equal(a2, xyz[:100]) and np.array_equal(b2, n)
    with pytest.raises(sym.SymmIcpError):
        sym.pcd_read(str(tmp_path / "missing.pcd"))


@pytest.mark.parametrize("bad", ["negative_size", "zero_count", "size_3", "type_x", "points_mismatch", "huge_record", "f2_xyz", "no_data"])
def test_pcd_reader_rejects_malformed_headers(sym, tmp_path, bad):
    """The PCD header is untrusted input (the reference hands it to pcl::PCDReader and ignores the status, myicp.cpp:22-30):
    sizes, counts and types this reader cannot place or load are refused with an I/O error instead of being trusted."""
    hdr = dict(FIELDS="x y z", SIZE="4 4 4", TYPE="F F F", COUNT="1 1 1", WIDTH="2", HEIGHT="1", POINTS="2", DATA="ascii")
    if bad == "negative_size": hdr["SIZE"] = "4 -4 4"
    if bad == "zero_count": hdr["COUNT"] = "1 0 1"
    if bad == "size_3": hdr["SIZE"] = "4 3 4"
    if bad == "type_x": hdr["TYPE"] = "F X F"
    if bad == "points_mismatch": hdr["POINTS"] = "5"
    if bad == "huge_record": hdr["COUNT"] = "1 1 4000"; hdr["SIZE"] = "4 4 8"; hdr["FIELDS"] = "x y z"; hdr["COUNT"] = "4000 4000 4000"
    if bad == "f2_xyz": hdr["SIZE"] = "2 2 2"
    if bad == "no_data": del hdr["DATA"]
    p = tmp_path / "bad.pcd"
    with open(p, "w") as f:
        f.write("# .PCD v0.7\nVERSION 0.7\n")
        for k in ("FIELDS", "SIZE", "TYPE", "COUNT", "WIDTH", "HEIGHT"):
            f.write("%s %s\n" % (k, hdr[k]))
        f.write("VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %s\n" % hdr["POINTS"])
        if "DATA" in hdr:
            f.write("DATA ascii\n")
        f.write("0 0 0\n1 1 1\n")
    with pytest.raises(sym.SymmIcpError):
        sym.pcd_read(str(p))


def test_reference_style_client_compiles_against_the_dropin(sym, tmp_path):
    """A client written the way the reference's driver uses the class -- only the precompiled header and myicp.h included,
    MyICP's four reference methods, pcl:: clouds and the headless pcl::visualization::PCLVisualizer -- builds against
    include/ (stdafx.h + the pcl:: stand-in) and links with libsymmicp.  Without a GPU the run must fail loudly, not
    fall back to a CPU path."""
    import shutil
    import subprocess
    (tmp_path / "client.cpp").write_text(r"""
#include "stdafx.h"
#include "myicp.h"

static pcl::PointCloud<pcl::PointXYZ>::Ptr as_xyz(const pcl::PointCloud<PointT>::Ptr &in)
{
    pcl::PointCloud<pcl::PointXYZ>::Ptr out(new pcl::PointCloud<pcl::PointXYZ>);
    for (size_t i = 0; i < in->points.size(); i++) {
        pcl::PointXYZ p;
        p.x = in->points[i].x; p.y = in->points[i].y; p.z = in->points[i].z;
        out->points.push_back(p);
    }
    return out;
}

int main()
{
    MyICP icp;
    int st = icp.LoadCloud("cat.pcd", "cat_out.pcd");
    cout << "load " << st << " src " << icp.GetSrcCloud()->points.size() << " tgt " << icp.GetTgtCloud()->points.size() << endl;
    icp.RegisterSymm();
    pcl::visualization::PCLVisualizer viewer("client");
    viewer.addPointCloud(as_xyz(icp.GetSrcCloud()));
    viewer.addPointCloud(as_xyz(icp.GetTgtCloud()), "target");
    while (!viewer.wasStopped())
        viewer.spinOnce();
    return 0;
}
""")
    exe = tmp_path / "client"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(tmp_path / "client.cpp"), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    import torch
    if not torch.cuda.is_available():
        # no GPU here: the drop-in must fail loudly, not fall back to a CPU path
        shutil.copy(os.path.join(GOLDEN, "cat.pcd"), tmp_path / "cat.pcd")
        shutil.copy(os.path.join(GOLDEN, "cat_out.pcd"), tmp_path / "cat_out.pcd")
        r = subprocess.run([str(exe)], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert "load 0 src 3400 tgt 3400" in r.stdout, r.stdout + r.stderr
        assert "no usable gfx950 HIP device" in r.stderr and "Result transform" not in r.stdout


def test_host_solve_p2p_matches_oracle(sym, oracle, cat):
    pivot = cat["tgt"].astype(np.float64).mean(0).astype(np.float32)
    S = oracle.reduce40(cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], pivot=pivot, p2p=True)
    st, _, _, _, _, rc, X = sym.solve(sym.MODE_P2P, S, pivot)
    st2, X2 = oracle.solve_p2p(S, pivot)
    assert st == st2 == 0 and np.abs(X - X2).max() < 1e-6
    c, s = np.cos(np.pi / 4), np.sin(np.pi / 4)
    T = np.array([[c, -s, 0, 2.5], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
    assert np.abs(X - T).max() < 1e-5


def test_header_is_plain_c_and_links_from_c(sym, tmp_path):
    """include/symmicp.h is the drop-in boundary: it must compile as C99 (no C++ in the signatures) and a C program
    must link against libsymmicp.so and get a clean error, not a crash, without a GPU."""
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    symmicp_config cfg;
    symmicp_ctx *ctx = NULL;
    symmicp_sums s;
    float X[16], pbar[3], qbar[3], a[3], t[3], rc = 0.f;
    size_t b = 0, c = 0;
    int k, st;
    symmicp_config_default(&cfg);
    if (cfg.struct_size != (int)sizeof(cfg) || cfg.max_iters != 10) return 2;
    if (symmicp_shard_range(10, 3, 2, &b, &c) != SYMMICP_OK || b + c != 10) return 3;
    for (k = 0; k < SYMMICP_NSUM; k++) s.s[k] = 0.0;
    st = symmicp_solve(SYMMICP_MODE_PAPER, &s, NULL, pbar, qbar, a, t, &rc, X);     /* empty record: flagged, no NaN crash */
    printf("version %d solve_status %d\n", symmicp_version(), st);
    st = symmicp_create(&cfg, &ctx);
    printf("create_status %d ctx %s\n", st, ctx ? "set" : "null");
    if (st == SYMMICP_OK) symmicp_destroy(ctx);
    return 0;
}
''')
    exe = tmp_path / "abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "version 100" in r.stdout
    import torch
    if not torch.cuda.is_available():
        assert "create_status" in r.stdout and "ctx null" in r.stdout and "create_status 0" not in r.stdout


def test_sweep_order_is_a_coherent_permutation():
    """synth.sweep_order (bench.py, N > 1): a permutation of the rows after which contiguous row ranges are spatially compact"""
    import numpy as np
    from symmicp import synth
    d = synth.c4_surface(20000)
    o = synth.sweep_order(d["src"])
    assert np.array_equal(np.sort(o), np.arange(20000))
    p = d["src"][o].astype(np.float64)
    def spread(q):          # mean bounding-box diagonal of 8 contiguous row ranges
        return np.mean([np.linalg.norm(q[k * 2500:(k + 1) * 2500].max(0) - q[k * 2500:(k + 1) * 2500].min(0)) for k in range(8)])
    assert spread(p) < 0.6 * spread(d["src"].astype(np.float64))


def test_host_solve_is_equivariant_under_power_of_two_units(sym, oracle, cat):
    """symmicp_solve (PAPER) on the cat pair's first-pass record in units 2^k times larger (k in -14..14): status 0, the same
    rotation block and rc bit for bit, a translation exactly 2^k times larger.  Absolute thresholds on the conditioning of
    the mixed rotation / translation system flagged the 2^14 copy degenerate."""
    from _frames import scale_record
    pivot = cat["tgt"].astype(np.float64).mean(0).astype(np.float32)
    S = oracle.reduce40(cat["src"], cat["src_n"], cat["tgt"], cat["tgt_n"], pivot=pivot)
    st0, pb0, qb0, a0, t0, rc0, X0 = sym.solve(sym.MODE_PAPER, S, pivot)
    assert st0 == 0
    for k in (-14, -8, 0, 8, 14):
        s = np.float32(2.0 ** k)
        st, pb, qb, a, t, rc, X = sym.solve(sym.MODE_PAPER, scale_record(S, float(s)), pivot * s)
        assert st == 0, (k, st, rc)
        assert np.array_equal(X[:3, :3], X0[:3, :3]), k
        assert np.array_equal(X[:3, 3], X0[:3, 3] * s), (k, X[:3, 3], X0[:3, 3])
        assert np.array_equal(a, a0) and np.array_equal(t, t0 * s), k
        assert rc == rc0, (k, rc, rc0)
    # the check keeps its teeth: a rank-deficient record (collinear bunny, one normal direction) is degenerate in every unit
    from conftest import GOLDEN as G
    bunny, _ = oracle.pcd_read(os.path.join(G, "txt2pcd_bunny1.pcd"))
    n = np.tile(np.array([[0, 0, 1]], np.float32), (bunny.shape[0], 1))
    tgt = bunny + np.array([0.01, 0.02, 0.0], np.float32)
    pv = tgt.astype(np.float64).mean(0).astype(np.float32)
    Sb = oracle.reduce40(bunny, n, tgt, n, pivot=pv)
    for k in (-14, -8, 0, 8, 14):
        s = np.float32(2.0 ** k)
        assert sym.solve(sym.MODE_PAPER, scale_record(Sb, float(s)), pv * s)[0] == sym.ERR_DEGENERATE, k


def test_estimate_normals_refuses_bad_arguments_before_any_device_work(sym, cat):
    """symmicp_estimate_normals checks its arguments before it creates a context, so this runs without a GPU: k outside 3..16 or
    above n, n = 0, and null inputs or outputs give ERR_ARG and leave the outputs untouched"""
    import ctypes as C
    L = sym.lib()
    x = np.ascontiguousarray(cat["src"][:40])
    n = len(x)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))                # noqa: E731
    nrm = np.full((n, 3), 7, np.float32)
    curv = np.full(n, 7, np.float32)
    for nn, k in ((n, 2), (n, 17), (n, n + 1), (0, 3), (10, 11)):
        assert L.symmicp_estimate_normals(-1, fp(x), 3, 1, nn, k, None, fp(nrm), fp(curv)) == sym.ERR_ARG
    assert L.symmicp_estimate_normals(-1, None, 3, 1, n, 10, None, fp(nrm), fp(curv)) == sym.ERR_ARG
    assert L.symmicp_estimate_normals(-1, fp(x), 3, 1, n, 10, None, None, fp(curv)) == sym.ERR_ARG
    assert (nrm == 7).all() and (curv == 7).all()
