"""CPU tests of the C boundary of colored ICP (SYMMICP_MODE_COLOR): the enum, what symmicp_create and symmicp_solve accept, the new
exports against the header and symmicp.EXPORTS, pedantic C99, NULL-context refusals, the Python surface that needs no device, and
symmicp_pcd_read_intensity on hand-written ASCII and binary files."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from _plane_ref import plane_record

NEW_INT = ["symmicp_set_color_weight", "symmicp_get_color_weight", "symmicp_set_source_intensity", "symmicp_set_target_intensity",
           "symmicp_get_source_intensity", "symmicp_intensity_gradient", "symmicp_ctx_intensity_gradient"]
NEW = NEW_INT + ["symmicp_pcd_read_intensity"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


def test_enum_is_7_and_4_and_6_stay_unassigned(sym):
    assert sym.MODE_COLOR == 7
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    assert re.search(r"SYMMICP_MODE_COLOR = 7\b", hdr)
    assert not re.search(r"SYMMICP_MODE_\w+ = (4|6)\b", hdr)


def test_create_accepts_mode_7_before_it_looks_for_a_device(sym):
    L = sym.lib()
    for mode, bad in ((sym.MODE_COLOR, False), (4, True), (6, True), (8, True), (-1, True)):
        cfg = sym.default_config(mode=mode)
        h = C.c_void_p()
        st = L.symmicp_create(C.byref(cfg), C.byref(h))
        if st == 0:
            L.symmicp_destroy(h)
        assert (st == sym.ERR_ARG) == bad, (mode, st)


def test_solve_of_mode_7_is_planes_solve_bit_for_bit(sym):
    rng = np.random.default_rng(7)
    for trial in range(4):
        n = 200
        p = rng.normal(size=(n, 3)).astype(np.float32) + np.float32(10.0)
        q = (p + rng.normal(scale=0.01, size=(n, 3))).astype(np.float32)
        nq = rng.normal(size=(n, 3))
        nq = (nq / np.linalg.norm(nq, axis=1, keepdims=True)).astype(np.float32)
        pivot = q.mean(0)
        S, _ = plane_record(p, q, nq, pivot)
        a = sym.solve(sym.MODE_PLANE, S, pivot)
        b = sym.solve(sym.MODE_COLOR, S, pivot)
        assert a[0] == b[0] == 0
        for x, y in zip(a[1:], b[1:]):
            assert np.array_equal(np.asarray(x), np.asarray(y))
    for mode in (4, 6, 8):
        assert sym.solve(mode, S, pivot)[0] == sym.ERR_ARG
    assert sym.solve(sym.MODE_COLOR, np.zeros(40))[0] == sym.solve(sym.MODE_PLANE, np.zeros(40))[0] == sym.ERR_DEGENERATE


def test_exports_header_and_python_surface_agree(sym):
    L = C.CDLL(sym.LIB_PATH)
    missing = [n for n in NEW if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW_INT:
        assert "int %s(" % n in hdr, n
    assert "long symmicp_pcd_read_intensity(" in hdr
    for name in ("set_color_weight", "color_weight", "set_source_intensity", "set_target_intensity", "source_intensity", "intensity_gradient"):
        assert callable(getattr(sym.Engine, name)), name
    for name in ("intensity_gradient", "pcd_read_intensity"):
        assert callable(getattr(sym, name)), name
    assert callable(sym.MyICP.setColorWeight)
    from symmicp import synth
    assert callable(synth.ridge_textured)


def test_header_with_the_color_declarations_is_pedantic_c99(sym, tmp_path):
    src = tmp_path / "color_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include "symmicp.h"
int main(void) {
    float x[9] = {0}, v[3] = {0}, g[9] = {0}, lam = 0.0f;
    int kind = -1, a, b, c, d, e, f;
    long n;
    symmicp_config cfg;
    a = symmicp_set_color_weight(NULL, 0.5f);
    b = symmicp_get_color_weight(NULL, &lam);
    c = symmicp_set_source_intensity(NULL, v, 1, 3);
    d = symmicp_set_target_intensity(NULL, v, 1, g, 3, 1, 3);
    e = symmicp_get_source_intensity(NULL, v, 3);
    f = symmicp_ctx_intensity_gradient(NULL, x, 3, 1, x, 3, 1, v, 1, 3, 3, g);
    n = symmicp_pcd_read_intensity("/nonexistent/file.pcd", NULL, 0, &kind);
    symmicp_config_default(&cfg);
    cfg.mode = SYMMICP_MODE_COLOR;
    printf("status %d %d %d %d %d %d read %ld kind %d mode %d size %d\n", a, b, c, d, e, f, n, kind, (int)cfg.mode, (int)sizeof(cfg));
    return 0;
}
''')
    exe = tmp_path / "color_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert "status 1 1 1 1 1 1 read -4 kind 0 mode 7 size 64" in r.stdout, r.stdout      # (symmicp_config stays 64 bytes)


def test_null_context_and_null_arguments_are_argument_errors(sym):
    L = sym.lib()
    fp = C.POINTER(C.c_float)
    v = np.full(4, 7.0, np.float32)
    g = np.full((4, 3), 7.0, np.float32)
    x = np.zeros((4, 3), np.float32)
    pv, pg, px = v.ctypes.data_as(fp), g.ctypes.data_as(fp), x.ctypes.data_as(fp)
    lam = C.c_float(7)
    assert L.symmicp_set_color_weight(None, 0.5) == sym.ERR_ARG
    assert L.symmicp_get_color_weight(None, C.byref(lam)) == sym.ERR_ARG
    assert L.symmicp_set_source_intensity(None, pv, 1, 4) == sym.ERR_ARG
    assert L.symmicp_set_target_intensity(None, pv, 1, pg, 3, 1, 4) == sym.ERR_ARG
    assert L.symmicp_get_source_intensity(None, pv, 4) == sym.ERR_ARG
    assert L.symmicp_ctx_intensity_gradient(None, px, 3, 1, px, 3, 1, pv, 1, 4, 3, pg) == sym.ERR_ARG
    # the device form checks its arguments before it makes a context
    assert L.symmicp_intensity_gradient(-1, None, 3, 1, px, 3, 1, pv, 1, 4, 3, pg) == sym.ERR_ARG
    assert L.symmicp_intensity_gradient(-1, px, 3, 1, None, 3, 1, pv, 1, 4, 3, pg) == sym.ERR_ARG
    assert L.symmicp_intensity_gradient(-1, px, 3, 1, px, 3, 1, None, 1, 4, 3, pg) == sym.ERR_ARG
    assert L.symmicp_intensity_gradient(-1, px, 3, 1, px, 3, 1, pv, 1, 4, 3, None) == sym.ERR_ARG
    for k in (2, 17, 5):                                   # 3 <= k <= 16 and k <= n
        assert L.symmicp_intensity_gradient(-1, px, 3, 1, px, 3, 1, pv, 1, 4, k, pg) == sym.ERR_ARG, k
    assert L.symmicp_intensity_gradient(-1, px, 3, 1, px, 3, 1, pv, 1, 0, 3, pg) == sym.ERR_ARG
    assert lam.value == 7.0 and (v == 7).all() and (g == 7).all()
    assert L.symmicp_pcd_read_intensity(None, None, 0, None) == -sym.ERR_ARG


def test_python_myicp_refuses_what_color_cannot_do(sym):
    m = sym.MyICP(mode=sym.MODE_COLOR, corr=sym.CORR_TREE, verbose=False)
    with pytest.raises(sym.SymmIcpError) as e:
        m.setVoxelLevels([(0.1, 5, 0.0)])
    assert e.value.status == sym.ERR_ARG
    m.setVoxelLevels([])
    x = np.zeros((8, 3), np.float32)
    m.setInputSource(x, x, intensity=np.zeros(8))
    m.setInputTarget(x, x)                                  # no target intensity
    with pytest.raises(sym.SymmIcpError) as e:
        m.align()
    assert e.value.status == sym.ERR_STATE
    with pytest.raises(ValueError):
        m.setInputTarget(x, x, intensity=np.zeros(7))
    m.setColorWeight(0.5)
    assert m._color_weight == 0.5


def test_entries_fail_loudly_without_gpu(sym):
    """no device: a COLOR context cannot be made and the gradient is not estimated on the host instead"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(sym.SymmIcpError) as e:
        sym.Engine(mode=sym.MODE_COLOR, corr=sym.CORR_TREE)
    assert e.value.status == sym.ERR_HIP
    x = np.random.default_rng(0).normal(size=(16, 3)).astype(np.float32)
    with pytest.raises(sym.SymmIcpError) as e:
        sym.intensity_gradient(x, x, x[:, 0], 5)
    assert e.value.status == sym.ERR_HIP


# ---- the PCD reader ------------------------------------------------------------------------------------------------------------
XYZ = np.array([[0.0, 1.0, 2.0], [3.0, 4.0, 5.0], [6.0, 7.0, 8.0], [-1.0, -2.0, -3.0]], np.float32)
RGB = np.array([0x00FF0000, 0x00102030, 0x00000000, 0x00FFFFFF], np.uint32)
RGB_I = np.array([255, 0x10 + 0x20 + 0x30, 0, 765], np.float32) / np.float32(765.0)


def _header(fields, sizes, types, n, data):
    return ("# .PCD v0.7 - Point Cloud Data file format\nVERSION 0.7\nFIELDS %s\nSIZE %s\nTYPE %s\nCOUNT %s\nWIDTH %d\nHEIGHT 1\n"
            "VIEWPOINT 0 0 0 1 0 0 0\nPOINTS %d\nDATA %s\n" % (" ".join(fields), " ".join(map(str, sizes)), " ".join(types),
                                                              " ".join("1" for _ in fields), n, n, data))


def test_pcd_intensity_field_ascii_and_binary(sym, tmp_path):
    it = np.array([0.25, 0.5, 1.0, 100.0], np.float32)
    a = tmp_path / "i_ascii.pcd"
    a.write_text(_header(["x", "y", "z", "intensity"], [4, 4, 4, 4], "FFFF", 4, "ascii") +
                 "".join("%.9g %.9g %.9g %.9g\n" % (*XYZ[i], it[i]) for i in range(4)))
    got, kind = sym.pcd_read_intensity(str(a))
    assert kind == 1 and np.array_equal(got, it)
    # binary, the intensity a 1-byte unsigned field in front of the coordinates
    b = tmp_path / "i_bin.pcd"
    u8 = np.array([0, 7, 255, 128], np.uint8)
    with open(b, "wb") as f:
        f.write(_header(["intensity", "x", "y", "z"], [1, 4, 4, 4], "UFFF", 4, "binary").encode())
        for i in range(4):
            f.write(struct.pack("<Bfff", int(u8[i]), *XYZ[i]))
    got, kind = sym.pcd_read_intensity(str(b))
    assert kind == 1 and np.array_equal(got, u8.astype(np.float32))
    xyz, nrm = sym.pcd_read(str(b))                         # symmicp_pcd_read is unchanged: it skips the field
    assert np.array_equal(xyz, XYZ) and nrm is None
    # `intensity` wins over `rgb`
    c = tmp_path / "both.pcd"
    c.write_text(_header(["x", "y", "z", "rgb", "intensity"], [4, 4, 4, 4, 4], "FFFUF", 4, "ascii") +
                 "".join("%.9g %.9g %.9g %d %.9g\n" % (*XYZ[i], RGB[i], it[i]) for i in range(4)))
    got, kind = sym.pcd_read_intensity(str(c))
    assert kind == 1 and np.array_equal(got, it)


@pytest.mark.parametrize("name", ["rgb", "rgba"])
@pytest.mark.parametrize("typ", ["U", "F"])
@pytest.mark.parametrize("data", ["ascii", "binary"])
def test_pcd_rgb_field(sym, tmp_path, name, typ, data):
    p = tmp_path / "c.pcd"
    as_float = RGB.view(np.float32)
    with open(p, "wb") as f:
        f.write(_header(["x", "y", "z", name], [4, 4, 4, 4], "FFF" + typ, 4, data).encode())
        for i in range(4):
            if data == "binary":
                f.write(struct.pack("<fffI", *XYZ[i], int(RGB[i])))
            elif typ == "U":
                f.write(("%.9g %.9g %.9g %d\n" % (*XYZ[i], RGB[i])).encode())
            else:
                f.write(("%.9g %.9g %.9g %.9g\n" % (*XYZ[i], as_float[i])).encode())      # PCL's way: the word printed as a float
    got, kind = sym.pcd_read_intensity(str(p))
    assert kind == 2
    assert np.array_equal(got, RGB_I), (got, RGB_I)
    xyz, _ = sym.pcd_read(str(p))
    assert np.array_equal(xyz, XYZ)


def test_pcd_without_colours_and_bad_files(sym, tmp_path):
    p = tmp_path / "plain.pcd"
    sym.pcd_write(str(p), XYZ)
    got, kind = sym.pcd_read_intensity(str(p))
    assert got is None and kind == 0
    L = sym.lib()
    k = C.c_int(5)
    assert L.symmicp_pcd_read_intensity(os.fsencode(str(p)), None, 0, C.byref(k)) == 0 and k.value == 0
    with pytest.raises(sym.SymmIcpError) as e:
        sym.pcd_read_intensity(str(tmp_path / "missing.pcd"))
    assert e.value.status == sym.ERR_IO
    # an rgb field that is not a 4-byte U or F word is refused, a short file too, and a small buffer is ERR_SIZE
    bad = tmp_path / "bad.pcd"
    bad.write_text(_header(["x", "y", "z", "rgb"], [4, 4, 4, 2], "FFFU", 1, "ascii") + "0 0 0 1\n")
    assert L.symmicp_pcd_read_intensity(os.fsencode(str(bad)), None, 0, None) == -sym.ERR_IO
    short = tmp_path / "short.pcd"
    short.write_text(_header(["x", "y", "z", "rgb"], [4, 4, 4, 4], "FFFU", 3, "ascii") + "0 0 0 1\n0 0 0\n")
    out = np.zeros(3, np.float32)
    po = out.ctypes.data_as(C.POINTER(C.c_float))
    assert L.symmicp_pcd_read_intensity(os.fsencode(str(short)), po, 3, None) == -sym.ERR_IO
    assert L.symmicp_pcd_read_intensity(os.fsencode(str(short)), po, 2, None) == -sym.ERR_SIZE
