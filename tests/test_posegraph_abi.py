"""CPU tests of the C boundary of the pose-graph optimiser: the header still compiles as pedantic C99, the library exports the new entry
points, the structs have the sizes the bindings assume, every argument error that is decided before a device is needed comes back as
SYMMICP_ERR_ARG with the outputs untouched, the two host helpers match tests/_posegraph_ref.py, and with valid arguments and no device
the calls fail loudly."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import _posegraph_ref as R
from conftest import ROOT

NEW = ["symmicp_ctx_posegraph_optimize", "symmicp_posegraph_optimize", "symmicp_ctx_posegraph_pass", "symmicp_posegraph_edge_error"]


@pytest.fixture(scope="module")
def sym():
    import symmicp
    if not os.path.exists(symmicp.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    symmicp.lib()       # through the package: one HIP runtime in the process (see tests/test_abi.py)
    return symmicp


dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))


def test_library_exports_the_new_entry_points(sym):
    L = C.CDLL(sym.LIB_PATH)
    extra = ["symmicp_posegraph_config_default", "symmicp_posegraph_line_weight"]
    missing = [n for n in NEW + extra if not hasattr(L, n)]
    assert not missing, missing
    assert set(NEW + extra) <= set(sym.EXPORTS)
    hdr = open(os.path.join(ROOT, "include", "symmicp.h")).read()
    for n in NEW:
        assert "int %s(" % n in hdr, n
    assert "void symmicp_posegraph_config_default(" in hdr and "double symmicp_posegraph_line_weight(" in hdr
    assert sym.lib().symmicp_version() == 100                      # additive: the version stays
    for name in ("PoseEdge", "PosegraphConfig", "PosegraphResult", "PosegraphIteration", "posegraph_config", "posegraph_optimize",
                 "build_pose_graph", "multiway_registration", "posegraph_edge_error", "posegraph_line_weight"):
        assert hasattr(sym, name), name
    assert hasattr(sym.Engine, "posegraph_optimize") and hasattr(sym.Engine, "posegraph_pass")


def test_struct_sizes_and_defaults(sym):
    assert C.sizeof(sym.PoseEdge) == 16 + 16 * 8 + 36 * 8 and C.sizeof(sym.PosegraphConfig) == 72
    assert C.sizeof(sym.PosegraphResult) == 64 and C.sizeof(sym.PosegraphIteration) == 80
    cfg = sym.PosegraphConfig()
    sym.lib().symmicp_posegraph_config_default(C.byref(cfg))
    assert (cfg.struct_size, cfg.max_iterations, cfg.reference_node, cfg.cg_max_iterations) == (72, 100, 0, 0)
    assert (cfg.max_dist, cfg.preference_loop_closure, cfg.line_process_weight, cfg.edge_prune_threshold) == (0.0, 1.0, 0.0, 0.25)
    assert (cfg.min_relative_decrease, cfg.min_increment, cfg.cg_tolerance) == (1e-6, 1e-9, 1e-10)
    sym.lib().symmicp_posegraph_config_default(None)               # tolerated
    c2 = sym.posegraph_config(0.5, max_iterations=7, reference_node=2, cg_max_iterations=11, preference_loop_closure=2.0,
                              line_process_weight=3.0, edge_prune_threshold=0.5, min_relative_decrease=1e-3, min_increment=1e-4, cg_tolerance=1e-5)
    assert (c2.struct_size, c2.max_dist, c2.max_iterations, c2.reference_node, c2.cg_max_iterations, c2.preference_loop_closure,
            c2.line_process_weight, c2.edge_prune_threshold, c2.min_relative_decrease, c2.min_increment, c2.cg_tolerance) == \
        (72, 0.5, 7, 2, 11, 2.0, 3.0, 0.5, 1e-3, 1e-4, 1e-5)


def test_header_with_the_new_declarations_is_pedantic_c99(sym, tmp_path):
    """a C99 program that calls the entry points compiles without a warning, links, and gets status codes, not crashes"""
    src = tmp_path / "pg_abi.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "symmicp.h"
int main(void) {
    double X[32] = {0}, out[32], w[1], e6[6], ev[6], c1[1], l1[1], g[12], h[72], d[12];
    uint8_t pr[1];
    symmicp_pose_edge edge;
    symmicp_posegraph_config cfg;
    symmicp_posegraph_result res;
    symmicp_posegraph_iteration tr[100], rec;
    int a, b, c, k, s;
    for (k = 0; k < 2; k++) { X[16 * k] = X[16 * k + 5] = X[16 * k + 10] = X[16 * k + 15] = 1.0; }
    X[16 + 3] = 0.5;
    memset(&edge, 0, sizeof(edge));
    edge.source = 0; edge.target = 0;                                               /* refused: s == t */
    for (k = 0; k < 4; k++) edge.transform[5 * k] = 1.0;
    for (k = 0; k < 6; k++) edge.information[7 * k] = 1.0;
    symmicp_posegraph_config_default(&cfg);
    a = symmicp_posegraph_optimize(-1, X, 2, &edge, 1, &cfg, out, &res, w, pr, tr);
    b = symmicp_ctx_posegraph_optimize(NULL, X, 2, &edge, 1, &cfg, out, &res, w, pr, tr);
    c = symmicp_ctx_posegraph_pass(NULL, X, 2, &edge, 1, 0, 1.0, 0.0, 1e-10, 0, ev, c1, l1, g, h, d, &rec);
    s = symmicp_posegraph_edge_error(X, X + 16, edge.transform, e6);
    printf("status %d %d %d %d sizes %d %d %d %d e %.3f %.3f l %.4f caps %d %d\n", a, b, c, s, (int)sizeof(edge), (int)sizeof(cfg), (int)sizeof(res),
           (int)sizeof(rec), e6[0], e6[3], symmicp_posegraph_line_weight(1.0, 1.0), SYMMICP_POSEGRAPH_MAX_NODES, SYMMICP_POSEGRAPH_MAX_EDGES);
    return 0;
}
''')
    exe = tmp_path / "pg_abi_c"
    libdir = os.path.dirname(sym.LIB_PATH)
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                        "-L", libdir, "-lsymmicp", "-Wl,-rpath," + libdir], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    # E = X_t^-1 X_s with X_t = a shift of +0.5 in x: tau_x = -0.5
    assert "status 1 1 1 0 sizes 432 72 64 80 e 0.000 -0.500 l 0.2500 caps 1024 16384" in r.stdout, r.stdout


def _graph(n=4):
    rng = np.random.default_rng(7)
    truth, edges = R.make_graph(rng, n, R.ring_pairs(n), noise=0.01)
    return R.perturb(rng, truth, 0, 0.02), edges


class Call:
    """symmicp_posegraph_optimize on device -1 with sentinel-filled outputs; .untouched() after a refusal"""

    def __init__(self, sym, poses, edges, cfg):
        self.sym = sym
        self.X = np.ascontiguousarray(poses, np.float64)
        self.E = sym.pose_edges(edges) if edges is not None else None
        self.m = len(edges) if edges is not None else 1
        self.cfg = cfg
        self.out = np.full_like(self.X, -7.0)
        self.res = sym.PosegraphResult()
        C.memset(C.byref(self.res), 0x5A, C.sizeof(self.res))
        self.w = np.full(max(self.m, 1), -7.0)
        self.pr = np.full(max(self.m, 1), 9, np.uint8)
        self.tr = (sym.PosegraphIteration * 100)()
        C.memset(self.tr, 0x5A, C.sizeof(self.tr))

    def run(self, n=None, m=None, poses=True, out=True, res=True, ctx=False):
        L = self.sym.lib()
        f, head = (L.symmicp_ctx_posegraph_optimize, (None,)) if ctx else (L.symmicp_posegraph_optimize, (-1,))
        return f(*head, dp(self.X) if poses else None, len(self.X) if n is None else n, self.E, self.m if m is None else m,
                 None if self.cfg is None else C.byref(self.cfg), dp(self.out) if out else None, C.byref(self.res) if res else None,
                 dp(self.w), self.pr.ctypes.data_as(C.POINTER(C.c_uint8)), self.tr)

    def untouched(self):
        return (self.out == -7.0).all() and (self.w == -7.0).all() and (self.pr == 9).all() and \
            bytes(self.res) == b"\x5a" * C.sizeof(self.res) and bytes(self.tr) == b"\x5a" * C.sizeof(self.tr)


def test_every_refusal_is_err_arg_with_the_outputs_untouched(sym):
    poses, edges = _graph()
    cfg = lambda **kw: sym.posegraph_config(0.05, **kw)

    def refused(P=None, Eg=None, c=None, **run):
        call = Call(sym, poses if P is None else P, edges if Eg is None else Eg, cfg() if c is None else c)
        st = call.run(**run)
        return st == sym.ERR_ARG and call.untouched()

    # NULL required pointers, struct_size
    for run in (dict(poses=False), dict(out=False), dict(res=False)):
        assert refused(**run), run
    call = Call(sym, poses, edges, None)
    assert call.run() == sym.ERR_ARG and call.untouched()
    call = Call(sym, poses, None, cfg())
    assert call.run() == sym.ERR_ARG and call.untouched()
    bad = cfg(); bad.struct_size = 68
    assert refused(c=bad)
    # n and m
    for n in (0, 1, 1025):
        assert refused(n=n), n
    for m in (0, 16385):
        assert refused(m=m), m
    # node indices, s == t
    for k, (s, t) in ((0, (-1, 1)), (1, (1, 4)), (2, (2, 2)), (3, (7, 0))):
        e2 = list(edges)
        e2[k] = (s, t) + e2[k][2:]
        assert refused(Eg=e2), (s, t)
    # not connected: node 3 reachable only through the edges dropped here
    assert refused(Eg=[edges[0], (1, 0) + edges[0][2:]])
    # reference_node
    for ref in (-1, 4, 1000):
        assert refused(c=cfg(reference_node=ref)), ref
    # non-finite entries: X, T, the upper triangle of L (the lower one is not read)
    for val in (np.nan, np.inf, -np.inf):
        p2 = poses.copy(); p2[2, 1, 3] = val
        assert refused(P=p2)
        T2 = edges[1][3].copy(); T2[0, 3] = val
        assert refused(Eg=[edges[0], edges[1][:3] + (T2, edges[1][4])] + edges[2:])
        L2 = edges[2][4].copy(); L2[1, 4] = val
        assert refused(Eg=edges[:2] + [edges[2][:4] + (L2,)] + edges[3:])
    L3 = edges[2][4].copy(); L3[4, 1] = np.nan                      # below the diagonal: accepted as far as the arguments go
    call = Call(sym, poses, edges[:2] + [edges[2][:4] + (L3,)] + edges[3:], cfg())
    assert call.run() != sym.ERR_ARG
    p3 = poses.copy(); p3[1, 3] = np.nan                            # the bottom row is not read either
    assert Call(sym, p3, edges, cfg()).run() != sym.ERR_ARG
    # rotation blocks
    p2 = poses.copy(); p2[3, :3, :3] *= 1.0 + 1e-6
    assert refused(P=p2)
    T2 = edges[0][3].copy(); T2[0, 1] += 1e-5
    assert refused(Eg=[edges[0][:3] + (T2, edges[0][4])] + edges[1:])
    p2 = poses.copy(); p2[3, :3, :3] *= 1.0 + 1e-8                  # within 1e-6: accepted
    assert Call(sym, p2, edges, cfg()).run() != sym.ERR_ARG
    # max_dist, while mu has to be derived from it
    for v in (0.0, -1.0, np.inf, np.nan):
        c = cfg(); c.max_dist = v
        assert refused(c=c), v
        c.line_process_weight = 2.0                                  # given: max_dist is not needed
        assert Call(sym, poses, edges, c).run() != sym.ERR_ARG
        c.line_process_weight = 0.0
        assert Call(sym, poses, [e[:2] + (0,) + e[3:] for e in edges], c).run() != sym.ERR_ARG      # no uncertain edge: neither
    for v in (0.0, -1.0, np.inf, np.nan):
        assert refused(c=cfg(preference_loop_closure=v)), v
    # thresholds outside their ranges
    for kw in (dict(max_iterations=0), dict(max_iterations=-1), dict(max_iterations=10001), dict(cg_max_iterations=-1), dict(cg_max_iterations=100001),
               dict(line_process_weight=-1.0), dict(line_process_weight=np.inf), dict(line_process_weight=np.nan),
               dict(edge_prune_threshold=-0.1), dict(edge_prune_threshold=1.1), dict(edge_prune_threshold=np.nan),
               dict(min_relative_decrease=-1e-9), dict(min_relative_decrease=np.inf), dict(min_relative_decrease=np.nan),
               dict(min_increment=-1e-9), dict(min_increment=np.inf), dict(min_increment=np.nan),
               dict(cg_tolerance=0.0), dict(cg_tolerance=1.0), dict(cg_tolerance=-1e-3), dict(cg_tolerance=np.nan)):
        assert refused(c=cfg(**kw)), kw
    # the context forms with no context
    assert Call(sym, poses, edges, cfg()).run(ctx=True) == sym.ERR_ARG
    X, E = np.ascontiguousarray(poses), sym.pose_edges(edges)
    assert sym.lib().symmicp_ctx_posegraph_pass(None, dp(X), 4, E, 4, 0, 1.0, 0.0, 1e-10, 0, None, None, None, None, None, None, None) == sym.ERR_ARG
    with pytest.raises(ValueError):
        sym.posegraph_optimize(poses[:, :3], edges, 0.05)
    with pytest.raises(ValueError):
        sym.pose_edges([(0, 1, 0, np.eye(3), np.eye(6))])


def test_host_helpers_match_the_reference(sym):
    rng = np.random.default_rng(8)
    sizes = [0.0, 1e-9, 5e-5, 2e-4, 1e-2, 1.0, 2.5, 3.0, np.pi - 1e-6]
    for size in sizes:
        Xs, Xt = R.random_pose(rng, 2.0, 3.0), R.random_pose(rng, 2.0, 3.0)
        w = rng.normal(size=3)
        w *= size / np.linalg.norm(w)
        D = np.eye(4)
        D[:3, :3] = R.exp_rot(w)
        D[:3, 3] = rng.uniform(-1, 1, 3)
        T = R.inv_rigid(D) @ R.relative(Xs, Xt)                     # E = X_t^-1 X_s T^-1 = D up to rounding
        e, ref = sym.posegraph_edge_error(Xs, Xt, T), R.edge_error(Xs, Xt, T)
        # the two evaluate one formula in two association orders on an E known to ~1e-15: they agree as far as the log is conditioned
        assert np.abs(e - ref).max() <= 1e-13 * (1.0 if size < 3.1 else 1e7), (size, e, ref)
        if size < 3.1:
            assert np.abs(e[:3] - w).max() <= 1e-12 and np.abs(e[3:] - D[:3, 3]).max() <= 1e-14
    assert sym.lib().symmicp_posegraph_edge_error(None, None, None, None) == sym.ERR_ARG
    for mu, c in ((1.0, 0.0), (1.0, 1.0), (2.5, 7.0), (1e-3, 1e3), (850.0, 1e-6)):
        assert sym.posegraph_line_weight(mu, c) == R.line_weight(mu, c)


def test_posegraph_fails_loudly_without_gpu(sym):
    """valid arguments and no device: SYMMICP_ERR_HIP from the context the call creates, no CPU fallback, no output"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    poses, edges = _graph()
    call = Call(sym, poses, edges, sym.posegraph_config(0.05))
    assert call.run() == sym.ERR_HIP and call.untouched()
    with pytest.raises(sym.SymmIcpError) as e:
        sym.posegraph_optimize(poses, edges, 0.05)
    assert e.value.status == sym.ERR_HIP
    with pytest.raises(sym.SymmIcpError) as e:
        sym.multiway_registration([np.zeros((4, 3), np.float32)] * 2, [np.zeros((4, 3), np.float32)] * 2, [(1, 0, 0, None)], 0.05)
    assert e.value.status == sym.ERR_HIP
