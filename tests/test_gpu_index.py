"""GPU tests of the index build itself (run with -m gpu on a real MI355X): kernels_build.hip and the packet table of
kernels_packet.hip against tests/_index_ref.py, through the read-only test entries of engine_probe.cpp.

An exact search hides a bad index: the searches prune by the boxes and ranges actually stored, so a wrong but conservative index
still returns bit-exact neighbours, only slower, and a wrong one that is not conservative loses neighbours only for the queries
that meet the defect.  Here every array and every scalar of the index is compared with a plain numpy restatement, with no tolerance
anywhere: integers by their bits, floats by value.

  1. primitives: the stable LSD radix sort against np.argsort(kind="stable"), the multi-block exclusive scan against np.cumsum, at
     sizes that straddle every tile constant of the code and with every key width the engine passes;
  2. the whole index of cat, bunny, c3_uniform 100k, c4_surface 1M and a c5_scan sample, plus the structural walk of the octree;
  3. edge clouds;
  4. forced shapes (grid level, octree leaf size, first-pass regime, points per cell), in child processes: the switches are read
     once in symmicp_create;
  5. the source share's order and the packet table's invariants, sharded and not, with the cost key on and off;
  6. the probes leave the context alone.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import _index_ref as R

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def sym():
    import symmicp
    symmicp.lib()
    return symmicp


@pytest.fixture(scope="module")
def eng(sym):
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        yield e


def _env_shape():
    """the shape switches of this process as build_reference's arguments (symmicp_create reads the same variables)"""
    env = os.environ
    kw = {}
    if "SYMMICP_GRID_PPC" in env:
        kw["grid_ppc"] = float(env["SYMMICP_GRID_PPC"])
    if "SYMMICP_GRID_MAXLEVEL" in env:
        kw["grid_maxlevel"] = int(env["SYMMICP_GRID_MAXLEVEL"])
    if "SYMMICP_GRID_LEVEL" in env:
        kw["grid_level"] = int(env["SYMMICP_GRID_LEVEL"])
    if "SYMMICP_FIRST_PASS" in env:
        kw["first_pass"] = 1 if env["SYMMICP_FIRST_PASS"][0] == "p" else 0
    if "SYMMICP_OCT_LEAF" in env:
        kw["oct_leaf"] = int(env["SYMMICP_OCT_LEAF"])
    return kw


def _pseudo_normals(n, seed=5):
    v = np.random.default_rng(seed).standard_normal((n, 3)).astype(f32)
    return v


def _check_target(e, xyz, nrm=None, **kw):
    """set_target, read the index back, compare everything with the reference -> (ref, got)"""
    xyz = np.ascontiguousarray(xyz, f32)
    nrm = _pseudo_normals(len(xyz)) if nrm is None else np.ascontiguousarray(nrm, f32)
    e.set_target(xyz, nrm)
    got = e.index_arrays()
    shape = _env_shape()
    shape.update(kw)
    ref = R.build_reference(xyz, nrm, **shape)
    leaves = R.check_index(ref, got)
    st = e.stats()
    assert st["grid_level"] == got["grid_level"] == ref["grid_level"]
    assert st["tree_levels"] == got["tree_levels"] == ref["tree_levels"]
    assert 1 <= leaves <= len(xyz)
    return ref, got


# ----------------------------------------------------------------------------------------------------------------------------------
# 1. primitives
# ----------------------------------------------------------------------------------------------------------------------------------
# every tile constant: 64 (wave), 256 (block), 2048 (scan tile), 4096 (sort tile), 16384 (above: the sort's histogram has more than
# 1024 words, k_rs_scan walks several words per thread), 2097152 (above: the scan's tile totals exceed 1024), and one odd large size
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385, 2097151, 2097152, 2097153, 8388611]
# 3 * kMortonBits (morton_order), the packets' 16 and 32 (set_source), the voxel sort's ceil(log2(voxels)) -- anything in 0 .. 32: its
# extremes 1 and 17 -- and 8 and 24, which are rounded up to an even pass count
KEY_BITS = [30, 16, 32, 8, 24, 1, 17]
PATTERNS = ["equal", "iota", "reversed", "random", "top-digit", "bottom-digit", "dup90"]


def _keys(pattern, n, kb, rng):
    mask = (1 << kb) - 1
    i = np.arange(n, dtype=np.uint64)
    r = rng.integers(0, mask + 1, n, dtype=np.uint64)
    if pattern == "equal":
        k = np.full(n, mask, np.uint64)
    elif pattern == "iota":
        k = i & np.uint64(mask)
    elif pattern == "reversed":
        k = (np.uint64(max(n, 1) - 1) - i) & np.uint64(mask)
    elif pattern == "random":
        k = r
    elif pattern == "top-digit":           # only the top 8 bits vary
        lowbits = max(kb - 8, 0)
        k = ((r >> np.uint64(lowbits)) << np.uint64(lowbits)) | np.uint64(0x155555 & ((1 << lowbits) - 1))
    elif pattern == "bottom-digit":        # only the bottom 8 bits vary
        k = (r & np.uint64(0xFF)) | np.uint64(mask & 0x2AAAAA00)
    else:                                  # 90 % of the keys are one value
        k = np.where(rng.random(n) < 0.9, np.uint64(mask // 3), r)
    assert n == 0 or int(k.max()) <= mask
    return k.astype(np.uint32)


def _check_sort(e, keys, kb, what, vals=None):
    n = len(keys)
    vals = np.arange(n, dtype=np.uint32) if vals is None else vals
    k, v = e.radix_sort_probe(keys, vals, kb)
    order = np.argsort(keys, kind="stable")
    bad = np.flatnonzero(k != keys[order])
    assert not len(bad), "%s: key[%d] = %d, expected %d (%d differ)" % (what, bad[0], k[bad[0]], keys[order][bad[0]], len(bad))
    bad = np.flatnonzero(v != vals[order])
    assert not len(bad), "%s: val[%d] = %d, expected %d (%d differ: not stable, or a value lost)" % (what, bad[0], v[bad[0]], vals[order][bad[0]], len(bad))


@pytest.mark.parametrize("n", SIZES)
def test_radix_sort_against_stable_argsort(eng, n):
    """every pattern x every key width (above 2M: every pattern at 30 bits, random keys at every width)"""
    rng = np.random.default_rng(n + 1)
    big = n > 100000
    for kb in KEY_BITS:
        for pat in PATTERNS:
            if big and kb != 30 and pat != "random":
                continue
            _check_sort(eng, _keys(pat, n, kb, rng), kb, "n=%d bits=%d %s" % (n, kb, pat))


def test_radix_sort_carries_arbitrary_values_and_zero_bits(eng):
    rng = np.random.default_rng(7)
    for n in (1, 65, 4097, 70001):
        keys = _keys("dup90", n, 30, rng)
        vals = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
        _check_sort(eng, keys, 30, "n=%d arbitrary values" % n, vals)
        k, v = eng.radix_sort_probe(np.zeros(n, np.uint32), vals, 0)          # a single voxel: no pass runs, nothing moves
        assert not k.any() and np.array_equal(v, vals)


@pytest.mark.parametrize("n", SIZES)
def test_exclusive_scan_against_cumsum(eng, n):
    rng = np.random.default_rng(n + 3)
    top = np.full(n, (2 ** 32 - 1) // max(n, 1), np.uint64)
    if n:
        top[rng.integers(0, n)] += np.uint64((2 ** 32 - 1) - int(top.sum()))       # the total is 2^32 - 1: the last sums do not wrap
    inputs = dict(zero=np.zeros(n, np.uint64), one=np.ones(n, np.uint64), flags=(rng.random(n) < 0.3).astype(np.uint64), total_2_32_m1=top)
    for name, d in inputs.items():
        assert n == 0 or int(d.sum()) <= 2 ** 32 - 1
        got = eng.scan_probe(d.astype(np.uint32))
        want = (np.cumsum(d) - d).astype(np.uint32)
        bad = np.flatnonzero(got != want)
        assert not len(bad), "n=%d %s: scan[%d] = %d, expected %d (%d differ)" % (n, name, bad[0], got[bad[0]], want[bad[0]], len(bad))


def test_primitive_argument_errors(sym, eng):
    L = sym.lib()
    u = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    k, v = np.arange(8, dtype=np.uint32), np.arange(8, dtype=np.uint32)
    assert L.symmicp_ctx_radix_sort_probe(eng._h, u(k), u(v), 8, 33) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(eng._h, u(k), u(v), 8, -1) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(eng._h, None, u(v), 8, 30) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(eng._h, u(k), None, 8, 30) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(eng._h, u(k), u(v), 2 ** 31, 30) == sym.ERR_ARG
    assert L.symmicp_ctx_scan_probe(eng._h, None, 8) == sym.ERR_ARG
    assert L.symmicp_ctx_scan_probe(eng._h, u(k), 2 ** 31) == sym.ERR_ARG
    assert L.symmicp_ctx_radix_sort_probe(eng._h, None, None, 0, 30) == sym.OK and L.symmicp_ctx_scan_probe(eng._h, None, 0) == sym.OK
    assert (k == np.arange(8)).all() and (v == np.arange(8)).all()
    info = sym.IndexInfo()
    info.struct_size = C.sizeof(sym.IndexInfo) - 4
    assert L.symmicp_ctx_index_info(eng._h, C.byref(info)) == sym.ERR_ARG and L.symmicp_ctx_index_info(eng._h, None) == sym.ERR_ARG


# ----------------------------------------------------------------------------------------------------------------------------------
# 2. the whole index of the workloads
# ----------------------------------------------------------------------------------------------------------------------------------
_DATA = {}


def _cloud(name, cat=None, bunny=None):
    if name not in _DATA:
        from symmicp import synth
        if name == "cat":
            _DATA[name] = dict(src=cat["src"], src_n=cat["src_n"], tgt=cat["tgt"], tgt_n=cat["tgt_n"])
        elif name == "bunny":
            _DATA[name] = dict(tgt=bunny, tgt_n=_pseudo_normals(len(bunny)))
        elif name == "c3_100k":
            _DATA[name] = synth.c3_uniform(100_000)
        elif name == "c4_1m":
            _DATA[name] = synth.c4_surface(1_000_000)
        elif name == "c4_100k":
            _DATA[name] = synth.c4_surface(100_000)
        elif name == "c5":
            _DATA[name] = synth.c5_scan(64 * 1500)
    return _DATA[name]


@pytest.mark.parametrize("name", ["cat", "bunny", "c3_100k", "c4_1m", "c5"])
def test_index_of_the_workloads(sym, cat, bunny, name):
    d = _cloud(name, cat, bunny)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        ref, got = _check_target(e, d["tgt"], d["tgt_n"])
    if name == "c3_100k":
        assert not ref["surface_like"] and ref["leaf_max"] == 8                      # a volume: the per-thread walk, small leaves
    if name == "c4_1m":
        assert ref["surface_like"] and ref["leaf_max"] == 24 and ref["grid_level"] == 8 and ref["n_onodes"] == 1382686


# ----------------------------------------------------------------------------------------------------------------------------------
# 3. edges
# ----------------------------------------------------------------------------------------------------------------------------------
def _edge_clouds():
    rng = np.random.default_rng(11)
    out = {}
    for n in (1, 2, 8, 9, 64, 65, 4096, 4097):
        out["n=%d" % n] = rng.random((n, 3)).astype(f32)
    out["identical"] = np.tile(np.array([[0.25, -3.0, 7.5]], f32), (300, 1))                      # extent 0: emax = 1
    slab = rng.random((5000, 3)).astype(f32); slab[:, 2] = f32(0.125)
    out["slab"] = slab
    needle = np.zeros((3000, 3), f32); needle[:, 0] = rng.random(3000).astype(f32) * f32(50)
    out["needle"] = needle
    neg = (rng.random((4000, 3)).astype(f32) - f32(0.5)) * f32(4)
    neg[::7, 1] = f32(-0.0); neg[3::7, 1] = f32(0.0); neg[::5, 0] = neg[:, 0].min(); neg[1::9, 2] = f32(-0.0)
    out["negative-and-minus-zero"] = neg
    out["shifted-1e6"] = (rng.random((6000, 3)).astype(f32) + f32(1.0e6)).astype(f32)             # 16 values per axis: many equal keys
    edge = rng.random((3000, 3)).astype(f32)
    edge[:400] = np.where(rng.random((400, 3)) < 0.5, f32(1.0), edge[:400]); edge[0] = 1.0; edge[1] = 0.0
    out["on-the-box-maximum"] = edge                                                              # cell 1024 clamps to 1023
    h0 = f32(f32(1.00001) / f32(1024))
    lat = (rng.integers(0, 1024, (6000, 3)).astype(f32) * h0).astype(f32)                         # k * h0: exactly on cell faces
    lat[0] = 0.0; lat[1] = 1.0                                                                    # (pins the extent, hence h0)
    out["lattice-on-cell-faces"] = lat
    sparse = rng.random((200, 3)).astype(f32)
    out["forty-copies"] = np.concatenate([np.tile(sparse[17:18], (40, 1)), sparse])[rng.permutation(240)]
    return out


_EDGES = _edge_clouds()


@pytest.mark.parametrize("name", list(_EDGES))
def test_index_of_edge_clouds(eng, name):
    xyz = _EDGES[name]
    ref, got = _check_target(eng, xyz)
    if name == "lattice-on-cell-faces":
        assert ref["h0"] == f32(f32(1.00001) / f32(1024))
    if name == "identical":
        assert ref["h0"] == f32(f32(1.00001) / f32(1024)) and not ref["keys"].any() and ref["order"].tolist() == list(range(300))
    if name == "on-the-box-maximum":
        assert (R.cell_of_key(ref["keys"]).max(0) == 1023).all()
    if name == "forty-copies":
        w = got["onodes"].view(np.uint32)
        a, b = int(got["olevel_off"][10]), int(got["olevel_off"][11])
        assert ((w[a:b, 1, 3] >> 28) == 0).all() and int(w[a:b, 1, 3].max()) >= 40 > got["leaf_max"]      # a level-10 leaf above leaf_max


def test_non_finite_target_is_refused_and_leaves_no_index(sym, eng):
    good = _EDGES["n=4097"]
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[1234, 1] = bad_value
        with pytest.raises(sym.SymmIcpError) as ex:
            eng.set_target(bad, _pseudo_normals(len(bad)))
        assert ex.value.status == sym.ERR_ARG
        for probe in (eng.index_info, eng.index_arrays):
            with pytest.raises(sym.SymmIcpError) as ex:
                probe()
            assert ex.value.status == sym.ERR_STATE
    _check_target(eng, good)


def test_probes_need_a_tree_context_with_a_target_and_a_source(sym):
    xyz = _EDGES["n=4097"]
    for corr in (sym.CORR_IDENTITY, sym.CORR_BRUTE):
        with sym.Engine(mode=sym.MODE_PAPER, corr=corr) as e:
            e.set_target(xyz, _pseudo_normals(len(xyz)))
            with pytest.raises(sym.SymmIcpError) as ex:
                e.index_info()
            assert ex.value.status == sym.ERR_STATE
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        for probe in (e.index_info, e.source_share):
            with pytest.raises(sym.SymmIcpError) as ex:
                probe()
            assert ex.value.status == sym.ERR_STATE
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, sort_source=0) as e:
        e.set_source(xyz, _pseudo_normals(len(xyz)))
        s = e.source_share()
        assert not s["sorted"] and s["order"] is None and s["n_local"] == len(xyz)
        o = np.zeros(len(xyz), np.uint32)
        st = e._L.symmicp_ctx_source_share(e._h, None, None, None, None, o.ctypes.data_as(C.POINTER(C.c_uint32)), None)
        assert st == sym.ERR_STATE and not o.any()


# ----------------------------------------------------------------------------------------------------------------------------------
# 5. source share and packets (before 4: the child processes of 4 run these too)
# ----------------------------------------------------------------------------------------------------------------------------------
def _env_packets():
    env = os.environ
    return dict(order=env.get("SYMMICP_PACKET_ORDER", "1")[0] != "0", jump=float(env.get("SYMMICP_PACKET_JUMP", "-1")),
                key_bits=int(env.get("SYMMICP_PACKET_KEY_BITS", "16")), cost_key=env.get("SYMMICP_PACKET_COST_KEY", "1")[0] != "0")


def _check_share(e, src, b0, bc, target_ref):
    """order and packet table of the share e holds (rows b0 .. b0 + bc of src) -> the share dict"""
    sw = _env_packets()
    s = e.source_share()
    assert s["n_local"] == bc == e.local_count() and e.local_offset() == b0 and s["sorted"]
    want = R.share_order(src, b0, bc)
    bad = np.flatnonzero(s["order"] != want)
    assert not len(bad), "share order[%d] = %d, expected %d (%d differ)" % (bad[0], s["order"][bad[0]], want[bad[0]], len(bad))
    nblk = (bc + 63) // 64
    if not sw["order"]:
        assert s["pkt_count"] == 0 and not s["cost_keyed"]            # packets as they lie: no table
        return s
    tab = s["pkt_tab"]
    assert nblk <= s["pkt_count"] == len(tab) <= 8 * nblk
    assert s["cost_keyed"] == (target_ref is not None and sw["cost_key"] and sw["key_bits"] > 0)
    pts = np.ascontiguousarray(src, f32)[want]
    if sw["key_bits"] <= 0:
        keys = -tab[:, 0].astype(np.int64)                          # Morton order: ascending first query
    elif s["cost_keyed"]:
        keys = R.cost_keys(pts, tab, target_ref, sw["key_bits"])
    else:
        keys = R.radius_keys(pts, tab, sw["key_bits"])
    R.check_packets(bc, tab, keys)
    if sw["jump"] == 0:
        assert s["pkt_count"] == nblk and sorted(map(tuple, tab.tolist())) == [(64 * b, min(64, bc - 64 * b)) for b in range(nblk)]
    return s


@pytest.mark.parametrize("with_target", [False, True], ids=["radius-key", "cost-key"])
@pytest.mark.parametrize("name", ["cat", "c4_100k"])
def test_forced_source_share_and_packets(sym, cat, name, with_target):
    d = _cloud(name, cat)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        ref = _check_target(e, d["tgt"], d["tgt_n"])[0] if with_target else None
        e.set_source(d["src"], d["src_n"])
        s = _check_share(e, d["src"], 0, len(d["src"]), ref)
        e.set_source(d["src"], d["src_n"])                           # again: the same table, up to the order inside equal keys
        s2 = e.source_share()
        assert np.array_equal(s["order"], s2["order"]) and s["pkt_count"] == s2["pkt_count"]
        assert sorted(map(tuple, s["pkt_tab"].tolist())) == sorted(map(tuple, s2["pkt_tab"].tolist()))


def test_share_and_packets_c4_1m_cost_key(sym):
    d = _cloud("c4_1m")
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        ref, _ = _check_target(e, d["tgt"], d["tgt_n"])
        e.set_source(d["src"], d["src_n"])
        _check_share(e, d["src"], 0, len(d["src"]), ref)


@pytest.mark.parametrize("world", [2, 5])
@pytest.mark.parametrize("name", ["cat", "c4_100k"])
def test_sharded_source_shares(sym, cat, name, world):
    d = _cloud(name, cat)
    n = len(d["src"])
    covered = np.zeros(n, int)
    for rank in range(world):
        b0, bc = R.shard_range(n, world, rank)
        a, b = C.c_size_t(0), C.c_size_t(0)
        assert sym.lib().symmicp_shard_range(n, world, rank, C.byref(a), C.byref(b)) == sym.OK and (a.value, b.value) == (b0, bc)
        with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
            e.comm_init_rank(world, rank, None)
            ref = _check_target(e, d["tgt"], d["tgt_n"])[0] if rank % 2 == 0 else None      # cost key on even ranks, radius key on odd ones
            e.set_source(d["src"], d["src_n"])
            s = _check_share(e, d["src"], b0, bc, ref)
            covered[s["order"]] += 1
    assert (covered == 1).all()


def _two_clusters():
    x = np.concatenate([np.arange(32) * 0.001, 100.0 + np.arange(32) * 0.001])
    return np.stack([x, np.zeros(64), np.zeros(64)], 1).astype(f32)


def _evenly_spaced():
    return np.stack([np.arange(64.0), np.zeros(64), np.zeros(64)], 1).astype(f32)


def test_forced_hand_built_jump(sym):
    """the cut itself: a block of two tight clusters far apart is cut exactly at the jump, a block of evenly spaced points is not cut
    (SYMMICP_PACKET_JUMP=0, in a child process: never cut)"""
    sw = _env_packets()
    never = sw["jump"] == 0
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        for pts, want in ((_two_clusters(), [(0, 64)] if never else [(0, 32), (32, 32)]), (_evenly_spaced(), [(0, 64)])):
            e.set_source(pts, _pseudo_normals(64))
            s = _check_share(e, pts, 0, 64, None)
            assert s["order"].tolist() == list(range(64))
            if not sw["order"]:
                want = []            # SYMMICP_PACKET_ORDER=0: no table at all, the first pass takes the 64 queries as they lie
            assert sorted(map(tuple, s["pkt_tab"].tolist())) == want


# ----------------------------------------------------------------------------------------------------------------------------------
# 4. forced shapes, in child processes
# ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["cat", "c4_100k"])
def test_forced_target_index(sym, cat, name):
    """(in this process: the default shape; in the children below: under every switch)"""
    d = _cloud(name, cat)
    with sym.Engine(mode=sym.MODE_PAPER, corr=sym.CORR_TREE) as e:
        ref, got = _check_target(e, d["tgt"], d["tgt_n"])
    env = os.environ
    if "SYMMICP_GRID_LEVEL" in env:
        assert got["grid_level"] == int(env["SYMMICP_GRID_LEVEL"]) and (got["grid_level"] > 0 or (got["gdim"] == 0 and got["n_blocks"] == 0))
    if "SYMMICP_OCT_LEAF" in env:
        assert got["leaf_max"] == int(env["SYMMICP_OCT_LEAF"])
    if "SYMMICP_FIRST_PASS" in env:
        assert got["surface_like"] == (env["SYMMICP_FIRST_PASS"] == "packet")
    if not set(env) & {"SYMMICP_OCT_LEAF", "SYMMICP_FIRST_PASS", "SYMMICP_GRID_LEVEL", "SYMMICP_GRID_PPC"}:
        assert got["leaf_max"] == (24 if got["surface_like"] else 8)       # the defaults of build_index


_FORCED = {
    "grid-level-0": dict(SYMMICP_GRID_LEVEL="0"), "grid-level-1": dict(SYMMICP_GRID_LEVEL="1"), "grid-level-3": dict(SYMMICP_GRID_LEVEL="3"),
    "grid-level-4": dict(SYMMICP_GRID_LEVEL="4"), "grid-level-10": dict(SYMMICP_GRID_LEVEL="10"),
    "oct-leaf-1": dict(SYMMICP_OCT_LEAF="1"), "oct-leaf-8": dict(SYMMICP_OCT_LEAF="8"), "oct-leaf-64": dict(SYMMICP_OCT_LEAF="64"),
    "first-pass-packet": dict(SYMMICP_FIRST_PASS="packet"), "first-pass-walk": dict(SYMMICP_FIRST_PASS="walk"),
    "grid-ppc-1": dict(SYMMICP_GRID_PPC="1.0"), "grid-ppc-12": dict(SYMMICP_GRID_PPC="12"),
    "packet-order-0": dict(SYMMICP_PACKET_ORDER="0"), "packet-jump-0": dict(SYMMICP_PACKET_JUMP="0"),
}


@pytest.mark.parametrize("shape", list(_FORCED))
def test_forced_shapes_in_a_subprocess(sym, shape):
    """The switches are read once in symmicp_create: rerun the test_forced_* tests of this module in a child under each of them."""
    import subprocess
    env = dict(os.environ, **_FORCED[shape])
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_forced_ and not subprocess"],
                       env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


# ----------------------------------------------------------------------------------------------------------------------------------
# 6. the probes leave the context alone
# ----------------------------------------------------------------------------------------------------------------------------------
def _all_probes(e):
    rng = np.random.default_rng(3)
    e.index_info()
    a = e.index_arrays()
    e.source_share()
    e.radix_sort_probe(rng.integers(0, 2 ** 30, 300001, dtype=np.uint64).astype(np.uint32), np.arange(300001, dtype=np.uint32), 30)
    e.scan_probe(np.ones(300001, np.uint32))
    return a


def _same_bytes(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


@pytest.mark.parametrize("name", ["cat", "c4_100k"])
def test_probes_leave_the_context_alone(sym, cat, name):
    d = _cloud(name, cat)
    cfg = dict(mode=sym.MODE_PAPER, corr=sym.CORR_TREE, max_iters=30)
    with sym.Engine(**cfg) as fresh, sym.Engine(**cfg) as e:
        for x in (fresh, e):
            x.set_target(d["tgt"], d["tgt_n"])
        a0 = _all_probes_target_only(e)
        for x in (fresh, e):
            x.set_source(d["src"], d["src_n"])
        a1 = _all_probes(e)
        _same_bytes(a0, a1)                                          # two read-backs of one target: byte-identical
        for round_ in range(2):
            rf, re_ = fresh.align(), e.align()
            assert rf["status"] == re_["status"] == 0 and rf["iters"] == re_["iters"]
            assert rf["transform"].tobytes() == re_["transform"].tobytes() and rf["diffs"].tobytes() == re_["diffs"].tobytes()
            # (PAPER applies cumulatively: the moved source is never materialised, the transform stands for it)
            st0, cert0, corr0, src0 = e.stats(), e.certificates(), e.correspondences(), (e.transform(), e.pivot())
            _same_bytes(a0, _all_probes(e))
            st1 = e.stats()
            assert st0 == st1
            for u, v in zip(cert0 + corr0 + src0, e.certificates() + e.correspondences() + (e.transform(), e.pivot())):
                assert u.tobytes() == v.tobytes()
            for u, v in zip(fresh.correspondences(), corr0):      # (certificates may depend on the packets' order inside equal start keys)
                assert u.tobytes() == v.tobytes()
        e.set_target(d["tgt"], d["tgt_n"])                           # the same target built again: the same bytes
        _same_bytes(a0, e.index_arrays())


def _all_probes_target_only(e):
    a = e.index_arrays()
    e.scan_probe(np.ones(5000, np.uint32))
    e.radix_sort_probe(np.arange(5000, dtype=np.uint32)[::-1], np.arange(5000, dtype=np.uint32), 16)
    return a
