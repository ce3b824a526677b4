"""CPU tests of tests/_index_ref.py, the numpy restatement the GPU index is compared with (tests/test_gpu_index.py):
  * against brute force on small clouds: per-cell enumeration for the table, per-prefix enumeration for the octree and the histogram,
    per-leaf loops for the box tree;
  * hand-worked clouds of 1, 2 and 9 points;
  * negative controls: every checker is fed the reference's own output with ONE defect of the kind a subtly wrong kernel would
    produce, and has to reject it by name.  This is how the suite shows that it would notice such a kernel: nothing is ever broken on
    purpose on a GPU.
"""
import copy

import numpy as np
import pytest

import _index_ref as R

f32 = np.float32


def _cloud(n, seed, dup=0, surface=False):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)).astype(f32)
    if surface:
        p[:, 2] = (0.2 * np.sin(5 * p[:, 0]) * np.cos(3 * p[:, 1])).astype(f32)
    if dup:
        p[rng.integers(0, n, dup)] = p[7]
    nrm = rng.standard_normal((n, 3)).astype(f32)
    return p, nrm


CLOUDS = [("uniform-700", dict(n=700, seed=1)), ("surface-3000-dups", dict(n=3000, seed=2, dup=40, surface=True)),
          ("tiny-65", dict(n=65, seed=3))]


@pytest.fixture(scope="module", params=CLOUDS, ids=[c[0] for c in CLOUDS])
def ref(request):
    p, nrm = _cloud(**request.param[1])
    r = R.build_reference(p, nrm)
    r["_xyz"], r["_nrm"] = p, nrm
    return r


# ---- against brute force ------------------------------------------------------------------------------------------------------
def test_keys_are_the_interleaved_cells_and_the_order_is_stable(ref):
    p = ref["_xyz"]
    lo = p.min(0)
    cells = R.cell_of_key(ref["keys"])
    inv = f32(1) / ref["h0"]
    for i in range(0, len(p), max(1, len(p) // 200)):
        row = int(ref["order"][i])
        for a in range(3):
            c = int(np.floor(f32(f32(p[row, a] - lo[a]) * inv)))
            assert cells[i, a] == min(max(c, 0), 1023)
    k = ref["keys"].astype(np.int64)
    assert (k[1:] >= k[:-1]).all()
    eq = k[1:] == k[:-1]
    assert (ref["order"][1:][eq] > ref["order"][:-1][eq]).all()
    assert sorted(ref["order"].tolist()) == list(range(len(p)))
    assert np.array_equal(ref["tq"][:, :3], p[ref["order"]]) and np.array_equal(ref["tn"][:, 1, :3], ref["_nrm"][ref["order"]])
    assert np.array_equal(ref["tq"].view(np.uint32)[:, 3], ref["order"].astype(np.uint32))


def test_box_tree_against_per_node_loops(ref):
    n, pts, B, off = ref["n"], ref["tq"][:, :3], ref["boxes"], ref["level_off"]
    nleaf = (n + 7) // 8
    for l in range(nleaf):
        seg = pts[8 * l:8 * l + 8]
        assert np.array_equal(B[l, 0, :3], seg.min(0)) and np.array_equal(B[l, 1, :3], seg.max(0))
    # every level: node p covers sorted points 8^(l+1) p ..; beyond the data the boxes are (+inf, -inf)
    span, l, cnt = 8, 0, nleaf
    while True:
        width = (int(off[l + 1]) if l < ref["top"] else ref["n_boxes"]) - int(off[l])
        for p_ in range(width):
            seg = pts[span * p_:span * (p_ + 1)]
            b = B[int(off[l]) + p_]
            if len(seg):
                assert np.array_equal(b[0, :3], seg.min(0)) and np.array_equal(b[1, :3], seg.max(0)), (l, p_)
            else:
                assert (b[0, :3] == np.inf).all() and (b[1, :3] == -np.inf).all(), (l, p_)
        if l == ref["top"]:
            assert width == ref["ntop"] <= 8 and width == cnt
            break
        assert width % 8 == 0 and width >= cnt
        cnt, span, l = width // 8, span * 8, l + 1


def test_histogram_counts_the_occupied_cells_of_every_level(ref):
    keys = ref["keys"].astype(np.int64)
    occ = 1
    assert ref["level_hist"][0] == 0 and (ref["level_hist"][11:] == 0).all()
    for l in range(1, 11):
        occ += int(ref["level_hist"][l])
        assert occ == len(set((keys >> (3 * (10 - l))).tolist())), l


@pytest.mark.parametrize("glevel", [1, 2, 3, 4, 6, 10])
def test_cell_table_against_per_cell_enumeration(ref, glevel):
    keys = ref["keys"].astype(np.int64)
    ctop, cells, nblocks = R.cell_table(ref["keys"], glevel)
    shift = 3 * (10 - glevel)
    ltop = max(glevel - 3, 0)
    assert len(ctop) == 8 ** ltop and len(cells) == nblocks * 512
    members = {}
    for i, k in enumerate(keys.tolist()):
        members.setdefault(k >> shift, []).append(i)
    tops = sorted({c >> 9 for c in members})
    assert nblocks == len(tops)
    expect = np.full(8 ** ltop, 0xFFFFFFFF, np.uint32)
    for j, s in enumerate(tops):
        expect[s] = j
    assert np.array_equal(ctop, expect)
    seen = np.zeros(len(cells), bool)
    for c, idx in members.items():
        slot = int(ctop[c >> 9]) * 512 + (c & 511)
        assert idx == list(range(idx[0], idx[-1] + 1))
        assert tuple(cells[slot]) == (idx[0], idx[-1] + 1), c
        seen[slot] = True
    assert (cells[~seen] == 0).all()


@pytest.mark.parametrize("leaf_max", [1, 8, 24])
def test_octree_against_per_prefix_enumeration(ref, leaf_max):
    keys, pts, n = ref["keys"].astype(np.int64), ref["tq"][:, :3], ref["n"]
    nodes, off = R.octree(ref["keys"], pts, leaf_max)
    w = nodes.view(np.uint32)
    prefixes = []
    for l in range(11):
        members = {}
        for i, k in enumerate((keys >> (3 * (10 - l))).tolist()):
            members.setdefault(k, []).append(i)
        prefixes.append(sorted(members.items()))
        assert int(off[l + 1]) - int(off[l]) == len(members)
    for l in range(11):
        nxt = {p: j for j, (p, _) in enumerate(prefixes[l + 1])} if l < 10 else {}
        kids_of = {}
        for q in nxt:
            kids_of.setdefault(q >> 3, []).append(q)
        for j, (pre, idx) in enumerate(prefixes[l]):
            g = int(off[l]) + j
            assert w[g, 0, 3] == idx[0]
            assert np.array_equal(nodes[g, 0, :3], pts[idx].min(0)) and np.array_equal(nodes[g, 1, :3], pts[idx].max(0))
            packed = int(w[g, 1, 3])
            if l == 10 or len(idx) <= leaf_max:
                assert packed == len(idx), (l, j)
            else:
                kids = kids_of[pre]
                assert packed >> 28 == len(kids) and packed & R.CF_MASK == nxt[min(kids)], (l, j)
    got = dict(n=n, olevel_off=off, onodes=nodes, tq=ref["tq"])
    leaves = R.walk_octree(got)
    assert 1 <= leaves <= n


def test_grid_rule():
    hist = np.zeros(16, np.uint32)
    hist[1:11] = [3, 12, 48, 190, 700, 1500, 400, 100, 30, 10]      # ~4x per level while cells hold several points: a surface
    n = 3000
    # occupied cells 4, 16, 64, 254, 954: level 5 still holds 3000 / 954 = 3.14 points per cell, level 4 holds 11.8
    assert R.choose_grid(hist, n) == (5, True) and R.choose_grid(hist, n, grid_ppc=3.2) == (4, True)
    assert R.choose_grid(hist, n, grid_maxlevel=3)[0] == 3 and R.choose_grid(hist, n, grid_level=0)[0] == 0
    assert R.choose_grid(hist, n, grid_level=10) == (10, True) and R.choose_grid(hist, n, first_pass=0)[1] is False
    hist[:] = 0
    hist[1:6] = [7, 56, 448, 3000, 9000]           # 8x per level: a volume (level 4: 5.7 points per cell, level 5: 1.6)
    assert R.choose_grid(hist, 20000)[0] == 4
    assert R.choose_grid(hist, 20000)[1] is False and R.choose_grid(hist, 20000, first_pass=1)[1] is True


# ---- hand-worked clouds --------------------------------------------------------------------------------------------------------
def test_one_point():
    r = R.build_reference(np.array([[1, 2, 3]], f32), np.array([[0, 0, 1]], f32))
    assert r["origin"].tolist() == [1, 2, 3] and r["h0"] == f32(f32(1.00001) / f32(1024))
    assert r["keys"].tolist() == [0] and r["tq"].view(np.uint32)[0, 3] == 0 and r["tq"][0, :3].tolist() == [1, 2, 3]
    assert (r["top"], r["ntop"], r["n_boxes"], r["tree_levels"]) == (0, 1, 1, 1)
    assert r["boxes"][0, :, :3].tolist() == [[1, 2, 3], [1, 2, 3]]
    assert not r["level_hist"].any() and (r["grid_level"], r["surface_like"], r["leaf_max"]) == (1, True, 24)
    assert r["ctop"].tolist() == [0] and r["cells"].shape == (512, 2) and r["cells"][0].tolist() == [0, 1] and not r["cells"][1:].any()
    assert r["olevel_off"].tolist() == list(range(12)) and (r["onodes"].view(np.uint32)[:, 1, 3] == 1).all()
    assert R.walk_octree(r) == 1


def test_two_points():
    r = R.build_reference(np.array([[1, 1, 1], [0, 0, 0]], f32), np.zeros((2, 3), f32))
    assert r["keys"].tolist() == [0, 2 ** 30 - 1] and r["order"].tolist() == [1, 0]
    assert r["level_hist"].tolist() == [0, 1] + [0] * 14 and r["grid_level"] == 1 and r["surface_like"]
    assert r["cells"][0].tolist() == [0, 1] and r["cells"][7].tolist() == [1, 2] and r["n_blocks"] == 1
    assert r["olevel_off"].tolist() == [0, 1] + list(range(3, 23, 2)) and r["n_onodes"] == 21
    w = r["onodes"].view(np.uint32)
    assert w[0, 1, 3] == 2 and (w[1:, 1, 3] == 1).all()                # the root is a leaf of two points
    assert r["boxes"][0, :, :3].tolist() == [[0, 0, 0], [1, 1, 1]] and R.walk_octree(r) == 1
    r = R.build_reference(np.array([[1, 1, 1], [0, 0, 0]], f32), np.zeros((2, 3), f32), oct_leaf=1)
    w = r["onodes"].view(np.uint32)
    assert w[0, 1, 3] == (2 << 28) | 0 and (w[1:, 1, 3] == 1).all() and R.walk_octree(r) == 2


def test_nine_points_on_a_line():
    x = np.arange(9, dtype=f32)[::-1]
    p = np.stack([x, np.zeros(9, f32), np.zeros(9, f32)], 1)
    r = R.build_reference(p, np.zeros((9, 3), f32), oct_leaf=2)
    assert r["order"].tolist() == list(range(8, -1, -1))
    assert R.cell_of_key(r["keys"])[:, 0].tolist() == [0, 127, 255, 383, 511, 639, 767, 895, 1023]
    assert r["level_hist"][:6].tolist() == [0, 1, 2, 4, 1, 0] and (r["grid_level"], r["surface_like"]) == (1, True)
    assert (r["top"], r["ntop"], r["n_boxes"]) == (0, 2, 2)
    assert r["boxes"][:, :, 0].tolist() == [[0, 7], [8, 8]]
    assert r["cells"][0].tolist() == [0, 5] and r["cells"][1].tolist() == [5, 9]
    assert r["olevel_off"][:6].tolist() == [0, 1, 3, 7, 15, 24]
    w = r["onodes"].view(np.uint32)
    assert w[0, 1, 3] == (2 << 28) | 0                                   # root: two children
    assert [int(v) for v in w[1:3, 1, 3]] == [(2 << 28) | 0, (2 << 28) | 2]      # 5 and 4 points: split again
    assert [int(v) for v in w[3:7, 1, 3]] == [(2 << 28) | 0, 2, 2, 2]            # 3, 2, 2, 2 points
    assert [int(v) for v in w[7:9, 1, 3]] == [2, 1]                           # (0, 127) and (255)
    assert R.walk_octree(r) == 5


# ---- negative controls ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def good():
    p, nrm = _cloud(3000, 2, dup=40, surface=True)
    r = R.build_reference(p, nrm)
    R.check_index(r, r)
    return r


def _broken(good):
    return copy.deepcopy(good)


def test_control_equal_key_rows_swapped(good):
    g = _broken(good)
    k = good["keys"]
    i = int(np.flatnonzero(k[1:] == k[:-1])[0])
    g["tq"][[i, i + 1]] = g["tq"][[i + 1, i]]
    g["tn"][[i, i + 1]] = g["tn"][[i + 1, i]]
    with pytest.raises(AssertionError, match="not stable"):
        R.check_order(good, g)


def test_control_adjacent_unequal_keys_swapped(good):
    g = _broken(good)
    k = good["keys"]
    i = int(np.flatnonzero(k[1:] != k[:-1])[5])
    g["tq"][[i, i + 1]] = g["tq"][[i + 1, i]]
    g["tn"][[i, i + 1]] = g["tn"][[i + 1, i]]
    with pytest.raises(AssertionError, match="not sorted"):
        R.check_order(good, g)


def test_control_pair_record_differs_from_tq(good):
    g = _broken(good)
    g["tn"][11, 1, 2] = np.nextafter(g["tn"][11, 1, 2], f32(9))
    with pytest.raises(AssertionError, match=r"tn\.xyz"):
        R.check_order(good, g)


@pytest.mark.parametrize("node", ["leaf", "top"])
@pytest.mark.parametrize("side,toward", [(0, np.inf), (0, -np.inf), (1, np.inf), (1, -np.inf)])
def test_control_box_bound_one_ulp_off(good, node, side, toward):
    """inward loses neighbours, outward only costs time: both are defects (the boxes are tight)"""
    g = _broken(good)
    j = 17 if node == "leaf" else int(good["level_off"][good["top"]])
    g["boxes"][j, side, 1] = np.nextafter(g["boxes"][j, side, 1], f32(toward))
    with pytest.raises(AssertionError, match=r"boxes\.xyz\[%d, %d, 1\]" % (j, side)):
        R.check_boxes(good, g)


def test_control_cell_range_end_off_by_one(good):
    g = _broken(good)
    s = int(np.flatnonzero(good["cells"][:, 1] > 0)[3])
    g["cells"][s, 1] -= 1
    with pytest.raises(AssertionError, match=r"cells\[%d, 1\]" % s):
        R.check_cells(good, g)
    g = _broken(good)
    g["cells"][s, 0] += 1
    with pytest.raises(AssertionError, match=r"cells\[%d, 0\]" % s):
        R.check_cells(good, g)


def test_control_ctop_blocks_swapped(good):
    p, nrm = _cloud(5000, 4)
    r = R.build_reference(p, nrm, grid_level=5)
    occ = np.flatnonzero(r["ctop"] != 0xFFFFFFFF)
    assert len(occ) >= 2
    g = _broken(r)
    g["ctop"][[occ[0], occ[1]]] = g["ctop"][[occ[1], occ[0]]]
    with pytest.raises(AssertionError, match=r"ctop\[%d\]" % occ[0]):
        R.check_cells(r, g)


def _leaf_and_inner(good):
    w = good["onodes"].view(np.uint32)
    off = good["olevel_off"].astype(np.int64)
    reach = np.zeros(len(w), bool)                  # nodes the walk reaches
    ids = [0]
    for l in range(11):
        nxt = []
        for i in ids:
            gnode = int(off[l]) + i
            reach[gnode] = True
            p = int(w[gnode, 1, 3])
            nxt += list(range(p & R.CF_MASK, (p & R.CF_MASK) + (p >> 28))) if p >> 28 else []
        ids = nxt
    packed = w[:, 1, 3]
    leaf = int(np.flatnonzero(reach & (packed >> 28 == 0))[4])
    inner = int(np.flatnonzero(reach & (packed >> 28 >= 2) & (packed & R.CF_MASK > 0))[1])
    return leaf, inner


@pytest.mark.parametrize("delta", [1, -1])
def test_control_leaf_count_off_by_one(good, delta):
    leaf, _ = _leaf_and_inner(good)
    g = _broken(good)
    w = g["onodes"].view(np.uint32)
    w[leaf, 1, 3] = int(w[leaf, 1, 3]) + delta
    with pytest.raises(AssertionError, match=r"child_first_or_count\[%d\]" % leaf):
        R.check_octree(good, g)
    with pytest.raises(AssertionError, match="octree walk: leaf node %d covers" % leaf):
        R.walk_octree(g)


@pytest.mark.parametrize("delta", [1, -1])
def test_control_child_first_off_by_one(good, delta):
    _, inner = _leaf_and_inner(good)
    g = _broken(good)
    w = g["onodes"].view(np.uint32)
    w[inner, 1, 3] = int(w[inner, 1, 3]) + delta
    with pytest.raises(AssertionError, match=r"child_first_or_count\[%d\]" % inner):
        R.check_octree(good, g)
    with pytest.raises(AssertionError, match="octree"):
        R.walk_octree(g)


def test_control_nchild_short_by_one(good):
    _, inner = _leaf_and_inner(good)
    g = _broken(good)
    g["onodes"].view(np.uint32)[inner, 1, 3] -= np.uint32(1 << 28)
    with pytest.raises(AssertionError, match=r"nchild\[%d\]" % inner):
        R.check_octree(good, g)
    with pytest.raises(AssertionError, match=r"octree walk: .*\(gap\)|the leaves end at"):
        R.walk_octree(g)


def test_control_octree_box_and_first_point(good):
    leaf, inner = _leaf_and_inner(good)
    g = _broken(good)
    g["onodes"][inner, 1, 0] = np.nextafter(g["onodes"][inner, 1, 0], f32(-np.inf))      # a parent's box one ulp short
    with pytest.raises(AssertionError, match=r"onodes\.xyz\[%d, 1, 0\]" % inner):
        R.check_octree(good, g)
    with pytest.raises(AssertionError, match="sticks out of its parent"):
        R.walk_octree(g)
    g = _broken(good)
    g["onodes"].view(np.uint32)[leaf, 0, 3] += 1
    with pytest.raises(AssertionError, match=r"onodes\.first\[%d\]" % leaf):
        R.check_octree(good, g)


def test_control_histogram_count_moved_to_the_next_level(good):
    g = _broken(good)
    l = int(np.flatnonzero(good["level_hist"])[-1])
    g["level_hist"][l] -= 1
    g["level_hist"][l - 1] += 1
    with pytest.raises(AssertionError, match=r"level_hist\[%d\]" % (l - 1)):
        R.check_info(good, g)


@pytest.mark.parametrize("field,value", [("grid_level", None), ("leaf_max", 16), ("surface_like", None), ("h0", None), ("n_blocks", None)])
def test_control_info_fields(good, field, value):
    g = _broken(good)
    if field == "surface_like":
        g[field] = not good[field]
    elif field == "h0":
        g[field] = np.nextafter(good[field], f32(9))
    else:
        g[field] = value if value is not None else good[field] + 1
    with pytest.raises(AssertionError, match=field):
        R.check_info(good, g)


def _table(n_loc=1000):
    """a legal table: blocks of 64 cut in two at lane 20, in descending key order"""
    tab = []
    for b in range((n_loc + 63) // 64):
        m = min(64, n_loc - 64 * b)
        tab += [(64 * b, min(20, m))] + ([(64 * b + 20, m - 20)] if m > 20 else [])
    tab = np.array(tab, np.int64)
    keys = np.arange(len(tab))[::-1].copy()
    return tab, keys


def test_control_packets():
    tab, keys = _table()
    R.check_packets(1000, tab, keys)
    R.check_packets(1000, tab[::-1], None)                                  # any permutation of the runs is a table
    with pytest.raises(AssertionError, match="a packet is missing"):
        R.check_packets(1000, np.delete(tab, 5, 0), np.delete(keys, 5))
    with pytest.raises(AssertionError, match="in more than one packet"):
        R.check_packets(1000, np.insert(tab, 9, tab[5], 0), np.insert(keys, 9, keys[9]))
    k2 = keys.copy()
    k2[[3, 4]] = k2[[4, 3]]
    with pytest.raises(AssertionError, match="entry 4 .* starts behind entry 3"):
        R.check_packets(1000, tab, k2)
    t2 = tab.copy()
    t2[0] = (0, 70); t2 = np.delete(t2, [1, 2], 0)
    with pytest.raises(AssertionError, match="count 70"):
        R.check_packets(1000, t2)
    t2 = tab.copy()
    t2[1] = (20, 50); t2[2] = (70, 14)
    with pytest.raises(AssertionError, match="cross a block"):
        R.check_packets(1000, t2)
    t2 = np.array([(i, 1) for i in range(9)] + [(9, 55)] + [(64, 36)], np.int64)
    with pytest.raises(AssertionError, match="cut into 10 runs"):
        R.check_packets(100, t2)
    with pytest.raises(AssertionError, match="queries 960 .. 999 are in no packet"):
        R.check_packets(1000, tab[:-2])


def test_start_keys_of_hand_built_runs():
    """radius keys: the top bits of the squared radius about the centroid, whatever lanes the run sits on"""
    pts = np.zeros((128, 3), f32)
    pts[:, 0] = np.arange(128)
    tab = np.array([(0, 64), (64, 3), (67, 61)])
    k = R.radius_keys(pts, tab, 32)
    assert k.view(f32).tolist() == [31.5 ** 2, 1.0, 30.0 ** 2]
    assert R.radius_keys(pts, tab, 16).tolist() == (k >> 16).tolist()
    assert R.share_order(pts[::-1]).tolist() == list(range(127, -1, -1)) and R.share_order(pts[::-1], 64, 64).tolist() == list(range(127, 63, -1))
    assert [R.shard_range(130, 5, r) for r in range(5)] == [(0, 26), (26, 26), (52, 26), (78, 26), (104, 26)]
    assert [R.shard_range(7, 2, r) for r in range(2)] == [(0, 3), (3, 4)]
