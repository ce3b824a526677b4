"""The search index restated in numpy (kernels_build.hip, build_index / build_octree in engine_index.cpp, the packet table of set_source).

Plain numpy, fp32 where the device uses fp32 (the build is compiled with contraction off, so every float below is the device's
bit for bit), integers everywhere else: nothing here has a tolerance.  `build_reference(xyz, nrm)` returns a dict with the keys of
`Engine.index_arrays()`; every structure has one checker `check_*(ref, got)` that raises an AssertionError naming the first offending
element.  Floats are compared by value (fminf(-0, +0) may return either zero), integer words by their bits.

The invariants ("index invariants and how they are tested"):
  order     tq is the cloud in ascending Morton key, equal keys in ascending original row (the sort is stable); tn its pair records
  boxes     leaf l = exact min / max of sorted points 8l .. 8l+7, padding (+inf, -inf), a parent = min / max of its 8 children
  info      origin, h0, the level histogram, the grid level and the surface-like flag chosen from it, leaf_max, every offset
  cells     ctop[s] = rank of occupied super-cell s (~0: empty), cells[block * 512 + (c & 511)] = (first, last + 1), (0, 0) when empty
  octree    per level one node per occupied key prefix in ascending order; leaf iff level 10 or npts <= leaf_max; exact boxes
  walk      from the root, child_first / nchild reach leaves that tile [0, n) exactly once, every child box inside its parent's
  packets   runs tile [0, n_loc) once, stay inside a 64-query block, 1 <= count <= 64, <= 8 per block, start keys non-increasing
"""
import numpy as np

f32 = np.float32
MORTON_BITS = 10
LEAF = 8
FAN = 8
MAX_TREE_LEVELS = 12
CF_MASK = 0x0FFFFFFF
EMPTY = 0xFFFFFFFF
MAX_RUNS_PER_BLOCK = 8


# ---------------------------------------------------------------------------------------------------------------------------------
# keys and order
# ---------------------------------------------------------------------------------------------------------------------------------
def spread3(v):
    """k_morton's spread3_b: bit i of the 10-bit v to bit 3i"""
    v = v.astype(np.uint32) & np.uint32(0x3FF)
    v = (v | (v << np.uint32(16))) & np.uint32(0x030000FF)
    v = (v | (v << np.uint32(8))) & np.uint32(0x0300F00F)
    v = (v | (v << np.uint32(4))) & np.uint32(0x030C30C3)
    v = (v | (v << np.uint32(2))) & np.uint32(0x09249249)
    return v


def frame(xyz):
    """-> (origin [3] f32, h0 f32): per-axis minimum and the finest cell edge fl32(fl32(emax * 1.00001f) / 1024)"""
    xyz = np.asarray(xyz, f32)
    lo, hi = xyz.min(0), xyz.max(0)
    emax = f32(0)
    for k in range(3):
        emax = max(emax, f32(hi[k] - lo[k]))
    if not emax > 0:
        emax = f32(1)
    h0 = f32(f32(emax * f32(1.00001)) / f32(1 << MORTON_BITS))
    return lo.astype(f32), h0


def morton_keys(xyz, origin, h0):
    """c = clip(floor(fl32(fl32(x - o) * fl32(1 / h0))), 0, 1023) per axis, interleaved z y x from the top"""
    xyz = np.asarray(xyz, f32)
    inv = f32(f32(1) / f32(h0))
    c = np.floor((xyz - origin.astype(f32)[None, :]).astype(f32) * inv)
    c = np.clip(c, 0, (1 << MORTON_BITS) - 1).astype(np.int64)
    return (spread3(c[:, 2]) << np.uint32(2)) | (spread3(c[:, 1]) << np.uint32(1)) | spread3(c[:, 0])


def cell_of_key(keys):
    """inverse of the interleave: keys -> integer cell coordinates [n, 3] (x, y, z) at level 10"""
    keys = np.asarray(keys, np.uint32)
    out = np.zeros((len(keys), 3), np.int64)
    for b in range(MORTON_BITS):
        for a in range(3):
            out[:, a] |= ((keys >> np.uint32(3 * b + a)) & np.uint32(1)).astype(np.int64) << b
    return out


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the structures
# ---------------------------------------------------------------------------------------------------------------------------------
def tree_layout(n):
    """the host recurrence of build_index -> (cnt, pad, level_off, top, ntop, total)"""
    cnt, pad, off = [], [], []
    m = (n + LEAF - 1) // LEAF
    total = 0
    while True:
        cnt.append(m)
        pad.append(m if m <= FAN else ((m + FAN - 1) // FAN) * FAN)
        off.append(total)
        total += pad[-1]
        if m <= FAN:
            break
        m = pad[-1] // FAN
        assert len(cnt) < MAX_TREE_LEVELS
    return cnt, pad, off, len(cnt) - 1, cnt[-1], total


def box_tree(pts, n):
    cnt, pad, off, top, ntop, total = tree_layout(n)
    boxes = np.zeros((total, 2, 4), f32)
    lo = np.full((pad[0] * LEAF, 3), np.inf, f32)
    hi = np.full((pad[0] * LEAF, 3), -np.inf, f32)
    lo[:n] = pts
    hi[:n] = pts
    lo = lo.reshape(pad[0], LEAF, 3).min(1)
    hi = hi.reshape(pad[0], LEAF, 3).max(1)
    boxes[off[0]:off[0] + pad[0], 0, :3] = lo
    boxes[off[0]:off[0] + pad[0], 1, :3] = hi
    for l in range(1, len(cnt)):
        plo = np.full((pad[l] * FAN, 3), np.inf, f32)
        phi = np.full((pad[l] * FAN, 3), -np.inf, f32)
        plo[:pad[l - 1]] = lo
        phi[:pad[l - 1]] = hi
        lo = plo.reshape(pad[l], FAN, 3).min(1)
        hi = phi.reshape(pad[l], FAN, 3).max(1)
        boxes[off[l]:off[l] + pad[l], 0, :3] = lo
        boxes[off[l]:off[l] + pad[l], 1, :3] = hi
    level_off = np.zeros(MAX_TREE_LEVELS, np.uint32)
    level_off[:len(off)] = off
    return boxes, level_off, top, ntop, total


def level_histogram(keys):
    """hist[l], l = 1 .. 10: adjacent sorted pairs whose keys first differ at octree level l"""
    x = (keys[1:] ^ keys[:-1]).astype(np.uint32)
    x = x[x != 0]
    _, e = np.frexp(x.astype(np.float64))          # x = m * 2^e, 0.5 <= m < 1: highest set bit = e - 1 (exact below 2^53)
    lvl = MORTON_BITS - (e - 1) // 3
    return np.bincount(lvl, minlength=16).astype(np.uint32)


def choose_grid(hist, n, grid_ppc=3.0, grid_maxlevel=MORTON_BITS, grid_level=-1, first_pass=-1):
    """build_index's rule -> (grid level, surface-like)"""
    lcap = min(int(grid_maxlevel), MORTON_BITS)
    glevel, occ = 1, 1.0
    for l in range(1, lcap + 1):
        occ += float(hist[l])
        if float(n) / occ >= float(grid_ppc):
            glevel = l
    if grid_level >= 0:
        glevel = grid_level
    glevel = max(min(glevel, lcap), 0)
    occ_l = [1.0]
    for l in range(1, MORTON_BITS + 1):
        occ_l.append(occ_l[-1] + float(hist[l]))
    lg = glevel - 1 if glevel >= 2 else 1
    surface = occ_l[lg] / occ_l[lg - 1] < 5.5
    if first_pass >= 0:
        surface = first_pass == 1
    return glevel, bool(surface)


def cell_table(keys, glevel):
    """-> (ctop [8^ltop], cells [nblocks * 512, 2], nblocks)"""
    n = len(keys)
    shift = 3 * (MORTON_BITS - glevel)
    ltop = glevel - 3 if glevel > 3 else 0
    c = (keys.astype(np.uint64) >> np.uint64(shift)).astype(np.int64)
    uc = np.unique(c)
    utop = np.unique(uc >> 9)
    ctop = np.full(1 << (3 * ltop), EMPTY, np.uint32)
    ctop[utop] = np.arange(len(utop), dtype=np.uint32)
    cells = np.zeros((len(utop) * 512, 2), np.uint32)
    slot = ctop[uc >> 9].astype(np.int64) * 512 + (uc & 511)
    cells[slot, 0] = np.searchsorted(c, uc, "left")
    cells[slot, 1] = np.searchsorted(c, uc, "right")
    assert n == 0 or cells[:, 1].max() == n
    return ctop, cells, len(utop)


def octree(keys, pts, leaf_max):
    """-> (onodes [total, 2, 4] f32 with the integer words in their bits, olevel_off [12])"""
    n = len(keys)
    k64 = keys.astype(np.uint64)
    starts = []
    for l in range(MORTON_BITS + 1):
        p = k64 >> np.uint64(3 * (MORTON_BITS - l))
        starts.append(np.concatenate([[0], 1 + np.flatnonzero(p[1:] != p[:-1])]).astype(np.int64))
    off = np.zeros(MORTON_BITS + 2, np.uint32)
    off[1:] = np.cumsum([len(s) for s in starts])
    nodes = np.zeros((int(off[-1]), 2, 4), f32)
    w = nodes.view(np.uint32)
    for l in range(MORTON_BITS + 1):
        s = starts[l]
        ends = np.append(s[1:], n)
        npts = ends - s
        a, b = int(off[l]), int(off[l + 1])
        nodes[a:b, 0, :3] = np.minimum.reduceat(pts, s, axis=0)
        nodes[a:b, 1, :3] = np.maximum.reduceat(pts, s, axis=0)
        w[a:b, 0, 3] = s
        leaf = (npts <= leaf_max) if l < MORTON_BITS else np.ones(len(s), bool)
        packed = (npts & CF_MASK).astype(np.uint32)
        if l < MORTON_BITS:
            c0 = np.searchsorted(starts[l + 1], s, "left")
            c1 = np.searchsorted(starts[l + 1], ends, "left")
            inner = ((c0 & CF_MASK) | ((c1 - c0) << 28)).astype(np.uint32)
            packed = np.where(leaf, packed, inner)
        w[a:b, 1, 3] = packed
    return nodes, off


def build_reference(xyz, nrm, grid_ppc=3.0, grid_maxlevel=MORTON_BITS, grid_level=-1, first_pass=-1, oct_leaf=0):
    """the whole target index -> dict with the keys of Engine.index_arrays() (+ keys, order: what the device does not keep)"""
    xyz, nrm = np.ascontiguousarray(xyz, f32), np.ascontiguousarray(nrm, f32)
    n = len(xyz)
    origin, h0 = frame(xyz)
    keys0 = morton_keys(xyz, origin, h0)
    order = np.argsort(keys0, kind="stable")
    keys = keys0[order]
    tq = np.zeros((n, 4), f32)
    tq[:, :3] = xyz[order]
    tq.view(np.uint32)[:, 3] = order.astype(np.uint32)
    tn = np.zeros((n, 2, 4), f32)
    tn[:, 0] = tq
    tn[:, 1, :3] = nrm[order]
    boxes, level_off, top, ntop, n_boxes = box_tree(tq[:, :3], n)
    hist = level_histogram(keys)
    glevel, surface = choose_grid(hist, n, grid_ppc, grid_maxlevel, grid_level, first_pass)
    leaf_max = int(oct_leaf) if oct_leaf > 0 else (24 if surface else 8)
    r = dict(n=n, origin=origin, h0=h0, keys=keys, order=order, tq=tq, tn=tn, boxes=boxes, level_off=level_off, top=top, ntop=ntop,
             n_boxes=n_boxes, tree_levels=top + 1, level_hist=hist, grid_level=glevel, surface_like=surface, leaf_max=leaf_max)
    if glevel > 0:
        sc = f32(1 << (MORTON_BITS - glevel))
        r["gdim"] = 1 << glevel
        r["h"] = f32(h0 * sc)
        r["inv_h"] = f32(f32(f32(1) / h0) / sc)
        r["ctop"], r["cells"], r["n_blocks"] = cell_table(keys, glevel)
        r["ctop_len"] = len(r["ctop"])
    else:
        r.update(gdim=0, h=f32(0), inv_h=f32(0), ctop=np.zeros(0, np.uint32), cells=np.zeros((0, 2), np.uint32), n_blocks=0, ctop_len=0)
    r["onodes"], r["olevel_off"] = octree(keys, tq[:, :3], leaf_max)
    r["n_onodes"] = int(r["olevel_off"][-1])
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# checkers
# ---------------------------------------------------------------------------------------------------------------------------------
def _same(name, ref, got, as_bits=False):
    """ref == got elementwise (floats by value, or every word by its bits), naming the first element that differs"""
    ref, got = np.asarray(ref), np.asarray(got)
    assert ref.shape == got.shape, "%s: shape %s, expected %s" % (name, got.shape, ref.shape)
    if as_bits:
        ref, got = np.ascontiguousarray(ref).view(np.uint32), np.ascontiguousarray(got).view(np.uint32)
    bad = np.flatnonzero((ref != got).reshape(-1))
    if len(bad):
        i = np.unravel_index(bad[0], ref.shape)
        raise AssertionError("%s%s = %r, expected %r (%d elements differ)" % (name, list(map(int, i)), got[i], ref[i], len(bad)))


def _same_nodes(name, ref, got):
    """[m, 2, 4] node arrays: xyz by value, the w words by their bits"""
    assert ref.shape == got.shape, "%s: shape %s, expected %s" % (name, got.shape, ref.shape)
    _same(name + ".w", ref[..., 3], got[..., 3], as_bits=True)
    _same(name + ".xyz", ref[..., :3], got[..., :3])


def check_order(ref, got):
    """tq / tn: the stable Morton order.  Independently of ref: the keys recomputed from got's tq ascend, rows ascend inside equal keys"""
    assert got["n"] == ref["n"], "n = %d, expected %d" % (got["n"], ref["n"])
    keys = morton_keys(got["tq"][:, :3], ref["origin"], ref["h0"])
    rows = bits(got["tq"][:, 3]).astype(np.int64)
    k = keys.astype(np.int64)
    bad = np.flatnonzero(k[1:] < k[:-1])
    assert not len(bad), "tq: key of position %d (%d) is below its predecessor's (%d): not sorted" % (bad[0] + 1, k[bad[0] + 1], k[bad[0]])
    bad = np.flatnonzero((k[1:] == k[:-1]) & (rows[1:] <= rows[:-1]))
    assert not len(bad), "tq: rows %d, %d of equal keys at positions %d, %d do not ascend: not stable" % (rows[bad[0]], rows[bad[0] + 1], bad[0], bad[0] + 1)
    _same_nodes("tq", ref["tq"][:, None, :], got["tq"][:, None, :])
    _same("tn.point.w", ref["tn"][:, 0, 3], got["tn"][:, 0, 3], as_bits=True)
    _same("tn.normal.w", ref["tn"][:, 1, 3], got["tn"][:, 1, 3], as_bits=True)
    _same("tn.xyz", ref["tn"][:, :, :3], got["tn"][:, :, :3])


def check_boxes(ref, got):
    """the implicit 8-ary tree: offsets and every box, tight (a bound one ulp off in either direction is an error)"""
    for k in ("top", "ntop", "n_boxes", "tree_levels"):
        assert int(got[k]) == int(ref[k]), "%s = %d, expected %d" % (k, got[k], ref[k])
    _same("level_off", ref["level_off"], got["level_off"])
    _same_nodes("boxes", ref["boxes"], got["boxes"])


def check_info(ref, got):
    """the frame, the histogram and what was decided from it"""
    _same("origin", ref["origin"], got["origin"])
    for k in ("h0", "h", "inv_h"):
        assert f32(got[k]) == f32(ref[k]), "%s = %r, expected %r" % (k, got[k], ref[k])
    _same("level_hist", ref["level_hist"], got["level_hist"])
    for k in ("n", "grid_level", "gdim", "leaf_max", "n_blocks", "ctop_len", "n_onodes"):
        assert int(got[k]) == int(ref[k]), "%s = %d, expected %d" % (k, got[k], ref[k])
    assert bool(got["surface_like"]) == bool(ref["surface_like"]), "surface_like = %r, expected %r" % (got["surface_like"], ref["surface_like"])
    _same("olevel_off", ref["olevel_off"], got["olevel_off"])


def check_cells(ref, got):
    """the two-level cell table, whole arrays"""
    _same("ctop", ref["ctop"], got["ctop"])
    _same("cells", ref["cells"], got["cells"])


def check_octree(ref, got):
    """every node of every level: first point, leaf count or (child_first, nchild), exact box"""
    _same("olevel_off", ref["olevel_off"], got["olevel_off"])
    r, g = ref["onodes"], got["onodes"]
    assert r.shape == g.shape, "onodes: shape %s, expected %s" % (g.shape, r.shape)
    rw, gw = r.view(np.uint32), np.ascontiguousarray(g).view(np.uint32)
    _same("onodes.first", rw[:, 0, 3], gw[:, 0, 3])
    _same("onodes.nchild", rw[:, 1, 3] >> 28, gw[:, 1, 3] >> 28)
    _same("onodes.child_first_or_count", rw[:, 1, 3] & CF_MASK, gw[:, 1, 3] & CF_MASK)
    _same("onodes.xyz", r[..., :3], g[..., :3])


def walk_octree(got):
    """What the search relies on, from got alone: from the root, child_first / nchild reach leaves that tile [0, n) exactly once, every
    child's box lies inside its parent's, and every leaf's points lie inside the leaf's box.  -> number of leaves reached"""
    n, off = int(got["n"]), got["olevel_off"].astype(np.int64)
    nodes = got["onodes"]
    w = np.ascontiguousarray(nodes).view(np.uint32)
    pts = got["tq"][:, :3]
    ids = np.zeros(1, np.int64)                  # node numbers within the level
    leaf_first, leaf_cnt, leaf_node = [], [], []
    assert off[1] - off[0] == 1, "octree: %d roots" % (off[1] - off[0])
    for l in range(MORTON_BITS + 1):
        if not len(ids):
            break
        g = off[l] + ids
        packed = w[g, 1, 3].astype(np.int64)
        nch, cf = packed >> 28, packed & CF_MASK
        leaf = nch == 0
        leaf_first.append(w[g[leaf], 0, 3].astype(np.int64)); leaf_cnt.append(cf[leaf]); leaf_node.append(g[leaf])
        par = g[~leaf]
        nch, cf = nch[~leaf], cf[~leaf]
        if not len(par):
            ids = np.zeros(0, np.int64)
            continue
        assert l < MORTON_BITS, "octree: node %d of level %d has children" % (ids[~leaf][0], l)
        width = off[l + 2] - off[l + 1]
        bad = np.flatnonzero((nch > 8) | (cf + nch > width))
        assert not len(bad), "octree: children %d .. %d of node %d, level %d: level %d has %d nodes" % (
            cf[bad[0]], cf[bad[0]] + nch[bad[0]] - 1, par[bad[0]] - off[l], l, l + 1, width)
        rep = np.repeat(np.arange(len(par)), nch)
        child = np.repeat(cf, nch) + (np.arange(len(rep)) - np.repeat(np.cumsum(nch) - nch, nch))
        cg, pg = off[l + 1] + child, par[rep]
        out = (nodes[cg, 0, :3] < nodes[pg, 0, :3]).any(1) | (nodes[cg, 1, :3] > nodes[pg, 1, :3]).any(1)
        bad = np.flatnonzero(out)
        assert not len(bad), "octree: box of node %d, level %d sticks out of its parent %d" % (child[bad[0]], l + 1, pg[bad[0]] - off[l])
        ids = child
    first, cnt, node = np.concatenate(leaf_first), np.concatenate(leaf_cnt), np.concatenate(leaf_node)
    o = np.argsort(first, kind="stable")
    first, cnt, node = first[o], cnt[o], node[o]
    assert len(first) and first[0] == 0, "octree walk: no leaf starts at point 0"
    assert (cnt > 0).all(), "octree walk: leaf node %d is empty" % node[np.flatnonzero(cnt <= 0)[0]]
    end = first + cnt
    bad = np.flatnonzero(end[:-1] != first[1:])
    assert not len(bad), "octree walk: leaf node %d covers points %d .. %d, the next leaf starts at %d (%s)" % (
        node[bad[0]], first[bad[0]], end[bad[0]] - 1, first[bad[0] + 1], "gap" if end[bad[0]] < first[bad[0] + 1] else "overlap")
    assert end[-1] == n, "octree walk: the leaves end at point %d of %d" % (end[-1], n)
    owner = np.repeat(node, cnt)
    out = (pts < nodes[owner, 0, :3]).any(1) | (pts > nodes[owner, 1, :3]).any(1)
    bad = np.flatnonzero(out)
    assert not len(bad), "octree walk: point %d lies outside the box of its leaf (node %d)" % (bad[0], owner[bad[0]])
    return len(first)


def check_index(ref, got):
    """everything at once, in the order a defect would propagate"""
    check_info(ref, got)
    check_order(ref, got)
    check_boxes(ref, got)
    check_cells(ref, got)
    check_octree(ref, got)
    return walk_octree(got)


# ---------------------------------------------------------------------------------------------------------------------------------
# source share and packets
# ---------------------------------------------------------------------------------------------------------------------------------
def share_order(xyz, b0=0, bc=None):
    """the sorted order of a rank's share (rows b0 .. b0 + bc of the caller's cloud, keyed in the share's own frame) as caller rows"""
    xyz = np.asarray(xyz, f32)
    bc = len(xyz) - b0 if bc is None else bc
    part = xyz[b0:b0 + bc]
    origin, h0 = frame(part)
    return (np.argsort(morton_keys(part, origin, h0), kind="stable") + b0).astype(np.uint32)


def shard_range(n, nranks, rank):
    """symmicp_shard_range restated -> (first row, count)"""
    b0, b1 = n * rank // nranks, n * (rank + 1) // nranks
    return b0, b1 - b0


def _butterfly(v):
    """the wave's xor-butterfly sum (offsets 32, 16, .., 1) of v [m, 64] in fp32: every lane ends with the same value"""
    lanes = np.arange(64)
    v = v.astype(f32)
    for off in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ off]).astype(f32)
    return v[:, 0]


def _dist2(a, b):
    d = (a - b).astype(f32)
    return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def _run_lanes(pts, tab, in_place):
    """the runs' points on a wave's lanes [m, 64, 3] + mask: at lanes first % 64 .. (k_packet_runs) or 0 .. (k_packet_cost)"""
    tab = np.asarray(tab, np.int64)
    m = len(tab)
    lane = np.arange(64)[None, :]
    l0 = (tab[:, 0] % 64)[:, None] if in_place else np.zeros((m, 1), np.int64)
    mask = (lane >= l0) & (lane < l0 + tab[:, 1][:, None])
    idx = np.clip(tab[:, 0][:, None] + lane - l0, 0, len(pts) - 1)
    p = np.where(mask[..., None], pts[idx], f32(0)).astype(f32)
    return p, mask


def _centroid_radius(p, mask):
    ac = _butterfly(mask.astype(f32))
    c = np.stack([(_butterfly(p[..., k]) / ac).astype(f32) for k in range(3)], 1)
    r2 = np.where(mask, _dist2(p, c[:, None, :]), f32(0)).max(1).astype(f32)
    return c, r2


def radius_keys(pts, tab, key_bits=16):
    """start keys of k_packet_runs: the top key_bits bits of the squared radius of every run about its centroid (larger starts first)"""
    p, mask = _run_lanes(np.asarray(pts, f32), tab, True)
    _, r2 = _centroid_radius(p, mask)
    return bits(r2) >> np.uint32(32 - key_bits)


def _boxdist2(c, lo, hi):
    d = np.maximum(np.maximum((lo - c).astype(f32), (c - hi).astype(f32)), f32(0)).astype(f32)
    return ((d[..., 0] * d[..., 0]).astype(f32) + (d[..., 1] * d[..., 1]).astype(f32)).astype(f32) + (d[..., 2] * d[..., 2]).astype(f32)


def cost_keys(pts, tab, index, key_bits=16):
    """start keys of k_packet_cost: centroid and radius r of the run, greedy descent of the target's octree to the leaf nearest to the
    centroid, d = distance to that leaf's nearest point (of its first 64), cost = 2 d r + r^2 in fp32 -> its top key_bits bits"""
    p, mask = _run_lanes(np.asarray(pts, f32), tab, False)
    c, r2 = _centroid_radius(p, mask)
    nodes, off = index["onodes"], index["olevel_off"].astype(np.int64)
    w = np.ascontiguousarray(nodes).view(np.uint32)
    m = len(c)
    node = np.zeros(m, np.int64)                 # global node number
    level = np.zeros(m, np.int64)
    while True:
        packed = w[node, 1, 3].astype(np.int64)
        nch, cf = packed >> 28, packed & CF_MASK
        act = np.flatnonzero(nch != 0)
        if not len(act):
            break
        best = np.full(len(act), EMPTY, np.int64)
        for j in range(8):
            ok = j < nch[act]
            ch = np.where(ok, off[level[act] + 1] + cf[act] + j, 0)
            key = (bits(_boxdist2(c[act], nodes[ch, 0, :3], nodes[ch, 1, :3])).astype(np.int64) & ~7) | j
            best = np.where(ok & (key < best), key, best)
        node[act] = off[level[act] + 1] + cf[act] + (best & 7)
        level[act] += 1
    first = w[node, 0, 3].astype(np.int64)
    cnt = np.minimum(w[node, 1, 3].astype(np.int64) & CF_MASK, 64)
    tq = index["tq"][:, :3]
    d2 = np.full(m, np.inf, f32)
    for j in range(int(cnt.max())):
        ok = j < cnt
        q = tq[np.where(ok, first + j, 0)]
        d2 = np.where(ok, np.minimum(d2, _dist2(c, q)), d2).astype(f32)
    cost = ((f32(2) * np.sqrt(d2)).astype(f32) * np.sqrt(r2)).astype(f32) + r2
    cost = np.where(np.isfinite(cost) & (cost < f32(3.0e38)), cost, r2).astype(f32)
    return bits(cost) >> np.uint32(32 - key_bits)


def check_packets(n_loc, tab, start_keys=None):
    """the packet table's invariants (start_keys: one per table entry, larger = started earlier; None: the order is not checked)"""
    tab = np.asarray(tab, np.int64).reshape(-1, 2)
    first, cnt = tab[:, 0], tab[:, 1]
    bad = np.flatnonzero((cnt < 1) | (cnt > 64))
    assert not len(bad), "packet %d: count %d" % (bad[0], cnt[bad[0]])
    bad = np.flatnonzero((first < 0) | (first + cnt > n_loc))
    assert not len(bad), "packet %d: queries %d .. %d of %d" % (bad[0], first[bad[0]], first[bad[0]] + cnt[bad[0]] - 1, n_loc)
    bad = np.flatnonzero(first // 64 != (first + cnt - 1) // 64)
    assert not len(bad), "packet %d: queries %d .. %d cross a block of 64" % (bad[0], first[bad[0]], first[bad[0]] + cnt[bad[0]] - 1)
    o = np.argsort(first, kind="stable")
    f, e = first[o], first[o] + cnt[o]
    assert len(f) and f[0] == 0, "packets: query 0 is in no packet"
    bad = np.flatnonzero(e[:-1] != f[1:])
    if len(bad):
        i = bad[0]
        what = "are in no packet (a packet is missing)" if e[i] < f[i + 1] else "are in more than one packet"
        raise AssertionError("packets: queries %d .. %d %s (table entries %d, %d)" % (min(e[i], f[i + 1]), max(e[i], f[i + 1]) - 1, what, o[i], o[i + 1]))
    assert e[-1] == n_loc, "packets: queries %d .. %d are in no packet" % (e[-1], n_loc - 1)
    per = np.bincount(first // 64)
    bad = np.flatnonzero(per > MAX_RUNS_PER_BLOCK)
    assert not len(bad), "packets: block %d is cut into %d runs" % (bad[0], per[bad[0]])
    if start_keys is not None:
        k = np.asarray(start_keys, np.int64)
        assert len(k) == len(tab), "packets: %d start keys for %d entries" % (len(k), len(tab))
        bad = np.flatnonzero(k[1:] > k[:-1])
        assert not len(bad), "packets: entry %d (key %d) starts behind entry %d (key %d)" % (bad[0] + 1, k[bad[0] + 1], bad[0], k[bad[0]])
