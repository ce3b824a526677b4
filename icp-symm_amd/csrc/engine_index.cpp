// engine_index.cpp -- the search index of libsymmicp on the host side: the store an index's device memory comes from, the upload of a cloud
// into planar arrays, the Morton sort, build_index (cell table, box tree, octree) and its two borrowers: the scratch index of a cloud
// operation, behind the target's arrays, and the reverse index with a store of its own.  The kernels are in kernels_build.hip.
#include "engine_internal.h"

// ---- IndexStore ---------------------------------------------------------------------------------
hipError_t IndexStore::alloc(void **out, size_t bytes)
{
    bytes = (bytes + 255) & ~(size_t)255;
    if (!bytes) bytes = 256;
    if (blk.base && blk.off + bytes <= blk.cap) { *out = blk.base + blk.off; blk.off += bytes; return hipSuccess; }
    void *p = nullptr;
    const hipError_t e = hipMalloc(&p, bytes);
    if (e == hipSuccess) { extra.push_back(p); *out = p; }
    return e;
}

void IndexStore::reserve(size_t want, size_t slack)
{
    if (blk.cap >= want) return;
    hipFree(blk.base);
    blk = Arena{};
    if (hipMalloc((void **)&blk.base, want + slack) == hipSuccess) blk.cap = want + slack;
    else (void)hipGetLastError();      // every alloc then falls back to its own hipMalloc
}

void IndexStore::rewind(Mark m)
{
    while (extra.size() > m.extras) { hipFree(extra.back()); extra.pop_back(); }
    blk.off = m.off;
}

void IndexStore::release()
{
    reset();
    if (blk.base) hipFree(blk.base);
    blk = Arena{};
}

// host strided cloud -> device block of 6 planar arrays.  The usual layouts never touch a host staging loop: records with
// contiguous x y z (packed AoS, PointXYZ, PointNormal) are copied as they are and split into columns on the device;
// column-major matrices (Eigen) are copied column by column.  Anything else goes through a host transpose.  nrm == NULL: the normal
// columns are zero-filled (a PLANE source: no kernel is ever handed an unallocated normal array).
int upload_planar(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n, DevBuf<float> &block,
                  IndexStore *store, double centroid[3])
{
    if (centroid) {
        // fp64, in row order (the oracle's order: the pivot has to come out bit-identical)
        double s[3] = {0, 0, 0};
        for (size_t i = 0; i < n; i++)
            for (int k = 0; k < 3; k++) s[k] += (double)xyz[i * xr + k * xc];
        for (int k = 0; k < 3; k++) centroid[k] = s[k] / (double)n;
    }
    if (!store) HIP_TRY(c, block.alloc_temp(c->arena, 6 * n));
    else { HIP_TRY(c, store->alloc((void **)&block.p, sizeof(float) * 6 * n)); block.owned = false; }
    float *col[6];
    for (int k = 0; k < 6; k++) col[k] = block.p + (size_t)k * n;
    struct Part { const float *base; size_t rs, cs; int first_col; } parts[2] = {{xyz, xr, xc, 0}, {nrm, nr, nc, 3}};
    if (!nrm) HIP_TRY(c, hipMemsetAsync(col[3], 0, sizeof(float) * 3 * n, c->stream));
    for (const Part &p : parts) {
        if (!p.base) continue;
        if (p.cs == 1 && p.rs >= 3) {
            const size_t fl = (n - 1) * p.rs + 3;                  // floats from the first x to the last z
            DevBuf<float> raw;
            HIP_TRY(c, raw.alloc_temp(c->arena, fl));
            HIP_TRY(c, hipMemcpyAsync(raw.p, p.base, sizeof(float) * fl, hipMemcpyHostToDevice, c->stream));
            launch_deinterleave3(raw.p, p.rs, 0, (uint32_t)n, col[p.first_col], col[p.first_col + 1], col[p.first_col + 2], c->stream);
            HIP_TRY(c, hipStreamSynchronize(c->stream));           // raw is freed on scope exit
        } else if (p.rs == 1 && p.cs >= n) {
            for (int k = 0; k < 3; k++)
                HIP_TRY(c, hipMemcpyAsync(col[p.first_col + k], p.base + (size_t)k * p.cs, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        } else {
            std::vector<float> stage(3 * n);
            for (size_t i = 0; i < n; i++)
                for (int k = 0; k < 3; k++) stage[(size_t)k * n + i] = p.base[i * p.rs + k * p.cs];
            HIP_TRY(c, hipMemcpyAsync(col[p.first_col], stage.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
        }
    }
    HIP_TRY(c, hipGetLastError());
    return SYMMICP_OK;
}

// Morton order of a planar cloud: fills order[n] (sorted position -> row) and, optionally, keeps the sorted keys.
int morton_order(symmicp_ctx *c, const CloudSoA &cl, uint32_t n, DevBuf<uint32_t> &vals, DevBuf<uint32_t> *keys_out, float origin[3], float *h0_out)
{
    DevBuf<uint32_t> bbox, keys_local, kt, vt, ws;
    DevBuf<uint32_t> &keys = keys_out ? *keys_out : keys_local;
    const size_t wse = radix_sort_ws_elems(n);
    HIP_TRY(c, bbox.alloc_temp(c->arena, 6));
    HIP_TRY(c, keys.alloc_temp(c->arena, n));
    HIP_TRY(c, vals.alloc_temp(c->arena, n));
    HIP_TRY(c, kt.alloc_temp(c->arena, n));
    HIP_TRY(c, vt.alloc_temp(c->arena, n));
    HIP_TRY(c, ws.alloc_temp(c->arena, wse));
    launch_bbox(cl.x, cl.y, cl.z, n, bbox.p, c->stream);
    uint32_t hb[6];
    HIP_TRY(c, hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float lo[3], hi[3];
    for (int k = 0; k < 3; k++) { lo[k] = ord2f(hb[k]); hi[k] = ord2f(hb[3 + k]); }
    float emax = 0.f;
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(lo[k]) || !std::isfinite(hi[k])) return fail(c, SYMMICP_ERR_ARG, "cloud has non-finite coordinates");
        emax = std::fmax(emax, hi[k] - lo[k]);
    }
    if (!(emax > 0.f)) emax = 1.f;
    const float h0 = emax * 1.00001f / (float)(1 << kMortonBits);
    launch_morton(cl.x, cl.y, cl.z, n, lo[0], lo[1], lo[2], 1.0f / h0, keys.p, vals.p, c->stream);
    radix_sort_pairs(keys.p, vals.p, kt.p, vt.p, n, 3 * kMortonBits, ws.p, wse, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    for (int k = 0; k < 3; k++) origin[k] = lo[k];
    *h0_out = h0;
    return SYMMICP_OK;
}

// sparse octree over the sorted keys (levels 0..kMortonBits, built bottom-up); see TargetIndex::onodes
static int build_octree(symmicp_ctx *c, IndexStore &store, const uint32_t *keys, uint32_t n, uint32_t leaf_max, TargetIndex *ix)
{
    constexpr int NL = kMortonBits + 1;
    DevBuf<uint32_t> nid;                         // [NL][n]: id of the node that starts at point i, per level
    DevBuf<uint32_t> scan_ws, first;
    float4 *nodes = nullptr;
    HIP_TRY(c, nid.alloc_temp(c->arena, (size_t)NL * n));
    HIP_TRY(c, scan_ws.alloc_temp(c->arena, (size_t)n / 2048 + 2));
    for (int l = 0; l < NL; l++) {
        launch_oct_flags(keys, n, l, nid.p + (size_t)l * n, c->stream);
        launch_exclusive_scan(nid.p + (size_t)l * n, n, scan_ws.p, c->stream);
    }
    // node counts: exclusive scan value at the last point, +1 if the last point starts a node (host checks the keys)
    uint32_t last_excl[NL], kl[2] = {0, 0};
    for (int l = 0; l < NL; l++)
        HIP_TRY(c, hipMemcpyAsync(&last_excl[l], nid.p + (size_t)l * n + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (n >= 2) HIP_TRY(c, hipMemcpyAsync(kl, keys + (n - 2), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t cnt[NL];
    size_t total = 0;
    for (int l = 0; l < NL; l++) {
        const int shift = 3 * (kMortonBits - l);
        const bool last_starts = (n == 1) || (shift < 30 && (kl[1] >> shift) != (kl[0] >> shift));
        cnt[l] = last_excl[l] + (last_starts ? 1u : 0u);
        ix->olevel_off[l] = (uint32_t)total;
        total += cnt[l];
    }
    ix->olevel_off[NL] = (uint32_t)total;
    for (int l = 0; l < NL; l++)
        // child_first is a 28-bit field of the node word: targets beyond ~268M distinct finest cells are refused
        if (cnt[l] > kOctCfMask) return fail(c, SYMMICP_ERR_SIZE, "octree level exceeds 2^28 nodes (target cloud too large for SYMMICP_CORR_TREE)");
    HIP_TRY(c, first.alloc_temp(c->arena, total + 1));
    HIP_TRY(c, store.alloc((void **)&nodes, sizeof(float4) * 2 * total));
    for (int l = 0; l < NL; l++)
        launch_oct_first(keys, n, l, nid.p + (size_t)l * n, first.p + ix->olevel_off[l], c->stream);
    for (int l = NL - 1; l >= 0; l--) {
        const bool bottom = (l == NL - 1);
        launch_oct_nodes(l, ix->tq, n, first.p + ix->olevel_off[l], cnt[l], bottom ? nullptr : nid.p + (size_t)(l + 1) * n,
                         bottom ? 0u : cnt[l + 1], bottom ? nullptr : nodes + 2 * (size_t)ix->olevel_off[l + 1],
                         nodes + 2 * (size_t)ix->olevel_off[l], leaf_max, c->stream);
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    ix->onodes = nodes;
    return SYMMICP_OK;
}

// Search index over a planar cloud: Morton sort -> float4 gather -> (optional) dense cell table at the chosen octree level -> implicit
// 8-ary box tree -> (optional) octree.  *out is written on success only; what a failed build took from the store is the caller's to rewind.
int build_index(symmicp_ctx *c, IndexStore &store, const CloudSoA &cl, uint32_t n, const IndexRequest &rq, BuiltIndex *out)
{
    DevBuf<uint32_t> order, keys;
    BuiltIndex b;
    IndexNotes &notes = b.notes;
    float h0;
    int st = morton_order(c, cl, n, order, &keys, notes.origin, &h0);
    if (st != SYMMICP_OK) return st;
    notes.h0 = h0;
    launch_gather_f4(cl.x, cl.y, cl.z, cl.nx, cl.ny, cl.nz, order.p, n, rq.tq, rq.tn, c->stream);
    TargetIndex &ix = b.ix;
    ix.tq = rq.tq; ix.tn = rq.tn; ix.n = n;
    int glevel = 0;
    if (rq.grid) {
        DevBuf<uint32_t> hist;
        HIP_TRY(c, hist.alloc_temp(c->arena, 16));
        launch_level_hist(keys.p, n, hist.p, c->stream);
        uint32_t *hh = notes.hist;
        HIP_TRY(c, hipMemcpyAsync(hh, hist.p, sizeof(notes.hist), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        // finest level whose occupied cells still hold >= ppc points on average
        const double ppc = c->sw.grid_ppc;
        int lcap = c->sw.grid_maxlevel;                  // the table is two-level: memory follows the occupied super-cells
        if (lcap > kMortonBits) lcap = kMortonBits;
        glevel = 1;
        double occ = 1.0;
        for (int l = 1; l <= lcap; l++) {
            occ += (double)hh[l];
            if ((double)n / occ >= ppc) glevel = l;
        }
        if (c->sw.grid_level >= 0) glevel = c->sw.grid_level;   // 0 disables the grid phase
        if (glevel > lcap) glevel = lcap;
        if (glevel < 0) glevel = 0;
        // Is the target a surface or a volume?  Occupied cells grow ~4x per octree level on a surface and ~8x in a volume
        // (measured one level above the grid level, where cells still hold several points).  On surface-like targets the
        // queries of a packet share most of their search (offset surfaces: every ball touches the target in a wide disc), so
        // the first pass runs as packets (kernels_packet.hip) over an octree with larger leaves; in a volume cloud the
        // neighbours are half a spacing away, nothing is shared, and the per-thread walk stays (100k uniform cube, first
        // pass: 0.11 ms per-thread walk, 0.31 ms packets; 1M surface pair: 1.69 ms against 0.87 ms).
        {
            double occ_l[kMortonBits + 1];
            double o = 1.0;
            occ_l[0] = 1.0;
            for (int l = 1; l <= kMortonBits; l++) { o += (double)hh[l]; occ_l[l] = o; }
            const int lg = glevel >= 2 ? glevel - 1 : 1;
            const double growth = occ_l[lg] / occ_l[lg - 1];
            b.surface_like = growth < 5.5;
            if (c->sw.first_pass >= 0) b.surface_like = c->sw.first_pass == 1;      // SYMMICP_FIRST_PASS=packet|walk: A/B runs
        }
    }
    ix.glevel = glevel;
    if (glevel > 0) {
        const int ltop = glevel > 3 ? glevel - 3 : 0;
        const size_t ntop = (size_t)1 << (3 * ltop);
        // block numbers of the occupied super-cells: exclusive scan of their start flags
        DevBuf<uint32_t> nid_top, scan_ws;
        HIP_TRY(c, nid_top.alloc_temp(c->arena, n));
        HIP_TRY(c, scan_ws.alloc_temp(c->arena, (size_t)n / 2048 + 2));
        launch_oct_flags(keys.p, n, ltop, nid_top.p, c->stream);
        launch_exclusive_scan(nid_top.p, n, scan_ws.p, c->stream);
        uint32_t last_excl = 0, kl[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(&last_excl, nid_top.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        if (n >= 2) HIP_TRY(c, hipMemcpyAsync(kl, keys.p + (n - 2), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        const int tshift = 3 * (kMortonBits - ltop);
        const bool last_starts = (n == 1) || (tshift < 30 && (kl[1] >> tshift) != (kl[0] >> tshift));
        const size_t nblocks = (size_t)last_excl + (last_starts ? 1 : 0);
        notes.nblocks = (uint32_t)nblocks; notes.ctop_len = (uint32_t)ntop;
        uint32_t *ctop = nullptr;
        uint2 *cells = nullptr;
        HIP_TRY(c, store.alloc((void **)&ctop, sizeof(uint32_t) * ntop));
        HIP_TRY(c, hipMemsetAsync(ctop, 0xFF, sizeof(uint32_t) * ntop, c->stream));
        HIP_TRY(c, store.alloc((void **)&cells, sizeof(uint2) * nblocks * 512));
        HIP_TRY(c, hipMemsetAsync(cells, 0, sizeof(uint2) * nblocks * 512, c->stream));
        launch_cell_table(keys.p, n, glevel, nid_top.p, ctop, cells, c->stream);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        ix.ctop = ctop;
        ix.cells = cells;
        ix.gdim = 1 << glevel;
        ix.ox = notes.origin[0]; ix.oy = notes.origin[1]; ix.oz = notes.origin[2];
        ix.h = h0 * (float)(1 << (kMortonBits - glevel));
        ix.inv_h = (1.0f / h0) / (float)(1 << (kMortonBits - glevel));
    }
    // tree levels: level 0 = leaves of kLeaf points, each level padded to a multiple of kFan
    uint32_t cnt[kMaxTreeLevels], pad[kMaxTreeLevels];
    int nl = 0;
    uint32_t m = (n + kLeaf - 1) / kLeaf;
    size_t total = 0;
    while (true) {
        cnt[nl] = m;
        pad[nl] = (m <= (uint32_t)kFan) ? m : ((m + kFan - 1) / kFan) * kFan;
        ix.level_off[nl] = (uint32_t)total;
        total += pad[nl];
        nl++;
        if (m <= (uint32_t)kFan) break;
        m = pad[nl - 1] / kFan;
        if (nl >= kMaxTreeLevels) return fail(c, SYMMICP_ERR_SIZE, "tree too deep");
    }
    ix.top = nl - 1;
    ix.ntop = cnt[nl - 1];
    float4 *boxes = nullptr;
    HIP_TRY(c, store.alloc((void **)&boxes, sizeof(float4) * 2 * total));
    launch_leaf_boxes(ix.tq, n, boxes + 2 * (size_t)ix.level_off[0], pad[0], c->stream);
    for (int l = 1; l < nl; l++)
        launch_node_boxes(boxes + 2 * (size_t)ix.level_off[l - 1], pad[l - 1], boxes + 2 * (size_t)ix.level_off[l], pad[l], c->stream);
    ix.boxes = boxes;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (rq.oct_leaf >= 0) {
        // (packets: 12 / 16 / 20 / 24 / 28 points per leaf: 0.425 / 0.411 / 0.394 / 0.389 / 0.394 ms first pass of the 1M surface pair)
        notes.leaf_max = rq.oct_leaf > 0 ? (uint32_t)rq.oct_leaf : (b.surface_like ? 24u : 8u);
        st = build_octree(c, store, keys.p, n, notes.leaf_max, &ix);
        if (st != SYMMICP_OK) return st;
    }
    b.grid_level = glevel;
    b.tree_levels = nl;
    *out = b;
    return SYMMICP_OK;
}

// ---- the scratch index of a cloud operation -----------------------------------------------------------------------------
ScratchIndex::~ScratchIndex()
{
    if (!c) return;      // begin() never got as far as the mark
    (void)hipStreamSynchronize(c->stream);
    c->tgt_store.rewind(mark);
}

int ScratchIndex::begin(symmicp_ctx *ctx, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n, size_t temp_bytes)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    IndexStore &store = ctx->tgt_store;
    // no target yet: give the store the size this cloud needs (a later set_target reuses it)
    if (store.cap() == 0) store.reserve(n * 96 + ((size_t)4 << 20), 0);
    c = ctx;
    mark = store.mark();
    arena_begin(c->arena, n * (96 + 4 * (xr + (nrm ? nr : 0))) + temp_bytes + ((size_t)1 << 20));
    DevBuf<float> block;      // (from the store: not owned)
    if (int st = upload_planar(c, xyz, xr, xc, nrm, nr, nc, n, block, &store, nullptr)) return st;
    CloudSoA cl;
    soa_from_block(block.p, n, cl);
    IndexRequest rq{nullptr, nullptr, /*grid=*/false, /*oct_leaf=*/-1};
    if (store.alloc((void **)&rq.tq, sizeof(float4) * (n + 8)) != hipSuccess || store.alloc((void **)&rq.tn, sizeof(float4) * 2 * n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, SYMMICP_ERR_HIP, "out of device memory");
    }
    BuiltIndex b;
    if (int st = build_index(c, store, cl, (uint32_t)n, rq, &b)) return st;
    ix = b.ix;
    return SYMMICP_OK;
}

// ---- the reverse index -------------------------------------------------------------------------------------------------------
// The source index of reciprocal passes (and the scratch index of the evaluation): no grid, and an octree with leaves of 8 points whatever
// the cloud looks like and whatever SYMMICP_OCT_LEAF says (that switch tunes the target's octree for the packet search).  The pair
// records (tn) are not needed: they go to the scratch arena.  Persistent: tq 16 B, the octree ~64 B and the run tree ~5 B per point.
static int fill_reverse_index(symmicp_ctx *c, const CloudSoA &cl, uint32_t n, const uint32_t *labels, ReverseIndex &ri)
{
    IndexRequest rq{nullptr, nullptr, /*grid=*/false, /*oct_leaf=*/8};
    DevBuf<float4> tn;
    HIP_TRY(c, ri.store.alloc((void **)&rq.tq, sizeof(float4) * ((size_t)n + 8)));
    HIP_TRY(c, hipMemsetAsync(rq.tq + n, 0, sizeof(float4) * 8, c->stream));
    HIP_TRY(c, tn.alloc_temp(c->arena, 2 * (size_t)n));
    rq.tn = tn.p;
    BuiltIndex b;
    if (int st = build_index(c, ri.store, cl, n, rq, &b)) return st;
    launch_relabel_tq(rq.tq, n, labels, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // (tn is about to go out of scope)
    HIP_TRY(c, hipGetLastError());
    ri.ix = b.ix;
    return SYMMICP_OK;
}

int build_reverse_index(symmicp_ctx *c, const CloudSoA &cl, uint32_t n, const uint32_t *labels, ReverseIndex &ri)
{
    ri.drop();
    ri.store.reserve((size_t)n * 96 + ((size_t)4 << 20), 0);
    arena_begin(c->arena, (size_t)n * 128 + ((size_t)1 << 20));
    if (int st = fill_reverse_index(c, cl, n, labels, ri)) {
        (void)hipStreamSynchronize(c->stream);      // (kernels of the failed build may still write what the store gives back)
        ri.drop();
        return st;
    }
    ri.valid = true;
    return SYMMICP_OK;
}
