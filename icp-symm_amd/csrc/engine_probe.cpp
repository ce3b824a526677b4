// engine_probe.cpp -- test entries of the index build (include/symmicp.h, "test entry points of the index build"): read-back of the
// target index and of the source share, and the build's two primitives (the radix sort and the exclusive scan) on caller arrays.
// Nothing here is on a hot path, and nothing here changes the context: the read-backs copy device arrays to the host, the
// primitives work in the scratch arena, which is dead between public calls anyway.
#include "engine_internal.h"

namespace {

int copy_back(symmicp_ctx *c, void *dst, const void *src, size_t bytes)
{
    if (!dst || !bytes) return SYMMICP_OK;
    if (!src) return fail(c, SYMMICP_ERR_STATE, "probe: the context does not hold this array");
    HIP_TRY(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return SYMMICP_OK;
}

bool has_target_index(const symmicp_ctx *c) { return c->have_index && c->cfg.corr == SYMMICP_CORR_TREE && c->ix.tq && c->ix.boxes && c->ix.onodes; }

void fill_info(const symmicp_ctx *c, symmicp_index_info *o)
{
    const TargetIndex &ix = c->ix;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->n = ix.n;
    o->grid_level = ix.glevel;
    o->gdim = ix.gdim;
    for (int k = 0; k < 3; k++) o->origin[k] = c->notes.origin[k];
    o->h0 = c->notes.h0;
    o->h = ix.h;
    o->inv_h = ix.inv_h;
    o->tree_levels = ix.top + 1;
    o->top = ix.top;
    o->ntop = ix.ntop;
    static_assert(sizeof(o->level_off) == sizeof(ix.level_off) && sizeof(o->olevel_off) == sizeof(ix.olevel_off), "info mirrors TargetIndex");
    std::memcpy(o->level_off, ix.level_off, sizeof(o->level_off));
    o->n_boxes = ix.level_off[ix.top] + ix.ntop;          // (the top level is not padded)
    std::memcpy(o->olevel_off, ix.olevel_off, sizeof(o->olevel_off));
    o->n_onodes = ix.olevel_off[kMortonBits + 1];
    o->n_blocks = c->notes.nblocks;
    o->ctop_len = c->notes.ctop_len;
    o->leaf_max = c->notes.leaf_max;
    o->surface_like = c->target_surface_like ? 1 : 0;
    std::memcpy(o->level_hist, c->notes.hist, sizeof(o->level_hist));
}

}  // namespace

extern "C" {

int symmicp_ctx_index_info(symmicp_ctx *c, symmicp_index_info *info)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!info || info->struct_size != (int32_t)sizeof(symmicp_index_info)) return fail(c, SYMMICP_ERR_ARG, "index_info: null info or wrong struct_size");
    if (!has_target_index(c)) return fail(c, SYMMICP_ERR_STATE, "index_info: no target index (SYMMICP_CORR_TREE after set_target)");
    fill_info(c, info);
    return SYMMICP_OK;
}

int symmicp_ctx_index_arrays(symmicp_ctx *c, float *tq, float *tn, float *boxes, uint32_t *ctop, uint32_t *cells, float *onodes)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!has_target_index(c)) return fail(c, SYMMICP_ERR_STATE, "index_arrays: no target index (SYMMICP_CORR_TREE after set_target)");
    symmicp_index_info o;
    fill_info(c, &o);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t f4 = sizeof(float4);
    const struct { void *dst; const void *src; size_t bytes; } parts[] = {
        {tq, c->ix.tq, f4 * o.n},
        {tn, c->ix.tn, f4 * 2 * o.n},
        {boxes, c->ix.boxes, f4 * 2 * o.n_boxes},
        {ctop, c->ix.ctop, sizeof(uint32_t) * (o.grid_level > 0 ? o.ctop_len : 0)},
        {cells, c->ix.cells, sizeof(uint2) * 512 * (size_t)(o.grid_level > 0 ? o.n_blocks : 0)},
        {onodes, c->ix.onodes, f4 * 2 * o.n_onodes},
    };
    for (const auto &p : parts) {
        const int st = copy_back(c, p.dst, p.src, p.bytes);
        if (st != SYMMICP_OK) { (void)hipStreamSynchronize(c->stream); return st; }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

// diagnostic: the pair certificates as they stand, in the share's sorted order: (ref.xyz, L), the neighbourhood's 8 members and radius, the
// current winner, target points named by their ROW in the caller's target cloud (the device holds sorted positions)
int symmicp_get_certificates(symmicp_ctx *c, float *cert4, uint32_t *hood8, float *hood_radius, int32_t *winner_row, size_t cap)
{
    if (!c || !cert4) return SYMMICP_ERR_ARG;
    if (!c->begun || !c->cert) return fail(c, SYMMICP_ERR_STATE, "no tree pass has run yet");
    if (cap < c->n_loc) return fail(c, SYMMICP_ERR_SIZE, "output too small");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemcpyAsync(cert4, c->cert, sizeof(float) * 4 * c->n_loc, hipMemcpyDeviceToHost, c->stream));
    std::vector<int32_t> pos(winner_row ? c->n_loc : 0);
    std::vector<float> tq((hood8 || winner_row) ? (size_t)c->n_t * 4 : 0);
    if (hood8) HIP_TRY(c, hipMemcpyAsync(hood8, c->certk, sizeof(uint32_t) * 8 * c->n_loc, hipMemcpyDeviceToHost, c->stream));
    std::vector<float> tr(hood_radius ? (size_t)c->n_loc * 2 : 0);
    if (hood_radius) HIP_TRY(c, hipMemcpyAsync(tr.data(), c->hoodr, sizeof(float) * 2 * c->n_loc, hipMemcpyDeviceToHost, c->stream));
    if (winner_row) HIP_TRY(c, hipMemcpyAsync(pos.data(), c->pos, sizeof(int32_t) * c->n_loc, hipMemcpyDeviceToHost, c->stream));
    if (!tq.empty()) HIP_TRY(c, hipMemcpyAsync(tq.data(), c->ix.tq, sizeof(float) * 4 * c->n_t, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto row_of = [&](uint32_t p) -> uint32_t {
        if (p >= c->n_t) return 0xFFFFFFFFu;
        uint32_t r; std::memcpy(&r, &tq[(size_t)p * 4 + 3], 4); return r;      // the row rides in the w slot of the sorted point
    };
    for (size_t i = 0; i < c->n_loc; i++) {
        if (hood8) for (int k = 0; k < 8; k++) hood8[i * 8 + k] = row_of(hood8[i * 8 + k]);
        if (winner_row) winner_row[i] = pos[i] < 0 ? -1 : (int32_t)row_of((uint32_t)pos[i]);
        if (hood_radius) hood_radius[i] = tr[i * 2];
    }
    return SYMMICP_OK;
}

int symmicp_ctx_source_share(symmicp_ctx *c, size_t *n_local, size_t *pkt_count, int32_t *sorted, int32_t *cost_keyed, uint32_t *order,
                             uint32_t *pkt_tab)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->src0_block) return fail(c, SYMMICP_ERR_STATE, "source_share: no source (set_source first)");
    if (order && !c->src_order) return fail(c, SYMMICP_ERR_STATE, "source_share: the share is not sorted (it is in the caller's order)");
    if (n_local) *n_local = c->n_loc;
    if (pkt_count) *pkt_count = c->pkt_tab ? c->pkt_count : 0;
    if (sorted) *sorted = c->src_order ? 1 : 0;
    if (cost_keyed) *cost_keyed = (c->pkt_tab && c->pkt_cost_keyed) ? 1 : 0;
    if (!order && !pkt_tab) return SYMMICP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    int st = copy_back(c, order, c->src_order, sizeof(uint32_t) * c->n_loc);
    if (st == SYMMICP_OK && c->pkt_tab) st = copy_back(c, pkt_tab, c->pkt_tab, sizeof(uint32_t) * 2 * c->pkt_count);
    const hipError_t e = hipStreamSynchronize(c->stream);
    if (st != SYMMICP_OK) return st;
    HIP_TRY(c, e);
    return SYMMICP_OK;
}

int symmicp_ctx_radix_sort_probe(symmicp_ctx *c, uint32_t *keys, uint32_t *vals, size_t n, int key_bits)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (key_bits < 0 || key_bits > 32 || n > 0x7fffffffull || (n && (!keys || !vals))) return fail(c, SYMMICP_ERR_ARG, "radix_sort_probe: bad arguments");
    if (n == 0) return SYMMICP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const uint32_t m = (uint32_t)n;
    const size_t wse = radix_sort_ws_elems(m), bytes = sizeof(uint32_t) * n;
    arena_begin(c->arena, 4 * (bytes + 256) + sizeof(uint32_t) * wse + 4096);
    DevBuf<uint32_t> k, v, kt, vt, ws;
    HIP_TRY(c, k.alloc_temp(c->arena, n));
    HIP_TRY(c, v.alloc_temp(c->arena, n));
    HIP_TRY(c, kt.alloc_temp(c->arena, n));
    HIP_TRY(c, vt.alloc_temp(c->arena, n));
    HIP_TRY(c, ws.alloc_temp(c->arena, wse));
    HIP_TRY(c, hipMemcpyAsync(k.p, keys, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(v.p, vals, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));        // (pageable host memory: the copies are done before the buffers may go)
    radix_sort_pairs(k.p, v.p, kt.p, vt.p, m, key_bits, ws.p, wse, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(keys, k.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(vals, v.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

int symmicp_ctx_select_probe(symmicp_ctx *c, const uint32_t *keys, size_t n, uint64_t k, uint32_t *kth_out, uint64_t *n_le_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!keys || !kth_out || !n_le_out || n == 0 || n > 0x7fffffffull || k < 1 || k > n) return fail(c, SYMMICP_ERR_ARG, "select_probe: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(uint32_t) * n;
    arena_begin(c->arena, bytes + sizeof(uint32_t) * kRejectWsWords + 4096);
    DevBuf<uint32_t> d, ws;
    HIP_TRY(c, d.alloc_temp(c->arena, n));
    HIP_TRY(c, ws.alloc_temp(c->arena, kRejectWsWords));      // (its own workspace: the context's trim state stays as it was)
    HIP_TRY(c, hipMemcpyAsync(d.p, keys, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_select_probe(d.p, (uint32_t)n, (uint32_t)k, ws.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    uint32_t state[8] = {};
    HIP_TRY(c, hipMemcpyAsync(state, ws.p, sizeof(state), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *kth_out = state[kRejectTauWord];
    *n_le_out = state[4];
    return SYMMICP_OK;
}

int symmicp_ctx_unique_probe(symmicp_ctx *c, const int32_t *tgt_row, const uint32_t *d2_bits, size_t n, size_t n_t, uint8_t *winner_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!tgt_row || !d2_bits || !winner_out || n == 0 || n > 0x7fffffffull || n_t == 0 || n_t > 0x7fffffffull) return fail(c, SYMMICP_ERR_ARG, "unique_probe: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    arena_begin(c->arena, (sizeof(int32_t) + sizeof(uint32_t) + 1) * n + sizeof(unsigned long long) * n_t + 4096);
    DevBuf<int32_t> d_row;
    DevBuf<uint32_t> d_d2;
    DevBuf<unsigned long long> table;      // (its own table: the context's claim table and rejection state stay as they were)
    DevBuf<uint8_t> d_win;
    HIP_TRY(c, table.alloc_temp(c->arena, n_t));
    HIP_TRY(c, d_row.alloc_temp(c->arena, n));
    HIP_TRY(c, d_d2.alloc_temp(c->arena, n));
    HIP_TRY(c, d_win.alloc_temp(c->arena, n));
    HIP_TRY(c, hipMemcpyAsync(d_row.p, tgt_row, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_d2.p, d2_bits, sizeof(uint32_t) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_unique_probe(d_row.p, d_d2.p, (uint32_t)n, table.p, (uint32_t)n_t, d_win.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(winner_out, d_win.p, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

int symmicp_ctx_reverse_nn_probe(symmicp_ctx *c, const float *db_xyz, const int32_t *labels, size_t n_db, const float *q_xyz, size_t n_q,
                                 const float *X16, int32_t *label_out, float *d2_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!db_xyz || !q_xyz || !label_out || !d2_out || n_db == 0 || n_db > 0x7fffffffull || n_q == 0 || n_q > 0x7fffffffull)
        return fail(c, SYMMICP_ERR_ARG, "reverse_nn_probe: bad arguments");
    if (labels)
        for (size_t i = 0; i < n_db; i++)
            if (labels[i] < 0) return fail(c, SYMMICP_ERR_ARG, "reverse_nn_probe: labels must be below 2^31");
    HIP_TRY(c, hipSetDevice(c->device));
    Affine inv{};
    float Xid[16];
    identity16(Xid);
    symmicp_inverse_rigid(X16 ? X16 : Xid, inv.m);
    // everything in allocations of its own (the index's build rewinds the scratch arena): db as a planar cloud, the labels, the queries, the results
    const size_t o_db = 0, o_lab = o_db + ((sizeof(float) * 3 * n_db + 255) & ~(size_t)255), o_raw = o_lab + ((sizeof(uint32_t) * n_db + 255) & ~(size_t)255),
                 raw_n = std::max(n_db, n_q), o_out = o_raw + ((sizeof(float) * 3 * raw_n + 255) & ~(size_t)255),
                 o_d2 = o_out + ((sizeof(int32_t) * n_q + 255) & ~(size_t)255), total = o_d2 + sizeof(float) * n_q;
    OwnSearch own(c);      // (its own index: the context's source index stays as it was)
    HIP_TRY(c, hipMalloc((void **)&own.d, total));
    char *d = own.d;
    float *raw = reinterpret_cast<float *>(d + o_raw), *col = reinterpret_cast<float *>(d + o_db);
    HIP_TRY(c, hipMemcpyAsync(raw, db_xyz, sizeof(float) * 3 * n_db, hipMemcpyHostToDevice, c->stream));
    if (labels) HIP_TRY(c, hipMemcpyAsync(d + o_lab, labels, sizeof(uint32_t) * n_db, hipMemcpyHostToDevice, c->stream));
    launch_deinterleave3(raw, 3, 0, (uint32_t)n_db, col, col + n_db, col + 2 * n_db, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    CloudSoA cl{col, col + n_db, col + 2 * n_db, col, col + n_db, col + 2 * n_db};      // (no normals: the build reads the slots and nothing keeps them)
    if (int st = build_reverse_index(c, cl, (uint32_t)n_db, labels ? reinterpret_cast<const uint32_t *>(d + o_lab) : nullptr, own.ri)) return st;
    HIP_TRY(c, hipMemcpyAsync(raw, q_xyz, sizeof(float) * 3 * n_q, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_reverse_nn_probe(own.ri.ix, inv, raw, (uint32_t)n_q, reinterpret_cast<int32_t *>(d + o_out), reinterpret_cast<float *>(d + o_d2), c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(label_out, d + o_out, sizeof(int32_t) * n_q, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d2_out, d + o_d2, sizeof(float) * n_q, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

int symmicp_ctx_reciprocal_info(const symmicp_ctx *c, int32_t *index_valid, uint64_t *index_bytes, uint64_t *index_builds, uint64_t *table_words)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (index_valid) *index_valid = c->rej.src_ix.valid ? 1 : 0;
    if (index_bytes) *index_bytes = c->rej.src_ix.store.cap();
    if (index_builds) *index_builds = c->rej.src_ix_builds;
    if (table_words) *table_words = c->rej.table_cap;
    return SYMMICP_OK;
}

int symmicp_ctx_scan_probe(symmicp_ctx *c, uint32_t *data, size_t n)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (n > 0x7fffffffull || (n && !data)) return fail(c, SYMMICP_ERR_ARG, "scan_probe: bad arguments");
    if (n == 0) return SYMMICP_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(uint32_t) * n, tiles = n / 2048 + 2;       // (as build_octree sizes the scan's scratch)
    arena_begin(c->arena, bytes + sizeof(uint32_t) * tiles + 4096);
    DevBuf<uint32_t> d, ws;
    HIP_TRY(c, d.alloc_temp(c->arena, n));
    HIP_TRY(c, ws.alloc_temp(c->arena, tiles));
    HIP_TRY(c, hipMemcpyAsync(d.p, data, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_exclusive_scan(d.p, (uint32_t)n, ws.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(data, d.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

}  // extern "C"
