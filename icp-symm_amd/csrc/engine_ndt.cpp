// engine_ndt.cpp -- the host side of SYMMICP_MODE_NDT (include/symmicp.h, "NDT registration"; kernels_ndt.hip): the configuration and its
// constants, the voxel map of a cloud (the target's, or any cloud's through symmicp_ctx_ndt_map), its read-back, the arguments of a pass.
#include "engine_internal.h"
#include "ndt_core.h"

namespace {

const char *ndt_cfg_error(const symmicp_ndt_config *cfg)
{
    if (!cfg) return "ndt: cfg is required";
    if (cfg->struct_size != (int32_t)sizeof(symmicp_ndt_config)) return "ndt: cfg->struct_size is not sizeof(symmicp_ndt_config)";
    if (!std::isfinite(cfg->resolution) || !(cfg->resolution > 0.f)) return "ndt: resolution must be finite and > 0";
    if (cfg->min_points < 3) return "ndt: min_points must be >= 3";
    if (!(cfg->eig_ratio > 0.f) || !(cfg->eig_ratio <= 1.f)) return "ndt: eig_ratio must be in (0, 1]";
    if (!(cfg->outlier_ratio > 0.f) || !(cfg->outlier_ratio < 1.f)) return "ndt: outlier_ratio must be in (0, 1)";
    if (cfg->neighbors != 1 && cfg->neighbors != 7) return "ndt: neighbors must be 1 or 7";
    return nullptr;
}

// The grid over a box, symmicp_ctx_voxel_downsample's in fp32 with IEEE ops, plus the 2^23 rule.  g: inv, lo, hi, lo_i, nx, ny
const char *ndt_grid(const float bmin[3], const float bmax[3], float resolution, NdtGrid &g, int32_t dims[3], int *bits_out)
{
    const float inv = 1.0f / resolution;
    g.inv = inv;
    uint64_t dim[3];
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(bmin[k]) || !std::isfinite(bmax[k])) return "cloud has non-finite coordinates";
        const float flo = std::floor(bmin[k] * inv), fhi = std::floor(bmax[k] * inv);
        // (cell coordinates below 2^23 are exact as floats, with their neighbours; this also covers the int32 rule of the voxel grid)
        if (!(std::fabs(flo) < 8388608.0f && std::fabs(fhi) < 8388608.0f))
            return "ndt: resolution is too small for the cloud: a cell coordinate reaches 2^23";
        g.lo[k] = flo; g.hi[k] = fhi;
        g.lo_i[k] = (int32_t)flo;
        dim[k] = (uint64_t)((int64_t)(int32_t)fhi - (int64_t)g.lo_i[k] + 1);
        dims[k] = (int32_t)dim[k];
    }
    const unsigned __int128 total = (unsigned __int128)dim[0] * dim[1] * dim[2];
    if (total > ((unsigned __int128)1 << 32)) return "ndt: resolution is too small for the cloud: more than 2^32 voxels in its box";
    int bits = 0;
    while (((unsigned __int128)1 << bits) < total) bits++;
    g.nx = (uint32_t)dim[0]; g.ny = (uint32_t)dim[1];
    *bits_out = bits;
    return nullptr;
}

// The map of a planar cloud in device memory into `map` (grown as needed).  Temporaries from the context's scratch arena, which the caller
// has rewound.  Box -> grid -> keys -> stable radix sort of (key, row) -> segments -> voxels with >= min_points points -> sorted gather
// -> one thread per voxel (mean, covariance, Jacobi) -> the surviving voxels compacted -> the lookup table.
int ndt_build(symmicp_ctx *c, const CloudSoA &cl, size_t n, const symmicp_ndt_config &cfg, NdtMap &map)
{
    map.valid = false;
    map.m = 0;
    const uint32_t n32 = (uint32_t)n;
    DevBuf<uint32_t> bbox;
    HIP_TRY(c, bbox.alloc_temp(c->arena, 6));
    launch_bbox(cl.x, cl.y, cl.z, n32, bbox.p, c->stream);
    uint32_t hb[6];
    HIP_TRY(c, hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float bmin[3], bmax[3];
    for (int k = 0; k < 3; k++) { bmin[k] = ord2f(hb[k]); bmax[k] = ord2f(hb[3 + k]); }
    NdtGrid g{};
    int bits = 0;
    if (const char *msg = ndt_grid(bmin, bmax, cfg.resolution, g, map.dims, &bits)) return fail(c, SYMMICP_ERR_ARG, msg);
    const uint64_t nx = g.nx, ny = g.ny;

    DevBuf<uint32_t> keys, rows, kt, vt, ws, vid, first, kid, kfirst, kcount, scan_ws, words;
    DevBuf<float> sorted;
    const size_t wse = radix_sort_ws_elems(n32);
    HIP_TRY(c, keys.alloc_temp(c->arena, n));
    HIP_TRY(c, rows.alloc_temp(c->arena, n));
    HIP_TRY(c, kt.alloc_temp(c->arena, n));
    HIP_TRY(c, vt.alloc_temp(c->arena, n));
    HIP_TRY(c, ws.alloc_temp(c->arena, wse));
    HIP_TRY(c, vid.alloc_temp(c->arena, n));
    HIP_TRY(c, first.alloc_temp(c->arena, n + 1));
    HIP_TRY(c, kid.alloc_temp(c->arena, n));
    HIP_TRY(c, kfirst.alloc_temp(c->arena, n));
    HIP_TRY(c, kcount.alloc_temp(c->arena, n));
    HIP_TRY(c, scan_ws.alloc_temp(c->arena, n / 2048 + 2));
    HIP_TRY(c, words.alloc_temp(c->arena, 2));
    HIP_TRY(c, sorted.alloc_temp(c->arena, 6 * n));
    launch_voxel_keys(cl, n32, g.inv, g.lo_i, nx, ny, keys.p, rows.p, c->stream);
    radix_sort_pairs(keys.p, rows.p, kt.p, vt.p, n32, bits, ws.p, wse, c->stream);
    launch_voxel_segments(keys.p, n32, vid.p, first.p, scan_ws.p, words.p, c->stream);
    uint32_t m0 = 0, mk = 0;
    HIP_TRY(c, hipMemcpyAsync(&m0, words.p, sizeof(m0), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_voxel_keep(first.p, m0, (uint32_t)cfg.min_points, kid.p, scan_ws.p, kfirst.p, kcount.p, words.p + 1, c->stream);
    HIP_TRY(c, hipMemcpyAsync(&mk, words.p + 1, sizeof(mk), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());

    uint32_t m = 0;
    if (mk > 0) {
        CloudSoA sc;
        soa_from_block(sorted.p, n, sc);
        launch_gather_soa(cl, rows.p, n32, sc, c->stream);
        DevBuf<float4> t_rec;
        DevBuf<double> t_cov;
        DevBuf<uint32_t> t_key, valid, pos;
        HIP_TRY(c, t_rec.alloc_temp(c->arena, 4 * (size_t)mk));
        HIP_TRY(c, t_cov.alloc_temp(c->arena, 6 * (size_t)mk));
        HIP_TRY(c, t_key.alloc_temp(c->arena, mk));
        HIP_TRY(c, valid.alloc_temp(c->arena, mk));
        HIP_TRY(c, pos.alloc_temp(c->arena, mk));
        launch_ndt_voxels(sc, keys.p, kfirst.p, kcount.p, mk, cfg.eig_ratio, t_rec.p, t_cov.p, t_key.p, valid.p, c->stream);
        HIP_TRY(c, hipMemcpyAsync(pos.p, valid.p, sizeof(uint32_t) * mk, hipMemcpyDeviceToDevice, c->stream));
        launch_exclusive_scan(pos.p, mk, scan_ws.p, c->stream);
        uint32_t last_pos = 0, last_valid = 0;
        HIP_TRY(c, hipMemcpyAsync(&last_pos, pos.p + (mk - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&last_valid, valid.p + (mk - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        m = last_pos + last_valid;
        if (m > mk) return fail(c, SYMMICP_ERR_HIP, "ndt: voxel count out of range");
        HIP_TRY(c, grow(map.rec, map.rec_cap, 4 * (size_t)(m ? m : 1)));
        HIP_TRY(c, grow(map.cov, map.cov_cap, 6 * (size_t)(m ? m : 1)));
        HIP_TRY(c, grow(map.key, map.key_cap, (size_t)(m ? m : 1)));
        launch_ndt_compact(t_rec.p, t_cov.p, t_key.p, valid.p, pos.p, mk, map.rec, map.cov, map.key, c->stream);
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the temporaries are about to go out of scope)
        HIP_TRY(c, hipGetLastError());
    }
    // the table: a power of two >= 2 m, at least 2
    int lg = 1;
    while (((size_t)1 << lg) < 2 * (size_t)m) lg++;
    const size_t capacity = (size_t)1 << lg;
    HIP_TRY(c, grow(map.table, map.table_cap, capacity));
    HIP_TRY(c, hipMemsetAsync(map.table, 0, sizeof(unsigned long long) * capacity, c->stream));
    g.shift = (uint32_t)(32 - lg);
    g.mask = (uint32_t)(capacity - 1);
    launch_ndt_insert(map.key, m, map.table, g.shift, g.mask, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    g.rec = map.rec;
    g.table = map.table;
    map.g = g;
    map.m = m;
    map.valid = true;
    return SYMMICP_OK;
}

// a map's arrays to the caller (each may be NULL); the cap protocol of the voxel entry
int ndt_read_map(symmicp_ctx *c, const NdtMap &map, const char *who, uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out,
                 float *axes_out, float *inv_eig_out, int32_t grid_out[6], size_t cap, size_t *m_out)
{
    const size_t m = map.m;
    *m_out = m;
    if (m > cap) return fail(c, SYMMICP_ERR_SIZE, std::string(who) + ": " + std::to_string(m) + " voxels do not fit cap " + std::to_string(cap));
    if (grid_out)
        for (int k = 0; k < 3; k++) { grid_out[k] = map.g.lo_i[k]; grid_out[3 + k] = map.dims[k]; }
    if (m == 0) return SYMMICP_OK;
    if (key_out) HIP_TRY(c, hipMemcpyAsync(key_out, map.key, sizeof(uint32_t) * m, hipMemcpyDeviceToHost, c->stream));
    if (cov_out) HIP_TRY(c, hipMemcpyAsync(cov_out, map.cov, sizeof(double) * 6 * m, hipMemcpyDeviceToHost, c->stream));
    std::vector<float> rec;
    if (count_out || mean_out || axes_out || inv_eig_out) {
        rec.resize(16 * m);
        HIP_TRY(c, hipMemcpyAsync(rec.data(), map.rec, sizeof(float) * 16 * m, hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t v = 0; v < m && !rec.empty(); v++) {
        const float *r = rec.data() + 16 * v;
        if (count_out) std::memcpy(count_out + v, r + 3, sizeof(int32_t));
        for (int k = 0; k < 3; k++) {
            if (mean_out) mean_out[3 * v + k] = r[k];
            if (inv_eig_out) inv_eig_out[3 * v + k] = r[4 * (1 + k) + 3];
            if (axes_out)
                for (int a = 0; a < 3; a++) axes_out[9 * v + 3 * k + a] = r[4 * (1 + k) + a];
        }
    }
    return SYMMICP_OK;
}

const char *ndt_map_args_error(const float *xyz, size_t xr, size_t xc, size_t n, const symmicp_ndt_config *cfg, const size_t *m_out)
{
    if (!xyz || !cfg || !m_out) return "ndt_map: xyz, cfg and m_out are required";
    if (n == 0 || n > 0x7fffffffull) return "ndt_map: n must be in 1 .. 2^31 - 1";
    if (const char *msg = ndt_cfg_error(cfg)) return msg;
    float bmin[3], bmax[3];
    for (int a = 0; a < 3; a++) bmin[a] = bmax[a] = xyz[a * xc];
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            const float v = xyz[i * xr + a * xc];
            if (!std::isfinite(v)) return "ndt_map: a coordinate is not finite";
            bmin[a] = std::fmin(bmin[a], v); bmax[a] = std::fmax(bmax[a], v);
        }
    NdtGrid g{};
    int32_t dims[3];
    int bits = 0;
    return ndt_grid(bmin, bmax, cfg->resolution, g, dims, &bits);
}

}  // namespace

const char *ndt_config_refusal(const symmicp_config &cfg)
{
    if (cfg.min_normal_dot > -1.0f) return "SYMMICP_MODE_NDT pairs points with voxels: there is no normal to gate on (min_normal_dot must stay <= -1)";
    if (cfg.apply == SYMMICP_APPLY_INCREMENTAL) return "SYMMICP_MODE_NDT reads the source through the cumulative transform: no SYMMICP_APPLY_INCREMENTAL";
    return nullptr;
}

const char *ndt_context_refusal(const symmicp_ctx *c)
{
    if (c->loss != SYMMICP_LOSS_NONE) return "SYMMICP_MODE_NDT takes no robust loss (set SYMMICP_LOSS_NONE first)";
    if (c->rej.trims()) return "SYMMICP_MODE_NDT takes no trim fraction below 1 (set 1 first)";
    if (c->rej.one_to_one || c->rej.median()) return "SYMMICP_MODE_NDT takes no one-to-one or median-distance rejector (switch them off first)";
    if (c->rej.reciprocal) return "SYMMICP_MODE_NDT takes no reciprocal correspondences (switch them off first)";
    return nullptr;
}

int ndt_build_target_map(symmicp_ctx *c)
{
    arena_begin(c->arena, (size_t)c->n_t * 128 + ((size_t)1 << 20));
    c->ndt.pass_valid = false;
    return ndt_build(c, c->tgt, c->n_t, c->ndt.cfg, c->ndt.map);
}

void ndt_pass_args(const symmicp_ctx *c, const float X[16], NdtPassArgs &a)
{
    a = NdtPassArgs{};
    a.x = c->src0.x; a.y = c->src0.y; a.z = c->src0.z;
    a.n = c->n_loc;
    for (int k = 0; k < 12; k++) a.X.m[k] = X[k];
    a.X.nrm_w = 0.0f;
    for (int k = 0; k < 3; k++) a.pivot[k] = c->pivot[k];
    a.max_d2 = c->cfg.max_corr_dist > 0.f ? c->cfg.max_corr_dist * c->cfg.max_corr_dist : 0.f;
    a.h = (float)(0.5 * c->ndt.d2);
    a.neighbors = c->ndt.cfg.neighbors;
    a.g = c->ndt.map.g;
    a.partials = c->partials;
}

extern "C" {

void symmicp_ndt_config_default(symmicp_ndt_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(*cfg);
    cfg->resolution = 1.0f;
    cfg->min_points = 6;
    cfg->eig_ratio = 0.01f;
    cfg->outlier_ratio = 0.55f;
    cfg->neighbors = 7;
}

int symmicp_ndt_gauss(double outlier_ratio, double *d1, double *d2)
{
    if (!d1 || !d2 || !(outlier_ratio > 0.0) || !(outlier_ratio < 1.0)) return SYMMICP_ERR_ARG;
    const double po = outlier_ratio;
    const double c1 = 10.0 * (1.0 - po), c2 = po;
    const double d3 = -std::log(c2);
    *d1 = -std::log(c1 + c2) - d3;
    *d2 = -2.0 * std::log((-std::log(c1 * std::exp(-0.5) + c2) - d3) / *d1);
    return SYMMICP_OK;
}

float symmicp_ndt_weight(float x) { return ndt_weight(x); }

int symmicp_set_ndt(symmicp_ctx *c, const symmicp_ndt_config *cfg)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = ndt_cfg_error(cfg)) return fail(c, SYMMICP_ERR_ARG, msg);
    const symmicp_ndt_config before = c->ndt.cfg;
    const double d1_before = c->ndt.d1, d2_before = c->ndt.d2;
    c->ndt.cfg = *cfg;
    symmicp_ndt_gauss((double)cfg->outlier_ratio, &c->ndt.d1, &c->ndt.d2);
    if (!ndt_mode(c) || !c->tgt_block) return SYMMICP_OK;
    // a live NDT context: the map of the target it holds, at once; the loop state as after symmicp_set_target
    HIP_TRY(c, hipSetDevice(c->device));
    c->begun = false;
    const int st = ndt_build_target_map(c);
    if (st == SYMMICP_ERR_ARG) {
        // (the new resolution does not fit this target's box: the configuration and the map stay as they were)
        c->ndt.cfg = before; c->ndt.d1 = d1_before; c->ndt.d2 = d2_before;
        const std::string msg = c->err;
        if (ndt_build_target_map(c) != SYMMICP_OK) return SYMMICP_ERR_HIP;
        return fail(c, SYMMICP_ERR_ARG, msg);
    }
    return st;
}

int symmicp_get_ndt(const symmicp_ctx *c, symmicp_ndt_config *cfg)
{
    if (!c || !cfg) return SYMMICP_ERR_ARG;
    *cfg = c->ndt.cfg;
    return SYMMICP_OK;
}

int symmicp_get_ndt_state(const symmicp_ctx *c, double *score, uint64_t *items)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun || !c->ndt.pass_valid) return SYMMICP_ERR_STATE;      // (const context: no message)
    if (score) *score = c->ndt.score;
    if (items) *items = c->ndt.items;
    return SYMMICP_OK;
}

int symmicp_ctx_ndt_map(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_ndt_config *cfg,
                        uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out, float *axes_out, float *inv_eig_out,
                        int32_t grid_out[6], size_t cap, size_t *m_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = ndt_map_args_error(xyz, row_stride, col_stride, n, cfg, m_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    HIP_TRY(c, hipSetDevice(c->device));
    // the cloud and every temporary from the scratch arena, the map in allocations of its own: the context's clouds, index, map and
    // loop state are not touched
    arena_begin(c->arena, n * (128 + 4 * row_stride) + ((size_t)1 << 20));
    NdtMap map;
    auto body = [&]() -> int {
        DevBuf<float> block;
        if (int st = upload_planar(c, xyz, row_stride, col_stride, nullptr, 0, 0, n, block, /*store=*/nullptr, nullptr)) return st;
        CloudSoA cl;
        soa_from_block(block.p, n, cl);
        if (int st = ndt_build(c, cl, n, *cfg, map)) return st;
        return ndt_read_map(c, map, "ndt_map", key_out, count_out, mean_out, cov_out, axes_out, inv_eig_out, grid_out, cap, m_out);
    };
    const int st = body();
    (void)hipStreamSynchronize(c->stream);
    map.release();
    return st;
}

int symmicp_ndt_map(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_ndt_config *cfg,
                    uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out, float *axes_out, float *inv_eig_out,
                    int32_t grid_out[6], size_t cap, size_t *m_out)
{
    if (ndt_map_args_error(xyz, row_stride, col_stride, n, cfg, m_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_ndt_map(c, xyz, row_stride, col_stride, n, cfg, key_out, count_out, mean_out, cov_out, axes_out, inv_eig_out, grid_out,
                                   cap, m_out);
    });
}

int symmicp_get_ndt_map(symmicp_ctx *c, uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out, float *axes_out,
                        float *inv_eig_out, int32_t grid_out[6], size_t cap, size_t *m_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!m_out) return fail(c, SYMMICP_ERR_ARG, "get_ndt_map: m_out is required");
    if (!ndt_mode(c) || !c->tgt_block || !c->ndt.map.valid) return fail(c, SYMMICP_ERR_STATE, "get_ndt_map: the context holds no NDT map (SYMMICP_MODE_NDT and symmicp_set_target come first)");
    HIP_TRY(c, hipSetDevice(c->device));
    return ndt_read_map(c, c->ndt.map, "get_ndt_map", key_out, count_out, mean_out, cov_out, axes_out, inv_eig_out, grid_out, cap, m_out);
}

}  // extern "C"
