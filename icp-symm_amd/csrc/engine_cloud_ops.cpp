// engine_cloud_ops.cpp -- the stand-alone cloud operations of libsymmicp: normals and k-NN, radius search, FPFH, ISS keypoints, outlier removal, clustering, region growing, the
// intensity gradient of colored ICP, voxel-grid downsampling.  Each runs on a context the caller owns (symmicp_ctx_*), whose target,
// source, index and certificates stay as they are, or as a one-shot on a context of its own (with_own_context).
#include "engine_internal.h"
#include "orient_core.h"

// Every operation runs on a ScratchIndex (engine_index.cpp): the caller's cloud and a box tree over it behind the target's arrays, given back on every exit.
namespace {
// the tail of every read-back: wait for the stream, then report what a launch on it left behind
int stream_done(symmicp_ctx *c)
{
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return SYMMICP_OK;
}

// the argument check of ISS, outlier removal and clustering: every coordinate of the cloud is finite
bool coords_finite(const float *xyz, size_t xr, size_t xc, size_t n)
{
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(xyz[i * xr + a * xc])) return false;
    return true;
}

// the host compaction of the outlier filters, with the cap protocol of the ISS entry: the count always, the rows (ascending) when they fit
template <class Keep>
int outlier_compact(symmicp_ctx *c, const char *who, size_t n, Keep &&keep, int32_t *rows_out, size_t cap, size_t *count_out)
{
    size_t count = 0;
    for (size_t i = 0; i < n; i++) count += keep(i) ? 1 : 0;
    *count_out = count;
    if (count > cap) return fail(c, SYMMICP_ERR_SIZE, std::string(who) + ": " + std::to_string(count) + " kept rows do not fit cap " + std::to_string(cap));
    size_t at = 0;
    for (size_t i = 0; i < n; i++) if (keep(i)) rows_out[at++] = (int32_t)i;
    return SYMMICP_OK;
}
// the host tail of the clustering and of the region growing, O(n) and sequential by definition.  root [n]: every row's representative, or
// kClusterNoise; a part's representative is a row that is its own root and can_lead (a core row, a seed row).  Parts numbered in ascending
// order of their representative, size = all their rows; then the size filter: the parts that stay, renumbered in the same order; then the cap
// protocol: labels and the count always, the sizes when they fit.
template <class CanLead>
int number_parts(symmicp_ctx *c, const char *who, const char *parts, const char *bad_root, size_t n, const std::vector<uint32_t> &root,
                 CanLead &&can_lead, int32_t lo, int32_t hi, int32_t *labels_out, size_t *count_out, int32_t *sizes_out, size_t cap)
{
    std::vector<int32_t> label(n, -1), size;
    for (size_t i = 0; i < n; i++)
        if (root[i] == (uint32_t)i && can_lead(i)) { label[i] = (int32_t)size.size(); size.push_back(0); }
    for (size_t i = 0; i < n; i++) {
        if (root[i] == kClusterNoise) continue;
        if (root[i] >= n || label[root[i]] < 0) return fail(c, SYMMICP_ERR_HIP, std::string(who) + ": " + bad_root);
        size[(size_t)label[root[i]]]++;
    }
    std::vector<int32_t> renum(size.size(), -1), kept;
    for (size_t k = 0; k < size.size(); k++)
        if ((lo == 0 || size[k] >= lo) && (hi == 0 || size[k] <= hi)) { renum[k] = (int32_t)kept.size(); kept.push_back(size[k]); }
    for (size_t i = 0; i < n; i++) labels_out[i] = root[i] == kClusterNoise ? -1 : renum[(size_t)label[root[i]]];
    *count_out = kept.size();
    if (kept.size() > cap)
        return fail(c, SYMMICP_ERR_SIZE, std::string(who) + ": " + std::to_string(kept.size()) + " " + parts + " do not fit cap " + std::to_string(cap));
    for (size_t k = 0; k < kept.size(); k++) sizes_out[k] = kept[k];
    return SYMMICP_OK;
}
}  // namespace

extern "C" {

// ---- normals pre-step (MyICP::estimateNormals, myicp.cpp:152-172) --------------------------------
// Runs on a context the caller owns (its stream and arenas are reused: a tracker that estimates normals per scan pays no
// context set-up); the context's target and source stay as they are -- what the estimate allocates behind the target's arrays
// in the target's store is released again.
// symmicp_ctx_knn runs the same index build and walk, and reads back the neighbour set (rows, d2) instead of the normals.
static bool normals_args_ok(const float *xyz, size_t n, int k)
{
    return xyz && n != 0 && n <= 0x7fffffffull && k >= 3 && k <= 16 && (size_t)k <= n;
}

static int normals_or_knn(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k,
                          const float viewpoint[3], float *nrm_out, float *curv_out, int32_t *rows_out, float *d2_out)
{
    const bool knn = rows_out != nullptr;
    ScratchIndex si;
    // the cloud has no normals yet: stage xyz twice (the normal slots are ignored)
    if (int st = si.begin(c, xyz, row_stride, col_stride, xyz, row_stride, col_stride, n, n * (knn ? 8 * (size_t)k : 16))) return st;
    // normals: [n][3] + [n]; neighbour set: [n][k] rows + [n][k] d2
    DevBuf<float> b_a, b_b;
    HIP_TRY(c, b_a.alloc_temp(c->arena, (knn ? (size_t)k : 3) * n));
    HIP_TRY(c, b_b.alloc_temp(c->arena, (knn ? (size_t)k : 1) * n));
    if (knn) {
        launch_knn(si.ix, k, (int32_t *)b_a.p, b_b.p, c->stream);
        HIP_TRY(c, hipMemcpyAsync(rows_out, b_a.p, sizeof(int32_t) * (size_t)k * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d2_out, b_b.p, sizeof(float) * (size_t)k * n, hipMemcpyDeviceToHost, c->stream));
    } else {
        const float vp0[3] = {0.f, 0.f, 0.f};
        launch_normals_knn(si.ix, k, viewpoint ? viewpoint : vp0, b_a.p, b_b.p, c->stream);
        HIP_TRY(c, hipMemcpyAsync(nrm_out, b_a.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
        if (curv_out) HIP_TRY(c, hipMemcpyAsync(curv_out, b_b.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    }
    return stream_done(c);
}

int symmicp_ctx_estimate_normals(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k,
                                 const float viewpoint[3], float *nrm_out, float *curv_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!nrm_out || !normals_args_ok(xyz, n, k)) return fail(c, SYMMICP_ERR_ARG, "bad cloud or k (3..16, <= n)");
    return normals_or_knn(c, xyz, row_stride, col_stride, n, k, viewpoint, nrm_out, curv_out, nullptr, nullptr);
}

int symmicp_ctx_knn(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k, int32_t *rows_out, float *d2_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!rows_out || !d2_out || !normals_args_ok(xyz, n, k)) return fail(c, SYMMICP_ERR_ARG, "bad cloud or k (3..16, <= n)");
    return normals_or_knn(c, xyz, row_stride, col_stride, n, k, nullptr, nullptr, nullptr, rows_out, d2_out);
}

int symmicp_estimate_normals(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k,
                             const float viewpoint[3], float *nrm_out, float *curv_out)
{
    if (!nrm_out || !normals_args_ok(xyz, n, k)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_estimate_normals(c, xyz, row_stride, col_stride, n, k, viewpoint, nrm_out, curv_out);
    });
}

// ---- radius search and FPFH features (kernels_fpfh.hip; DESIGN.md 4, "FPFH features and radius search") ------------------
// Both run like the normals pre-step above: a ScratchIndex over the caller's cloud, walked per point.  The context's own clouds, index
// and certificates are not touched.
static const char *radius_args_error(const float *xyz, size_t n, float radius, const int32_t *count_out, const int64_t *offsets_out,
                                     const int32_t *rows_out, const size_t *total_out)
{
    if (!xyz || !count_out || !total_out) return "radius_search: xyz, count_out and total_out are required";
    if (rows_out && !offsets_out) return "radius_search: rows_out needs offsets_out";
    if (n == 0 || n > 0x7fffffffull) return "radius_search: n must be in 1 .. 2^31 - 1";
    if (!std::isfinite(radius) || !(radius > 0.f)) return "radius_search: radius must be finite and > 0";
    return nullptr;
}

static int radius_search(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, size_t n, float radius, int32_t *count_out,
                         int64_t *offsets_out, int32_t *rows_out, float *d2_out, size_t cap, size_t *total_out)
{
    ScratchIndex si;
    if (int st = si.begin(c, xyz, xr, xc, nullptr, 0, 0, n, n * 8 + 8192)) return st;
    const float r2 = radius * radius;
    DevBuf<int32_t> d_count, d_rows;
    DevBuf<uint32_t> d_offs, scan_ws;
    DevBuf<float> d_d2;
    HIP_TRY(c, d_count.alloc_temp(c->arena, n));
    HIP_TRY(c, d_offs.alloc_temp(c->arena, n));
    HIP_TRY(c, scan_ws.alloc_temp(c->arena, n / 2048 + 2));
    launch_radius_count(si.ix, r2, d_count.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(d_offs.p, d_count.p, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, c->stream));
    launch_exclusive_scan(d_offs.p, (uint32_t)n, scan_ws.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(count_out, d_count.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (int st = stream_done(c)) return st;
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) total += (uint64_t)(uint32_t)count_out[i];
    *total_out = (size_t)total;
    if (offsets_out) {
        int64_t at = 0;
        for (size_t i = 0; i < n; i++) { offsets_out[i] = at; at += count_out[i]; }
        offsets_out[n] = at;
    }
    if (!rows_out) return SYMMICP_OK;
    if (total > cap) return fail(c, SYMMICP_ERR_SIZE, "radius_search: " + std::to_string(total) + " neighbours do not fit cap " + std::to_string(cap));
    // the device's offsets are 32-bit words (launch_exclusive_scan)
    if (total > 0xffffffffull) return fail(c, SYMMICP_ERR_SIZE, "radius_search: more than 2^32 - 1 neighbours in all; use a smaller radius or split the cloud");
    if (total == 0) return SYMMICP_OK;
    HIP_TRY(c, d_rows.alloc_temp(c->arena, total));
    if (d2_out) HIP_TRY(c, d_d2.alloc_temp(c->arena, total));
    launch_radius_fill(si.ix, r2, d_offs.p, d_rows.p, d_d2.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(rows_out, d_rows.p, sizeof(int32_t) * total, hipMemcpyDeviceToHost, c->stream));
    if (d2_out) HIP_TRY(c, hipMemcpyAsync(d2_out, d_d2.p, sizeof(float) * total, hipMemcpyDeviceToHost, c->stream));
    return stream_done(c);
}

int symmicp_ctx_radius_search(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, float radius,
                              int32_t *count_out, int64_t *offsets_out, int32_t *rows_out, float *d2_out, size_t cap, size_t *total_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = radius_args_error(xyz, n, radius, count_out, offsets_out, rows_out, total_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    return radius_search(c, xyz, row_stride, col_stride, n, radius, count_out, offsets_out, rows_out, d2_out, cap, total_out);
}

int symmicp_radius_search(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, float radius, int32_t *count_out,
                          int64_t *offsets_out, int32_t *rows_out, float *d2_out, size_t cap, size_t *total_out)
{
    if (radius_args_error(xyz, n, radius, count_out, offsets_out, rows_out, total_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_radius_search(c, xyz, row_stride, col_stride, n, radius, count_out, offsets_out, rows_out, d2_out, cap, total_out);
    });
}

static const char *fpfh_args_error(const float *xyz, const float *nrm, size_t n, float radius, const float *fpfh_out)
{
    if (!xyz || !nrm || !fpfh_out) return "fpfh: xyz, nrm and fpfh_out are required";
    if (n == 0 || n > 0x7fffffffull) return "fpfh: n must be in 1 .. 2^31 - 1";
    if (!std::isfinite(radius) || !(radius > 0.f)) return "fpfh: radius must be finite and > 0";
    return nullptr;
}

int symmicp_ctx_fpfh(symmicp_ctx *c, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm, size_t nrm_row_stride,
                     size_t nrm_col_stride, size_t n, float radius, float *fpfh_out, float *spfh_out, int32_t *count_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = fpfh_args_error(xyz, nrm, n, radius, fpfh_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    ScratchIndex si;
    if (int st = si.begin(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, n * (36 + 33 + 33 + 1) * 4 + 8192)) return st;
    const float r2 = radius * radius;
    DevBuf<float> d_sorted, d_spfh, d_fpfh;
    DevBuf<int32_t> d_count;
    HIP_TRY(c, d_sorted.alloc_temp(c->arena, n * 36));
    HIP_TRY(c, d_fpfh.alloc_temp(c->arena, n * 33));
    HIP_TRY(c, d_count.alloc_temp(c->arena, n));
    if (spfh_out) HIP_TRY(c, d_spfh.alloc_temp(c->arena, n * 33));
    launch_spfh(si.ix, r2, d_sorted.p, d_spfh.p, d_count.p, c->stream);
    launch_fpfh(si.ix, r2, d_sorted.p, d_fpfh.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(fpfh_out, d_fpfh.p, sizeof(float) * 33 * n, hipMemcpyDeviceToHost, c->stream));
    if (spfh_out) HIP_TRY(c, hipMemcpyAsync(spfh_out, d_spfh.p, sizeof(float) * 33 * n, hipMemcpyDeviceToHost, c->stream));
    if (count_out) HIP_TRY(c, hipMemcpyAsync(count_out, d_count.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    return stream_done(c);
}

int symmicp_fpfh(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm, size_t nrm_row_stride,
                 size_t nrm_col_stride, size_t n, float radius, float *fpfh_out, float *spfh_out, int32_t *count_out)
{
    if (fpfh_args_error(xyz, nrm, n, radius, fpfh_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_fpfh(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, radius, fpfh_out, spfh_out, count_out);
    });
}

// ---- ISS keypoints (kernels_keypoints.hip; DESIGN.md 4, "ISS keypoints") ---------------------------------------------------
// Like the FPFH entry above: the cloud's own scratch index, the radius walk twice (saliency at the salient radius, non-maximum
// suppression at the other), then the flags scanned over rows and the kept rows scattered in ascending order.
static const char *iss_args_error(const float *xyz, size_t xr, size_t xc, size_t n, const symmicp_iss_config *cfg, const int32_t *rows_out, size_t cap,
                                  const size_t *count_out)
{
    if (!xyz || !cfg || !count_out) return "iss_keypoints: xyz, cfg and count_out are required";
    if (!rows_out && cap > 0) return "iss_keypoints: rows_out is required when cap > 0";
    if (n == 0 || n > 0x7fffffffull) return "iss_keypoints: n must be in 1 .. 2^31 - 1";
    if (cfg->struct_size != sizeof(symmicp_iss_config)) return "iss_keypoints: cfg->struct_size is not sizeof(symmicp_iss_config)";
    if (!std::isfinite(cfg->salient_radius) || !(cfg->salient_radius > 0.f)) return "iss_keypoints: salient_radius must be finite and > 0";
    if (!std::isfinite(cfg->non_max_radius) || !(cfg->non_max_radius > 0.f)) return "iss_keypoints: non_max_radius must be finite and > 0";
    if (!(cfg->gamma21 > 0.f) || !(cfg->gamma21 <= 1.f)) return "iss_keypoints: gamma21 must be in (0, 1]";
    if (!(cfg->gamma32 > 0.f) || !(cfg->gamma32 <= 1.f)) return "iss_keypoints: gamma32 must be in (0, 1]";
    if (cfg->min_neighbors < 1) return "iss_keypoints: min_neighbors must be >= 1";
    if (!coords_finite(xyz, xr, xc, n)) return "iss_keypoints: a coordinate is not finite";
    return nullptr;
}

void symmicp_iss_config_default(symmicp_iss_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->gamma21 = 0.975f;
    cfg->gamma32 = 0.975f;
    cfg->min_neighbors = 5;
}

int symmicp_ctx_iss_keypoints(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_iss_config *cfg,
                              int32_t *rows_out, size_t cap, size_t *count_out, float *saliency_out, int32_t *neighbors_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = iss_args_error(xyz, row_stride, col_stride, n, cfg, rows_out, cap, count_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    ScratchIndex si;
    if (int st = si.begin(c, xyz, row_stride, col_stride, nullptr, 0, 0, n, n * 6 * 4 + 16384)) return st;
    const float rs2 = cfg->salient_radius * cfg->salient_radius, rn2 = cfg->non_max_radius * cfg->non_max_radius;
    DevBuf<float> d_sorted, d_srows;
    DevBuf<int32_t> d_k, d_rows;
    DevBuf<uint32_t> d_flag, d_pos, scan_ws;
    HIP_TRY(c, d_sorted.alloc_temp(c->arena, n));
    HIP_TRY(c, d_srows.alloc_temp(c->arena, n));
    HIP_TRY(c, d_k.alloc_temp(c->arena, n));
    HIP_TRY(c, d_flag.alloc_temp(c->arena, n));
    HIP_TRY(c, d_pos.alloc_temp(c->arena, n));
    HIP_TRY(c, scan_ws.alloc_temp(c->arena, n / 2048 + 2));
    launch_iss_saliency(si.ix, rs2, cfg->min_neighbors, cfg->gamma21, cfg->gamma32, d_sorted.p, d_srows.p, d_k.p, c->stream);
    launch_iss_nms(si.ix, rn2, cfg->min_neighbors, d_sorted.p, d_flag.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(d_pos.p, d_flag.p, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, c->stream));
    launch_exclusive_scan(d_pos.p, (uint32_t)n, scan_ws.p, c->stream);
    uint32_t last_pos = 0, last_flag = 0;
    HIP_TRY(c, hipMemcpyAsync(&last_pos, d_pos.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&last_flag, d_flag.p + (n - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    if (saliency_out) HIP_TRY(c, hipMemcpyAsync(saliency_out, d_srows.p, sizeof(float) * n, hipMemcpyDeviceToHost, c->stream));
    if (neighbors_out) HIP_TRY(c, hipMemcpyAsync(neighbors_out, d_k.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    if (int st = stream_done(c)) return st;
    const size_t count = (size_t)last_pos + last_flag;
    *count_out = count;
    if (count > cap) return fail(c, SYMMICP_ERR_SIZE, "iss_keypoints: " + std::to_string(count) + " keypoints do not fit cap " + std::to_string(cap));
    if (count == 0) return SYMMICP_OK;
    HIP_TRY(c, d_rows.alloc_temp(c->arena, count));
    launch_iss_scatter(d_flag.p, d_pos.p, (uint32_t)n, d_rows.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(rows_out, d_rows.p, sizeof(int32_t) * count, hipMemcpyDeviceToHost, c->stream));
    return stream_done(c);
}

int symmicp_iss_keypoints(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_iss_config *cfg,
                          int32_t *rows_out, size_t cap, size_t *count_out, float *saliency_out, int32_t *neighbors_out)
{
    if (iss_args_error(xyz, row_stride, col_stride, n, cfg, rows_out, cap, count_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_iss_keypoints(c, xyz, row_stride, col_stride, n, cfg, rows_out, cap, count_out, saliency_out, neighbors_out);
    });
}

// ---- statistical and radius outlier removal (kernels_outlier.hip, kernels_fpfh.hip; DESIGN.md 4, "Outlier removal") -------------------
// Like the ISS entry above: the cloud's own scratch index and one walk per point (the k-NN mean distance, or the radius count of the
// radius search).  The per-point values are read back; the statistics and the compaction are O(n), sequential by definition, and
// run on the host.
static const char *outlier_args_error(const float *xyz, size_t xr, size_t xc, size_t n, const int32_t *rows_out, size_t cap,
                                      const size_t *count_out)
{
    if (!xyz || !count_out) return "outlier removal: xyz and count_out are required";
    if (!rows_out && cap > 0) return "outlier removal: rows_out is required when cap > 0";
    if (n == 0 || n > 0x7fffffffull) return "outlier removal: n must be in 1 .. 2^31 - 1";
    if (!coords_finite(xyz, xr, xc, n)) return "outlier removal: a coordinate is not finite";
    return nullptr;
}

static const char *sor_args_error(const float *xyz, size_t xr, size_t xc, size_t n, int k, float std_mul, const int32_t *rows_out, size_t cap,
                                  const size_t *count_out)
{
    if (!xyz || !count_out) return "statistical_outlier_removal: xyz and count_out are required";
    if (n == 0 || n > 0x7fffffffull) return "statistical_outlier_removal: n must be in 1 .. 2^31 - 1";
    if (k < 1 || k > 64 || (size_t)k > n - 1) return "statistical_outlier_removal: k must be in 1 .. 64 and <= n - 1";
    if (!std::isfinite(std_mul)) return "statistical_outlier_removal: std_mul must be finite";
    return outlier_args_error(xyz, xr, xc, n, rows_out, cap, count_out);
}

static const char *ror_args_error(const float *xyz, size_t xr, size_t xc, size_t n, float radius, int min_neighbors, const int32_t *rows_out,
                                  size_t cap, const size_t *count_out)
{
    if (!xyz || !count_out) return "radius_outlier_removal: xyz and count_out are required";
    if (n == 0 || n > 0x7fffffffull) return "radius_outlier_removal: n must be in 1 .. 2^31 - 1";
    if (!std::isfinite(radius) || !(radius > 0.f)) return "radius_outlier_removal: radius must be finite and > 0";
    if (min_neighbors < 1) return "radius_outlier_removal: min_neighbors must be >= 1";
    return outlier_args_error(xyz, xr, xc, n, rows_out, cap, count_out);
}

int symmicp_ctx_statistical_outlier_removal(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k, float std_mul,
                                            int32_t *rows_out, size_t cap, size_t *count_out, double *mean_dist_out, double stats_out[3])
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = sor_args_error(xyz, row_stride, col_stride, n, k, std_mul, rows_out, cap, count_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<double> own;
    double *m = mean_dist_out;
    {
        ScratchIndex si;
        if (int st = si.begin(c, xyz, row_stride, col_stride, nullptr, 0, 0, n, n * 8 + 8192)) return st;
        DevBuf<double> d_mean;
        HIP_TRY(c, d_mean.alloc_temp(c->arena, n));
        launch_knn_mean_dist(si.ix, k, d_mean.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (!m) { own.resize(n); m = own.data(); }
        HIP_TRY(c, hipMemcpyAsync(m, d_mean.p, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
        if (int st = stream_done(c)) return st;
    }
    // PCL's formula, sequentially in row order (this file is built with -ffp-contract=off: nothing here is fused)
    double s1 = 0.0, s2 = 0.0;
    for (size_t i = 0; i < n; i++) { s1 = s1 + m[i]; s2 = s2 + m[i] * m[i]; }
    const double dn = (double)n;
    const double mu = s1 / dn;
    const double var = (s2 - s1 * s1 / dn) / (dn - 1.0);
    const double sd = std::sqrt(var < 0.0 ? 0.0 : var);      // (a NaN variance stays NaN: the threshold then keeps nothing)
    const double thr = mu + (double)std_mul * sd;
    if (stats_out) { stats_out[0] = mu; stats_out[1] = sd; stats_out[2] = thr; }
    return outlier_compact(c, "statistical_outlier_removal", n, [&](size_t i) { return m[i] <= thr; }, rows_out, cap, count_out);
}

int symmicp_statistical_outlier_removal(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k, float std_mul,
                                        int32_t *rows_out, size_t cap, size_t *count_out, double *mean_dist_out, double stats_out[3])
{
    if (sor_args_error(xyz, row_stride, col_stride, n, k, std_mul, rows_out, cap, count_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_statistical_outlier_removal(c, xyz, row_stride, col_stride, n, k, std_mul, rows_out, cap, count_out, mean_dist_out,
                                                       stats_out);
    });
}

int symmicp_ctx_radius_outlier_removal(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, float radius,
                                       int min_neighbors, int32_t *rows_out, size_t cap, size_t *count_out, int32_t *neighbors_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = ror_args_error(xyz, row_stride, col_stride, n, radius, min_neighbors, rows_out, cap, count_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<int32_t> own;
    int32_t *nb = neighbors_out;
    {
        ScratchIndex si;
        if (int st = si.begin(c, xyz, row_stride, col_stride, nullptr, 0, 0, n, n * 4 + 8192)) return st;
        DevBuf<int32_t> d_count;
        HIP_TRY(c, d_count.alloc_temp(c->arena, n));
        launch_radius_count(si.ix, radius * radius, d_count.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (!nb) { own.resize(n); nb = own.data(); }
        HIP_TRY(c, hipMemcpyAsync(nb, d_count.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (int st = stream_done(c)) return st;
    }
    return outlier_compact(c, "radius_outlier_removal", n, [&](size_t i) { return nb[i] >= min_neighbors; }, rows_out, cap, count_out);
}

int symmicp_radius_outlier_removal(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, float radius, int min_neighbors,
                                   int32_t *rows_out, size_t cap, size_t *count_out, int32_t *neighbors_out)
{
    if (ror_args_error(xyz, row_stride, col_stride, n, radius, min_neighbors, rows_out, cap, count_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_radius_outlier_removal(c, xyz, row_stride, col_stride, n, radius, min_neighbors, rows_out, cap, count_out, neighbors_out);
    });
}

// ---- DBSCAN / Euclidean cluster extraction (kernels_cluster.hip, kernels_fpfh.hip; DESIGN.md 4, "Clustering") -------------------------
// Like the radius filter above: the cloud's own scratch index, the count pass of the radius search (the core test), then the union-find
// over the implicit radius graph and the border pass.  The per-row representative is read back; the dense numbering, the sizes and the
// size filter are O(n), sequential by definition, and run on the host (number_parts).
static const char *cluster_args_error(const float *xyz, size_t xr, size_t xc, size_t n, const symmicp_cluster_config *cfg, const int32_t *labels_out,
                                      const size_t *clusters_out, const int32_t *sizes_out, size_t cap)
{
    if (!xyz || !cfg || !labels_out || !clusters_out) return "cluster: xyz, cfg, labels_out and clusters_out are required";
    if (!sizes_out && cap > 0) return "cluster: sizes_out is required when cap > 0";
    if (n == 0 || n > 0x7fffffffull) return "cluster: n must be in 1 .. 2^31 - 1";
    if (cfg->struct_size != sizeof(symmicp_cluster_config)) return "cluster: cfg->struct_size is not sizeof(symmicp_cluster_config)";
    if (!std::isfinite(cfg->eps) || !(cfg->eps > 0.f)) return "cluster: eps must be finite and > 0";
    if (cfg->min_points < 1) return "cluster: min_points must be >= 1";
    if (cfg->min_cluster_size < 0 || cfg->max_cluster_size < 0) return "cluster: min_cluster_size and max_cluster_size must be >= 0";
    if (cfg->min_cluster_size > 0 && cfg->max_cluster_size > 0 && cfg->max_cluster_size < cfg->min_cluster_size)
        return "cluster: max_cluster_size is below min_cluster_size";
    if (!coords_finite(xyz, xr, xc, n)) return "cluster: a coordinate is not finite";
    return nullptr;
}

void symmicp_cluster_config_default(symmicp_cluster_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->min_points = 1;
}

int symmicp_ctx_cluster(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_cluster_config *cfg,
                        int32_t *labels_out, size_t *clusters_out, int32_t *sizes_out, size_t cap, uint8_t *core_out, int32_t *neighbors_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = cluster_args_error(xyz, row_stride, col_stride, n, cfg, labels_out, clusters_out, sizes_out, cap)) return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<int32_t> own;
    std::vector<uint32_t> root(n);
    int32_t *nb = neighbors_out;
    const int32_t need = cfg->min_points - 1;
    {
        ScratchIndex si;
        if (int st = si.begin(c, xyz, row_stride, col_stride, nullptr, 0, 0, n, n * 8 + 8192)) return st;
        DevBuf<int32_t> d_count;
        DevBuf<uint32_t> d_parent;
        DevBuf<unsigned long long> d_stats;
        HIP_TRY(c, d_count.alloc_temp(c->arena, n));
        HIP_TRY(c, d_parent.alloc_temp(c->arena, n));
        if (c->sw.debug_counters) {
            HIP_TRY(c, d_stats.alloc_temp(c->arena, 2));
            HIP_TRY(c, hipMemsetAsync(d_stats.p, 0, 2 * sizeof(unsigned long long), c->stream));
        }
        const float r2 = cfg->eps * cfg->eps;
        launch_radius_count(si.ix, r2, d_count.p, c->stream);
        launch_cluster_roots(si.ix, r2, d_count.p, cfg->min_points, d_parent.p, d_stats.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (!nb) { own.resize(n); nb = own.data(); }
        unsigned long long stats[2] = {0, 0};
        HIP_TRY(c, hipMemcpyAsync(nb, d_count.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(root.data(), d_parent.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (d_stats.p) HIP_TRY(c, hipMemcpyAsync(stats, d_stats.p, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
        if (int st = stream_done(c)) return st;
        if (d_stats.p) std::fprintf(stderr, "symmicp cluster: n %zu, %llu unions, %llu lost compare-and-swaps\n", n, stats[0], stats[1]);
    }
    if (core_out) for (size_t i = 0; i < n; i++) core_out[i] = nb[i] >= need ? 1 : 0;
    return number_parts(c, "cluster", "clusters", "a row's representative is not a cluster's lowest core row", n, root,
                        [&](size_t i) { return nb[i] >= need; }, cfg->min_cluster_size, cfg->max_cluster_size, labels_out, clusters_out, sizes_out, cap);
}

int symmicp_cluster(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_cluster_config *cfg,
                    int32_t *labels_out, size_t *clusters_out, int32_t *sizes_out, size_t cap, uint8_t *core_out, int32_t *neighbors_out)
{
    if (cluster_args_error(xyz, row_stride, col_stride, n, cfg, labels_out, clusters_out, sizes_out, cap)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_cluster(c, xyz, row_stride, col_stride, n, cfg, labels_out, clusters_out, sizes_out, cap, core_out, neighbors_out);
    });
}

// ---- region-growing segmentation (kernels_region.hip; DESIGN.md 4, "Region growing") ---------------------------------------------------
// Like the clustering above with the normals sorted next to the points (ScratchIndex::begin takes them): seed flags from the curvature, the
// union-find over the implicit smooth graph on the seeds, the border pass over the rest, and the clustering's host tail.  The count of
// smooth neighbours is one more walk, launched only when smooth_out is given.
static const char *region_args_error(const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, const float *curv, size_t cs,
                                     size_t n, const symmicp_region_config *cfg, const int32_t *labels_out, const size_t *regions_out,
                                     const int32_t *sizes_out, size_t cap)
{
    if (!xyz || !nrm || !cfg || !labels_out || !regions_out) return "region_growing: xyz, nrm, cfg, labels_out and regions_out are required";
    if (!sizes_out && cap > 0) return "region_growing: sizes_out is required when cap > 0";
    if (n == 0 || n > 0x7fffffffull) return "region_growing: n must be in 1 .. 2^31 - 1";
    if (cfg->struct_size != sizeof(symmicp_region_config)) return "region_growing: cfg->struct_size is not sizeof(symmicp_region_config)";
    if (!std::isfinite(cfg->eps) || !(cfg->eps > 0.f)) return "region_growing: eps must be finite and > 0";
    if (!std::isfinite(cfg->smoothness_cos) || !(cfg->smoothness_cos >= 0.f) || !(cfg->smoothness_cos <= 1.f))
        return "region_growing: smoothness_cos must be in [0, 1]";
    if (std::isnan(cfg->curvature_threshold)) return "region_growing: curvature_threshold is NaN";
    if (cfg->min_region_size < 0 || cfg->max_region_size < 0) return "region_growing: min_region_size and max_region_size must be >= 0";
    if (cfg->min_region_size > 0 && cfg->max_region_size > 0 && cfg->max_region_size < cfg->min_region_size)
        return "region_growing: max_region_size is below min_region_size";
    if (!coords_finite(xyz, xr, xc, n)) return "region_growing: a coordinate is not finite";
    if (!coords_finite(nrm, nr, nc, n)) return "region_growing: a normal is not finite";
    if (curv)
        for (size_t i = 0; i < n; i++)
            if (std::isnan(curv[i * cs])) return "region_growing: a curvature is NaN";
    return nullptr;
}

void symmicp_region_config_default(symmicp_region_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->smoothness_cos = 0.8660254f;
    cfg->curvature_threshold = 0.05f;
}

int symmicp_ctx_region_growing(symmicp_ctx *c, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm, size_t nrm_row_stride,
                               size_t nrm_col_stride, const float *curv, size_t curv_stride, size_t n, const symmicp_region_config *cfg,
                               int32_t *labels_out, size_t *regions_out, int32_t *sizes_out, size_t cap, uint8_t *seed_out, int32_t *smooth_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = region_args_error(xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, curv, curv_stride, n, cfg,
                                            labels_out, regions_out, sizes_out, cap))
        return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<uint32_t> root(n);
    std::vector<int32_t> seed(n);
    std::vector<float> curv_rows;
    if (curv) {
        curv_rows.resize(n);
        for (size_t i = 0; i < n; i++) curv_rows[i] = curv[i * curv_stride];
    }
    {
        ScratchIndex si;
        if (int st = si.begin(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, n * 16 + 8192)) return st;
        DevBuf<int32_t> d_seed, d_smooth;
        DevBuf<uint32_t> d_parent;
        DevBuf<float> d_curv;
        DevBuf<unsigned long long> d_stats;
        HIP_TRY(c, d_seed.alloc_temp(c->arena, n));
        HIP_TRY(c, d_parent.alloc_temp(c->arena, n));
        if (curv) {
            HIP_TRY(c, d_curv.alloc_temp(c->arena, n));
            HIP_TRY(c, hipMemcpyAsync(d_curv.p, curv_rows.data(), sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
        }
        if (smooth_out) HIP_TRY(c, d_smooth.alloc_temp(c->arena, n));
        if (c->sw.debug_counters) {
            HIP_TRY(c, d_stats.alloc_temp(c->arena, 4));
            HIP_TRY(c, hipMemsetAsync(d_stats.p, 0, 4 * sizeof(unsigned long long), c->stream));
        }
        const float r2 = cfg->eps * cfg->eps;
        launch_region_seeds(d_curv.p, cfg->curvature_threshold, (uint32_t)n, d_seed.p, c->stream);
        launch_region_roots(si.ix, r2, cfg->smoothness_cos, d_seed.p, curv != nullptr, d_parent.p, d_stats.p, c->stream);
        if (smooth_out) launch_region_smooth_count(si.ix, r2, cfg->smoothness_cos, d_smooth.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        unsigned long long stats[4] = {0, 0, 0, 0};
        HIP_TRY(c, hipMemcpyAsync(seed.data(), d_seed.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(root.data(), d_parent.p, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (smooth_out) HIP_TRY(c, hipMemcpyAsync(smooth_out, d_smooth.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        if (d_stats.p) HIP_TRY(c, hipMemcpyAsync(stats, d_stats.p, sizeof(stats), hipMemcpyDeviceToHost, c->stream));
        if (int st = stream_done(c)) return st;
        if (d_stats.p)
            std::fprintf(stderr, "symmicp region_growing: n %zu, %llu unions, %llu lost compare-and-swaps, %llu edges examined, %llu normal loads\n", n,
                         stats[0], stats[1], stats[2], stats[3]);
    }
    if (seed_out) for (size_t i = 0; i < n; i++) seed_out[i] = seed[i] ? 1 : 0;
    return number_parts(c, "region_growing", "regions", "a row's representative is not a region's lowest seed row", n, root,
                        [&](size_t i) { return seed[i] != 0; }, cfg->min_region_size, cfg->max_region_size, labels_out, regions_out, sizes_out, cap);
}

int symmicp_region_growing(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm, size_t nrm_row_stride,
                           size_t nrm_col_stride, const float *curv, size_t curv_stride, size_t n, const symmicp_region_config *cfg,
                           int32_t *labels_out, size_t *regions_out, int32_t *sizes_out, size_t cap, uint8_t *seed_out, int32_t *smooth_out)
{
    if (region_args_error(xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, curv, curv_stride, n, cfg, labels_out, regions_out,
                          sizes_out, cap))
        return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_region_growing(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, curv, curv_stride, n, cfg,
                                          labels_out, regions_out, sizes_out, cap, seed_out, smooth_out);
    });
}

// ---- consistent normal orientation (kernels_orient.hip, orient_core.h; DESIGN.md 4, "Normal orientation") ----------------------------
// Like the intensity gradient below: the cloud's own scratch index and the exact k-NN walk (launch_knn), then Boruvka rounds over those
// lists.  The host reads one word per round (the hooks so far) and stops at a round without any; the counts of the result are O(n) over
// the read-back flags and components, on the host.
static const char *orient_args_error(const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n,
                                     const symmicp_orient_config *cfg, const float *nrm_out, const int32_t *tree_out, const size_t *tree_count)
{
    if (!xyz || !nrm || !cfg || !nrm_out) return "orient_normals: xyz, nrm, cfg and nrm_out are required";
    if (tree_out && !tree_count) return "orient_normals: tree_out needs tree_count";
    if (n == 0 || n > 0x7fffffffull) return "orient_normals: n must be in 1 .. 2^31 - 1";
    if (cfg->struct_size != sizeof(symmicp_orient_config)) return "orient_normals: cfg->struct_size is not sizeof(symmicp_orient_config)";
    if (cfg->k < 3 || cfg->k > 16 || (size_t)cfg->k > n) return "orient_normals: k must be in 3 .. 16 and <= n";
    if (cfg->seed_rule != SYMMICP_ORIENT_VIEWPOINT && cfg->seed_rule != SYMMICP_ORIENT_DIRECTION) return "orient_normals: unknown seed_rule";
    if (!std::isfinite(cfg->ref[0]) || !std::isfinite(cfg->ref[1]) || !std::isfinite(cfg->ref[2])) return "orient_normals: ref is not finite";
    if (cfg->seed_rule == SYMMICP_ORIENT_DIRECTION && cfg->ref[0] == 0.f && cfg->ref[1] == 0.f && cfg->ref[2] == 0.f)
        return "orient_normals: the direction is zero";
    if (!coords_finite(xyz, xr, xc, n)) return "orient_normals: a coordinate is not finite";
    if (!coords_finite(nrm, nr, nc, n)) return "orient_normals: a normal is not finite";
    return nullptr;
}

void symmicp_orient_config_default(symmicp_orient_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->k = 16;      // (the cat of tests/golden is one component at 16 and four at 10)
    cfg->seed_rule = SYMMICP_ORIENT_VIEWPOINT;
}

int symmicp_ctx_orient_normals(symmicp_ctx *c, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                               size_t nrm_row_stride, size_t nrm_col_stride, size_t n, const symmicp_orient_config *cfg, float *nrm_out,
                               uint8_t *flip_out, int32_t *component_out, int32_t *tree_out, size_t *tree_count, symmicp_orient_result *result)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = orient_args_error(xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, cfg, nrm_out, tree_out,
                                            tree_count))
        return fail(c, SYMMICP_ERR_ARG, msg);
    if (tree_count) *tree_count = 0;
    const int k = cfg->k;
    const uint32_t n32 = (uint32_t)n;
    // both clouds packed by row: the kernels gather normals by the rows the neighbour lists name
    std::vector<float> rows(6 * n);
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) {
            rows[3 * i + a] = xyz[i * xyz_row_stride + a * xyz_col_stride];
            rows[3 * n + 3 * i + a] = nrm[i * nrm_row_stride + a * nrm_col_stride];
        }
    std::vector<uint8_t> flip(n);
    std::vector<int32_t> comp(n);
    unsigned long long graph_edges = 0;
    uint32_t hooked = 0;
    int rounds = 0;
    {
        ScratchIndex si;
        if (int st = si.begin(c, xyz, xyz_row_stride, xyz_col_stride, nullptr, 0, 0, n, n * (16 * (size_t)k + 96) + 65536)) return st;
        DevBuf<int32_t> d_knn, d_tree, d_comp;
        DevBuf<float> d_d2, d_rows, d_out;
        DevBuf<uint32_t> d_erow, d_eww, d_words, d_mid, d_hi, d_small;
        DevBuf<unsigned long long> d_best;
        DevBuf<uint8_t> d_flip;
        HIP_TRY(c, d_best.alloc_temp(c->arena, n + 1));      // [n] the slots, [n] the edge count
        HIP_TRY(c, d_knn.alloc_temp(c->arena, n * (size_t)k));
        HIP_TRY(c, d_d2.alloc_temp(c->arena, n * (size_t)k));
        HIP_TRY(c, d_erow.alloc_temp(c->arena, n * (size_t)k));
        HIP_TRY(c, d_eww.alloc_temp(c->arena, n * (size_t)k));
        HIP_TRY(c, d_rows.alloc_temp(c->arena, 6 * n));
        HIP_TRY(c, d_out.alloc_temp(c->arena, 3 * n));
        HIP_TRY(c, d_words.alloc_temp(c->arena, n));
        HIP_TRY(c, d_mid.alloc_temp(c->arena, n));
        HIP_TRY(c, d_hi.alloc_temp(c->arena, n));
        HIP_TRY(c, d_tree.alloc_temp(c->arena, 2 * n));
        HIP_TRY(c, d_comp.alloc_temp(c->arena, n));
        HIP_TRY(c, d_small.alloc_temp(c->arena, 2));         // [0] the hooks so far, [1] the walk guard
        HIP_TRY(c, d_flip.alloc_temp(c->arena, n));
        const float *d_xyz = d_rows.p, *d_nrm = d_rows.p + 3 * n;
        unsigned long long *d_edges = d_best.p + n;
        HIP_TRY(c, hipMemcpyAsync(d_rows.p, rows.data(), sizeof(float) * 6 * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemsetAsync(d_edges, 0, sizeof(unsigned long long), c->stream));
        HIP_TRY(c, hipMemsetAsync(d_small.p, 0, 2 * sizeof(uint32_t), c->stream));
        launch_knn(si.ix, k, d_knn.p, d_d2.p, c->stream);
        launch_orient_edges(d_knn.p, d_nrm, n32, k, d_erow.p, d_eww.p, d_edges, d_words.p, c->stream);
        for (int round = 0;; round++) {
            if (round > symmicp::orient::kMaxRounds) return fail(c, SYMMICP_ERR_INTERNAL, "orient_normals: more than 32 rounds");
            launch_orient_round(d_erow.p, d_eww.p, d_words.p, d_mid.p, n32, k, d_best.p, d_hi.p, d_nrm, d_tree.p, d_small.p, c->stream);
            uint32_t state[2] = {0, 0};
            HIP_TRY(c, hipMemcpyAsync(state, d_small.p, sizeof(state), hipMemcpyDeviceToHost, c->stream));
            if (int st = stream_done(c)) return st;
            if (state[1]) return fail(c, SYMMICP_ERR_INTERNAL, "orient_normals: a walk up the parents exceeded the hooks of its round");
            if (state[0] >= n32) return fail(c, SYMMICP_ERR_INTERNAL, "orient_normals: more tree edges than a forest has");
            const uint32_t hooks = state[0] - hooked;
            hooked = state[0];
            if (hooks == 0) break;
            rounds++;
            launch_orient_flatten(d_mid.p, d_words.p, n32, hooks + 1, d_small.p + 1, c->stream);
        }
        // the slots of the rounds are free now: min_row <- d_hi, seed_key <- d_best, root_flip <- d_mid
        launch_orient_finish(d_words.p, d_xyz, d_nrm, n32, cfg->seed_rule, cfg->ref, d_hi.p, d_best.p, d_mid.p, d_out.p, d_flip.p, d_comp.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(nrm_out, d_out.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(flip.data(), d_flip.p, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(comp.data(), d_comp.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&graph_edges, d_edges, sizeof(graph_edges), hipMemcpyDeviceToHost, c->stream));
        if (tree_out && hooked) HIP_TRY(c, hipMemcpyAsync(tree_out, d_tree.p, sizeof(int32_t) * 2 * hooked, hipMemcpyDeviceToHost, c->stream));
        if (int st = stream_done(c)) return st;
    }
    if (tree_count) *tree_count = hooked;
    std::vector<uint32_t> size(n, 0);
    uint64_t components = 0, largest = 0, flipped = 0;
    for (size_t i = 0; i < n; i++) {
        if (comp[i] < 0 || (size_t)comp[i] > i) return fail(c, SYMMICP_ERR_INTERNAL, "orient_normals: a row's component is not its lowest row");
        components += (size_t)comp[i] == i ? 1 : 0;
        const uint64_t s = ++size[(size_t)comp[i]];
        largest = s > largest ? s : largest;
        flipped += flip[i];
    }
    if (components + hooked != n) return fail(c, SYMMICP_ERR_INTERNAL, "orient_normals: tree edges and components do not add up to n");
    if (flip_out) std::memcpy(flip_out, flip.data(), n);
    if (component_out) std::memcpy(component_out, comp.data(), sizeof(int32_t) * n);
    if (result) {
        std::memset(result, 0, sizeof(*result));
        result->graph_edges = graph_edges;
        result->tree_edges = hooked;
        result->components = components;
        result->largest_component = largest;
        result->flipped = flipped;
        result->rounds = rounds;
    }
    return SYMMICP_OK;
}

int symmicp_orient_normals(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm, size_t nrm_row_stride,
                           size_t nrm_col_stride, size_t n, const symmicp_orient_config *cfg, float *nrm_out, uint8_t *flip_out,
                           int32_t *component_out, int32_t *tree_out, size_t *tree_count, symmicp_orient_result *result)
{
    if (orient_args_error(xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, cfg, nrm_out, tree_out, tree_count))
        return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_orient_normals(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, cfg, nrm_out, flip_out,
                                          component_out, tree_out, tree_count, result);
    });
}

// ---- intensity gradient of colored ICP (kernels_color.hip; DESIGN.md 4, "Colored ICP") ------------------------------------
// Like the FPFH entry above: the cloud's own scratch index, the exact k-NN walk of the normals pre-step (launch_knn: rows in (d2, row) order),
// then the tangent-plane moments and the 3x3 solve per point.
static const char *gradient_args_error(const float *xyz, const float *nrm, const float *intensity, size_t n, int k, const float *grad_out)
{
    if (!xyz || !nrm || !intensity || !grad_out) return "intensity gradient: xyz, nrm, intensity and grad_out are required";
    if (n == 0 || n > 0x7fffffffull) return "intensity gradient: n must be in 1 .. 2^31 - 1";
    if (k < 3 || k > 16 || (size_t)k > n) return "intensity gradient: k must be in 3 .. 16 and <= n";
    return nullptr;
}

int symmicp_ctx_intensity_gradient(symmicp_ctx *c, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                                   size_t nrm_row_stride, size_t nrm_col_stride, const float *intensity, size_t intensity_stride, size_t n,
                                   int k, float *grad_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = gradient_args_error(xyz, nrm, intensity, n, k, grad_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<float> hi(n);
    for (size_t i = 0; i < n; i++) hi[i] = intensity[i * intensity_stride];
    ScratchIndex si;
    if (int st = si.begin(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n,
                        n * (8 * (size_t)k + 4 + 16 + 12) + 8192)) return st;
    DevBuf<int32_t> d_rows;
    DevBuf<float> d_d2, d_int, d_grad;
    DevBuf<float4> d_rec;
    HIP_TRY(c, d_rows.alloc_temp(c->arena, n * (size_t)k));
    HIP_TRY(c, d_d2.alloc_temp(c->arena, n * (size_t)k));
    HIP_TRY(c, d_int.alloc_temp(c->arena, n));
    HIP_TRY(c, d_rec.alloc_temp(c->arena, n));
    HIP_TRY(c, d_grad.alloc_temp(c->arena, 3 * n));
    HIP_TRY(c, hipMemcpyAsync(d_int.p, hi.data(), sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    launch_knn(si.ix, k, d_rows.p, d_d2.p, c->stream);
    launch_color_gradient(si.ix, d_int.p, d_rows.p, k, d_rec.p, d_grad.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(grad_out, d_grad.p, sizeof(float) * 3 * n, hipMemcpyDeviceToHost, c->stream));
    return stream_done(c);
}

int symmicp_intensity_gradient(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                               size_t nrm_row_stride, size_t nrm_col_stride, const float *intensity, size_t intensity_stride, size_t n,
                               int k, float *grad_out)
{
    if (gradient_args_error(xyz, nrm, intensity, n, k, grad_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_intensity_gradient(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, intensity, intensity_stride,
                                              n, k, grad_out);
    });
}

// ---- voxel-grid downsampling (kernels_voxel.hip; DESIGN.md 4, "Voxel downsampling") ---------------------------------------
// Box (launch_bbox) -> grid set-up here in fp32 -> keys -> stable radix sort of (key, row) -> run heads, scan, first positions ->
// kept voxels (>= min_points), scan, compaction -> sorted SoA gather -> per-voxel sequential means.  Temporaries come from the
// context's arena only: its target, source, index and certificates are not touched.
static int voxel_downsample(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n,
                            float leaf, int min_points, float *xyz_out, float *nrm_out, int32_t *count_out, int32_t *voxel_of, size_t cap,
                            size_t *n_out)
{
    HIP_TRY(c, hipSetDevice(c->device));
    const bool with_nrm = nrm_out != nullptr;
    arena_begin(c->arena, n * (128 + 4 * (xr + (with_nrm ? nr : 0))) + ((size_t)1 << 20));
    const uint32_t n32 = (uint32_t)n;
    DevBuf<float> block;
    int st = upload_planar(c, xyz, xr, xc, with_nrm ? nrm : nullptr, nr, nc, n, block, /*store=*/nullptr, nullptr);
    if (st != SYMMICP_OK) return st;
    CloudSoA cl;
    soa_from_block(block.p, n, cl);

    DevBuf<uint32_t> bbox;
    HIP_TRY(c, bbox.alloc_temp(c->arena, 6));
    launch_bbox(cl.x, cl.y, cl.z, n32, bbox.p, c->stream);
    uint32_t hb[6];
    HIP_TRY(c, hipMemcpyAsync(hb, bbox.p, sizeof(hb), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // the grid, in fp32 with IEEE ops: floorf(v * inv) is monotone in v, so the box's ends give every point's cell range
    const float inv = 1.0f / leaf;
    int lo[3];
    uint64_t dim[3];
    for (int k = 0; k < 3; k++) {
        const float bmin = ord2f(hb[k]), bmax = ord2f(hb[3 + k]);
        if (!std::isfinite(bmin) || !std::isfinite(bmax)) return fail(c, SYMMICP_ERR_ARG, "cloud has non-finite coordinates");
        const float flo = std::floor(bmin * inv), fhi = std::floor(bmax * inv);
        if (!(flo >= -2147483648.0f && flo < 2147483648.0f && fhi >= -2147483648.0f && fhi < 2147483648.0f))
            return fail(c, SYMMICP_ERR_ARG, "leaf size is too small for the input cloud: voxel indices overflow an int32");
        lo[k] = (int)flo;
        dim[k] = (uint64_t)((int64_t)(int)fhi - (int64_t)lo[k] + 1);
    }
    const unsigned __int128 total = (unsigned __int128)dim[0] * dim[1] * dim[2];
    if (total > ((unsigned __int128)1 << 32))
        return fail(c, SYMMICP_ERR_ARG, "leaf size is too small for the input cloud: more than 2^32 voxels in its box");
    int bits = 0;
    while (((unsigned __int128)1 << bits) < total) bits++;

    DevBuf<uint32_t> keys, rows, kt, vt, ws, vid, first, kid, kfirst, kcount, scan_ws, words;
    DevBuf<float> sorted, d_xyz, d_nrm;
    DevBuf<int32_t> d_count, d_vof;
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
    launch_voxel_keys(cl, n32, inv, lo, dim[0], dim[1], keys.p, rows.p, c->stream);
    radix_sort_pairs(keys.p, rows.p, kt.p, vt.p, n32, bits, ws.p, wse, c->stream);
    launch_voxel_segments(keys.p, n32, vid.p, first.p, scan_ws.p, words.p, c->stream);
    uint32_t m0 = 0, m = 0;
    HIP_TRY(c, hipMemcpyAsync(&m0, words.p, sizeof(m0), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    launch_voxel_keep(first.p, m0, (uint32_t)min_points, kid.p, scan_ws.p, kfirst.p, kcount.p, words.p + 1, c->stream);
    HIP_TRY(c, hipMemcpyAsync(&m, words.p + 1, sizeof(m), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    *n_out = m;
    if (m > cap) return fail(c, SYMMICP_ERR_SIZE, "voxel_downsample: " + std::to_string(m) + " voxels do not fit cap " + std::to_string(cap));
    CloudSoA sc;
    soa_from_block(sorted.p, n, sc);
    launch_gather_soa(cl, rows.p, n32, sc, c->stream);
    HIP_TRY(c, d_xyz.alloc_temp(c->arena, 3 * (size_t)m));
    HIP_TRY(c, d_count.alloc_temp(c->arena, m));
    if (with_nrm) HIP_TRY(c, d_nrm.alloc_temp(c->arena, 3 * (size_t)m));
    launch_voxel_mean(sc, kfirst.p, kcount.p, m, with_nrm ? 1 : 0, d_xyz.p, d_nrm.p, d_count.p, c->stream);
    if (voxel_of) {
        HIP_TRY(c, d_vof.alloc_temp(c->arena, n));
        launch_voxel_of(keys.p, rows.p, vid.p, first.p, kid.p, n32, (uint32_t)min_points, d_vof.p, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(xyz_out, d_xyz.p, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, c->stream));
    if (with_nrm) HIP_TRY(c, hipMemcpyAsync(nrm_out, d_nrm.p, sizeof(float) * 3 * m, hipMemcpyDeviceToHost, c->stream));
    if (count_out) HIP_TRY(c, hipMemcpyAsync(count_out, d_count.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, c->stream));
    if (voxel_of) HIP_TRY(c, hipMemcpyAsync(voxel_of, d_vof.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream));
    return stream_done(c);
}

static const char *voxel_args_error(const float *xyz, const float *nrm, size_t n, float leaf, int min_points, const float *xyz_out,
                                    const float *nrm_out, const size_t *n_out)
{
    if (!xyz || !xyz_out || !n_out) return "voxel_downsample: xyz, xyz_out and n_out are required";
    if (n == 0 || n > 0x7fffffffull) return "voxel_downsample: n must be in 1 .. 2^31 - 1";
    if (!std::isfinite(leaf) || !(leaf > 0.f)) return "voxel_downsample: leaf must be finite and > 0";
    if (min_points < 1) return "voxel_downsample: min_points must be >= 1";
    if (nrm_out && !nrm) return "voxel_downsample: nrm_out needs nrm";
    return nullptr;
}

int symmicp_ctx_voxel_downsample(symmicp_ctx *c, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                                 size_t nrm_row_stride, size_t nrm_col_stride, size_t n, float leaf, int min_points, float *xyz_out,
                                 float *nrm_out, int32_t *count_out, int32_t *voxel_of, size_t cap, size_t *n_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = voxel_args_error(xyz, nrm, n, leaf, min_points, xyz_out, nrm_out, n_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    return voxel_downsample(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, leaf, min_points, xyz_out, nrm_out,
                            count_out, voxel_of, cap, n_out);
}

int symmicp_voxel_downsample(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                             size_t nrm_row_stride, size_t nrm_col_stride, size_t n, float leaf, int min_points, float *xyz_out,
                             float *nrm_out, int32_t *count_out, int32_t *voxel_of, size_t cap, size_t *n_out)
{
    if (voxel_args_error(xyz, nrm, n, leaf, min_points, xyz_out, nrm_out, n_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_voxel_downsample(c, xyz, xyz_row_stride, xyz_col_stride, nrm, nrm_row_stride, nrm_col_stride, n, leaf, min_points,
                                            xyz_out, nrm_out, count_out, voxel_of, cap, n_out);
    });
}

}  // extern "C"
