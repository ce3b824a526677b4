// engine_plane.cpp -- RANSAC plane segmentation (symmicp_ctx_segment_plane, symmicp_ctx_plane_hypotheses; kernels_plane.hip; DESIGN.md 4,
// "Plane segmentation").  A host pre-step entry like those of engine_cloud_ops.cpp, without an index: the cloud goes up once about its
// pivot, the hypotheses are drawn, scored and ranked on the device, and the host reads back the winner's flags; the refit over them is
// O(n), sequential by definition, and runs here in fp64.  Temporaries come from the context's arena only: its target, source, index and
// certificates are not touched.
#include "engine_internal.h"
#include "plane_core.h"
#include "eig3.h"

namespace {

const char *plane_args_error(const float *xyz, size_t xr, size_t xc, size_t n, const symmicp_plane_config *cfg)
{
    if (!xyz || !cfg) return "segment_plane: xyz and cfg are required";
    if (n < 3 || n > 0x7fffffffull) return "segment_plane: n must be in 3 .. 2^31 - 1";
    if (cfg->struct_size != sizeof(symmicp_plane_config)) return "segment_plane: cfg->struct_size is not sizeof(symmicp_plane_config)";
    if (cfg->hypotheses < 1 || cfg->hypotheses > (1u << 24)) return "segment_plane: hypotheses must be in 1 .. 2^24";
    if (!std::isfinite(cfg->max_dist) || !(cfg->max_dist > 0.f)) return "segment_plane: max_dist must be finite and > 0";
    if (cfg->min_inliers < 0 || (size_t)cfg->min_inliers > n) return "segment_plane: min_inliers must be in 0 .. n";
    if (cfg->refits < 0 || cfg->refits > 8) return "segment_plane: refits must be in 0 .. 8";
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(cfg->axis[a])) return "segment_plane: the axis is not finite";
    const bool have_axis = cfg->axis[0] != 0.f || cfg->axis[1] != 0.f || cfg->axis[2] != 0.f;
    if (have_axis && !(cfg->max_angle_deg > 0.f && cfg->max_angle_deg <= 90.f)) return "segment_plane: max_angle_deg must be in (0, 90] with an axis";
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(xyz[i * xr + a * xc])) return "segment_plane: a coordinate is not finite";
    return nullptr;
}

const char *plane_outputs_error(const float *plane4_out, const symmicp_plane_result *res, const int32_t *rows_out, size_t cap, const size_t *count_out)
{
    if (!plane4_out || !res || !count_out) return "segment_plane: plane4_out, result and count_out are required";
    if (!rows_out && cap > 0) return "segment_plane: rows_out is required when cap > 0";
    return nullptr;
}

inline double dot3(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// the cloud about the pivot in fp64, row i
struct Pivoted {
    const float *xyz;
    size_t xr, xc;
    double c[3];
    void at(size_t i, double x[3]) const
    {
        for (int a = 0; a < 3; a++) x[a] = (double)xyz[i * xr + a * xc] - c[a];
    }
};

// one refit (include/symmicp.h): the least-squares plane of the flagged rows, then the flags recomputed under it; returns their number
size_t plane_refit(const Pivoted &P, size_t n, std::vector<uint8_t> &mask, double max_dist, double nd[4])
{
    double s[3] = {0, 0, 0}, k = 0.0, x[3];
    for (size_t i = 0; i < n; i++)
        if (mask[i]) { P.at(i, x); for (int a = 0; a < 3; a++) s[a] = s[a] + x[a]; k += 1.0; }
    const double m[3] = {s[0] / k, s[1] / k, s[2] / k};
    double S[6] = {0, 0, 0, 0, 0, 0};                      // xx, xy, xz, yy, yz, zz
    for (size_t i = 0; i < n; i++)
        if (mask[i]) {
            P.at(i, x);
            const double e[3] = {x[0] - m[0], x[1] - m[1], x[2] - m[2]};
            S[0] = S[0] + e[0] * e[0]; S[1] = S[1] + e[0] * e[1]; S[2] = S[2] + e[0] * e[2];
            S[3] = S[3] + e[1] * e[1]; S[4] = S[4] + e[1] * e[2]; S[5] = S[5] + e[2] * e[2];
        }
    double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    jacobi3<true>(A, V);
    int j = 0;
    if (A[1][1] < A[j][j]) j = 1;
    if (A[2][2] < A[j][j]) j = 2;
    const double v[3] = {V[0][j], V[1][j], V[2][j]};
    const double len = std::sqrt(dot3(v, v));
    for (int a = 0; a < 3; a++) nd[a] = v[a] / len;
    nd[3] = -dot3(nd, m);
    size_t count = 0;
    for (size_t i = 0; i < n; i++) {
        P.at(i, x);
        mask[i] = std::fabs(dot3(nd, x) + nd[3]) <= max_dist ? 1 : 0;
        count += mask[i];
    }
    return count;
}

void clear_result(float plane4_out[4], symmicp_plane_result *res)
{
    std::memset(res, 0, sizeof(*res));
    res->best_hypothesis = -1;
    for (int k = 0; k < 4; k++) plane4_out[k] = 0.f;
}

// hyp_out / pivot_out: the test entry (plane4_out == NULL): the hypotheses are drawn and read back, nothing is scored
int plane_run(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, size_t n, const symmicp_plane_config &cfg, float plane4_out[4],
              symmicp_plane_result *res, int32_t *rows_out, size_t cap, size_t *count_out, double *distance_out, uint8_t *status_out,
              int32_t *inliers_out, float *hyp_out, float *pivot_out)
{
    const uint32_t H = cfg.hypotheses;
    const bool full = plane4_out != nullptr;
    // the pivot and the fp32 differences the device works on
    Pivoted P{xyz, xr, xc, {0, 0, 0}};
    double sum[3] = {0, 0, 0};
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) sum[a] += (double)xyz[i * xr + a * xc];
    float piv[3];
    for (int a = 0; a < 3; a++) { piv[a] = (float)(sum[a] / (double)n); P.c[a] = (double)piv[a]; }
    if (pivot_out) for (int a = 0; a < 3; a++) pivot_out[a] = piv[a];
    std::vector<float> pts(4 * n);
    for (size_t i = 0; i < n; i++) {
        for (int a = 0; a < 3; a++) pts[4 * i + a] = xyz[i * xr + a * xc] - piv[a];
        pts[4 * i + 3] = 0.f;
    }
    const bool have_axis = cfg.axis[0] != 0.f || cfg.axis[1] != 0.f || cfg.axis[2] != 0.f;
    float axis[3] = {0.f, 0.f, 0.f}, cos_min = 0.f;
    if (have_axis) {
        const double a64[3] = {cfg.axis[0], cfg.axis[1], cfg.axis[2]};
        const double len = std::sqrt(dot3(a64, a64));
        for (int a = 0; a < 3; a++) axis[a] = (float)(a64[a] / len);
        cos_min = (float)std::cos((double)cfg.max_angle_deg * 3.14159265358979323846 / 180.0);
    }

    HIP_TRY(c, hipSetDevice(c->device));
    arena_begin(c->arena, n * 17 + (size_t)H * (16 + 1 + 4 + 4) + ((size_t)1 << 20));
    DevBuf<float> d_pts, d_hyp, d_nd;
    DevBuf<uint8_t> d_status, d_mask;
    DevBuf<int32_t> d_inl;
    DevBuf<uint32_t> d_surv;
    DevBuf<unsigned long long> d_words;          // [0] the arg-max key, [1] low word: the survivor count
    HIP_TRY(c, d_pts.alloc_temp(c->arena, 4 * n));
    HIP_TRY(c, d_hyp.alloc_temp(c->arena, 4 * (size_t)H));
    HIP_TRY(c, d_nd.alloc_temp(c->arena, 4));
    HIP_TRY(c, d_status.alloc_temp(c->arena, H));
    HIP_TRY(c, d_inl.alloc_temp(c->arena, H));
    HIP_TRY(c, d_surv.alloc_temp(c->arena, H));
    HIP_TRY(c, d_words.alloc_temp(c->arena, 2));
    if (full) HIP_TRY(c, d_mask.alloc_temp(c->arena, n));
    uint32_t *d_nsurv = reinterpret_cast<uint32_t *>(d_words.p + 1);
    HIP_TRY(c, hipMemcpyAsync(d_pts.p, pts.data(), sizeof(float) * 4 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_words.p, 0, 2 * sizeof(unsigned long long), c->stream));
    launch_plane_hyp(d_pts.p, (uint32_t)n, H, plane_base(cfg.seed), have_axis ? axis : nullptr, cos_min, d_hyp.p, d_status.p, d_inl.p, d_surv.p,
                     d_nsurv, c->stream);
    unsigned long long key = 0;
    uint32_t n_surv = 0;
    float nd32[4] = {0.f, 0.f, 0.f, 0.f};
    std::vector<uint8_t> mask;
    if (full) {
        // one stream, no host decision in between: score, rank, flag the winner's rows
        launch_plane_score(d_pts.p, (uint32_t)n, d_hyp.p, d_surv.p, d_nsurv, H, cfg.max_dist, d_inl.p, c->sw.plane_score, c->stream);
        launch_ransac_argmax(d_status.p, d_inl.p, H, d_words.p, c->stream);
        launch_plane_mask(d_pts.p, (uint32_t)n, d_hyp.p, d_words.p, cfg.max_dist, d_mask.p, d_nd.p, c->stream);
        mask.resize(n);
        HIP_TRY(c, hipMemcpyAsync(&key, d_words.p, sizeof(key), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&n_surv, d_nsurv, sizeof(n_surv), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(nd32, d_nd.p, sizeof(nd32), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(mask.data(), d_mask.p, n, hipMemcpyDeviceToHost, c->stream));
    }
    if (status_out) HIP_TRY(c, hipMemcpyAsync(status_out, d_status.p, H, hipMemcpyDeviceToHost, c->stream));
    if (inliers_out) HIP_TRY(c, hipMemcpyAsync(inliers_out, d_inl.p, sizeof(int32_t) * H, hipMemcpyDeviceToHost, c->stream));
    if (hyp_out) HIP_TRY(c, hipMemcpyAsync(hyp_out, d_hyp.p, sizeof(float) * 4 * H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (!full) return SYMMICP_OK;          // (symmicp_ctx_plane_hypotheses)

    clear_result(plane4_out, res);
    *count_out = 0;
    res->evaluated = (int32_t)n_surv;
    const size_t need = (size_t)std::max(3, cfg.min_inliers);
    const uint32_t best_inl = (uint32_t)(key >> 32);
    if (key != 0ull) { res->best_hypothesis = (int32_t)(0xFFFFFFFFu - (uint32_t)key); res->inliers_ransac = (int32_t)best_inl; }
    if (key == 0ull || best_inl < need)
        return fail(c, SYMMICP_ERR_NO_CONSENSUS, key == 0ull ? "segment_plane: no hypothesis passed the checks (" + std::to_string(H) + " drawn)"
                                                             : "segment_plane: the best hypothesis has " + std::to_string(best_inl) + " inliers (" +
                                                                   std::to_string(need) + " are needed)");
    double nd[4] = {nd32[0], nd32[1], nd32[2], nd32[3]};
    size_t count = best_inl;
    for (int r = 0; r < cfg.refits; r++) {
        count = plane_refit(P, n, mask, (double)cfg.max_dist, nd);
        if (count < need) return fail(c, SYMMICP_ERR_NO_CONSENSUS, "segment_plane: a refit left " + std::to_string(count) + " inliers (" +
                                                                       std::to_string(need) + " are needed)");
    }
    // orientation: along the axis, or the largest component positive
    bool flip;
    if (have_axis) {
        const double a64[3] = {axis[0], axis[1], axis[2]};
        flip = dot3(nd, a64) < 0.0;
    } else {
        int j = 0;
        if (std::fabs(nd[1]) > std::fabs(nd[j])) j = 1;
        if (std::fabs(nd[2]) > std::fabs(nd[j])) j = 2;
        flip = nd[j] < 0.0;
    }
    if (flip) for (double &v : nd) v = -v;
    double sse = 0.0, x[3];
    for (size_t i = 0; i < n; i++) {
        if (!distance_out && !mask[i]) continue;
        P.at(i, x);
        const double s = dot3(nd, x) + nd[3];
        if (distance_out) distance_out[i] = s;
        if (mask[i]) sse = sse + s * s;
    }
    res->inliers_final = (int32_t)count;
    res->rmse_final = std::sqrt(sse / (double)count);
    for (int a = 0; a < 3; a++) res->plane[a] = nd[a];
    res->plane[3] = nd[3] - dot3(nd, P.c);
    for (int k = 0; k < 4; k++) plane4_out[k] = (float)res->plane[k];
    *count_out = count;
    if (count > cap) return fail(c, SYMMICP_ERR_SIZE, "segment_plane: " + std::to_string(count) + " inlier rows do not fit cap " + std::to_string(cap));
    size_t at = 0;
    for (size_t i = 0; i < n; i++) if (mask[i]) rows_out[at++] = (int32_t)i;
    return SYMMICP_OK;
}

}  // namespace

extern "C" {

void symmicp_plane_config_default(symmicp_plane_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->hypotheses = 1000;
    cfg->min_inliers = 3;
    cfg->refits = 1;
}

int symmicp_ctx_segment_plane(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_plane_config *cfg,
                              float plane4_out[4], symmicp_plane_result *result, int32_t *rows_out, size_t cap, size_t *count_out,
                              double *distance_out, uint8_t *status_out, int32_t *inliers_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = plane_outputs_error(plane4_out, result, rows_out, cap, count_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    if (const char *msg = plane_args_error(xyz, row_stride, col_stride, n, cfg)) return fail(c, SYMMICP_ERR_ARG, msg);
    return plane_run(c, xyz, row_stride, col_stride, n, *cfg, plane4_out, result, rows_out, cap, count_out, distance_out, status_out, inliers_out,
                     nullptr, nullptr);
}

int symmicp_segment_plane(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_plane_config *cfg,
                          float plane4_out[4], symmicp_plane_result *result, int32_t *rows_out, size_t cap, size_t *count_out, double *distance_out,
                          uint8_t *status_out, int32_t *inliers_out)
{
    if (plane_outputs_error(plane4_out, result, rows_out, cap, count_out) || plane_args_error(xyz, row_stride, col_stride, n, cfg)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_segment_plane(c, xyz, row_stride, col_stride, n, cfg, plane4_out, result, rows_out, cap, count_out, distance_out,
                                         status_out, inliers_out);
    });
}

int symmicp_ctx_plane_hypotheses(symmicp_ctx *c, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_plane_config *cfg,
                                 float *hyp_out, uint8_t *status_out, float pivot_out[3])
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!hyp_out) return fail(c, SYMMICP_ERR_ARG, "plane_hypotheses: hyp_out is required");
    if (const char *msg = plane_args_error(xyz, row_stride, col_stride, n, cfg)) return fail(c, SYMMICP_ERR_ARG, msg);
    return plane_run(c, xyz, row_stride, col_stride, n, *cfg, nullptr, nullptr, nullptr, 0, nullptr, nullptr, status_out, nullptr, hyp_out, pivot_out);
}

}  // extern "C"
