// engine_fgr.cpp -- host side of Fast Global Registration (symmicp_ctx_fgr, symmicp_fgr, symmicp_ctx_fgr_pass; kernels_fgr.hip has
// the kernels, include/symmicp.h the contract): argument checks that need no device, the pivots and D2, the tuple test's scan, one
// launch of the loop, the result in the caller's coordinates.  Temporaries come from the context's arena only: its source, target,
// index, attributes and certificates are not touched.
#include "engine_internal.h"
#include "ransac_core.h"

namespace {

constexpr size_t kFgrMaxDirect = (size_t)1 << 20;      // the largest set: m with the tuple test off, M of symmicp_ctx_fgr_pass

const char *fgr_args_error(const float *src, size_t sr, size_t sc, size_t ns, const float *tgt, size_t tr, size_t tc, size_t nt, const int32_t *pairs,
                           size_t m, const symmicp_fgr_config *cfg)
{
    if (!src || !tgt || !pairs || !cfg) return "fgr: src_xyz, tgt_xyz, pairs and cfg are required";
    if (cfg->struct_size != sizeof(symmicp_fgr_config)) return "fgr: cfg->struct_size is not sizeof(symmicp_fgr_config)";
    if (ns == 0 || ns > 0x7fffffffull || nt == 0 || nt > 0x7fffffffull) return "fgr: ns and nt must be in 1 .. 2^31 - 1";
    if (m < 3 || m > 0x7fffffffull) return "fgr: m must be in 3 .. 2^31 - 1";
    if (!std::isfinite(cfg->max_dist) || !(cfg->max_dist > 0.f)) return "fgr: max_dist must be finite and > 0";
    if (cfg->iterations < 1 || cfg->iterations > 1024) return "fgr: iterations must be in 1 .. 1024";
    if (cfg->decrease_every < 1) return "fgr: decrease_every must be >= 1";
    if (!std::isfinite(cfg->division_factor) || !(cfg->division_factor > 1.f)) return "fgr: division_factor must be finite and > 1";
    if (!(cfg->tuple_scale > 0.f) || !(cfg->tuple_scale <= 1.f)) return "fgr: tuple_scale must be in (0, 1]";
    if (cfg->max_tuples > (1u << 18)) return "fgr: max_tuples must be in 0 .. 2^18";
    if (cfg->tuple_trials > (1u << 24)) return "fgr: tuple_trials must be in 1 .. 2^24 (0: min(100 m, 2^24))";
    if (cfg->max_tuples == 0 && m > kFgrMaxDirect) return "fgr: with the tuple test off m must be <= 2^20";
    for (size_t k = 0; k < m; k++)
        if (pairs[2 * k] < 0 || (size_t)pairs[2 * k] >= ns || pairs[2 * k + 1] < 0 || (size_t)pairs[2 * k + 1] >= nt) return "fgr: a pair names a row outside its cloud";
    for (size_t k = 0; k < m; k++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(src[(size_t)pairs[2 * k] * sr + a * sc]) || !std::isfinite(tgt[(size_t)pairs[2 * k + 1] * tr + a * tc]))
                return "fgr: a paired point has a non-finite coordinate";
    return nullptr;
}

const char *fgr_pass_args_error(const float *p, const float *q, size_t M, const float *X16, float mu, const double *sums_out)
{
    if (!p || !q || !X16 || !sums_out) return "fgr_pass: p, q, X16 and sums_out are required";
    if (M == 0 || M > kFgrMaxDirect) return "fgr_pass: M must be in 1 .. 2^20";
    if (!std::isfinite(mu)) return "fgr_pass: mu is not finite";
    for (int k = 0; k < 16; k++) if (!std::isfinite(X16[k])) return "fgr_pass: X16 holds a non-finite value";
    for (size_t k = 0; k < 3 * M; k++) if (!std::isfinite(p[k]) || !std::isfinite(q[k])) return "fgr_pass: p or q holds a non-finite value";
    return nullptr;
}

void set_identity_result(float transform16[16], symmicp_fgr_result *res)
{
    std::memset(res, 0, sizeof(*res));
    for (int k = 0; k < 16; k++) { res->transform[k] = (k % 5 == 0) ? 1.0 : 0.0; transform16[k] = (k % 5 == 0) ? 1.f : 0.f; }
}

float norm2(const float *v) { return (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]; }

int fgr_run(symmicp_ctx *c, const float *src, size_t sr, size_t sc, const float *tgt, size_t tr, size_t tc, const int32_t *pairs, size_t m,
            const symmicp_fgr_config &cfg, float transform16[16], symmicp_fgr_result *res, int32_t *set_out, float *weight_out, float *X_trace,
            double *sums_trace, float *mu_trace)
{
    // the paired points, their fp64 means (the pivots), the fp32 differences the device works on and D2
    std::vector<double> X(3 * m), Y(3 * m);
    double sx[3] = {0, 0, 0}, sy[3] = {0, 0, 0};
    for (size_t k = 0; k < m; k++)
        for (int a = 0; a < 3; a++) {
            const float xv = src[(size_t)pairs[2 * k] * sr + a * sc], yv = tgt[(size_t)pairs[2 * k + 1] * tr + a * tc];
            X[3 * k + a] = xv; Y[3 * k + a] = yv;
            sx[a] += xv; sy[a] += yv;
        }
    float cs[3], ct[3];
    for (int a = 0; a < 3; a++) { cs[a] = (float)(sx[a] / (double)m); ct[a] = (float)(sy[a] / (double)m); }
    std::vector<float> pq(8 * m, 0.f);
    float D2 = 0.f;
    for (size_t k = 0; k < m; k++) {
        for (int a = 0; a < 3; a++) { pq[8 * k + a] = (float)X[3 * k + a] - cs[a]; pq[8 * k + 4 + a] = (float)Y[3 * k + a] - ct[a]; }
        D2 = std::max(D2, std::max(norm2(&pq[8 * k]), norm2(&pq[8 * k + 4])));
    }

    const bool tuples = cfg.max_tuples > 0;
    const uint32_t trials = !tuples ? 0u : cfg.tuple_trials ? cfg.tuple_trials : (uint32_t)std::min<size_t>(100 * m, (size_t)1 << 24);
    const size_t set_cap = tuples ? 3 * (size_t)cfg.max_tuples : m, iters = (size_t)cfg.iterations;
    HIP_TRY(c, hipSetDevice(c->device));
    arena_begin(c->arena, m * 32 + ((size_t)trials + 1) * 4 + ((size_t)trials / 2048 + 2) * 4 + set_cap * 8 + (iters + 1) * 64 + iters * (8 * SYMMICP_NSUM + 4) +
                              sizeof(FgrOut) + 16 * 256);
    DevBuf<float> d_pq, d_weight, d_trX, d_trMu;
    DevBuf<double> d_trS;
    DevBuf<uint32_t> d_rank, d_ws;
    DevBuf<int32_t> d_set;
    DevBuf<FgrOut> d_out;
    HIP_TRY(c, d_pq.alloc_temp(c->arena, 8 * m));
    HIP_TRY(c, hipMemcpyAsync(d_pq.p, pq.data(), sizeof(float) * 8 * m, hipMemcpyHostToDevice, c->stream));

    // ---- the tuple test: flags, their exclusive scan, the scatter in trial order
    uint32_t accepted = 0;
    size_t M = m;
    if (tuples) {
        HIP_TRY(c, d_rank.alloc_temp(c->arena, (size_t)trials + 1));
        HIP_TRY(c, d_ws.alloc_temp(c->arena, (size_t)trials / 2048 + 2));
        HIP_TRY(c, d_set.alloc_temp(c->arena, set_cap));
        const unsigned long long base = ransac_base_stream1(cfg.seed);
        launch_fgr_tuples(d_pq.p, (uint32_t)m, trials, base, cfg.tuple_scale * cfg.tuple_scale, d_rank.p, c->stream);
        launch_exclusive_scan(d_rank.p, trials + 1, d_ws.p, c->stream);
        launch_fgr_scatter(d_rank.p, (uint32_t)m, trials, base, cfg.max_tuples, d_set.p, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&accepted, d_rank.p + trials, sizeof(accepted), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        M = 3 * (size_t)std::min(accepted, cfg.max_tuples);
        res->tuples_accepted = accepted;
        if (accepted == 0)
            return fail(c, SYMMICP_ERR_NO_CONSENSUS, "fgr: no trial passed the tuple test (" + std::to_string(trials) + " drawn)");
        if (set_out) HIP_TRY(c, hipMemcpyAsync(set_out, d_set.p, sizeof(int32_t) * M, hipMemcpyDeviceToHost, c->stream));
    } else if (set_out) {
        for (size_t k = 0; k < m; k++) set_out[k] = (int32_t)k;
    }
    res->set_size = (uint32_t)M;

    // ---- the loop: one launch
    HIP_TRY(c, d_out.alloc_temp(c->arena, 1));
    HIP_TRY(c, hipMemsetAsync(d_out.p, 0, sizeof(FgrOut), c->stream));
    if (weight_out) HIP_TRY(c, d_weight.alloc_temp(c->arena, M));
    if (X_trace) {
        HIP_TRY(c, d_trX.alloc_temp(c->arena, 16 * (iters + 1)));
        HIP_TRY(c, hipMemsetAsync(d_trX.p, 0, sizeof(float) * 16 * (iters + 1), c->stream));
    }
    if (sums_trace) {
        HIP_TRY(c, d_trS.alloc_temp(c->arena, SYMMICP_NSUM * iters));
        HIP_TRY(c, hipMemsetAsync(d_trS.p, 0, sizeof(double) * SYMMICP_NSUM * iters, c->stream));
    }
    if (mu_trace) {
        HIP_TRY(c, d_trMu.alloc_temp(c->arena, iters));
        HIP_TRY(c, hipMemsetAsync(d_trMu.p, 0, sizeof(float) * iters, c->stream));
    }
    FgrArgs a{};
    a.pq = reinterpret_cast<const float4 *>(d_pq.p);
    a.set = tuples ? d_set.p : nullptr;
    a.M = (uint32_t)M;
    identity16(a.X0);
    a.mu0 = D2; a.delta2 = cfg.max_dist * cfg.max_dist; a.division = cfg.division_factor;
    a.iterations = cfg.iterations; a.decrease_every = cfg.decrease_every; a.pass_only = 0;
    a.weight = weight_out ? d_weight.p : nullptr;
    a.X_trace = X_trace ? d_trX.p : nullptr; a.sums_trace = sums_trace ? d_trS.p : nullptr; a.mu_trace = mu_trace ? d_trMu.p : nullptr;
    a.out = d_out.p;
    launch_fgr_optimize(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    FgrOut o;
    HIP_TRY(c, hipMemcpyAsync(&o, d_out.p, sizeof(o), hipMemcpyDeviceToHost, c->stream));
    if (weight_out) HIP_TRY(c, hipMemcpyAsync(weight_out, d_weight.p, sizeof(float) * M, hipMemcpyDeviceToHost, c->stream));
    if (X_trace) HIP_TRY(c, hipMemcpyAsync(X_trace, d_trX.p, sizeof(float) * 16 * (iters + 1), hipMemcpyDeviceToHost, c->stream));
    if (sums_trace) HIP_TRY(c, hipMemcpyAsync(sums_trace, d_trS.p, sizeof(double) * SYMMICP_NSUM * iters, hipMemcpyDeviceToHost, c->stream));
    if (mu_trace) HIP_TRY(c, hipMemcpyAsync(mu_trace, d_trMu.p, sizeof(float) * iters, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());

    // ---- into the caller's coordinates, fp64: T = T(ct) X T(-cs); inliers and RMSE over all m pairs
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(o.X[k])) return fail(c, SYMMICP_ERR_DEGENERATE, "fgr: the loop left a non-finite transform");
    double T[16];
    for (int k = 0; k < 16; k++) T[k] = k == 15 ? 1.0 : 0.0;
    for (int r = 0; r < 3; r++) {
        for (int b = 0; b < 3; b++) T[4 * r + b] = (double)o.X[4 * r + b];
        T[4 * r + 3] = ((double)o.X[4 * r + 3] + (double)ct[r]) - ((double)o.X[4 * r] * cs[0] + (double)o.X[4 * r + 1] * cs[1] + (double)o.X[4 * r + 2] * cs[2]);
    }
    const double md2 = (double)cfg.max_dist * (double)cfg.max_dist;
    size_t n_in = 0;
    double sse = 0.0;
    for (size_t k = 0; k < m; k++) {
        double r2 = 0.0;
        for (int r = 0; r < 3; r++) {
            const double d = T[4 * r] * X[3 * k] + T[4 * r + 1] * X[3 * k + 1] + T[4 * r + 2] * X[3 * k + 2] + T[4 * r + 3] - Y[3 * k + r];
            r2 += d * d;
        }
        if (r2 <= md2) { n_in++; sse += r2; }
    }
    res->iterations = o.iters;
    res->inliers = (int32_t)n_in;
    res->mu = o.mu;
    res->weight_sum = o.sums[34];
    res->rmse = n_in ? std::sqrt(sse / (double)n_in) : 0.0;
    for (int k = 0; k < 16; k++) { res->transform[k] = T[k]; transform16[k] = (float)T[k]; }
    if (o.status != SYMMICP_OK)
        return fail(c, SYMMICP_ERR_DEGENERATE, "fgr: degenerate system in iteration " + std::to_string(o.iters) + " (rank-deficient normal equations or non-finite transform)");
    return SYMMICP_OK;
}

}  // namespace

extern "C" {

void symmicp_fgr_config_default(symmicp_fgr_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->iterations = 64;
    cfg->decrease_every = 4;
    cfg->max_tuples = 1000;
    cfg->tuple_trials = 0;
    cfg->max_dist = 0.f;
    cfg->division_factor = 1.4f;
    cfg->tuple_scale = 0.95f;
    cfg->seed = 0;
}

int symmicp_ctx_fgr(symmicp_ctx *c, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns, const float *tgt_xyz,
                    size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const int32_t *pairs, size_t m, const symmicp_fgr_config *cfg,
                    float transform16[16], symmicp_fgr_result *result, int32_t *set_out, float *weight_out, float *X_trace, double *sums_trace,
                    float *mu_trace)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!transform16 || !result) return fail(c, SYMMICP_ERR_ARG, "fgr: transform16 and result are required");
    if (const char *msg = fgr_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg)) return fail(c, SYMMICP_ERR_ARG, msg);
    set_identity_result(transform16, result);
    return fgr_run(c, src_xyz, src_row_stride, src_col_stride, tgt_xyz, tgt_row_stride, tgt_col_stride, pairs, m, *cfg, transform16, result, set_out,
                   weight_out, X_trace, sums_trace, mu_trace);
}

int symmicp_fgr(int device, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns, const float *tgt_xyz,
                size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const int32_t *pairs, size_t m, const symmicp_fgr_config *cfg,
                float transform16[16], symmicp_fgr_result *result, int32_t *set_out, float *weight_out, float *X_trace, double *sums_trace,
                float *mu_trace)
{
    if (!transform16 || !result || fgr_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_fgr(c, src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg, transform16,
                               result, set_out, weight_out, X_trace, sums_trace, mu_trace);
    });
}

int symmicp_ctx_fgr_pass(symmicp_ctx *c, const float *p, const float *q, size_t M, const float X16[16], float mu, double *sums_out, float *weight_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = fgr_pass_args_error(p, q, M, X16, mu, sums_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<float> pq(8 * M, 0.f);
    for (size_t k = 0; k < M; k++)
        for (int a = 0; a < 3; a++) { pq[8 * k + a] = p[3 * k + a]; pq[8 * k + 4 + a] = q[3 * k + a]; }
    HIP_TRY(c, hipSetDevice(c->device));
    arena_begin(c->arena, M * 36 + sizeof(FgrOut) + 16 * 256);
    DevBuf<float> d_pq, d_weight;
    DevBuf<FgrOut> d_out;
    HIP_TRY(c, d_pq.alloc_temp(c->arena, 8 * M));
    HIP_TRY(c, d_out.alloc_temp(c->arena, 1));
    if (weight_out) HIP_TRY(c, d_weight.alloc_temp(c->arena, M));
    HIP_TRY(c, hipMemcpyAsync(d_pq.p, pq.data(), sizeof(float) * 8 * M, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_out.p, 0, sizeof(FgrOut), c->stream));
    FgrArgs a{};
    a.pq = reinterpret_cast<const float4 *>(d_pq.p);
    a.M = (uint32_t)M;
    std::memcpy(a.X0, X16, sizeof(a.X0));
    a.mu0 = mu; a.division = 2.f;
    a.iterations = 1; a.decrease_every = 1; a.pass_only = 1;
    a.weight = weight_out ? d_weight.p : nullptr;
    a.out = d_out.p;
    launch_fgr_optimize(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    FgrOut o;
    HIP_TRY(c, hipMemcpyAsync(&o, d_out.p, sizeof(o), hipMemcpyDeviceToHost, c->stream));
    if (weight_out) HIP_TRY(c, hipMemcpyAsync(weight_out, d_weight.p, sizeof(float) * M, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    std::memcpy(sums_out, o.sums, sizeof(o.sums));
    return SYMMICP_OK;
}

}  // extern "C"
