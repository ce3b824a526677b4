// engine_batch.cpp -- host side of the batched alignment (symmicp_ctx_batch_align, symmicp_batch_align; kernels_batch.hip has the
// kernel, include/symmicp.h the contract): argument checks that need no device, the pivots, the start order, one launch, the read-back.
#include <map>
#include <numeric>

#include "engine_internal.h"

void symmicp_batch_config_default(symmicp_batch_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->mode = SYMMICP_MODE_PAPER;
    cfg->max_iters = 10;
    cfg->diff_threshold = 1.0f;
    cfg->min_normal_dot = -2.0f;
}

namespace {

constexpr size_t kBatchMaxProblems = (size_t)1 << 20;

// rows of a pool that some problem uses, as a difference array over the pool (O(B + n), however the ranges overlap)
struct Coverage {
    std::vector<int32_t> d;
    explicit Coverage(size_t n) : d(n + 1, 0) {}
    void add(size_t first, size_t count) { d[first]++; d[first + count]--; }
    template <typename F>
    bool all_used(F &&ok) const
    {
        int64_t depth = 0;
        for (size_t i = 0; i + 1 < d.size(); i++) {
            depth += d[i];
            if (depth > 0 && !ok(i)) return false;
        }
        return true;
    }
};

inline bool row_finite(const float *pool, size_t i)
{
    return std::isfinite(pool[3 * i]) && std::isfinite(pool[3 * i + 1]) && std::isfinite(pool[3 * i + 2]);
}

// every SYMMICP_ERR_ARG / _SIZE of the contract; no device is touched
int batch_args_error(const float *src_xyz, const float *src_nrm, size_t ns_total, const float *tgt_xyz, const float *tgt_nrm, size_t nt_total,
                     const symmicp_batch_problem *problems, size_t B, const symmicp_batch_config *cfg, const symmicp_batch_result *out,
                     std::string &msg)
{
    auto bad = [&msg](int code, const std::string &m) { msg = "batch_align: " + m; return code; };
    if (!src_xyz || !tgt_xyz || !tgt_nrm || !problems || !cfg || !out) return bad(SYMMICP_ERR_ARG, "src_xyz, tgt_xyz, tgt_nrm, problems, cfg and out are required");
    if (cfg->struct_size != sizeof(symmicp_batch_config)) return bad(SYMMICP_ERR_ARG, "cfg->struct_size is not sizeof(symmicp_batch_config)");
    if (cfg->mode != SYMMICP_MODE_PAPER && cfg->mode != SYMMICP_MODE_P2P && cfg->mode != SYMMICP_MODE_PLANE)
        return bad(SYMMICP_ERR_ARG, "the mode must be PAPER, P2P or PLANE (QUIRKS, GICP and COLOR are out of scope)");
    if (B == 0 || B > kBatchMaxProblems) return bad(SYMMICP_ERR_ARG, "B must be in 1 .. 2^20");
    if (cfg->max_iters < 0 || cfg->max_iters > 1000) return bad(SYMMICP_ERR_ARG, "max_iters must be in 0 .. 1000");
    for (float v : {cfg->diff_threshold, cfg->max_corr_dist, cfg->min_normal_dot, cfg->eps_rotation, cfg->eps_translation})
        if (!std::isfinite(v)) return bad(SYMMICP_ERR_ARG, "a threshold is not finite");
    if (!src_nrm && cfg->mode != SYMMICP_MODE_PLANE) return bad(SYMMICP_ERR_ARG, "src_nrm may be NULL in PLANE only");
    if (!src_nrm && cfg->min_normal_dot > -1.0f) return bad(SYMMICP_ERR_ARG, "min_normal_dot > -1 needs source normals");
    for (size_t b = 0; b < B; b++) {
        const symmicp_batch_problem &p = problems[b];
        if (p.src_count == 0 || p.tgt_count == 0) return bad(SYMMICP_ERR_ARG, "problem " + std::to_string(b) + " has an empty cloud");
        if (p.src_count > SYMMICP_BATCH_MAX_POINTS || p.tgt_count > SYMMICP_BATCH_MAX_POINTS)
            return bad(SYMMICP_ERR_SIZE, "problem " + std::to_string(b) + " has a cloud above SYMMICP_BATCH_MAX_POINTS = " +
                                             std::to_string(SYMMICP_BATCH_MAX_POINTS) + " points: use a context with the tree search");
        if ((size_t)p.src_first + p.src_count > ns_total || (size_t)p.tgt_first + p.tgt_count > nt_total)
            return bad(SYMMICP_ERR_ARG, "problem " + std::to_string(b) + " names rows outside its pool");
    }
    Coverage cs(ns_total), ct(nt_total);
    for (size_t b = 0; b < B; b++) { cs.add(problems[b].src_first, problems[b].src_count); ct.add(problems[b].tgt_first, problems[b].tgt_count); }
    if (!cs.all_used([&](size_t i) { return row_finite(src_xyz, i) && (!src_nrm || row_finite(src_nrm, i)); }))
        return bad(SYMMICP_ERR_ARG, "a source row some problem uses is not finite");
    if (!ct.all_used([&](size_t i) { return row_finite(tgt_xyz, i) && row_finite(tgt_nrm, i); }))
        return bad(SYMMICP_ERR_ARG, "a target row some problem uses is not finite");
    return SYMMICP_OK;
}

// the pivot of a target range: the fp64 sum of its rows in row order over the count, rounded to fp32
void range_pivot(const float *tgt_xyz, uint32_t first, uint32_t count, float out[3])
{
    double s[3] = {0.0, 0.0, 0.0};
    for (size_t i = first; i < (size_t)first + count; i++)
        for (int k = 0; k < 3; k++) s[k] += (double)tgt_xyz[3 * i + k];
    for (int k = 0; k < 3; k++) out[k] = (float)(s[k] / (double)count);
}

}  // namespace

int symmicp_ctx_batch_align(symmicp_ctx *c, const float *src_xyz, const float *src_nrm, size_t ns_total, const float *tgt_xyz,
                            const float *tgt_nrm, size_t nt_total, const symmicp_batch_problem *problems, const float *guess16, size_t B,
                            const symmicp_batch_config *cfg, symmicp_batch_result *out, float *trace_X, double *trace_sums)
{
    if (!c) return SYMMICP_ERR_ARG;
    std::string msg;
    if (const int st = batch_args_error(src_xyz, src_nrm, ns_total, tgt_xyz, tgt_nrm, nt_total, problems, B, cfg, out, msg)) return fail(c, st, msg);

    // start order: descending src_count x tgt_count (the longest problems first, as the packets are started), ties by index; the pivots
    // once per distinct target range (multi-start: one range for the whole batch)
    std::vector<uint32_t> order(B);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return (uint64_t)problems[x].src_count * problems[x].tgt_count > (uint64_t)problems[y].src_count * problems[y].tgt_count;
    });
    std::map<uint64_t, uint32_t> pivot_of;      // (tgt_first, tgt_count) -> the first problem with that range
    std::vector<BatchProblem> plist(B);
    std::vector<float> pivots(3 * B);
    for (size_t b = 0; b < B; b++) {
        const uint64_t key = ((uint64_t)problems[b].tgt_first << 32) | problems[b].tgt_count;
        const auto it = pivot_of.find(key);
        if (it == pivot_of.end()) { pivot_of.emplace(key, (uint32_t)b); range_pivot(tgt_xyz, problems[b].tgt_first, problems[b].tgt_count, &pivots[3 * b]); }
        else std::memcpy(&pivots[3 * b], &pivots[3 * (size_t)it->second], sizeof(float) * 3);
    }
    for (size_t k = 0; k < B; k++) {
        const uint32_t b = order[k];
        BatchProblem &p = plist[k];
        p.src_first = problems[b].src_first; p.src_count = problems[b].src_count;
        p.tgt_first = problems[b].tgt_first; p.tgt_count = problems[b].tgt_count;
        std::memcpy(p.pivot, &pivots[3 * (size_t)b], sizeof(float) * 3);
        p.slot = b;
    }

    HIP_TRY(c, hipSetDevice(c->device));
    const size_t rows = (size_t)cfg->max_iters + 1;
    const size_t b_src = sizeof(float) * 3 * ns_total, b_tgt = sizeof(float) * 3 * nt_total, b_out = sizeof(symmicp_batch_result) * B,
                 b_tx = trace_X ? sizeof(float) * 16 * rows * B : 0, b_ts = trace_sums ? sizeof(double) * SYMMICP_NSUM * rows * B : 0;
    arena_begin(c->arena, 2 * b_src + 2 * b_tgt + sizeof(BatchProblem) * B + sizeof(float) * 16 * B + b_out + b_tx + b_ts + 16 * 256);
    DevBuf<float> d_sx, d_sn, d_tx, d_tn, d_guess, d_trX;
    DevBuf<double> d_trS;
    DevBuf<BatchProblem> d_prob;
    DevBuf<symmicp_batch_result> d_out;
    HIP_TRY(c, d_sx.alloc_temp(c->arena, 3 * ns_total));
    HIP_TRY(c, d_tx.alloc_temp(c->arena, 3 * nt_total));
    HIP_TRY(c, d_tn.alloc_temp(c->arena, 3 * nt_total));
    HIP_TRY(c, d_prob.alloc_temp(c->arena, B));
    HIP_TRY(c, d_out.alloc_temp(c->arena, B));
    HIP_TRY(c, hipMemcpyAsync(d_sx.p, src_xyz, b_src, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_tx.p, tgt_xyz, b_tgt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_tn.p, tgt_nrm, b_tgt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_prob.p, plist.data(), sizeof(BatchProblem) * B, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_out.p, 0, b_out, c->stream));
    if (src_nrm) {
        HIP_TRY(c, d_sn.alloc_temp(c->arena, 3 * ns_total));
        HIP_TRY(c, hipMemcpyAsync(d_sn.p, src_nrm, b_src, hipMemcpyHostToDevice, c->stream));
    }
    if (guess16) {
        HIP_TRY(c, d_guess.alloc_temp(c->arena, 16 * B));
        HIP_TRY(c, hipMemcpyAsync(d_guess.p, guess16, sizeof(float) * 16 * B, hipMemcpyHostToDevice, c->stream));
    }
    if (trace_X) {
        HIP_TRY(c, d_trX.alloc_temp(c->arena, 16 * rows * B));
        HIP_TRY(c, hipMemsetAsync(d_trX.p, 0, b_tx, c->stream));
    }
    if (trace_sums) {
        HIP_TRY(c, d_trS.alloc_temp(c->arena, SYMMICP_NSUM * rows * B));
        HIP_TRY(c, hipMemsetAsync(d_trS.p, 0, b_ts, c->stream));
    }

    BatchArgs a{};
    a.src_xyz = d_sx.p; a.src_nrm = src_nrm ? d_sn.p : nullptr; a.tgt_xyz = d_tx.p; a.tgt_nrm = d_tn.p;
    a.problems = d_prob.p;
    a.guess = guess16 ? d_guess.p : nullptr;
    a.out = d_out.p; a.trace_X = trace_X ? d_trX.p : nullptr; a.trace_sums = trace_sums ? d_trS.p : nullptr;
    a.mode = cfg->mode; a.max_iters = cfg->max_iters; a.fixed_iters = cfg->fixed_iters;
    a.diff_threshold = cfg->diff_threshold;
    a.max_d2 = cfg->max_corr_dist > 0.f ? cfg->max_corr_dist * cfg->max_corr_dist : 0.f;      // the fp32 square, as every pass takes it
    a.min_ndot = cfg->min_normal_dot;
    a.eps_rotation = cfg->eps_rotation; a.eps_translation = cfg->eps_translation;
    launch_batch_align(a, (uint32_t)B, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(out, d_out.p, b_out, hipMemcpyDeviceToHost, c->stream));
    if (trace_X) HIP_TRY(c, hipMemcpyAsync(trace_X, d_trX.p, b_tx, hipMemcpyDeviceToHost, c->stream));
    if (trace_sums) HIP_TRY(c, hipMemcpyAsync(trace_sums, d_trS.p, b_ts, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

int symmicp_batch_align(int device, const float *src_xyz, const float *src_nrm, size_t ns_total, const float *tgt_xyz, const float *tgt_nrm,
                        size_t nt_total, const symmicp_batch_problem *problems, const float *guess16, size_t B, const symmicp_batch_config *cfg,
                        symmicp_batch_result *out, float *trace_X, double *trace_sums)
{
    std::string msg;
    if (const int st = batch_args_error(src_xyz, src_nrm, ns_total, tgt_xyz, tgt_nrm, nt_total, problems, B, cfg, out, msg)) return st;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_batch_align(c, src_xyz, src_nrm, ns_total, tgt_xyz, tgt_nrm, nt_total, problems, guess16, B, cfg, out, trace_X, trace_sums);
    });
}
