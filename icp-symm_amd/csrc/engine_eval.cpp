// engine_eval.cpp -- registration evaluation (symmicp.h: symmicp_evaluation; kernels_eval.hip; DESIGN.md 4, "Registration evaluation"):
// fitness, inlier RMSE and the 6x6 information matrix of K transforms of one cloud pair, as a pure function of (source, target, transform,
// distance).  The host-array form uploads both clouds, builds a scratch index over the target (build_reverse_index: the octree of the
// reverse search, tq labelled with the caller's rows) and reads the source through its Morton order; the context form runs on the clouds
// the context holds -- its own index when it is a TREE context, a scratch one otherwise -- and leaves the context as it found it.
#include <cmath>
#include "engine_internal.h"

extern "C" {

int symmicp_information_from_sums(uint64_t n, const double sum_q[3], const double sum_qq[6], double out36[36])
{
    if (!sum_q || !sum_qq || !out36) return SYMMICP_ERR_ARG;
    const double sx = sum_q[0], sy = sum_q[1], sz = sum_q[2];
    const double xx = sum_qq[0], xy = sum_qq[1], xz = sum_qq[2], yy = sum_qq[3], yz = sum_qq[4], zz = sum_qq[5];
    const double nd = (double)n;
    const double L[36] = {
        yy + zz, -xy,     -xz,     0.0, -sz, sy,
        -xy,     xx + zz, -yz,     sz,  0.0, -sx,
        -xz,     -yz,     xx + yy, -sy, sx,  0.0,
        0.0,     sz,      -sy,     nd,  0.0, 0.0,
        -sz,     0.0,     sx,      0.0, nd,  0.0,
        sy,      -sx,     0.0,     0.0, 0.0, nd,
    };
    std::memcpy(out36, L, sizeof(L));
    return SYMMICP_OK;
}

}  // extern "C"

namespace {

constexpr size_t kEvalMaxK = 4096;

// everything that is decided before a device is needed; the clouds may be null (the context form has its own)
const char *eval_common_error(const float *X16, size_t K, float max_dist, const symmicp_evaluation *out)
{
    if (!out) return "evaluate: out is required";
    if (K < 1 || K > kEvalMaxK) return "evaluate: K must be in 1 .. 4096";
    if (!X16 && K != 1) return "evaluate: X16 == NULL needs K == 1";
    if (!std::isfinite(max_dist)) return "evaluate: max_dist must be finite (<= 0: no gate)";
    if (X16)
        for (size_t k = 0; k < K; k++)
            for (int e = 0; e < 12; e++)
                if (!std::isfinite(X16[16 * k + e])) return "evaluate: a transform has a non-finite entry in its top three rows";
    return nullptr;
}

const char *eval_cloud_error(const float *xyz, size_t rs, size_t cs, size_t n)
{
    if (!xyz) return "evaluate: src_xyz and tgt_xyz are required";
    if (n == 0 || n > 0x7fffffffull) return "evaluate: ns and nt must be in 1 .. 2^31 - 1";
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(xyz[i * rs + a * cs])) return "evaluate: a coordinate is not finite";
    return nullptr;
}

const char *eval_args_error(const float *src, size_t sr, size_t sc, size_t ns, const float *tgt, size_t tr, size_t tc, size_t nt,
                            const float *X16, size_t K, float max_dist, const symmicp_evaluation *out)
{
    if (!src || !tgt) return "evaluate: src_xyz and tgt_xyz are required";
    if (const char *m = eval_common_error(X16, K, max_dist, out)) return m;
    if (ns == 0 || ns > 0x7fffffffull || nt == 0 || nt > 0x7fffffffull) return "evaluate: ns and nt must be in 1 .. 2^31 - 1";
    if (const char *m = eval_cloud_error(src, sr, sc, ns)) return m;
    return eval_cloud_error(tgt, tr, tc, nt);
}

void planar_stage(const float *xyz, size_t rs, size_t cs, size_t n, std::vector<float> &out)
{
    out.resize(3 * n);
    for (size_t i = 0; i < n; i++)
        for (int a = 0; a < 3; a++) out[(size_t)a * n + i] = xyz[i * rs + a * cs];
}

// The launches and the read-back: K transforms in chunks whose per-row arrays fit kChunkBytes (a result does not depend on its chunk).
// args: everything but X12 / nn / d2 / partials filled in.  X16 == nullptr: X_default.
int eval_run(symmicp_ctx *c, EvalArgs args, const float *X16, const float *X_default, size_t K, float max_dist, symmicp_evaluation *out,
             int32_t *nn_out, float *d2_out)
{
    constexpr size_t kChunkBytes = (size_t)256 << 20;
    const size_t ns = args.ns;
    const size_t Kc = std::min(K, std::max<size_t>(1, kChunkBytes / (8 * ns)));
    const uint32_t nb = eval_sum_blocks(args.ns);
    auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_X = 0, o_nn = o_X + pad(sizeof(float) * 12 * K), o_d2 = o_nn + pad(sizeof(int32_t) * Kc * ns),
                 o_part = o_d2 + pad(sizeof(float) * Kc * ns), o_sums = o_part + pad(sizeof(double) * Kc * nb * kEvalNSum),
                 total = o_sums + pad(sizeof(double) * K * kEvalNSum);
    std::vector<float> X12(12 * K);
    for (size_t k = 0; k < K; k++)
        for (int e = 0; e < 12; e++) X12[12 * k + e] = X16 ? X16[16 * k + e] : X_default[e];
    std::vector<double> sums(K * kEvalNSum);
    OwnSearch own(c);      // (no index of its own: the block, freed once the stream is done with it on every exit)
    HIP_TRY(c, hipMalloc((void **)&own.d, total));
    char *d = own.d;
    HIP_TRY(c, hipMemcpyAsync(d + o_X, X12.data(), sizeof(float) * 12 * K, hipMemcpyHostToDevice, c->stream));
    args.r2 = max_dist > 0.f ? max_dist * max_dist : std::numeric_limits<float>::infinity();
    args.nn = reinterpret_cast<int32_t *>(d + o_nn);
    args.d2 = reinterpret_cast<float *>(d + o_d2);
    args.partials = reinterpret_cast<double *>(d + o_part);
    for (size_t k0 = 0; k0 < K; k0 += Kc) {
        const size_t kn = std::min(Kc, K - k0);
        args.X12 = reinterpret_cast<const float *>(d + o_X) + 12 * k0;
        launch_eval(args, (uint32_t)kn, reinterpret_cast<double *>(d + o_sums) + k0 * kEvalNSum, c->stream);
        HIP_TRY(c, hipGetLastError());
        if (nn_out) HIP_TRY(c, hipMemcpyAsync(nn_out + k0 * ns, args.nn, sizeof(int32_t) * kn * ns, hipMemcpyDeviceToHost, c->stream));
        if (d2_out) HIP_TRY(c, hipMemcpyAsync(d2_out + k0 * ns, args.d2, sizeof(float) * kn * ns, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // (the next chunk writes the same arrays)
    }
    HIP_TRY(c, hipMemcpyAsync(sums.data(), d + o_sums, sizeof(double) * K * kEvalNSum, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < K; k++) {
        const double *s = sums.data() + k * kEvalNSum;
        symmicp_evaluation &e = out[k];
        std::memset(&e, 0, sizeof(e));
        e.inliers = (uint64_t)s[0];
        e.sum_d2 = s[1];
        for (int a = 0; a < 3; a++) e.sum_q[a] = s[2 + a];
        for (int a = 0; a < 6; a++) e.sum_qq[a] = s[5 + a];
        e.fitness = (double)e.inliers / (double)ns;
        e.mean_d2 = e.inliers ? e.sum_d2 / (double)e.inliers : 0.0;
        e.rmse = e.inliers ? std::sqrt(e.sum_d2 / (double)e.inliers) : 0.0;
        symmicp_information_from_sums(e.inliers, e.sum_q, e.sum_qq, e.information);
    }
    return SYMMICP_OK;
}

}  // namespace

extern "C" {

int symmicp_ctx_evaluate_registration(symmicp_ctx *c, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                                      const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const float *X16, size_t K,
                                      float max_dist, symmicp_evaluation *out, int32_t *nn_out, float *d2_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *m = eval_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, X16, K, max_dist, out))
        return fail(c, SYMMICP_ERR_ARG, m);
    HIP_TRY(c, hipSetDevice(c->device));
    // both clouds planar in allocations of their own (the index's build rewinds the scratch arena)
    std::vector<float> hs, ht;
    planar_stage(src_xyz, src_row_stride, src_col_stride, ns, hs);
    planar_stage(tgt_xyz, tgt_row_stride, tgt_col_stride, nt, ht);
    const size_t o_t = 0, o_s = (sizeof(float) * 3 * nt + 255) & ~(size_t)255, total = o_s + sizeof(float) * 3 * ns;
    OwnSearch own(c);      // (a scratch index: the context's own indexes stay as they were)
    HIP_TRY(c, hipMalloc((void **)&own.d, total));
    float *t = reinterpret_cast<float *>(own.d + o_t), *s = reinterpret_cast<float *>(own.d + o_s);
    HIP_TRY(c, hipMemcpyAsync(t, ht.data(), sizeof(float) * 3 * nt, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(s, hs.data(), sizeof(float) * 3 * ns, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    CloudSoA ct{t, t + nt, t + 2 * nt, t, t + nt, t + 2 * nt};      // (no normals: the build reads the slots and nothing keeps them)
    if (int st = build_reverse_index(c, ct, (uint32_t)nt, nullptr, own.ri)) return st;
    // the source's Morton order: the lanes of a wave then walk one region of the tree.  The points stay where they are and are read
    // through the order (12 B gathered per row and transform; the results are written by caller row either way)
    CloudSoA cs{s, s + ns, s + 2 * ns, s, s + ns, s + 2 * ns};
    arena_begin(c->arena, ns * 24 + ((size_t)1 << 20));
    DevBuf<uint32_t> order;
    float origin[3], h0;
    if (int st = morton_order(c, cs, (uint32_t)ns, order, nullptr, origin, &h0)) return st;
    EvalArgs a{};
    a.ix = own.ri.ix;
    a.sx = cs.x; a.sy = cs.y; a.sz = cs.z;
    a.order = order.p; a.gather = 1; a.ns = (uint32_t)ns;
    a.tx = ct.x; a.ty = ct.y; a.tz = ct.z;
    float I[16];
    identity16(I);
    return eval_run(c, a, X16, I, K, max_dist, out, nn_out, d2_out);
}

int symmicp_evaluate_registration(int device, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                                  const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const float *X16, size_t K,
                                  float max_dist, symmicp_evaluation *out, int32_t *nn_out, float *d2_out)
{
    if (eval_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, X16, K, max_dist, out))
        return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_evaluate_registration(c, src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, X16, K,
                                                 max_dist, out, nn_out, d2_out);
    });
}

int symmicp_evaluate(symmicp_ctx *c, const float *X16, size_t K, float max_dist, symmicp_evaluation *out, int32_t *nn_out, float *d2_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *m = eval_common_error(X16, K, max_dist, out)) return fail(c, SYMMICP_ERR_ARG, m);
    if (c->n_t == 0 || c->n_s_total == 0) return fail(c, SYMMICP_ERR_STATE, "evaluate: set_target and set_source come first");
    if (c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "evaluate: sharded contexts are out of scope (the sums would need an exchange)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    // a TREE context walks its own index; the others get a scratch one over the target they hold, dropped before returning
    // (a BRUTE context's c->ix holds tq and tn only, an IDENTITY context's nothing: have_index is false on both)
    const bool own = c->cfg.corr == SYMMICP_CORR_TREE && c->have_index && c->ix.onodes;
    OwnSearch scratch(c);
    if (!own)
        if (int st = build_reverse_index(c, c->tgt, c->n_t, nullptr, scratch.ri)) return st;
    EvalArgs a{};
    a.ix = own ? c->ix : scratch.ri.ix;
    a.ix.dbg = nullptr; a.ix.dbg_trace = nullptr;
    a.sx = c->src0.x; a.sy = c->src0.y; a.sz = c->src0.z;      // the source as set_source received it, in the share's order
    a.order = c->src_order; a.gather = 0; a.ns = c->n_loc;
    a.tx = c->tgt.x; a.ty = c->tgt.y; a.tz = c->tgt.z;
    return eval_run(c, a, X16, c->X, K, max_dist, out, nn_out, d2_out);
}

}  // extern "C"
