// engine_global.cpp -- feature matching and RANSAC (kernels_global.hip; DESIGN.md 4, "Feature matching and RANSAC"): the host side
// of symmicp_ctx_feature_nn, symmicp_ctx_feature_correspondences and symmicp_ctx_ransac.  Temporaries come from the context's arena
// only: its source, target, index and certificates are not touched.
#include "engine_internal.h"
#include "ransac_core.h"
#include <limits>

// ---- feature matching ------------------------------------------------------------------------------------------------------
static const char *features_error(const float *fa, size_t na, const float *fb, size_t nb)
{
    if (!fa || !fb) return "feature_nn: fa and fb are required";
    if (na == 0 || na > 0x7fffffffull || nb == 0 || nb > 0x7fffffffull) return "feature_nn: na and nb must be in 1 .. 2^31 - 1";
    for (size_t k = 0; k < na * 33; k++) if (!std::isfinite(fa[k])) return "feature_nn: fa holds a non-finite value";
    for (size_t k = 0; k < nb * 33; k++) if (!std::isfinite(fb[k])) return "feature_nn: fb holds a non-finite value";
    return nullptr;
}

// queries per thread and candidate splits of one search (kernels_global.hip): two queries per thread from 1 024 queries on (they
// halve the LDS reads per pair: 5-6 % faster at 16k and 64k queries, 1 % slower at 256k), candidates split over
// blockIdx.y while the queries alone give fewer than 512 workgroups
static void nn_shape(const symmicp_ctx *c, size_t na, size_t nb, int &q, uint32_t &splits)
{
    q = c->sw.feature_nn_queries == 1 || c->sw.feature_nn_queries == 2 ? c->sw.feature_nn_queries : (na >= 1024 ? 2 : 1);
    const size_t blocks = (na + 256 * (size_t)q - 1) / (256 * (size_t)q);
    size_t s = 1;
    if (c->sw.feature_nn_splits > 0) s = (size_t)c->sw.feature_nn_splits;
    else if (blocks < 512) s = std::min<size_t>(std::max<size_t>(nb / 512, 1), (1024 + blocks - 1) / blocks);
    splits = (uint32_t)std::min<size_t>(std::min<size_t>(s, nb), 65535);
}

struct NnDev {
    DevBuf<int32_t> nn;
    DevBuf<float> d2, second;
    DevBuf<char> partial;
};

// one search between device arrays, queued on the context's stream
static int nn_search(symmicp_ctx *c, const float *d_fa, size_t na, const float *d_fb, size_t nb, bool want_d2, NnDev &o)
{
    int q;
    uint32_t splits;
    nn_shape(c, na, nb, q, splits);
    HIP_TRY(c, o.nn.alloc_temp(c->arena, na));
    if (want_d2) {
        HIP_TRY(c, o.d2.alloc_temp(c->arena, na));
        HIP_TRY(c, o.second.alloc_temp(c->arena, na));
    }
    if (splits > 1) HIP_TRY(c, o.partial.alloc_temp(c->arena, feature_nn_partial_bytes((uint32_t)na, splits)));
    launch_feature_nn(d_fa, (uint32_t)na, d_fb, (uint32_t)nb, q, splits, o.partial.p, o.nn.p, o.d2.p, o.second.p, c->stream);
    HIP_TRY(c, hipGetLastError());
    return SYMMICP_OK;
}

static int upload_features(symmicp_ctx *c, const float *fa, size_t na, const float *fb, size_t nb, DevBuf<float> &d_fa, DevBuf<float> &d_fb)
{
    HIP_TRY(c, hipSetDevice(c->device));
    int q;
    uint32_t splits;
    nn_shape(c, std::min(na, nb), std::max(na, nb), q, splits);
    arena_begin(c->arena, (na + nb) * (33 * 4 + 2 * 12) + 2 * feature_nn_partial_bytes((uint32_t)std::max(na, nb), splits) + ((size_t)1 << 20));
    HIP_TRY(c, d_fa.alloc_temp(c->arena, na * 33));
    HIP_TRY(c, d_fb.alloc_temp(c->arena, nb * 33));
    HIP_TRY(c, hipMemcpyAsync(d_fa.p, fa, sizeof(float) * 33 * na, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(d_fb.p, fb, sizeof(float) * 33 * nb, hipMemcpyHostToDevice, c->stream));
    return SYMMICP_OK;
}

extern "C" {

int symmicp_ctx_feature_nn(symmicp_ctx *c, const float *fa, size_t na, const float *fb, size_t nb, int32_t *nn_out, float *d2_out,
                           float *d2_second_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!nn_out) return fail(c, SYMMICP_ERR_ARG, "feature_nn: nn_out is required");
    if (const char *msg = features_error(fa, na, fb, nb)) return fail(c, SYMMICP_ERR_ARG, msg);
    DevBuf<float> d_fa, d_fb;
    int st = upload_features(c, fa, na, fb, nb, d_fa, d_fb);
    if (st != SYMMICP_OK) return st;
    NnDev o;
    st = nn_search(c, d_fa.p, na, d_fb.p, nb, true, o);
    if (st != SYMMICP_OK) { (void)hipStreamSynchronize(c->stream); return st; }
    HIP_TRY(c, hipMemcpyAsync(nn_out, o.nn.p, sizeof(int32_t) * na, hipMemcpyDeviceToHost, c->stream));
    if (d2_out) HIP_TRY(c, hipMemcpyAsync(d2_out, o.d2.p, sizeof(float) * na, hipMemcpyDeviceToHost, c->stream));
    if (d2_second_out) HIP_TRY(c, hipMemcpyAsync(d2_second_out, o.second.p, sizeof(float) * na, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    return SYMMICP_OK;
}

static const char *corr_args_error(const float *fa, size_t na, const float *fb, size_t nb, float max_ratio, const int32_t *pairs_out, size_t cap,
                                   const size_t *count_out)
{
    if (!count_out) return "feature_correspondences: count_out is required";
    if (!pairs_out && cap > 0) return "feature_correspondences: pairs_out is required when cap > 0";
    if (std::isnan(max_ratio)) return "feature_correspondences: max_ratio is NaN";
    return features_error(fa, na, fb, nb);
}

int symmicp_ctx_feature_correspondences(symmicp_ctx *c, const float *fa, size_t na, const float *fb, size_t nb, int mutual, float max_ratio,
                                        int32_t *pairs_out, float *d2_out, size_t cap, size_t *count_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = corr_args_error(fa, na, fb, nb, max_ratio, pairs_out, cap, count_out)) return fail(c, SYMMICP_ERR_ARG, msg);
    std::vector<int32_t> ab(na), ba(mutual ? nb : 0);
    std::vector<float> d2(na), second(na);
    {
        DevBuf<float> d_fa, d_fb;
        int st = upload_features(c, fa, na, fb, nb, d_fa, d_fb);
        if (st != SYMMICP_OK) return st;
        NnDev o_ab, o_ba;
        st = nn_search(c, d_fa.p, na, d_fb.p, nb, true, o_ab);
        if (st == SYMMICP_OK && mutual) st = nn_search(c, d_fb.p, nb, d_fa.p, na, false, o_ba);
        if (st != SYMMICP_OK) { (void)hipStreamSynchronize(c->stream); return st; }
        HIP_TRY(c, hipMemcpyAsync(ab.data(), o_ab.nn.p, sizeof(int32_t) * na, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(d2.data(), o_ab.d2.p, sizeof(float) * na, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipMemcpyAsync(second.data(), o_ab.second.p, sizeof(float) * na, hipMemcpyDeviceToHost, c->stream));
        if (mutual) HIP_TRY(c, hipMemcpyAsync(ba.data(), o_ba.nn.p, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
    }
    // the filter: O(na) on the host, in fp32 as the header writes it
    const float ratio2 = max_ratio * max_ratio;
    auto kept = [&](size_t i) {
        if (mutual && ba[(size_t)ab[i]] != (int32_t)i) return false;
        if (max_ratio > 0.f && !(d2[i] <= ratio2 * second[i])) return false;
        return true;
    };
    size_t count = 0;
    for (size_t i = 0; i < na; i++) count += kept(i) ? 1 : 0;
    *count_out = count;
    if (count > cap) return fail(c, SYMMICP_ERR_SIZE, "feature_correspondences: " + std::to_string(count) + " pairs do not fit cap " + std::to_string(cap));
    size_t at = 0;
    for (size_t i = 0; i < na; i++) {
        if (!kept(i)) continue;
        pairs_out[2 * at] = (int32_t)i;
        pairs_out[2 * at + 1] = ab[i];
        if (d2_out) d2_out[at] = d2[i];
        at++;
    }
    return SYMMICP_OK;
}

}  // extern "C"

// ---- RANSAC ----------------------------------------------------------------------------------------------------------------
static const char *ransac_args_error(const float *src, size_t sr, size_t sc, size_t ns, const float *tgt, size_t tr, size_t tc, size_t nt,
                                     const int32_t *pairs, size_t m, const symmicp_ransac_config *cfg)
{
    if (!src || !tgt || !pairs || !cfg) return "ransac: src_xyz, tgt_xyz, pairs and cfg are required";
    if (cfg->struct_size != sizeof(symmicp_ransac_config)) return "ransac: cfg->struct_size is not sizeof(symmicp_ransac_config)";
    if (ns == 0 || ns > 0x7fffffffull || nt == 0 || nt > 0x7fffffffull) return "ransac: ns and nt must be in 1 .. 2^31 - 1";
    if (m < 3 || m > 0x7fffffffull) return "ransac: m must be in 3 .. 2^31 - 1";
    if (cfg->hypotheses < 1 || cfg->hypotheses > (1u << 24)) return "ransac: hypotheses must be in 1 .. 2^24";
    if (!std::isfinite(cfg->max_dist) || !(cfg->max_dist > 0.f)) return "ransac: max_dist must be finite and > 0";
    if (std::isnan(cfg->edge_ratio) || cfg->edge_ratio > 1.f) return "ransac: edge_ratio must be <= 1 (<= 0: check off)";
    if (cfg->refits < 0 || cfg->refits > 8) return "ransac: refits must be in 0 .. 8";
    for (size_t k = 0; k < m; k++)
        if (pairs[2 * k] < 0 || (size_t)pairs[2 * k] >= ns || pairs[2 * k + 1] < 0 || (size_t)pairs[2 * k + 1] >= nt) return "ransac: a pair names a row outside its cloud";
    for (size_t k = 0; k < m; k++)
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(src[(size_t)pairs[2 * k] * sr + a * sc]) || !std::isfinite(tgt[(size_t)pairs[2 * k + 1] * tr + a * tc]))
                return "ransac: a paired point has a non-finite coordinate";
    return nullptr;
}

// symmetric 4x4 eigen-decomposition by cyclic Jacobi rotations: A is overwritten by its diagonal form, V's columns are the vectors
static void jacobi4(double A[4][4], double V[4][4])
{
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) V[i][j] = i == j ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 64; sweep++) {
        double off = 0.0, diag = 0.0;
        for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) (i == j ? diag : off) += A[i][j] * A[i][j];
        if (off <= 1e-60 * diag || off == 0.0) break;
        for (int p = 0; p < 3; p++)
            for (int q = p + 1; q < 4; q++) {
                if (A[p][q] == 0.0) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * A[p][q]);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                for (int k = 0; k < 4; k++) { const double akp = A[k][p], akq = A[k][q]; A[k][p] = cs * akp - sn * akq; A[k][q] = sn * akp + cs * akq; }
                for (int k = 0; k < 4; k++) { const double apk = A[p][k], aqk = A[q][k]; A[p][k] = cs * apk - sn * aqk; A[q][k] = sn * apk + cs * aqk; }
                for (int k = 0; k < 4; k++) { const double vkp = V[k][p], vkq = V[k][q]; V[k][p] = cs * vkp - sn * vkq; V[k][q] = sn * vkp + cs * vkq; }
            }
    }
}

// Horn's closed form: the proper rotation R and translation t minimising sum |R x + t - y|^2 over the masked pairs, ascending k
static void horn_fit(const std::vector<double> &X, const std::vector<double> &Y, const std::vector<uint8_t> &mask, double T[16])
{
    const size_t m = mask.size();
    double cx[3] = {0, 0, 0}, cy[3] = {0, 0, 0}, cnt = 0;
    for (size_t k = 0; k < m; k++) if (mask[k]) { for (int a = 0; a < 3; a++) { cx[a] += X[3 * k + a]; cy[a] += Y[3 * k + a]; } cnt += 1.0; }
    for (int a = 0; a < 3; a++) { cx[a] /= cnt; cy[a] /= cnt; }
    double S[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    for (size_t k = 0; k < m; k++) if (mask[k])
        for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) S[a][b] += (X[3 * k + a] - cx[a]) * (Y[3 * k + b] - cy[b]);
    double N[4][4] = {{S[0][0] + S[1][1] + S[2][2], S[1][2] - S[2][1], S[2][0] - S[0][2], S[0][1] - S[1][0]},
                      {S[1][2] - S[2][1], S[0][0] - S[1][1] - S[2][2], S[0][1] + S[1][0], S[2][0] + S[0][2]},
                      {S[2][0] - S[0][2], S[0][1] + S[1][0], -S[0][0] + S[1][1] - S[2][2], S[1][2] + S[2][1]},
                      {S[0][1] - S[1][0], S[2][0] + S[0][2], S[1][2] + S[2][1], -S[0][0] - S[1][1] + S[2][2]}};
    double V[4][4];
    jacobi4(N, V);
    int best = 0;
    for (int i = 1; i < 4; i++) if (N[i][i] > N[best][best]) best = i;
    double q[4] = {V[0][best], V[1][best], V[2][best], V[3][best]};
    const double nq = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (double &v : q) v /= nq;
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double R[3][3] = {{w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)},
                            {2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)},
                            {2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z}};
    for (int k = 0; k < 16; k++) T[k] = k == 15 ? 1.0 : 0.0;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) T[4 * a + b] = R[a][b];
        T[4 * a + 3] = cy[a] - (R[a][0] * cx[0] + R[a][1] * cx[1] + R[a][2] * cx[2]);
    }
}

// the inlier set of T over all pairs in fp64; returns its size, *sse = the inliers' sum of squared residuals
static size_t inliers64(const std::vector<double> &X, const std::vector<double> &Y, const double T[16], double max_dist2, std::vector<uint8_t> &mask,
                        double *sse)
{
    size_t n = 0;
    double s = 0.0;
    for (size_t k = 0; k < mask.size(); k++) {
        double r2 = 0.0;
        for (int a = 0; a < 3; a++) {
            const double d = T[4 * a] * X[3 * k] + T[4 * a + 1] * X[3 * k + 1] + T[4 * a + 2] * X[3 * k + 2] + T[4 * a + 3] - Y[3 * k + a];
            r2 += d * d;
        }
        mask[k] = r2 <= max_dist2 ? 1 : 0;
        if (mask[k]) { n++; s += r2; }
    }
    *sse = s;
    return n;
}

static void set_identity_result(float transform16[16], symmicp_ransac_result *res)
{
    std::memset(res, 0, sizeof(*res));
    res->best_hypothesis = -1;
    for (int k = 0; k < 16; k++) { res->transform[k] = (k % 5 == 0) ? 1.0 : 0.0; transform16[k] = (k % 5 == 0) ? 1.f : 0.f; }
}

static int ransac_run(symmicp_ctx *c, const float *src, size_t sr, size_t sc, const float *tgt, size_t tr, size_t tc, const int32_t *pairs, size_t m,
                      const symmicp_ransac_config &cfg, float transform16[16], symmicp_ransac_result *res, uint8_t *mask_out, uint8_t *status_out,
                      int32_t *inliers_out, float *hyp_out, float *pivots_out)
{
    const uint32_t H = cfg.hypotheses;
    // the paired points, their fp64 means (the pivots) and the fp32 differences the device works on
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
    if (pivots_out) for (int a = 0; a < 3; a++) { pivots_out[a] = cs[a]; pivots_out[3 + a] = ct[a]; }
    std::vector<float> pq(8 * m, 0.f);
    for (size_t k = 0; k < m; k++)
        for (int a = 0; a < 3; a++) { pq[8 * k + a] = (float)X[3 * k + a] - cs[a]; pq[8 * k + 4 + a] = (float)Y[3 * k + a] - ct[a]; }

    HIP_TRY(c, hipSetDevice(c->device));
    arena_begin(c->arena, m * 32 + (size_t)H * (48 + 1 + 4 + 4) + ((size_t)1 << 20));
    DevBuf<float> d_pq, d_hyp;
    DevBuf<uint8_t> d_status;
    DevBuf<int32_t> d_inl;
    DevBuf<uint32_t> d_surv;
    DevBuf<unsigned long long> d_words;          // [0] the arg-max key, [1] low word: the survivor count
    HIP_TRY(c, d_pq.alloc_temp(c->arena, 8 * m));
    HIP_TRY(c, d_hyp.alloc_temp(c->arena, 12 * (size_t)H));
    HIP_TRY(c, d_status.alloc_temp(c->arena, H));
    HIP_TRY(c, d_inl.alloc_temp(c->arena, H));
    HIP_TRY(c, d_surv.alloc_temp(c->arena, H));
    HIP_TRY(c, d_words.alloc_temp(c->arena, 2));
    uint32_t *d_nsurv = reinterpret_cast<uint32_t *>(d_words.p + 1);
    HIP_TRY(c, hipMemcpyAsync(d_pq.p, pq.data(), sizeof(float) * 8 * m, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_words.p, 0, 2 * sizeof(unsigned long long), c->stream));
    const float max_dist2 = cfg.max_dist * cfg.max_dist;
    const float edge2 = cfg.edge_ratio > 0.f ? cfg.edge_ratio * cfg.edge_ratio : 0.f;
    launch_ransac_hyp(d_pq.p, (uint32_t)m, H, ransac_base(cfg.seed), max_dist2, edge2, d_hyp.p, d_status.p, d_inl.p, d_surv.p, d_nsurv, c->stream);
    uint32_t n_surv = 0;
    HIP_TRY(c, hipMemcpyAsync(&n_surv, d_nsurv, sizeof(n_surv), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    unsigned long long key = 0;
    if (transform16) {
        launch_ransac_eval(d_pq.p, (uint32_t)m, d_hyp.p, d_surv.p, d_nsurv, n_surv, max_dist2, d_inl.p, c->stream);
        launch_ransac_argmax(d_status.p, d_inl.p, H, d_words.p, c->stream);
        HIP_TRY(c, hipMemcpyAsync(&key, d_words.p, sizeof(key), hipMemcpyDeviceToHost, c->stream));
    }
    if (status_out) HIP_TRY(c, hipMemcpyAsync(status_out, d_status.p, H, hipMemcpyDeviceToHost, c->stream));
    if (inliers_out) HIP_TRY(c, hipMemcpyAsync(inliers_out, d_inl.p, sizeof(int32_t) * H, hipMemcpyDeviceToHost, c->stream));
    if (hyp_out) HIP_TRY(c, hipMemcpyAsync(hyp_out, d_hyp.p, sizeof(float) * 12 * H, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (!transform16 || !res) return SYMMICP_OK;          // (symmicp_ctx_ransac_hypotheses)

    set_identity_result(transform16, res);
    res->evaluated = (int32_t)n_surv;
    if (mask_out) std::memset(mask_out, 0, m);
    const uint32_t best_inl = (uint32_t)(key >> 32);
    if (key == 0ull || best_inl < 3) {
        if (key != 0ull) { res->best_hypothesis = (int32_t)(0xFFFFFFFFu - (uint32_t)key); res->inliers_ransac = (int32_t)best_inl; }
        return fail(c, SYMMICP_ERR_NO_CONSENSUS, n_surv == 0 ? "ransac: no hypothesis passed the checks (" + std::to_string(H) + " drawn)"
                                                              : "ransac: the best hypothesis has " + std::to_string(best_inl) + " inliers (3 are needed)");
    }
    const uint32_t hb = 0xFFFFFFFFu - (uint32_t)key;
    res->best_hypothesis = (int32_t)hb;
    res->inliers_ransac = (int32_t)best_inl;
    float Rt[12];
    HIP_TRY(c, hipMemcpy(Rt, d_hyp.p + 12 * (size_t)hb, sizeof(Rt), hipMemcpyDeviceToHost));
    // the winner's inlier set: the kernel's own test (ransac_core.h, fp32)
    std::vector<uint8_t> mask(m);
    size_t n_in = 0;
    double sse = 0.0;
    for (size_t k = 0; k < m; k++) {
        const float r2 = ransac_residual2<float>(Rt, &pq[8 * k], &pq[8 * k + 4]);
        mask[k] = r2 <= max_dist2 ? 1 : 0;
        if (mask[k]) { n_in++; sse += (double)r2; }
    }
    // into the caller's coordinates: x -> R (x - cs) + t + ct
    double T[16];
    for (int k = 0; k < 16; k++) T[k] = k == 15 ? 1.0 : 0.0;
    for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) T[4 * a + b] = (double)Rt[3 * a + b];
        T[4 * a + 3] = ((double)Rt[9 + a] + (double)ct[a]) - ((double)Rt[3 * a] * cs[0] + (double)Rt[3 * a + 1] * cs[1] + (double)Rt[3 * a + 2] * cs[2]);
    }
    const double md2 = (double)cfg.max_dist * (double)cfg.max_dist;
    int st = SYMMICP_OK;
    for (int r = 0; r < cfg.refits; r++) {
        horn_fit(X, Y, mask, T);
        n_in = inliers64(X, Y, T, md2, mask, &sse);
        if (n_in < 3) { st = SYMMICP_ERR_NO_CONSENSUS; break; }
    }
    if (st != SYMMICP_OK) {
        const int32_t hbest = res->best_hypothesis, ir = res->inliers_ransac, ev = res->evaluated;
        set_identity_result(transform16, res);
        res->best_hypothesis = hbest; res->inliers_ransac = ir; res->evaluated = ev;
        if (mask_out) std::memset(mask_out, 0, m);
        return fail(c, st, "ransac: a refit left fewer than 3 inliers");
    }
    res->inliers_final = (int32_t)n_in;
    res->rmse_final = std::sqrt(sse / (double)n_in);
    for (int k = 0; k < 16; k++) { res->transform[k] = T[k]; transform16[k] = (float)T[k]; }
    if (mask_out) std::memcpy(mask_out, mask.data(), m);
    return SYMMICP_OK;
}

extern "C" {

void symmicp_ransac_config_default(symmicp_ransac_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->hypotheses = 100000;
    cfg->seed = 0;
    cfg->max_dist = 0.f;
    cfg->edge_ratio = 0.9f;
    cfg->refits = 1;
}

int symmicp_ctx_ransac(symmicp_ctx *c, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns, const float *tgt_xyz,
                       size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const int32_t *pairs, size_t m, const symmicp_ransac_config *cfg,
                       float transform16[16], symmicp_ransac_result *result, uint8_t *inlier_mask_out, uint8_t *status_out, int32_t *inliers_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!transform16 || !result) return fail(c, SYMMICP_ERR_ARG, "ransac: transform16 and result are required");
    if (const char *msg = ransac_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg)) return fail(c, SYMMICP_ERR_ARG, msg);
    set_identity_result(transform16, result);
    return ransac_run(c, src_xyz, src_row_stride, src_col_stride, tgt_xyz, tgt_row_stride, tgt_col_stride, pairs, m, *cfg, transform16, result,
                      inlier_mask_out, status_out, inliers_out, nullptr, nullptr);
}

int symmicp_ctx_ransac_hypotheses(symmicp_ctx *c, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                                  const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const int32_t *pairs, size_t m,
                                  const symmicp_ransac_config *cfg, float *hyp_out, uint8_t *status_out, float pivots_out[6])
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!hyp_out) return fail(c, SYMMICP_ERR_ARG, "ransac_hypotheses: hyp_out is required");
    if (const char *msg = ransac_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg)) return fail(c, SYMMICP_ERR_ARG, msg);
    return ransac_run(c, src_xyz, src_row_stride, src_col_stride, tgt_xyz, tgt_row_stride, tgt_col_stride, pairs, m, *cfg, nullptr, nullptr, nullptr,
                      status_out, nullptr, hyp_out, pivots_out);
}

// ---- the same three on a context of their own ----
int symmicp_feature_nn(int device, const float *fa, size_t na, const float *fb, size_t nb, int32_t *nn_out, float *d2_out, float *d2_second_out)
{
    if (!nn_out || features_error(fa, na, fb, nb)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_feature_nn(c, fa, na, fb, nb, nn_out, d2_out, d2_second_out);
    });
}

int symmicp_feature_correspondences(int device, const float *fa, size_t na, const float *fb, size_t nb, int mutual, float max_ratio,
                                    int32_t *pairs_out, float *d2_out, size_t cap, size_t *count_out)
{
    if (corr_args_error(fa, na, fb, nb, max_ratio, pairs_out, cap, count_out)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_feature_correspondences(c, fa, na, fb, nb, mutual, max_ratio, pairs_out, d2_out, cap, count_out);
    });
}

int symmicp_ransac(int device, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns, const float *tgt_xyz,
                   size_t tgt_row_stride, size_t tgt_col_stride, size_t nt, const int32_t *pairs, size_t m, const symmicp_ransac_config *cfg,
                   float transform16[16], symmicp_ransac_result *result, uint8_t *inlier_mask_out, uint8_t *status_out, int32_t *inliers_out)
{
    if (!transform16 || !result || ransac_args_error(src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_ransac(c, src_xyz, src_row_stride, src_col_stride, ns, tgt_xyz, tgt_row_stride, tgt_col_stride, nt, pairs, m, cfg, transform16,
                                  result, inlier_mask_out, status_out, inliers_out);
    });
}

}  // extern "C"
