// engine_posegraph.cpp -- host side of the pose-graph optimiser (symmicp_ctx_posegraph_optimize, symmicp_posegraph_optimize,
// symmicp_ctx_posegraph_pass and the two host helpers; kernels_posegraph.hip has the kernel, include/symmicp.h the contract): argument
// checks that need no device, the connectivity check, the incidence list, the upload, the Levenberg-Marquardt control loop on one
// record per launch, the result.  Temporaries come from the context's arena only: its clouds, index, options and states are not touched.
#include "engine_internal.h"
#include "posegraph_core.h"

namespace {

bool finite_pos(double v) { return std::isfinite(v) && v > 0.0; }
bool finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// the top three rows of a row-major 4x4: finite, and the rotation block orthonormal to 1e-6
const char *rigid_error(const double *X)
{
    for (int k = 0; k < 12; k++) if (!std::isfinite(X[k])) return "a pose or an edge transform holds a non-finite value";
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double d = (X[i] * X[j] + X[4 + i] * X[4 + j]) + X[8 + i] * X[8 + j] - (i == j ? 1.0 : 0.0);
            if (!(std::fabs(d) <= 1e-6)) return "a rotation block is not orthonormal (max |R^T R - I| > 1e-6)";
        }
    return nullptr;
}

const char *graph_error(const double *poses, size_t n, const symmicp_pose_edge *edges, size_t m, int32_t ref)
{
    if (!poses || !edges) return "posegraph: poses and edges are required";
    if (n < 2 || n > SYMMICP_POSEGRAPH_MAX_NODES) return "posegraph: n must be in 2 .. 1024";
    if (m < 1 || m > SYMMICP_POSEGRAPH_MAX_EDGES) return "posegraph: m must be in 1 .. 16384";
    if (ref < 0 || (size_t)ref >= n) return "posegraph: reference_node is out of range";
    for (size_t e = 0; e < m; e++) {
        const symmicp_pose_edge &E = edges[e];
        if (E.source < 0 || (size_t)E.source >= n || E.target < 0 || (size_t)E.target >= n) return "posegraph: an edge names a node out of range";
        if (E.source == E.target) return "posegraph: an edge joins a node to itself";
    }
    // connected: union-find over the edges
    std::vector<int32_t> root(n);
    for (size_t i = 0; i < n; i++) root[i] = (int32_t)i;
    auto find = [&](int32_t i) { while (root[i] != i) { root[i] = root[root[i]]; i = root[i]; } return i; };
    size_t parts = n;
    for (size_t e = 0; e < m; e++) {
        const int32_t a = find(edges[e].source), b = find(edges[e].target);
        if (a != b) { root[a] = b; parts--; }
    }
    if (parts != 1) return "posegraph: the graph is not connected";
    for (size_t i = 0; i < n; i++)
        if (const char *msg = rigid_error(poses + 16 * i)) return msg;
    for (size_t e = 0; e < m; e++) {
        if (const char *msg = rigid_error(edges[e].transform)) return msg;
        for (int i = 0; i < 6; i++)
            for (int j = i; j < 6; j++)
                if (!std::isfinite(edges[e].information[6 * i + j])) return "posegraph: an information matrix holds a non-finite value";
    }
    return nullptr;
}

bool any_uncertain(const symmicp_pose_edge *edges, size_t m)
{
    for (size_t e = 0; e < m; e++) if (edges[e].uncertain) return true;
    return false;
}

const char *optimize_args_error(const double *poses, size_t n, const symmicp_pose_edge *edges, size_t m, const symmicp_posegraph_config *cfg,
                                const double *poses_out, const symmicp_posegraph_result *res)
{
    if (!poses || !edges || !cfg || !poses_out || !res) return "posegraph: poses_in, edges, cfg, poses_out and result are required";
    if (cfg->struct_size != sizeof(symmicp_posegraph_config)) return "posegraph: cfg->struct_size is not sizeof(symmicp_posegraph_config)";
    if (cfg->max_iterations < 1 || cfg->max_iterations > 10000) return "posegraph: max_iterations must be in 1 .. 10000";
    if (cfg->cg_max_iterations < 0 || cfg->cg_max_iterations > 100000) return "posegraph: cg_max_iterations must be in 0 .. 100000";
    if (!finite_nonneg(cfg->line_process_weight)) return "posegraph: line_process_weight must be finite and >= 0";
    if (!(cfg->edge_prune_threshold >= 0.0 && cfg->edge_prune_threshold <= 1.0)) return "posegraph: edge_prune_threshold must be in [0, 1]";
    if (!finite_nonneg(cfg->min_relative_decrease)) return "posegraph: min_relative_decrease must be finite and >= 0";
    if (!finite_nonneg(cfg->min_increment)) return "posegraph: min_increment must be finite and >= 0";
    if (!(cfg->cg_tolerance > 0.0 && cfg->cg_tolerance < 1.0)) return "posegraph: cg_tolerance must be in (0, 1)";
    if (const char *msg = graph_error(poses, n, edges, m, cfg->reference_node)) return msg;
    if (cfg->line_process_weight == 0.0 && any_uncertain(edges, m)) {
        if (!finite_pos(cfg->max_dist)) return "posegraph: max_dist must be finite and > 0 to derive mu";
        if (!finite_pos(cfg->preference_loop_closure)) return "posegraph: preference_loop_closure must be finite and > 0 to derive mu";
    }
    return nullptr;
}

const char *pass_args_error(const double *poses, size_t n, const symmicp_pose_edge *edges, size_t m, int32_t ref, double mu, double lambda,
                            double cg_tol, int32_t cg_max)
{
    if (!finite_pos(mu)) return "posegraph_pass: mu must be finite and > 0";
    if (!finite_nonneg(lambda)) return "posegraph_pass: lambda must be finite and >= 0";
    if (!(cg_tol > 0.0 && cg_tol < 1.0)) return "posegraph_pass: cg_tolerance must be in (0, 1)";
    if (cg_max < 0 || cg_max > 100000) return "posegraph_pass: cg_max_iterations must be in 0 .. 100000";
    return graph_error(poses, n, edges, m, ref);
}

// the graph in device memory and everything a launch writes, all from the context's arena
struct PgDevice {
    DevBuf<double> X[2], T, L, e, ce, l, l_trial, slot_v, slot_h, g, hdiag, chol, x, r, z, p;
    DevBuf<int32_t> es, et, eunc;
    DevBuf<uint32_t> off, slot_s, slot_t;
    DevBuf<PgRecord> rec;
    PgArgs a{};
    int cur = 0;          // X[cur]: the poses of the next launch; X[1 - cur]: its trial poses

    int setup(symmicp_ctx *c, const double *poses, size_t n, const symmicp_pose_edge *edges, size_t m, int32_t ref)
    {
        // host side: the top rows of the poses, the planar edge data, the incidence list sorted by (node, edge index) and the slots
        std::vector<double> hX(12 * n), hT(12 * m), hL(21 * m);
        std::vector<int32_t> hs(m), ht(m), hu(m);
        std::vector<uint32_t> hoff(n + 1, 0), hss(m), hst(m);
        for (size_t i = 0; i < n; i++) std::memcpy(&hX[12 * i], poses + 16 * i, sizeof(double) * 12);
        for (size_t k = 0; k < m; k++) {
            const symmicp_pose_edge &E = edges[k];
            hs[k] = E.source; ht[k] = E.target; hu[k] = E.uncertain ? 1 : 0;
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) hT[(size_t)(3 * i + j) * m + k] = E.transform[4 * i + j];
                hT[(size_t)(9 + i) * m + k] = E.transform[4 * i + 3];
            }
            for (int i = 0; i < 6; i++)
                for (int j = i; j < 6; j++) hL[(size_t)pg::tri(i, j) * m + k] = E.information[6 * i + j];
            hoff[E.source + 1]++; hoff[E.target + 1]++;
        }
        for (size_t i = 0; i < n; i++) hoff[i + 1] += hoff[i];
        std::vector<uint32_t> fill(hoff.begin(), hoff.end() - 1);
        for (size_t k = 0; k < m; k++) { hss[k] = fill[hs[k]]++; hst[k] = fill[ht[k]]++; }      // ascending k: every row sorted by edge index

        HIP_TRY(c, hipSetDevice(c->device));
        arena_begin(c->arena, sizeof(double) * (24 * n + 33 * m + 9 * m + 12 * m + 72 * m + 6 * n + 36 * n + 21 * n + 24 * n) + 4 * (6 * m + n + 1) +
                                  sizeof(PgRecord) + 32 * 256);
        HIP_TRY(c, X[0].alloc_temp(c->arena, 12 * n)); HIP_TRY(c, X[1].alloc_temp(c->arena, 12 * n));
        HIP_TRY(c, T.alloc_temp(c->arena, 12 * m)); HIP_TRY(c, L.alloc_temp(c->arena, 21 * m));
        HIP_TRY(c, e.alloc_temp(c->arena, 6 * m)); HIP_TRY(c, ce.alloc_temp(c->arena, m));
        HIP_TRY(c, l.alloc_temp(c->arena, m)); HIP_TRY(c, l_trial.alloc_temp(c->arena, m));
        HIP_TRY(c, slot_v.alloc_temp(c->arena, 12 * m)); HIP_TRY(c, slot_h.alloc_temp(c->arena, 72 * m));
        HIP_TRY(c, g.alloc_temp(c->arena, 6 * n)); HIP_TRY(c, hdiag.alloc_temp(c->arena, 36 * n)); HIP_TRY(c, chol.alloc_temp(c->arena, 21 * n));
        HIP_TRY(c, x.alloc_temp(c->arena, 6 * n)); HIP_TRY(c, r.alloc_temp(c->arena, 6 * n));
        HIP_TRY(c, z.alloc_temp(c->arena, 6 * n)); HIP_TRY(c, p.alloc_temp(c->arena, 6 * n));
        HIP_TRY(c, es.alloc_temp(c->arena, m)); HIP_TRY(c, et.alloc_temp(c->arena, m)); HIP_TRY(c, eunc.alloc_temp(c->arena, m));
        HIP_TRY(c, off.alloc_temp(c->arena, n + 1)); HIP_TRY(c, slot_s.alloc_temp(c->arena, m)); HIP_TRY(c, slot_t.alloc_temp(c->arena, m));
        HIP_TRY(c, rec.alloc_temp(c->arena, 1));
        // (pageable host memory: each of these copies has left its host buffer when the call returns)
        HIP_TRY(c, hipMemcpyAsync(X[0].p, hX.data(), sizeof(double) * 12 * n, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(T.p, hT.data(), sizeof(double) * 12 * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(L.p, hL.data(), sizeof(double) * 21 * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(es.p, hs.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(et.p, ht.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(eunc.p, hu.data(), sizeof(int32_t) * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(off.p, hoff.data(), sizeof(uint32_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(slot_s.p, hss.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipMemcpyAsync(slot_t.p, hst.data(), sizeof(uint32_t) * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));

        a.n = (uint32_t)n; a.m = (uint32_t)m; a.ref = ref;
        a.es = es.p; a.et = et.p; a.eunc = eunc.p; a.T = T.p; a.L = L.p; a.off = off.p; a.slot_s = slot_s.p; a.slot_t = slot_t.p;
        a.e = e.p; a.c = ce.p; a.l = l.p; a.l_trial = l_trial.p; a.slot_v = slot_v.p; a.slot_h = slot_h.p;
        a.g = g.p; a.hdiag = hdiag.p; a.chol = chol.p; a.x = x.p; a.r = r.p; a.z = z.p; a.p = p.p; a.rec = rec.p;
        return SYMMICP_OK;
    }

    // one launch at X[cur] with (mu, lambda): the record
    int launch(symmicp_ctx *c, double mu, double lambda, double cg_tol, int32_t cg_max, PgRecord &out)
    {
        a.X = X[cur].p; a.Xtrial = X[1 - cur].p;
        a.mu = mu; a.lambda = lambda; a.cg_tol = cg_tol;
        a.cg_max = cg_max > 0 ? cg_max : 6 * ((int32_t)a.n - 1);
        launch_posegraph_iteration(a, c->stream);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipMemcpyAsync(&out, rec.p, sizeof(out), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return SYMMICP_OK;
    }
};

void fill_iteration(const PgRecord &r, int accepted, symmicp_posegraph_iteration &o)
{
    o.cost = r.cost; o.cost_trial = r.cost_trial; o.model_decrease = r.model_decrease; o.grad_max = r.grad_max; o.delta_max = r.delta_max;
    o.hdiag_max = r.hdiag_max; o.lambda = r.lambda; o.cg_residual = r.cg_residual;
    o.cg_iterations = r.cg_iterations; o.accepted = accepted; o.status = r.status; o.reserved = 0;
}

template <typename T>
int download(symmicp_ctx *c, T *dst, const T *src, size_t count)
{
    if (dst) HIP_TRY(c, hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost, c->stream));
    return SYMMICP_OK;
}

int optimize_run(symmicp_ctx *c, const double *poses_in, size_t n, const symmicp_pose_edge *edges, size_t m, const symmicp_posegraph_config &cfg,
                 double *poses_out, symmicp_posegraph_result *res, double *weight_out, uint8_t *pruned_out, symmicp_posegraph_iteration *trace_out)
{
    // mu, in fp64 on the host
    double mu = cfg.line_process_weight;
    const bool has_uncertain = any_uncertain(edges, m);
    if (!(mu > 0.0) && has_uncertain) {
        double sum = 0.0;
        for (size_t e = 0; e < m; e++) sum += edges[e].information[35];
        mu = cfg.preference_loop_closure * (cfg.max_dist * cfg.max_dist) * (sum / (double)m);
        if (!finite_pos(mu)) return fail(c, SYMMICP_ERR_ARG, "posegraph: the derived mu is not finite and > 0 (the mean of information[35] must be > 0)");
    }
    double ref_pose[16];
    std::memcpy(ref_pose, poses_in + 16 * (size_t)cfg.reference_node, sizeof(ref_pose));      // (poses_out may be poses_in)

    std::memset(res, 0, sizeof(*res));
    res->mu = mu;
    PgDevice d;
    if (const int st = d.setup(c, poses_in, n, edges, m, cfg.reference_node)) return res->status = st;

    // the device needs a mu > 0 even when no edge reads it
    const double mu_dev = has_uncertain ? mu : 1.0;
    double lambda = -1.0, nu = 2.0;      // (< 0: the first launch derives lambda_0 and reports it)
    int status = SYMMICP_OK, reason = 0;
    bool last_accepted = false;
    while (true) {
        PgRecord r;
        if (const int st = d.launch(c, mu_dev, lambda, cfg.cg_tolerance, cfg.cg_max_iterations, r)) return res->status = st;
        if (res->iterations == 0) res->cost_initial = res->cost_final = r.cost;
        if (r.status != SYMMICP_OK) {
            if (trace_out) fill_iteration(r, 0, trace_out[res->iterations]);
            res->iterations++;
            status = SYMMICP_ERR_DEGENERATE;
            last_accepted = false;
            break;
        }
        lambda = r.lambda;
        const bool accepted = r.cost_trial < r.cost;
        if (trace_out) fill_iteration(r, accepted ? 1 : 0, trace_out[res->iterations]);
        res->iterations++;
        res->cg_iterations += r.cg_iterations;
        res->grad_max = r.grad_max;
        last_accepted = accepted;
        bool stop = false;
        if (accepted) {
            const double rho = (r.cost - r.cost_trial) / r.model_decrease;
            const double q = 2.0 * rho - 1.0;
            lambda = lambda * std::max(1.0 / 3.0, 1.0 - q * q * q);
            nu = 2.0;
            d.cur = 1 - d.cur;
            res->accepted_steps++;
            res->cost_final = r.cost_trial;
            if (r.cost - r.cost_trial <= cfg.min_relative_decrease * r.cost) { stop = true; reason = 2; }
        } else {
            lambda = lambda * nu;
            nu = 2.0 * nu;
        }
        if (!stop && r.delta_max <= cfg.min_increment) { stop = true; reason = 3; }
        if (!stop && res->iterations >= cfg.max_iterations) { stop = true; reason = 1; }
        if (stop) break;
    }
    res->stop_reason = reason;
    res->lambda_final = lambda;

    // the poses, the weights at them, the pruned closures
    std::vector<double> hX(12 * n), hl(m);
    HIP_TRY(c, hipMemcpyAsync(hX.data(), d.X[d.cur].p, sizeof(double) * 12 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(hl.data(), last_accepted ? d.l_trial.p : d.l.p, sizeof(double) * m, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    for (size_t i = 0; i < n; i++) {
        if (i == (size_t)cfg.reference_node) { std::memcpy(poses_out + 16 * i, ref_pose, sizeof(ref_pose)); continue; }
        std::memcpy(poses_out + 16 * i, &hX[12 * i], sizeof(double) * 12);
        poses_out[16 * i + 12] = 0.0; poses_out[16 * i + 13] = 0.0; poses_out[16 * i + 14] = 0.0; poses_out[16 * i + 15] = 1.0;
    }
    for (size_t e = 0; e < m; e++) {
        const bool pruned = edges[e].uncertain && hl[e] < cfg.edge_prune_threshold;
        if (pruned) res->pruned++;
        if (pruned_out) pruned_out[e] = pruned ? 1 : 0;
        if (weight_out) weight_out[e] = hl[e];
    }
    res->status = status;
    if (status != SYMMICP_OK)
        return fail(c, status, "posegraph: a node block H_ii + lambda I is not finite or not positive definite in iteration " + std::to_string(res->iterations));
    return SYMMICP_OK;
}

}  // namespace

extern "C" {

void symmicp_posegraph_config_default(symmicp_posegraph_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (uint32_t)sizeof(*cfg);
    cfg->max_iterations = 100;
    cfg->reference_node = 0;
    cfg->cg_max_iterations = 0;
    cfg->max_dist = 0.0;
    cfg->preference_loop_closure = 1.0;
    cfg->line_process_weight = 0.0;
    cfg->edge_prune_threshold = 0.25;
    cfg->min_relative_decrease = 1e-6;
    cfg->min_increment = 1e-9;
    cfg->cg_tolerance = 1e-10;
}

int symmicp_ctx_posegraph_optimize(symmicp_ctx *c, const double *poses_in, size_t n, const symmicp_pose_edge *edges, size_t m,
                                   const symmicp_posegraph_config *cfg, double *poses_out, symmicp_posegraph_result *result, double *weight_out,
                                   uint8_t *pruned_out, symmicp_posegraph_iteration *trace_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = optimize_args_error(poses_in, n, edges, m, cfg, poses_out, result)) return fail(c, SYMMICP_ERR_ARG, msg);
    if (c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "posegraph: not on a sharded context");
    return optimize_run(c, poses_in, n, edges, m, *cfg, poses_out, result, weight_out, pruned_out, trace_out);
}

int symmicp_posegraph_optimize(int device, const double *poses_in, size_t n, const symmicp_pose_edge *edges, size_t m,
                               const symmicp_posegraph_config *cfg, double *poses_out, symmicp_posegraph_result *result, double *weight_out,
                               uint8_t *pruned_out, symmicp_posegraph_iteration *trace_out)
{
    if (optimize_args_error(poses_in, n, edges, m, cfg, poses_out, result)) return SYMMICP_ERR_ARG;
    return with_own_context(device, [&](symmicp_ctx *c) {
        return symmicp_ctx_posegraph_optimize(c, poses_in, n, edges, m, cfg, poses_out, result, weight_out, pruned_out, trace_out);
    });
}

int symmicp_ctx_posegraph_pass(symmicp_ctx *c, const double *poses, size_t n, const symmicp_pose_edge *edges, size_t m, int32_t reference_node,
                               double mu, double lambda, double cg_tolerance, int32_t cg_max_iterations, double *e_out, double *c_out,
                               double *l_out, double *g_out, double *hdiag_out, double *delta_out, symmicp_posegraph_iteration *record_out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (const char *msg = pass_args_error(poses, n, edges, m, reference_node, mu, lambda, cg_tolerance, cg_max_iterations)) return fail(c, SYMMICP_ERR_ARG, msg);
    if (c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "posegraph_pass: not on a sharded context");
    PgDevice d;
    if (const int st = d.setup(c, poses, n, edges, m, reference_node)) return st;
    PgRecord r;
    if (const int st = d.launch(c, mu, lambda, cg_tolerance, cg_max_iterations, r)) return st;
    if (r.status != SYMMICP_OK) return fail(c, SYMMICP_ERR_DEGENERATE, "posegraph_pass: a node block H_ii + lambda I is not finite or not positive definite");
    if (int st = download(c, e_out, d.e.p, 6 * m)) return st;
    if (int st = download(c, c_out, d.ce.p, m)) return st;
    if (int st = download(c, l_out, d.l.p, m)) return st;
    if (int st = download(c, g_out, d.g.p, 6 * n)) return st;
    if (int st = download(c, hdiag_out, d.hdiag.p, 36 * n)) return st;
    if (int st = download(c, delta_out, d.x.p, 6 * n)) return st;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    if (record_out) fill_iteration(r, 0, *record_out);
    return SYMMICP_OK;
}

int symmicp_posegraph_edge_error(const double Xs16[16], const double Xt16[16], const double T16[16], double e6_out[6])
{
    if (!Xs16 || !Xt16 || !T16 || !e6_out) return SYMMICP_ERR_ARG;
    double RT[9], tT[3], RE[9];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) RT[3 * i + j] = T16[4 * i + j];
        tT[i] = T16[4 * i + 3];
    }
    pg::edge_E(Xs16, Xt16, RT, tT, RE, e6_out + 3);
    pg::log_rot(RE, e6_out);
    return SYMMICP_OK;
}

double symmicp_posegraph_line_weight(double mu, double c)
{
    return pg::line_weight(mu, c);
}

}  // extern "C"
