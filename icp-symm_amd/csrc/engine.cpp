// engine.cpp -- host side of libsymmicp: the C-ABI of include/symmicp.h.
//
// Host C++ owns control flow and the 6x6 / 3x3 solve (host_solve.cpp); the GPU owns
// every O(N) pass (kernels_pass.hip) and the one-time index build (kernels_build.hip).
// Per iteration of the reference loop (ICP/myicp.cpp:123-142) the host does:
//   solve(last sums) -> 4x4 increment -> launch the pass (one streaming kernel for identity pairing; search + accumulate
//   kernels for the nearest-neighbour modes) + the final reduce -> [RCCL all-reduce of 40 doubles when sharded] ->
//   spin on the record's sequence word in host-mapped memory -> repeat.
// There is no CPU fallback: without a HIP device every entry point fails loudly.
#include "engine_internal.h"
#include "robust_loss.h"

void read_switches(Switches &w)
{
    auto flag = [](const char *n) { return std::getenv(n) != nullptr; };
    auto num = [](const char *n, long def) { const char *e = std::getenv(n); return e ? std::atol(e) : def; };
    auto tri = [](const char *n) { const char *e = std::getenv(n); return e ? (e[0] == '1' ? 1 : 0) : -1; };
    w.allow_any_arch = flag("SYMMICP_ALLOW_ANY_ARCH");
    w.debug_host = flag("SYMMICP_DEBUG_HOST");
    w.debug_counters = flag("SYMMICP_DEBUG_COUNTERS");
    if (const char *e = std::getenv("SYMMICP_DEBUG_TRACE")) w.debug_trace = e;
    if (const char *e = std::getenv("SYMMICP_GRID_PPC")) w.grid_ppc = std::atof(e);
    w.grid_maxlevel = (int)num("SYMMICP_GRID_MAXLEVEL", kMortonBits);
    w.grid_level = (int)num("SYMMICP_GRID_LEVEL", -1);
    if (const char *e = std::getenv("SYMMICP_FIRST_PASS")) w.first_pass = (e[0] == 'p') ? 1 : 0;      // "packet" / "walk"
    w.oct_leaf = (int)num("SYMMICP_OCT_LEAF", 0);
    if (const char *e = std::getenv("SYMMICP_PACKET_ORDER")) w.packet_order = e[0] != '0';
    if (const char *e = std::getenv("SYMMICP_PACKET_JUMP")) w.packet_jump = (float)std::atof(e);
    w.packet_key_bits = (int)num("SYMMICP_PACKET_KEY_BITS", 16);
    w.packet_chunk = (uint32_t)num("SYMMICP_PACKET_CHUNK", 0);
    w.packet_lds_pad = (uint32_t)num("SYMMICP_PACKET_LDS_PAD", 0);
    w.packet_waves = (uint32_t)num("SYMMICP_PACKET_WAVES", 0);
    w.packet_front_cap = (uint32_t)num("SYMMICP_PACKET_FRONT_CAP", 0);
    if (const char *e = std::getenv("SYMMICP_HOOD_FRAC")) w.hood_frac = std::atof(e);
    w.no_hood = flag("SYMMICP_NO_NEIGHBOURHOOD");
    w.no_cert = flag("SYMMICP_NO_CERT");
    w.walk_full_grid = flag("SYMMICP_WALK_FULL_GRID");
    { const char *e = std::getenv("SYMMICP_HOST_LOOP"); w.host_loop = e && e[0] == '1'; }
    w.no_loop_stragglers = flag("SYMMICP_NO_LOOP_STRAGGLERS");
    w.force_comm = flag("SYMMICP_FORCE_COMM");
    if (const char *e = std::getenv("SYMMICP_PACKET_COST_KEY")) w.packet_cost_key = e[0] != '0';
    w.budget_walk = tri("SYMMICP_BUDGET_WALK");
    w.optimistic = tri("SYMMICP_OPTIMISTIC");
    w.compact = tri("SYMMICP_COMPACT");
    w.cert_pass = (int)num("SYMMICP_CERT_PASS", 1);
    w.cert_head = (int)num("SYMMICP_CERT_HEAD", 4);
    w.pass_blocks = (int)num("SYMMICP_PASS_BLOCKS", 2048);
    w.id_blocks = (int)num("SYMMICP_ID_BLOCKS", 2048);
    w.acc_blocks = (int)num("SYMMICP_ACC_BLOCKS", 512);
    w.fused_blocks = (int)num("SYMMICP_FUSED_BLOCKS", 512);
    w.compact_blocks = (int)num("SYMMICP_COMPACT_BLOCKS", 1280);
    w.feature_nn_splits = (int)num("SYMMICP_FEATURE_NN_SPLITS", 0);
    w.feature_nn_queries = (int)num("SYMMICP_FEATURE_NN_QUERIES", 0);
    w.plane_score = (int)num("SYMMICP_PLANE_SCORE", 0);
    w.tune.wave_mode_max =(uint32_t)num("SYMMICP_WAVE_MODE_MAX", 20000);
    w.tune.cells_chunk = (uint32_t)num("SYMMICP_CELLS_CHUNK", 16);
    w.tune.cells_queries = (uint32_t)num("SYMMICP_CELLS_QUERIES", 0);
    w.tune.walk_budget = (uint32_t)num("SYMMICP_WALK_BUDGET", 160);
}

// rewind the arena and make sure it holds `want` bytes (contents are dead: called at the start of a public call)
void arena_begin(Arena &a, size_t want)
{
    a.off = 0;
    if (a.cap >= want) return;
    if (a.base) hipFree(a.base);
    a.base = nullptr; a.cap = 0;
    const size_t cap = want + want / 4;
    if (hipMalloc((void **)&a.base, cap) == hipSuccess) a.cap = cap;      // on failure every alloc_temp falls back to hipMalloc
    else (void)hipGetLastError();
}


extern "C" {

int symmicp_version(void) { return 100; }

void symmicp_config_default(symmicp_config *cfg)
{
    if (!cfg) return;
    std::memset(cfg, 0, sizeof(*cfg));
    cfg->struct_size = (int32_t)sizeof(*cfg);
    cfg->device = -1;
    cfg->mode = SYMMICP_MODE_QUIRKS;
    cfg->corr = SYMMICP_CORR_IDENTITY;
    cfg->apply = SYMMICP_APPLY_DEFAULT;
    cfg->max_iters = 10;            // myicp.cpp:6
    cfg->diff_threshold = 1.0f;     // myicp.cpp:6
    cfg->max_corr_dist = 0.f;
    cfg->fixed_iters = 0;
    cfg->sort_source = 1;
    cfg->verbose = 0;
    cfg->min_normal_dot = -2.0f;
    cfg->eps_rotation = 0.f;
    cfg->eps_translation = 0.f;
}

static int check_cfg(const symmicp_config *cfg)
{
    if (!cfg || cfg->struct_size != (int32_t)sizeof(symmicp_config)) return SYMMICP_ERR_ARG;
    if (!mode_known(cfg->mode)) return SYMMICP_ERR_ARG;
    if (cfg->corr < SYMMICP_CORR_IDENTITY || cfg->corr > SYMMICP_CORR_TREE) return SYMMICP_ERR_ARG;
    if (cfg->apply < SYMMICP_APPLY_DEFAULT || cfg->apply > SYMMICP_APPLY_CUMULATIVE) return SYMMICP_ERR_ARG;
    if (cfg->max_iters < 0) return SYMMICP_ERR_ARG;
    if (cfg->mode == SYMMICP_MODE_NDT && ndt_config_refusal(*cfg)) return SYMMICP_ERR_ARG;
    return SYMMICP_OK;
}

int symmicp_create(const symmicp_config *cfg, symmicp_ctx **out)
{
    if (!out) return SYMMICP_ERR_ARG;
    *out = nullptr;
    if (check_cfg(cfg) != SYMMICP_OK) return SYMMICP_ERR_ARG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return SYMMICP_ERR_HIP;   // no CPU fallback
    symmicp_ctx *c = new symmicp_ctx();
    read_switches(c->sw);
    c->cfg = *cfg;
    if (cfg->device >= 0) {
        if (cfg->device >= ndev || hipSetDevice(cfg->device) != hipSuccess) { delete c; return SYMMICP_ERR_HIP; }
        c->device = cfg->device;
    } else if (hipGetDevice(&c->device) != hipSuccess) { delete c; return SYMMICP_ERR_HIP; }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c->device) != hipSuccess) { delete c; return SYMMICP_ERR_HIP; }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0 && !c->sw.allow_any_arch) {
        // the code object only carries gfx950 ISA
        delete c;
        return SYMMICP_ERR_HIP;
    }
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return SYMMICP_ERR_HIP; }
    bool ok = hipMalloc((void **)&c->partials, sizeof(double) * kNSum * 8192) == hipSuccess &&
              hipMalloc((void **)&c->d_sums, sizeof(double) * kNSum) == hipSuccess &&
              hipHostMalloc((void **)&c->h_sums, sizeof(double) * (kNSum + 8), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipMalloc((void **)&c->ticket, 2 * sizeof(uint32_t)) == hipSuccess && hipMemset(c->ticket, 0, 2 * sizeof(uint32_t)) == hipSuccess &&
              hipHostGetDevicePointer((void **)&c->h_sums_dev, c->h_sums, 0) == hipSuccess &&
              std::memset(c->h_sums, 0, sizeof(double) * (kNSum + 8)) != nullptr &&
              hipMalloc((void **)&c->d_loop, sizeof(LoopState)) == hipSuccess &&
              hipHostMalloc((void **)&c->h_loop, sizeof(LoopState), hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void **)&c->h_loop_dev, c->h_loop, 0) == hipSuccess &&
              hipHostMalloc((void **)&c->h_ring, sizeof(LoopRecord) * symmicp_ctx::kRing, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void **)&c->h_ring_dev, c->h_ring, 0) == hipSuccess &&
              hipHostMalloc((void **)&c->h_done, 64, hipHostMallocMapped | hipHostMallocCoherent) == hipSuccess &&
              hipHostGetDevicePointer((void **)&c->h_done_dev, c->h_done, 0) == hipSuccess &&
              std::memset(c->h_done, 0, 64) != nullptr &&
              true;
    for (int k = 0; ok && k < symmicp_ctx::kEvRing * symmicp_ctx::kEvPer; k++) ok = hipEventCreateWithFlags(&c->ev[k], hipEventDisableSystemFence) == hipSuccess;      // timing only: no system-scope cache flush per record
    if (!ok) { symmicp_destroy(c); return SYMMICP_ERR_HIP; }
    c->pkt_fallbacks = c->ticket + 1;
    symmicp_ndt_config_default(&c->ndt.cfg);
    symmicp_ndt_gauss((double)c->ndt.cfg.outlier_ratio, &c->ndt.d1, &c->ndt.d2);
    identity16(c->X);
    *out = c;
    return SYMMICP_OK;
}

extern "C++" void free_target(symmicp_ctx *c)
{
    c->tgt_store.reset();      // (the arrays live in its block, which stays allocated for the next target)
    hipFree(c->ix.dbg); hipFree(c->ix.dbg_trace);
    c->ix = TargetIndex{}; c->tgt_block = nullptr;
    c->have_index = false; c->target_surface_like = false; c->n_t = 0;
    c->have_tgt_color = false;
    c->ndt.map.valid = false; c->ndt.pass_valid = false;
    c->notes = IndexNotes{};
}

extern "C++" void forget_source(symmicp_ctx *c)
{
    // (the arrays live in one block, c->src_all, which is kept for the next source of the same or a smaller size)
    c->worklist = c->wl_count = nullptr; c->cert = nullptr; c->certk = nullptr; c->hoodr = nullptr; c->pkt_tab = nullptr; c->pkt_count = 0; c->pkt_cost_keyed = false; c->pairrec = nullptr;
    c->src0_block = c->cur_block = nullptr; c->src_order = nullptr; c->pos = nullptr; c->d2 = nullptr; c->best64 = nullptr;
    c->n_loc = c->n_s_total = c->src_off = 0;
    c->src_no_normals = false;
    c->have_src_int = false;
    c->rej.src_ix.drop();
}

static void free_source(symmicp_ctx *c)
{
    forget_source(c);
    hipFree(c->src_all);
    c->src_all = nullptr; c->src_all_cap = 0;
}

void symmicp_destroy(symmicp_ctx *c)
{
    if (!c) return;
    if (c->sw.debug_host && c->n_pass_timed)
        std::fprintf(stderr, "[symmicp host] passes %ld: launch %.1f us, spin %.1f us, between passes %.1f us (per pass)\n", c->n_pass_timed, 1e6 * c->t_launch / c->n_pass_timed, 1e6 * c->t_spin / c->n_pass_timed, 1e6 * c->t_between / c->n_pass_timed);
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    shm_close(c);
    free_target(c);
    free_source(c);
    hipFree(c->partials); hipFree(c->d_sums); hipFree(c->ticket); hipFree(c->arena.base);
    hipFree(c->rej.keys); hipFree(c->rej.ws); hipFree(c->rej.table);
    hipFree(c->tgt_color); hipFree(c->src_int);
    c->ndt.map.release();
    c->tgt_store.release(); c->rej.src_ix.store.release();      // (their destructors, at the delete below, find nothing left)
    if (c->h_sums) hipHostFree(c->h_sums);
    hipFree(c->d_loop);
    if (c->h_loop) hipHostFree(c->h_loop);
    if (c->h_ring) hipHostFree(c->h_ring);
    if (c->h_done) hipHostFree(c->h_done);
    for (hipEvent_t e : c->ev) if (e) hipEventDestroy(e);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
}

const char *symmicp_last_error(const symmicp_ctx *c) { return c ? c->err.c_str() : "null ctx"; }

int symmicp_set_config(symmicp_ctx *c, const symmicp_config *cfg)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (check_cfg(cfg) != SYMMICP_OK) return fail(c, SYMMICP_ERR_ARG, "bad config");
    // correspondence kind decides device layouts: it can only change before clouds are set
    if ((c->n_t || c->n_loc) && cfg->corr != c->cfg.corr) return fail(c, SYMMICP_ERR_STATE, "corr cannot change after clouds are set");
    if ((c->n_t || c->n_loc) && cfg->sort_source != c->cfg.sort_source) return fail(c, SYMMICP_ERR_STATE, "sort_source cannot change after clouds are set");
    if (cfg->mode == SYMMICP_MODE_QUIRKS && c->loss != SYMMICP_LOSS_NONE)
        return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no robust loss (set SYMMICP_LOSS_NONE first)");
    if (cfg->mode == SYMMICP_MODE_QUIRKS && c->rej.trims())
        return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no trim fraction below 1 (set 1 first)");
    if (cfg->mode == SYMMICP_MODE_QUIRKS && (c->rej.one_to_one || c->rej.median()))
        return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no one-to-one or median-distance rejector (switch them off first)");
    if (c->rej.reciprocal && cfg->mode == SYMMICP_MODE_QUIRKS)
        return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no reciprocal correspondences (switch them off first)");
    if (c->rej.reciprocal && cfg->corr == SYMMICP_CORR_IDENTITY)
        return fail(c, SYMMICP_ERR_ARG, "identity pairs were never searched: no reciprocal correspondences (switch them off first)");
    if (cfg->mode == SYMMICP_MODE_COLOR && c->nranks > 1)
        return fail(c, SYMMICP_ERR_STATE, "SYMMICP_MODE_COLOR runs on single-rank contexts only");
    if (cfg->mode == SYMMICP_MODE_NDT) {
        // (check_cfg has refused min_normal_dot > -1 and the incremental apply)
        if (const char *msg = ndt_context_refusal(c)) return fail(c, SYMMICP_ERR_ARG, msg);
        if (c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "SYMMICP_MODE_NDT runs on single-rank contexts only");
    }
    // an NDT context holds a voxel map where the others hold an index, and its source has none of their per-pair arrays
    if ((cfg->mode == SYMMICP_MODE_NDT) != (c->cfg.mode == SYMMICP_MODE_NDT) && (c->tgt_block || c->src0_block))
        return fail(c, SYMMICP_ERR_STATE, "the mode cannot change into or out of SYMMICP_MODE_NDT after clouds are set");
    if (c->src_no_normals && cfg->mode != SYMMICP_MODE_PLANE && cfg->mode != SYMMICP_MODE_NDT)
        return fail(c, SYMMICP_ERR_STATE, "the source was set without normals: only SYMMICP_MODE_PLANE can run on it");
    if (c->src_no_normals && cfg->min_normal_dot > -1.0f)
        return fail(c, SYMMICP_ERR_ARG, "min_normal_dot needs source normals (the source was set without them)");
    int dev = c->cfg.device;
    c->cfg = *cfg;
    c->cfg.device = dev;
    c->begun = false;
    c->rej.invalidate();
    return SYMMICP_OK;
}

// ---- robust loss ---------------------------------------------------------------------------------
static bool loss_args_ok(int loss, float scale)
{
    if (loss < SYMMICP_LOSS_NONE || loss > SYMMICP_LOSS_GEMAN_MCCLURE) return false;
    return loss == SYMMICP_LOSS_NONE || (std::isfinite(scale) && scale > 0.f);
}

int symmicp_set_robust_loss(symmicp_ctx *c, int loss, float scale)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!loss_args_ok(loss, scale)) return fail(c, SYMMICP_ERR_ARG, "robust loss: unknown loss, or scale not finite and > 0");
    if (loss != SYMMICP_LOSS_NONE && c->cfg.mode == SYMMICP_MODE_QUIRKS) return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no robust loss");
    if (loss != SYMMICP_LOSS_NONE && ndt_mode(c)) return fail(c, SYMMICP_ERR_ARG, "SYMMICP_MODE_NDT takes no robust loss");
#if defined(RS_STAMPS) || defined(RS_STAMPS2)
    if (loss != SYMMICP_LOSS_NONE) return fail(c, SYMMICP_ERR_ARG, "a build with RS_STAMPS keeps its stamps in slots 37..39: no robust loss");
#endif
    c->loss = loss;
    c->loss_scale = loss == SYMMICP_LOSS_NONE ? 0.f : scale;
    return SYMMICP_OK;
}

int symmicp_get_robust_loss(const symmicp_ctx *c, int *loss, float *scale)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (loss) *loss = c->loss;
    if (scale) *scale = c->loss_scale;
    return SYMMICP_OK;
}

// ---- trimmed ICP ---------------------------------------------------------------------------------
int symmicp_set_trim_fraction(symmicp_ctx *c, float fraction)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!(fraction > 0.f && fraction <= 1.f)) return fail(c, SYMMICP_ERR_ARG, "trim fraction: 0 < fraction <= 1");      // (NaN fails both)
    if (fraction < 1.f && c->cfg.mode == SYMMICP_MODE_QUIRKS) return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no trim fraction below 1");
    if (fraction < 1.f && ndt_mode(c)) return fail(c, SYMMICP_ERR_ARG, "SYMMICP_MODE_NDT takes no trim fraction below 1");
    if (fraction < 1.f && c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "trimming needs a quantile over all ranks: single-rank contexts only");
    if (fraction < 1.f && c->rej.median()) return fail(c, SYMMICP_ERR_ARG, "a trim fraction below 1 and a median factor exclude each other (set the factor to 0 first)");
    c->rej.trim_frac = fraction;
    return SYMMICP_OK;
}

int symmicp_get_trim_fraction(const symmicp_ctx *c, float *fraction)
{
    if (!c || !fraction) return SYMMICP_ERR_ARG;
    *fraction = c->rej.trim_frac;
    return SYMMICP_OK;
}

int symmicp_get_trim_state(const symmicp_ctx *c, uint64_t *candidates, uint64_t *kept, float *tau_d2)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun || !c->rej.trim_state_valid()) return SYMMICP_ERR_STATE;      // (const context: no message)
    if (candidates) *candidates = c->rej.last.population;
    if (kept) *kept = c->rej.last.kept;
    if (tau_d2) std::memcpy(tau_d2, &c->rej.last.tau_bits, sizeof(float));
    return SYMMICP_OK;
}

// ---- one-to-one and median-distance rejectors ------------------------------------------------------
int symmicp_set_one_to_one(symmicp_ctx *c, int on)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (on && c->cfg.mode == SYMMICP_MODE_QUIRKS) return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no one-to-one rejector");
    if (on && ndt_mode(c)) return fail(c, SYMMICP_ERR_ARG, "SYMMICP_MODE_NDT takes no one-to-one rejector");
    if (on && c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "the one-to-one claim needs a minimum over all ranks: single-rank contexts only");
    c->rej.one_to_one = on != 0;
    return SYMMICP_OK;
}

int symmicp_get_one_to_one(const symmicp_ctx *c, int *on)
{
    if (!c || !on) return SYMMICP_ERR_ARG;
    *on = c->rej.one_to_one ? 1 : 0;
    return SYMMICP_OK;
}

int symmicp_set_median_factor(symmicp_ctx *c, float factor)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!(factor == 0.f || (std::isfinite(factor) && factor > 0.f))) return fail(c, SYMMICP_ERR_ARG, "median factor: 0 (off), or finite and > 0");
    if (factor > 0.f && c->cfg.mode == SYMMICP_MODE_QUIRKS) return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no median-distance rejector");
    if (factor > 0.f && ndt_mode(c)) return fail(c, SYMMICP_ERR_ARG, "SYMMICP_MODE_NDT takes no median-distance rejector");
    if (factor > 0.f && c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "the median needs a quantile over all ranks: single-rank contexts only");
    if (factor > 0.f && c->rej.trims()) return fail(c, SYMMICP_ERR_ARG, "a median factor and a trim fraction below 1 exclude each other (set the fraction to 1 first)");
    c->rej.med_factor = factor == 0.f ? 0.f : factor;      // (-0 is off too)
    return SYMMICP_OK;
}

int symmicp_get_median_factor(const symmicp_ctx *c, float *factor)
{
    if (!c || !factor) return SYMMICP_ERR_ARG;
    *factor = c->rej.med_factor;
    return SYMMICP_OK;
}

int symmicp_get_rejection_state(const symmicp_ctx *c, uint64_t *gated, uint64_t *unique, uint64_t *kept, float *tau_d2)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun || !c->rej.rejection_state_valid()) return SYMMICP_ERR_STATE;      // (const context: no message)
    if (gated) *gated = c->rej.last.gated;
    if (unique) *unique = c->rej.last.population;      // (the claim's winners; without a claim every candidate)
    if (kept) *kept = c->rej.last.kept;
    if (tau_d2) std::memcpy(tau_d2, &c->rej.last.tau_bits, sizeof(float));
    return SYMMICP_OK;
}

// ---- reciprocal correspondences ---------------------------------------------------------------------
int symmicp_set_reciprocal(symmicp_ctx *c, int on)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (on && c->cfg.mode == SYMMICP_MODE_QUIRKS) return fail(c, SYMMICP_ERR_ARG, "QUIRKS takes no reciprocal correspondences");
    if (on && ndt_mode(c)) return fail(c, SYMMICP_ERR_ARG, "SYMMICP_MODE_NDT takes no reciprocal correspondences");
    if (on && c->cfg.corr == SYMMICP_CORR_IDENTITY) return fail(c, SYMMICP_ERR_ARG, "identity pairs were never searched: no reciprocal correspondences");
    if (on && c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "reciprocal correspondences need the claim and the source index over all ranks: single-rank contexts only");
    c->rej.reciprocal = on != 0;
    return SYMMICP_OK;
}

int symmicp_get_reciprocal(const symmicp_ctx *c, int *on)
{
    if (!c || !on) return SYMMICP_ERR_ARG;
    *on = c->rej.reciprocal ? 1 : 0;
    return SYMMICP_OK;
}

int symmicp_get_reciprocal_state(const symmicp_ctx *c, uint64_t *claimed, uint64_t *reciprocal)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun || !c->rej.reciprocal_state_valid()) return SYMMICP_ERR_STATE;      // (const context: no message)
    if (claimed) *claimed = c->rej.last.claimed;
    if (reciprocal) *reciprocal = c->rej.last.reciprocal;
    return SYMMICP_OK;
}

// (include/symmicp.h has the definition: fp64 from the fp32 entries -- every product is exact there -- one rounding to fp32 per entry)
int symmicp_inverse_rigid(const float X16[16], float out12[12])
{
    if (!X16 || !out12) return SYMMICP_ERR_ARG;
    const double t0 = X16[3], t1 = X16[7], t2 = X16[11];
    for (int r = 0; r < 3; r++) {
        const double a = X16[r], b = X16[4 + r], d = X16[8 + r];
        out12[4 * r + 0] = X16[r]; out12[4 * r + 1] = X16[4 + r]; out12[4 * r + 2] = X16[8 + r];
        out12[4 * r + 3] = (float)(-((a * t0 + b * t1) + d * t2));
    }
    return SYMMICP_OK;
}

// ---- GICP's covariances -------------------------------------------------------------------------
int symmicp_set_gicp_epsilon(symmicp_ctx *c, float eps)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!(std::isfinite(eps) && eps > 0.f && eps <= 1.f)) return fail(c, SYMMICP_ERR_ARG, "gicp epsilon: 0 < eps <= 1 and finite");
    // the kernels use 1 - eps in fp32 (fill_pass_args): an eps it rounds away (eps <= 2^-25) would make a pair of equal normals
    // singular (lambda_u = 0, gamma_u = inf, a NaN record)
    if (1.0f - eps == 1.0f) return fail(c, SYMMICP_ERR_ARG, "gicp epsilon: 1 - eps must differ from 1 in fp32 (eps > 2^-25)");
    c->gicp_eps = eps;
    return SYMMICP_OK;
}

int symmicp_get_gicp_epsilon(const symmicp_ctx *c, float *eps)
{
    if (!c || !eps) return SYMMICP_ERR_ARG;
    *eps = c->gicp_eps;
    return SYMMICP_OK;
}

// ---- colored ICP: lambda and the per-point attributes ---------------------------------------------
int symmicp_set_color_weight(symmicp_ctx *c, float lambda)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!(std::isfinite(lambda) && lambda >= 0.f && lambda <= 1.f)) return fail(c, SYMMICP_ERR_ARG, "color weight: 0 <= lambda <= 1 and finite");
    c->color_lam = lambda;
    return SYMMICP_OK;
}

int symmicp_get_color_weight(const symmicp_ctx *c, float *lambda)
{
    if (!c || !lambda) return SYMMICP_ERR_ARG;
    *lambda = c->color_lam;
    return SYMMICP_OK;
}

// the caller's strided values, staged contiguously and checked (false: a non-finite value)
static bool stage_finite(const float *base, size_t rs, size_t cs, size_t n, int cols, std::vector<float> &out)
{
    out.resize(n * (size_t)cols);
    bool ok = true;
    for (size_t i = 0; i < n; i++)
        for (int k = 0; k < cols; k++) {
            const float v = base[i * rs + (size_t)k * cs];
            ok = ok && std::isfinite(v);
            out[i * (size_t)cols + k] = v;
        }
    return ok;
}

int symmicp_set_source_intensity(symmicp_ctx *c, const float *intensity, size_t stride, size_t n)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!intensity) return fail(c, SYMMICP_ERR_ARG, "null source intensity");
    if (!c->src0_block) return fail(c, SYMMICP_ERR_STATE, "symmicp_set_source_intensity follows symmicp_set_source");
    if (n != c->n_s_total) return fail(c, SYMMICP_ERR_SIZE, "source intensity: n differs from the source's count");
    std::vector<float> host;
    if (!stage_finite(intensity, stride, 0, n, 1, host)) return fail(c, SYMMICP_ERR_ARG, "source intensity: non-finite value");
    HIP_TRY(c, hipSetDevice(c->device));
    c->have_src_int = false;
    c->begun = false;
    HIP_TRY(c, grow(c->src_int, c->src_int_cap, c->n_loc ? c->n_loc : 1));
    arena_begin(c->arena, n * 4 + 4096);
    DevBuf<float> raw;
    HIP_TRY(c, raw.alloc_temp(c->arena, n));
    HIP_TRY(c, hipMemcpyAsync(raw.p, host.data(), sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    launch_color_permute_source(raw.p, c->src_order, c->src_off, c->n_loc, c->src_int, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    c->have_src_int = true;
    return SYMMICP_OK;
}

int symmicp_set_target_intensity(symmicp_ctx *c, const float *intensity, size_t stride, const float *grad, size_t grs, size_t gcs, size_t n)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!intensity || !grad) return fail(c, SYMMICP_ERR_ARG, "null target intensity or gradient (symmicp_ctx_intensity_gradient estimates one)");
    if (!c->tgt_block) return fail(c, SYMMICP_ERR_STATE, "symmicp_set_target_intensity follows symmicp_set_target");
    if (n != c->n_t) return fail(c, SYMMICP_ERR_SIZE, "target intensity: n differs from the target's count");
    if (c->cfg.corr != SYMMICP_CORR_IDENTITY && !c->ix.tq) return fail(c, SYMMICP_ERR_STATE, "target was set under a different corr mode");
    std::vector<float> hi, hg;
    if (!stage_finite(intensity, stride, 0, n, 1, hi) || !stage_finite(grad, grs, gcs, n, 3, hg))
        return fail(c, SYMMICP_ERR_ARG, "target intensity or gradient: non-finite value");
    HIP_TRY(c, hipSetDevice(c->device));
    c->have_tgt_color = false;
    c->begun = false;
    HIP_TRY(c, grow(c->tgt_color, c->tgt_color_cap, n));
    arena_begin(c->arena, n * 16 + 8192);
    DevBuf<float> di, dg;
    HIP_TRY(c, di.alloc_temp(c->arena, n));
    HIP_TRY(c, dg.alloc_temp(c->arena, 3 * n));
    HIP_TRY(c, hipMemcpyAsync(di.p, hi.data(), sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(dg.p, hg.data(), sizeof(float) * 3 * n, hipMemcpyHostToDevice, c->stream));
    // (identity pairing reads the planar target in the caller's order; BRUTE's tq is in that order too and says so in its w words)
    launch_color_permute_target(di.p, dg.p, c->cfg.corr == SYMMICP_CORR_IDENTITY ? nullptr : c->ix.tq, (uint32_t)n, c->tgt_color, c->stream);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipGetLastError());
    c->have_tgt_color = true;
    return SYMMICP_OK;
}

int symmicp_get_source_intensity(symmicp_ctx *c, float *intensity, size_t cap)
{
    if (!c || !intensity) return SYMMICP_ERR_ARG;
    if (!c->src0_block || !c->have_src_int) return fail(c, SYMMICP_ERR_STATE, "no source intensity is set");
    const size_t need = c->src_order ? c->n_s_total : c->n_loc;
    if (cap < need) return fail(c, SYMMICP_ERR_SIZE, "output too small");
    HIP_TRY(c, hipSetDevice(c->device));
    arena_begin(c->arena, need * 4 + 4096);
    DevBuf<float> out;
    HIP_TRY(c, out.alloc_temp(c->arena, need));
    HIP_TRY(c, hipMemsetAsync(out.p, 0, sizeof(float) * need, c->stream));
    launch_color_unpermute_source(c->src_int, c->src_order, c->n_loc, out.p, c->stream);
    HIP_TRY(c, hipMemcpyAsync(intensity, out.p, sizeof(float) * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

float symmicp_robust_weight(int loss, float scale, float r)
{
    if (!loss_args_ok(loss, scale)) return std::numeric_limits<float>::quiet_NaN();
    return loss == SYMMICP_LOSS_NONE ? 1.0f : robust_weight(loss, scale, r);
}

int symmicp_set_target(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!xyz || (!nrm && !ndt_mode(c))) return fail(c, SYMMICP_ERR_ARG, "null target cloud (myicp.cpp:102 assert)");
    if (!nrm) nr = nc = 0;
    if (n == 0 || n > 0x7fffffffull) return fail(c, SYMMICP_ERR_SIZE, "target size out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    const double t0 = now_s();
    free_target(c);
    c->begun = false;
    // the target's persistent arrays: planar cloud 24 B, tq 16, pair records 32, octree ~64, run tree ~5, cell table
    const size_t want = n * 160 + ((size_t)16 << 20);
    c->tgt_store.reserve(want, want / 8);
    // temporaries of the upload and of the index build: ~80 B per point (11 octree-level id arrays, sort buffers, raw rows)
    arena_begin(c->arena, n * (96 + 4 * (xr + nr)) + ((size_t)1 << 20));
    double cen[3];
    DevBuf<float> tblock;
    int st = upload_planar(c, xyz, xr, xc, nrm, nr, nc, n, tblock, &c->tgt_store, cen);
    if (st != SYMMICP_OK) return st;
    c->tgt_block = tblock.release();
    soa_from_block(c->tgt_block, n, c->tgt);
    c->n_t = (uint32_t)n;
    for (int k = 0; k < 3; k++) c->pivot[k] = (float)cen[k];
    c->st.upload_ms += (now_s() - t0) * 1e3;
    if (ndt_mode(c)) {
        // NDT reads no index and no pair records: the voxel map over the planar copy (cfg.corr is not read in this mode)
        const double t1 = now_s();
        st = ndt_build_target_map(c);
        if (st != SYMMICP_OK) { free_target(c); return st; }
        c->st.build_ms = (now_s() - t1) * 1e3;
        return SYMMICP_OK;
    }
    if (c->cfg.corr == SYMMICP_CORR_IDENTITY) return SYMMICP_OK;

    const double t1 = now_s();
    // (SYMMICP_OCT_LEAF > 0 sets the octree's leaf size; otherwise the build chooses it from what the cloud looks like)
    IndexRequest rq{nullptr, nullptr, /*grid=*/true, /*oct_leaf=*/c->sw.oct_leaf > 0 ? c->sw.oct_leaf : 0};
    HIP_TRY(c, c->tgt_store.alloc((void **)&rq.tq, sizeof(float4) * (n + 8)));     // + 8: the packet search reads a leaf's points in groups of 8
    HIP_TRY(c, hipMemsetAsync(rq.tq + n, 0, sizeof(float4) * 8, c->stream));
    HIP_TRY(c, c->tgt_store.alloc((void **)&rq.tn, sizeof(float4) * 2 * n));      // (point, normal) pair records
    TargetIndex &ix = c->ix;      // (empty since free_target)
    ix.tq = rq.tq; ix.tn = rq.tn; ix.n = c->n_t;      // all a BRUTE target has of an index
    if (c->cfg.corr == SYMMICP_CORR_BRUTE) {
        launch_iota_f4(c->tgt.x, c->tgt.y, c->tgt.z, c->tgt.nx, c->tgt.ny, c->tgt.nz, c->n_t, rq.tq, rq.tn, c->stream);
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->st.build_ms = (now_s() - t1) * 1e3;
        return SYMMICP_OK;
    }
    BuiltIndex b;
    st = build_index(c, c->tgt_store, c->tgt, c->n_t, rq, &b);
    if (st != SYMMICP_OK) { free_target(c); return st; }
    ix = b.ix;
    c->target_surface_like = b.surface_like;
    c->notes = b.notes;
    c->st.grid_level = b.grid_level; c->st.tree_levels = b.tree_levels;
    if (c->sw.debug_counters) {
        HIP_TRY(c, hipMalloc((void **)&ix.dbg, 12 * sizeof(unsigned long long)));
        HIP_TRY(c, hipMemset(ix.dbg, 0, 12 * sizeof(unsigned long long)));
    }
    if (!c->sw.debug_trace.empty()) {          // (alone: the production kernel with a timing-only trace)
        HIP_TRY(c, hipMalloc((void **)&ix.dbg_trace, ((size_t)1 << 22) * 8));      // (kTraceWords)
        HIP_TRY(c, hipMemset(ix.dbg_trace, 0, ((size_t)1 << 22) * 8));
    }
    c->have_index = true;
    c->st.build_ms = (now_s() - t1) * 1e3;
    return SYMMICP_OK;
}

int symmicp_set_source(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!xyz) return fail(c, SYMMICP_ERR_ARG, "null source cloud (myicp.cpp:102 assert)");
    if (!nrm && c->cfg.mode != SYMMICP_MODE_PLANE && !ndt_mode(c))
        return fail(c, SYMMICP_ERR_ARG, "null source normals (only SYMMICP_MODE_PLANE and SYMMICP_MODE_NDT run without them)");
    if (!nrm && c->cfg.min_normal_dot > -1.0f) return fail(c, SYMMICP_ERR_ARG, "min_normal_dot needs source normals");
    if (!nrm) nr = nc = 0;
    if (n == 0 || n > 0x7fffffffull) return fail(c, SYMMICP_ERR_SIZE, "source size out of range");
    HIP_TRY(c, hipSetDevice(c->device));
    const double t0 = now_s();
    forget_source(c);
    c->begun = false;
    c->rej.invalidate();
    // This rank's share is a contiguous block of the CALLER's rows, and only those rows are uploaded and sorted: set_source costs
    // 1/nranks of the single-GPU call on every rank (round 1 uploaded and sorted the whole cloud on every rank and kept a
    // slice of the global Morton order).  Any partition of the source is exact -- queries are independent given the
    // transform -- and the share's own Morton sort below gives the waves their locality.
    size_t b0 = 0, bc = 0;
    symmicp_shard_range(n, c->nranks, c->rank, &b0, &bc);
    const size_t nu = bc > 0 ? bc : 1;                       // rows uploaded (an empty share still stages one row)
    const size_t r0 = bc > 0 ? b0 : 0;
    arena_begin(c->arena, nu * (56 + 4 * (xr + nr)) + ((size_t)1 << 20));      // (+8 B per point: the packet table's temporaries)
    DevBuf<float> full;
    int st = upload_planar(c, xyz + r0 * xr, xr, xc, nrm ? nrm + r0 * nr : nullptr, nr, nc, nu, full, /*store=*/nullptr, nullptr);
    if (st != SYMMICP_OK) return st;
    c->src_no_normals = !nrm;
    CloudSoA fs;
    soa_from_block(full.p, nu, fs);
    const uint32_t nl = bc > 0 ? (uint32_t)bc : 1;
    // (NDT: cfg.corr is not read; the share is sorted as BRUTE / TREE sort it and carries none of their per-pair arrays)
    const bool ndt = ndt_mode(c);
    const bool sorted = (ndt || c->cfg.corr != SYMMICP_CORR_IDENTITY) && c->cfg.sort_source;
    const bool tree = !ndt && c->cfg.corr == SYMMICP_CORR_TREE, brute = !ndt && c->cfg.corr == SYMMICP_CORR_BRUTE;
    // every per-source array in ONE allocation (a hipFree costs ~100 us, and a tracker calls this once per frame)
    const uint32_t cap = shard_capacity(nl);
    const size_t per_list = (size_t)kShards * cap, ncount = (size_t)kShards * kShardStride;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_src0 = take(sizeof(float) * 6 * nl), o_cur = take(sizeof(float) * 6 * nl);
    const size_t o_order = sorted ? take(sizeof(uint32_t) * nl) : 0;
    const size_t o_pos = take(sizeof(int32_t) * nl), o_d2 = take(sizeof(float) * nl);
    const size_t o_best = brute ? take(sizeof(unsigned long long) * nl) : 0;
    const size_t o_cert = tree ? take(sizeof(float) * 4 * nl) : 0;
    const size_t o_certk = tree ? take(sizeof(uint32_t) * 8 * nl) : 0, o_hoodr = tree ? take(sizeof(float) * 2 * nl) : 0;
    const size_t o_pkt = tree ? take(sizeof(uint32_t) * 2 * 8 * ((nl + 63) / 64)) : 0;        // (a block of 64 queries may be cut into 8 packets: kMaxRunsPerBlock)
    const size_t o_prec = tree ? take(sizeof(float4) * 2 * nl) : 0;
    const size_t o_wl = tree ? take(sizeof(uint32_t) * 2 * per_list) : 0, o_cnt = tree ? take(sizeof(uint32_t) * 2 * ncount) : 0;      // work + retry lists
    HIP_TRY(c, grow(c->src_all, c->src_all_cap, off));
    c->n_s_total = (uint32_t)n;
    c->src_off = (uint32_t)b0;
    c->n_loc = (uint32_t)bc;
    c->src0_block = reinterpret_cast<float *>(c->src_all + o_src0);
    c->cur_block = reinterpret_cast<float *>(c->src_all + o_cur);
    soa_from_block(c->src0_block, nl, c->src0);
    soa_from_block(c->cur_block, nl, c->cur);
    c->pos = reinterpret_cast<int32_t *>(c->src_all + o_pos);
    c->d2 = reinterpret_cast<float *>(c->src_all + o_d2);
    if (brute) c->best64 = reinterpret_cast<unsigned long long *>(c->src_all + o_best);
    if (sorted) {
        DevBuf<uint32_t> order;
        float origin[3], h0;
        st = morton_order(c, fs, (uint32_t)nu, order, nullptr, origin, &h0);
        if (st != SYMMICP_OK) { forget_source(c); return st; }
        c->src_order = reinterpret_cast<uint32_t *>(c->src_all + o_order);
        if (c->n_loc) {
            launch_gather_soa(fs, order.p, c->n_loc, c->src0, c->stream);               // share position -> row of the uploaded block
            launch_offset_u32(order.p, (uint32_t)b0, c->n_loc, c->src_order, c->stream); // ... -> row of the caller's cloud
        }
    } else if (c->n_loc) {
        HIP_TRY(c, hipMemcpyAsync(c->src0_block, full.p, sizeof(float) * 6 * c->n_loc, hipMemcpyDeviceToDevice, c->stream));
    }
    if (tree) {
        c->cert = reinterpret_cast<float *>(c->src_all + o_cert);
        c->certk = reinterpret_cast<uint32_t *>(c->src_all + o_certk);      // (validity lives in bit 0 of the certificate word: no clearing needed)
        c->hoodr = reinterpret_cast<float *>(c->src_all + o_hoodr);
        HIP_TRY(c, hipMemsetAsync(c->hoodr, 0, sizeof(float) * 2 * nl, c->stream));                // no radius hints yet
        c->pairrec = reinterpret_cast<float4 *>(c->src_all + o_prec);
        c->worklist = reinterpret_cast<uint32_t *>(c->src_all + o_wl);
        c->wl_count = reinterpret_cast<uint32_t *>(c->src_all + o_cnt);
        HIP_TRY(c, hipMemsetAsync(c->cert, 0, sizeof(float) * 4 * nl, c->stream));
        HIP_TRY(c, hipMemsetAsync(c->wl_count, 0, sizeof(uint32_t) * 2 * ncount, c->stream));
        c->wl.work = ShardList{c->worklist, c->wl_count, cap};
        c->wl.retry = ShardList{c->worklist + per_list, c->wl_count + ncount, cap};
    }
    if (tree && c->n_loc) {
        // The first pass's packets, in start order: by decreasing radius.  A packet that straddles a jump of the Morton curve takes several
        // times as many sweep steps as a compact one (median 210 us, 1 % above 830 us in the traced build), and a launch that meets such
        // packets last ends with a handful of waves running: longest-first is the classic remedy.  Radius keys, the index build's radix
        // sort (n / 64 keys) and the table, all on the device (+0.1 ms of set_source at 1M points; a host sort cost 0.85 ms).
        // Measured on the 1M surface pair: 0.81 -> 0.67 ms (only the widest third first: 0.70 -- the Morton order of the rest, i.e. XCD
        // locality, is worth less than the balance; splitting the widest packets into halves / quarters on top: no gain).
        const uint32_t nblk = (c->n_loc + 63u) / 64u;
        const bool ordered = c->sw.packet_order;      // (SYMMICP_PACKET_ORDER=0: packets as they lie)
        c->pkt_tab = nullptr; c->pkt_count = 0;
        if (ordered) {
            // (a block of 64 queries is cut into runs at its jumps of the Morton curve: k_packet_runs)
            const float jump = c->sw.packet_jump;      // x the block's scale; 0: never cut
            const int key_bits = c->sw.packet_key_bits;      // (with the blocks cut at their jumps the order needs no more: 10 / 12 / 16 / 32 bits all 0.56-0.58 ms; two radix passes instead of four)
            const uint32_t cap = 8u * nblk;            // (kMaxRunsPerBlock)
            DevBuf<uint32_t> keys, vals, kt, vt, ws, cnt;
            DevBuf<uint2> runs;
            const size_t wse = radix_sort_ws_elems(cap);
            HIP_TRY(c, keys.alloc_temp(c->arena, cap));
            HIP_TRY(c, vals.alloc_temp(c->arena, cap));
            HIP_TRY(c, kt.alloc_temp(c->arena, cap));
            HIP_TRY(c, vt.alloc_temp(c->arena, cap));
            HIP_TRY(c, runs.alloc_temp(c->arena, cap));
            HIP_TRY(c, ws.alloc_temp(c->arena, wse));
            HIP_TRY(c, cnt.alloc_temp(c->arena, 1));
            HIP_TRY(c, hipMemsetAsync(cnt.p, 0, sizeof(uint32_t), c->stream));
            launch_packet_runs(c->src0, c->n_loc, jump, runs.p, keys.p, vals.p, cnt.p, key_bits, c->stream);
            uint32_t npk = 0;
            HIP_TRY(c, hipMemcpyAsync(&npk, cnt.p, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(c, hipStreamSynchronize(c->stream));
            if (npk < nblk || npk > cap) { forget_source(c); return fail(c, SYMMICP_ERR_HIP, "packet table: count out of range"); }
            // the target is known already: key the start order by what a packet will cost (its distance to the target), not by its extent alone
            c->pkt_cost_keyed = c->have_index && c->ix.onodes && key_bits > 0 && c->sw.packet_cost_key;
            if (c->pkt_cost_keyed) launch_packet_cost(c->src0, runs.p, npk, c->ix, keys.p, key_bits, c->stream);
            radix_sort_pairs(keys.p, vals.p, kt.p, vt.p, npk, key_bits > 0 ? key_bits : 32, ws.p, wse, c->stream);
            c->pkt_tab = reinterpret_cast<uint32_t *>(c->src_all + o_pkt);
            c->pkt_count = npk;
            launch_packet_table(vals.p, runs.p, npk, reinterpret_cast<uint2 *>(c->pkt_tab), c->stream);
            HIP_TRY(c, hipStreamSynchronize(c->stream));       // (the temporaries are about to go out of scope)
        }
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));       // (the arena-backed upload is read by the gather above)
    HIP_TRY(c, hipGetLastError());
    c->fb.forget_list();
    c->st.upload_ms += (now_s() - t0) * 1e3;
    return SYMMICP_OK;
}

// resolve the recorded event ring into per-kernel totals (called lazily: ring full, or stats requested)
extern "C++" void flush_events(symmicp_ctx *c)
{
    for (int p = 0; p < c->ev_used; p++) {
        hipEvent_t *e = c->ev + p * symmicp_ctx::kEvPer;
        if (hipEventSynchronize(c->ev_split[p] == 1 ? e[4] : e[5]) != hipSuccess) continue;
        float ms = 0.f;
        double pass_ms = 0.0;
        if (c->ev_split[p] == 2) {
            for (int k = 0; k < 5; k++)
                if (hipEventElapsedTime(&ms, e[k], e[k + 1]) == hipSuccess) { c->st.kernel_ms[k] += ms; c->st.kernel_launches[k]++; if (k < 4) pass_ms += ms; }
        } else if (c->ev_split[p] == 1) {
            if (hipEventElapsedTime(&ms, e[0], e[4]) == hipSuccess) { pass_ms += ms; c->st.kernel_ms[6] += ms; c->st.kernel_launches[6]++; }
        } else {
            if (hipEventElapsedTime(&ms, e[0], e[4]) == hipSuccess) { c->st.kernel_ms[5] += ms; c->st.kernel_launches[5]++; pass_ms += ms; }
            if (hipEventElapsedTime(&ms, e[4], e[5]) == hipSuccess) { c->st.kernel_ms[4] += ms; c->st.kernel_launches[4]++; }
        }
        if (c->ev_coll[p] && hipEventElapsedTime(&ms, e[6], e[7]) == hipSuccess) { c->st.allreduce_ms += ms; c->st.allreduce_timed++; }
        c->ev_coll[p] = 0;
        const int w = c->ev_weight[p] > 0 ? c->ev_weight[p] : 1;
        c->st.last_pass_ms = pass_ms;
        c->st.sum_pass_ms += pass_ms * w;
        for (int k = 0; k < w && c->st.passes_timed + k < 8; k++) c->st.pass_ms_head[c->st.passes_timed + k] = pass_ms;      // (a sampled pass stands for w passes)
        c->st.passes_timed += w;
    }
    c->ev_used = 0;
}

int symmicp_get_transform(const symmicp_ctx *c, float out16[16])
{
    if (!c || !out16) return SYMMICP_ERR_ARG;
    std::memcpy(out16, c->X, sizeof(float) * 16);
    return SYMMICP_OK;
}

int symmicp_get_pivot(const symmicp_ctx *c, float out3[3])
{
    if (!c || !out3) return SYMMICP_ERR_ARG;
    const bool paper = c->cfg.mode != SYMMICP_MODE_QUIRKS;
    for (int k = 0; k < 3; k++) out3[k] = paper ? c->pivot[k] : 0.f;
    return SYMMICP_OK;
}

size_t symmicp_local_source_count(const symmicp_ctx *c) { return c ? c->n_loc : 0; }
size_t symmicp_local_source_offset(const symmicp_ctx *c) { return c ? c->src_off : 0; }

// rows are reported relative to this rank's share; with a sorted source the share is a set of
// caller rows (not a contiguous range), so indices are written at [row] of a full-size array.
int symmicp_get_correspondences(symmicp_ctx *c, int32_t *idx, float *d2, size_t cap)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun) return fail(c, SYMMICP_ERR_STATE, "no pass has run yet");
    const size_t need = c->src_order ? c->n_s_total : c->n_loc;
    if (cap < need) return fail(c, SYMMICP_ERR_SIZE, "output too small");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<int32_t> d_idx;
    DevBuf<float> d_d2;
    arena_begin(c->arena, need * 8 + 4096);
    HIP_TRY(c, d_idx.alloc_temp(c->arena, need));
    HIP_TRY(c, d_d2.alloc_temp(c->arena, need));
    HIP_TRY(c, hipMemsetAsync(d_idx.p, 0xFF, sizeof(int32_t) * need, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_d2.p, 0, sizeof(float) * need, c->stream));
    if (ndt_mode(c)) {
        // the map row of every point's own cell at the last pass's transform, and d2 to that voxel's mean
        NdtPassArgs na;
        ndt_pass_args(c, c->X, na);
        launch_ndt_corr(na, c->src_order, d_idx.p, d_d2.p, c->stream);
        if (idx) HIP_TRY(c, hipMemcpyAsync(idx, d_idx.p, sizeof(int32_t) * need, hipMemcpyDeviceToHost, c->stream));
        if (d2) HIP_TRY(c, hipMemcpyAsync(d2, d_d2.p, sizeof(float) * need, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        return SYMMICP_OK;
    }
    const int mode = c->cfg.corr == SYMMICP_CORR_IDENTITY ? 0 : (c->cfg.corr == SYMMICP_CORR_BRUTE ? 1 : 2);
    if (mode != 1 && d2) {
        // the identity pass streams without storing distances, the tree passes store one only for the pairs they searched: evaluate all
        // of them now, at the positions of the last pass
        const bool incr = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL;
        Affine X{};
        float I[16];
        identity16(I);
        const float *m = incr ? I : c->X;
        for (int k = 0; k < 12; k++) X.m[k] = m[k];
        X.nrm_w = 0.f;
        if (mode == 0) launch_identity_d2(incr ? c->cur : c->src0, X, c->tgt, c->src_off, c->n_loc, c->d2, c->stream);
        else launch_pairs_d2(incr ? c->cur : c->src0, X, c->pos, c->ix.tq, c->n_t, c->n_loc, c->d2, c->stream);
    }
    // (after a pass with a rejector -- trim fraction, one-to-one, median -- a row that was no candidate, or was rejected, is reported as rejected)
    launch_corr_out(c->pos, c->best64, c->d2, c->ix.tq, c->src_order, c->n_loc, mode, c->src_off, d_idx.p, d_d2.p,
                    c->rej.keys_valid() ? c->rej.keys : nullptr, c->rej.last.tau_bits, c->stream);
    if (idx) HIP_TRY(c, hipMemcpyAsync(idx, d_idx.p, sizeof(int32_t) * need, hipMemcpyDeviceToHost, c->stream));
    if (d2) HIP_TRY(c, hipMemcpyAsync(d2, d_d2.p, sizeof(float) * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

int symmicp_get_source(symmicp_ctx *c, float *xyz, float *nrm, size_t cap)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun) return fail(c, SYMMICP_ERR_STATE, "no pass has run yet");
    if (resolved_apply(c->cfg) != SYMMICP_APPLY_INCREMENTAL)
        return fail(c, SYMMICP_ERR_STATE, "the transformed source is only materialised with SYMMICP_APPLY_INCREMENTAL");
    const size_t need = c->src_order ? c->n_s_total : c->n_loc;
    if (cap < need) return fail(c, SYMMICP_ERR_SIZE, "output too small");
    HIP_TRY(c, hipSetDevice(c->device));
    DevBuf<float> dx, dn;
    arena_begin(c->arena, need * 24 + 4096);
    HIP_TRY(c, dx.alloc_temp(c->arena, 3 * need));
    HIP_TRY(c, dn.alloc_temp(c->arena, 3 * need));
    HIP_TRY(c, hipMemsetAsync(dx.p, 0, sizeof(float) * 3 * need, c->stream));
    HIP_TRY(c, hipMemsetAsync(dn.p, 0, sizeof(float) * 3 * need, c->stream));
    launch_unpermute(c->cur, c->src_order, c->n_loc, dx.p, dn.p, c->stream);
    if (xyz) HIP_TRY(c, hipMemcpyAsync(xyz, dx.p, sizeof(float) * 3 * need, hipMemcpyDeviceToHost, c->stream));
    if (nrm) HIP_TRY(c, hipMemcpyAsync(nrm, dn.p, sizeof(float) * 3 * need, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return SYMMICP_OK;
}

// ---- stats -------------------------------------------------------------------------------------
int symmicp_enable_timing(symmicp_ctx *c, int on)
{
    if (!c) return SYMMICP_ERR_ARG;
    c->timing = on < 0 ? 0 : (on > 3 ? 3 : on);
    return SYMMICP_OK;
}

int symmicp_reset_stats(symmicp_ctx *c)
{
    if (!c) return SYMMICP_ERR_ARG;
    flush_events(c);
    c->st.last_pass_ms = c->st.sum_pass_ms = 0.0;
    c->st.passes = 0;
    c->st.passes_timed = 0;
    c->st.loop_passes = c->st.loop_straggler_passes = 0;
    c->st.allreduce_ms = 0.0; c->st.allreduce_timed = 0;
    for (int k = 0; k < 8; k++) { c->st.kernel_ms[k] = 0.0; c->st.kernel_launches[k] = 0; c->st.pass_ms_head[k] = 0.0; }
    return SYMMICP_OK;
}

int symmicp_get_stats(symmicp_ctx *c, symmicp_stats *out)
{
    if (!c || !out) return SYMMICP_ERR_ARG;
    flush_events(c);
    c->st.pass_blocks = c->pass_blocks;
    const bool incr = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL;
    int64_t b = 0;
    if (c->cfg.corr == SYMMICP_CORR_IDENTITY) b = (int64_t)c->n_loc * 48;
    else b = (int64_t)c->n_loc * (48 + 4 + 4) + (int64_t)c->n_t * 12;
    if (incr) b += (int64_t)c->n_loc * 24;
    else if ((c->cfg.mode == SYMMICP_MODE_PLANE || c->cfg.mode == SYMMICP_MODE_COLOR) && !(c->cfg.min_normal_dot > -1.0f)) b -= (int64_t)c->n_loc * 12;      // (no source normals read)
    if (c->cfg.mode == SYMMICP_MODE_COLOR) b += (int64_t)c->n_loc * (4 + 16);      // the source's intensity per point, the target's (gradient, intensity) per pair
    c->st.bytes_algorithmic_per_pass = b;
    {
        uint32_t fb = 0;
        if (c->pkt_fallbacks && hipMemcpy(&fb, c->pkt_fallbacks, sizeof(fb), hipMemcpyDeviceToHost) == hipSuccess) c->st.packet_fallbacks = (int64_t)fb;
    }
    *out = c->st;
    return SYMMICP_OK;
}

}  // extern "C"
