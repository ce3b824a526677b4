// engine_loop.cpp -- the iteration loop of libsymmicp (reference ICP/myicp.cpp:117-150): one pass over the source share (run_pass), device-driven
// runs of passes (run_batch), symmicp_begin / step / align, the host solve entry point and the reference's result block.
#include "engine_internal.h"

extern "C" {

// ---- one pass over the source share ------------------------------------------------------------
// The rejectors of the next pass (symmicp.h: trim fraction, one-to-one, median distance, reciprocal): the buffers, for a reciprocal pass the
// source index and this pass's RecipArgs in device memory, and what the pass kernels read.  With none set: nothing is touched, r stays zero
// and the pass is the one of a build without rejectors.  The result lands behind the record's sequence word in host-mapped memory.
static int prepare_rejectors(symmicp_ctx *c, RejectArgs &r)
{
    Rejectors &j = c->rej;
    r = RejectArgs{};
    if (!pass_rejects(c)) return SYMMICP_OK;
    HIP_TRY(c, grow(j.keys, j.keys_cap, c->n_loc ? c->n_loc : 1));
    if (!j.ws) HIP_TRY(c, hipMalloc((void **)&j.ws, sizeof(uint32_t) * kRejectWsWords));
    r.keys = j.keys; r.ws = j.ws;
    r.host = reinterpret_cast<RejectRecord *>(c->h_sums_dev + kNSum + 1);
    r.rho = j.trim_frac; r.med_f2 = j.median() ? j.med_factor * j.med_factor : 0.0f;
    if (!pass_claims(c)) return SYMMICP_OK;
    HIP_TRY(c, grow(j.table, j.table_cap, Rejectors::table_words(c->n_t, pass_reciprocal(c))));
    r.table = j.table; r.n_t = c->n_t; r.order = c->src_order;
    r.claim = kClaimOneToOne;
    if (!pass_reciprocal(c)) return SYMMICP_OK;
    // the source index: once per set_source, over the whole original source, labelled with the caller's rows; and this pass's inverse
    if (!j.src_ix.valid) {
        const double t0 = now_s();
        if (int st = build_reverse_index(c, c->src0, c->n_loc, c->src_order, j.src_ix)) return st;
        j.src_ix_builds++;
        if (c->sw.debug_host) {
            std::fprintf(stderr, "[symmicp host] source index: %u points, %zu bytes in its arena (+%zu allocations beside it), built in %.3f ms\n", c->n_loc,
                         j.src_ix.store.used(), j.src_ix.store.beside(), (now_s() - t0) * 1e3);
        }
    }
    j.recip_args.six = j.src_ix.ix;
    symmicp_inverse_rigid(c->X, j.recip_args.inv.m);
    j.recip_args.inv.nrm_w = 0.0f;
    RecipArgs *tail = reinterpret_cast<RecipArgs *>(j.table + c->n_t);      // (table_words left the room)
    // (a pageable source that the next pass overwrites: safe because a copy this small is staged before the call returns, and because
    // the host loop waits for every pass's record before it comes here again.  A loop that queued rejecting passes would need a slot per pass)
    HIP_TRY(c, hipMemcpyAsync(tail, &j.recip_args, sizeof(RecipArgs), hipMemcpyHostToDevice, c->stream));
    r.recip = tail; r.claim = kClaimReciprocal;
    return SYMMICP_OK;
}

// Waits until the device has written seq to a host-mapped word: a spin instead of a stream-synchronise wake-up.  A stream that ends
// without the word (kernel fault), or limit_seconds of nothing, falls back to the synchronise and its error.  spun: the time in the spin is added
static int wait_for_word(symmicp_ctx *c, const volatile unsigned long long *flag, unsigned long long seq, double limit_seconds, const char *what,
                         double *spun = nullptr)
{
    const double t0 = now_s();
    unsigned spins = 0;
    bool got = false;
    while (!(got = (*flag == seq))) {
        __builtin_ia32_pause();
        if ((++spins & 0xFFFu) == 0) {
            if (hipStreamQuery(c->stream) != hipErrorNotReady) { got = (*flag == seq); break; }
            if (now_s() - t0 > limit_seconds) break;
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    if (spun) *spun += now_s() - t0;
    if (!got) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipGetLastError());
        if (*flag != seq) return fail(c, SYMMICP_ERR_HIP, what);
    }
    return SYMMICP_OK;
}

static_assert(kPlanTile == (uint32_t)kPassThreads, "loop_plan.h sizes grids in tiles of kPassThreads points");

// the pass honours the pair certificates (not the first pass of an alignment: they are not valid yet)
static bool pass_uses_slack(const symmicp_ctx *c, bool first) { return !first && c->cert && !c->sw.no_cert; }

// The plan of the next pass (plan_tree_pass, loop_plan.h) from the context: the feedback of the pass before, the sizes and the switches.
// (Every kind of pass asks: the pass arguments carry make_hood and budget_walk whatever the correspondences.)
static TreePassPlan plan_pass(const symmicp_ctx *c, bool first, bool writeback)
{
    TreePassIn in{};
    in.first = first; in.writeback = writeback; in.rejecting = pass_rejects(c);
    in.fb = c->fb;
    in.n_s_total = c->n_s_total; in.n_loc = c->n_loc; in.nranks = c->nranks;
    in.use_slack = pass_uses_slack(c, first);
    in.have_certk = c->certk && !c->sw.no_hood;
    in.walk_full_grid = c->sw.walk_full_grid;
    in.optimistic = c->sw.optimistic; in.compact = c->sw.compact; in.budget_walk = c->sw.budget_walk;
    in.hood_frac = c->sw.hood_frac;
    in.acc_blocks = c->sw.acc_blocks; in.compact_blocks = c->sw.compact_blocks;
    return plan_tree_pass(in);
}

static void fill_pass_args(symmicp_ctx *c, PassArgs &a, const RejectArgs &rej, const TreePassPlan &plan, const float Xapply[16], bool from_cur, bool writeback,
                           bool first)
{
    a.in = from_cur ? c->cur : c->src0;
    a.out = c->cur;
    a.n = c->n_loc;
    a.tgt_offset = c->src_off;
    for (int k = 0; k < 12; k++) a.X.m[k] = Xapply[k];
    a.X.nrm_w = (c->cfg.mode == SYMMICP_MODE_QUIRKS) ? 1.0f : 0.0f;   // myicp.cpp:137 quirk
    const bool paper = c->cfg.mode != SYMMICP_MODE_QUIRKS;          // PAPER and P2P take their sums about the pivot
    for (int k = 0; k < 3; k++) a.pivot[k] = paper ? c->pivot[k] : 0.0f;
    a.p2p = c->cfg.mode == SYMMICP_MODE_P2P ? 1 : 0;
    a.obj = mode_obj(c->cfg.mode);
    a.gicp_k = 1.0f - c->gicp_eps;
    a.tgt_color = c->tgt_color;
    a.src_int = c->src_int;
    a.color_lam = c->color_lam;
    a.color_om = 1.0f - c->color_lam;
    a.max_d2 = c->cfg.max_corr_dist > 0.f ? c->cfg.max_corr_dist * c->cfg.max_corr_dist : 0.f;
    a.min_ndot = c->cfg.min_normal_dot;
    a.writeback = writeback ? 1 : 0;
    a.best64 = c->best64;
    a.pos_prev = first ? nullptr : c->pos;
    a.pos_out = c->pos;
    // identity pairing streams at the HBM roof: the per-pair distances (4 B/point) are only written on request
    a.d2_out = (c->cfg.corr == SYMMICP_CORR_IDENTITY) ? nullptr : c->d2;
    a.partials = c->partials;
    a.cert = reinterpret_cast<float4 *>(c->cert);
    a.certk = c->sw.no_hood ? nullptr : reinterpret_cast<uint4 *>(c->certk);
    a.hoodr = reinterpret_cast<float2 *>(c->hoodr);
    a.make_hood = plan.make_hood ? 1 : 0;
    a.pairrec = c->pairrec;
    a.budget_walk = plan.budget_walk ? 1 : 0;
    a.use_slack = pass_uses_slack(c, first) ? 1 : 0;
    a.loop = nullptr;
    a.pkt_tab = reinterpret_cast<const uint2 *>(c->pkt_tab);
    a.pkt_count = c->pkt_count;
    a.pkt_waves = c->sw.packet_waves;
    a.pkt_front_cap = c->sw.packet_front_cap;
    a.pkt_fallbacks = c->pkt_fallbacks;
    a.pkt_chunk = c->sw.packet_chunk;
    a.pkt_lds_pad = c->sw.packet_lds_pad;
    a.loss = c->loss;
    a.loss_scale = c->loss_scale;
    a.rej = rej;
}

// The pass's events in timing mode (null without): a slot of the ring, event 0 in front of the pass
static hipEvent_t *begin_pass_events(symmicp_ctx *c, bool tree_pass)
{
    if (!c->timing) return nullptr;
    if (c->ev_used == symmicp_ctx::kEvRing) flush_events(c);
    hipEvent_t *ev = c->ev + c->ev_used * symmicp_ctx::kEvPer;
    c->ev_split[c->ev_used] = (c->timing == 1 || c->timing == 3) ? 1 : 0;
    c->ev_weight[c->ev_used] = 1;
    // (in per-kernel mode the split launcher records ev[0] itself)
    if (!(c->timing == 2 && tree_pass)) hipEventRecord(ev[0], c->stream);
    return ev;
}

// The launchers of a pass's search and accumulation, one per kind of correspondence.  Each returns the number of partial records it leaves.
// (NDT: cfg.corr is not read -- no search, no work list, no rejector)
static int launch_ndt(symmicp_ctx *c, const float Xapply[16])
{
    const int blocks = ndt_blocks(c->n_loc, c->sw.acc_blocks);
    NdtPassArgs na;
    ndt_pass_args(c, Xapply, na);
    launch_pass_ndt(na, blocks, c->stream);
    return blocks;
}

static int launch_identity(symmicp_ctx *c, const PassArgs &a)
{
    const int cap = identity_vec4(c->n_loc, c->n_t, c->src_off) ? c->sw.id_blocks : host_pass_cap(c->sw.pass_blocks);
    const IdentityGrid g = identity_grid(c->n_loc, c->n_t, c->src_off, cap);
    launch_pass_identity(a, c->tgt, g.blocks, g.vec4, c->stream);
    return g.blocks;
}

static int launch_brute(symmicp_ctx *c, const PassArgs &a)
{
    const int blocks = capped_blocks(c->n_loc, host_pass_cap(c->sw.pass_blocks), false, 1);
    launch_nn_brute(a.in, c->n_loc, a.X, c->ix.tq, c->n_t, c->best64, c->stream);
    launch_pass_indexed(a, c->ix.tn, blocks, c->stream);
    return blocks;
}

static int launch_tree(symmicp_ctx *c, const PassArgs &a, const TreePassPlan &plan, bool first, hipEvent_t *ev)
{
    // per-kernel events only in timing mode 2; mode 1 brackets the pass (events 0 and 4)
    hipEvent_t *kernel_ev = c->timing == 2 ? ev : nullptr;
    if (first && c->target_surface_like) launch_pass_tree_first(a, c->ix, c->wl, plan.acc_blocks, c->stream, kernel_ev);
    else launch_pass_tree_split(a, c->ix, c->wl, plan.acc_blocks, plan.walk_blocks, plan.optimistic ? 1 : 0, plan.compact_blocks, c->sw.tune, c->stream, kernel_ev);
    if (kernel_ev) c->ev_split[c->ev_used] = 2;
    return plan.acc_blocks;
}

// sums the record in d_sums over the ranks, in the stream.  A failure leaves the cleanup to the caller
static int allreduce_record(symmicp_ctx *c)
{
    const int r = g_rccl.AllReduce(c->d_sums, c->d_sums, kNSum, kNcclFloat64, kNcclSum, c->comm, c->stream);
    if (r != 0) return fail(c, SYMMICP_ERR_COMM, std::string("ncclAllReduce: ") + (g_rccl.GetErrorString ? g_rccl.GetErrorString(r) : "?"));
    return SYMMICP_OK;
}

// Final reduce (+ all-reduce or shared-memory exchange over ranks), then wait for the record.  It arrives in host-mapped memory followed
// by its sequence number: spin on that word instead of paying a stream-synchronise wake-up per iteration.  A stuck stream (kernel fault)
// is caught by the fallback.
static int reduce_and_wait(symmicp_ctx *c, int blocks, bool tree_pass, hipEvent_t *ev, int keep_nonempty)
{
    const unsigned long long seq = ++c->seq;
    volatile unsigned long long *flag = reinterpret_cast<volatile unsigned long long *>(c->h_sums + kNSum);
    launch_final_reduce(c->partials, blocks, c->d_sums, c->comm ? nullptr : c->h_sums_dev, c->ticket, seq, tree_pass ? c->wl_count : nullptr, keep_nonempty,
                        c->stream);
    if (c->comm) {
        if (ev) { hipEventRecord(ev[6], c->stream); c->ev_coll[c->ev_used] = 1; }
        if (int st = allreduce_record(c)) return st;
        if (ev) hipEventRecord(ev[7], c->stream);
        launch_publish(c->d_sums, c->h_sums_dev, seq, c->stream);
    }
    // the final-reduce time is only separated out in per-kernel mode; otherwise event 5 is event 4 again
    if (ev && c->ev_split[c->ev_used] != 1) hipEventRecord(ev[5], c->stream);
    if (int st = wait_for_word(c, flag, seq, 30.0, "pass finished without publishing its record", &c->t_spin)) return st;
    return c->shm.slots ? shm_exchange(c, c->h_sums) : SYMMICP_OK;
}

// What a TREE pass's record says beside its sums (the two feedback slots, summed over ranks by the exchange, so every rank takes the same
// decision): overflow check, the counts, the repair of an optimistic pass, the list.  *list_len: the work list's length
static int absorb_tree_feedback(symmicp_ctx *c, const PassArgs &a, int blocks, bool first, bool optimistic, hipEvent_t *ev, uint64_t *list_len)
{
    const FeedbackWords w = feedback_decode(c->h_sums[kFeedbackListSlot], c->h_sums[kFeedbackCountSlot]);
    if (w.dropped) return fail(c, SYMMICP_ERR_HIP, "a work-list shard overflowed: appends were dropped (internal capacity error)");
    *list_len = (uint64_t)w.list_len;
    if (first) c->fb.forget_counts(); else c->fb.set_counts((uint64_t)w.searched, (uint64_t)w.scans);
    if (optimistic && *list_len > 0) {
        // the walk was skipped but some queries needed it: their pairs are provisional, so are the sums
        c->st.kernel_launches[7]++;
        launch_pass_tree_split(a, c->ix, c->wl, blocks, repair_walk_blocks(*list_len), 2, 0, c->sw.tune, c->stream, nullptr);
        if (ev && c->ev_split[c->ev_used] != 2) hipEventRecord(ev[4], c->stream);
        if (int st = reduce_and_wait(c, blocks, true, ev, 0)) return st;
    }
    // (the packet first pass has no work list; the pass after it always has one)
    if (first && c->target_surface_like) c->fb.expect_list(); else c->fb.set_list(*list_len);
    return SYMMICP_OK;
}

static int run_pass(symmicp_ctx *c, const float Xapply[16], bool from_cur, bool writeback, bool first)
{
    // A rejecting pass: search as always, then the claim, the keys of the candidates and tau (kernels_select.hip: issued by the pass
    // launchers in front of the accumulating kernel), then the accumulation over the pairs at or below tau and the final reduce.
    RejectArgs rej;
    if (int st = prepare_rejectors(c, rej)) return st;
    c->rej.invalidate();
    const TreePassPlan plan = plan_pass(c, first, writeback);
    PassArgs a{};
    fill_pass_args(c, a, rej, plan, Xapply, from_cur, writeback, first);
    const bool ndt = ndt_mode(c);
    const bool tree_pass = !ndt && c->cfg.corr == SYMMICP_CORR_TREE;
    const double t_l0 = now_s();
    if (c->t_last_done > 0) c->t_between += t_l0 - c->t_last_done;
    hipEvent_t *ev = begin_pass_events(c, tree_pass);
    const int blocks = ndt                                     ? launch_ndt(c, Xapply)
                     : c->cfg.corr == SYMMICP_CORR_IDENTITY    ? launch_identity(c, a)
                     : c->cfg.corr == SYMMICP_CORR_BRUTE       ? launch_brute(c, a)
                                                               : launch_tree(c, a, plan, first, ev);
    c->pass_blocks = blocks;
    if (ev && c->ev_split[c->ev_used] != 2) hipEventRecord(ev[4], c->stream);
    c->t_launch += now_s() - t_l0;
    const bool optimistic = tree_pass && plan.optimistic;
    if (int st = reduce_and_wait(c, blocks, tree_pass, ev, optimistic ? 1 : 0)) return st;
    uint64_t list_len = 0;
    if (tree_pass) { if (int st = absorb_tree_feedback(c, a, blocks, first, optimistic, ev, &list_len)) return st; }
    else { c->fb.forget_counts(); c->fb.forget_list(); }
    if (pass_rejects(a)) {
        std::memcpy(&c->rej.last, c->h_sums + kNSum + 1, sizeof(RejectRecord));      // (written before the record: same stream)
        c->rej.ran = c->rej.settings_mask(c->cfg.corr);
    }
    if (ev) c->ev_used++;
    c->t_last_done = now_s(); c->n_pass_timed++;
    if (c->ix.dbg_trace && first) dump_packet_trace(c);
    if (c->ix.dbg) print_pass_counters(c, first, tree_pass ? (long long)list_len : -1);
    std::memcpy(c->last.s, c->h_sums, sizeof(double) * kNSum);
    if (tree_pass) c->last.s[kFeedbackListSlot] = c->last.s[kFeedbackCountSlot] = 0.0;      // those slots carried the feedback, not sums
    if (ndt) {
        c->ndt.score = -c->ndt.d1 * c->last.s[34];
        c->ndt.items = (uint64_t)c->last.s[37];
        c->ndt.pass_valid = true;
    }
    c->st.passes++;
    return SYMMICP_OK;
}

// ---- device-driven runs of passes -------------------------------------------------------------------
// Once an alignment has converged a pass is ~30 us of kernels, and the host's share of an iteration (read the record back,
// solve, launch) is as long as a kernel.  So symmicp_align hands runs of passes to the device: the solve of func.cpp:76-102
// runs at the end of the reduce (k_reduce_solve, same source as the host solve: solve_core.h), the next pass reads its
// transform from device memory, and the loop test of myicp.cpp:123 sets a stop flag every later kernel of the batch
// honours.  The host solve stays the reference: anything but a clean, well-conditioned solve, and any pass that needs
// the tree walk, stops the batch and the host loop takes that iteration (LOOP_HOST_SOLVE / LOOP_REDO_PASS).
// When a run may start, how it is cut into chunks and which kernel runs a chunk: batch_eligible and ChunkPlanner, loop_plan.h.
static bool may_start_batch(const symmicp_ctx *c)
{
    BatchEligibleIn in{};
    in.host_loop_switch = c->sw.host_loop;
    in.rejecting = pass_rejects(c);
    in.color = c->cfg.mode == SYMMICP_MODE_COLOR;
    in.host_loop_config = c->cfg.host_loop != 0;
    in.host_exchange = c->external_exchange || c->shm.slots;
    in.host_diagnostics = c->timing == 2 || c->ix.dbg;
    in.device_solves = mode_device_solves(c->cfg.mode);
    in.empty_share_alone = c->n_loc == 0 && !c->comm;
    in.host_passes_since_bailout = c->host_passes_since_bailout;
    in.identity = c->cfg.corr == SYMMICP_CORR_IDENTITY;
    in.tree = c->cfg.corr == SYMMICP_CORR_TREE;
    in.incremental = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL;
    in.certificates = c->cert && !c->sw.no_cert;
    in.no_loop_stragglers = c->sw.no_loop_stragglers;
    in.n_s_total = c->n_s_total;
    in.fb = c->fb;
    return batch_eligible(in);
}

static constexpr int kListBlocks = 8;      // partial columns of the straggler stage
static constexpr int kEvSampleStride = 4;  // timing mode 3: passes of a device-driven run that carry events

// A device-driven run: what its chunks share
struct BatchRun {
    LoopConfig lc;
    PassArgs a;
    ChunkPlanner planner;
    bool tree, vec4;
    bool timed;                      // timing modes 1 and 3: passes carry events, every ev_stride-th of the run
    int ev_stride;
    int want, it0;                   // passes asked for; c->iters at entry
    int blocks_full;                 // partial columns of a pass without the straggler stage
    uint32_t *counters;              // the work list's counters (TREE)
    int enq, n_stage;                // passes enqueued so far; passes that ran with the straggler stage
    uint8_t pass_kernel[symmicp_ctx::kRing];      // by iteration % kRing: 1 = the certified-only kernel ran (or was to run) that pass
    symmicp_sums last0;              // loop log: the record the solve-only launch solves from
    PassFeedback fb0;                // the feedback of the host pass in front of the run
};
// ... and one chunk of it
struct Chunk {
    int nq, it_before, ev_used0;     // passes; c->iters and c->ev_used in front of it
    bool certified, stage;           // the certified-only kernel runs its passes; they carry the straggler stage
    int fused_blocks, blocks;        // grid of the pass kernel; partial columns in all
};

static LoopConfig make_loop_config(const symmicp_ctx *c, int want)
{
    LoopConfig lc{};
    lc.mode = c->cfg.mode; lc.fixed_iters = c->cfg.fixed_iters; lc.max_iters = c->iters + want;
    lc.incremental = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL ? 1 : 0; lc.tree = c->cfg.corr == SYMMICP_CORR_TREE ? 1 : 0;
    lc.diff_threshold = c->cfg.diff_threshold; lc.eps_rotation = c->cfg.eps_rotation; lc.eps_translation = c->cfg.eps_translation;
    lc.nrm_w = (c->cfg.mode == SYMMICP_MODE_QUIRKS) ? 1.0f : 0.0f;
    for (int k = 0; k < 3; k++) lc.pivot[k] = c->pivot[k];
    lc.uncertified_limit = loop_slow_limit(c->n_s_total);
    lc.list_limit = kLoopListLimit;
    if (lc.max_iters > c->cfg.max_iters) lc.max_iters = c->cfg.max_iters;
    return lc;
}

// The run's constants, the loop state as the host loop left it (in device memory), the pass arguments and the grid
static int begin_batch(symmicp_ctx *c, BatchRun &run, int want)
{
    const bool incr = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL;
    run.tree = c->cfg.corr == SYMMICP_CORR_TREE;
    run.want = want; run.it0 = c->iters; run.fb0 = c->fb;
    run.lc = make_loop_config(c, want);
    const int cert_mode = (run.tree && c->cert && !c->sw.no_cert && !c->cert_pass_failed) ? c->sw.cert_pass : 0;
    const bool one_piece = run.lc.fixed_iters && !(run.lc.eps_rotation > 0.f && run.lc.eps_translation > 0.f);
    run.planner = ChunkPlanner(run.tree && !c->sw.no_loop_stragglers, c->fb.has_list(), cert_mode, one_piece, c->sw.cert_head);
    LoopState ls{};
    std::memcpy(ls.X, c->X, sizeof(ls.X));
    for (int k = 0; k < 12; k++) ls.Xapply.m[k] = c->X[k];
    ls.Xapply.nrm_w = run.lc.nrm_w;
    ls.iters = run.it0;
    *c->h_loop = ls;
    if (c->loop_log_on) {
        run.last0 = c->last;
        ring_at(c, run.it0).solved = 0;                                        // (the solve-only launch writes its entry only when it solves)
    }
    HIP_TRY(c, hipMemcpyAsync(c->d_loop, c->h_loop, sizeof(LoopState), hipMemcpyHostToDevice, c->stream));
    fill_pass_args(c, run.a, RejectArgs{}, plan_pass(c, /*first=*/false, /*writeback=*/incr), c->X, /*from_cur=*/incr, /*writeback=*/incr, /*first=*/false);      // (batch_eligible: no rejector)
    run.a.loop = c->d_loop;
    if (run.tree) run.blocks_full = fused_pass_blocks(c->n_loc, c->sw.fused_blocks);
    else {
        const IdentityGrid g = identity_grid(c->n_loc, c->n_t, c->src_off, c->sw.id_blocks);
        run.blocks_full = g.blocks; run.vec4 = g.vec4;
    }
    c->pass_blocks = run.blocks_full;
    run.counters = run.tree ? c->wl_count : nullptr;
    run.timed = c->timing == 1 || c->timing == 3;
    run.ev_stride = c->timing == 3 ? kEvSampleStride : 1;      // mode 3: every 4th pass of the run
    if (run.timed && c->ev_used + want > symmicp_ctx::kEvRing) flush_events(c);
    return SYMMICP_OK;
}

// The chunk `plan` asks for: its variant of the pass (partial columns, what a non-empty list means to the solve)
static Chunk begin_chunk(symmicp_ctx *c, BatchRun &run, const ChunkPlan &plan)
{
    Chunk ch{};
    ch.nq = (run.want - run.enq < plan.passes) ? run.want - run.enq : plan.passes;
    ch.it_before = c->h_loop->iters;
    ch.ev_used0 = c->ev_used;
    ch.certified = plan.certified;
    ch.stage = run.planner.stragglers();
    // (with the stage: 512 partial columns in all, k_reduce_solve's fast path)
    ch.fused_blocks = (ch.stage && run.blocks_full + kListBlocks > 512) ? 512 - kListBlocks : run.blocks_full;
    ch.blocks = ch.fused_blocks + (ch.stage ? kListBlocks : 0);
    run.a.partial_cols = ch.stage ? (uint32_t)ch.blocks : 0u;
    run.a.partial_col0 = (uint32_t)ch.fused_blocks;
    run.lc.walk_in_loop = ch.stage ? 1 : 0;
    return ch;
}

// Pass p of the chunk: (pass, reduce, [all-reduce,] solve)
static int enqueue_pass(symmicp_ctx *c, BatchRun &run, const Chunk &ch, int p)
{
    hipEvent_t *ev = nullptr;
    if (run.timed && (run.enq + p) % run.ev_stride == 0 && c->ev_used < symmicp_ctx::kEvRing) {
        ev = c->ev + c->ev_used * symmicp_ctx::kEvPer;
        c->ev_split[c->ev_used] = 1;
        c->ev_weight[c->ev_used] = 1;
        hipEventRecord(ev[0], c->stream);
    }
    if (run.tree) {
        run.pass_kernel[ring_slot(ch.it_before + 1 + p)] = ch.certified ? 1 : 0;      // (the pass this launch is when no stop comes before it)
        if (ch.certified) launch_pass_certified(run.a, c->ix, c->wl, ch.fused_blocks, c->stream);
        else launch_pass_fused(run.a, c->ix, c->wl, ch.fused_blocks, c->stream);
        if (ch.stage) launch_loop_stragglers(run.a, c->ix, c->wl, kListBlocks, c->sw.tune, c->stream);
    }
    else launch_pass_identity(run.a, c->tgt, ch.blocks, run.vec4, c->stream);
    if (ev) { hipEventRecord(ev[4], c->stream); c->ev_used++; }
    if (!(c->comm || ch.blocks > 512)) {
        launch_reduce_solve(c->partials, ch.blocks, c->d_sums, 0, c->d_loop, run.lc, c->h_ring_dev, symmicp_ctx::kRing, run.counters, c->stream);
        return SYMMICP_OK;
    }
    // sharded: the record is summed over the ranks before the solve; many partial records (an 8M-point identity pass): the 40-block
    // reduce is faster than one block's
    launch_final_reduce(c->partials, ch.blocks, c->d_sums, nullptr, c->ticket, 0ull, run.counters, 0, c->stream);
    if (c->comm) {
        if (ev) { hipEventRecord(ev[6], c->stream); c->ev_coll[c->ev_used - 1] = 1; }
        if (int st = allreduce_record(c)) {
            // passes are already queued behind this point and (incremental mode) write into `cur`: drain the stream and make the
            // context ask for a fresh symmicp_begin -- its loop state no longer describes device memory
            (void)hipStreamSynchronize(c->stream);
            c->begun = false;
            c->ev_used = 0;
            return st;
        }
        if (ev) hipEventRecord(ev[7], c->stream);
    }
    launch_reduce_solve(c->partials, ch.blocks, c->d_sums, 1, c->d_loop, run.lc, c->h_ring_dev, symmicp_ctx::kRing, run.counters, c->stream);
    return SYMMICP_OK;
}

// The end of a chunk: the loop state comes back, the events of launches that did nothing go
static int close_chunk(symmicp_ctx *c, BatchRun &run, const Chunk &ch)
{
    const unsigned long long seq = ++c->batch_seq;
    launch_loop_end(c->d_loop, c->h_loop_dev, c->h_done_dev, seq, c->stream);
    if (int st = wait_for_word(c, c->h_done, seq, 60.0, "batch finished without publishing its end flag")) return st;
    // passes of this chunk that did run (a pass that has to be redone ran too); the events of the no-op launches behind a stop are dropped
    const int ran = (c->h_loop->iters - ch.it_before) + (c->h_loop->reason == LOOP_REDO_PASS ? 1 : 0);
    if (run.timed && ran >= 0) {
        int sampled_ran = 0;                      // event pairs of the passes that ran; each stands for the passes up to the next pair
        for (int p = 0; p < ran && p < ch.nq; p++) {
            if ((run.enq + p) % run.ev_stride != 0) continue;
            if (ch.ev_used0 + sampled_ran < symmicp_ctx::kEvRing) {
                const int left = (ran < ch.nq ? ran : ch.nq) - p;
                c->ev_weight[ch.ev_used0 + sampled_ran] = left < run.ev_stride ? left : run.ev_stride;
            }
            sampled_ran++;
        }
        if (ch.ev_used0 + sampled_ran < c->ev_used) c->ev_used = ch.ev_used0 + sampled_ran;
    }
    run.enq += ch.nq;
    if (ch.stage) run.n_stage += c->h_loop->iters - ch.it_before;
    return SYMMICP_OK;
}

// The ring into the context: on return c->iters, c->X, c->last and c->fb describe the last complete pass
static int finish_batch(symmicp_ctx *c, const BatchRun &run, float *diffs_before, int *n_done, bool *small_step)
{
    const LoopState &hl = *c->h_loop;
    const int it0 = run.it0, it1 = hl.iters;          // passes complete
    if (it1 < it0 || it1 > it0 + run.want) return fail(c, SYMMICP_ERR_HIP, "device loop state out of range");
    // the diffs the reference prints before iterations it0+1 .. it1 (+1 when the loop went on into a pass that was not completed)
    for (int k = it0; k < it1; k++) diffs_before[k - it0] = (k == it0) ? (float)c->last.s[33] : (float)ring_at(c, k).sums[33];
    if (it1 > it0) {
        const LoopRecord &r = ring_at(c, it1);
        std::memcpy(c->last.s, r.sums, sizeof(double) * kNSum);
        std::memcpy(c->X, ring_at(c, it1 - 1).X, sizeof(float) * 16);      // transform the last complete pass applied
        c->st.passes += it1 - it0;
        c->st.loop_passes += it1 - it0;
        c->st.loop_straggler_passes += run.n_stage;
        if (run.tree) { c->fb.set_list_from_record(r.list_len); c->fb.set_counts_from_record(r.searched, r.scans); }
    }
    if (!run.tree) c->fb.forget_list();
    c->iters = it1;
    *n_done = it1 - it0;
    *small_step = hl.reason == LOOP_DONE && hl.small_step != 0;
    const bool redo = hl.reason == LOOP_REDO_PASS;
    if (redo && run.pass_kernel[ring_slot(it1 + 1)]) c->cert_pass_failed = true;
    if (c->sw.debug_host) print_batch_summary(c, it0, it1, run.want, run.enq, run.n_stage, run.pass_kernel, run.fb0);
    if (hl.reason == LOOP_SLOW) c->host_passes_since_bailout = 1;      // one host pass, then look again
    if (redo || hl.reason == LOOP_HOST_SOLVE) {
        c->host_passes_since_bailout = 0;
        c->fb.forget_list();                          // the host's next pass runs the full search
        c->st.kernel_launches[7]++;                   // counted with the repairs
    }
    return SYMMICP_OK;
}

// the batch's passes: it0 (the host's last pass, whose record the solve-only launch solved from) .. the last complete one
static void append_loop_log(symmicp_ctx *c, const BatchRun &run)
{
    const LoopState &hl = *c->h_loop;
    const int it0 = run.it0, it1 = hl.iters;
    for (int k = it0; k <= it1; k++) {
        const LoopRecord &r = ring_at(c, k);
        symmicp_loop_log_entry e{};
        std::memcpy(e.sums, k == it0 ? run.last0.s : r.sums, sizeof(e.sums));
        std::memcpy(e.increment, r.increment, sizeof(e.increment));
        std::memcpy(e.X, r.X, sizeof(e.X));
        e.rcond = r.rcond; e.iter = k; e.status = r.status; e.solved = r.solved; e.list_len = k == it0 ? 0 : r.list_len;
        e.reason = hl.reason; e.batch = c->loop_log_batches;
        // which kernel ran the pass (0: k_pass_fused or the host, 1: k_pass_certified); + 0x100 on the batch's last entry when the pass
        // behind it ran certified-only and was handed back incomplete
        e.reserved = k == it0 ? 0 : run.pass_kernel[ring_slot(k)];
        if (k == it1 && hl.reason == LOOP_REDO_PASS && run.pass_kernel[ring_slot(it1 + 1)]) e.reserved |= 0x100;
        if (!e.solved) { std::memset(e.increment, 0, sizeof(e.increment)); std::memset(e.X, 0, sizeof(e.X)); e.rcond = 0.f; e.status = -1; }
        c->loop_log.push_back(e);
    }
    c->loop_log_batches++;
}

// Runs up to `want` iterations on the device.  On return c->iters, c->X and c->last describe the last COMPLETE pass, exactly as
// if symmicp_step had been called (c->iters - iters_before) times; diffs_before[k] = the diff the reference prints before
// iteration iters_before + 1 + k.  *small_step: the increment rule ended the alignment.
static int run_batch(symmicp_ctx *c, int want, float *diffs_before, int *n_done, bool *small_step)
{
    *n_done = 0;
    *small_step = false;
    if (want > symmicp_ctx::kRing - 1) want = symmicp_ctx::kRing - 1;
    if (want <= 0) return SYMMICP_OK;
    BatchRun run{};
    if (int st = begin_batch(c, run, want)) return st;
    ChunkPlan plan = run.planner.next(c->fb.list_len, c->fb.scans, want, 0);
    while (run.enq < want) {
        const Chunk ch = begin_chunk(c, run, plan);
        // the record of the last complete pass is in d_sums: solve from it first
        if (run.enq == 0) launch_reduce_solve(c->partials, ch.blocks, c->d_sums, 2, c->d_loop, run.lc, c->h_ring_dev, symmicp_ctx::kRing, run.counters, c->stream);
        for (int p = 0; p < ch.nq; p++)
            if (int st = enqueue_pass(c, run, ch, p)) return st;
        if (int st = close_chunk(c, run, ch)) return st;
        if (c->h_loop->stop) break;
        if (run.tree) {
            bool any_list = false;
            for (int k = ch.it_before + 1; k <= c->h_loop->iters; k++) any_list = any_list || ring_at(c, k).list_len > 0;
            run.planner.after_chunk(any_list);
        }
        const LoopRecord &lr = ring_at(c, c->h_loop->iters);      // the last complete pass (this chunk completed one: no stop)
        plan = run.planner.next((uint64_t)lr.list_len, (uint64_t)lr.scans, want - run.enq, plan.passes);
    }
    if (int st = finish_batch(c, run, diffs_before, n_done, small_step)) return st;
    if (c->loop_log_on) append_loop_log(c, run);
    return SYMMICP_OK;
}

static int check_ready(symmicp_ctx *c)
{
    if (!c->tgt_block || !c->src0_block) return fail(c, SYMMICP_ERR_STATE, "source and target must be set first (myicp.cpp:102)");
    if (ndt_mode(c)) {
        // (cfg.corr is not read: none of the rules below applies)
        if (c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "SYMMICP_MODE_NDT runs on single-rank contexts only");
        if (!c->ndt.map.valid) return fail(c, SYMMICP_ERR_STATE, "the target's NDT map is missing");
        return SYMMICP_OK;
    }
    if (c->cfg.corr == SYMMICP_CORR_IDENTITY && c->n_s_total != c->n_t)
        return fail(c, SYMMICP_ERR_SIZE, "identity pairing needs N_s == N_t (func.cpp:21)");
    if (c->cfg.corr == SYMMICP_CORR_TREE && !c->have_index) return fail(c, SYMMICP_ERR_STATE, "target index missing");
    if (c->cfg.corr != SYMMICP_CORR_IDENTITY && !c->ix.tq) return fail(c, SYMMICP_ERR_STATE, "target was set under a different corr mode");
    if (c->cfg.mode == SYMMICP_MODE_COLOR) {
        if (c->nranks > 1) return fail(c, SYMMICP_ERR_STATE, "SYMMICP_MODE_COLOR runs on single-rank contexts only");
        if (!c->have_src_int || !c->have_tgt_color)
            return fail(c, SYMMICP_ERR_STATE, "SYMMICP_MODE_COLOR needs symmicp_set_source_intensity and symmicp_set_target_intensity after the clouds");
    }
    return SYMMICP_OK;
}

static void fill_iter(symmicp_ctx *c, symmicp_iter_result *out, int status, float rcond, const float *incr)
{
    if (!out) return;
    out->status = status;
    out->iter = c->iters;
    out->diff = (float)c->last.s[33];
    out->rcond = rcond;
    out->pairs = c->last.s[(c->loss != SYMMICP_LOSS_NONE || ndt_mode(c)) ? 37 : 34];      // (with a robust loss, and in NDT, slot 34 is the sum of the weights)
    if (incr) std::memcpy(out->increment, incr, sizeof(float) * 16); else identity16(out->increment);
    out->sums = c->last;
}

int symmicp_begin(symmicp_ctx *c, const float *guess16, symmicp_iter_result *out)
{
    if (!c) return SYMMICP_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->device));
    int st = check_ready(c);
    if (st != SYMMICP_OK) return st;
    if (guess16) std::memcpy(c->X, guess16, sizeof(float) * 16); else identity16(c->X);
    c->iters = 0;
    const bool incr = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL;
    // incremental: cur <- X * src0 (write-back); cumulative: read src0 through X every pass
    st = run_pass(c, c->X, /*from_cur=*/false, /*writeback=*/incr, /*first=*/true);
    if (st != SYMMICP_OK) return st;
    c->begun = true;
    c->sums_exchanged = false;
    fill_iter(c, out, SYMMICP_OK, 1.0f, nullptr);
    return SYMMICP_OK;
}

int symmicp_step(symmicp_ctx *c, symmicp_iter_result *out)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!c->begun) return fail(c, SYMMICP_ERR_STATE, "symmicp_step before symmicp_begin");
    if (c->external_exchange && !c->sums_exchanged)
        return fail(c, SYMMICP_ERR_STATE, "external exchange: symmicp_set_sums(total over ranks) must follow every pass");
    c->sums_exchanged = false;
    HIP_TRY(c, hipSetDevice(c->device));
    float pbar[3], qbar[3], a[3], t[3], rc = 0.f, Xi[16];
    int st = (c->cfg.mode == SYMMICP_MODE_P2P) ? solve_p2p(c->last, c->pivot, &rc, Xi) : solve_mode(mode_solves_as(c->cfg.mode), c->last, c->pivot, pbar, qbar, a, t, &rc, Xi);
    if (st != SYMMICP_OK) {
        c->err = "degenerate system (rank-deficient normal equations or non-finite transform; func.cpp:70,96)";
        fill_iter(c, out, st, rc, nullptr);
        return st;
    }
    mat4_mul(Xi, c->X, c->X);                     // myicp.cpp:138
    const bool incr = resolved_apply(c->cfg) == SYMMICP_APPLY_INCREMENTAL;
    st = incr ? run_pass(c, Xi, true, true, false) : run_pass(c, c->X, false, false, false);
    if (st != SYMMICP_OK) return st;
    c->iters++;
    fill_iter(c, out, SYMMICP_OK, rc, Xi);
    return SYMMICP_OK;
}

// ---- the reference's result block (myicp.cpp:146-149) --------------------------------------------------------------
// `std::cout << matrix` with Eigen's default IOFormat: every coefficient through the stream's default float formatting (precision 6:
// what "%g" prints), right-aligned to the widest coefficient OF THAT MATRIX, columns separated by one space, rows by a newline
// (Eigen/src/Core/IO.h, print_matrix; published behaviour -- Eigen is not under /root/reference).
static size_t append_eigen(std::string &out, const float *m, int rows, int cols, int stride)
{
    char cell[16][32];
    size_t width = 0;
    for (int r = 0; r < rows; r++)
        for (int c = 0; c < cols; c++) {
            std::snprintf(cell[r * cols + c], sizeof(cell[0]), "%g", (double)m[r * stride + c]);
            width = std::max(width, std::strlen(cell[r * cols + c]));
        }
    for (int r = 0; r < rows; r++) {
        for (int c = 0; c < cols; c++) {
            if (c) out += ' ';
            const size_t len = std::strlen(cell[r * cols + c]);
            out.append(width - len, ' ');
            out += cell[r * cols + c];
        }
        out += '\n';                 // (rows are separated by "\n"; the reference ends each matrix with std::endl)
    }
    return width;
}

// Affine3f::rotation() is the orthogonal polar factor of the linear part (Eigen computes it as U V^T of a JacobiSVD in fp32): here by
// Newton's iteration R <- (R + R^-T) / 2 in fp64, which converges to the same matrix; for the rigid transforms of this path it differs
// from the linear part in the last bit or two.  A singular linear part is printed as it is.
static void polar_rotation(const float X[16], float R[9])
{
    double A[3][3];
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) A[r][c] = X[4 * r + c];
    for (int it = 0; it < 100; it++) {
        const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) + A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
        if (!(std::fabs(det) > 1e-300) || !std::isfinite(det)) break;
        double inv_t[3][3];          // A^-T = cofactor matrix / det
        inv_t[0][0] = (A[1][1] * A[2][2] - A[1][2] * A[2][1]) / det; inv_t[0][1] = (A[1][2] * A[2][0] - A[1][0] * A[2][2]) / det; inv_t[0][2] = (A[1][0] * A[2][1] - A[1][1] * A[2][0]) / det;
        inv_t[1][0] = (A[0][2] * A[2][1] - A[0][1] * A[2][2]) / det; inv_t[1][1] = (A[0][0] * A[2][2] - A[0][2] * A[2][0]) / det; inv_t[1][2] = (A[0][1] * A[2][0] - A[0][0] * A[2][1]) / det;
        inv_t[2][0] = (A[0][1] * A[1][2] - A[0][2] * A[1][1]) / det; inv_t[2][1] = (A[0][2] * A[1][0] - A[0][0] * A[1][2]) / det; inv_t[2][2] = (A[0][0] * A[1][1] - A[0][1] * A[1][0]) / det;
        double change = 0.0;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) { const double v = 0.5 * (A[r][c] + inv_t[r][c]); change = std::max(change, std::fabs(v - A[r][c])); A[r][c] = v; }
        if (change < 1e-15) break;
    }
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) R[3 * r + c] = std::isfinite(A[r][c]) ? (float)A[r][c] : X[4 * r + c];
}

size_t symmicp_format_result(const float transform16[16], char *buf, size_t cap)
{
    if (!transform16) return 0;
    std::string out = "Result transform:\n";
    append_eigen(out, transform16, 4, 4, 4);
    out += "  rotation:\n";
    float R[9];
    polar_rotation(transform16, R);
    append_eigen(out, R, 3, 3, 3);
    out += "  translation:\n";
    append_eigen(out, transform16 + 3, 3, 1, 4);
    if (buf && cap) {
        const size_t n = std::min(out.size(), cap - 1);
        std::memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return out.size();
}

int symmicp_align(symmicp_ctx *c, const float *guess16, symmicp_result *out)
{
    if (!c || !out) return SYMMICP_ERR_ARG;
    std::memset(out, 0, sizeof(*out));
    if (c->external_exchange) { out->status = SYMMICP_ERR_STATE; return fail(c, SYMMICP_ERR_STATE, "symmicp_align is not available with external exchange: drive begin/set_sums/step"); }
    const double t0 = now_s();
    c->cert_pass_failed = false;
    c->loop_log.clear();
    c->loop_log_batches = 0;
    symmicp_iter_result it;
    int st = symmicp_begin(c, guess16, &it);
    if (st != SYMMICP_OK) { out->status = st; return st; }
    float diff = it.diff;                                           // myicp.cpp:122
    out->diff_initial = diff;
    int iters = 0;
    // myicp.cpp:123: while (diff > diff_threshold && iters++ < max_iters)
    while ((c->cfg.fixed_iters || diff > c->cfg.diff_threshold) && iters < c->cfg.max_iters) {
        if (may_start_batch(c)) {
            // the same loop, run by the device for the iterations that are left (run_batch); afterwards this loop goes on from the
            // last complete pass -- and ends by its own test where the device loop ended by the same test
            float db[symmicp_ctx::kRing];
            int done = 0;
            bool small = false;
            st = run_batch(c, c->cfg.max_iters - iters, db, &done, &small);
            if (st != SYMMICP_OK) break;
            for (int k = 0; k < done; k++) {
                iters++;
                if (c->cfg.verbose) std::printf("iters#%d\ndiff: %g\n", iters, db[k]);
                if (iters <= 64) out->diffs[iters - 1] = db[k];
            }
            diff = (float)c->last.s[33];
            if (small) break;
            if (done > 0 || c->host_passes_since_bailout == 0) continue;
            // (the device did nothing and asked for nothing: take one step here)
        }
        iters++;
        if (c->cfg.verbose) std::printf("iters#%d\ndiff: %g\n", iters, diff);                       // myicp.cpp:125-126
        if (iters <= 64) out->diffs[iters - 1] = diff;
        st = symmicp_step(c, &it);
        if (st != SYMMICP_OK) { iters--; break; }
        c->host_passes_since_bailout++;
        diff = it.diff;                                             // myicp.cpp:141
        // convergence on the increment (the reference only has the diff threshold, myicp.cpp:123)
        if (c->cfg.eps_rotation > 0.f && c->cfg.eps_translation > 0.f && !c->cfg.fixed_iters && small_increment(it.increment, c->cfg.eps_rotation, c->cfg.eps_translation)) break;
    }
    out->status = st;
    out->iters = iters;
    out->diff_final = diff;
    std::memcpy(out->transform, c->X, sizeof(float) * 16);
    out->seconds_total = now_s() - t0;
    if (c->cfg.verbose) {                                           // myicp.cpp:146-149
        char buf[1024];
        symmicp_format_result(c->X, buf, sizeof(buf));
        std::fputs(buf, stdout);
    }
    return st;
}

int symmicp_solve(int mode, const symmicp_sums *sums, const float pivot[3], float pbar[3], float qbar[3], float a[3],
                  float t[3], float *rcond, float out16[16])
{
    if (!sums || !pbar || !qbar || !a || !t || !out16) return SYMMICP_ERR_ARG;
    if (mode == SYMMICP_MODE_P2P) {
        for (int k = 0; k < 3; k++) pbar[k] = qbar[k] = a[k] = t[k] = 0.f;
        return solve_p2p(*sums, pivot, rcond, out16);
    }
    mode = mode_solves_as(mode);      // (COLOR's record has PLANE's shape)
    return mode_device_solves(mode) ? solve_mode(mode, *sums, pivot, pbar, qbar, a, t, rcond, out16) : SYMMICP_ERR_ARG;
}

// ---- test entry points of the device-driven loop ----
int symmicp_ctx_solve_probe(symmicp_ctx *c, int mode, int exact_rc, const symmicp_sums *sums, size_t n, const float pivot[3], const float *X_in16,
                            int32_t *status, float *pbar, float *qbar, float *a, float *t, float *rcond, float *out16, float *X_out16)
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!mode_device_solves(mode)) return fail(c, SYMMICP_ERR_ARG, "probe: QUIRKS, PAPER, PLANE or GICP");
    if (!sums || n == 0 || n > (1u << 24) || !status || !pbar || !qbar || !a || !t || !rcond || !out16 || (X_in16 && !X_out16))
        return fail(c, SYMMICP_ERR_ARG, "probe: bad arguments");
    HIP_TRY(c, hipSetDevice(c->device));
    // one allocation: records | pivot | X_in | status | pbar qbar a t | rcond | out16 | X_out
    const size_t b_sums = sizeof(symmicp_sums) * n, b_f3 = sizeof(float) * 3 * n, b_16 = sizeof(float) * 16 * n;
    const size_t o_piv = b_sums, o_xin = o_piv + 16, o_st = o_xin + b_16, o_pb = o_st + 4 * n, o_qb = o_pb + b_f3, o_a = o_qb + b_f3, o_t = o_a + b_f3,
                 o_rc = o_t + b_f3, o_out = o_rc + 4 * n, o_xo = o_out + b_16, total = o_xo + b_16;
    char *d = nullptr;
    HIP_TRY(c, hipMalloc((void **)&d, total));
    float piv[4] = {0.f, 0.f, 0.f, 0.f};
    if (pivot) for (int k = 0; k < 3; k++) piv[k] = pivot[k];
    int st = SYMMICP_OK;
    if (hipMemcpy(d, sums, b_sums, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + o_piv, piv, 16, hipMemcpyHostToDevice) != hipSuccess ||
        (X_in16 && hipMemcpy(d + o_xin, X_in16, b_16, hipMemcpyHostToDevice) != hipSuccess))
        st = fail(c, SYMMICP_ERR_HIP, "probe: upload");
    if (st == SYMMICP_OK) {
        launch_solve_probe(mode, exact_rc, (const symmicp_sums *)d, (int)n, (const float *)(d + o_piv), X_in16 ? (const float *)(d + o_xin) : nullptr,
                           (int32_t *)(d + o_st), (float *)(d + o_pb), (float *)(d + o_qb), (float *)(d + o_a), (float *)(d + o_t), (float *)(d + o_rc),
                           (float *)(d + o_out), (float *)(d + o_xo), c->stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) st = fail(c, SYMMICP_ERR_HIP, "probe: kernel");
    }
    if (st == SYMMICP_OK) {
        const struct { size_t off, bytes; void *dst; } back[] = {{o_st, 4 * n, status}, {o_pb, b_f3, pbar}, {o_qb, b_f3, qbar}, {o_a, b_f3, a}, {o_t, b_f3, t},
                                                              {o_rc, 4 * n, rcond}, {o_out, b_16, out16}, {o_xo, X_in16 ? b_16 : 0, X_out16}};
        for (const auto &b : back)
            if (b.bytes && hipMemcpy(b.dst, d + b.off, b.bytes, hipMemcpyDeviceToHost) != hipSuccess) { st = fail(c, SYMMICP_ERR_HIP, "probe: read back"); break; }
    }
    (void)hipFree(d);
    return st;
}

int symmicp_ctx_loop_solve(symmicp_ctx *c, const symmicp_sums *sums, const float pivot[3], const float X_in16[16], const int32_t in_i[6], const float in_f[3],
                           int32_t state_out[4], float X_out16[16], float Xapply_out12[12], float ring_inc16[16], float ring_X16[16], float *ring_rcond,
                           int32_t ring_i2[2])
{
    if (!c) return SYMMICP_ERR_ARG;
    if (!sums || !X_in16 || !in_i || !in_f || !state_out || !X_out16 || !Xapply_out12 || !ring_inc16 || !ring_X16 || !ring_rcond || !ring_i2)
        return fail(c, SYMMICP_ERR_ARG, "loop_solve: bad arguments");
    const int mode = in_i[0];
    if (!mode_device_solves(mode)) return fail(c, SYMMICP_ERR_ARG, "loop_solve: QUIRKS, PAPER, PLANE or GICP");
    HIP_TRY(c, hipSetDevice(c->device));
    LoopConfig lc{};
    lc.mode = mode; lc.fixed_iters = in_i[1]; lc.max_iters = in_i[2]; lc.incremental = in_i[5] ? 1 : 0; lc.tree = 0;
    lc.diff_threshold = in_f[0]; lc.eps_rotation = in_f[1]; lc.eps_translation = in_f[2];
    lc.nrm_w = (mode == SYMMICP_MODE_QUIRKS) ? 1.0f : 0.0f;
    for (int k = 0; k < 3; k++) lc.pivot[k] = pivot ? pivot[k] : 0.f;
    LoopState ls{};
    std::memcpy(ls.X, X_in16, sizeof(ls.X));
    for (int k = 0; k < 12; k++) ls.Xapply.m[k] = X_in16[k];
    ls.Xapply.nrm_w = lc.nrm_w;
    ls.iters = in_i[3];
    ls.small_step = in_i[4];
    // device copies: the record (where the solve-only launch reads it), the loop state, a ring of one entry
    char *d = nullptr;
    const size_t o_loop = 512, o_ring = o_loop + ((sizeof(LoopState) + 255) & ~(size_t)255), total = o_ring + sizeof(LoopRecord);
    HIP_TRY(c, hipMalloc((void **)&d, total));
    int st = SYMMICP_OK;
    if (hipMemcpy(d, sums, sizeof(symmicp_sums), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d + o_loop, &ls, sizeof(ls), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d + o_ring, 0xFF, sizeof(LoopRecord)) != hipSuccess)
        st = fail(c, SYMMICP_ERR_HIP, "loop_solve: upload");
    if (st == SYMMICP_OK) {
        launch_reduce_solve(nullptr, 0, (double *)d, 2, (LoopState *)(d + o_loop), lc, (LoopRecord *)(d + o_ring), 1, nullptr, c->stream);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) st = fail(c, SYMMICP_ERR_HIP, "loop_solve: kernel");
    }
    LoopState lo{};
    LoopRecord r{};
    if (st == SYMMICP_OK && (hipMemcpy(&lo, d + o_loop, sizeof(lo), hipMemcpyDeviceToHost) != hipSuccess ||
                             hipMemcpy(&r, d + o_ring, sizeof(r), hipMemcpyDeviceToHost) != hipSuccess))
        st = fail(c, SYMMICP_ERR_HIP, "loop_solve: read back");
    (void)hipFree(d);
    if (st != SYMMICP_OK) return st;
    state_out[0] = lo.stop; state_out[1] = lo.reason; state_out[2] = lo.iters; state_out[3] = lo.small_step;
    std::memcpy(X_out16, lo.X, sizeof(lo.X));
    std::memcpy(Xapply_out12, lo.Xapply.m, sizeof(lo.Xapply.m));
    std::memcpy(ring_inc16, r.increment, sizeof(r.increment));
    std::memcpy(ring_X16, r.X, sizeof(r.X));
    std::memcpy(ring_rcond, &r.rcond, sizeof(float));
    ring_i2[0] = r.status; ring_i2[1] = r.solved;
    return SYMMICP_OK;
}

int symmicp_set_loop_log(symmicp_ctx *c, int on)
{
    if (!c) return SYMMICP_ERR_ARG;
    c->loop_log_on = on != 0;
    if (!c->loop_log_on) { c->loop_log.clear(); c->loop_log.shrink_to_fit(); }
    return SYMMICP_OK;
}

int symmicp_get_loop_log(const symmicp_ctx *c, symmicp_loop_log_entry *out, size_t cap, size_t *count)
{
    if (!c || !count) return SYMMICP_ERR_ARG;
    *count = c->loop_log.size();
    if (out) std::memcpy(out, c->loop_log.data(), sizeof(symmicp_loop_log_entry) * std::min(cap, c->loop_log.size()));
    return SYMMICP_OK;
}

}  // extern "C"
