// engine_debug.cpp -- diagnostics of libsymmicp, off unless asked for: SYMMICP_DEBUG_COUNTERS=1 (per-pass counters of the search kernels on
// stderr) and SYMMICP_DEBUG_TRACE=file (per-packet trace of the first pass, read by scratch/pkt_timeline.py and friends).
#include "engine_internal.h"

// SYMMICP_DEBUG_TRACE=file: the per-packet trace of the first pass that has just run (k_search_packet), then cleared for the next one
static constexpr size_t kTraceWords = (size_t)1 << 22;
void dump_packet_trace(symmicp_ctx *c)
{
    if (FILE *f = std::fopen(c->sw.debug_trace.c_str(), "wb")) {
        std::vector<unsigned long long> t(kTraceWords);
        hipMemcpy(t.data(), c->ix.dbg_trace, t.size() * 8, hipMemcpyDeviceToHost);
        std::fwrite(t.data(), 8, t.size(), f);
        std::fclose(f);
    }
    hipMemset(c->ix.dbg_trace, 0, kTraceWords * 8);
}


// the device-side counters of the pass that has just run (k_search_packet / cells_tile / k_search_walk), then cleared
void print_pass_counters(symmicp_ctx *c, bool first, long long list_len)
{
        unsigned long long h[12];
        hipMemcpy(h, c->ix.dbg, sizeof(h), hipMemcpyDeviceToHost);
        hipMemset(c->ix.dbg, 0, sizeof(h));
        if (first && c->cfg.corr == SYMMICP_CORR_TREE && c->target_surface_like)
            std::fprintf(stderr, "[symmicp dbg] pass %lld (packets): steps=%llu nodes+leaf candidates=%llu leaf candidates rejected=%llu points=%llu tie rescans=%llu overflows=%llu lanes wanting a scanned leaf (sum)=%llu | packet ticks (10 ns): sum=%llu max=%llu\n",
                         (long long)c->st.passes, h[0], h[4], h[5], h[3], h[2], h[1], h[8], h[7], h[6]);
        else
        std::fprintf(stderr, "[symmicp dbg] pass %lld: cells: certified=%llu (by neighbourhood %llu) scans=%llu (neighbourhoods kept %llu, not kept %llu) probes=%llu to-walk=%llu items=%llu points=%llu | walk list=%lld visits=%llu wave-max*64=%llu\n",
                     (long long)c->st.passes, h[1], h[8], h[2], h[9], h[10], h[6], h[7], h[0], h[3], list_len, h[4], h[5]);
}

// SYMMICP_DEBUG_HOST: a device-driven run that has just ended (engine_loop.cpp, run_batch).  Unknown lists and counts print as -1, an
// expected list as -2
void print_batch_summary(const symmicp_ctx *c, int it0, int it1, int want, int enq, int n_stage, const uint8_t *pass_kernel, const PassFeedback &before)
{
    const bool tree = c->cfg.corr == SYMMICP_CORR_TREE;
    auto list_of = [](const PassFeedback &f) { return f.list_known() ? (long long)f.list_len : (f.expects_list() ? -2ll : -1ll); };
    if (it1 - it0 >= 2) {      // (a library built with -DRS_STAMPS leaves k_reduce_solve's phase durations in the spare slots of each record)
        const double *q = ring_at(c, it1 - 1).sums;
        if (q[37] != 0.0) std::fprintf(stderr, "[symmicp host] k_reduce_solve stamps of pass %d: load + reduce %.2f us (loop state there after %.2f us), bookkeeping + solve %.2f us, publish %.2f us\n", it1 - 1, std::floor(q[37]) * 0.01, (q[37] - std::floor(q[37])) * 1e4 * 0.01, q[38] * 0.01, q[39] * 0.01);
    }
    int n_cert = 0;
    for (int k = it0 + 1; k <= it1; k++) n_cert += pass_kernel[ring_slot(k)];
    if (tree) {
        std::fprintf(stderr, "[symmicp host] batch: work list / searched pairs / scanned pairs after each device pass (c: certified-only kernel):");
        for (int k = it0 + 1; k <= it1; k++) {
            const LoopRecord &r = ring_at(c, k);
            std::fprintf(stderr, " %d/%d/%d%s", r.list_len, r.searched, r.scans, pass_kernel[ring_slot(k)] ? "c" : "");
        }
        std::fprintf(stderr, "\n");
    }
    std::fprintf(stderr, "[symmicp host] batch: %d of %d passes on the device (%d enqueued), reason %d, %d with the straggler stage, %d certified-only%s, list after %lld (host pass before: list %lld, scanned %lld)\n", it1 - it0, want, enq, c->h_loop->reason, n_stage, n_cert, c->cert_pass_failed ? " (now off: a pass came back incomplete)" : "", list_of(c->fb), list_of(before), before.counts_known() ? (long long)before.scans : -1ll);
}
