// loop_plan.h -- the scheduling rules of the ICP loop as plain functions over plain values: what a pass tells the next one (PassFeedback and
// the two record slots that carry it), the grid sizes, the plan of one TREE pass, when a device-driven run may start and how it is cut
// into chunks.  engine_loop.cpp launches what these functions decide ("Converged passes", describes the loop); the two
// reduce kernels of kernels_reduce.hip share the slot codec.  Plain C++17: no HIP header, no context, so that a host program can call
// every rule (tests/cpp/loop_plan.cpp).
#pragma once
#include <math.h>
#include <stdint.h>
#include "symmicp.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LOOP_PLAN_HD __host__ __device__
#else
#define LOOP_PLAN_HD
#endif

namespace symmicp {

// ---- what a pass tells the next one -------------------------------------------------------------------------------
// The work list of the last pass (queries handed to the tree walk, all ranks) is known with its length, unknown (no TREE pass since
// set_source, or a device-driven run handed a pass back: the next pass runs the full search), or expected: the packet first pass has no
// work list, and the pass after it (the cloud has just moved by its whole misalignment) always has one -- no optimistic skip of the walk,
// which would only be repaired, and a mid-sized walk grid.  The counts -- pairs the last TREE pass had to search again, and those of them
// that reached a scan, a probe or the walk (all ranks) -- are known after every TREE pass but the first.
struct PassFeedback {
    enum class List : uint8_t { kUnknown, kKnown, kExpected };
    List list = List::kUnknown;
    bool counts = false;
    uint64_t list_len = 0;                 // 0 unless the list is known
    uint64_t searched = 0, scans = 0;      // 0 unless the counts are known

    bool list_known() const { return list == List::kKnown; }
    bool list_empty() const { return list_known() && list_len == 0; }
    bool has_list() const { return list_known() && list_len > 0; }
    bool expects_list() const { return list == List::kExpected; }
    bool counts_known() const { return counts; }

    void set_list(uint64_t len) { list = List::kKnown; list_len = len; }
    void expect_list() { list = List::kExpected; list_len = 0; }
    void forget_list() { list = List::kUnknown; list_len = 0; }
    void set_counts(uint64_t searched_, uint64_t scans_) { counts = true; searched = searched_; scans = scans_; }
    void forget_counts() { counts = false; searched = scans = 0; }
    // from a LoopRecord's int32 words; a word that does not fit them reads as unknown
    void set_list_from_record(int32_t len) { if (len >= 0) set_list((uint64_t)len); else forget_list(); }
    void set_counts_from_record(int32_t searched_, int32_t scans_)
    {
        if (searched_ >= 0 && scans_ >= 0) set_counts((uint64_t)searched_, (uint64_t)scans_); else forget_counts();
    }
};

// TREE passes: the final reduce leaves the feedback in the record's two spare slots, where it is summed over the ranks like every other
// slot.  The list slot carries the work list's length; appends dropped for lack of room (must not happen) add kListDropped to it, so that
// the flag survives the sum.  The count slot carries two counts: the pairs searched (below 2^32) + kScanUnit x those of them that reached
// a scan: both stay exact in the sum over ranks (the slot is a double: while the scanned pairs of all ranks stay below 2^21; the rules
// below ask about far fewer).  (Slot 37 is a sum: the pair count of a weighted record.)
constexpr int kFeedbackListSlot = SYMMICP_NSUM - 1, kFeedbackCountSlot = SYMMICP_NSUM - 2;
constexpr double kListDropped = 4294967296.0;
constexpr double kScanUnit = 4294967296.0;
struct FeedbackSlots { double list, count; };
// what the slots say: whole numbers (list_len below 2^32 and meaningful only when nothing was dropped)
struct FeedbackWords {
    double list_len;
    bool dropped;
    double searched, scans;
};
LOOP_PLAN_HD inline FeedbackSlots feedback_encode(uint32_t len, bool dropped, uint32_t searched, uint32_t scans)
{
    return FeedbackSlots{(double)len + (dropped ? kListDropped : 0.0), (double)searched + (double)scans * kScanUnit};
}
LOOP_PLAN_HD inline FeedbackWords feedback_decode(double list_slot, double count_slot)
{
    FeedbackWords w;
    w.list_len = list_slot;
    w.dropped = list_slot >= kListDropped;
    w.scans = floor(count_slot / kScanUnit);
    w.searched = count_slot - w.scans * kScanUnit;
    return w;
}

// ---- grid sizes ---------------------------------------------------------------------------------------------------
constexpr uint32_t kPlanTile = 256;      // points per block and trip of every pass kernel (kPassThreads)
inline uint32_t plan_tiles(uint32_t n_items) { return (n_items + kPlanTile - 1) / kPlanTile; }
// blocks for n_items: one per tile up to the cap, optionally a multiple of 8 below it (the XCD remap), never under the floor
inline int capped_blocks(uint32_t n_items, int cap, bool round_to_8, int floor_blocks)
{
    const int tiles = (int)plan_tiles(n_items);
    int b = tiles < cap ? (round_to_8 ? ((tiles + 7) / 8) * 8 : tiles) : cap;
    if (b < floor_blocks) b = floor_blocks;
    return b;
}
// The number of partial columns fixes the order of the fp64 sums of a pass, so these caps are part of what a run computes: none of them
// may change, and a grid that two callers size must come out the same in both.
// the single pass kernel of a host pass (brute-force pairs; identity pairs whose columns cannot be read 16 bytes at a time)
inline int host_pass_cap(int pass_blocks) { return pass_blocks > 8192 ? 8192 : pass_blocks; }
// the accumulate kernel is streaming with a 40-value block reduction at the end of every block: 2 blocks per CU measured best (18 us at
// 512 blocks, 23 us at 2048, 1M points); a multiple of 8 for the XCD remap.  (A rank whose share is empty still writes its zero record.)
inline int accumulate_blocks(uint32_t n_loc, int acc_cap) { return capped_blocks(n_loc, acc_cap, true, 8); }
// NDT: one accumulating kernel over (point, voxel) items, its grid capped like the others' (2 blocks per CU)
inline int ndt_blocks(uint32_t n_loc, int acc_cap) { return capped_blocks(n_loc, acc_cap, false, 1); }
// the fused pass of a device-driven run (an empty share still writes its zero record)
inline int fused_pass_blocks(uint32_t n_loc, int fused_cap) { return capped_blocks(n_loc, fused_cap, false, 1); }
// Identity pairing: 16-byte column loads need every planar column (length n_loc / n_t) and the shard offset to keep 16-B alignment; a
// block then covers four points per thread.  The host pass caps the 16-byte grid by id_blocks and the other one by
// host_pass_cap(pass_blocks); the device loop caps both by id_blocks.  The two defaults are equal (2048); the difference is kept as it
// is because of the summation order (above).
struct IdentityGrid { int blocks; bool vec4; };
inline bool identity_vec4(uint32_t n_loc, uint32_t n_t, uint32_t src_off) { return (n_loc % 4 == 0) && (n_t % 4 == 0) && (src_off % 4 == 0); }
inline IdentityGrid identity_grid(uint32_t n_loc, uint32_t n_t, uint32_t src_off, int cap)
{
    const bool vec4 = identity_vec4(n_loc, n_t, src_off);
    return IdentityGrid{capped_blocks(vec4 ? n_loc / 4 : n_loc, cap, false, 1), vec4};
}

// ---- one TREE pass ------------------------------------------------------------------------------------------------
struct TreePassIn {
    bool first, writeback, rejecting;
    PassFeedback fb;                 // of the pass before
    uint32_t n_s_total, n_loc;
    int nranks;
    bool use_slack;                  // the pass honours the pair certificates (not the first of an alignment)
    bool have_certk;                 // neighbourhood certificates exist
    // switches (Switches, engine_internal.h)
    bool walk_full_grid;
    int optimistic, compact, budget_walk;      // -1 auto, 0 never, 1 always
    double hood_frac;
    int acc_blocks, compact_blocks;
};
struct TreePassPlan {
    int acc_blocks;                  // grid of the accumulating kernel = partial columns of the pass
    uint32_t walk_blocks;            // grid of k_search_walk; 0 = full grid
    bool optimistic;                 // the walk is skipped and the pass repaired if the list turns out non-empty
    int compact_blocks;              // > 0: the cell search runs as the streaming, compacting kernel on that many blocks
    bool make_hood;                  // scans keep neighbourhoods
    bool budget_walk;                // the thread-per-query walk runs with a visit budget + retry launch
};
constexpr uint64_t kWalkSizedListMax = 50000;      // work lists up to this length get a walk grid sized from them
// the walk grid of the repair of an optimistic pass whose list (list_len > 0) turned up after all
inline uint32_t repair_walk_blocks(uint64_t list_len) { return list_len <= kWalkSizedListMax ? 8192u : 0u; }

inline TreePassPlan plan_tree_pass(const TreePassIn &in)
{
    TreePassPlan p{};
    p.acc_blocks = accumulate_blocks(in.n_loc, in.acc_blocks);
    // Walk grid: any size is correct (the kernel strides over the list); sized from the previous pass's list length, which only shrinks
    // while an alignment converges.  Unknown or long lists get the full grid.
    if (!in.first && in.fb.list_known() && in.fb.list_len <= kWalkSizedListMax) {
        p.walk_blocks = (uint32_t)(2 * in.fb.list_len);
        if (p.walk_blocks < 256u) p.walk_blocks = 256u;
        if (p.walk_blocks > 8192u) p.walk_blocks = 8192u;
    }
    if (!in.first && in.fb.expects_list()) p.walk_blocks = 16384u;
    if (in.walk_full_grid) p.walk_blocks = 0;
    // Once an alignment has converged the work list stays empty (every pair is certified or settled by the cell scan), and an empty
    // walk launch still costs ~6 us of a ~50 us pass.  So after a pass with an empty list the walk is skipped; the final reduce reports
    // the list's length, and in the rare case that it is not empty after all the pass is repaired (walk, accumulate and reduce again).
    p.optimistic = in.optimistic >= 0 ? in.optimistic == 1 : (!in.first && in.fb.list_empty());      // (SYMMICP_OPTIMISTIC: "0" never, "1" always)
    if (in.writeback) p.optimistic = false;      // in-place write-back: a repair would transform the cloud twice
    if (in.rejecting) p.optimistic = false;      // the keys are taken from final pairs
    // Sparse scans (the previous pass searched under a tenth of the pairs): the streaming kernel compacts the failures of several tiles
    // into full scan rounds; blocks enough to fill the chip at 5 waves per SIMD
    const bool compact = in.use_slack && (in.compact >= 0 ? in.compact == 1 : (in.fb.counts_known() && in.fb.searched < (uint64_t)(in.n_s_total / 10)));
    p.compact_blocks = compact ? in.compact_blocks : 0;
    // neighbourhoods are worth their stores once the alignment is settling (the previous pass searched under 80 % of the pairs: 8M scan pair
    // 2 680 iter/s at 50 %, 2 776 at 80 %, 2 742 always; 1M surface pair 16 050 / 15 960 / 15 700)
    p.make_hood = in.have_certk && !in.first && in.fb.counts_known() && (double)in.fb.searched < in.hood_frac * (double)in.n_s_total;
    // sharded runs: the first pass over a small share is bound by its slowest walks, not by throughput
    p.budget_walk = in.budget_walk >= 0 ? in.budget_walk != 0 : (in.first && in.nranks > 1 && in.n_loc < 400000u);      // (SYMMICP_BUDGET_WALK: "0" never, "1" always)
    return p;
}

// ---- device-driven runs of passes: when one may start -------------------------------------------------------------
// work lists up to this length are walked inside a device-driven loop (straggler stage); longer ones go back to the host, which sizes the walk
constexpr uint32_t kLoopListLimit = 8192;
// Scans are what the fused pass is slow at (two waves per SIMD: a dense cell's dependent loads are not hidden; ~6 ns per scanned pair
// against 0.3 in k_search_cells), so a run starts once the last pass searched under 0.4 % of the pairs and under 8192 of them -- the
// separate kernels win above that whatever the cloud's size (8M scan pair: 328 us fused against 150 + 80 at 30 k scans) -- and is left
// (LOOP_SLOW) at four times as many.
inline uint32_t loop_scan_limit(uint32_t n) { const uint32_t f = n / 256; return f < 8192u ? f : 8192u; }
inline uint32_t loop_slow_limit(uint32_t n) { return 4 * loop_scan_limit(n); }

struct BatchEligibleIn {
    bool host_loop_switch;           // SYMMICP_HOST_LOOP=1
    bool rejecting;                  // the passes run a rejector
    bool color;                      // SYMMICP_MODE_COLOR
    bool host_loop_config;           // symmicp_config::host_loop
    bool host_exchange;              // the records are exchanged on the host (external or shared-memory exchange)
    bool host_diagnostics;           // per-kernel timing tables or debug counters
    bool device_solves;              // mode_device_solves
    bool empty_share_alone;          // an empty share outside an RCCL run
    int host_passes_since_bailout;
    bool identity, tree;             // the correspondence kind (neither: brute force)
    bool incremental;
    bool certificates;               // pair certificates exist and are not switched off
    bool no_loop_stragglers;         // SYMMICP_NO_LOOP_STRAGGLERS
    uint32_t n_s_total;
    PassFeedback fb;
};
inline bool batch_eligible(const BatchEligibleIn &in)
{
    if (in.host_loop_switch) return false;                                // SYMMICP_HOST_LOOP=1: never batch (A/B runs, tests)
    if (in.rejecting) return false;                                       // trimmed and other rejecting passes: the fused pass and the device loop have no select
    if (in.color) return false;                                           // colored ICP: the fused pass and the straggler stage have no COLOR form
    if (in.host_loop_config) return false;
    if (in.host_exchange) return false;                                   // those exchanges run on the host
    if (in.host_diagnostics) return false;                                // per-kernel tables and debug counters: host loop
    if (!in.device_solves) return false;                                  // (P2P: 3x3 SVD by Jacobi sweeps: host)
    if (in.empty_share_alone) return false;                               // (an empty share of an RCCL run takes part: every input below is global,
                                                                          // and a rank that stayed in the host loop would issue a different number of all-reduces)
    if (in.host_passes_since_bailout < 2) return false;
    if (in.identity) return true;
    // TREE: the fused pass is for converged alignments: under 0.4 % of the pairs searched again, a short work list at most (stragglers
    // outside the overlap: real scans always have some)
    if (in.tree)
        return !in.incremental && in.fb.list_known() && in.fb.list_len <= (in.no_loop_stragglers ? 0u : kLoopListLimit) && in.fb.counts_known() &&
               in.fb.searched <= loop_scan_limit(in.n_s_total) / (in.fb.list_len > 0 ? 2u : 1u) && in.certificates;      // (the straggler stage costs two launches per pass)
    return false;
}

// ---- device-driven runs of passes: their chunks -------------------------------------------------------------------
// Passes are enqueued in chunks with one look at the loop state between chunks: a loop that stops early (convergence, a pass that has
// to be redone) leaves at most one chunk of no-op launches behind.  The plan of the next chunk comes from the last complete pass (its work
// list and scan count; `left` passes to go, `prev` passes in the chunk before, 0: none): which kernel runs it and how many passes it
// holds.  All of the chunking is here: with the straggler stage on, chunks stay at 4 (the stage can only be dropped between chunks); a run
// that can stop by itself doubles them (4, 8, 16, ...); a run that only a bail-out can stop sends fused heads while passes still scan and
// then the rest in one piece.
//
// Stragglers: while passes leave a work list, every fused pass is followed by the walk over the list and the accumulation of its pairs (two
// more launches per pass, ~10 us); decided per chunk of passes from the lists the previous chunk left.  Without the stage a list that turns
// up stops the loop: the host redoes that pass and the next run starts with the stage.  With the stage on, chunks stay short: lists die
// out within a few passes of a run's start (8M scan pair: 8 8 6 2 | 2 0 1 0 | 0 ...); once it is off and only a bail-out can stop the
// run, the rest goes out in one piece.
//
// The certified-only pass (k_pass_certified) runs a chunk when the last complete pass left no work list and sent no pair to a scan (and
// the chunk carries no straggler stage); a pass of it that comes back incomplete is redone by the host like any pass with an unexpected
// list, and the kernel is then left alone for the rest of the alignment: one repeated pass at most.  cert_mode (SYMMICP_CERT_PASS, 0 for
// runs that cannot use the kernel): 0 never, 1 by this rule, 2 from the first device pass whatever the counts say and without the
// straggler stage (tests of the redo path, A/B runs).
//
// One piece: a run that only a bail-out can stop -- fixed iteration count, no increment criterion, no work list at entry -- is enqueued in
// one piece: every chunk boundary is a host look at the loop state, ~12 us of idle GPU ... but its head goes out in short chunks of
// cert_head fused passes while the last complete pass still scanned: a run starts while a few hundred pairs are still settling and single
// scans trickle on for some passes (1M surface pair, scans per device pass: 159 113 1 8 3 1 0 0 ...), so one short head would see a scan
// and leave the whole run to the fused kernel.  kCertHeads chunks at most; the rest goes out in one piece with the kernel the last
// head's last pass allows.  (A boundary is paid back by two certified-only passes.)
struct ChunkPlan {
    int passes;
    bool certified;                  // the chunk's pass kernel is the certified-only one
};
class ChunkPlanner {
public:
    static constexpr int kCertHeads = 3;
    ChunkPlanner() = default;        // (chunks of 4, 8, 16, ... of the fused kernel, no stage)
    // stage_allowed: a TREE run without SYMMICP_NO_LOOP_STRAGGLERS; list_at_entry: the last host pass left a work list
    ChunkPlanner(bool stage_allowed, bool list_at_entry, int cert_mode, bool one_piece, int cert_head)
        : cert_mode_(cert_mode), cert_head_(cert_head), stage_allowed_(stage_allowed), one_piece_(one_piece)
    {
        set_stage(list_at_entry);
        heads_left_ = (one_piece_ && !stragglers_ && cert_mode_ == 1 && cert_head_ > 0) ? kCertHeads : 0;
    }
    bool stragglers() const { return stragglers_; }      // the next chunk carries the straggler stage
    ChunkPlan next(uint64_t list_len, uint64_t scans, int left, int prev)
    {
        const bool certified = cert_mode_ == 2 || (cert_mode_ == 1 && !stragglers_ && list_len == 0 && scans == 0);
        if (stragglers_) return ChunkPlan{4, certified};
        if (!one_piece_) return ChunkPlan{prev ? 2 * prev : 4, certified};
        if (!certified && heads_left_ > 0 && left > cert_head_) { heads_left_--; return ChunkPlan{cert_head_, certified}; }
        return ChunkPlan{left, certified};
    }
    // the stage stays (or comes) on while any pass of the chunk that has just run left a list
    void after_chunk(bool any_list_in_chunk) { set_stage(any_list_in_chunk); }

private:
    void set_stage(bool on) { stragglers_ = stage_allowed_ && on && cert_mode_ != 2; }
    int cert_mode_ = 0, cert_head_ = 0, heads_left_ = 0;
    bool stage_allowed_ = false, one_piece_ = false, stragglers_ = false;
};

}  // namespace symmicp
