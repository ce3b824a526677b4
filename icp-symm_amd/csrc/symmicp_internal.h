// symmicp_internal.h -- shared between the HIP kernels and the host engine.
// gfx950 (MI355X, CDNA4) only: wave = 64 lanes, 256 CUs in 8 XCDs, 160 KB LDS/CU.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include "symmicp.h"

namespace symmicp {

constexpr int kNSum = SYMMICP_NSUM;   // 40 doubles per reduction record
constexpr int kNAcc = 37;             // live accumulators (rest of the record is 0)
constexpr int kNAccW = 38;            // ... of the weighted passes (robust loss): slot 37 = the unweighted pair count
// (TREE passes: the final reduce leaves the work list's length in slot 39 and the pairs searched and scanned in 38: loop_plan.h)
constexpr int kLeaf = 8;              // target points per leaf (8 x 16 B = one 128-B line)
constexpr int kFan = 8;               // children per tree node
constexpr int kMaxTreeLevels = 12;
constexpr int kMortonBits = 10;       // per axis -> 30-bit keys
constexpr int kPassThreads = 256;
constexpr int kBruteTile = 1024;      // target points staged in LDS per tile (16 KB)
constexpr int kBruteQ = 4;            // queries per thread in the brute-force kernel

// The modes symmicp_config accepts (4, 6 and 8 are unassigned), and those whose record solve::solve_mode solves, on the host and on the device: all but P2P, whose
// solve is host-only, and COLOR and NDT, which stay in the host loop (their records have PLANE's shape: mode_solves_as maps them)
constexpr bool mode_device_solves(int mode)
{
    return mode == SYMMICP_MODE_QUIRKS || mode == SYMMICP_MODE_PAPER || mode == SYMMICP_MODE_PLANE || mode == SYMMICP_MODE_GICP;
}
constexpr bool mode_known(int mode)
{
    return mode_device_solves(mode) || mode == SYMMICP_MODE_P2P || mode == SYMMICP_MODE_COLOR || mode == SYMMICP_MODE_NDT;
}
constexpr int mode_solves_as(int mode) { return (mode == SYMMICP_MODE_COLOR || mode == SYMMICP_MODE_NDT) ? SYMMICP_MODE_PLANE : mode; }

// The record a mode's passes accumulate (PassArgs::obj, the OBJ parameter of every accumulating kernel): the symmetric rows of
// QUIRKS / PAPER / P2P, PLANE's, GICP's or COLOR's (host-loop kernels only: the fused pass and the straggler stage have no COLOR form)
constexpr int kObjSym = 0, kObjPlane = 1, kObjGicp = 2, kObjColor = 3;
constexpr int mode_obj(int mode)
{
    return mode == SYMMICP_MODE_PLANE ? kObjPlane : mode == SYMMICP_MODE_GICP ? kObjGicp : mode == SYMMICP_MODE_COLOR ? kObjColor : kObjSym;
}

// 3x4 affine passed by value in kernel arguments (row-major), plus the weight
// the translation column gets when it is applied to normals
// (1 = reference quirk myicp.cpp:137, 0 = rotate only).
struct Affine {
    float m[12];
    float nrm_w;
};

// planar (structure-of-arrays) cloud: the layout of the reference's column-major
// Eigen::MatrixXf N x 3 blocks (func.cpp:5-15).
struct CloudSoA {
    float *x, *y, *z, *nx, *ny, *nz;
};

// Search index over the target: Morton-sorted points, dense cell table at one
// octree level (the "grid"), and an implicit 8-ary tree of tight boxes over
// runs of the sorted order (the "linear BVH").
struct TargetIndex {
    const float4 *tq;        // sorted: xyz + original row (int bits) in w
    const float4 *tn;        // sorted, 2 per point: (xyz + original row, normal xyz + 0) -- the 32-byte pair record of the accumulating kernels
    uint32_t n;
    // tree: 2 float4 per node (lo, hi); level l starts at node level_off[l]
    const float4 *boxes;
    uint32_t level_off[kMaxTreeLevels];
    int32_t top;             // index of the top level
    uint32_t ntop;           // nodes in the top level (<= kFan)
    // grid
    // two-level cell table: ctop[morton >> 9] = block number (or ~0 when the 8x8x8 super-cell is empty),
    // cells[block * 512 + (morton & 511)] = (first, last+1) of the Morton cell, 0/0 when empty.
    // Memory follows the occupied super-cells (a surface touches few), so the grid can go to level 10.
    const uint32_t *ctop;
    const uint2 *cells;
    int32_t glevel;          // 0 = no grid
    int32_t gdim;            // 1 << glevel
    float ox, oy, oz;        // grid origin (target bbox min)
    float h, inv_h;          // cell edge at glevel
    unsigned long long *dbg; // optional debug counters (SYMMICP_DEBUG_COUNTERS=1), else null
    unsigned long long *dbg_trace;   // with dbg: per packet (start tick, ticks), (pops, hw id) -- 2 x u64 x 2 stages
    // sparse octree over the same sorted points: node = one Morton prefix (an octree cell that holds points),
    // levels 0 (root) .. kMortonBits.  Two float4 per node:
    //   A = (lo.x, lo.y, lo.z, first point as int bits)
    //   B = (hi.x, hi.y, hi.z, packed)   packed = child_first (28 bits, index within the next level) | nchild << 28 ;
    //                                     nchild == 0 marks a leaf, whose low 28 bits hold its point count
    //                                     (oct_nch / oct_cf below; 2^28 nodes per level: targets of ~250M points)
    // Sibling cells are disjoint, so box distances discriminate at every level (unlike runs of the sorted order,
    // whose boxes straddle the big jumps of the Z curve).
    const float4 *onodes;
    uint32_t olevel_off[kMortonBits + 2];
};

constexpr uint32_t kOctCfMask = 0x0FFFFFFFu;
__host__ __device__ inline uint32_t oct_nch(uint32_t packed) { return packed >> 28; }
__host__ __device__ inline uint32_t oct_cf(uint32_t packed) { return packed & kOctCfMask; }

// Append lists for queries a kernel hands to a later kernel of the same pass.  One returning atomic on a single
// word tops out near 88 per microsecond chip-wide, so a list is 64 shards (counter words 64 B apart); a producer
// block appends to shard (blockIdx & 63) and consumer block b drains shard (b & 63): same XCD on both sides.
constexpr int kShards = 64;
constexpr int kShardStride = 16;          // uint32 words between shard counters
struct ShardList {
    uint32_t *items;                      // [kShards][cap]
    uint32_t *counts;                     // [kShards * kShardStride]
    uint32_t cap;
};
struct WorkLists {
    ShardList work;                       // queries k_search_cells hands to k_search_walk
    ShardList retry;                      // queries the budgeted thread-per-query walk gave up on
};                                        // the two counter blocks are contiguous and cleared by the final reduce

// Device-resident state of a device-driven run of passes (symmicp_align's batches): written by k_reduce_solve, read by the
// pass kernels.  Lives in device memory; `ring` entries live in host-mapped memory and are read by the host afterwards.
struct LoopState {
    float X[16];             // cumulative transform (myicp.cpp:138)
    Affine Xapply;           // what the next pass applies to its input (cumulative apply: X; incremental: the last increment)
    int32_t stop;            // != 0: every kernel of the batch returns at once
    int32_t reason;          // LOOP_* below
    int32_t iters;           // passes of this alignment completed so far (the reference's `iters`)
    int32_t small_step;      // the last increment was below eps_rotation / eps_translation: stop after the pass that applies it
};
enum { LOOP_RUNNING = 0, LOOP_DONE = 1, LOOP_REDO_PASS = 2, LOOP_HOST_SOLVE = 3, LOOP_SLOW = 4 };
struct LoopConfig {
    int32_t mode, fixed_iters, max_iters, incremental, tree;
    float diff_threshold, eps_rotation, eps_translation, nrm_w;
    float pivot[3];
    uint32_t uncertified_limit;   // TREE: more pairs than this searched in a pass -> back to the separate kernels (LOOP_SLOW)
    int32_t walk_in_loop;         // TREE: the batch runs k_search_walk + k_accumulate_list behind every fused pass: a non-empty work list is
                                  // handled there (it stops the loop otherwise: LOOP_REDO_PASS)
    uint32_t list_limit;          // ... unless it is longer than this (LOOP_SLOW: the host sizes the walk for long lists)
};
struct LoopRecord {          // one per pass, host-mapped
    double sums[SYMMICP_NSUM];       // the pass's record (after the exchange over ranks)
    float increment[16], X[16];      // the increment solved FROM this record and the cumulative transform after it
    float rcond;
    int32_t status;                  // status of that solve
    int32_t solved;                  // 1: increment / X are valid (the loop went on)
    int32_t searched;                // pairs searched in this pass
    int32_t list_len, scans;         // work-list length of this pass (queries handed to the tree walk); searched pairs that reached a scan
};
static_assert(sizeof(LoopRecord) == 472 && offsetof(LoopRecord, searched) == 460 && offsetof(LoopRecord, list_len) == 464 && offsetof(LoopRecord, scans) == 468,
              "LoopRecord keeps its layout");

// ---- pair rejection (kernels_select.hip): trim fraction, one-to-one, median distance, reciprocal ----
// what a reciprocal pass adds to the claim (k_recip_check): the index over the ORIGINAL source, whose tq carries the caller's row in w,
// and the 3x4 inverse of the pass's cumulative transform (symmicp_inverse_rigid).  Read by the kernel from device memory (the tail of
// the claim table), so PassArgs, an argument of every pass kernel, carries a pointer for it and nothing more
struct RecipArgs {
    TargetIndex six;
    Affine inv;
};
constexpr size_t kRecipTailWords = (sizeof(RecipArgs) + 7) / 8;      // 64-bit words the claim table is allocated beyond its entries
constexpr uint32_t kRejectWsWords = 16 + 3 * 2048;                   // the select's state and its three histograms
constexpr uint32_t kRejectTauWord = 3;                               // ... where the accumulating kernels find the pass's tau
// What a rejecting pass leaves for the host, behind the record's sequence word in host-mapped memory
struct RejectRecord {
    uint32_t population;                // the select's population: the candidates (n_c), with a claim its winners (n_u)
    uint32_t kept, tau_bits;            // keys <= tau; tau as fp32 bits
    uint32_t gated;                     // n_c: pairs that exist and pass the gates
    uint32_t claimed, reciprocal;       // reciprocal passes: targets claimed (n_u), claims the reverse search confirmed (n_r); 0 otherwise
};
enum RejectClaim : int32_t { kClaimNone = 0, kClaimOneToOne = 1, kClaimReciprocal = 2 };
// The rejectors of one pass.  keys != null makes it a rejecting pass (pass_rejects): the launchers run the claim, the keys and the select
// (launch_reject) in front of the T instantiation of the pass's accumulating kernel, which keeps a pair only if its d2 bits are <= the
// tau in ws[kRejectTauWord].  All of them run through the same keys, the same select and the same T instantiations.
struct RejectArgs {
    uint32_t *keys;                     // [n] per share row: the candidate's d2 bits, 0xFFFFFFFF otherwise
    uint32_t *ws;                       // [kRejectWsWords]
    RejectRecord *host;                 // host-mapped: the pass's result
    unsigned long long *table;          // claim: [n_t] per target position the smallest claim (d2 bits << 32 | caller row)
    const uint32_t *order;              // ... share row -> caller row (null: the share is in caller order)
    const RecipArgs *recip;             // kClaimReciprocal: in device memory, filled in by the host before the pass
    uint32_t n_t;                       // claim: entries of the table
    int32_t claim;                      // RejectClaim.  != none: the accumulating kernel reads keys[i] and drops the sentinel rows, the claim's losers
    float rho;                          // trim fraction (1: off)
    float med_f2;                       // median distance: factor * factor in fp32 (0: off): tau = med_f2 * the select's median
};
static_assert(sizeof(RejectArgs) == 64 && sizeof(RejectRecord) == 24, "RejectArgs takes the room of the nine fields it replaced");

struct PassArgs {
    // source share (planar).  `in` is read; if writeback, `out` receives the transformed points/normals
    CloudSoA in, out;
    uint32_t n;              // points in this share
    uint32_t tgt_offset;     // identity pairing: target row = tgt_offset + i
    Affine X;                // transform applied to `in` on the fly
    float pivot[3];          // subtracted from p and q before forming rows (0 in QUIRKS)
    float max_d2;            // <= 0: keep all pairs
    float min_ndot;          // <= -1: keep all pairs; else drop pairs with n_p . n_q below it
    int32_t p2p;             // point-to-point mode: slots 0..8 accumulate p q^T instead of the 6x6 Gram / rhs
    int32_t writeback;
    // correspondences
    const unsigned long long *best64;   // BRUTE: (d2 bits << 32 | target row), ~0 = none
    int32_t *pos_prev;                  // TREE: sorted position found by the previous pass (-1 = none); updated
    float *d2_out;                      // optional per-point squared distance (may be null)
    int32_t *pos_out;                   // sorted position / target row chosen this pass (may alias pos_prev)
    double *partials;                   // [blocks][kNSum]: block b's record at partials[b * kNSum + k]
    // pair certificates (TREE): position of the query when its pair was last searched, and the radius around it known
    // to hold no other target point (see k_search_cells)
    float4 *pairrec;                    // TREE: per pair, its own copy of the target's (point, normal) record (2 float4)
    int32_t budget_walk;                // this pass's thread-per-query walk runs with a visit budget + retry launch (see k_search_walk)
    int32_t refresh_records;            // k_accumulate may replace stale copies (0 in a pass that may still be repaired)
    float4 *cert;                       // per pair: (ref.xyz, clear radius L around ref; L <= 0: no single certificate); bit 0 of L's word: certk[i] is valid
    uint4 *certk;                       // per pair, 2 x uint4: the neighbourhood certificate's members (8 sorted positions; see hood_test in pair_search.h)
    float2 *hoodr;                      // ... its radius T and the radius hint for the pair's next scan
    int32_t make_hood;                  // k_search_cells keeps neighbourhoods in this pass (existing ones are honoured either way)
    int32_t use_slack;                  // 0 on the first pass of an alignment (certificates not valid yet)
    const LoopState *loop;              // device-driven loop: the transform comes from here (null: from X above)
    uint32_t partial_cols, partial_col0;   // partial records: columns in all (0: the grid's size) and this launch's first column
    const uint2 *pkt_tab;               // first pass (packets): (first query, count <= 64) per packet in start order (null: 64 as they lie)
    uint32_t pkt_count;
    uint32_t pkt_waves;                 // first pass: waves that share one packet (1, 2 or 4; 0: the launcher decides from the packet count)
    uint32_t pkt_front_cap;             // ... frontier capacity per level (0: kFrontCap; smaller values force the depth-first fallback: tests)
    uint32_t *pkt_fallbacks;            // ... counts the packets that finished depth-first (may be null)
    uint32_t pkt_chunk, pkt_lds_pad;    // ... packets per XCD chunk (0: 64); extra dynamic LDS per workgroup (occupancy experiments)
    int32_t loss;                       // robust loss (SYMMICP_LOSS_*): != NONE selects the weighted instantiation of every accumulating kernel
    float loss_scale;                   // ... its scale (robust_loss.h)
    int32_t obj;                        // the record (kObjSym / kObjPlane / kObjGicp, mode_obj): the launchers pick the instantiations; read by the host only
    float gicp_k;                       // ... 1 - eps of its covariances (symmicp_set_gicp_epsilon), fp32: read by the GICP instantiations only
    RejectArgs rej;                     // the pass's rejectors (above); zeroed: none, and the kernels are the plain ones
    // colored ICP (SYMMICP_MODE_COLOR; read by the kObjColor instantiations only)
    const float4 *tgt_color;            // per target point, in the order of tn (IDENTITY: of the planar target): (gradient xyz, intensity)
    const float *src_int;               // per share row: the source point's intensity
    float color_lam, color_om;          // lambda and omega = 1.0f - lambda
};
// (the layout the kernels without a rejector were compiled against before RejectArgs: they read the same offsets, so their code is the same)
static_assert(sizeof(PassArgs) == 432 && offsetof(PassArgs, rej) == 344 && offsetof(PassArgs, tgt_color) == 408 && offsetof(PassArgs, src_int) == 416,
              "PassArgs keeps its layout");
__host__ __device__ inline bool pass_rejects(const PassArgs &a) { return a.rej.keys != nullptr; }

// host-side launch tuning of the tree passes (environment switches, read once by the engine)
struct PassTuning {
    uint32_t wave_mode_max = 20000u;    // work lists longer than this use one thread per query (the 48k-entry list after the first move of the 1M surface pair: 115 -> 85 us)
    uint32_t cells_chunk = 16u;         // tiles per XCD chunk of k_search_cells
    uint32_t cells_queries = 0u;        // queries per tile of k_search_cells (64, 128, 256; 0: from the share's size)
    uint32_t walk_budget = 160u;        // node visits of the budgeted walk (sharded first passes on volume-like targets)
};

// ---- batched alignment (kernels_batch.hip, engine_batch.cpp): one workgroup per problem, the whole loop inside it ----
constexpr int kBatchThreads = 512;        // workgroup size of k_batch_align
constexpr int kBatchQ = 4;                // queries per thread in registers
constexpr int kBatchChunk = kBatchThreads * kBatchQ;      // queries per sweep of the target (2048)
constexpr int kBatchTile = SYMMICP_BATCH_MAX_POINTS;      // target points staged in LDS, once per problem: the whole cloud (3 x 16 KB planar)
constexpr int kBatchMerge = 1024;         // largest source that is searched with the target split over the workgroup's waves
// How many ways the target is split for a source of n rows: the largest power of two S with (kBatchThreads / S) * kBatchQ >= n and whole
// waves per split, so that a source of <= 1024 rows still occupies every wave (8 for <= 256 rows, 4 for <= 512, 2 for <= 1024, else 1)
__host__ __device__ constexpr uint32_t batch_splits(uint32_t n) { return n <= 256u ? 8u : n <= 512u ? 4u : n <= 1024u ? 2u : 1u; }
static_assert(kBatchThreads / 8 >= 64 && (kBatchThreads / 2) * kBatchQ == kBatchMerge, "a split is at least one wave; two splits cover kBatchMerge rows");
struct BatchProblem {                     // one per workgroup, in start order (descending src_count x tgt_count)
    uint32_t src_first, src_count, tgt_first, tgt_count;
    float pivot[3];
    uint32_t slot;                        // the problem's index in the caller's arrays (guess, out, traces)
};
struct BatchArgs {
    const float *src_xyz, *src_nrm, *tgt_xyz, *tgt_nrm;      // packed [n][3] pools; src_nrm may be null (zeros)
    const BatchProblem *problems;
    const float *guess;                   // [B][16] by slot, or null (identity)
    symmicp_batch_result *out;            // [B] by slot, zeroed by the host
    float *trace_X;                       // [B][max_iters + 1][16] by slot, zeroed, or null
    double *trace_sums;                   // [B][max_iters + 1][40], or null
    int32_t mode, max_iters, fixed_iters;
    float diff_threshold, max_d2, min_ndot, eps_rotation, eps_translation;
};
void launch_batch_align(const BatchArgs &a, uint32_t n_problems, hipStream_t s);

// ---- kernel launchers (kernels_pass.hip, kernels_search.hip, kernels_reduce.hip) ---------------------------------------
void launch_pass_identity(const PassArgs &a, CloudSoA tgt, int blocks, bool vec4_ok, hipStream_t s);
void launch_pass_indexed(const PassArgs &a, const float4 *tn /* pair records */, int blocks, hipStream_t s);
// ev: null, or 5 events recorded before cells / after cells / (same again) / after walk / after accumulate
// walk_blocks: grid of k_search_walk (any size is correct; 0 = one thread per possible list entry)
// stage: 0 = cells, walk, accumulate; 1 = cells, accumulate (walk skipped); 2 = walk, accumulate (repair of a stage-1 pass)
// compact_blocks > 0: the cell search runs as the streaming, compacting kernel (k_pass_fused<false>) on that many blocks
void launch_pass_tree_split(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int acc_blocks, uint32_t walk_blocks,
                            int stage, int compact_blocks, const PassTuning &tune, hipStream_t s, hipEvent_t *ev);
void launch_pass_tree_first(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int acc_blocks, hipStream_t s, hipEvent_t *ev);
// the search kernels behind launch_pass_tree_split and launch_loop_stragglers (kernels_search.hip): k_search_cells; k_search_walk on the work
// list (and the retry list); the walk of the straggler stage
void launch_search_cells(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const PassTuning &tune, hipStream_t s);
void launch_search_walk(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, uint32_t walk_blocks, const PassTuning &tune, hipStream_t s);
void launch_straggler_walk(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const PassTuning &tune, hipStream_t s);
uint32_t walk_blocks_full(const WorkLists &wl);
uint32_t shard_capacity(uint32_t n_points);
// keep_nonempty: leave the append-list counters alone when the work list is not empty (stage-1 passes)
void launch_final_reduce(const double *partials, int blocks, double *out_dev, double *out_host_mapped, uint32_t *ticket,
                         unsigned long long seq, uint32_t *counters_to_clear, int keep_nonempty, hipStream_t s);
// fused pass of a converged alignment (k_pass_fused) (kernels_pass.hip) and the device-side end of a pass (k_reduce_solve, kernels_reduce.hip)
void launch_pass_fused(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int blocks, hipStream_t s);
// ... the same pass for a chunk in which no pair needs a scan (k_pass_certified): an unsettled pair makes the pass incomplete (LOOP_REDO_PASS)
void launch_pass_certified(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int blocks, hipStream_t s);
// device-driven loop, straggler stage behind a fused pass: the work list through the tree walk, then its pairs into `list_blocks` more partial columns
void launch_loop_stragglers(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int list_blocks, const PassTuning &tune, hipStream_t s);
// mode 0: reduce + check + solve (single GPU); 1: the record is already in out_dev (after the all-reduce); 2: solve only (start of a batch)
void launch_reduce_solve(const double *partials, int blocks, double *out_dev, int mode, LoopState *loop, LoopConfig cfg, LoopRecord *ring, int ring_len,
                         uint32_t *counters_to_clear, hipStream_t s);
// test entry: solve_core.h on the device for n records, one thread each (symmicp_ctx_solve_probe); X_in may be null
void launch_solve_probe(int mode, int exact_rc, const symmicp_sums *sums, int n, const float *pivot, const float *X_in, int32_t *status, float *pbar,
                        float *qbar, float *a, float *t, float *rcond, float *out16, float *X_out, hipStream_t s);
void launch_loop_end(const LoopState *loop, LoopState *host_copy, unsigned long long *done_flag, unsigned long long seq, hipStream_t s);
void launch_publish(const double *sums_dev, double *out_host_mapped, unsigned long long seq, hipStream_t s);
void launch_nn_brute(const CloudSoA &src, uint32_t n_s, const Affine &X, const float4 *tq, uint32_t n_t,
                     unsigned long long *best64, hipStream_t s);

// index build
void launch_bbox(const float *x, const float *y, const float *z, uint32_t n, uint32_t *bbox_ord6, hipStream_t s);
void launch_morton(const float *x, const float *y, const float *z, uint32_t n, float ox, float oy, float oz,
                   float inv_h0, uint32_t *keys, uint32_t *vals, hipStream_t s);
// sorts (keys, vals) ascending, stable; tmp arrays same size; result lands back in keys/vals
void radix_sort_pairs(uint32_t *keys, uint32_t *vals, uint32_t *keys_tmp, uint32_t *vals_tmp, uint32_t n,
                      int key_bits, uint32_t *hist_ws, size_t hist_ws_elems, hipStream_t s);
size_t radix_sort_ws_elems(uint32_t n);
void launch_gather_f4(const float *x, const float *y, const float *z, const float *nx, const float *ny, const float *nz,
                      const uint32_t *order, uint32_t n, float4 *tq, float4 *tn, hipStream_t s);
void launch_gather_soa(const CloudSoA &src, const uint32_t *order, uint32_t n, CloudSoA dst, hipStream_t s);
void launch_offset_u32(const uint32_t *in, uint32_t off, uint32_t n, uint32_t *out, hipStream_t s);
// first pass: the packets (runs of <= 64 queries, blocks cut at jumps of the Morton curve; jump_factor < 0: the default) with radius keys, and the table in start order
void launch_packet_runs(const CloudSoA &src, uint32_t n, float jump_factor, uint2 *runs, uint32_t *keys, uint32_t *vals, uint32_t *count, int key_bits, hipStream_t s);
// start keys from the packets' distance to the target (identity transform): replaces the radius keys of launch_packet_runs when the target index exists
void launch_packet_cost(const CloudSoA &src, const uint2 *runs, uint32_t npk, const TargetIndex &ix, uint32_t *keys, int key_bits, hipStream_t s);
void launch_packet_table(const uint32_t *order, const uint2 *runs, uint32_t npk, uint2 *tab, hipStream_t s);
void launch_deinterleave3(const float *raw, size_t row_stride, size_t offset, uint32_t n, float *x, float *y, float *z, hipStream_t s);
void launch_level_hist(const uint32_t *keys, uint32_t n, uint32_t *hist16, hipStream_t s);
void launch_cell_table(const uint32_t *keys, uint32_t n, int glevel, const uint32_t *nid_top, uint32_t *ctop, uint2 *cells, hipStream_t s);
// sparse octree build (levels bottom-up); see TargetIndex::onodes
void launch_oct_flags(const uint32_t *keys, uint32_t n, int level, uint32_t *nid, hipStream_t s);
void launch_exclusive_scan(uint32_t *data, uint32_t n, uint32_t *tile_ws /* >= ceil(n/2048) words */, hipStream_t s);
void launch_oct_first(const uint32_t *keys, uint32_t n, int level, const uint32_t *nid, uint32_t *first, hipStream_t s);
void launch_oct_nodes(int level, const float4 *tq, uint32_t n, const uint32_t *first, uint32_t n_nodes, const uint32_t *nid_next,
                      uint32_t n_nodes_next, const float4 *nodes_next, float4 *nodes, uint32_t leaf_max, hipStream_t s);
void launch_leaf_boxes(const float4 *tq, uint32_t n, float4 *boxes, uint32_t nleaf_padded, hipStream_t s);
void launch_node_boxes(const float4 *child, uint32_t nchild_padded, float4 *parent, uint32_t nparent_padded, hipStream_t s);
void launch_iota_f4(const float *x, const float *y, const float *z, const float *nx, const float *ny, const float *nz,
                    uint32_t n, float4 *tq, float4 *tn, hipStream_t s);
void launch_unpermute(const CloudSoA &cur, const uint32_t *order, uint32_t n, float *xyz_aos, float *nrm_aos, hipStream_t s);
void launch_corr_out(const int32_t *pos, const unsigned long long *best64, const float *d2, const float4 *tq,
                     const uint32_t *src_order, uint32_t n, int mode, uint32_t tgt_offset, int32_t *idx_out, float *d2_out,
                     const uint32_t *rej_keys /* null, or: rows whose key is above rej_tau report -1 */, uint32_t rej_tau, hipStream_t s);

// the rejection steps of a pass (kernels_select.hip has the order); called by the pass launchers when pass_rejects(a).  corr: symmicp_corr
// (which of tgt / tn is read)
void launch_reject(const PassArgs &a, int corr, CloudSoA tgt, const float4 *tn, hipStream_t s);
// test entry: the select alone on n keys, rank k (1-based); afterwards ws[kRejectTauWord] = the k-th smallest key, ws[4] = keys <= it
void launch_select_probe(const uint32_t *keys, uint32_t n, uint32_t k, uint32_t *ws, hipStream_t s);
// test entry: the one-to-one claim alone (k_unique_claim's claim_wave and the winner test) on n rows given as (target row, d2 bits), the row
// being the array index; tgt_row < 0 or >= n_t: no pair.  table: [n_t] scratch; winner_out[i] = 1 where row i wins its target
void launch_unique_probe(const int32_t *tgt_row, const uint32_t *d2_bits, uint32_t n, unsigned long long *table, uint32_t n_t,
                         uint8_t *winner_out, hipStream_t s);

// reciprocal correspondences: tq[i].w = labels[tq[i].w] over an index's sorted points (labels == null: nothing is launched); and the
// test entry of the reverse search: queries [n_q][3] through inv and the walk -> back() and d2' per query
void launch_relabel_tq(float4 *tq, uint32_t n, const uint32_t *labels, hipStream_t s);
void launch_reverse_nn_probe(const TargetIndex &six, const Affine &inv, const float *q_xyz, uint32_t n_q, int32_t *label_out, float *d2_out, hipStream_t s);

void launch_identity_d2(const CloudSoA &in, const Affine &X, const CloudSoA &tgt, uint32_t tgt_offset, uint32_t n, float *d2, hipStream_t s);
void launch_pairs_d2(const CloudSoA &in, const Affine &X, const int32_t *pos, const float4 *tq, uint32_t n_t, uint32_t n, float *d2, hipStream_t s);
void launch_normals_knn(const TargetIndex &ix, int k, const float vp[3], float *nrm_out, float *curv_out, hipStream_t s);
void launch_knn(const TargetIndex &ix, int k, int32_t *rows_out, float *d2_out, hipStream_t s);

// colored ICP (kernels_color.hip).  The attributes into engine order: dst[i] = (grad[row(i)], intensity[row(i)]) with row(i) the w word of
// tq[i] (tq == null: i), and dst[i] = intensity[order ? order[i] : off + i]; the read-back scatters the other way (out[order ? order[i] : i], as launch_unpermute).  The gradient
// (symmicp_ctx_intensity_gradient): rec_rows [n] = (xyz, intensity) by original row, scattered from the index; then one thread per sorted
// point over the neighbour rows launch_knn left in knn_rows [n][k]
void launch_color_permute_target(const float *intensity, const float *grad3, const float4 *tq, uint32_t n, float4 *dst, hipStream_t s);
void launch_color_permute_source(const float *intensity, const uint32_t *order, uint32_t off, uint32_t n, float *dst, hipStream_t s);
void launch_color_unpermute_source(const float *src_int, const uint32_t *order, uint32_t n, float *out_rows, hipStream_t s);
void launch_color_gradient(const TargetIndex &ix, const float *intensity_rows, const int32_t *knn_rows, int k, float4 *rec_rows, float *grad_rows,
                           hipStream_t s);

// voxel-grid downsampling (kernels_voxel.hip; symmicp_ctx_voxel_downsample): keys + iota rows; run heads -> exclusive scan -> first
// position of every voxel (first[m0] = n) and the voxel count m0 in *m0_out; kept voxels (>= min_points) -> exclusive scan ->
// their (first, count) and number m in *m_out; the per-voxel means; the output id of every row (-1: dropped voxel)
void launch_voxel_keys(const CloudSoA &cl, uint32_t n, float inv, const int lo[3], uint64_t nx, uint64_t ny, uint32_t *keys, uint32_t *vals,
                       hipStream_t s);
void launch_voxel_segments(const uint32_t *keys, uint32_t n, uint32_t *vid_excl, uint32_t *first, uint32_t *scan_ws, uint32_t *m0_out,
                           hipStream_t s);
void launch_voxel_keep(const uint32_t *first, uint32_t m0, uint32_t min_points, uint32_t *kid_excl, uint32_t *scan_ws, uint32_t *kfirst,
                       uint32_t *kcount, uint32_t *m_out, hipStream_t s);
void launch_voxel_mean(const CloudSoA &sorted, const uint32_t *kfirst, const uint32_t *kcount, uint32_t m, int with_normals, float *xyz_out,
                       float *nrm_out, int32_t *count_out, hipStream_t s);
void launch_voxel_of(const uint32_t *keys, const uint32_t *rows, const uint32_t *vid_excl, const uint32_t *first, const uint32_t *kid_excl,
                     uint32_t n, uint32_t min_points, int32_t *voxel_of, hipStream_t s);

// NDT (kernels_ndt.hip; SYMMICP_MODE_NDT, symmicp_ctx_ndt_map).  The map of a cloud: per kept voxel (ascending key) a record of 4
// float4 -- (mean xyz, count as int bits), then (axis l_r xyz, o_r) for r = 0, 1, 2 -- its key, and the 6 doubles of its covariance; and
// an open-addressing table over the keys: a power of two >= 2 m entries of (key << 32 | row + 1), 0 = empty, probed linearly from
// (key * 0x9E3779B1) >> shift.  A lookup is exact (a row is found iff the voxel exists) and costs one 8-byte load per probe.
struct NdtGrid {
    float inv;                          // 1.0f / resolution
    float lo[3], hi[3];                 // the box's cells as floats (|.| < 2^23: exact)
    int32_t lo_i[3];
    uint32_t nx, ny;                    // key = ix + nx * (iy + ny * iz)
    const float4 *rec;                  // [m][4]
    const unsigned long long *table;
    uint32_t shift, mask;               // 32 - log2(capacity), capacity - 1
};
struct NdtPassArgs {
    const float *x, *y, *z;             // the source share as set (planar): read through X every pass
    uint32_t n;
    Affine X;
    float pivot[3];
    float max_d2;                       // <= 0: keep every item
    float h;                            // (float)(0.5 * d2) of the Gauss constants
    int32_t neighbors;                  // 1 or 7
    NdtGrid g;
    double *partials;                   // [blocks][kNSum], as every accumulating kernel writes them
};
// sorted: the cloud gathered in (key, row) order; skeys: the sorted keys; (kfirst, kcount): the voxels with >= min_points points.  One
// thread per such voxel: rec / cov / key at its index, valid[o] = 1 unless the voxel is dropped (lambda_max not finite or <= 0)
void launch_ndt_voxels(const CloudSoA &sorted, const uint32_t *skeys, const uint32_t *kfirst, const uint32_t *kcount, uint32_t m, float eig_ratio,
                       float4 *rec, double *cov, uint32_t *key, uint32_t *valid, hipStream_t s);
// the valid voxels, dense in the same order: pos = the exclusive scan of valid
void launch_ndt_compact(const float4 *rec, const double *cov, const uint32_t *key, const uint32_t *valid, const uint32_t *pos, uint32_t m,
                        float4 *rec_out, double *cov_out, uint32_t *key_out, hipStream_t s);
// table: capacity entries, zeroed by the caller
void launch_ndt_insert(const uint32_t *key, uint32_t m, unsigned long long *table, uint32_t shift, uint32_t mask, hipStream_t s);
void launch_pass_ndt(const NdtPassArgs &a, int blocks, hipStream_t s);
// per share row i, at [order ? order[i] : i]: the map row of the moved point's own cell (-1: none) and the pass's d2 to its mean (0: none)
void launch_ndt_corr(const NdtPassArgs &a, const uint32_t *order, int32_t *idx_out, float *d2_out, hipStream_t s);

// radius search and FPFH (kernels_fpfh.hip; symmicp_ctx_radius_search, symmicp_ctx_fpfh): one thread per sorted point, the box-tree
// walk with the fixed bound r2.  count / offs / spfh_rows / fpfh_rows are indexed by ORIGINAL row, spfh_sorted ([n][36] floats)
// by sorted position; the fill pass writes list `row` from offs[row] on, in ascending sorted position.
void launch_radius_count(const TargetIndex &ix, float r2, int32_t *count_rows, hipStream_t s);
void launch_radius_fill(const TargetIndex &ix, float r2, const uint32_t *offs_rows, int32_t *rows_out, float *d2_out, hipStream_t s);
void launch_spfh(const TargetIndex &ix, float r2, float *spfh_sorted, float *spfh_rows /* may be null */, int32_t *count_rows, hipStream_t s);
void launch_fpfh(const TargetIndex &ix, float r2, const float *spfh_sorted, float *fpfh_rows, hipStream_t s);

// ISS keypoints (kernels_keypoints.hip; symmicp_ctx_iss_keypoints): the same walk at the salient radius (s_sorted by sorted position,
// s_rows / k_rows by ORIGINAL row) and at the non-maximum radius (flag_rows by original row: 1 = keypoint); after an exclusive scan of
// the flags into pos_rows the scatter writes the kept rows in ascending order
void launch_iss_saliency(const TargetIndex &ix, float r2, int32_t min_neighbors, float gamma21, float gamma32, float *s_sorted, float *s_rows,
                         int32_t *k_rows, hipStream_t s);
void launch_iss_nms(const TargetIndex &ix, float r2, int32_t min_neighbors, const float *s_sorted, uint32_t *flag_rows, hipStream_t s);
void launch_iss_scatter(const uint32_t *flag_rows, const uint32_t *pos_rows, uint32_t n, int32_t *rows_out, hipStream_t s);

// statistical outlier removal (kernels_outlier.hip; symmicp_ctx_statistical_outlier_removal): one thread per sorted point, the box-tree
// walk pruned by the k-th smallest distance so far (1 <= k <= 64, k <= n - 1; the candidate list lives in LDS sized from k);
// mean_rows [n] by ORIGINAL row = the fp64 mean of sqrt(d2) over the k nearest other points
void launch_knn_mean_dist(const TargetIndex &ix, int k, double *mean_rows, hipStream_t s);

// DBSCAN / Euclidean clustering (kernels_cluster.hip; symmicp_ctx_cluster): count_rows = launch_radius_count's at the same r2.  Leaves in
// parent_rows [n], by ORIGINAL row, the representative (lowest core row) of the row's cluster, or kClusterNoise.  stats (may be null):
// two zeroed words, += unite calls and lost compare-and-swaps of the union kernel.
constexpr uint32_t kClusterNoise = 0xffffffffu;
void launch_cluster_roots(const TargetIndex &ix, float r2, const int32_t *count_rows, int32_t min_points, uint32_t *parent_rows,
                          unsigned long long *stats, hipStream_t s);
// its first and third step on their own (the region growing runs them around its own union): parent_rows[row] = row; then, once every
// union is done, parent_rows[row] = the root of row for the rows with count_rows[row] >= need
void launch_cluster_init(uint32_t *parent_rows, uint32_t n, hipStream_t s);
void launch_cluster_flatten(const int32_t *count_rows, int32_t need, uint32_t *parent_rows, uint32_t n, hipStream_t s);

// region growing (kernels_region.hip; symmicp_ctx_region_growing).  ix carries the normals (ix.tn).  seed_rows [n] int32 0 / 1 and
// parent_rows [n] by ORIGINAL row; curv_rows [n] by ORIGINAL row or null (every row a seed).  launch_region_roots leaves in parent_rows
// the representative (lowest seed row) of the row's region, or kClusterNoise.  stats (may be null): four zeroed words, += unite calls,
// lost compare-and-swaps, edges examined by the union kernel (in range, at a higher sorted position) and normal loads among them.
void launch_region_seeds(const float *curv_rows, float threshold, uint32_t n, int32_t *seed_rows, hipStream_t s);
// border: run the pass over the non-seed rows (false when every row is a seed)
void launch_region_roots(const TargetIndex &ix, float r2, float smoothness_cos, const int32_t *seed_rows, bool border, uint32_t *parent_rows,
                         unsigned long long *stats, hipStream_t s);
// smooth_rows [n] by ORIGINAL row = |{ j : smooth(row, j) }|
void launch_region_smooth_count(const TargetIndex &ix, float r2, float smoothness_cos, int32_t *smooth_rows, hipStream_t s);

// normal orientation (kernels_orient.hip; symmicp_ctx_orient_normals; the state words, keys and the hook rule are orient_core.h's).
// Everything is indexed by ORIGINAL row; xyz3 / nrm3 / nrm_out are packed [n][3].
//   edges    knn_rows [n][k] = launch_knn's -> erow / eww [k][n] (lists and weight words, transposed), *edge_count (zeroed) += |E|,
//            words [n] = every row a root
//   round    best [n] / best_hi [n]: the candidate slots, reset here; words (flat) -> words_mid with this round's hooks; tree [n][2] and
//            *counter (zeroed before the first round) take the hooked edges
//   flatten  words_mid -> words, flat again; bound = the round's hooks + 1; *err (zeroed) |= 1 when a walk was longer
//   finish   rule 0 = viewpoint at ref, 1 = direction ref; min_row [n], seed_key [n], root_flip [n] are scratch
void launch_orient_edges(const int32_t *knn_rows, const float *nrm3, uint32_t n, int k, uint32_t *erow, uint32_t *eww, unsigned long long *edge_count,
                         uint32_t *words, hipStream_t s);
void launch_orient_round(const uint32_t *erow, const uint32_t *eww, const uint32_t *words, uint32_t *words_mid, uint32_t n, int k,
                         unsigned long long *best, uint32_t *best_hi, const float *nrm3, int32_t *tree, uint32_t *counter, hipStream_t s);
void launch_orient_flatten(const uint32_t *words_mid, uint32_t *words, uint32_t n, uint32_t bound, uint32_t *err, hipStream_t s);
void launch_orient_finish(const uint32_t *words, const float *xyz3, const float *nrm3, uint32_t n, int rule, const float ref[3], uint32_t *min_row,
                          unsigned long long *seed_key, uint32_t *root_flip, float *nrm_out, uint8_t *flip_out, int32_t *component_out, hipStream_t s);

// feature matching and RANSAC (kernels_global.hip; symmicp_ctx_feature_nn, symmicp_ctx_ransac).  feature_nn: fa / fb packed [n][33];
// splits > 1 needs feature_nn_partial_bytes of `partial`.  ransac: pq8 [m][8] = p.xyz, 0, q.xyz, 0 about the pivots; hyp [H][12].
void launch_feature_nn(const float *fa, uint32_t na, const float *fb, uint32_t nb, int queries_per_thread, uint32_t splits, void *partial,
                       int32_t *nn_out, float *d2_out, float *second_out, hipStream_t s);
size_t feature_nn_partial_bytes(uint32_t na, uint32_t splits);
void launch_ransac_hyp(const float *pq8, uint32_t m, uint32_t H, unsigned long long base, float max_dist2, float edge2, float *hyp,
                       uint8_t *status, int32_t *inliers, uint32_t *surv, uint32_t *n_surv, hipStream_t s);
void launch_ransac_eval(const float *pq8, uint32_t m, const float *hyp, const uint32_t *surv, const uint32_t *n_surv, uint32_t n_surv_host,
                        float max_dist2, int32_t *inliers, hipStream_t s);
void launch_ransac_argmax(const uint8_t *status, const int32_t *inliers, uint32_t H, unsigned long long *best, hipStream_t s);

// RANSAC plane segmentation (kernels_plane.hip; symmicp_ctx_segment_plane).  pts4 [n][4] = p.xyz, 0 about the pivot; hyp4 [H][4] = n, d;
// axis: null, or the unit axis of the constraint.  score: inliers[h] += the points within max_dist of survivor h; the survivor count stays
// on the device (the grid is sized for H).  shape: 0 the kernel in use (hypotheses in lanes, the chunk staged in LDS); the others are
// the A/B shapes of kernels_plane.hip (SYMMICP_PLANE_SCORE; profiles/plane_workload.py).  mask [n]: the inlier flags of the winner named by the arg-max key
// `best` (launch_ransac_argmax), nd_out [4] its (n, d); zeros when the key is 0.
constexpr int kPlaneChunk = 512;          // points a workgroup of the scoring kernel stages at a time (tests/_segplane_ref.py: K_CHUNK)
constexpr int kPlaneLaneHyps = 2;         // evaluated hypotheses per lane: 256 * kPlaneLaneHyps per workgroup (K_BATCH)
constexpr int kPlaneBlocks = 2048;        // workgroups of a scoring launch, about: 8 resident on each of 256 CUs
void launch_plane_hyp(const float *pts4, uint32_t n, uint32_t H, unsigned long long base, const float *axis, float cos_min, float *hyp4,
                      uint8_t *status, int32_t *inliers, uint32_t *surv, uint32_t *n_surv, hipStream_t s);
void launch_plane_score(const float *pts4, uint32_t n, const float *hyp4, const uint32_t *surv, const uint32_t *n_surv, uint32_t H, float max_dist,
                        int32_t *inliers, int shape, hipStream_t s);
void launch_plane_mask(const float *pts4, uint32_t n, const float *hyp4, const unsigned long long *best, float max_dist, uint8_t *mask,
                       float *nd_out, hipStream_t s);

// Fast Global Registration (kernels_fgr.hip; symmicp_ctx_fgr).  pq8 as RANSAC's.  Tuple test: flags [trials + 1] (the last word 0) = 1 for
// an accepted trial; after an exclusive scan of them (rank [trials + 1], rank[trials] = the accepted count) the scatter writes the
// draws of the trials of rank < max_tuples to set [3 * max_tuples].  The loop: one workgroup, every pass of it in one launch.
constexpr int kFgrThreads = 512;          // workgroup size of k_fgr_optimize
constexpr uint32_t kFgrResident = 4096;   // the largest set that stays on chip (gathered once into 96 KB of LDS); above it every pass streams from global memory
struct FgrOut {                           // what the loop leaves (device memory)
    float X[16];
    float mu;
    int32_t iters, status, reserved;
    double sums[kNSum];                   // the record of the last pass run
};
struct FgrArgs {
    const float4 *pq;                     // [m][2]: (p, 0), (q, 0)
    const int32_t *set;                   // [M] rows of pq, or null: element e is row e
    uint32_t M;
    float X0[16];                         // X of the first pass
    float mu0, delta2, division;          // mu before the first pass's schedule step
    int32_t iterations, decrease_every;
    int32_t pass_only;                    // 1: one pass at (X0, mu0), no schedule and no solve (symmicp_ctx_fgr_pass)
    float *weight;                        // [M] or null: l of every element, rewritten each pass
    float *X_trace;                       // [iterations + 1][16], zeroed, or null
    double *sums_trace;                   // [iterations][kNSum], zeroed, or null
    float *mu_trace;                      // [iterations], zeroed, or null
    FgrOut *out;
};
void launch_fgr_tuples(const float *pq8, uint32_t m, uint32_t trials, unsigned long long base, float edge2, uint32_t *flags, hipStream_t s);
void launch_fgr_scatter(const uint32_t *rank, uint32_t m, uint32_t trials, unsigned long long base, uint32_t max_tuples, int32_t *set, hipStream_t s);
void launch_fgr_optimize(const FgrArgs &a, hipStream_t s);

// pose-graph optimisation (kernels_posegraph.hip; symmicp_ctx_posegraph_optimize): one launch of one workgroup = one Levenberg-Marquardt
// iteration at the poses X: edge errors and blocks, the nodes' gathers, the block-Jacobi PCG, the trial poses and their cost, a record.
// Every array is fp64 in device memory.  An edge owns two slots of the incidence list (CSR by node, sorted by edge index): slot_s in its
// source's list, slot_t in its target's; what an edge contributes to a node goes to its slot, and the node adds its slots in order.
constexpr int kPgThreads = 256;           // workgroup size of k_posegraph_iteration
struct PgRecord {                         // what one launch leaves (device memory)
    double cost, cost_trial, model_decrease, grad_max, delta_max, hdiag_max, lambda, cg_residual;
    int32_t cg_iterations, status;
};
struct PgArgs {
    uint32_t n, m;
    int32_t ref, cg_max;
    double mu, lambda, cg_tol;            // lambda < 0: 1e-5 * the largest diagonal entry of H (the first iteration)
    const double *X;                      // [n][12]: the top three rows of every pose
    double *Xtrial;                       // [n][12]: X Exp(d); the reference node's rows copied
    const int32_t *es, *et, *eunc;        // [m]
    const double *T;                      // planar [12][m]: R_T row-major, t_T
    const double *L;                      // planar [21][m]: the upper triangle of the information matrix, row-major
    const uint32_t *off;                  // [n + 1]: the incidence list's row starts
    const uint32_t *slot_s, *slot_t;      // [m]
    double *e, *c, *l, *l_trial;          // [m][6], [m], [m], [m]
    double *slot_v;                       // [2 m][6]: gradient terms, then the matvec's terms
    double *slot_h;                       // [2 m][36]: diagonal-block terms
    double *g, *hdiag, *chol;             // [n][6], [n][36], [n][21]: the lower Cholesky factor of H_ii + lambda I, row-major triangle
    double *x, *r, *z, *p;                // [n][6]: the solve's vectors (x = d)
    PgRecord *rec;
};
void launch_posegraph_iteration(const PgArgs &a, hipStream_t s);

// registration evaluation (kernels_eval.hip; symmicp_ctx_evaluate_registration, symmicp_evaluate): K transforms of one source against one
// indexed target whose tq carries the caller's row in w.  The search runs over source positions (order: position -> caller row, null: the
// position; gather: the coordinates are stored by caller row and read through order), the sums over caller rows in an order that is a
// function of ns alone.  nn / d2 [K][ns] by caller row; partials [K][eval_sum_blocks(ns)][kEvalNSum]; sums [K][kEvalNSum] =
// inliers, sum d2, sum q (3), upper triangle of sum q q^T (6).
constexpr int kEvalThreads = 256;
constexpr int kEvalSearchThreads = 64;        // workgroup of k_eval_search: one wave (256: 5 % slower at K = 64; tiles dealt out strided: 25 - 45 % slower)
constexpr uint32_t kEvalRows = 1024;          // caller rows per block and trip of k_eval_sums
constexpr uint32_t kEvalMaxBlocks = 4096;     // ... and the most blocks per transform
constexpr int kEvalNSum = 11;
struct EvalArgs {
    TargetIndex ix;
    const float *sx, *sy, *sz;                // source coordinates, planar
    const uint32_t *order;
    int32_t gather;
    uint32_t ns;
    const float *X12;                         // [K][12]: the three top rows of every transform
    float r2;                                 // max_dist^2 in fp32, +Inf without a gate
    const float *tx, *ty, *tz;                // target coordinates by caller row, planar
    int32_t *nn;
    float *d2;
    double *partials;
};
uint32_t eval_sum_blocks(uint32_t ns);
void launch_eval(const EvalArgs &a, uint32_t K, double *sums, hipStream_t s);

}  // namespace symmicp
