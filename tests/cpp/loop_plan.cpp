// tests/cpp/loop_plan.cpp -- the scheduling rules of the ICP loop (icp-symm_amd/csrc/loop_plan.h) on the host, without a GPU.
//
//   loop_plan             (no arguments; built and run by tests/test_loop_plan.py, plain or with -fsanitize=address,undefined)
// Every expected value is a literal worked out from the rule as DESIGN.md states it (thresholds 50000, 2x, 256, 8192, 16384, n/10, 0.8,
// 400000, n/256 and 8192 scans, chunks 4/8/16, three heads), never a call of the function under test.
// Prints one line per group; exit code != 0 on the first failure.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "loop_plan.h"

using namespace symmicp;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static PassFeedback fb_list(uint64_t len) { PassFeedback f; f.set_list(len); return f; }
static PassFeedback fb_counts(uint64_t searched, uint64_t scans) { PassFeedback f; f.set_counts(searched, scans); return f; }
static PassFeedback fb_both(uint64_t len, uint64_t searched, uint64_t scans) { PassFeedback f; f.set_list(len); f.set_counts(searched, scans); return f; }
static PassFeedback fb_expected() { PassFeedback f; f.expect_list(); return f; }

static void test_feedback()
{
    PassFeedback f;
    CHECK(!f.list_known() && !f.list_empty() && !f.has_list() && !f.expects_list() && !f.counts_known());
    f.set_list(0);
    CHECK(f.list_known() && f.list_empty() && !f.has_list() && !f.expects_list());
    f.set_list(7);
    CHECK(f.list_known() && !f.list_empty() && f.has_list() && f.list_len == 7);
    f.expect_list();
    CHECK(!f.list_known() && !f.list_empty() && !f.has_list() && f.expects_list() && f.list_len == 0);
    f.set_counts(5, 3);
    CHECK(f.counts_known() && f.searched == 5 && f.scans == 3);
    f.forget_list();                                  // set_source and a bail-out of the device loop: the list alone
    CHECK(!f.list_known() && !f.expects_list() && f.counts_known() && f.searched == 5);
    f.forget_counts();
    CHECK(!f.counts_known() && f.searched == 0 && f.scans == 0);
    f.set_list_from_record(12); f.set_counts_from_record(9, 4);
    CHECK(f.has_list() && f.list_len == 12 && f.counts_known() && f.searched == 9 && f.scans == 4);
    f.set_list_from_record(-1); f.set_counts_from_record(-1, 0);
    CHECK(!f.list_known() && !f.counts_known());
    std::printf("feedback ok\n");
}

static void test_codec()
{
    CHECK(kFeedbackListSlot == 39 && kFeedbackCountSlot == 38);
    const uint32_t lens[] = {0u, 1u, 4294967294u}, searched[] = {0u, 4294967295u}, scans[] = {0u, 1u, 1048576u};
    for (uint32_t l : lens)
        for (uint32_t s : searched)
            for (uint32_t c : scans) {
                const FeedbackSlots e = feedback_encode(l, false, s, c);
                CHECK(e.list == (double)l && e.count == (double)s + 4294967296.0 * (double)c);
                const FeedbackWords w = feedback_decode(e.list, e.count);
                CHECK(!w.dropped && w.list_len == (double)l && w.searched == (double)s && w.scans == (double)c);
                CHECK(feedback_decode(feedback_encode(l, true, s, c).list, 0.0).dropped);
            }
    // eight ranks: the all-reduce adds the slots; exact while the total searched stays below 2^32 (and the total scanned below 2^21: the
    // slot is a double)
    const FeedbackSlots one = feedback_encode(1000u, false, 536870911u, 131072u);      // 8 x (2^29 - 1) = 2^32 - 8 searched, 8 x 2^17 = 2^20 scanned
    double list = 0.0, count = 0.0;
    for (int r = 0; r < 8; r++) { list += one.list; count += one.count; }
    FeedbackWords w = feedback_decode(list, count);
    CHECK(!w.dropped && w.list_len == 8000.0 && w.searched == 4294967288.0 && w.scans == 1048576.0);
    // one rank of the eight dropped appends
    list = feedback_encode(3u, true, 0u, 0u).list;
    for (int r = 1; r < 8; r++) list += feedback_encode(3u, false, 0u, 0u).list;
    CHECK(feedback_decode(list, 0.0).dropped);
    std::printf("codec ok\n");
}

// a TREE pass of a 1M-point single-rank run after its first pass, every switch on auto, certificates and neighbourhoods in place
static TreePassIn tree_in(const PassFeedback &fb)
{
    TreePassIn in{};
    in.first = false; in.writeback = false; in.rejecting = false;
    in.fb = fb;
    in.n_s_total = 1000000u; in.n_loc = 1000000u; in.nranks = 1;
    in.use_slack = true; in.have_certk = true;
    in.walk_full_grid = false;
    in.optimistic = in.compact = in.budget_walk = -1;
    in.hood_frac = 0.8;
    in.acc_blocks = 512; in.compact_blocks = 1280;
    return in;
}

static void test_walk_grid()
{
    const std::pair<uint64_t, uint32_t> known[] = {{0, 256u}, {100, 256u}, {128, 256u}, {129, 258u}, {4096, 8192u}, {50000, 8192u}, {50001, 0u}};
    for (const auto &k : known) CHECK(plan_tree_pass(tree_in(fb_list(k.first))).walk_blocks == k.second);
    CHECK(plan_tree_pass(tree_in(PassFeedback{})).walk_blocks == 0u);
    CHECK(plan_tree_pass(tree_in(fb_expected())).walk_blocks == 16384u);
    TreePassIn in = tree_in(fb_list(100));
    in.first = true;
    CHECK(plan_tree_pass(in).walk_blocks == 0u);
    in = tree_in(fb_expected()); in.first = true;
    CHECK(plan_tree_pass(in).walk_blocks == 0u);
    in = tree_in(fb_list(100)); in.walk_full_grid = true;
    CHECK(plan_tree_pass(in).walk_blocks == 0u);
    in = tree_in(fb_expected()); in.walk_full_grid = true;
    CHECK(plan_tree_pass(in).walk_blocks == 0u);
    CHECK(repair_walk_blocks(1) == 8192u && repair_walk_blocks(50000) == 8192u && repair_walk_blocks(50001) == 0u);
    std::printf("walk grid ok\n");
}

static void test_optimistic()
{
    CHECK(plan_tree_pass(tree_in(fb_list(0))).optimistic);
    CHECK(!plan_tree_pass(tree_in(fb_list(1))).optimistic);
    CHECK(!plan_tree_pass(tree_in(PassFeedback{})).optimistic);
    CHECK(!plan_tree_pass(tree_in(fb_expected())).optimistic);
    TreePassIn in = tree_in(fb_list(0)); in.first = true;
    CHECK(!plan_tree_pass(in).optimistic);
    in = tree_in(fb_list(0)); in.optimistic = 0;
    CHECK(!plan_tree_pass(in).optimistic);
    in = tree_in(fb_list(9)); in.optimistic = 1;
    CHECK(plan_tree_pass(in).optimistic);
    in.first = true;                                  // (the switch does not ask about the pass)
    CHECK(plan_tree_pass(in).optimistic);
    in = tree_in(fb_list(0)); in.optimistic = 1; in.writeback = true;
    CHECK(!plan_tree_pass(in).optimistic);
    in = tree_in(fb_list(0)); in.optimistic = 1; in.rejecting = true;
    CHECK(!plan_tree_pass(in).optimistic);
    in = tree_in(fb_list(0)); in.writeback = true;
    CHECK(!plan_tree_pass(in).optimistic);
    in = tree_in(fb_list(0)); in.rejecting = true;
    CHECK(!plan_tree_pass(in).optimistic);
    std::printf("optimistic ok\n");
}

static void test_compact()
{
    TreePassIn in = tree_in(fb_counts(99, 0)); in.n_s_total = 1000u;
    CHECK(plan_tree_pass(in).compact_blocks == 1280);
    in.fb = fb_counts(100, 0);
    CHECK(plan_tree_pass(in).compact_blocks == 0);
    in.fb = fb_counts(0, 0); in.n_s_total = 9u;       // 9 / 10 == 0: nothing is below it
    CHECK(plan_tree_pass(in).compact_blocks == 0);
    in = tree_in(PassFeedback{});                     // counts unknown
    CHECK(plan_tree_pass(in).compact_blocks == 0);
    in = tree_in(fb_counts(99, 0)); in.n_s_total = 1000u; in.use_slack = false;
    CHECK(plan_tree_pass(in).compact_blocks == 0);
    in.compact = 1;                                   // the switch does not replace use_slack
    CHECK(plan_tree_pass(in).compact_blocks == 0);
    in.use_slack = true; in.fb = PassFeedback{};
    CHECK(plan_tree_pass(in).compact_blocks == 1280);
    in = tree_in(fb_counts(0, 0)); in.compact = 0;
    CHECK(plan_tree_pass(in).compact_blocks == 0);
    in = tree_in(fb_counts(0, 0)); in.compact_blocks = 640;
    CHECK(plan_tree_pass(in).compact_blocks == 640);
    std::printf("compact ok\n");
}

static void test_make_hood()
{
    TreePassIn in = tree_in(fb_counts(799, 0)); in.n_s_total = 1000u;      // 0.8 x 1000 = 800
    CHECK(plan_tree_pass(in).make_hood);
    in.fb = fb_counts(800, 0);
    CHECK(!plan_tree_pass(in).make_hood);
    in.fb = fb_counts(799, 0); in.have_certk = false;
    CHECK(!plan_tree_pass(in).make_hood);
    in.have_certk = true; in.first = true;
    CHECK(!plan_tree_pass(in).make_hood);
    in.first = false; in.fb = PassFeedback{};
    CHECK(!plan_tree_pass(in).make_hood);
    in.fb = fb_counts(499, 0); in.hood_frac = 0.5;
    CHECK(plan_tree_pass(in).make_hood);
    in.fb = fb_counts(500, 0);
    CHECK(!plan_tree_pass(in).make_hood);
    std::printf("make_hood ok\n");
}

static void test_budget_walk()
{
    TreePassIn in = tree_in(PassFeedback{});
    in.first = true; in.nranks = 2; in.n_loc = 399999u;
    CHECK(plan_tree_pass(in).budget_walk);
    in.n_loc = 400000u;
    CHECK(!plan_tree_pass(in).budget_walk);
    in.n_loc = 399999u; in.nranks = 1;
    CHECK(!plan_tree_pass(in).budget_walk);
    in.nranks = 2; in.first = false;
    CHECK(!plan_tree_pass(in).budget_walk);
    in.budget_walk = 1;
    CHECK(plan_tree_pass(in).budget_walk);
    in.first = true; in.budget_walk = 0;
    CHECK(!plan_tree_pass(in).budget_walk);
    std::printf("budget_walk ok\n");
}

static void test_grids()
{
    // accumulate, cap 512: a multiple of 8 below the cap, 8 at the least
    CHECK(accumulate_blocks(256u, 512) == 8 && accumulate_blocks(9u * 256u, 512) == 16 && accumulate_blocks(600u * 256u, 512) == 512);
    CHECK(accumulate_blocks(0u, 512) == 8 && accumulate_blocks(1u, 512) == 8 && accumulate_blocks(8u * 256u + 1u, 512) == 16 && accumulate_blocks(511u * 256u, 512) == 512);
    CHECK(capped_blocks(256u, 512, true, 8) == 8 && capped_blocks(9u * 256u, 512, true, 8) == 16 && capped_blocks(600u * 256u, 512, true, 8) == 512);
    TreePassIn in = tree_in(PassFeedback{}); in.n_loc = 9u * 256u;
    CHECK(plan_tree_pass(in).acc_blocks == 16);
    // NDT: one block per tile up to the cap
    CHECK(ndt_blocks(256u, 512) == 1 && ndt_blocks(9u * 256u, 512) == 9 && ndt_blocks(600u * 256u, 512) == 512 && ndt_blocks(0u, 512) == 1);
    CHECK(fused_pass_blocks(0u, 512) == 1 && fused_pass_blocks(257u, 512) == 2 && fused_pass_blocks(1000000u, 512) == 512);
    CHECK(host_pass_cap(2048) == 2048 && host_pass_cap(8192) == 8192 && host_pass_cap(8193) == 8192 && host_pass_cap(100000) == 8192);
    // identity: 16-byte loads need all three of n_loc, n_t and the shard offset divisible by 4
    CHECK(identity_grid(1024u, 1024u, 0u, 2048).vec4 && identity_vec4(1024u, 2048u, 512u));
    CHECK(!identity_grid(1025u, 1024u, 0u, 2048).vec4 && !identity_grid(1024u, 1026u, 0u, 2048).vec4 && !identity_grid(1024u, 1024u, 2u, 2048).vec4);
    CHECK(!identity_vec4(1023u, 1024u, 0u) && !identity_vec4(1024u, 1023u, 0u) && !identity_vec4(1024u, 1024u, 1u));
    const std::pair<uint32_t, int> vec4[] = {{4u, 1}, {1024u, 1}, {1028u, 2}, {4u * 256u * 2048u + 4u, 2048}, {4u * 256u * 2048u, 2048}, {4u * 256u * 2047u, 2047}, {0u, 1}};
    for (const auto &k : vec4) {
        const IdentityGrid g = identity_grid(k.first, k.first, 0u, 2048);
        CHECK(g.vec4 && g.blocks == k.second);
    }
    // ... and one point per thread otherwise
    const std::pair<uint32_t, int> scalar[] = {{4u, 1}, {1024u, 4}, {1028u, 5}, {4u * 256u * 2048u + 4u, 2048}, {256u * 2047u + 1u, 2048}, {256u * 2047u, 2047}};
    for (const auto &k : scalar) {
        const IdentityGrid g = identity_grid(k.first, k.first, 1u, 2048);
        CHECK(!g.vec4 && g.blocks == k.second);
    }
    std::printf("grids ok\n");
}

// a TREE run that may start: cumulative PAPER, certificates, 1M points (scan limit 3906), an empty list, nothing searched
static BatchEligibleIn eligible_in()
{
    BatchEligibleIn in{};
    in.device_solves = true;
    in.host_passes_since_bailout = 2;
    in.tree = true;
    in.certificates = true;
    in.n_s_total = 1000000u;
    in.fb = fb_both(0, 0, 0);
    return in;
}

static void test_batch_eligible()
{
    CHECK(loop_scan_limit(255u) == 0u && loop_scan_limit(256u) == 1u && loop_scan_limit(256u * 8192u + 1u) == 8192u);
    CHECK(loop_scan_limit(256u * 8192u - 1u) == 8191u && loop_scan_limit(4294967295u) == 8192u && loop_scan_limit(1000000u) == 3906u);
    CHECK(loop_slow_limit(1000000u) == 15624u && loop_slow_limit(4294967295u) == 32768u && kLoopListLimit == 8192u);
    CHECK(batch_eligible(eligible_in()));
    // one refusal each
    BatchEligibleIn in = eligible_in(); in.host_loop_switch = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.rejecting = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.color = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.host_loop_config = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.host_exchange = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.host_diagnostics = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.device_solves = false; CHECK(!batch_eligible(in));
    in = eligible_in(); in.empty_share_alone = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.host_passes_since_bailout = 1; CHECK(!batch_eligible(in));
    in = eligible_in(); in.host_passes_since_bailout = 0; CHECK(!batch_eligible(in));
    in = eligible_in(); in.tree = false; CHECK(!batch_eligible(in));                       // brute force
    // identity pairing asks nothing of the feedback, the apply mode or the certificates
    in = eligible_in(); in.tree = false; in.identity = true; in.fb = PassFeedback{}; in.incremental = true; in.certificates = false;
    CHECK(batch_eligible(in));
    in.host_passes_since_bailout = 1; CHECK(!batch_eligible(in));
    // TREE
    in = eligible_in(); in.incremental = true; CHECK(!batch_eligible(in));
    in = eligible_in(); in.certificates = false; CHECK(!batch_eligible(in));
    in = eligible_in(); in.fb = fb_counts(0, 0); CHECK(!batch_eligible(in));              // list unknown
    in = eligible_in(); in.fb = fb_expected(); in.fb.set_counts(0, 0); CHECK(!batch_eligible(in));
    in = eligible_in(); in.fb = fb_list(0); CHECK(!batch_eligible(in));                   // counts unknown
    // the scan limit (3906 at 1M points) halves when the last pass left a list
    in = eligible_in(); in.fb = fb_both(0, 3906, 0); CHECK(batch_eligible(in));
    in.fb = fb_both(0, 3907, 0); CHECK(!batch_eligible(in));
    in.fb = fb_both(1, 1953, 0); CHECK(batch_eligible(in));
    in.fb = fb_both(1, 1954, 0); CHECK(!batch_eligible(in));
    in.fb = fb_both(8192, 1953, 0); CHECK(batch_eligible(in));
    in.fb = fb_both(8193, 1953, 0); CHECK(!batch_eligible(in));
    in.fb = fb_both(8193, 0, 0); CHECK(!batch_eligible(in));
    in = eligible_in(); in.no_loop_stragglers = true; CHECK(batch_eligible(in));
    in.fb = fb_both(1, 0, 0); CHECK(!batch_eligible(in));
    in = eligible_in(); in.n_s_total = 255u; CHECK(batch_eligible(in));                    // limit 0: nothing searched passes
    in.fb = fb_both(0, 1, 0); CHECK(!batch_eligible(in));
    in = eligible_in(); in.n_s_total = 4294967295u; in.fb = fb_both(0, 8192, 0); CHECK(batch_eligible(in));
    in.fb = fb_both(0, 8193, 0); CHECK(!batch_eligible(in));
    std::printf("batch_eligible ok\n");
}

typedef std::vector<std::pair<int, bool>> Chunks;
// chunks of a run of `want` passes; (list, scans)[k] is what the last complete pass in front of chunk k left, any_list[k] whether a pass
// of chunk k left a list
static Chunks run_chunks(ChunkPlanner pl, int want, const std::vector<std::pair<uint64_t, uint64_t>> &last, const std::vector<bool> &any_list,
                         std::vector<bool> *stage = nullptr)
{
    Chunks out;
    int enq = 0, prev = 0;
    for (size_t k = 0; enq < want; k++) {
        const std::pair<uint64_t, uint64_t> &l = last[k < last.size() ? k : last.size() - 1];
        if (stage) stage->push_back(pl.stragglers());
        const ChunkPlan p = pl.next(l.first, l.second, want - enq, prev);
        const int nq = want - enq < p.passes ? want - enq : p.passes;
        out.push_back({nq, p.certified});
        enq += nq; prev = p.passes;
        pl.after_chunk(any_list[k < any_list.size() ? k : any_list.size() - 1]);
    }
    return out;
}

static void test_chunks()
{
    // a run that can stop by itself: 4, 8, 16, ..., the last one cut to what is left
    CHECK((run_chunks(ChunkPlanner(true, false, 1, false, 4), 64, {{0, 5}}, {false}) == Chunks{{4, false}, {8, false}, {16, false}, {32, false}, {4, false}}));
    CHECK((run_chunks(ChunkPlanner(false, false, 0, false, 4), 30, {{0, 0}}, {false}) == Chunks{{4, false}, {8, false}, {16, false}, {2, false}}));      // identity
    CHECK((run_chunks(ChunkPlanner(), 12, {{0, 0}}, {false}) == Chunks{{4, false}, {8, false}}));
    // ... and the certified-only kernel as soon as a chunk's last pass left no list and scanned nothing
    CHECK((run_chunks(ChunkPlanner(true, false, 1, false, 4), 28, {{0, 5}, {0, 0}, {0, 1}}, {false}) == Chunks{{4, false}, {8, true}, {16, false}}));
    // the stage on at entry: chunks of 4 while passes leave lists, then doubling from 4 ...
    std::vector<bool> stage;
    CHECK((run_chunks(ChunkPlanner(true, true, 1, false, 4), 40, {{3, 9}, {2, 4}, {0, 0}}, {true, true, false}, &stage) ==
           Chunks{{4, false}, {4, false}, {4, false}, {8, true}, {16, true}, {4, true}}));
    CHECK((stage == std::vector<bool>{true, true, true, false, false, false}));
    // ... or the rest in one piece
    CHECK((run_chunks(ChunkPlanner(true, true, 1, true, 4), 40, {{3, 9}, {2, 4}, {0, 0}}, {true, true, false}) == Chunks{{4, false}, {4, false}, {4, false}, {28, true}}));
    CHECK((run_chunks(ChunkPlanner(true, true, 1, true, 4), 40, {{3, 9}, {2, 4}, {0, 2}}, {true, true, false}) == Chunks{{4, false}, {4, false}, {4, false}, {28, false}}));
    // the stage comes on when a chunk leaves a list, and never without permission (SYMMICP_NO_LOOP_STRAGGLERS, identity runs)
    stage.clear();
    run_chunks(ChunkPlanner(true, false, 1, false, 4), 20, {{0, 0}}, {true, false}, &stage);
    CHECK((stage == std::vector<bool>{false, true, false, false}));
    stage.clear();
    run_chunks(ChunkPlanner(false, true, 1, false, 4), 12, {{5, 5}}, {true}, &stage);
    CHECK((stage == std::vector<bool>{false, false}));
    // one piece, scans at entry: three heads of cert_head fused passes, then the rest
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 4), 30, {{0, 7}}, {false}) == Chunks{{4, false}, {4, false}, {4, false}, {18, false}}));
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 4), 30, {{0, 7}, {0, 0}}, {false}) == Chunks{{4, false}, {26, true}}));
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 4), 30, {{0, 0}}, {false}) == Chunks{{30, true}}));
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 4), 4, {{0, 7}}, {false}) == Chunks{{4, false}}));         // not above cert_head: one piece
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 4), 5, {{0, 7}}, {false}) == Chunks{{4, false}, {1, false}}));
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 7), 30, {{0, 7}}, {false}) == Chunks{{7, false}, {7, false}, {7, false}, {9, false}}));
    CHECK((run_chunks(ChunkPlanner(true, false, 1, true, 0), 30, {{0, 7}}, {false}) == Chunks{{30, false}}));       // SYMMICP_CERT_HEAD=0: no heads
    CHECK((run_chunks(ChunkPlanner(true, false, 0, true, 4), 30, {{0, 0}}, {false}) == Chunks{{30, false}}));       // SYMMICP_CERT_PASS=0
    // a list at entry: the stage, and no heads afterwards
    CHECK((run_chunks(ChunkPlanner(true, true, 1, true, 4), 30, {{2, 7}, {0, 7}}, {false}) == Chunks{{4, false}, {26, false}}));
    // SYMMICP_CERT_PASS=2: certified-only from the first chunk, and the stage never on
    stage.clear();
    CHECK((run_chunks(ChunkPlanner(true, true, 2, false, 4), 28, {{5, 9}}, {true}, &stage) == Chunks{{4, true}, {8, true}, {16, true}}));
    CHECK((stage == std::vector<bool>{false, false, false}));
    CHECK((run_chunks(ChunkPlanner(true, true, 2, true, 4), 30, {{5, 9}}, {true}) == Chunks{{30, true}}));
    std::printf("chunks ok\n");
}

int main()
{
    test_feedback();
    test_codec();
    test_walk_grid();
    test_optimistic();
    test_compact();
    test_make_hood();
    test_budget_walk();
    test_grids();
    test_batch_eligible();
    test_chunks();
    std::printf("loop_plan: ok\n");
    return 0;
}
