// engine_internal.h -- what the host-side translation units of libsymmicp share: the context, its scratch arenas, the environment
// switches, the RCCL loader and the helpers every entry point uses.
//   engine.cpp           lifetime, configuration, set_target / set_source, getters, statistics
//   engine_index.cpp     the index: its store (IndexStore), upload_planar, morton_order, build_index, ScratchIndex, the reverse index
//   engine_cloud_ops.cpp stand-alone cloud operations on a scratch index: normals and k-NN, radius search, FPFH, ISS keypoints, intensity
//                        gradient; voxel downsampling
//   engine_loop.cpp      the iteration loop: one pass (run_pass), device-driven runs of passes (run_batch), begin / step / align, result block;
//                        what it launches is decided by the plain functions of loop_plan.h (no HIP, no context: tests/cpp/loop_plan.cpp)
//   engine_exchange.cpp  multi-GPU: RCCL (loaded lazily), shared-memory exchange, communicator entry points
//   engine_global.cpp    feature matching and RANSAC (symmicp_ctx_feature_nn, symmicp_ctx_feature_correspondences, symmicp_ctx_ransac)
//   engine_debug.cpp     SYMMICP_DEBUG_COUNTERS / SYMMICP_DEBUG_TRACE dumps
//   engine_probe.cpp     test entries: read-back of the target index and the source share, the sort and the scan on caller arrays
//   engine_eval.cpp      registration evaluation (symmicp_evaluate_registration, symmicp_evaluate, symmicp_information_from_sums)
//   engine_fgr.cpp       Fast Global Registration (symmicp_ctx_fgr, symmicp_ctx_fgr_pass)
//   engine_posegraph.cpp pose-graph optimisation (symmicp_ctx_posegraph_optimize, symmicp_ctx_posegraph_pass, the two host helpers)
//   engine_plane.cpp     RANSAC plane segmentation (symmicp_ctx_segment_plane, symmicp_ctx_plane_hypotheses)
//   engine_ndt.cpp       SYMMICP_MODE_NDT: configuration, Gauss constants, the voxel map (build, read-back, symmicp_ctx_ndt_map), pass arguments
#pragma once
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <vector>

#include "symmicp.h"
#include "symmicp_internal.h"
#include "host_solve.h"
#include "loop_plan.h"


namespace symmicp {}
using namespace symmicp;

// ---- RCCL, loaded lazily (single-GPU users never touch it) ---------------------
typedef struct { char internal[128]; } rcclUniqueId;
typedef void *rcclComm_t;
typedef int (*fn_ncclGetUniqueId)(rcclUniqueId *);
typedef int (*fn_ncclCommInitRank)(rcclComm_t *, int, rcclUniqueId, int);
typedef int (*fn_ncclCommDestroy)(rcclComm_t);
typedef int (*fn_ncclAllReduce)(const void *, void *, size_t, int, int, rcclComm_t, hipStream_t);
typedef const char *(*fn_ncclGetErrorString)(int);
constexpr int kNcclFloat64 = 8;   // ncclDouble (rccl.h ncclDataType_t)
constexpr int kNcclSum = 0;       // ncclSum

struct Rccl {
    void *handle = nullptr;
    fn_ncclGetUniqueId GetUniqueId = nullptr;
    fn_ncclCommInitRank CommInitRank = nullptr;
    fn_ncclCommDestroy CommDestroy = nullptr;
    fn_ncclAllReduce AllReduce = nullptr;
    fn_ncclGetErrorString GetErrorString = nullptr;
    std::string err;
    std::mutex mu;
    bool load()
    {
        std::lock_guard<std::mutex> lock(mu);       // contexts of different host threads may attach communicators concurrently
        if (handle && AllReduce) return true;
        // prefer an RCCL already mapped into the process (e.g. the copy torch links against)
        const char *names[] = {"librccl.so.1", "librccl.so"};
        for (const char *nm : names) { handle = dlopen(nm, RTLD_NOW | RTLD_NOLOAD | RTLD_GLOBAL); if (handle) break; }
        if (!handle)
            for (const char *nm : names) { handle = dlopen(nm, RTLD_NOW | RTLD_GLOBAL); if (handle) break; }
        if (!handle) { err = std::string("cannot load librccl: ") + dlerror(); return false; }
        GetUniqueId = (fn_ncclGetUniqueId)dlsym(handle, "ncclGetUniqueId");
        CommInitRank = (fn_ncclCommInitRank)dlsym(handle, "ncclCommInitRank");
        CommDestroy = (fn_ncclCommDestroy)dlsym(handle, "ncclCommDestroy");
        AllReduce = (fn_ncclAllReduce)dlsym(handle, "ncclAllReduce");
        GetErrorString = (fn_ncclGetErrorString)dlsym(handle, "ncclGetErrorString");
        if (!GetUniqueId || !CommInitRank || !CommDestroy || !AllReduce) { err = "librccl misses nccl* symbols"; return false; }
        return true;
    }
};
extern Rccl g_rccl;      // (engine_exchange.cpp)

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Every SYMMICP_* environment switch, read ONCE in symmicp_create (A/B runs and tests; none is needed in production -- DESIGN.md 6 lists
// them).  Nothing on the pass loop calls getenv.
struct Switches {
    bool allow_any_arch = false, debug_host = false, debug_counters = false;
    std::string debug_trace;               // per-packet trace file of the first pass ("" = off)
    double grid_ppc = 3.0;                 // points per occupied cell the grid level is chosen for (2.0 until the end of round 3: one level finer on the surface pairs -- 15 (query, cell) items of ~1 point per probe instead of 8 of ~4; 1M pair 12 740 -> 13 230 iter/s at 20 iterations, 250k / 4M +3 %, scan pairs and the 100k cube unchanged)
    int grid_maxlevel = kMortonBits, grid_level = -1;      // -1: chosen from the cloud; 0 disables the grid phase
    int first_pass = -1;                   // -1: decided per target (build_index); 0: per-thread walk; 1: packets
    int oct_leaf = 0;                      // octree leaf size (0: 24 on surface-like targets, 8 otherwise)
    bool packet_order = true;              // packets started longest-first
    bool packet_cost_key = true;           // ... keyed by their distance to the target when it is known at set_source (0: by radius alone)
    float packet_jump = -1.0f;             // cut factor of k_packet_runs (< 0: the default, 0: never cut)
    int packet_key_bits = 16;
    uint32_t packet_chunk = 0, packet_lds_pad = 0, packet_waves = 0, packet_front_cap = 0;
    double hood_frac = 0.8;                // scans keep neighbourhoods once the previous pass searched under this fraction of the pairs
    bool no_hood = false, no_cert = false, walk_full_grid = false, host_loop = false, no_loop_stragglers = false, force_comm = false;
    int budget_walk = -1, optimistic = -1, compact = -1;      // -1 auto, 0 never, 1 always
    int cert_pass = 1;                     // k_pass_certified in the device loop: 0 never, 1 by run_batch's rule, 2 from the first device pass whatever the counts say
    int cert_head = 4;                     // ... passes of the fused head of a run that goes out in one piece (run_batch)
    int pass_blocks = 2048, id_blocks = 2048, acc_blocks = 512, fused_blocks = 512, compact_blocks = 1280;
    int feature_nn_splits = 0, feature_nn_queries = 0;      // symmicp_ctx_feature_nn: candidate splits / queries per thread (0: chosen from the sizes)
    int plane_score = 0;                   // symmicp_ctx_segment_plane: the scoring kernel (launch_plane_score's shape; A/B runs)
    PassTuning tune;                       // wave_mode_max, cells_chunk, walk_budget
};

void read_switches(Switches &w);

// Scratch arena of a context: the builds need dozens of temporaries, and every hipFree costs ~100 us (it synchronises the
// device) -- half of a set_target + set_source at 1M points.  Temporaries are bump-allocated from one block that is
// rewound at the start of each public call and only ever grows; persistent results are hipMalloc'ed as before.
struct Arena {
    char *base = nullptr;
    size_t cap = 0, off = 0;
};

// Intra-node exchange of the 40-double record through POSIX shared memory (symmicp_comm_init_shm): every rank spins on
// its own GPU's record as in the single-GPU path, publishes it in its slot, waits for the other ranks' slots and adds
// them up in rank order (so every rank gets bit-identical sums).  For a 320-byte latency-bound exchange this beats a
// collective kernel launch; slots are double-buffered by exchange parity (a rank cannot be more than one exchange ahead).
struct ShmSlot {
    volatile unsigned long long seq;
    double s[SYMMICP_NSUM];
    char pad[512 - 8 - 8 * SYMMICP_NSUM];
};
static_assert(sizeof(ShmSlot) == 512, "slot = 4 cache lines");
struct ShmExchange {
    ShmSlot *slots = nullptr;        // [2][nranks]
    size_t bytes = 0;
    unsigned long long count = 0;    // exchanges done
    std::string name;
    bool owner = false;
};

// What build_index knew and the index itself does not keep: a few words per target, read back by symmicp_ctx_index_info (tests)
struct IndexNotes {
    float origin[3] = {0, 0, 0}, h0 = 0.f;      // Morton frame: bounding-box minimum and the finest cell edge
    uint32_t hist[16] = {};                    // level histogram the grid level and the surface-like flag were decided from
    uint32_t leaf_max = 0;                     // octree leaf size in force
    uint32_t nblocks = 0, ctop_len = 0;        // occupied super-cell blocks of the cell table, length of ctop
};

// The device memory of one index: a block that only grows, bump-allocated in 256-byte steps, and the allocations that did not fit it.
// The context's target owns one (the scratch index of a cloud operation goes behind the target's arrays, under a mark), every
// ReverseIndex one.  (engine_index.cpp)
struct IndexStore {
    struct Mark { size_t off = 0, extras = 0; };
    IndexStore() = default;
    IndexStore(const IndexStore &) = delete;
    IndexStore &operator=(const IndexStore &) = delete;
    ~IndexStore() { release(); }
    hipError_t alloc(void **out, size_t bytes);      // from the block when it fits, else a hipMalloc of its own (tracked)
    // cap() < want: the block is replaced by one of want + slack bytes (contents dead); if that fails, every alloc falls back
    void reserve(size_t want, size_t slack);
    Mark mark() const { return Mark{blk.off, extra.size()}; }
    void rewind(Mark m);                             // what was allocated since the mark is given back (beside the block: freed)
    void reset() { rewind(Mark{}); }                 // empty; the block is kept for the next index
    void release();                                  // everything freed; idempotent
    size_t cap() const { return blk.cap; }
    size_t used() const { return blk.off; }
    size_t beside() const { return extra.size(); }   // allocations that did not fit the block

private:
    Arena blk;
    std::vector<void *> extra;
};

// What build_index is asked for, and what it returns
struct IndexRequest {
    float4 *tq, *tn;      // the caller's arrays: n sorted points (the target's and the reverse index's: + 8 zeroed, the packet search reads a
                          // leaf's points in groups of 8) and n (point, normal) pair records
    bool grid;            // the cell table, and with it the surface-like decision
    int oct_leaf;         // -1: no octree; 0: leaves of 24 points on a surface-like cloud, else of 8; > 0: that size
};
struct BuiltIndex {
    TargetIndex ix{};
    bool surface_like = false;      // (grid only) decides the first-pass regime
    int32_t grid_level = 0, tree_levels = 0;
    IndexNotes notes;
};

// An index with a store of its own: the source index of reciprocal passes, the scratch index of the evaluation and of the reverse probe
struct ReverseIndex {
    IndexStore store;
    TargetIndex ix{};
    bool valid = false;
    void drop() { store.reset(); ix = TargetIndex{}; valid = false; }      // back to "not built"; the block is kept for the next build
};

// The rejectors of a context (symmicp_set_trim_fraction / _one_to_one / _median_factor / _reciprocal): what is set, the buffers a rejecting
// pass runs on (allocated by the first such pass, kept for the next), and what the most recent pass left for the three state getters.
struct Rejectors {
    float trim_frac = 1.0f, med_factor = 0.0f;    // 1 and 0: off
    bool one_to_one = false, reciprocal = false;
    uint32_t *keys = nullptr, *ws = nullptr;      // per share row; the select's workspace
    unsigned long long *table = nullptr;          // the claim table: one word per target point, and behind them a reciprocal pass's RecipArgs
    size_t keys_cap = 0, table_cap = 0;
    ReverseIndex src_ix;             // reciprocal: the index over the original source, built by the first reciprocal pass after a set_source
    uint64_t src_ix_builds = 0;      // ... builds since symmicp_create (symmicp_ctx_reciprocal_info: tests)
    RecipArgs recip_args{};          // ... host copy of what the pass's kernel reads: that index and the inverse of c->X
    // the most recent pass: which rejectors were set when it ran (0: it rejected nothing, or there was none since set_config / set_source)
    enum : uint32_t { kTrim = 1, kMedian = 2, kOneToOne = 4, kReciprocal = 8 };
    uint32_t ran = 0;
    RejectRecord last{};
    void invalidate() { ran = 0; }

    bool trims() const { return trim_frac < 1.0f; }
    bool median() const { return med_factor > 0.0f; }
    // Identity pairs are one-to-one as they are: the option launches nothing there.  Reciprocal correspondences (never IDENTITY: the setter
    // and set_config see to it) imply the claim.
    bool claims(int corr) const { return (one_to_one || reciprocal) && corr != SYMMICP_CORR_IDENTITY; }
    bool checks_back(int corr) const { return reciprocal && corr != SYMMICP_CORR_IDENTITY; }
    bool rejects(int corr) const { return trims() || median() || claims(corr); }
    uint32_t settings_mask(int corr) const
    {
        if (!rejects(corr)) return 0u;
        return (trims() ? kTrim : 0u) | (median() ? kMedian : 0u) | (one_to_one ? kOneToOne : 0u) | (checks_back(corr) ? kReciprocal : 0u);
    }
    // what the getters may report: the keys (symmicp_get_correspondences) after any rejecting pass, symmicp_get_trim_state after a trimmed
    // one, symmicp_get_rejection_state after one with any of the other three, symmicp_get_reciprocal_state after a reciprocal one
    bool keys_valid() const { return ran != 0u; }
    bool trim_state_valid() const { return (ran & kTrim) != 0u; }
    bool rejection_state_valid() const { return (ran & (kMedian | kOneToOne | kReciprocal)) != 0u; }
    bool reciprocal_state_valid() const { return (ran & kReciprocal) != 0u; }
    // 64-bit words of the claim table for n_t target points
    static size_t table_words(size_t n_t, bool with_recip_tail) { return (n_t ? n_t : 1) + (with_recip_tail ? kRecipTailWords : 0); }
};

// The voxel map of SYMMICP_MODE_NDT in device memory (kernels_ndt.hip): own allocations that only grow, kept for the next target
struct NdtMap {
    float4 *rec = nullptr;               // [m][4]
    double *cov = nullptr;               // [m][6]
    uint32_t *key = nullptr;             // [m]
    unsigned long long *table = nullptr;
    size_t rec_cap = 0, cov_cap = 0, key_cap = 0, table_cap = 0;
    uint32_t m = 0;
    NdtGrid g{};                         // what the kernels read of it
    int32_t dims[3] = {0, 0, 0};
    bool valid = false;
    void release()
    {
        hipFree(rec); hipFree(cov); hipFree(key); hipFree(table);
        *this = NdtMap{};
    }
};
// NDT on a context: the configuration, the constants derived from it, the target's map and what the most recent pass left
struct NdtState {
    symmicp_ndt_config cfg{};
    double d1 = 0.0, d2 = 0.0;           // symmicp_ndt_gauss(cfg.outlier_ratio)
    NdtMap map;
    bool pass_valid = false;
    double score = 0.0;
    uint64_t items = 0;
};

struct symmicp_ctx {
    Switches sw;                     // environment switches as they stood at symmicp_create
    Arena arena;                     // temporaries of one public call
    IndexStore tgt_store;            // the target's persistent arrays (reused by the next set_target)
    ShmExchange shm;
    symmicp_config cfg{};
    int loss = SYMMICP_LOSS_NONE;    // robust loss (symmicp_set_robust_loss) and its scale: read by every pass
    float loss_scale = 0.f;
    float gicp_eps = 1e-3f;          // SYMMICP_MODE_GICP's covariance eps (symmicp_set_gicp_epsilon): read by every GICP pass
    // colored ICP (SYMMICP_MODE_COLOR): lambda, and the attributes in the order the clouds are kept in -- (gradient, intensity) per target
    // point (the order of tn; of the planar target with identity pairing), the intensity per share row.  Own allocations, kept for the
    // next cloud; have_*: set by symmicp_set_*_intensity, dropped by the cloud's next set_target / set_source
    float color_lam = 0.968f;
    float4 *tgt_color = nullptr;
    float *src_int = nullptr;
    size_t tgt_color_cap = 0, src_int_cap = 0;
    bool have_tgt_color = false, have_src_int = false;
    NdtState ndt;                    // SYMMICP_MODE_NDT: configuration, the target's voxel map, the last pass's score
    Rejectors rej;                   // trim fraction, one-to-one, median distance, reciprocal: settings, buffers, the last pass's result
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    // communicator
    int nranks = 1, rank = 0;
    rcclComm_t comm = nullptr;
    bool external_exchange = false;  // sharded, but the application sums the records (symmicp_set_sums)
    bool sums_exchanged = false;     // ... and has done so for the last pass
    // target
    uint32_t n_t = 0;
    float *tgt_block = nullptr;      // 6 planar arrays
    CloudSoA tgt{};
    TargetIndex ix{};                   // TREE: the whole index; BRUTE: tq, tn and n only; IDENTITY: empty.  dbg / dbg_trace: own allocations
                                        // (SYMMICP_DEBUG_COUNTERS; SYMMICP_DEBUG_TRACE=file, the per-packet trace of the first pass)
    bool have_index = false;            // the tree index exists (TREE)
    bool target_surface_like = false;   // decides the first-pass regime (set_target, from build_index's result)
    IndexNotes notes;                   // (tests: symmicp_ctx_index_info)
    float pivot[3] = {0, 0, 0};
    // source share
    uint32_t n_s_total = 0, n_loc = 0, src_off = 0;
    bool src_no_normals = false;     // the source came without normals (PLANE only): its normal columns hold zeros
    char *src_all = nullptr;         // one allocation behind all per-source arrays below (reused by the next set_source)
    size_t src_all_cap = 0;
    float *src0_block = nullptr, *cur_block = nullptr;
    CloudSoA src0{}, cur{};
    uint32_t *src_order = nullptr;   // share position -> row in the caller's cloud (null = identity)
    int32_t *pos = nullptr;
    float *d2 = nullptr;
    float4 *pairrec = nullptr;       // TREE: per pair, its own copy of the target's (point, normal) record
    float *cert = nullptr;           // TREE pair certificates: one float4 (ref.xyz, clear radius) per source point
    uint32_t *certk = nullptr;       // ... and their neighbourhood certificates: 8 member words per source point
    float *hoodr = nullptr;          // ... (T, radius hint) per source point
    uint32_t *pkt_tab = nullptr;     // TREE: the first pass's packets, (first query, count) in start order (widest first)
    uint32_t pkt_count = 0;
    bool pkt_cost_keyed = false;     // ... started by their distance to the target (k_packet_cost), not by their radius
    uint32_t *pkt_fallbacks = nullptr;  // device counter: packets of first passes that finished depth-first (k_search_packet)
    unsigned long long *best64 = nullptr;
    uint32_t *worklist = nullptr, *wl_count = nullptr;   // the sharded work list + its counters
    WorkLists wl{};
    // reduction
    int pass_blocks = 0;
    double *partials = nullptr, *d_sums = nullptr, *h_sums = nullptr, *h_sums_dev = nullptr;   // h_sums: 40 doubles + sequence word
    uint32_t *ticket = nullptr;          // ticket of the final reduce
    PassFeedback fb;                     // what the last pass tells the next: its work list and the pairs it searched and scanned (loop_plan.h)
    bool cert_pass_failed = false;       // a certified-only pass of this alignment came back incomplete: the kernel is not chosen again
    // device-driven runs of passes (run_batch): loop state in device memory, per-pass records + end flag in host-mapped memory
    static constexpr int kRing = 65;
    LoopState *d_loop = nullptr, *h_loop = nullptr, *h_loop_dev = nullptr;
    LoopRecord *h_ring = nullptr, *h_ring_dev = nullptr;
    unsigned long long *h_done = nullptr, *h_done_dev = nullptr;
    unsigned long long batch_seq = 0;
    bool loop_log_on = false;                            // symmicp_set_loop_log (tests): run_batch appends every device-driven pass
    std::vector<symmicp_loop_log_entry> loop_log;        // ... of the last symmicp_align
    int loop_log_batches = 0;
    int host_passes_since_bailout = 1000;   // batches resume after two clean host-driven passes
    unsigned long long seq = 0;
    // loop state
    bool begun = false;
    int iters = 0;
    float X[16];
    symmicp_sums last{};
    // stats
    int timing = 0;                  // 0 off, 1 two events per pass, 2 events around every kernel of a pass
    // timing mode: 6 events per pass in a ring of kEvRing passes, resolved lazily (no sync inside the loop)
    static constexpr int kEvRing = 64, kEvPer = 8;      // per pass: 0..4 the kernels, 5 the reduce, 6..7 around the collective (sharded runs)
    hipEvent_t ev[kEvRing * kEvPer] = {};
    int ev_split[kEvRing] = {};      // 1 = split TREE pass (5 kernels), 0 = single pass kernel
    int ev_weight[kEvRing] = {};     // passes this entry stands for (timing mode 3 samples the passes of a device-driven run)
    int ev_coll[kEvRing] = {};       // 1: events 6 and 7 bracket this pass's all-reduce
    int ev_used = 0;
    symmicp_stats st{};
    // host-side timing of the pass loop, printed by symmicp_destroy under SYMMICP_DEBUG_HOST
    double t_launch = 0, t_spin = 0, t_between = 0, t_last_done = 0;
    long n_pass_timed = 0;
};

// device buffer freed on every exit path.  alloc(): its own hipMalloc (release() hands the pointer to the context);
// alloc_temp(): from the context's arena when it fits (nothing to free), else its own hipMalloc.
template <typename T>
struct DevBuf {
    T *p = nullptr;
    bool owned = true;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { if (p && owned) hipFree(p); }
    hipError_t alloc(size_t count) { owned = true; return hipMalloc((void **)&p, sizeof(T) * (count ? count : 1)); }
    hipError_t alloc_temp(Arena &a, size_t count)
    {
        const size_t bytes = ((sizeof(T) * (count ? count : 1)) + 255) & ~(size_t)255;
        if (a.base && a.off + bytes <= a.cap) { p = reinterpret_cast<T *>(a.base + a.off); a.off += bytes; owned = false; return hipSuccess; }
        return alloc(count);
    }
    T *release() { T *q = p; p = nullptr; return q; }           // (owned buffers only)
};

// a context-owned device array that only grows: at least `want` elements afterwards, contents dead
template <typename T>
inline hipError_t grow(T *&p, size_t &cap, size_t want)
{
    if (cap >= want) return hipSuccess;
    hipFree(p);
    p = nullptr; cap = 0;
    const hipError_t e = hipMalloc((void **)&p, sizeof(T) * want);
    if (e == hipSuccess) cap = want;
    return e;
}

// rewind the arena and make sure it holds `want` bytes (contents are dead: called at the start of a public call)
void arena_begin(Arena &a, size_t want);

#define HIP_TRY(ctx, call)                                                                                  \
    do {                                                                                                    \
        hipError_t e__ = (call);                                                                            \
        if (e__ != hipSuccess) {                                                                            \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                                \
            return SYMMICP_ERR_HIP;                                                                         \
        }                                                                                                   \
    } while (0)



inline int fail(symmicp_ctx *c, int code, const std::string &msg)
{
    if (c) c->err = msg;
    return code;
}

inline void soa_from_block(float *block, size_t n, CloudSoA &s)
{
    s.x = block; s.y = block + n; s.z = block + 2 * n; s.nx = block + 3 * n; s.ny = block + 4 * n; s.nz = block + 5 * n;
}

// a float from its order-preserving uint32 key (launch_bbox, the Morton frame)
inline float ord2f(uint32_t o)
{
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
}

inline void identity16(float X[16])
{
    for (int k = 0; k < 16; k++) X[k] = (k % 5 == 0) ? 1.f : 0.f;
}

// the pass-time questions about the rejectors, for the loop, the exchange and the configuration alike
inline bool pass_claims(const symmicp_ctx *c) { return c->rej.claims(c->cfg.corr); }
inline bool pass_reciprocal(const symmicp_ctx *c) { return c->rej.checks_back(c->cfg.corr); }
inline bool pass_rejects(const symmicp_ctx *c) { return c->rej.rejects(c->cfg.corr); }

inline int resolved_apply(const symmicp_config &c)
{
    if (c.apply == SYMMICP_APPLY_INCREMENTAL || c.apply == SYMMICP_APPLY_CUMULATIVE) return c.apply;
    return c.mode == SYMMICP_MODE_QUIRKS ? SYMMICP_APPLY_INCREMENTAL : SYMMICP_APPLY_CUMULATIVE;
}


// engine.cpp
void free_target(symmicp_ctx *c);
void forget_source(symmicp_ctx *c);
void flush_events(symmicp_ctx *c);
// engine_index.cpp
// the octree over cl (n points, a planar cloud in device memory) into ri's own store, its tq relabelled through labels (device, [n];
// null: the row).  Rewinds the context's scratch arena.  On failure ri is dropped.
int build_reverse_index(symmicp_ctx *c, const CloudSoA &cl, uint32_t n, const uint32_t *labels, ReverseIndex &ri);
// What a one-shot search allocates for itself: a reverse index and one device block.  Kernels on the stream may still use both when an
// error path leaves: the destructor synchronises the stream, then frees them.
struct OwnSearch {
    symmicp_ctx *c;
    char *d = nullptr;
    ReverseIndex ri;
    explicit OwnSearch(symmicp_ctx *ctx) : c(ctx) {}
    ~OwnSearch() { (void)hipStreamSynchronize(c->stream); ri.store.release(); if (d) (void)hipFree(d); }
};
// host strided cloud -> device block of 6 planar arrays, from `store` or (null) from the scratch arena; nrm null: zero normals;
// centroid: null, or the fp64 mean of xyz in row order.  (This and build_index are hidden, so the library's dynamic symbols stay what they were.)
__attribute__((visibility("hidden")))
int upload_planar(symmicp_ctx *c, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n, DevBuf<float> &block,
                  IndexStore *store, double centroid[3]);
// the index over cl (n points, planar, device memory) into rq.tq / rq.tn and what it allocates from `store`.  Of the context it uses the stream,
// the scratch arena (not rewound), the grid-tuning switches and the error string, and writes nothing else.
__attribute__((visibility("hidden")))
int build_index(symmicp_ctx *c, IndexStore &store, const CloudSoA &cl, uint32_t n, const IndexRequest &rq, BuiltIndex *out);
// Morton order of a planar cloud, temporaries and result from the context's scratch arena: vals[n] = sorted position -> row (keys_out:
// null, or it keeps the sorted keys); origin / h0_out: the Morton frame.  SYMMICP_ERR_ARG for non-finite coordinates.
int morton_order(symmicp_ctx *c, const CloudSoA &cl, uint32_t n, DevBuf<uint32_t> &vals, DevBuf<uint32_t> *keys_out, float origin[3], float *h0_out);
// The scratch index of a cloud operation: the caller's cloud uploaded and a box tree built over its Morton order, behind the target's arrays
// in the target's store; the destructor gives all of it back (stream sync, then the store rewound to the mark), on every exit.
// Declare it BEFORE the DevBufs that work on its index: they have to be destroyed before this destructor syncs and rewinds.
struct ScratchIndex {
    TargetIndex ix{};
    ScratchIndex() = default;
    ScratchIndex(const ScratchIndex &) = delete;
    ScratchIndex &operator=(const ScratchIndex &) = delete;
    ~ScratchIndex();
    // nrm may be NULL (zero normals).  temp_bytes: what the caller will take from the arena afterwards.
    int begin(symmicp_ctx *ctx, const float *xyz, size_t xr, size_t xc, const float *nrm, size_t nr, size_t nc, size_t n, size_t temp_bytes);

private:
    symmicp_ctx *c = nullptr;      // set once the mark is taken
    IndexStore::Mark mark;
};
// A one-shot entry: f(c) on a default context of its own on `device`, destroyed again.  The entry checks its arguments first, so that a
// bad call returns SYMMICP_ERR_ARG without touching the device.
template <class F>
inline int with_own_context(int device, F &&f)
{
    symmicp_config cfg;
    symmicp_config_default(&cfg);
    cfg.device = device;
    symmicp_ctx *c = nullptr;
    int st = symmicp_create(&cfg, &c);
    if (st != SYMMICP_OK) return st;
    st = f(c);
    symmicp_destroy(c);
    return st;
}
// engine_ndt.cpp
inline bool ndt_mode(const symmicp_ctx *c) { return c->cfg.mode == SYMMICP_MODE_NDT; }
// what keeps a configuration out of NDT (null: nothing): min_normal_dot and the incremental apply; and what keeps a context out of it
const char *ndt_config_refusal(const symmicp_config &cfg);
const char *ndt_context_refusal(const symmicp_ctx *c);
// the map over the context's planar target (c->tgt, c->n_t) into c->ndt.map; rewinds the scratch arena
int ndt_build_target_map(symmicp_ctx *c);
// the arguments of a pass (or of the correspondence read-back) at the cumulative transform X
void ndt_pass_args(const symmicp_ctx *c, const float X[16], NdtPassArgs &a);
// engine_exchange.cpp
void shm_close(symmicp_ctx *c);
int shm_exchange(symmicp_ctx *c, double *rec);      // rec[40]: this rank's record in, the sum over ranks out
// engine_debug.cpp
void dump_packet_trace(symmicp_ctx *c);
void print_pass_counters(symmicp_ctx *c, bool first, long long list_len);
// SYMMICP_DEBUG_HOST: what a device-driven run (passes it0 + 1 .. it1 of `want`, `enq` enqueued) did; pass_kernel: by iteration % kRing,
// 1 = the certified-only kernel; before: the feedback of the host pass in front of the run
void print_batch_summary(const symmicp_ctx *c, int it0, int it1, int want, int enq, int n_stage, const uint8_t *pass_kernel, const PassFeedback &before);
// the record of iteration k in the ring of a device-driven run
inline int ring_slot(int k) { return k % symmicp_ctx::kRing; }
inline LoopRecord &ring_at(const symmicp_ctx *c, int k) { return c->h_ring[ring_slot(k)]; }
