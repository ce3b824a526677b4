// kernels_search.hip -- the correspondence search kernels of the symmetric-ICP loop for gfx950, and the distance read-backs.
//
// The nearest-neighbour pass (SYMMICP_CORR_TREE) is three kernels plus the final reduce:
//   k_search_cells  thread = query: pair certificate / cell scan / two-round cell probe (cells_tile, pair_search.h); what it cannot
//                   finish goes to a work list (64-shard append list)
//   k_search_walk   the work list: one thread per entry on the sparse octree (long lists: the first pass), or one
//                   wave per entry on the run tree (short lists: stragglers).  Not launched after a pass whose list
//                   was empty; the host repairs the pass if the list turns out non-empty (engine.cpp, run_pass)
//   k_accumulate    streaming: rows + 37 fp64 sums from the stored pairs (and the optional write-back): kernels_pass.hip
// Blocks are dealt to XCDs round-robin, so block b is remapped to a contiguous chunk of the Morton-sorted source
// per XCD: each XCD's 4 MB L2 then serves one compact region of the target.
// Also here: k_nn_brute (SYMMICP_CORR_BRUTE), and k_identity_d2 / k_pairs_d2, the pairs' distances on request.
//
// fp32 expressions here must stay UNFUSED (compiled with -ffp-contract=off) and
// keep the association written: the CPU oracle uses the same expressions, so
// nearest-neighbour choices compare bit for bit.
#include "symmicp_internal.h"
#include "device_common.h"
#include "oct_walk.h"
#include "pair_search.h"
#pragma clang fp contract(off)

namespace symmicp {

template <bool HOOD>
__global__ __launch_bounds__(kPassThreads) void k_search_cells(PassArgs a, TargetIndex ix, WorkLists wl, uint32_t chunk, uint32_t qshift)
{
    // (tiles dealt to the XCDs in chunks of kCellsChunk: the regions of a cloud differ in cost, see xcd_remap_chunked; tiles past the end idle)
    // A tile is 1 << qshift queries (256, 128 or 64) scanned by all 256 threads.  A workgroup lives as long as its chain of scan rounds
    // (256 items each: three dependent gathers and a barrier): a share of 125 k queries (1M points over 8 ranks) is 488 tiles of 256 --
    // under two per CU, and the launch lasts one workgroup's 15 rounds; tiles of 64 are four times as many workgroups of 4 rounds each.
    const uint32_t tile = xcd_remap_chunked(blockIdx.x, chunk);
    const uint32_t i = threadIdx.x < (1u << qshift) ? (tile << qshift) + threadIdx.x : 0xFFFFFFFFu;
    cells_tile<HOOD>(a, ix, wl, a.X, i, tile & (kShards - 1), false);      // (the shard follows the tile: the lists' capacity assumes an even spread)
}

// ---------------------------------------------------------------------------
// Stragglers.  In a converged pass only a few thousand queries are left on the work list (source
// points outside the overlap: far from the target, but with a TIGHT bound from their previous pair).
// One thread per query would serialise ~100 dependent loads each (hundreds of microseconds for a
// handful of waves), so when the list is short each query gets a whole WAVE: a level-synchronous
// branch-and-bound over the same box tree.  The frontier of one level lives in LDS; a batch of 8
// frontier nodes x 8 children is tested by the 64 lanes at once; survivors are compacted with
// __ballot + popcount.  The pruning radius is min(best real candidate, smallest max-distance of any
// box seen) -- a non-empty box guarantees a point within its farthest corner.  Leaves: 8 leaves x 8
// points per batch, wave-wide argmin on (d2 bits << 32 | row).  If a frontier outgrows its LDS slot
// lane 0 finishes the query with the per-thread octree walk instead (exact either way).
// ---------------------------------------------------------------------------
constexpr int kWaveFrontier = 512;        // frontier nodes per level in the wave-per-entry walk

__device__ __forceinline__ float boxmaxdist2(float px, float py, float pz, const float4 &lo, const float4 &hi)
{
    float dx = fmaxf(fabsf(px - lo.x), fabsf(px - hi.x));
    float dy = fmaxf(fabsf(py - lo.y), fabsf(py - hi.y));
    float dz = fmaxf(fabsf(pz - lo.z), fabsf(pz - hi.z));
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        unsigned long long o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float wave_min_f32(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off, 64));
    return v;
}

// k_search_walk: ONE launch for both regimes of the work list (single-wave blocks: walk lengths differ several-fold
// between regions, and single-wave blocks let the dispatcher backfill CUs at wave granularity).
//   long list  (first pass: every query)      -> one THREAD per entry, near-first walk of the sparse octree
//   short list (stragglers of later passes)   -> one WAVE per entry (the scheme described above), first 8192 blocks
constexpr int kWalkThreads = 64;
constexpr uint32_t kWaveWorkers = 8192;

// BUDGETED instantiation (sharded runs, first pass of a small share): `list` is the list to drain (the work list, or the
// retry list of the previous launch); in the one-thread-per-query regime a walk gets `budget` node visits, and what it
// has not settled by then goes to wl.retry with the best point seen so far as its bound, for a second launch in the
// wave-per-query regime.  Why: a wave is as slow as its slowest lane (471 visits against a mean of 81 on the 1M-point
// surface pair), and with ~100k queries per rank that tail is the whole kernel.
template <bool BUDGETED>
__global__ __launch_bounds__(kWalkThreads, 6) void k_search_walk(PassArgs a, TargetIndex ix, WorkLists wl, ShardList list, uint32_t kWaveModeMax,
                                                                 uint32_t budget)
{
    if (a.loop) {                                   // straggler stage of a device-driven loop
        if (a.loop->stop) return;
        a.X = a.loop->Xapply;
    }
    __shared__ uint32_t fr[1][2][kWaveFrontier];
    __shared__ uint32_t pre[kShards + 1];
    sl_prefix(list, pre);
    const float inf = __int_as_float(0x7f800000);
    if (pre[kShards] > kWaveModeMax) {
        // ---- long list: one thread per entry (the launcher normally sizes the grid so that this loop runs once) ----
        for (uint32_t g = blockIdx.x * kWalkThreads + threadIdx.x; ; g += gridDim.x * kWalkThreads) {
            uint32_t i;
            if (!sl_locate(list, pre, g, i)) break;
            const float x = a.in.x[i], y = a.in.y[i], z = a.in.z[i];
            const float px = xf_row(a.X.m + 0, x, y, z, 1.0f), py = xf_row(a.X.m + 4, x, y, z, 1.0f), pz = xf_row(a.X.m + 8, x, y, z, 1.0f);
            Best b;
            b.pos = a.pos_out[i]; b.d2 = a.d2_out[i]; b.row = 0x7fffffff;
            if (b.pos >= 0) b.row = __float_as_int(ix.tq[b.pos].w);
            const uint32_t visits = oct_walk<BUDGETED>(ix, px, py, pz, b, budget);
            a.pos_out[i] = b.pos;
            a.d2_out[i] = b.d2;
            if (BUDGETED && visits > budget) sl_push(wl.retry, blockIdx.x & (kShards - 1), i);      // unfinished: the wave regime takes over
            if (ix.dbg) {
                uint32_t mx = visits;
                for (int off = 32; off > 0; off >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, off, 64));
                atomicAdd(ix.dbg + 4, (unsigned long long)visits);
                if ((threadIdx.x & 63) == 0) atomicAdd(ix.dbg + 5, (unsigned long long)mx * 64ull);
            }
        }
        return;
    }
    // ---- short list: one wave per entry ----
    if (blockIdx.x >= kWaveWorkers) return;
    const int lane = threadIdx.x, wave = 0;
    const uint32_t nwaves = min(gridDim.x, kWaveWorkers);
    for (uint32_t w = blockIdx.x; ; w += nwaves) {
        uint32_t i;
        if (!sl_locate(list, pre, w, i)) break;
        const float x = a.in.x[i], y = a.in.y[i], z = a.in.z[i];
        const float px = xf_row(a.X.m + 0, x, y, z, 1.0f), py = xf_row(a.X.m + 4, x, y, z, 1.0f), pz = xf_row(a.X.m + 8, x, y, z, 1.0f);
        // wave-uniform best: key = (d2 bits << 32 | row), plus the sorted position of that row
        int32_t bpos = a.pos_out[i];
        float bd2 = a.d2_out[i];
        unsigned long long bkey = ~0ull;
        if (bpos >= 0) bkey = ((unsigned long long)__float_as_uint(bd2) << 32) | (unsigned long long)(uint32_t)__float_as_int(ix.tq[bpos].w);
        else bd2 = inf;
        float radius2 = bd2;                    // pruning radius: never below the true nearest distance
        const float pad = kSlackFrac * ix.h;    // scan D beyond it, so the result carries a pair certificate (k_search_cells)
        bool overflowed = false;
        // top level: <= 8 nodes, lanes 0..7
        uint32_t nf = 0;
        {
            float mind = inf, maxd = inf;
            if (lane < (int)ix.ntop) {
                const float4 *bx = ix.boxes + 2 * ((size_t)ix.level_off[ix.top] + lane);
                const float4 lo = bx[0], hi = bx[1];
                if (lo.x <= hi.x) { mind = boxdist2(px, py, pz, lo, hi); maxd = boxmaxdist2(px, py, pz, lo, hi); }
            }
            radius2 = fminf(radius2, wave_min_f32(maxd));
            const float rp = __builtin_amdgcn_sqrtf(radius2) * 1.00001f + pad;
            const bool keep = mind <= rp * rp * 1.00001f && mind < inf;
            const unsigned long long m = __ballot(keep);
            if (keep) fr[wave][0][__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)lane;
            nf = (uint32_t)__popcll(m);
            __builtin_amdgcn_wave_barrier();
        }
        int cur = 0;
        for (int L = ix.top; L >= 1 && !overflowed; L--) {
            // expand the frontier of level L into level L-1
            uint32_t nn = 0;
            for (uint32_t f0 = 0; f0 < nf; f0 += 8) {
                const uint32_t f = f0 + (uint32_t)(lane >> 3);
                float mind = inf, maxd = inf;
                uint32_t child = 0;
                if (f < nf) {
                    child = (fr[wave][cur][f] << 3) + (uint32_t)(lane & 7);
                    const float4 *bx = ix.boxes + 2 * ((size_t)ix.level_off[L - 1] + child);
                    const float4 lo = bx[0], hi = bx[1];
                    if (lo.x <= hi.x) { mind = boxdist2(px, py, pz, lo, hi); maxd = boxmaxdist2(px, py, pz, lo, hi); }
                }
                radius2 = fminf(radius2, wave_min_f32(maxd));
                const float rp = __builtin_amdgcn_sqrtf(radius2) * 1.00001f + pad;
                const bool keep = mind <= rp * rp * 1.00001f && mind < inf;
                const unsigned long long m = __ballot(keep);
                const uint32_t slot = nn + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                if (keep && slot < (uint32_t)kWaveFrontier) fr[wave][cur ^ 1][slot] = child;
                nn += (uint32_t)__popcll(m);
            }
            if (nn > (uint32_t)kWaveFrontier) { overflowed = true; break; }
            nf = nn;
            cur ^= 1;
            __builtin_amdgcn_wave_barrier();
        }
        if (overflowed) {
            // a frontier outgrew its LDS slot (loose bound): lane 0 finishes this one with the per-thread octree walk
            if (lane == 0) {
                Best b;
                b.pos = bpos; b.d2 = bd2; b.row = (bkey == ~0ull) ? 0x7fffffff : (int32_t)(uint32_t)(bkey & 0xFFFFFFFFull);
                oct_walk(ix, px, py, pz, b);
                a.pos_out[i] = b.pos;
                a.d2_out[i] = b.d2;
            }
            continue;
        }
        // frontier = leaves: 8 leaves x 8 points per batch; keep the two smallest keys seen
        uint32_t second = 0x7f800000u;          // d2 bits of the nearest point that is not the winner
        for (uint32_t f0 = 0; f0 < nf; f0 += 8) {
            const uint32_t f = f0 + (uint32_t)(lane >> 3);
            unsigned long long key = ~0ull;
            uint32_t j = 0;
            if (f < nf) {
                j = fr[wave][cur][f] * kLeaf + (uint32_t)(lane & 7);
                if (j < ix.n) {
                    const float4 q = ix.tq[j];
                    const float d2 = dist2(px, py, pz, q.x, q.y, q.z);
                    if (d2 == d2) key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)__float_as_int(q.w);
                }
            }
            const unsigned long long best = wave_min_u64(key);
            const unsigned long long runner = wave_min_u64(key == best ? ~0ull : key);
            if (best < bkey) {
                second = min(second, min((uint32_t)(bkey >> 32), (uint32_t)(runner >> 32)));
                bkey = best;
                const unsigned long long who = __ballot(key == best);
                bpos = (int32_t)__shfl((int)j, __ffsll((long long)who) - 1, 64);
            } else if (best == bkey) {
                second = min(second, (uint32_t)(runner >> 32));           // the previous pair found again
            } else {
                second = min(second, (uint32_t)(best >> 32));
            }
        }
        if (lane == 0 && bkey != ~0ull) {
            // everything not scanned was pruned beyond (nearest + pad): same certificate as in k_search_cells
            const float d1 = sqrtf(__uint_as_float((uint32_t)(bkey >> 32)));
            const float L = fminf(sqrtf(__uint_as_float(second)) * 0.999999f, (d1 + pad) * 0.99999f);
            a.cert[i] = make_float4(px, py, pz, cert_word((L > d1 * 1.000001f) ? L : 0.0f, false));      // (an even word: no neighbourhood)
        }
        if (lane == 0) {
            a.pos_out[i] = bpos;
            a.d2_out[i] = (bkey == ~0ull) ? inf : __uint_as_float((uint32_t)(bkey >> 32));
        }
    }
}

// ---------------------------------------------------------------------------
// brute-force exact NN (SURVEY 8(a) k_nn_brute): target tiles of 1024 points staged in LDS,
// 4 queries per thread, every lane reads the same LDS address (broadcast, conflict-free).
// grid = (query blocks, target splits); splits are merged with a 64-bit atomicMin on
// (d2 bits << 32 | row): min is order independent, and equal d2 resolves to the lowest row.
// VALU-bound by design (N_s x N_t distance evaluations); used for small clouds and as the
// on-device cross-check of the tree search.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kPassThreads) void k_nn_brute(CloudSoA src, uint32_t n_s, Affine X,
                                                          const float4 *__restrict__ tq, uint32_t n_t,
                                                          uint32_t tiles_per_split, unsigned long long *best64)
{
    __shared__ float4 tile[kBruteTile];
    float px[kBruteQ], py[kBruteQ], pz[kBruteQ], bd[kBruteQ];
    uint32_t bj[kBruteQ];
    const uint32_t q0 = blockIdx.x * (kPassThreads * kBruteQ) + threadIdx.x;
#pragma unroll
    for (int k = 0; k < kBruteQ; k++) {
        uint32_t i = q0 + k * kPassThreads;
        float x = 0.f, y = 0.f, z = 0.f;
        if (i < n_s) { x = src.x[i]; y = src.y[i]; z = src.z[i]; }
        px[k] = xf_row(X.m + 0, x, y, z, 1.0f); py[k] = xf_row(X.m + 4, x, y, z, 1.0f); pz[k] = xf_row(X.m + 8, x, y, z, 1.0f);
        bd[k] = __int_as_float(0x7f800000); bj[k] = 0xFFFFFFFFu;
    }
    const uint32_t tile0 = blockIdx.y * tiles_per_split;
    const uint32_t ntiles = (n_t + kBruteTile - 1) / kBruteTile;
    const uint32_t tile1 = min(tile0 + tiles_per_split, ntiles);
    for (uint32_t t = tile0; t < tile1; t++) {
        const uint32_t base = t * kBruteTile;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < kBruteTile / kPassThreads; k++) {
            uint32_t j = base + k * kPassThreads + threadIdx.x;
            // out-of-range slots get a NaN coordinate: every comparison with them is false
            tile[k * kPassThreads + threadIdx.x] = (j < n_t) ? tq[j] : make_float4(__int_as_float(0x7fc00000), 0.f, 0.f, 0.f);
        }
        __syncthreads();
        // rows inside a tile ascend, tiles ascend -> strict '<' keeps the lowest row on ties
#pragma unroll 4
        for (int j = 0; j < kBruteTile; j++) {
            float4 q = tile[j];
#pragma unroll
            for (int k = 0; k < kBruteQ; k++) {
                float d2 = dist2(px[k], py[k], pz[k], q.x, q.y, q.z);
                if (d2 < bd[k]) { bd[k] = d2; bj[k] = base + j; }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kBruteQ; k++) {
        uint32_t i = q0 + k * kPassThreads;
        if (i < n_s && bj[k] != 0xFFFFFFFFu) {
            unsigned long long key = ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned long long)bj[k];
            atomicMin(best64 + i, key);
        }
    }
}

// per-pair squared distances of the identity pairing, on request (the streaming pass does not store them)
__global__ __launch_bounds__(256) void k_identity_d2(CloudSoA in, Affine X, CloudSoA tgt, uint32_t tgt_offset, uint32_t n, float *d2)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = in.x[i], y = in.y[i], z = in.z[i];
    const float px = xf_row(X.m + 0, x, y, z, 1.0f), py = xf_row(X.m + 4, x, y, z, 1.0f), pz = xf_row(X.m + 8, x, y, z, 1.0f);
    const uint32_t j = tgt_offset + i;
    d2[i] = dist2(px, py, pz, tgt.x[j], tgt.y[j], tgt.z[j]);
}

// TREE: the distance of every current pair, from the positions the last pass gave the queries.  The passes store a distance only where
// they searched; a certified pair keeps its target, and the expression below is the one every kernel evaluates for it (same operations,
// same order: the same bits).  No pair: +inf, as the searches store it.
__global__ __launch_bounds__(256) void k_pairs_d2(CloudSoA in, Affine X, const int32_t *__restrict__ pos, const float4 *__restrict__ tq, uint32_t n_t, uint32_t n, float *d2)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int32_t p = pos[i];
    float v = __int_as_float(0x7f800000);
    if (p >= 0 && (uint32_t)p < n_t) {
        const float x = in.x[i], y = in.y[i], z = in.z[i];
        const float px = xf_row(X.m + 0, x, y, z, 1.0f), py = xf_row(X.m + 4, x, y, z, 1.0f), pz = xf_row(X.m + 8, x, y, z, 1.0f);
        const float4 q = tq[p];
        v = dist2(px, py, pz, q.x, q.y, q.z);
    }
    d2[i] = v;
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_pairs_d2(const CloudSoA &in, const Affine &X, const int32_t *pos, const float4 *tq, uint32_t n_t, uint32_t n, float *d2, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_pairs_d2, dim3((n + 255) / 256), dim3(256), 0, s, in, X, pos, tq, n_t, n, d2);
}

void launch_identity_d2(const CloudSoA &in, const Affine &X, const CloudSoA &tgt, uint32_t tgt_offset, uint32_t n, float *d2, hipStream_t s)
{
    hipLaunchKernelGGL(k_identity_d2, dim3((n + 255) / 256), dim3(256), 0, s, in, X, tgt, tgt_offset, n, d2);
}

uint32_t shard_capacity(uint32_t n_points)
{
    // a shard only receives appends from producer blocks with (blockIdx & 63) == shard
    const uint32_t nb = (n_points + kPassThreads - 1) / kPassThreads;
    const uint32_t nbp = ((nb + 7u) / 8u) * 8u;
    return ((nbp + kShards - 1) / kShards) * kPassThreads;
}

uint32_t walk_blocks_full(const WorkLists &wl)
{
    return kShards * (wl.work.cap / kWalkThreads);      // one thread per possible list entry
}

// the cell search of a split pass (launch_pass_tree_split), as k_search_cells
void launch_search_cells(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const PassTuning &tune, hipStream_t s)
{
    const uint32_t nb = (a.n + kPassThreads - 1) / kPassThreads;
    const uint32_t chunk = tune.cells_chunk ? tune.cells_chunk : 16u;      // tiles per chunk
    // queries per tile: 256 while that fills the chip a few times over (256 CUs x 6-7 workgroups), else 128 or 64 (k_search_cells)
    uint32_t qshift = nb >= 3072u ? 8u : (nb >= 1536u ? 7u : 6u);
    if (tune.cells_queries == 64u) qshift = 6u; else if (tune.cells_queries == 128u) qshift = 7u; else if (tune.cells_queries == 256u) qshift = 8u;
    const uint32_t nq = (a.n + (1u << qshift) - 1u) >> qshift;
    const uint32_t nbc = ((nq + 8u * chunk - 1u) / (8u * chunk)) * (8u * chunk);
    if (a.make_hood) hipLaunchKernelGGL(k_search_cells<true>, dim3(nbc), dim3(kPassThreads), 0, s, a, ix, wl, chunk, qshift);
    else hipLaunchKernelGGL(k_search_cells<false>, dim3(nbc), dim3(kPassThreads), 0, s, a, ix, wl, chunk, qshift);
}

// the tree walk of a split pass: the work list, and with a.budget_walk the retry list behind it
void launch_search_walk(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, uint32_t walk_blocks, const PassTuning &tune, hipStream_t s)
{
    if (walk_blocks == 0 || walk_blocks > walk_blocks_full(wl)) walk_blocks = walk_blocks_full(wl);
    // first pass of an alignment: no query has a bound yet, which the wave-per-query walk needs (its frontier would
    // overflow and fall back to one lane): one thread per query whatever the list length (matters for shares or
    // clouds below the threshold, e.g. 1M points over 8 ranks)
    const uint32_t wmm = a.pos_prev ? tune.wave_mode_max : 0u;
    if (a.budget_walk) {
        const uint32_t budget = tune.walk_budget;
        hipLaunchKernelGGL(k_search_walk<true>, dim3(walk_blocks), dim3(kWalkThreads), 0, s, a, ix, wl, wl.work, wmm, budget);
        // the retry list: wave regime forced (every entry carries a bound now), no budget
        hipLaunchKernelGGL(k_search_walk<false>, dim3(8192), dim3(kWalkThreads), 0, s, a, ix, wl, wl.retry, 0xFFFFFFFFu, 0xFFFFFFFFu);
    } else {
        hipLaunchKernelGGL(k_search_walk<false>, dim3(walk_blocks), dim3(kWalkThreads), 0, s, a, ix, wl, wl.work, wmm, 0xFFFFFFFFu);
    }
}

// the walk of the device-driven loop's straggler stage (launch_loop_stragglers)
void launch_straggler_walk(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const PassTuning &tune, hipStream_t s)
{
    // (short lists: the wave-per-entry regime; anything above the threshold strides one thread per entry over this grid)
    hipLaunchKernelGGL(k_search_walk<false>, dim3(512), dim3(kWalkThreads), 0, s, a, ix, wl, wl.work, tune.wave_mode_max, 0xFFFFFFFFu);
}

void launch_nn_brute(const CloudSoA &src, uint32_t n_s, const Affine &X, const float4 *tq, uint32_t n_t,
                     unsigned long long *best64, hipStream_t s)
{
    const uint32_t qblocks = (n_s + kPassThreads * kBruteQ - 1) / (kPassThreads * kBruteQ);
    const uint32_t ntiles = (n_t + kBruteTile - 1) / kBruteTile;
    uint32_t splits = 1;
    if (qblocks < 2048) splits = (2048 + qblocks - 1) / qblocks;
    if (splits > ntiles) splits = ntiles;
    if (splits < 1) splits = 1;
    if (splits > 65535) splits = 65535;
    const uint32_t tiles_per_split = (ntiles + splits - 1) / splits;
    splits = (ntiles + tiles_per_split - 1) / tiles_per_split;
    hipMemsetAsync(best64, 0xFF, sizeof(unsigned long long) * (size_t)n_s, s);
    hipLaunchKernelGGL(k_nn_brute, dim3(qblocks, splits), dim3(kPassThreads), 0, s, src, n_s, X, tq, n_t, tiles_per_split, best64);
}

}  // namespace symmicp
