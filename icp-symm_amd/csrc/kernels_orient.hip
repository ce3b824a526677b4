// kernels_orient.hip -- consistent normal orientation on gfx950 (symmicp_ctx_orient_normals; include/symmicp.h defines the result,
// DESIGN.md 4 "Normal orientation" has the reasoning; tests/_orient_ref.py restates it in numpy): the minimum spanning forest of
// the symmetrised k-NN graph by Boruvka rounds, the sign carried along as a parity (orient_core.h).
//
//   k_orient_edges     once: the lists of launch_knn ([n][k] by caller row) transposed to [k][n] (lane i reads entry j of row i at
//                      j * n + i: coalesced in every round), the row itself and empty slots replaced by i (a self-loop, skipped by
//                      every round because its ends share a root), the weight word of every edge beside it, and |E| counted (an
//                      edge listed from both ends counts at its lower end).
//   a round            every component is FLAT at its start (words[i] = (root, parity of i against the root)):
//     k_orient_min_key   per row, every listed edge whose ends have different roots: 64-bit minimum of (w bits << 32 | lo) into the
//                        slot of EITHER root.  A plain load first, the atomic only when the key can win (a stale load is only ever
//                        too high: the skip is safe); the key for the row's own root is reduced across the wave first when every
//                        lane of it offers to the same root -- the late rounds, where a few components hold everything.
//     k_orient_min_hi    the same edges again: among those whose key is the slot's minimum, the 32-bit minimum of hi.
//     k_orient_hook      one thread per row, from words_in to words_mid (two buffers: no thread reads what another writes in this
//                        launch): a root that chose an edge writes its hook word unless orient::hook_writes says the other root does;
//                        the edge goes to the tree list through the counter (one add per wave), which is also the count of hooks.
//     k_orient_flatten   from words_mid back to words: every row walks up at most hooks + 1 links (orient::walk_up; more raises *err).
//   The host reads the counter once per round and stops at a round without hooks.
//   k_orient_seed_key  per row: the component's lowest row (32-bit minimum) and its seed (64-bit minimum of an order-preserving key
//                      over the row) into the root's slots, with the same load-first rule, both reduced across the wave first (a
//                      per-lane offer of a million rows to one component's slot cost 3.4 ms at 1M points; DESIGN.md has it).
//   k_orient_root_flip per root: the seed's flip test, composed with the seed's parity = the flip of a row whose parity is 0.
//   k_orient_apply     per row: flip = parity ^ root flip; the sign-only write of nrm_out, flip_out, component_out.
// No loop in these kernels waits for another thread: a list of k entries, a walk of bounded length, a wave reduction of six steps.
#include "symmicp_internal.h"
#pragma clang fp contract(off)
#include "orient_core.h"

namespace symmicp {

constexpr int kOrientThreads = 256;

namespace {

__device__ __forceinline__ void offer64(unsigned long long *p, unsigned long long key)
{
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

__device__ __forceinline__ void offer32(uint32_t *p, uint32_t key)
{
    if (key < __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(p, key);
}

// every lane of the wave calls this (key == kNoKey: nothing to offer): one atomic for the wave when all offers go to one root
__device__ __forceinline__ void wave_offer64(unsigned long long *slots, uint32_t root, unsigned long long key)
{
    const bool has = key != orient::kNoKey;
    const unsigned long long mask = __ballot(has);
    if (mask == 0ull) return;
    const int leader = __ffsll((long long)mask) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)root, leader);
    if (__all(!has || root == r0)) {
        unsigned long long m = key;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(m, off);
            m = o < m ? o : m;
        }
        if ((int)__lane_id() == leader) offer64(slots + r0, m);
    } else if (has) {
        offer64(slots + root, key);
    }
}

// the same for a 32-bit minimum (key == kNoRow: nothing to offer)
__device__ __forceinline__ void wave_offer32(uint32_t *slots, uint32_t root, uint32_t key)
{
    const bool has = key != orient::kNoRow;
    const unsigned long long mask = __ballot(has);
    if (mask == 0ull) return;
    const int leader = __ffsll((long long)mask) - 1;
    const uint32_t r0 = (uint32_t)__shfl((int)root, leader);
    if (__all(!has || root == r0)) {
        uint32_t m = key;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = (uint32_t)__shfl_xor((int)m, off);
            m = o < m ? o : m;
        }
        if ((int)__lane_id() == leader) offer32(slots + r0, m);
    } else if (has) {
        offer32(slots + root, key);
    }
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

}  // namespace

__global__ __launch_bounds__(kOrientThreads) void k_orient_edges(const int32_t *__restrict__ knn_rows, const float *__restrict__ nrm3, uint32_t n, int k,
                                                                 uint32_t *__restrict__ erow, uint32_t *__restrict__ eww,
                                                                 unsigned long long *edge_count)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long mine = 0;
    if (i < n) {
        const float nx = nrm3[3 * (size_t)i], ny = nrm3[3 * (size_t)i + 1], nz = nrm3[3 * (size_t)i + 2];
        for (int j = 0; j < k; j++) {
            const uint32_t r = (uint32_t)knn_rows[(size_t)i * k + j];
            uint32_t row = i, ww = 0;
            if (r != i && r < n) {
                row = r;
                ww = orient::weight_word(nx, ny, nz, nrm3[3 * (size_t)r], nrm3[3 * (size_t)r + 1], nrm3[3 * (size_t)r + 2]);
                bool counted_there = false;      // r < i and r lists i: the edge counts at r
                if (r < i)
                    for (int t = 0; t < k; t++) counted_there |= (uint32_t)knn_rows[(size_t)r * k + t] == i;
                mine += counted_there ? 0 : 1;
            }
            erow[(size_t)j * n + i] = row;
            eww[(size_t)j * n + i] = ww;
        }
    }
    mine = wave_sum(mine);
    if (__lane_id() == 0 && mine) atomicAdd(edge_count, mine);
}

__global__ __launch_bounds__(kOrientThreads) void k_orient_init(uint32_t *words, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) words[i] = orient::pack(i, 0);
}

__global__ __launch_bounds__(kOrientThreads) void k_orient_min_key(const uint32_t *__restrict__ erow, const uint32_t *__restrict__ eww,
                                                                   const uint32_t *__restrict__ words, uint32_t n, int k, unsigned long long *best)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long own = orient::kNoKey;
    uint32_t ri = 0;
    if (i < n) {
        ri = orient::parent_of(words[i]);
        for (int j = 0; j < k; j++) {
            const uint32_t r = erow[(size_t)j * n + i];
            if (r == i) continue;
            const uint32_t rj = orient::parent_of(words[r]);
            if (rj == ri) continue;
            const unsigned long long key = orient::key64(eww[(size_t)j * n + i], i < r ? i : r);
            own = key < own ? key : own;
            offer64(best + rj, key);
        }
    }
    wave_offer64(best, ri, own);
}

__global__ __launch_bounds__(kOrientThreads) void k_orient_min_hi(const uint32_t *__restrict__ erow, const uint32_t *__restrict__ eww,
                                                                  const uint32_t *__restrict__ words, uint32_t n, int k,
                                                                  const unsigned long long *__restrict__ best, uint32_t *best_hi)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t ri = orient::parent_of(words[i]);
    const unsigned long long best_i = best[ri];
    for (int j = 0; j < k; j++) {
        const uint32_t r = erow[(size_t)j * n + i];
        if (r == i) continue;
        const uint32_t rj = orient::parent_of(words[r]);
        if (rj == ri) continue;
        const unsigned long long key = orient::key64(eww[(size_t)j * n + i], i < r ? i : r);
        const uint32_t hi = i < r ? r : i;
        if (key == best_i) offer32(best_hi + ri, hi);
        if (key == best[rj]) offer32(best_hi + rj, hi);
    }
}

// tree [n - 1][2]; counter: the hooks so far = the tree edges so far
__global__ __launch_bounds__(kOrientThreads) void k_orient_hook(const uint32_t *__restrict__ words_in, uint32_t *__restrict__ words_mid, uint32_t n,
                                                                const unsigned long long *__restrict__ best, const uint32_t *__restrict__ best_hi,
                                                                const float *__restrict__ nrm3, int32_t *__restrict__ tree, uint32_t *counter)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t out = 0, lo = 0, hi = 0;
    bool hooks = false;
    if (a < n) {
        out = words_in[a];
        const unsigned long long key = best[a];
        if (orient::parent_of(out) == a && key != orient::kNoKey) {
            lo = (uint32_t)(key & 0xffffffffull);
            hi = best_hi[a];
            if (lo < n && hi < n) {      // (always: the slots hold rows of listed edges)
                const uint32_t word_lo = words_in[lo], word_hi = words_in[hi];
                const bool lo_mine = orient::parent_of(word_lo) == a;
                const uint32_t word_u = lo_mine ? word_lo : word_hi, word_v = lo_mine ? word_hi : word_lo;
                const uint32_t b = orient::parent_of(word_v);
                if (b < n && orient::hook_writes(a, b, best[b] == key && best_hi[b] == hi)) {
                    const uint32_t ww = orient::weight_word(nrm3[3 * (size_t)lo], nrm3[3 * (size_t)lo + 1], nrm3[3 * (size_t)lo + 2],
                                                            nrm3[3 * (size_t)hi], nrm3[3 * (size_t)hi + 1], nrm3[3 * (size_t)hi + 2]);
                    out = orient::hook_word(word_u, word_v, ww);
                    hooks = true;
                }
            }
        }
        words_mid[a] = out;
    }
    // one add to the counter per wave (every lane is here): the first hooking lane takes the wave's slots, each lane its rank among them
    const unsigned long long mask = __ballot(hooks);
    if (mask == 0ull) return;
    const int leader = __ffsll((long long)mask) - 1;
    uint32_t base = 0;
    if ((int)__lane_id() == leader) base = atomicAdd(counter, (uint32_t)__popcll(mask));
    base = (uint32_t)__shfl((int)base, leader);
    if (hooks) {
        const uint32_t slot = base + (uint32_t)__popcll(mask & ((1ull << __lane_id()) - 1ull));
        if (slot + 1 < n) { tree[2 * (size_t)slot] = (int32_t)lo; tree[2 * (size_t)slot + 1] = (int32_t)hi; }
    }
}

__global__ __launch_bounds__(kOrientThreads) void k_orient_flatten(const uint32_t *__restrict__ words_mid, uint32_t *__restrict__ words, uint32_t n,
                                                                   uint32_t bound, uint32_t *err)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t w;
    if (!orient::walk_up(words_mid, i, bound, &w)) atomicOr(err, 1u);
    words[i] = w;
}

// rule 0: viewpoint (the smallest d2 to ref), rule 1: direction (the largest projection on ref); ties to the lowest row
__global__ __launch_bounds__(kOrientThreads) void k_orient_seed_key(const uint32_t *__restrict__ words, const float *__restrict__ xyz3, uint32_t n,
                                                                    int rule, float ax, float ay, float az, uint32_t *min_row,
                                                                    unsigned long long *seed_key)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = orient::kNoKey;
    uint32_t root = 0;
    if (i < n) {
        root = orient::parent_of(words[i]);
        const float x = xyz3[3 * (size_t)i], y = xyz3[3 * (size_t)i + 1], z = xyz3[3 * (size_t)i + 2];
        uint32_t hi;
        if (rule == 0) {
            const float dx = x - ax, dy = y - ay, dz = z - az;
            hi = orient::bits_of((dx * dx + dy * dy) + dz * dz);      // >= 0: its bits order it
        } else {
            float p = ((x * ax + y * ay) + z * az) + 0.0f;               // (-0 -> +0)
            if (!(p == p)) p = __int_as_float((int)0xff800000);        // an overflow of both signs: never the largest
            hi = ~orient::ordered_bits(p);
        }
        key = ((unsigned long long)hi << 32) | (unsigned long long)i;
    }
    wave_offer32(min_row, root, i < n ? i : orient::kNoRow);
    wave_offer64(seed_key, root, key);
}

__global__ __launch_bounds__(kOrientThreads) void k_orient_root_flip(const uint32_t *__restrict__ words, const float *__restrict__ xyz3,
                                                                     const float *__restrict__ nrm3, uint32_t n, int rule, float ax, float ay, float az,
                                                                     const unsigned long long *__restrict__ seed_key, uint32_t *__restrict__ root_flip)
{
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= n || orient::parent_of(words[a]) != a) return;
    const uint32_t seed = (uint32_t)(seed_key[a] & 0xffffffffull);
    if (seed >= n) { root_flip[a] = 0; return; }      // (cannot happen: the root itself offered a key)
    const float nx = nrm3[3 * (size_t)seed], ny = nrm3[3 * (size_t)seed + 1], nz = nrm3[3 * (size_t)seed + 2];
    bool flip;
    if (rule == 0) {
        // the flip test of k_normals_knn (flipNormalTowardsViewpoint), in fp64 from the fp32 values
        const double px = (double)xyz3[3 * (size_t)seed], py = (double)xyz3[3 * (size_t)seed + 1], pz = (double)xyz3[3 * (size_t)seed + 2];
        const double dot = ((double)ax - px) * (double)nx + ((double)ay - py) * (double)ny + ((double)az - pz) * (double)nz;
        flip = dot < 0;
    } else {
        flip = ((nx * ax + ny * ay) + nz * az) < 0.0f;
    }
    root_flip[a] = orient::parity_of(words[seed]) ^ (flip ? 1u : 0u);
}

__global__ __launch_bounds__(kOrientThreads) void k_orient_apply(const uint32_t *__restrict__ words, const uint32_t *__restrict__ root_flip,
                                                                 const uint32_t *__restrict__ min_row, const float *__restrict__ nrm3, uint32_t n,
                                                                 float *__restrict__ nrm_out, uint8_t *__restrict__ flip_out,
                                                                 int32_t *__restrict__ component_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t w = words[i], root = orient::parent_of(w);
    const uint32_t flip = root < n ? orient::parity_of(w) ^ (root_flip[root] & 1u) : 0u;
    const uint32_t sign = flip ? orient::kSignBit : 0u;
#pragma unroll
    for (int a = 0; a < 3; a++)
        nrm_out[3 * (size_t)i + a] = __uint_as_float(__float_as_uint(nrm3[3 * (size_t)i + a]) ^ sign);
    flip_out[i] = (uint8_t)flip;
    component_out[i] = root < n ? (int32_t)min_row[root] : -1;
}

static dim3 orient_grid(uint32_t n) { return dim3((n + kOrientThreads - 1) / kOrientThreads); }

void launch_orient_edges(const int32_t *knn_rows, const float *nrm3, uint32_t n, int k, uint32_t *erow, uint32_t *eww, unsigned long long *edge_count,
                         uint32_t *words, hipStream_t s)
{
    hipLaunchKernelGGL(k_orient_edges, orient_grid(n), dim3(kOrientThreads), 0, s, knn_rows, nrm3, n, k, erow, eww, edge_count);
    hipLaunchKernelGGL(k_orient_init, orient_grid(n), dim3(kOrientThreads), 0, s, words, n);
}

void launch_orient_round(const uint32_t *erow, const uint32_t *eww, const uint32_t *words, uint32_t *words_mid, uint32_t n, int k,
                         unsigned long long *best, uint32_t *best_hi, const float *nrm3, int32_t *tree, uint32_t *counter, hipStream_t s)
{
    (void)hipMemsetAsync(best, 0xff, sizeof(unsigned long long) * n, s);
    (void)hipMemsetAsync(best_hi, 0xff, sizeof(uint32_t) * n, s);
    hipLaunchKernelGGL(k_orient_min_key, orient_grid(n), dim3(kOrientThreads), 0, s, erow, eww, words, n, k, best);
    hipLaunchKernelGGL(k_orient_min_hi, orient_grid(n), dim3(kOrientThreads), 0, s, erow, eww, words, n, k, best, best_hi);
    hipLaunchKernelGGL(k_orient_hook, orient_grid(n), dim3(kOrientThreads), 0, s, words, words_mid, n, best, best_hi, nrm3, tree, counter);
}

void launch_orient_flatten(const uint32_t *words_mid, uint32_t *words, uint32_t n, uint32_t bound, uint32_t *err, hipStream_t s)
{
    hipLaunchKernelGGL(k_orient_flatten, orient_grid(n), dim3(kOrientThreads), 0, s, words_mid, words, n, bound, err);
}

void launch_orient_finish(const uint32_t *words, const float *xyz3, const float *nrm3, uint32_t n, int rule, const float ref[3], uint32_t *min_row,
                          unsigned long long *seed_key, uint32_t *root_flip, float *nrm_out, uint8_t *flip_out, int32_t *component_out, hipStream_t s)
{
    (void)hipMemsetAsync(seed_key, 0xff, sizeof(unsigned long long) * n, s);
    (void)hipMemsetAsync(min_row, 0xff, sizeof(uint32_t) * n, s);
    hipLaunchKernelGGL(k_orient_seed_key, orient_grid(n), dim3(kOrientThreads), 0, s, words, xyz3, n, rule, ref[0], ref[1], ref[2], min_row, seed_key);
    hipLaunchKernelGGL(k_orient_root_flip, orient_grid(n), dim3(kOrientThreads), 0, s, words, xyz3, nrm3, n, rule, ref[0], ref[1], ref[2], seed_key,
                       root_flip);
    hipLaunchKernelGGL(k_orient_apply, orient_grid(n), dim3(kOrientThreads), 0, s, words, root_flip, min_row, nrm3, n, nrm_out, flip_out, component_out);
}

}  // namespace symmicp
