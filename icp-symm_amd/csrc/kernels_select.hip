// kernels_select.hip -- pair rejection by rank for gfx950 (trimmed ICP, symmicp_set_trim_fraction; one-to-one and median distance below):
// the keys of a pass's candidate pairs and the exact order statistic over them.
//
// A trimmed pass keeps the closest fraction rho of its candidate pairs (include/symmicp.h has the definition).  Between the search
// and the accumulating kernel of the pass run
//   k_reject_keys    per share row: the bits of the candidate's fp32 d2 -- non-negative floats order as their bit patterns -- or the
//                    sentinel 0xFFFFFFFF for a row without a pair or dropped by a gate; counts the candidates (n_c) and builds the
//                    histogram of the keys' first digit on the way
//   k_select_scan    one workgroup: k = ceil(rho n_c) in fp64 (first digit only), prefix sum over the digit's bins, the bin that
//                    holds rank k; fixes the digit, k becomes the rank inside that bin
//   k_select_hist    histogram of the next digit over the keys that match the digits fixed so far
// as keys, scan, hist, scan, hist, scan: an exact radix select over 32-bit keys in 11 + 11 + 10 bits.  Histograms are per-block in
// LDS (2048 bins, 8 KB), filled with wave-aggregated LDS atomics (the keys of a pass cluster: a handful of first digits hold them
// all) and merged into the global one with integer atomics: order-independent, so tau is reproducible bit for bit.  The last scan
// leaves tau, n_c and the kept count (keys <= tau, ties included) in device memory for the accumulating kernel and, as a RejectRecord, in
// host-mapped memory for the state getters.  Every step is launch-bound (4 B per row and digit), so there is no host round trip in between.
//
// The one-to-one and median-distance rejectors (symmicp_set_one_to_one / symmicp_set_median_factor) use the same keys and the same select:
//   k_unique_claim   in front of the keys: every candidate claims its target with (d2 bits << 32 | caller row) by a 64-bit atomicMin on a
//                    table of one word per target point; k_reject_keys<UNIQ> then gives every candidate that is not the minimum of its
//                    target the sentinel, so the select's population is the winners
//   k_median_tau     behind the select at rho = 0.5: tau = factor^2 x the median; k_count_le counts the keys <= tau, k_reject_publish
//                    hands the RejectRecord to the host; k_reject_all does both for one-to-one alone (every winner is kept)
// Reciprocal correspondences (symmicp_set_reciprocal) add one kernel between the claim and the keys:
//   k_recip_check    per claimed target j: q_j through the inverse of the pass's transform, one exact walk of the octree over the ORIGINAL
//                    source (oct_walk.h), and a winner that is not the reverse neighbour loses its claim (the entry goes back to ~0), so
//                    k_reject_keys<UNIQ> finds no winner there; counts the claimed targets (n_u) and the survivors (n_r)
// launch_reject has the order.
//
// The gates below are pair_step's (kernels_pass.hip), on the same fp32 expressions: unfused, in the association written.
#include "symmicp_internal.h"
#include "device_common.h"
#include "oct_walk.h"
#pragma clang fp contract(off)

namespace symmicp {

constexpr int kSelThreads = 256;
constexpr uint32_t kSelBins = 2048;           // bins of the widest digit (11 bits)
constexpr uint32_t kSelMaxBlocks = 1024;      // grid-stride beyond this
// workspace words (RejectArgs::ws): the state, then one histogram per digit
enum { SEL_NC = 0, SEL_K = 1, SEL_PREFIX = 2, SEL_TAU = 3, SEL_KEPT = 4, SEL_K0 = 5, SEL_GATED = 6, SEL_MED = 7, SEL_CLAIMED = 8, SEL_RECIP = 9, SEL_STATE_WORDS = 16 };
static_assert(kRejectWsWords == SEL_STATE_WORDS + 3 * kSelBins, "symmicp_internal.h sizes the workspace");
static_assert(kRejectTauWord == SEL_TAU, "the accumulating kernels read tau from this word");

// the pass's result for the host, from the workspace as the last step of the pass left it (out == null: a probe, or not the last step)
__device__ __forceinline__ void publish_record(const uint32_t *ws, RejectRecord *out)
{
    if (out) *out = RejectRecord{ws[SEL_NC], ws[SEL_KEPT], ws[SEL_TAU], ws[SEL_GATED], ws[SEL_CLAIMED], ws[SEL_RECIP]};
}

template <int PASS> __device__ __forceinline__ uint32_t sel_digit(uint32_t key)
{
    return PASS == 0 ? key >> 21 : (PASS == 1 ? (key >> 10) & 2047u : key & 1023u);
}
// the bits fixed before digit PASS
template <int PASS> __device__ __forceinline__ uint32_t sel_mask() { return PASS == 0 ? 0u : (PASS == 1 ? 0xFFE00000u : 0xFFFFFC00u); }

// One count per valid lane into the block's LDS histogram.  Lanes of a wave that hold the same digit add once: up to four rounds of
// (first live lane's digit, ballot, one atomic of the popcount), then whatever is left adds on its own -- clustered keys take one or
// two rounds, uniformly random ones fall through to plain LDS atomics.  `valid` may differ per lane; the call is wave-uniform.
__device__ __forceinline__ void hist_add(uint32_t *h, uint32_t digit, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long live = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < 4 && live; r++) {
        const int lead = __ffsll((long long)live) - 1;
        const uint32_t d = (uint32_t)__shfl((int)digit, lead, 64);
        const unsigned long long same = __ballot(valid && digit == d);
        if (lane == lead) atomicAdd(&h[d], (uint32_t)__popcll(same));
        if (digit == d) valid = false;
        live &= ~same;
    }
    if (valid) atomicAdd(&h[digit], 1u);
}

__device__ __forceinline__ void hist_zero(uint32_t *h)
{
    for (uint32_t b = threadIdx.x; b < kSelBins; b += kSelThreads) h[b] = 0u;
    __syncthreads();
}

__device__ __forceinline__ void hist_merge(const uint32_t *h, uint32_t *ghist)
{
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < kSelBins; b += kSelThreads) {
        const uint32_t v = h[b];
        if (v) atomicAdd(&ghist[b], v);
    }
}

// Candidate status of share row i -- a pair that exists and passes pair_step's gates -- with its d2 and the target position j the pass
// holds for it (IDENTITY: the target row; BRUTE: best64's low word; TREE: pos_out).  One source for the keys and for the one-to-one claim.
// CORR: 0 identity (target row = tgt_offset + i), 1 brute (best64), 2 tree (pos_out -> the target's pair record)
template <int CORR>
__device__ __forceinline__ bool pair_candidate(const PassArgs &a, const CloudSoA &tgt, const float4 *__restrict__ tn, bool gate_n, uint32_t i,
                                               float &d2, uint32_t &j)
{
    bool cand = false;
    d2 = 0.0f; j = 0u;
    const float x = a.in.x[i], y = a.in.y[i], z = a.in.z[i];
    const float px = xf_row(a.X.m + 0, x, y, z, 1.0f), py = xf_row(a.X.m + 4, x, y, z, 1.0f), pz = xf_row(a.X.m + 8, x, y, z, 1.0f);
    float nqx = 0.0f, nqy = 0.0f, nqz = 0.0f;
    if (CORR == 0) {
        j = a.tgt_offset + i;
        d2 = dist2(px, py, pz, tgt.x[j], tgt.y[j], tgt.z[j]);
        cand = true;
        if (gate_n) { nqx = tgt.nx[j]; nqy = tgt.ny[j]; nqz = tgt.nz[j]; }
    } else if (CORR == 1) {
        const unsigned long long b = a.best64[i];
        cand = b != ~0ull;
        d2 = __uint_as_float((uint32_t)(b >> 32));
        j = (uint32_t)(b & 0xFFFFFFFFull);
        if (cand && gate_n) { const float4 nq = tn[2 * (size_t)j + 1]; nqx = nq.x; nqy = nq.y; nqz = nq.z; }
    } else {
        const int32_t pos = a.pos_out[i];
        cand = pos >= 0;
        if (cand) {
            j = (uint32_t)pos;
            const float4 q = tn[2 * (size_t)pos];
            d2 = dist2(px, py, pz, q.x, q.y, q.z);
            if (gate_n) { const float4 nq = tn[2 * (size_t)pos + 1]; nqx = nq.x; nqy = nq.y; nqz = nq.z; }
        }
    }
    if (cand && a.max_d2 > 0.0f && d2 > a.max_d2) cand = false;
    if (cand && gate_n) {
        const float nx = a.in.nx[i], ny = a.in.ny[i], nz = a.in.nz[i];
        const float npx = xf_row(a.X.m + 0, nx, ny, nz, a.X.nrm_w), npy = xf_row(a.X.m + 4, nx, ny, nz, a.X.nrm_w),
                    npz = xf_row(a.X.m + 8, nx, ny, nz, a.X.nrm_w);
        if ((npx * nqx + npy * nqy) + npz * nqz < a.min_ndot) cand = false;
    }
    return cand;
}

// ---- one-to-one (symmicp_set_one_to_one) ---------------------------------------------------------
// Every candidate claims its target with K = (d2 bits << 32 | caller row); the table keeps the minimum.  An integer minimum does not
// depend on the order of the claims, so the winners are reproducible bit for bit; ties in d2 go to the lowest caller row.
__device__ __forceinline__ unsigned long long claim_key(uint32_t d2_bits, uint32_t row) { return ((unsigned long long)d2_bits << 32) | row; }
__device__ __forceinline__ uint32_t caller_row(const PassArgs &a, uint32_t i) { return a.rej.order ? a.rej.order[i] : i; }

// One claim.  A claim that the entry already beats cannot win -- the entry only falls -- so it is read first; a stale read costs one
// atomic more, never a winner.
__device__ __forceinline__ void claim(unsigned long long *table, uint32_t j, unsigned long long key)
{
    if (__hip_atomic_load(&table[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > key) atomicMin(&table[j], key);
}

// The claims of one wave.  Source points outside the overlap pair with the target's boundary, and neighbours in the share's Morton
// order pair with the same few boundary points: such a wave would send most of its 64 atomics to a handful of addresses, where they
// serialise.  So lanes that hold the same target combine first: up to eight rounds of (first live lane's target, ballot, minimum of the
// keys over those lanes, one claim).  A round whose leader is alone ends the rounds -- a wave inside the overlap, whose targets are
// mostly distinct, pays one round -- and whatever is left claims on its own.  `valid` may differ per lane; the call is wave-uniform.
__device__ __forceinline__ void claim_wave(unsigned long long *table, uint32_t j, unsigned long long key, bool valid)
{
    const int lane = threadIdx.x & 63;
    unsigned long long live = __ballot(valid);
#pragma unroll 1
    for (int r = 0; r < 8 && live; r++) {
        const int lead = __ffsll((long long)live) - 1;
        const uint32_t jl = (uint32_t)__shfl((int)j, lead, 64);
        const bool mine = valid && j == jl;
        const unsigned long long same = __ballot(mine);
        if (__popcll(same) == 1) break;
        unsigned long long v = mine ? key : ~0ull;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const unsigned long long o = __shfl_xor(v, off, 64);
            v = o < v ? o : v;
        }
        if (lane == lead) claim(table, jl, v);
        if (mine) valid = false;
        live &= ~same;
    }
    if (valid) claim(table, j, key);
}

template <int CORR>
__global__ __launch_bounds__(kSelThreads) void k_unique_claim(PassArgs a, CloudSoA tgt, const float4 *__restrict__ tn)
{
    const bool gate_n = a.min_ndot > -1.0f;
    const uint32_t stride = gridDim.x * kSelThreads;
    // (whole waves stay in the loop: claim_wave is wave-uniform)
    for (uint32_t base = blockIdx.x * kSelThreads; base < a.n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool cand = false;
        float d2 = 0.0f;
        uint32_t j = 0u;
        unsigned long long key = ~0ull;
        if (i < a.n) {
            cand = pair_candidate<CORR>(a, tgt, tn, gate_n, i, d2, j) && j < a.rej.n_t;
            if (cand) key = claim_key(__float_as_uint(d2), caller_row(a, i));
        }
        claim_wave(a.rej.table, j, key, cand);
    }
}

// ---- reciprocal correspondences (symmicp_set_reciprocal) -------------------------------------------
// back(j): target point q through the inverse of the pass's transform (fp32, unfused: xf_row with w = 1), then the exact walk of the
// source's octree.  Its tq carries the caller's row in w, so the walk's tie-break (lowest row) and Best::row speak the claim key's language.
__device__ __forceinline__ void reverse_nn(const TargetIndex &six, const Affine &inv, float qx, float qy, float qz, Best &b)
{
    const float yx = xf_row(inv.m + 0, qx, qy, qz, 1.0f), yy = xf_row(inv.m + 4, qx, qy, qz, 1.0f), yz = xf_row(inv.m + 8, qx, qy, qz, 1.0f);
    b.d2 = __int_as_float(0x7f800000); b.pos = -1; b.row = 0x7fffffff;
    oct_walk(six, yx, yy, yz, b);
}

// In partial overlap two thirds of the table's entries are unclaimed, and a lane without a claim would idle through its neighbours' whole
// walks.  So a block compacts the claimed slots of its tiles into a ring in LDS (ballot + mbcnt per wave, the waves' counts through LDS)
// and walks only when the ring holds a full block of items, or at the end: every walk round but the last has all its lanes at work.  The
// ring's counters are block-uniform registers.  A vetoed entry is written back as ~0 by the one lane that owns it: no other thread of
// this launch reads it.
constexpr int kRecipThreads = 256;
constexpr uint32_t kRecipRing = 2 * kRecipThreads;      // under a block of items before a tile is appended, at most a block more after

// q_j is the point half of the target's pair record tn[2 j] in both pairings: TREE keeps the records in the index's order (ix.tq[j]'s bits),
// BRUTE in the caller's (the planar target's bits); the table is indexed the same way.
__global__ __launch_bounds__(kRecipThreads) void k_recip_check(unsigned long long *table, uint32_t n_t, const float4 *__restrict__ tn,
                                                               const RecipArgs *__restrict__ ra, uint32_t *ws)
{
    const TargetIndex &six = ra->six;      // (uniform loads from device memory: the index and the inverse are not kernel arguments)
    const Affine inv = ra->inv;
    __shared__ uint32_t ring[kRecipRing];
    __shared__ uint32_t s_wave[kRecipThreads / 64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t ntiles = (n_t + kRecipThreads - 1) / kRecipThreads;
    uint32_t head = 0u, tail = 0u, claimed = 0u, surv = 0u;
    for (uint32_t tile = blockIdx.x;; tile += gridDim.x) {
        const bool more = tile < ntiles;                   // (block-uniform)
        if (more) {
            const uint32_t j = tile * kRecipThreads + threadIdx.x;
            const bool c = j < n_t && table[j] != ~0ull;
            const unsigned long long m = __ballot(c);
            if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
            __syncthreads();                               // (also: every wave has left the walk round that read the ring before it is written)
            uint32_t off = 0u, total = 0u;
#pragma unroll
            for (uint32_t w = 0; w < kRecipThreads / 64; w++) { const uint32_t v = s_wave[w]; off += w < wave ? v : 0u; total += v; }
            if (c) ring[(tail + off + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))) % kRecipRing] = j;
            tail += total;
            claimed += c ? 1u : 0u;
            __syncthreads();
        }
        while (tail - head >= (uint32_t)kRecipThreads || (!more && tail != head)) {
            const uint32_t left = tail - head, take = left < (uint32_t)kRecipThreads ? left : (uint32_t)kRecipThreads;
            if (threadIdx.x < take) {
                const uint32_t j = ring[(head + threadIdx.x) % kRecipRing];
                const unsigned long long key = table[j];
                const float4 q = tn[2 * (size_t)j];
                Best b;
                reverse_nn(six, inv, q.x, q.y, q.z, b);
                if ((uint32_t)b.row != (uint32_t)(key & 0xFFFFFFFFull)) table[j] = ~0ull;
                else surv++;
            }
            head += take;
        }
        if (!more) break;
    }
    // n_u and n_r: one atomic per wave and word
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        claimed += (uint32_t)__shfl_xor((int)claimed, off, 64);
        surv += (uint32_t)__shfl_xor((int)surv, off, 64);
    }
    if (lane == 0 && claimed) atomicAdd(ws + SEL_CLAIMED, claimed);
    if (lane == 0 && surv) atomicAdd(ws + SEL_RECIP, surv);
}

// UNIQ: the table of k_unique_claim is complete: a candidate that did not win its target gets the sentinel and leaves the population
// (SEL_NC and the histogram); SEL_GATED counts the candidates either way.
template <int CORR, bool UNIQ>
__global__ __launch_bounds__(kSelThreads) void k_reject_keys(PassArgs a, CloudSoA tgt, const float4 *__restrict__ tn)
{
    __shared__ uint32_t h[kSelBins];
    __shared__ uint32_t s_count, s_gated;
    if (threadIdx.x == 0) { s_count = 0u; s_gated = 0u; }
    hist_zero(h);
    const bool gate_n = a.min_ndot > -1.0f;
    uint32_t mine = 0u, gated = 0u;
    const uint32_t stride = gridDim.x * kSelThreads;
    // (whole waves stay in the loop: hist_add is wave-uniform)
    for (uint32_t base = blockIdx.x * kSelThreads; base < a.n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool cand = false;
        float d2 = 0.0f;
        if (i < a.n) {
            uint32_t j;
            cand = pair_candidate<CORR>(a, tgt, tn, gate_n, i, d2, j);
            gated += cand ? 1u : 0u;
            if (UNIQ && cand) cand = j < a.rej.n_t && a.rej.table[j] == claim_key(__float_as_uint(d2), caller_row(a, i));
            a.rej.keys[i] = cand ? __float_as_uint(d2) : 0xFFFFFFFFu;
        }
        hist_add(h, sel_digit<0>(__float_as_uint(d2)), cand);
        mine += cand ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_count, mine);
    if (gated) atomicAdd(&s_gated, gated);
    hist_merge(h, a.rej.ws + SEL_STATE_WORDS);
    if (threadIdx.x == 0 && s_count) atomicAdd(a.rej.ws + SEL_NC, s_count);
    if (threadIdx.x == 0 && s_gated) atomicAdd(a.rej.ws + SEL_GATED, s_gated);
}

// histogram of digit PASS over the keys whose earlier digits equal the prefix fixed so far (PASS 0: every key)
template <int PASS>
__global__ __launch_bounds__(kSelThreads) void k_select_hist(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *ws)
{
    __shared__ uint32_t h[kSelBins];
    hist_zero(h);
    const uint32_t prefix = PASS == 0 ? 0u : ws[SEL_PREFIX], mask = sel_mask<PASS>();
    const uint32_t stride = gridDim.x * kSelThreads;
    for (uint32_t base = blockIdx.x * kSelThreads; base < n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t key = i < n ? keys[i] : 0u;
        hist_add(h, sel_digit<PASS>(key), i < n && (key & mask) == prefix);
    }
    hist_merge(h, ws + SEL_STATE_WORDS + PASS * kSelBins);
}

// One workgroup: the bin of digit PASS that holds rank k (1-based) among the keys that match the prefix.  PASS 0 first sets the rank:
// k_fixed (the probe), else ceil(rho n_c) in fp64 clamped to [1, n_c].  PASS 2 completes tau and the kept count:
// (keys below tau) + (keys equal to tau) = (k0 - rank inside the last bin) + that bin's count.  n_c == 0: tau = 0, nothing kept.
template <int PASS>
__global__ __launch_bounds__(kSelThreads) void k_select_scan(uint32_t *ws, float rho, uint32_t k_fixed, uint32_t n_fixed, RejectRecord *out_host)
{
    constexpr uint32_t kPer = kSelBins / kSelThreads;      // consecutive bins per thread
    __shared__ uint32_t incl[kSelThreads];
    __shared__ uint32_t s_k;
    const uint32_t *hist = ws + SEL_STATE_WORDS + PASS * kSelBins;
    const uint32_t t = threadIdx.x;
    if (t == 0) {
        uint32_t k;
        if (PASS == 0) {
            const uint32_t nc = k_fixed ? n_fixed : ws[SEL_NC];
            if (k_fixed) k = k_fixed;
            else {
                const double kd = ceil((double)rho * (double)nc);
                k = kd < 1.0 ? 1u : (kd > (double)nc ? nc : (uint32_t)kd);
                if (nc == 0u) k = 0u;
            }
            ws[SEL_NC] = nc; ws[SEL_K0] = k; ws[SEL_PREFIX] = 0u;
        } else k = ws[SEL_K];
        s_k = k;
    }
    uint32_t bins[kPer], sum = 0u;
#pragma unroll
    for (uint32_t j = 0; j < kPer; j++) { bins[j] = hist[t * kPer + j]; sum += bins[j]; }
    incl[t] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kSelThreads; off <<= 1) {
        const uint32_t v = t >= off ? incl[t - off] : 0u;
        __syncthreads();
        incl[t] += v;
        __syncthreads();
    }
    const uint32_t k = s_k;
    uint32_t before = incl[t] - sum;                        // keys in the bins below this thread's
    if (k >= 1u && before < k && k <= incl[t]) {
        // (exactly one thread: the prefix sums are monotone and 1 <= k <= total)
        uint32_t j = 0;
        while (j + 1 < kPer && before + bins[j] < k) { before += bins[j]; j++; }
        const uint32_t digit = t * kPer + j;
        const uint32_t prefix = ws[SEL_PREFIX] | (PASS == 0 ? digit << 21 : (PASS == 1 ? digit << 10 : digit));
        ws[SEL_PREFIX] = prefix;
        ws[SEL_K] = k - before;
        if (PASS == 2) {
            const uint32_t kept = ws[SEL_K0] - (k - before) + bins[j];
            ws[SEL_TAU] = prefix; ws[SEL_KEPT] = kept;
            publish_record(ws, out_host);
        }
    }
    if (k == 0u && t == 0) {
        ws[SEL_K] = 0u;
        if (PASS == 2) {
            ws[SEL_TAU] = 0u; ws[SEL_KEPT] = 0u;
            publish_record(ws, out_host);
        }
    }
}

static uint32_t sel_blocks(uint32_t n)
{
    const uint32_t nb = (n + kSelThreads - 1) / kSelThreads;
    return nb < 1u ? 1u : (nb > kSelMaxBlocks ? kSelMaxBlocks : nb);
}

// scan 0, hist 1, scan 1, hist 2, scan 2: the five launches behind the first histogram
static void launch_select_tail(const uint32_t *keys, uint32_t n, uint32_t *ws, float rho, uint32_t k_fixed, RejectRecord *out_host, hipStream_t s)
{
    const uint32_t nb = sel_blocks(n);
    hipLaunchKernelGGL(k_select_scan<0>, dim3(1), dim3(kSelThreads), 0, s, ws, rho, k_fixed, n, nullptr);
    hipLaunchKernelGGL(k_select_hist<1>, dim3(nb), dim3(kSelThreads), 0, s, keys, n, ws);
    hipLaunchKernelGGL(k_select_scan<1>, dim3(1), dim3(kSelThreads), 0, s, ws, rho, k_fixed, n, nullptr);
    hipLaunchKernelGGL(k_select_hist<2>, dim3(nb), dim3(kSelThreads), 0, s, keys, n, ws);
    hipLaunchKernelGGL(k_select_scan<2>, dim3(1), dim3(kSelThreads), 0, s, ws, rho, k_fixed, n, out_host);
}

// ---- tau without a fixed fraction -------------------------------------------------------------------
// One-to-one alone: every non-sentinel key is kept (tau = +Inf: a candidate's d2 is never NaN for finite clouds and transforms).
__global__ void k_reject_all(uint32_t *ws, RejectRecord *out_host)
{
    ws[SEL_TAU] = 0x7F800000u; ws[SEL_KEPT] = ws[SEL_NC];
    publish_record(ws, out_host);
}

// Median distance: the select (rho = 0.5) left the median in SEL_TAU; tau = f2 * med, one fp32 product.  Population 0: tau = 0.  A NaN
// product (f2 overflowed to +Inf and med = 0) counts as +Inf: everything is kept.
__global__ void k_median_tau(uint32_t *ws, float f2)
{
    const uint32_t med = ws[SEL_TAU];
    float tau = ws[SEL_NC] ? f2 * __uint_as_float(med) : 0.0f;
    if (tau != tau) tau = __uint_as_float(0x7F800000u);
    ws[SEL_MED] = med; ws[SEL_TAU] = __float_as_uint(tau); ws[SEL_KEPT] = 0u;
}

// ... and the kept count: the keys <= tau (the sentinel is above every tau)
__global__ __launch_bounds__(kSelThreads) void k_count_le(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *ws)
{
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0) s_count = 0u;
    __syncthreads();
    const uint32_t tau = ws[SEL_TAU];
    uint32_t mine = 0u;
    const uint32_t stride = gridDim.x * kSelThreads;
    for (uint32_t i = blockIdx.x * kSelThreads + threadIdx.x; i < n; i += stride) mine += keys[i] <= tau ? 1u : 0u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mine += (uint32_t)__shfl_xor((int)mine, off, 64);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(&s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && s_count) atomicAdd(ws + SEL_KEPT, s_count);
}

__global__ void k_reject_publish(const uint32_t *ws, RejectRecord *out_host) { publish_record(ws, out_host); }

template <bool UNIQ>
static void launch_keys(const PassArgs &a, int corr, CloudSoA tgt, const float4 *tn, uint32_t nb, hipStream_t s)
{
    if (corr == SYMMICP_CORR_IDENTITY) hipLaunchKernelGGL((k_reject_keys<0, UNIQ>), dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
    else if (corr == SYMMICP_CORR_BRUTE) hipLaunchKernelGGL((k_reject_keys<1, UNIQ>), dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
    else hipLaunchKernelGGL((k_reject_keys<2, UNIQ>), dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
}

// The rejection steps of a pass, behind its search and in front of its accumulating kernel:
//   one-to-one (r.claim; never IDENTITY, whose pairs are one-to-one)   memset of the table, k_unique_claim
//   reciprocal (kClaimReciprocal: r.recip is this pass's RecipArgs)     k_recip_check
//   keys                                                                memset of the workspace, k_reject_keys
//   tau: trim fraction            the select (5 launches), which publishes
//        median factor            the select at rho = 0.5, k_median_tau, k_count_le, k_reject_publish
//        neither                  k_reject_all
// The table is reset by a memset every pass: 8 B per target point at the HBM roof, against a claim that gathers 32 B per source point.
void launch_reject(const PassArgs &a, int corr, CloudSoA tgt, const float4 *tn, hipStream_t s)
{
    const RejectArgs &r = a.rej;
    hipMemsetAsync(r.ws, 0, sizeof(uint32_t) * kRejectWsWords, s);
    const uint32_t nb = sel_blocks(a.n);
    if (r.claim != kClaimNone && corr != SYMMICP_CORR_IDENTITY) {
        hipMemsetAsync(r.table, 0xFF, sizeof(unsigned long long) * r.n_t, s);
        if (corr == SYMMICP_CORR_BRUTE) hipLaunchKernelGGL(k_unique_claim<1>, dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
        else hipLaunchKernelGGL(k_unique_claim<2>, dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
        if (r.claim == kClaimReciprocal)
            hipLaunchKernelGGL(k_recip_check, dim3(sel_blocks(r.n_t)), dim3(kRecipThreads), 0, s, r.table, r.n_t, tn, r.recip, r.ws);
        launch_keys<true>(a, corr, tgt, tn, nb, s);
    } else launch_keys<false>(a, corr, tgt, tn, nb, s);
    if (r.med_f2 > 0.0f) {
        launch_select_tail(r.keys, a.n, r.ws, 0.5f, 0u, nullptr, s);
        hipLaunchKernelGGL(k_median_tau, dim3(1), dim3(1), 0, s, r.ws, r.med_f2);
        hipLaunchKernelGGL(k_count_le, dim3(nb), dim3(kSelThreads), 0, s, r.keys, a.n, r.ws);
        hipLaunchKernelGGL(k_reject_publish, dim3(1), dim3(1), 0, s, r.ws, r.host);
    } else if (r.rho < 1.0f) launch_select_tail(r.keys, a.n, r.ws, r.rho, 0u, r.host, s);
    else hipLaunchKernelGGL(k_reject_all, dim3(1), dim3(1), 0, s, r.ws, r.host);
}

void launch_select_probe(const uint32_t *keys, uint32_t n, uint32_t k, uint32_t *ws, hipStream_t s)
{
    hipMemsetAsync(ws, 0, sizeof(uint32_t) * kRejectWsWords, s);
    hipLaunchKernelGGL(k_select_hist<0>, dim3(sel_blocks(n)), dim3(kSelThreads), 0, s, keys, n, ws);
    launch_select_tail(keys, n, ws, 1.0f, k, nullptr, s);
}

// the claim and the winner test of the probe: the pass's claim_wave and key on rows given as arrays
__global__ __launch_bounds__(kSelThreads) void k_probe_claim(const int32_t *__restrict__ tgt_row, const uint32_t *__restrict__ d2_bits, uint32_t n,
                                                             unsigned long long *table, uint32_t n_t)
{
    const uint32_t stride = gridDim.x * kSelThreads;
    for (uint32_t base = blockIdx.x * kSelThreads; base < n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        const int32_t j = i < n ? tgt_row[i] : -1;
        const bool cand = j >= 0 && (uint32_t)j < n_t;
        claim_wave(table, cand ? (uint32_t)j : 0u, cand ? claim_key(d2_bits[i], i) : ~0ull, cand);
    }
}

__global__ __launch_bounds__(kSelThreads) void k_probe_winner(const int32_t *__restrict__ tgt_row, const uint32_t *__restrict__ d2_bits, uint32_t n,
                                                              const unsigned long long *__restrict__ table, uint32_t n_t, uint8_t *winner)
{
    const uint32_t stride = gridDim.x * kSelThreads;
    for (uint32_t i = blockIdx.x * kSelThreads + threadIdx.x; i < n; i += stride) {
        const int32_t j = tgt_row[i];
        winner[i] = (j >= 0 && (uint32_t)j < n_t && table[j] == claim_key(d2_bits[i], i)) ? 1 : 0;
    }
}

void launch_unique_probe(const int32_t *tgt_row, const uint32_t *d2_bits, uint32_t n, unsigned long long *table, uint32_t n_t,
                         uint8_t *winner_out, hipStream_t s)
{
    hipMemsetAsync(table, 0xFF, sizeof(unsigned long long) * n_t, s);
    hipLaunchKernelGGL(k_probe_claim, dim3(sel_blocks(n)), dim3(kSelThreads), 0, s, tgt_row, d2_bits, n, table, n_t);
    hipLaunchKernelGGL(k_probe_winner, dim3(sel_blocks(n)), dim3(kSelThreads), 0, s, tgt_row, d2_bits, n, table, n_t, winner_out);
}


// ---- reciprocal correspondences: the relabelling of the source index and the test entry of the reverse search ----
__global__ __launch_bounds__(kSelThreads) void k_relabel_tq(float4 *tq, uint32_t n, const uint32_t *__restrict__ labels)
{
    const uint32_t i = blockIdx.x * kSelThreads + threadIdx.x;
    if (i < n) tq[i].w = __uint_as_float(labels[__float_as_uint(tq[i].w)]);
}

void launch_relabel_tq(float4 *tq, uint32_t n, const uint32_t *labels, hipStream_t s)
{
    if (labels && n) hipLaunchKernelGGL(k_relabel_tq, dim3((n + kSelThreads - 1) / kSelThreads), dim3(kSelThreads), 0, s, tq, n, labels);
}

__global__ __launch_bounds__(kRecipThreads) void k_reverse_nn_probe(TargetIndex six, Affine inv, const float *__restrict__ q_xyz, uint32_t n_q,
                                                                    int32_t *label_out, float *d2_out)
{
    const uint32_t i = blockIdx.x * kRecipThreads + threadIdx.x;
    if (i >= n_q) return;
    Best b;
    reverse_nn(six, inv, q_xyz[3 * (size_t)i], q_xyz[3 * (size_t)i + 1], q_xyz[3 * (size_t)i + 2], b);
    label_out[i] = b.row;
    d2_out[i] = b.d2;
}

void launch_reverse_nn_probe(const TargetIndex &six, const Affine &inv, const float *q_xyz, uint32_t n_q, int32_t *label_out, float *d2_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_reverse_nn_probe, dim3((n_q + kRecipThreads - 1) / kRecipThreads), dim3(kRecipThreads), 0, s, six, inv, q_xyz, n_q, label_out, d2_out);
}


}  // namespace symmicp
