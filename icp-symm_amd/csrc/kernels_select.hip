// kernels_select.hip -- trimmed ICP (symmicp_set_trim_fraction) for gfx950: the keys of a pass's candidate pairs and the exact
// order statistic over them.
//
// A trimmed pass keeps the closest fraction rho of its candidate pairs (include/symmicp.h has the definition).  Between the search
// and the accumulating kernel of the pass run
//   k_trim_keys      per share row: the bits of the candidate's fp32 d2 -- non-negative floats order as their bit patterns -- or the
//                    sentinel 0xFFFFFFFF for a row without a pair or dropped by a gate; counts the candidates (n_c) and builds the
//                    histogram of the keys' first digit on the way
//   k_select_scan    one workgroup: k = ceil(rho n_c) in fp64 (first digit only), prefix sum over the digit's bins, the bin that
//                    holds rank k; fixes the digit, k becomes the rank inside that bin
//   k_select_hist    histogram of the next digit over the keys that match the digits fixed so far
// as keys, scan, hist, scan, hist, scan: an exact radix select over 32-bit keys in 11 + 11 + 10 bits.  Histograms are per-block in
// LDS (2048 bins, 8 KB), filled with wave-aggregated LDS atomics (the keys of a pass cluster: a handful of first digits hold them
// all) and merged into the global one with integer atomics: order-independent, so tau is reproducible bit for bit.  The last scan
// leaves tau, n_c and the kept count (keys <= tau, ties included) in device memory for the accumulating kernel and in host-mapped
// memory for symmicp_get_trim_state.  Every step is launch-bound (4 B per row and digit), so there is no host round trip in between.
//
// The gates below are pair_step's (kernels_pass.hip), on the same fp32 expressions: unfused, in the association written.
#include "symmicp_internal.h"
#include "device_common.h"
#pragma clang fp contract(off)

namespace symmicp {

constexpr int kSelThreads = 256;
constexpr uint32_t kSelBins = 2048;           // bins of the widest digit (11 bits)
constexpr uint32_t kSelMaxBlocks = 1024;      // grid-stride beyond this
// workspace words (PassArgs::trim_ws): the state, then one histogram per digit
enum { SEL_NC = 0, SEL_K = 1, SEL_PREFIX = 2, SEL_TAU = 3, SEL_KEPT = 4, SEL_K0 = 5, SEL_STATE_WORDS = 16 };
static_assert(kTrimWsWords == SEL_STATE_WORDS + 3 * kSelBins, "symmicp_internal.h sizes the workspace");
static_assert(kTrimTauWord == SEL_TAU, "the accumulating kernels read tau from this word");

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

// CORR: 0 identity (target row = tgt_offset + i), 1 brute (best64), 2 tree (pos_out -> the target's pair record)
template <int CORR>
__global__ __launch_bounds__(kSelThreads) void k_trim_keys(PassArgs a, CloudSoA tgt, const float4 *__restrict__ tn)
{
    __shared__ uint32_t h[kSelBins];
    __shared__ uint32_t s_count;
    if (threadIdx.x == 0) s_count = 0u;
    hist_zero(h);
    const bool gate_n = a.min_ndot > -1.0f;
    uint32_t mine = 0u;
    const uint32_t stride = gridDim.x * kSelThreads;
    // (whole waves stay in the loop: hist_add is wave-uniform)
    for (uint32_t base = blockIdx.x * kSelThreads; base < a.n; base += stride) {
        const uint32_t i = base + threadIdx.x;
        bool cand = false;
        float d2 = 0.0f;
        if (i < a.n) {
            const float x = a.in.x[i], y = a.in.y[i], z = a.in.z[i];
            const float px = xf_row(a.X.m + 0, x, y, z, 1.0f), py = xf_row(a.X.m + 4, x, y, z, 1.0f), pz = xf_row(a.X.m + 8, x, y, z, 1.0f);
            float nqx = 0.0f, nqy = 0.0f, nqz = 0.0f;
            if (CORR == 0) {
                const uint32_t j = a.tgt_offset + i;
                d2 = dist2(px, py, pz, tgt.x[j], tgt.y[j], tgt.z[j]);
                cand = true;
                if (gate_n) { nqx = tgt.nx[j]; nqy = tgt.ny[j]; nqz = tgt.nz[j]; }
            } else if (CORR == 1) {
                const unsigned long long b = a.best64[i];
                cand = b != ~0ull;
                d2 = __uint_as_float((uint32_t)(b >> 32));
                if (cand && gate_n) { const float4 nq = tn[2 * (size_t)(uint32_t)(b & 0xFFFFFFFFull) + 1]; nqx = nq.x; nqy = nq.y; nqz = nq.z; }
            } else {
                const int32_t pos = a.pos_out[i];
                cand = pos >= 0;
                if (cand) {
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
            a.trim_keys[i] = cand ? __float_as_uint(d2) : 0xFFFFFFFFu;
        }
        hist_add(h, sel_digit<0>(__float_as_uint(d2)), cand);
        mine += cand ? 1u : 0u;
    }
    if (mine) atomicAdd(&s_count, mine);
    hist_merge(h, a.trim_ws + SEL_STATE_WORDS);
    if (threadIdx.x == 0 && s_count) atomicAdd(a.trim_ws + SEL_NC, s_count);
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
__global__ __launch_bounds__(kSelThreads) void k_select_scan(uint32_t *ws, float rho, uint32_t k_fixed, uint32_t n_fixed, uint32_t *out_host)
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
            if (out_host) { out_host[0] = ws[SEL_NC]; out_host[1] = kept; out_host[2] = prefix; }
        }
    }
    if (k == 0u && t == 0) {
        ws[SEL_K] = 0u;
        if (PASS == 2) {
            ws[SEL_TAU] = 0u; ws[SEL_KEPT] = 0u;
            if (out_host) { out_host[0] = ws[SEL_NC]; out_host[1] = 0u; out_host[2] = 0u; }
        }
    }
}

static uint32_t sel_blocks(uint32_t n)
{
    const uint32_t nb = (n + kSelThreads - 1) / kSelThreads;
    return nb < 1u ? 1u : (nb > kSelMaxBlocks ? kSelMaxBlocks : nb);
}

// scan 0, hist 1, scan 1, hist 2, scan 2: the five launches behind the first histogram
static void launch_select_tail(const uint32_t *keys, uint32_t n, uint32_t *ws, float rho, uint32_t k_fixed, uint32_t *out_host, hipStream_t s)
{
    const uint32_t nb = sel_blocks(n);
    hipLaunchKernelGGL(k_select_scan<0>, dim3(1), dim3(kSelThreads), 0, s, ws, rho, k_fixed, n, nullptr);
    hipLaunchKernelGGL(k_select_hist<1>, dim3(nb), dim3(kSelThreads), 0, s, keys, n, ws);
    hipLaunchKernelGGL(k_select_scan<1>, dim3(1), dim3(kSelThreads), 0, s, ws, rho, k_fixed, n, nullptr);
    hipLaunchKernelGGL(k_select_hist<2>, dim3(nb), dim3(kSelThreads), 0, s, keys, n, ws);
    hipLaunchKernelGGL(k_select_scan<2>, dim3(1), dim3(kSelThreads), 0, s, ws, rho, k_fixed, n, out_host);
}

void launch_trim_select(const PassArgs &a, int corr, CloudSoA tgt, const float4 *tn, hipStream_t s)
{
    hipMemsetAsync(a.trim_ws, 0, sizeof(uint32_t) * kTrimWsWords, s);
    const uint32_t nb = sel_blocks(a.n);
    if (corr == SYMMICP_CORR_IDENTITY) hipLaunchKernelGGL(k_trim_keys<0>, dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
    else if (corr == SYMMICP_CORR_BRUTE) hipLaunchKernelGGL(k_trim_keys<1>, dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
    else hipLaunchKernelGGL(k_trim_keys<2>, dim3(nb), dim3(kSelThreads), 0, s, a, tgt, tn);
    launch_select_tail(a.trim_keys, a.n, a.trim_ws, a.trim_rho, 0u, a.trim_host, s);
}

void launch_select_probe(const uint32_t *keys, uint32_t n, uint32_t k, uint32_t *ws, hipStream_t s)
{
    hipMemsetAsync(ws, 0, sizeof(uint32_t) * kTrimWsWords, s);
    hipLaunchKernelGGL(k_select_hist<0>, dim3(sel_blocks(n)), dim3(kSelThreads), 0, s, keys, n, ws);
    launch_select_tail(keys, n, ws, 1.0f, k, nullptr, s);
}

}  // namespace symmicp
