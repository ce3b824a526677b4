// kernels_global.hip -- feature matching and RANSAC on gfx950: the two thirds of global registration that follow the FPFH
// features.  include/symmicp.h defines the arithmetic; tests/_global_ref.py restates it in numpy.
//
//   k_feature_nn<Q>   exact nearest and second-nearest candidate of every query in the 33-d feature space, brute force.  256 threads,
//                     Q queries per thread held in registers (33 floats each, statically indexed), candidates staged through LDS in
//                     tiles of rows padded to 36 floats: every lane of a wave reads the same 16-byte word of a row (a broadcast, no
//                     bank conflict).  D(i, j) is the sum of 33 squared differences in ascending bin order, fp32 and unfused, so the
//                     result is the same bits on any tiling.  blockIdx.y splits the candidates when the queries alone do not fill
//                     the device; every block writes its partial (D, j, second) and
//   k_feature_merge   folds the partials of a query in ascending split order: minimum and second minimum under the (D, j) order
//                     are associative, so the split changes nothing.
//   k_ransac_hyp      one thread per hypothesis: three SplitMix64 draws, the checks of symmicp.h in their order, the two frames,
//                     R and t; writes status and 12 floats and appends the hypothesis to the list of survivors (position in the
//                     list carries no meaning: every result is keyed by h).
//   k_ransac_eval     grid = (batches of kEvalBatch survivors) x (tiles of 1024 correspondences): a thread keeps 4 correspondences
//                     in registers, the 12 floats of a hypothesis are wave-uniform loads; __ballot + popcount per wave, one
//                     integer atomicAdd per wave and hypothesis.
//   k_ransac_argmax   max over the evaluated hypotheses of (inliers << 32) | (0xFFFFFFFF - h): most inliers, lowest h.
#include "symmicp_internal.h"
#include "ransac_core.h"
#pragma clang fp contract(off)

namespace symmicp {

constexpr int kFeat = 33;
constexpr int kFeatPad = 36;            // floats per candidate row in LDS: nine 16-byte words
constexpr int kNnThreads = 256;
constexpr int kNnTile = 128;            // candidate rows per LDS tile (18 KB)

struct NnPartial { float d, second; int32_t j; int32_t pad; };

// one candidate row (LDS, wave-uniform address) against one query in registers: the contract's D(i, j)
__device__ __forceinline__ float feat_dist(const float (&q)[kFeatPad], const float4 *row)
{
    float acc = 0.0f;
#pragma unroll
    for (int v = 0; v < kFeatPad / 4; v++) {
        const float4 c = row[v];
        float t = q[4 * v] - c.x;
        acc = acc + t * t;
        if (4 * v + 1 < kFeat) {
            t = q[4 * v + 1] - c.y; acc = acc + t * t;
            t = q[4 * v + 2] - c.z; acc = acc + t * t;
            t = q[4 * v + 3] - c.w; acc = acc + t * t;
        }
    }
    return acc;
}

// candidates [j_lo, j_hi) of this block's split against Q queries per thread; out: partial[split][query] when gridDim.y > 1
template <int Q>
__global__ __launch_bounds__(kNnThreads) void k_feature_nn(const float *__restrict__ fa, uint32_t na, const float *__restrict__ fb, uint32_t nb,
                                                           uint32_t per_split, NnPartial *partial, int32_t *nn_out, float *d2_out,
                                                           float *second_out)
{
    __shared__ float4 tile[kNnTile * kFeatPad / 4];
    float *tile_f = reinterpret_cast<float *>(tile);
    const uint32_t i0 = (blockIdx.x * kNnThreads + threadIdx.x) * Q;
    float q[Q][kFeatPad];
    float best[Q], second[Q];
    int32_t bj[Q];
#pragma unroll
    for (int u = 0; u < Q; u++) {
        const uint32_t i = min(i0 + u, na - 1);           // rows past the end compute a copy of the last one and write nothing
        const float *src = fa + (size_t)i * kFeat;
#pragma unroll
        for (int b = 0; b < kFeatPad; b++) q[u][b] = b < kFeat ? src[b] : 0.0f;
        best[u] = INFINITY; second[u] = INFINITY; bj[u] = -1;
    }
    const uint32_t j_lo = min((uint32_t)blockIdx.y * per_split, nb);
    const uint32_t j_hi = (uint32_t)min((uint64_t)j_lo + per_split, (uint64_t)nb);
    for (uint32_t j0 = j_lo; j0 < j_hi; j0 += kNnTile) {
        const uint32_t cnt = min((uint32_t)kNnTile, j_hi - j0);
        __syncthreads();
        const float *src = fb + (size_t)j0 * kFeat;
        for (uint32_t e = threadIdx.x; e < cnt * kFeat; e += kNnThreads) {
            const uint32_t r = e / kFeat, b = e - r * kFeat;
            tile_f[r * kFeatPad + b] = src[e];
        }
        __syncthreads();
        for (uint32_t r = 0; r < cnt; r++) {
            const float4 *row = tile + r * (kFeatPad / 4);
#pragma unroll
            for (int u = 0; u < Q; u++) {
                const float d = feat_dist(q[u], row);
                // ascending j and strict <: ties keep the lowest row; the first candidate always enters (D is finite)
                if (d < best[u] || bj[u] < 0) { second[u] = best[u]; best[u] = d; bj[u] = (int32_t)(j0 + r); }
                else if (d < second[u]) second[u] = d;
            }
        }
    }
#pragma unroll
    for (int u = 0; u < Q; u++) {
        const uint32_t i = i0 + u;
        if (i >= na) continue;
        if (gridDim.y > 1) {
            NnPartial p; p.d = best[u]; p.second = second[u]; p.j = bj[u]; p.pad = 0;
            partial[(size_t)blockIdx.y * na + i] = p;
        } else {
            nn_out[i] = bj[u];
            if (d2_out) d2_out[i] = best[u];
            if (second_out) second_out[i] = second[u];
        }
    }
}

__global__ __launch_bounds__(256) void k_feature_merge(const NnPartial *__restrict__ partial, uint32_t na, uint32_t splits, int32_t *nn_out,
                                                       float *d2_out, float *second_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= na) return;
    float best = INFINITY, second = INFINITY;
    int32_t bj = -1;
    for (uint32_t s = 0; s < splits; s++) {
        const NnPartial p = partial[(size_t)s * na + i];
        if (p.j < 0) continue;                             // an empty split
        // splits hold ascending candidate ranges: strict < keeps the lowest row on ties
        if (p.d < best || bj < 0) { second = fminf(best, p.second); best = p.d; bj = p.j; }
        else second = fminf(second, p.d);                  // (p.second >= p.d)
    }
    nn_out[i] = bj;
    if (d2_out) d2_out[i] = best;
    if (second_out) second_out[i] = second;
}

void launch_feature_nn(const float *fa, uint32_t na, const float *fb, uint32_t nb, int queries_per_thread, uint32_t splits, void *partial,
                       int32_t *nn_out, float *d2_out, float *second_out, hipStream_t s)
{
    const uint32_t per_split = (uint32_t)(((uint64_t)nb + splits - 1) / splits);
    NnPartial *pp = static_cast<NnPartial *>(partial);
    if (queries_per_thread == 2) {
        const dim3 grid((na + 2 * kNnThreads - 1) / (2 * kNnThreads), splits);
        hipLaunchKernelGGL(k_feature_nn<2>, grid, dim3(kNnThreads), 0, s, fa, na, fb, nb, per_split, pp, nn_out, d2_out, second_out);
    } else {
        const dim3 grid((na + kNnThreads - 1) / kNnThreads, splits);
        hipLaunchKernelGGL(k_feature_nn<1>, grid, dim3(kNnThreads), 0, s, fa, na, fb, nb, per_split, pp, nn_out, d2_out, second_out);
    }
    if (splits > 1) hipLaunchKernelGGL(k_feature_merge, dim3((na + 255) / 256), dim3(256), 0, s, pp, na, splits, nn_out, d2_out, second_out);
}

size_t feature_nn_partial_bytes(uint32_t na, uint32_t splits) { return splits > 1 ? sizeof(NnPartial) * (size_t)na * splits : 0; }

// ---- RANSAC ------------------------------------------------------------------------------------------------------------------
constexpr int kEvalBatch = 32;          // survivors per block of k_ransac_eval
constexpr int kEvalPer = 4;             // correspondences per thread
constexpr int kEvalTile = 256 * kEvalPer;

// pq [m][8]: p.xyz, 0, q.xyz, 0 about the pivots.  hyp [H][12], status [H]; survivors appended to surv, counted in *n_surv.
__global__ __launch_bounds__(256) void k_ransac_hyp(const float4 *__restrict__ pq, uint32_t m, uint32_t H, unsigned long long base,
                                                    float max_dist2, float edge2, float *hyp, uint8_t *status, int32_t *inliers,
                                                    uint32_t *surv, uint32_t *n_surv)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    uint32_t c[3];
#pragma unroll
    for (int k = 0; k < 3; k++) c[k] = ransac_draw(base, 3ull * h + k, m);
    float P[3][3], Qp[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float4 p = pq[2 * (size_t)c[k]], q = pq[2 * (size_t)c[k] + 1];
        P[k][0] = p.x; P[k][1] = p.y; P[k][2] = p.z;
        Qp[k][0] = q.x; Qp[k][1] = q.y; Qp[k][2] = q.z;
    }
    float Rt[12];
    const int st = ransac_hypothesis<float>(c, P, Qp, edge2, max_dist2, Rt);
    status[h] = (uint8_t)st;
    inliers[h] = 0;
    const bool have = st == SYMMICP_RANSAC_EVALUATED || st == SYMMICP_RANSAC_FAR;
#pragma unroll
    for (int k = 0; k < 12; k++) hyp[(size_t)h * 12 + k] = have ? Rt[k] : 0.0f;
    if (st == SYMMICP_RANSAC_EVALUATED) surv[atomicAdd(n_surv, 1u)] = h;
}

__global__ __launch_bounds__(256) void k_ransac_eval(const float4 *__restrict__ pq, uint32_t m, const float *__restrict__ hyp,
                                                     const uint32_t *__restrict__ surv, const uint32_t *__restrict__ n_surv, float max_dist2,
                                                     int32_t *inliers)
{
    const uint32_t ns = *n_surv;
    const uint32_t s0 = blockIdx.x * kEvalBatch;
    if (s0 >= ns) return;
    const uint32_t s1 = min(s0 + kEvalBatch, ns);
    const uint32_t tiles = (m + kEvalTile - 1) / kEvalTile;
    for (uint32_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
        float p[kEvalPer][3], q[kEvalPer][3];
        bool live[kEvalPer];
#pragma unroll
        for (int u = 0; u < kEvalPer; u++) {
            const uint32_t k = tile * kEvalTile + u * 256 + threadIdx.x;
            live[u] = k < m;
            const float4 a = pq[2 * (size_t)min(k, m - 1)], b = pq[2 * (size_t)min(k, m - 1) + 1];
            p[u][0] = a.x; p[u][1] = a.y; p[u][2] = a.z;
            q[u][0] = b.x; q[u][1] = b.y; q[u][2] = b.z;
        }
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t h = surv[s];
            const float *Rt = hyp + (size_t)h * 12;
            float r[12];
#pragma unroll
            for (int k = 0; k < 12; k++) r[k] = Rt[k];
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < kEvalPer; u++) {
                const bool in = live[u] && ransac_residual2<float>(r, p[u], q[u]) <= max_dist2;
                cnt += __popcll(__ballot(in));
            }
            if ((threadIdx.x & 63) == 0 && cnt > 0) atomicAdd(&inliers[h], cnt);
        }
    }
}

__global__ __launch_bounds__(256) void k_ransac_argmax(const uint8_t *__restrict__ status, const int32_t *__restrict__ inliers, uint32_t H,
                                                       unsigned long long *best)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long key = 0ull;
    if (h < H && status[h] == SYMMICP_RANSAC_EVALUATED) key = ((unsigned long long)(uint32_t)inliers[h] << 32) | (0xFFFFFFFFull - h);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best, key);
}

void launch_ransac_hyp(const float *pq8, uint32_t m, uint32_t H, unsigned long long base, float max_dist2, float edge2, float *hyp,
                       uint8_t *status, int32_t *inliers, uint32_t *surv, uint32_t *n_surv, hipStream_t s)
{
    hipLaunchKernelGGL(k_ransac_hyp, dim3((H + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4 *>(pq8), m, H, base, max_dist2,
                       edge2, hyp, status, inliers, surv, n_surv);
}

// n_surv_host: the survivor count as the host read it (sizes the grid; the kernel reads the device's copy)
void launch_ransac_eval(const float *pq8, uint32_t m, const float *hyp, const uint32_t *surv, const uint32_t *n_surv, uint32_t n_surv_host,
                        float max_dist2, int32_t *inliers, hipStream_t s)
{
    if (n_surv_host == 0) return;
    const uint32_t tiles = (m + kEvalTile - 1) / kEvalTile;
    const dim3 grid((n_surv_host + kEvalBatch - 1) / kEvalBatch, min(tiles, 4096u));
    hipLaunchKernelGGL(k_ransac_eval, grid, dim3(256), 0, s, reinterpret_cast<const float4 *>(pq8), m, hyp, surv, n_surv, max_dist2, inliers);
}

void launch_ransac_argmax(const uint8_t *status, const int32_t *inliers, uint32_t H, unsigned long long *best, hipStream_t s)
{
    hipLaunchKernelGGL(k_ransac_argmax, dim3((H + 255) / 256), dim3(256), 0, s, status, inliers, H, best);
}

}  // namespace symmicp
