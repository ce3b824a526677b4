// kernels_plane.hip -- RANSAC plane segmentation on gfx950: H plane hypotheses scored against all n points of a cloud.
// include/symmicp.h defines the arithmetic (plane_core.h holds it); tests/_segplane_ref.py restates it in numpy.
//
//   k_plane_hyp        one thread per hypothesis: three SplitMix64 draws of (seed, stream 2), the checks of symmicp.h in their order,
//                      n and d; writes status and 4 floats and appends an EVALUATED hypothesis to the list of survivors (the position in
//                      the list carries no meaning: every result is keyed by h).
//   k_plane_score<LDS, Q>  HYPOTHESES IN LANES, THE POINT WAVE-UNIFORM.  grid = (batches of 256 Q survivors) x (rows of workgroups that
//                      stride over the chunks of kPlaneChunk points).  A lane keeps (n, d) of Q survivors and their counts in registers
//                      and walks the chunk; every lane of a wave reads the same point -- from LDS, staged once per chunk (a broadcast
//                      read: one address, no bank conflict), or with LDS = false straight from global memory at a wave-uniform address,
//                      which the compiler turns into scalar loads (the point then sits in SGPRs and the VALU reads it as an operand).
//                      No cross-lane operation, no per-point atomic: one integer atomicAdd per (hypothesis, workgroup) at the end.
//                      Integer sums are order-free.  Q = 2 halves the LDS reads per evaluation: at Q = 1 the LDS array (a 16-byte
//                      broadcast read costs 4 of its cycles) is as busy as the VALU.
//   k_plane_score_pts  the alternative, k_ransac_eval's shape: 4 points per thread in registers, (n, d) of a survivor wave-uniform,
//                      __ballot + popcount, one atomicAdd per (hypothesis, wave, tile).  Kept for the A/B of profiles/plane_workload.py
//                      (SYMMICP_PLANE_SCORE=2); DESIGN.md 4, "Plane segmentation" has the times.
//   k_plane_mask       the winner's inlier flags over all points, the winner read from the arg-max key on the device
//                      (k_ransac_argmax, kernels_global.hip: EVALUATED is 0 for both), and its (n, d) for the host.
#include "symmicp_internal.h"
#include "plane_core.h"
#pragma clang fp contract(off)

namespace symmicp {

constexpr int kPlanePtsPer = 4;                       // k_plane_score_pts: points per thread
constexpr int kPlanePtsTile = 256 * kPlanePtsPer;
constexpr int kPlanePtsBatch = 32;                    // ... survivors per block

// pts [n]: (p.xyz, 0) about the pivot.  hyp [H][4], status [H], inliers [H] (zeroed here); survivors appended to surv, counted in *n_surv.
__global__ __launch_bounds__(256) void k_plane_hyp(const float4 *__restrict__ pts, uint32_t n, uint32_t H, unsigned long long base, int have_axis,
                                                   float ax, float ay, float az, float cos_min, float4 *hyp, uint8_t *status, int32_t *inliers,
                                                   uint32_t *surv, uint32_t *n_surv)
{
    const uint32_t h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= H) return;
    uint32_t c[3];
    float P[3][3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        c[k] = ransac_draw(base, 3ull * h + k, n);
        const float4 p = pts[c[k]];
        P[k][0] = p.x; P[k][1] = p.y; P[k][2] = p.z;
    }
    const float axis[3] = {ax, ay, az};
    float nd[4] = {0.f, 0.f, 0.f, 0.f};
    const int st = plane_hypothesis<float>(c, P, have_axis != 0, axis, cos_min, nd);
    status[h] = (uint8_t)st;
    inliers[h] = 0;
    const bool have = st == SYMMICP_PLANE_EVALUATED || st == SYMMICP_PLANE_OFF_AXIS;
    hyp[h] = have ? make_float4(nd[0], nd[1], nd[2], nd[3]) : make_float4(0.f, 0.f, 0.f, 0.f);
    if (st == SYMMICP_PLANE_EVALUATED) surv[atomicAdd(n_surv, 1u)] = h;
}

template <bool LDS, int Q>
__global__ __launch_bounds__(256) void k_plane_score(const float4 *__restrict__ pts, uint32_t n, const float4 *__restrict__ hyp,
                                                     const uint32_t *__restrict__ surv, const uint32_t *__restrict__ n_surv, float max_dist,
                                                     int32_t *inliers)
{
    __shared__ float4 tile[LDS ? kPlaneChunk : 1];
    const uint32_t ns = *n_surv;
    const uint32_t s0 = blockIdx.x * (256u * Q);
    if (s0 >= ns) return;                                  // (block-uniform: the grid is sized for H survivors)
    uint32_t h[Q];
    float nd[Q][4];
    int cnt[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) {
        const uint32_t s = s0 + j * 256u + threadIdx.x;
        h[j] = surv[s < ns ? s : s0];                      // (a lane past the end scores a copy of the block's first and adds nothing)
        const float4 q = hyp[h[j]];
        nd[j][0] = q.x; nd[j][1] = q.y; nd[j][2] = q.z; nd[j][3] = q.w;
        cnt[j] = 0;
    }
    const uint32_t chunks = (n + kPlaneChunk - 1) / kPlaneChunk;
    for (uint32_t chunk = blockIdx.y; chunk < chunks; chunk += gridDim.y) {
        const uint32_t i0 = chunk * kPlaneChunk;
        const uint32_t m = min((uint32_t)kPlaneChunk, n - i0);
        const float4 *src = pts + i0;
        if (LDS) {
            __syncthreads();
            for (uint32_t r = threadIdx.x; r < m; r += 256u) tile[r] = src[r];
            __syncthreads();
            src = tile;
        }
#pragma unroll 4
        for (uint32_t r = 0; r < m; r++) {
            const float4 a = src[r];                       // one address for the whole wave
            const float p[3] = {a.x, a.y, a.z};
#pragma unroll
            for (int j = 0; j < Q; j++) cnt[j] += fabsf(plane_offset<float>(nd[j], p)) <= max_dist ? 1 : 0;
        }
    }
#pragma unroll
    for (int j = 0; j < Q; j++)
        if (s0 + j * 256u + threadIdx.x < ns && cnt[j] > 0) atomicAdd(&inliers[h[j]], cnt[j]);
}

__global__ __launch_bounds__(256) void k_plane_score_pts(const float4 *__restrict__ pts, uint32_t n, const float4 *__restrict__ hyp,
                                                         const uint32_t *__restrict__ surv, const uint32_t *__restrict__ n_surv, float max_dist,
                                                         int32_t *inliers)
{
    const uint32_t ns = *n_surv;
    const uint32_t s0 = blockIdx.x * kPlanePtsBatch;
    if (s0 >= ns) return;
    const uint32_t s1 = min(s0 + kPlanePtsBatch, ns);
    const uint32_t tiles = (n + kPlanePtsTile - 1) / kPlanePtsTile;
    for (uint32_t t = blockIdx.y; t < tiles; t += gridDim.y) {
        float p[kPlanePtsPer][3];
        bool live[kPlanePtsPer];
#pragma unroll
        for (int u = 0; u < kPlanePtsPer; u++) {
            const uint32_t i = t * kPlanePtsTile + u * 256 + threadIdx.x;
            live[u] = i < n;
            const float4 a = pts[min(i, n - 1)];
            p[u][0] = a.x; p[u][1] = a.y; p[u][2] = a.z;
        }
        for (uint32_t s = s0; s < s1; s++) {
            const uint32_t h = surv[s];
            const float4 q = hyp[h];
            const float nd[4] = {q.x, q.y, q.z, q.w};
            int cnt = 0;
#pragma unroll
            for (int u = 0; u < kPlanePtsPer; u++) {
                const bool in = live[u] && fabsf(plane_offset<float>(nd, p[u])) <= max_dist;
                cnt += __popcll(__ballot(in));
            }
            if ((threadIdx.x & 63) == 0 && cnt > 0) atomicAdd(&inliers[h], cnt);
        }
    }
}

// best: the arg-max key (0: nothing evaluated).  mask [n] = the winner's inlier flags (zeros without a winner); nd_out = its (n, d).
__global__ __launch_bounds__(256) void k_plane_mask(const float4 *__restrict__ pts, uint32_t n, const float4 *__restrict__ hyp,
                                                    const unsigned long long *__restrict__ best, float max_dist, uint8_t *mask, float4 *nd_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long key = *best;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (key != 0ull) q = hyp[0xFFFFFFFFu - (uint32_t)key];
    if (i == 0) *nd_out = q;
    if (i >= n) return;
    const float4 a = pts[i];
    const float nd[4] = {q.x, q.y, q.z, q.w}, p[3] = {a.x, a.y, a.z};
    mask[i] = (key != 0ull && fabsf(plane_offset<float>(nd, p)) <= max_dist) ? 1 : 0;
}

void launch_plane_hyp(const float *pts4, uint32_t n, uint32_t H, unsigned long long base, const float *axis, float cos_min, float *hyp4,
                      uint8_t *status, int32_t *inliers, uint32_t *surv, uint32_t *n_surv, hipStream_t s)
{
    hipLaunchKernelGGL(k_plane_hyp, dim3((H + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4 *>(pts4), n, H, base, axis ? 1 : 0,
                       axis ? axis[0] : 0.f, axis ? axis[1] : 0.f, axis ? axis[2] : 0.f, cos_min, reinterpret_cast<float4 *>(hyp4), status, inliers,
                       surv, n_surv);
}

template <bool LDS, int Q>
static void launch_score_lanes(const float4 *pts, uint32_t n, const float4 *hyp, const uint32_t *surv, const uint32_t *n_surv, uint32_t H,
                               float max_dist, int32_t *inliers, hipStream_t s)
{
    // about kPlaneBlocks workgroups in all, each striding over the chunks of its row of the grid: the chip is filled once, evenly
    const uint32_t batches = (H + 256 * Q - 1) / (256 * Q), chunks = (n + kPlaneChunk - 1) / kPlaneChunk;
    const dim3 grid(batches, min(chunks, max(1u, (uint32_t)kPlaneBlocks / batches)));
    hipLaunchKernelGGL((k_plane_score<LDS, Q>), grid, dim3(256), 0, s, pts, n, hyp, surv, n_surv, max_dist, inliers);
}

// The grid is sized for H survivors (the count stays on the device: blocks past it leave at once).  shape: 0 the lane-per-hypothesis
// kernel from LDS with kPlaneLaneHyps hypotheses per lane, 1 the same with one, 4 with four, 3 with one on scalar loads, 2 the
// points-in-registers alternative.
void launch_plane_score(const float *pts4, uint32_t n, const float *hyp4, const uint32_t *surv, const uint32_t *n_surv, uint32_t H, float max_dist,
                        int32_t *inliers, int shape, hipStream_t s)
{
    const float4 *pts = reinterpret_cast<const float4 *>(pts4), *hyp = reinterpret_cast<const float4 *>(hyp4);
    if (shape == 2) {
        const uint32_t tiles = (n + kPlanePtsTile - 1) / kPlanePtsTile;
        const uint32_t batches = (H + kPlanePtsBatch - 1) / kPlanePtsBatch;
        const dim3 grid(batches, min(tiles, max(1u, min(4096u, (1u << 22) / batches))));
        hipLaunchKernelGGL(k_plane_score_pts, grid, dim3(256), 0, s, pts, n, hyp, surv, n_surv, max_dist, inliers);
    }
    else if (shape == 1) launch_score_lanes<true, 1>(pts, n, hyp, surv, n_surv, H, max_dist, inliers, s);
    else if (shape == 3) launch_score_lanes<false, 1>(pts, n, hyp, surv, n_surv, H, max_dist, inliers, s);
    else if (shape == 4) launch_score_lanes<true, 4>(pts, n, hyp, surv, n_surv, H, max_dist, inliers, s);
    else launch_score_lanes<true, kPlaneLaneHyps>(pts, n, hyp, surv, n_surv, H, max_dist, inliers, s);
}

void launch_plane_mask(const float *pts4, uint32_t n, const float *hyp4, const unsigned long long *best, float max_dist, uint8_t *mask,
                       float *nd_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_plane_mask, dim3((n + 255) / 256), dim3(256), 0, s, reinterpret_cast<const float4 *>(pts4), n,
                       reinterpret_cast<const float4 *>(hyp4), best, max_dist, mask, reinterpret_cast<float4 *>(nd_out));
}

}  // namespace symmicp
