// kernels_eval.hip -- registration evaluation (symmicp_evaluate_registration, symmicp_evaluate; DESIGN.md 4, "Registration evaluation").
//
// For K transforms X_k of one source against one indexed target, two launches over (source tile x transform) and one over the transforms:
//   k_eval_search   one thread per (source position, k): move the point by X_k (xf_row), walk the target's octree exactly (oct_walk) from
//                   the bound r2 = max_dist^2 -- a row farther than that finds nothing and is pruned at the root -- and store (nn, d2) of the
//                   row at [k][caller row]: the caller's target row and the distance bits for an inlier, -1 and +Inf otherwise.  Positions
//                   are taken in the order the engine holds the source (Morton order: the 64 lanes of a wave walk one region of the tree).
//   k_eval_sums     one block per (tile of kEvalRows CALLER rows, k): 11 fp64 values per lane (inliers, sum d2, sum q, upper triangle of
//                   sum q q^T, q = the caller's target point widened to fp64), reduced in a fixed order per block.
//   k_eval_final    one block per k: the blocks' records in a fixed order.
// The sums are taken over caller rows, not over the positions the search ran in: the order a context keeps its source in (sort_source) must
// not show in the result, and the walk wants Morton order while the sums want an order that is a function of ns alone.  The price is 8 B
// written and read per row and transform between the two launches.
//
// Summation order (a function of ns alone): nb = min(ceil(ns / kEvalRows), kEvalMaxBlocks) blocks.  Block b, thread t takes the rows
// tile * kEvalRows + j * kEvalThreads + t for tile = b, b + nb, ... and j = 0 .. kEvalRows / kEvalThreads - 1 in that order, adding each
// term to its 11 running sums; the block's 256 lane sums are added pairwise in LDS (t += t + 128, + 64, ... + 1); the nb block records are
// added by thread t over the blocks t, t + 256, ... in ascending order and then by the same pairwise tree.  No floating-point atomics.
//
// fp32 expressions stay UNFUSED and in the association written (the header and tests/_eval_ref.py state the same expressions).
#include "symmicp_internal.h"
#include "device_common.h"
#include "oct_walk.h"
#pragma clang fp contract(off)

namespace symmicp {

__global__ __launch_bounds__(kEvalSearchThreads) void k_eval_search(EvalArgs a)
{
    const uint32_t p = blockIdx.x * kEvalSearchThreads + threadIdx.x, k = blockIdx.y;
    if (p >= a.ns) return;
    const float *__restrict__ m = a.X12 + 12 * (size_t)k;
    // where the point lies and which caller row it is: a context's share is stored in its own order (order: position -> caller row);
    // the host-array form keeps the caller's arrays and reads them through the Morton order (gather)
    const uint32_t row = a.order ? a.order[p] : p;
    const uint32_t at = a.gather ? row : p;
    const float x = a.sx[at], y = a.sy[at], z = a.sz[at];
    const float yx = xf_row(m + 0, x, y, z, 1.0f), yy = xf_row(m + 4, x, y, z, 1.0f), yz = xf_row(m + 8, x, y, z, 1.0f);
    Best b;
    b.d2 = a.r2; b.pos = -1; b.row = 0x7fffffff;      // (r2 = +Inf without a gate; a point AT the bound still wins: its row is below this one)
    oct_walk(a.ix, yx, yy, yz, b);
    const bool hit = b.pos >= 0;
    const size_t o = (size_t)k * a.ns + row;
    a.nn[o] = hit ? b.row : -1;
    a.d2[o] = hit ? b.d2 : __int_as_float(0x7f800000);
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_sums(EvalArgs a, uint32_t nb)
{
    __shared__ double red[kEvalThreads];
    const uint32_t k = blockIdx.y, t = threadIdx.x;
    const int32_t *__restrict__ nn = a.nn + (size_t)k * a.ns;
    const float *__restrict__ d2 = a.d2 + (size_t)k * a.ns;
    double s[kEvalNSum];
#pragma unroll
    for (int v = 0; v < kEvalNSum; v++) s[v] = 0.0;
    const uint32_t ntiles = (a.ns + kEvalRows - 1) / kEvalRows;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += nb) {
        for (uint32_t j = 0; j < kEvalRows / kEvalThreads; j++) {
            const uint32_t i = tile * kEvalRows + j * kEvalThreads + t;      // (ns < 2^31, tile * kEvalRows < ns + kEvalRows: no wrap)
            if (i >= a.ns) break;
            const int32_t r = nn[i];
            if (r < 0) continue;
            const double qx = (double)a.tx[r], qy = (double)a.ty[r], qz = (double)a.tz[r];
            s[0] += 1.0;
            s[1] += (double)d2[i];
            s[2] += qx; s[3] += qy; s[4] += qz;
            s[5] += qx * qx; s[6] += qx * qy; s[7] += qx * qz;
            s[8] += qy * qy; s[9] += qy * qz; s[10] += qz * qz;
        }
    }
    double *out = a.partials + ((size_t)k * nb + blockIdx.x) * kEvalNSum;
#pragma unroll
    for (int v = 0; v < kEvalNSum; v++) {
        red[t] = s[v];
        __syncthreads();
#pragma unroll
        for (int off = kEvalThreads / 2; off > 0; off >>= 1) {
            if (t < (uint32_t)off) red[t] += red[t + off];
            __syncthreads();
        }
        if (t == 0) out[v] = red[0];
        __syncthreads();
    }
}

__global__ __launch_bounds__(kEvalThreads) void k_eval_final(const double *__restrict__ partials, uint32_t nb, double *sums)
{
    __shared__ double red[kEvalThreads];
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    const double *__restrict__ in = partials + (size_t)k * nb * kEvalNSum;
    for (int v = 0; v < kEvalNSum; v++) {
        double s = 0.0;
        for (uint32_t j = t; j < nb; j += kEvalThreads) s += in[(size_t)j * kEvalNSum + v];
        red[t] = s;
        __syncthreads();
#pragma unroll
        for (int off = kEvalThreads / 2; off > 0; off >>= 1) {
            if (t < (uint32_t)off) red[t] += red[t + off];
            __syncthreads();
        }
        if (t == 0) sums[(size_t)k * kEvalNSum + v] = red[0];
        __syncthreads();
    }
}

uint32_t eval_sum_blocks(uint32_t ns)
{
    const uint32_t ntiles = (ns + kEvalRows - 1) / kEvalRows;
    return ntiles < kEvalMaxBlocks ? ntiles : kEvalMaxBlocks;
}

void launch_eval(const EvalArgs &a, uint32_t K, double *sums, hipStream_t s)
{
    const uint32_t nb = eval_sum_blocks(a.ns);
    hipLaunchKernelGGL(k_eval_search, dim3((a.ns + kEvalSearchThreads - 1) / kEvalSearchThreads, K), dim3(kEvalSearchThreads), 0, s, a);
    hipLaunchKernelGGL(k_eval_sums, dim3(nb, K), dim3(kEvalThreads), 0, s, a, nb);
    hipLaunchKernelGGL(k_eval_final, dim3(K), dim3(kEvalThreads), 0, s, a.partials, nb, sums);
}

}  // namespace symmicp
