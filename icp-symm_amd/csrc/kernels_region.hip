// kernels_region.hip -- region-growing segmentation on gfx950 (symmicp_ctx_region_growing; include/symmicp.h defines the result,
// DESIGN.md 4 "Region growing" has the measurements; tests/_region_ref.py restates it in numpy).
//
// The regions are the connected components of the SMOOTH graph on the SEED rows: the radius graph of the clustering with one more
// test per edge, |n_i . n_j| >= smoothness_cos.  Like the radius graph it is never stored: every kernel walks the box tree with the
// exact radius walk of box_walk.h and meets the edges of its point on the way; the normals are the sorted ones of the index
// (ix.tn[2 * jj + 1], as kernels_fpfh.hip reads them).
//
//   k_region_seeds     seed[row] = curv == null || curv[row] <= threshold, an int32 0 / 1 by caller row: with need = 1 it is a `count` to
//                      k_cluster_init / k_cluster_flatten (launch_cluster_init, launch_cluster_flatten), which run unchanged
//   k_region_union     one thread per SEED point in sorted order: for every seed neighbour at a HIGHER sorted position (each edge once)
//                      whose parent word does not already show it to be in the point's set, and whose normal passes the test,
//                      cluster::unite.  The tests run cheapest first: position, seed flag (4 B), parent word (4 B), and only then the
//                      16-byte normal (at 1M points the parent word settles 5 % of the examined edges at 2 spacings and 17 % at 4).
//   k_region_border    one thread per NON-seed point: the minimum of (d2 bits << 32 | representative) over its smooth seed neighbours, kept
//                      in a register; the low word is the point's root, kClusterNoise when it has none.  Seed entries of parent[] are only
//                      read here and non-seed entries only written, each by its own thread.
//   k_region_smooth    (only when smooth_out is asked for) smooth[row] = the number of smooth neighbours, seeds or not
// No loop in these kernels waits for another thread (cluster_core.h): a lost compare-and-swap descends and goes on.
#include "symmicp_internal.h"
#pragma clang fp contract(off)
#include "box_walk.h"             // radius_walk, stage_level_off
#include "cluster_core.h"

namespace symmicp {

using cluster::AgentOps;

constexpr int kRegionThreads = 256;

// the smoothness test of the header: fp32, unfused, in this association; symmetric in (a, b) bit for bit, blind to either sign
__device__ __forceinline__ bool region_smooth(const float4 &a, const float4 &b, float smoothness_cos)
{
    return fabsf((a.x * b.x + a.y * b.y) + a.z * b.z) >= smoothness_cos;
}

__global__ __launch_bounds__(kRegionThreads) void k_region_seeds(const float *__restrict__ curv, float threshold, uint32_t n, int32_t *seed)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) seed[i] = (!curv || curv[i] <= threshold) ? 1 : 0;
}

// stats (may be null): [0] += unite calls, [1] += lost compare-and-swaps, [2] += edges examined (in range, higher position), [3] += normal loads
__global__ __launch_bounds__(kRegionThreads) void k_region_union(TargetIndex ix, float r2, float smoothness_cos, const int32_t *__restrict__ seed,
                                                                 uint32_t *parent, unsigned long long *stats)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const uint32_t row_me = (uint32_t)__float_as_int(me.w);
    if (!seed[row_me]) return;
    const float4 mn = ix.tn[2 * (size_t)i + 1];
    // top: the row this point's set hung from when last seen, and a stale parent word that equals it settles an edge without a union
    // (k_cluster_union says why both are sound); here it settles the edge without the normal as well
    uint32_t calls = 0, lost = 0, edges = 0, loads = 0, top = row_me;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &q, float) {
        if (jj <= i) return;
        edges++;
        const uint32_t row_j = (uint32_t)__float_as_int(q.w);
        if (!seed[row_j]) return;
        if (parent[row_j] == top) return;
        loads++;
        if (!region_smooth(mn, ix.tn[2 * (size_t)jj + 1], smoothness_cos)) return;
        calls++;
        top = cluster::unite<AgentOps>(parent, top, row_j, &lost);
    });
    if (stats) {
        atomicAdd(stats + 0, (unsigned long long)calls);
        if (lost) atomicAdd(stats + 1, (unsigned long long)lost);
        atomicAdd(stats + 2, (unsigned long long)edges);
        atomicAdd(stats + 3, (unsigned long long)loads);
    }
}

__global__ __launch_bounds__(kRegionThreads) void k_region_border(TargetIndex ix, float r2, float smoothness_cos, const int32_t *__restrict__ seed,
                                                                  uint32_t *parent)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const uint32_t row_me = (uint32_t)__float_as_int(me.w);
    if (seed[row_me]) return;                                   // seed: flattened already
    const float4 mn = ix.tn[2 * (size_t)i + 1];
    unsigned long long best = ~0ull;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &q, float d2) {
        const uint32_t row_j = (uint32_t)__float_as_int(q.w);
        if (!seed[row_j]) return;
        if (!region_smooth(mn, ix.tn[2 * (size_t)jj + 1], smoothness_cos)) return;
        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)parent[row_j];
        best = key < best ? key : best;
    });
    parent[row_me] = best == ~0ull ? kClusterNoise : (uint32_t)(best & 0xffffffffull);
}

__global__ __launch_bounds__(kRegionThreads) void k_region_smooth(TargetIndex ix, float r2, float smoothness_cos, int32_t *smooth)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const float4 mn = ix.tn[2 * (size_t)i + 1];
    int32_t cnt = 0;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &, float) {
        cnt += region_smooth(mn, ix.tn[2 * (size_t)jj + 1], smoothness_cos) ? 1 : 0;
    });
    smooth[(uint32_t)__float_as_int(me.w)] = cnt;
}

static dim3 region_grid(uint32_t n) { return dim3((n + kRegionThreads - 1) / kRegionThreads); }

void launch_region_seeds(const float *curv_rows, float threshold, uint32_t n, int32_t *seed_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_region_seeds, region_grid(n), dim3(kRegionThreads), 0, s, curv_rows, threshold, n, seed_rows);
}

void launch_region_roots(const TargetIndex &ix, float r2, float smoothness_cos, const int32_t *seed_rows, bool border, uint32_t *parent_rows,
                         unsigned long long *stats, hipStream_t s)
{
    launch_cluster_init(parent_rows, ix.n, s);
    hipLaunchKernelGGL(k_region_union, region_grid(ix.n), dim3(kRegionThreads), 0, s, ix, r2, smoothness_cos, seed_rows, parent_rows, stats);
    launch_cluster_flatten(seed_rows, 1, parent_rows, ix.n, s);
    if (border) hipLaunchKernelGGL(k_region_border, region_grid(ix.n), dim3(kRegionThreads), 0, s, ix, r2, smoothness_cos, seed_rows, parent_rows);
}

void launch_region_smooth_count(const TargetIndex &ix, float r2, float smoothness_cos, int32_t *smooth_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_region_smooth, region_grid(ix.n), dim3(kRegionThreads), 0, s, ix, r2, smoothness_cos, smooth_rows);
}

}  // namespace symmicp
