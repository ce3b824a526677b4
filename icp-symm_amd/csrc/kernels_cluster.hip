// kernels_cluster.hip -- DBSCAN / Euclidean cluster extraction on gfx950 (symmicp_ctx_cluster; include/symmicp.h defines the result,
// DESIGN.md 4 "Clustering" has the measurements; tests/_cluster_ref.py restates it in numpy).
//
// The clusters are the connected components of the radius graph on the CORE rows.  That graph is never stored (1M points with 30
// neighbours each would be 30M edges): every kernel walks the box tree with the exact radius walk of box_walk.h and meets the edges
// of its point on the way.  The core flags are the counts of launch_radius_count (kernels_fpfh.hip) compared with min_points - 1.
//
//   k_cluster_init     parent[row] = row
//   k_cluster_union    one thread per CORE point in sorted order: for every core neighbour at a HIGHER sorted position (each edge once)
//                      whose parent word does not already show it to be in the point's set, cluster::unite -- the concurrent
//                      union-find of cluster_core.h over parent[], indexed by caller row.
//                      The compare-and-swaps go to as many different words as there are roots: nothing is funnelled through one word.
//   k_cluster_flatten  (a launch of its own: every union is done) parent[row] = find(row) for the core rows = the component's lowest row
//   k_cluster_border   one thread per NON-core point: the minimum of (d2 bits << 32 | representative) over its core neighbours; the low
//                      word is the point's root, kNoise when it has no core neighbour.  Core entries of parent[] are only read here and
//                      non-core entries only written, each by its own thread.
// No loop in these kernels waits for another thread (cluster_core.h): a lost compare-and-swap descends and goes on.
#include "symmicp_internal.h"
#pragma clang fp contract(off)
#include "box_walk.h"             // radius_walk, stage_level_off
#include "cluster_core.h"

namespace symmicp {

constexpr int kClusterThreads = 256;

using cluster::AgentOps;      // relaxed agent-scope atomics (cluster_core.h)

__global__ __launch_bounds__(kClusterThreads) void k_cluster_init(uint32_t *parent, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) parent[i] = i;
}

// need = min_points - 1: row j is core iff count[j] >= need.  stats (may be null): [0] += unite calls, [1] += lost compare-and-swaps
__global__ __launch_bounds__(kClusterThreads) void k_cluster_union(TargetIndex ix, float r2, const int32_t *__restrict__ count, int32_t need,
                                                                   uint32_t *parent, unsigned long long *stats)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const uint32_t row_me = (uint32_t)__float_as_int(me.w);
    if (count[row_me] < need) return;
    // top: the row this point's set hung from when last seen -- an ancestor of row_me for good, so the next union starts there and not
    // at row_me again.  ANY value ever read from parent[row_j], however stale (a plain load may be served by this XCD's L2), is an
    // ancestor of row_j for good too: if it is `top` the two rows are in one set already and the edge needs no union.  In a dense
    // neighbourhood that is most edges after the first few.
    uint32_t calls = 0, lost = 0, top = row_me;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &q, float) {
        if (jj <= i) return;
        const uint32_t row_j = (uint32_t)__float_as_int(q.w);
        if (need > 0 && count[row_j] < need) return;
        if (parent[row_j] == top) return;
        calls++;
        top = cluster::unite<AgentOps>(parent, top, row_j, &lost);
    });
    if (stats) {
        atomicAdd(stats + 0, (unsigned long long)calls);
        if (lost) atomicAdd(stats + 1, (unsigned long long)lost);
    }
}

__global__ __launch_bounds__(kClusterThreads) void k_cluster_flatten(const int32_t *__restrict__ count, int32_t need, uint32_t *parent, uint32_t n)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || count[i] < need) return;
    const uint32_t root = cluster::find<AgentOps>(parent, i);
    // (a concurrent halving of this word can only have written an ancestor of i, and loses to this store or leaves the root itself)
    __hip_atomic_store(parent + i, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kClusterThreads) void k_cluster_border(TargetIndex ix, float r2, const int32_t *__restrict__ count, int32_t need,
                                                                    uint32_t *parent)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const uint32_t row_me = (uint32_t)__float_as_int(me.w);
    const int32_t mine = count[row_me];
    if (mine >= need) return;                                   // core: flattened already
    unsigned long long best = ~0ull;
    if (mine > 0) {
        radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t, const float4 &q, float d2) {
            const uint32_t row_j = (uint32_t)__float_as_int(q.w);
            if (count[row_j] < need) return;
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)parent[row_j];
            best = key < best ? key : best;
        });
    }
    parent[row_me] = best == ~0ull ? kClusterNoise : (uint32_t)(best & 0xffffffffull);
}

static dim3 cluster_grid(uint32_t n) { return dim3((n + kClusterThreads - 1) / kClusterThreads); }

void launch_cluster_init(uint32_t *parent_rows, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_cluster_init, cluster_grid(n), dim3(kClusterThreads), 0, s, parent_rows, n);
}

void launch_cluster_flatten(const int32_t *count_rows, int32_t need, uint32_t *parent_rows, uint32_t n, hipStream_t s)
{
    hipLaunchKernelGGL(k_cluster_flatten, cluster_grid(n), dim3(kClusterThreads), 0, s, count_rows, need, parent_rows, n);
}

void launch_cluster_roots(const TargetIndex &ix, float r2, const int32_t *count_rows, int32_t min_points, uint32_t *parent_rows,
                          unsigned long long *stats, hipStream_t s)
{
    const int32_t need = min_points - 1;
    launch_cluster_init(parent_rows, ix.n, s);
    hipLaunchKernelGGL(k_cluster_union, cluster_grid(ix.n), dim3(kClusterThreads), 0, s, ix, r2, count_rows, need, parent_rows, stats);
    launch_cluster_flatten(count_rows, need, parent_rows, ix.n, s);
    if (need > 0) hipLaunchKernelGGL(k_cluster_border, cluster_grid(ix.n), dim3(kClusterThreads), 0, s, ix, r2, count_rows, need, parent_rows);
}

}  // namespace symmicp
