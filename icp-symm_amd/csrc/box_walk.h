// box_walk.h -- the exact walk of the implicit 8-ary box tree over a cloud's Morton order, shared by every per-point cloud operation:
// the k-NN walk (kernels_normals.hip: a shrinking bound; kernels_outlier.hip keeps the same loop written out and says why) and the
// fixed-radius walk (kernels_fpfh.hip, kernels_keypoints.hip, kernels_cluster.hip).  One thread per point walks the tree in pre-order
// and skips every box farther than its bound.
// Why pruning loses no point: the fp32 box distance (boxdist2) is a lower bound of the fp32 point distance (dist2) of every point in
// the box -- subtraction, square and sum are monotone under rounding, and both use the association (dx*dx + dy*dy) + dz*dz
// (device_common.h, the one definition of the pair) -- so a box skipped at boxdist2 > bound holds no point with d2 <= bound.  The walk
// meets the leaves, and the points in them, in ascending sorted position: that is the order of the radius lists and of every sum over them.
// Include after symmicp_internal.h, under #pragma clang fp contract(off).
#pragma once
#include "symmicp_internal.h"
#include "device_common.h"

namespace symmicp {

// point(jj, q, d2) for every sorted position jj of every leaf whose box is within bound(), in ascending jj; bound() is read once per
// node, when that node's box is tested, so it may shrink as points come in.  loff: the tree's level offsets in LDS (stage_level_off;
// the level is a per-lane value: indexing the kernel argument with it would spill the array).
template <class Bound, class Point>
__device__ __forceinline__ void box_walk(const TargetIndex &ix, const uint32_t *loff, float px, float py, float pz, Bound &&bound, Point &&point)
{
    int level = ix.top;
    uint32_t node = 0;
    while (true) {
        const float4 *bx = ix.boxes + 2 * ((size_t)loff[level] + node);
        const float4 lo = bx[0], hi = bx[1];
        const bool hit = (boxdist2(px, py, pz, lo, hi) <= bound()) && (lo.x <= hi.x);
        if (hit && level > 0) { level--; node <<= 3; continue; }
        if (hit) {
            const uint32_t j0 = node * kLeaf, j1 = min(j0 + kLeaf, ix.n);
            for (uint32_t jj = j0; jj < j1; jj++) {
                const float4 q = ix.tq[jj];
                point(jj, q, dist2(px, py, pz, q.x, q.y, q.z));
            }
        }
        node++;
        while ((node & (kFan - 1)) == 0 && level < ix.top) { node >>= 3; level++; }
        if (level == ix.top && node >= ix.ntop) break;
    }
}

// the walk with a FIXED bound: visit(jj, q, d2) for every sorted position jj != self with d2(self, jj) <= r2, in ascending jj
template <class F>
__device__ __forceinline__ void radius_walk(const TargetIndex &ix, const uint32_t *loff, uint32_t self, float px, float py, float pz,
                                            float r2, F &&visit)
{
    box_walk(ix, loff, px, py, pz, [&] { return r2; }, [&](uint32_t jj, const float4 &q, float d2) {
        if (d2 <= r2 && jj != self) visit(jj, q, d2);
    });
}

// every thread of the block calls it once, before any early return: loff[0 .. kMaxTreeLevels) = ix.level_off
__device__ __forceinline__ void stage_level_off(const TargetIndex &ix, uint32_t *loff)
{
    if (threadIdx.x < kMaxTreeLevels) {
        uint32_t v = 0;
#pragma unroll
        for (int l = 0; l < kMaxTreeLevels; l++) if ((int)threadIdx.x == l) v = ix.level_off[l];
        loff[threadIdx.x] = v;
    }
    __syncthreads();
}

}  // namespace symmicp
