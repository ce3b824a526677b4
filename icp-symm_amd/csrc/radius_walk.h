// radius_walk.h -- the exact fixed-radius walk of the implicit 8-ary box tree, shared by kernels_fpfh.hip and kernels_keypoints.hip.
// One thread per point in the index's sorted (Morton) order walks the tree in pre-order with a FIXED bound r2.  The fp32 box distance
// is a lower bound of the fp32 point distance of every point in the box (subtraction, square and sum are monotone under rounding, and
// both use the association (dx*dx + dy*dy) + dz*dz), so pruning at boxdist2 > r2 loses no member of { d2 <= r2 }.  The walk meets the
// leaves, and the points in them, in ascending sorted position: that is the order of the radius lists and of every sum over them.
// Include after symmicp_internal.h, under #pragma clang fp contract(off).
#pragma once
#include "symmicp_internal.h"

namespace symmicp {

__device__ __forceinline__ float f_dist2(float ax, float ay, float az, float bx, float by, float bz)
{
    float dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float f_boxdist2(float px, float py, float pz, const float4 &lo, const float4 &hi)
{
    float dx = fmaxf(fmaxf(lo.x - px, px - hi.x), 0.0f);
    float dy = fmaxf(fmaxf(lo.y - py, py - hi.y), 0.0f);
    float dz = fmaxf(fmaxf(lo.z - pz, pz - hi.z), 0.0f);
    return (dx * dx + dy * dy) + dz * dz;
}

// visit(jj, q, d2) for every sorted position jj != self with d2(self, jj) <= r2, in ascending jj.  loff: the tree's level
// offsets in LDS (the level is a per-lane value: indexing the kernel argument with it would spill the array).
template <class F>
__device__ __forceinline__ void radius_walk(const TargetIndex &ix, const uint32_t *loff, uint32_t self, float px, float py, float pz,
                                            float r2, F &&visit)
{
    int level = ix.top;
    uint32_t node = 0;
    while (true) {
        const float4 *bx = ix.boxes + 2 * ((size_t)loff[level] + node);
        const float4 lo = bx[0], hi = bx[1];
        const bool hit = (f_boxdist2(px, py, pz, lo, hi) <= r2) && (lo.x <= hi.x);
        if (hit && level > 0) { level--; node <<= 3; continue; }
        if (hit) {
            const uint32_t j0 = node * kLeaf, j1 = min(j0 + kLeaf, ix.n);
            for (uint32_t jj = j0; jj < j1; jj++) {
                const float4 q = ix.tq[jj];
                const float d2 = f_dist2(px, py, pz, q.x, q.y, q.z);
                if (d2 <= r2 && jj != self) visit(jj, q, d2);
            }
        }
        node++;
        while ((node & (kFan - 1)) == 0 && level < ix.top) { node >>= 3; level++; }
        if (level == ix.top && node >= ix.ntop) break;
    }
}

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
