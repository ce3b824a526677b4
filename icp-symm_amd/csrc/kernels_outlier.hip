// kernels_outlier.hip -- the hot kernel of statistical outlier removal on gfx950 (symmicp_ctx_statistical_outlier_removal; DESIGN.md 4,
// "Outlier removal"): per point the exact mean distance to its k nearest neighbours, k up to 64.
// One thread per point in the index's sorted (Morton) order walks the implicit 8-ary box tree in pre-order, pruned by the current k-th
// smallest distance (box_walk.h has the proof that this loses no point), as k_normals_knn does (kernels_normals.hip).  That kernel
// keeps (d2, row, position) of k <= 16 candidates in registers; here k runs to 64 and only the DISTANCES matter (ties at the k-th value leave the multiset of values unchanged), so the
// list is one fp32 per slot, in LDS, slot-major: list[slot * blockDim + tid].  A lane's bank is tid % 32 whatever slot it touches, so
// lanes inserting at different depths never conflict.  The list is a max-heap (the root is the k-th smallest so far, the pruning bound);
// it is heap-sorted in place at the end, because the fp64 sum has to run in ascending d2.  Block and LDS are sized from k at launch
// (outlier_block).
#include "symmicp_internal.h"
#pragma clang fp contract(off)
#include "box_walk.h"             // dist2, boxdist2, stage_level_off

namespace symmicp {

constexpr int kOutlierKMax = 64;
constexpr size_t kOutlierListBytes = 32768;      // dynamic LDS of one block at most: four such blocks share a CU's 160 KiB

// threads per block: the largest of 256 / 128 whose list fits kOutlierListBytes (k <= 32: 256, k <= 64: 128)
static int outlier_block(int k)
{
    return (size_t)k * 256 * sizeof(float) <= kOutlierListBytes ? 256 : 128;
}

// The list is a binary max-heap (children of slot j: 2j + 1 and 2j + 2; the root, slot 0, is the largest value kept).  sift_down places v
// at or below slot j of the heap in slots [0, len): about log2(len) levels of two loads and a store, against len / 2 shifts of a
// sorted insertion.
__device__ __forceinline__ void sift_down(float *mine, uint32_t stride, int len, int j, float v)
{
    while (true) {
        int c = 2 * j + 1;
        if (c >= len) break;
        float a = mine[(uint32_t)c * stride];
        if (c + 1 < len) {
            const float b = mine[(uint32_t)(c + 1) * stride];
            if (b > a) { a = b; c++; }
        }
        if (!(a > v)) break;
        mine[(uint32_t)j * stride] = a;
        j = c;
    }
    mine[(uint32_t)j * stride] = v;
}

// d2 < the root: d2 replaces it; returns the new root
__device__ __forceinline__ float heap_replace_root(float *mine, uint32_t stride, int k, float d2)
{
    sift_down(mine, stride, k, 0, d2);
    return mine[0];
}

__global__ __launch_bounds__(256) void k_knn_mean_dist(TargetIndex ix, int k, double *mean_rows)
{
    extern __shared__ float knn_list[];            // [k][blockDim.x]
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const uint32_t stride = blockDim.x;
    float *mine = knn_list + threadIdx.x;
    const float inf = __int_as_float(0x7f800000);
    const float4 me = ix.tq[i];
    const float px = me.x, py = me.y, pz = me.z;

    // The first bound comes from the neighbours on the Morton curve, as k_normals_knn seeds its own: the 2k+1 points around the query
    // in the sorted order (itself left out; there are at least k of them, k <= n - 1) are near it in space, and the k-th smallest of
    // their distances bounds the k-th nearest neighbour's from above.  Only distances are kept here, so unlike k_normals_knn the
    // window's points STAY in the list and the walk skips the window's positions [w0, w1) instead of finding them again: the list is
    // full, and its root a finite bound, before the first box is tested.
    for (int j = 0; j < k; j++) mine[(uint32_t)j * stride] = inf;
    float worst = inf;
    const uint32_t w = 2u * (uint32_t)k + 2u;
    const uint32_t w1 = min(((i > (uint32_t)k) ? i - (uint32_t)k : 0u) + w, ix.n);
    const uint32_t w0 = (w1 >= w) ? w1 - w : 0u;
    for (uint32_t jj = w0; jj < w1; jj++) {
        if (jj == i) continue;
        const float4 q = ix.tq[jj];
        const float d2 = dist2(px, py, pz, q.x, q.y, q.z);
        if (d2 < worst) worst = heap_replace_root(mine, stride, k, d2);
    }

    // The loop of box_walk (box_walk.h), written out.  Through box_walk the compiler emits the same instructions with one scalar move
    // placed ahead of the walk, which pushes the walk 4 bytes on: the two sift loops inside it no longer start on a 64-byte line, and
    // the kernel measured 3 to 7 % slower at every k on 1M points ("Outlier removal").
    int level = ix.top;
    uint32_t node = 0;
    while (true) {
        const float4 *bx = ix.boxes + 2 * ((size_t)loff[level] + node);
        const float4 lo = bx[0], hi = bx[1];
        const bool hit = (boxdist2(px, py, pz, lo, hi) <= worst) && (lo.x <= hi.x);
        if (hit && level > 0) { level--; node <<= 3; continue; }
        if (hit) {
            const uint32_t j0 = node * kLeaf, j1 = min(j0 + kLeaf, ix.n);
            for (uint32_t jj = j0; jj < j1; jj++) {
                const float4 q = ix.tq[jj];
                const float d2 = dist2(px, py, pz, q.x, q.y, q.z);
                if (d2 < worst && jj - w0 >= w1 - w0) worst = heap_replace_root(mine, stride, k, d2);
            }
        }
        node++;
        while ((node & (kFan - 1)) == 0 && level < ix.top) { node >>= 3; level++; }
        if (level == ix.top && node >= ix.ntop) break;
    }

    // heap sort in place: the root goes to the end of the shrinking heap, so the slots end up ascending
    for (int end = k - 1; end > 0; end--) {
        const float top = mine[0], last = mine[(uint32_t)end * stride];
        mine[(uint32_t)end * stride] = top;
        sift_down(mine, stride, end, 0, last);
    }
    // m = (sum of sqrt((double)d2) in ascending d2, from 0.0) / k: fp64 sqrt, add and divide are correctly rounded here
    double s = 0.0;
    for (int j = 0; j < k; j++) s = s + sqrt((double)mine[(uint32_t)j * stride]);
    mean_rows[__float_as_int(me.w)] = s / (double)k;
}

void launch_knn_mean_dist(const TargetIndex &ix, int k, double *mean_rows, hipStream_t s)
{
    static_assert((size_t)kOutlierKMax * 128 * sizeof(float) <= kOutlierListBytes, "the list of the largest k has to fit a 128-thread block");
    const int block = outlier_block(k);
    hipLaunchKernelGGL(k_knn_mean_dist, dim3((ix.n + block - 1) / block), dim3(block), (size_t)k * block * sizeof(float), s, ix, k, mean_rows);
}

}  // namespace symmicp
