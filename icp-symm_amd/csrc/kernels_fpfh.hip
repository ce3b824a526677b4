// kernels_fpfh.hip -- exact fixed-radius neighbour search and Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009;
// PCL FPFHEstimation) on gfx950.  include/symmicp.h defines the arithmetic; tests/_fpfh_ref.py restates it in numpy.
//
// All four kernels run one thread per point in the index's sorted (Morton) order and walk the implicit 8-ary box tree in
// pre-order, as k_normals_knn does, with a FIXED bound r2 instead of a shrinking one (radius_walk, box_walk.h: pruning loses no
// member of { d2 <= r2 }).  The walk meets the leaves, and the points in them, in ascending sorted position: that is the order of
// the radius lists and of the FPFH sums.
//
//   k_radius<false>  count pass:  count[row] = |N(row)|
//   k_radius<true>   fill pass:   the same walk again, writing (row, d2) from offs[row] on (no atomics)
//   k_spfh           pair features of every (point, neighbour), binned into 33 counters per thread that live in LDS, laid out
//                    [bin][thread] (a runtime-indexed register array would go to scratch; a wave's 64 increments hit 64 banks)
//   k_fpfh           the walk again: s[b] += spfh_j[b] * (1 / d2), 33 accumulators in registers (static indexing), the
//                    neighbour's histogram fetched by sorted position (stride 36 floats: nine 16-byte loads), normalised per block
// Per-neighbour work runs inside the walk, with the lanes that meet a neighbour at that step; queueing the neighbours per lane
// and working the queues off wave-wide was measured and gained nothing.
#include "symmicp_internal.h"
#pragma clang fp contract(off)
#include "box_walk.h"             // radius_walk, stage_level_off

namespace symmicp {

constexpr int kFpfhBins = 33;          // 3 features x 11 bins
constexpr int kSpfhStride = 36;        // floats per point of the sorted SPFH array (33 + 3 of padding: float4 loads)
constexpr int kFpfhThreads = 256;
constexpr float kPiF = 3.14159274f;            // fl32(pi)
constexpr float kInv2PiF = 0.159154937f;       // fl32(1 / (2 pi))

__device__ __forceinline__ float f_dot3(float ax, float ay, float az, float bx, float by, float bz)
{
    return (ax * bx + ay * by) + az * bz;
}

template <bool FILL>
__global__ __launch_bounds__(kFpfhThreads) void k_radius(TargetIndex ix, float r2, int32_t *count, const uint32_t *offs, int32_t *rows_out,
                                                         float *d2_out)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const int row_me = __float_as_int(me.w);
    if constexpr (FILL) {
        size_t at = offs[row_me];
        radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t, const float4 &q, float d2) {
            rows_out[at] = __float_as_int(q.w);
            if (d2_out) d2_out[at] = d2;
            at++;
        });
    } else {
        int32_t cnt = 0;
        radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t, const float4 &, float) { cnt++; });
        count[row_me] = cnt;
    }
}

// Pair features of the point (p, n) with its neighbour (q, m) at squared distance d2 (symmicp.h, "FPFH"): returns false for an
// invalid pair, else the three bins (0..10 each).
__device__ __forceinline__ bool pair_bins(float px, float py, float pz, float nx, float ny, float nz, float qx, float qy, float qz, float mx,
                                          float my, float mz, float d2, int &b1, int &b2, int &b3)
{
    float dx = qx - px, dy = qy - py, dz = qz - pz;
    const float f4 = sqrtf(d2);
    const float a1 = f_dot3(nx, ny, nz, dx, dy, dz) / f4;
    const float a2 = f_dot3(mx, my, mz, dx, dy, dz) / f4;
    float ax = nx, ay = ny, az = nz, bx = mx, by = my, bz = mz, f3 = a1;
    if (fabsf(a1) < fabsf(a2)) {
        ax = mx; ay = my; az = mz; bx = nx; by = ny; bz = nz;
        dx = -dx; dy = -dy; dz = -dz;
        f3 = -a2;
    }
    float vx = dy * az - dz * ay, vy = dz * ax - dx * az, vz = dx * ay - dy * ax;
    const float vn = sqrtf(f_dot3(vx, vy, vz, vx, vy, vz));
    vx = vx / vn; vy = vy / vn; vz = vz / vn;
    const float wx = ay * vz - az * vy, wy = az * vx - ax * vz, wz = ax * vy - ay * vx;
    const float f2 = f_dot3(vx, vy, vz, bx, by, bz);
    const float f1 = atan2f(f_dot3(wx, wy, wz, bx, by, bz), f_dot3(ax, ay, az, bx, by, bz));
    if (!(f4 > 0.0f) || !(vn > 0.0f) || !isfinite(f1) || !isfinite(f2) || !isfinite(f3)) return false;
    const float c1 = floorf((11.0f * (f1 + kPiF)) * kInv2PiF);
    const float c2 = floorf((11.0f * (f2 + 1.0f)) * 0.5f);
    const float c3 = floorf((11.0f * (f3 + 1.0f)) * 0.5f);
    b1 = (int)fminf(fmaxf(c1, 0.0f), 10.0f);
    b2 = (int)fminf(fmaxf(c2, 0.0f), 10.0f);
    b3 = (int)fminf(fmaxf(c3, 0.0f), 10.0f);
    return true;
}

// spfh_sorted [n][kSpfhStride] by sorted position (what k_fpfh gathers); spfh_rows [n][33] by original row (may be null);
// count [n] by original row
__global__ __launch_bounds__(kFpfhThreads) void k_spfh(TargetIndex ix, float r2, float *spfh_sorted, float *spfh_rows, int32_t *count)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    __shared__ uint32_t hist[kFpfhBins * kFpfhThreads];      // [bin][thread]
    uint32_t *mine = hist + threadIdx.x;
#pragma unroll
    for (int b = 0; b < kFpfhBins; b++) mine[b * kFpfhThreads] = 0u;
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const float4 mn = ix.tn[2 * (size_t)i + 1];
    int32_t cnt = 0;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &q, float d2) {
        cnt++;
        const float4 qn = ix.tn[2 * (size_t)jj + 1];
        int b1, b2, b3;
        if (pair_bins(me.x, me.y, me.z, mn.x, mn.y, mn.z, q.x, q.y, q.z, qn.x, qn.y, qn.z, d2, b1, b2, b3)) {
            mine[b1 * kFpfhThreads] += 1u;
            mine[(11 + b2) * kFpfhThreads] += 1u;
            mine[(22 + b3) * kFpfhThreads] += 1u;
        }
    });
    const int row_me = __float_as_int(me.w);
    count[row_me] = cnt;
    const float k = (float)cnt;
    float *ds = spfh_sorted + (size_t)i * kSpfhStride;
#pragma unroll
    for (int b = 0; b < kFpfhBins; b++) {
        const float h = cnt > 0 ? (100.0f * (float)mine[b * kFpfhThreads]) / k : 0.0f;
        ds[b] = h;
        if (spfh_rows) spfh_rows[(size_t)row_me * kFpfhBins + b] = h;
    }
    ds[33] = 0.0f; ds[34] = 0.0f; ds[35] = 0.0f;
}

__global__ __launch_bounds__(kFpfhThreads) void k_fpfh(TargetIndex ix, float r2, const float *__restrict__ spfh_sorted, float *fpfh_rows)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    float s[kSpfhStride];
#pragma unroll
    for (int b = 0; b < kSpfhStride; b++) s[b] = 0.0f;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &, float d2) {
        if (!(d2 > 0.0f)) return;
        const float w = 1.0f / d2;
        const float4 *h4 = reinterpret_cast<const float4 *>(spfh_sorted + (size_t)jj * kSpfhStride);
#pragma unroll
        for (int v = 0; v < kSpfhStride / 4; v++) {
            const float4 h = h4[v];
            s[4 * v + 0] = s[4 * v + 0] + h.x * w;
            if (4 * v + 1 < kFpfhBins) {
                s[4 * v + 1] = s[4 * v + 1] + h.y * w;
                s[4 * v + 2] = s[4 * v + 2] + h.z * w;
                s[4 * v + 3] = s[4 * v + 3] + h.w * w;
            }
        }
    });
    float *out = fpfh_rows + (size_t)__float_as_int(me.w) * kFpfhBins;
#pragma unroll
    for (int f = 0; f < 3; f++) {
        float t = 0.0f;
#pragma unroll
        for (int b = 0; b < 11; b++) t = t + s[11 * f + b];
        const bool ok = (t > 0.0f) && isfinite(t);
        const float g = 100.0f / t;
#pragma unroll
        for (int b = 0; b < 11; b++) out[11 * f + b] = ok ? s[11 * f + b] * g : 0.0f;
    }
}

static dim3 fpfh_grid(uint32_t n) { return dim3((n + kFpfhThreads - 1) / kFpfhThreads); }

void launch_radius_count(const TargetIndex &ix, float r2, int32_t *count_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_radius<false>, fpfh_grid(ix.n), dim3(kFpfhThreads), 0, s, ix, r2, count_rows, nullptr, nullptr, nullptr);
}

void launch_radius_fill(const TargetIndex &ix, float r2, const uint32_t *offs_rows, int32_t *rows_out, float *d2_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_radius<true>, fpfh_grid(ix.n), dim3(kFpfhThreads), 0, s, ix, r2, nullptr, offs_rows, rows_out, d2_out);
}

void launch_spfh(const TargetIndex &ix, float r2, float *spfh_sorted, float *spfh_rows, int32_t *count_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_spfh, fpfh_grid(ix.n), dim3(kFpfhThreads), 0, s, ix, r2, spfh_sorted, spfh_rows, count_rows);
}

void launch_fpfh(const TargetIndex &ix, float r2, const float *spfh_sorted, float *fpfh_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_fpfh, fpfh_grid(ix.n), dim3(kFpfhThreads), 0, s, ix, r2, spfh_sorted, fpfh_rows);
}

}  // namespace symmicp
