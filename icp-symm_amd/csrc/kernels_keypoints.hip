// kernels_keypoints.hip -- Intrinsic Shape Signatures keypoints (Zhong 2009; PCL's ISSKeypoint3D, Open3D's compute_iss_keypoints)
// on gfx950.  include/symmicp.h defines the arithmetic; tests/_iss_ref.py restates it in numpy.
//
// Both stages run one thread per point in the index's sorted (Morton) order over the exact radius walk of box_walk.h, which
// meets the neighbours in ascending sorted position: that is the order of the fp64 sums.
//
//   k_iss_saliency  the walk at the salient radius: e = x_j - x_i in fp32, the six upper entries of the scatter matrix summed in
//                   fp64 (the products of two fp32 values are exact in fp64), C = S / k, its eigenvalues by cyclic Jacobi
//                   rotations (jacobi3 of eig3.h, without the vector matrix), the two
//                   ratio tests as products.  Six fp64 accumulators and the count live in registers.  Writes the saliency by
//                   sorted position (what k_iss_nms gathers: 4 B per neighbour) and, with the count, by original row.
//   k_iss_nms       the walk at the non-maximum radius: a point with s > 0 stays a keypoint unless a neighbour has a larger
//                   saliency, or an equal one and a lower row.  Points with s == 0 do not walk at all; a lane that is beaten stops
//                   reading saliencies (its answer is "no" whatever the count).  One flag word per original row.
//   k_iss_scatter   after the exclusive scan of the flags over rows: rows_out[pos[row]] = row -- ascending rows, no atomics.
#include "symmicp_internal.h"
#pragma clang fp contract(off)
#include "box_walk.h"
#include "eig3.h"

namespace symmicp {

constexpr int kIssThreads = 256;

// eigenvalues of the symmetric 3x3 (fp64) by cyclic Jacobi (jacobi3, eig3.h), without the eigenvector matrix; l1 >= l2 >= l3
__device__ __forceinline__ void eigvals3(double a00, double a01, double a02, double a11, double a12, double a22, double &l1, double &l2,
                                         double &l3)
{
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    jacobi3<false>(A, nullptr);
    double w0 = A[0][0], w1 = A[1][1], w2 = A[2][2], t;
    if (w0 < w1) { t = w0; w0 = w1; w1 = t; }
    if (w1 < w2) { t = w1; w1 = w2; w2 = t; }
    if (w0 < w1) { t = w0; w0 = w1; w1 = t; }
    l1 = w0; l2 = w1; l3 = w2;
}

// s_sorted [n] by sorted position; s_rows [n] and k_rows [n] by original row
__global__ __launch_bounds__(kIssThreads) void k_iss_saliency(TargetIndex ix, float r2, int32_t min_neighbors, double gamma21, double gamma32,
                                                              float *s_sorted, float *s_rows, int32_t *k_rows)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
    int32_t cnt = 0;
    radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t, const float4 &q, float) {
        const float ex = q.x - me.x, ey = q.y - me.y, ez = q.z - me.z;
        const double dx = (double)ex, dy = (double)ey, dz = (double)ez;
        s00 = s00 + dx * dx; s01 = s01 + dx * dy; s02 = s02 + dx * dz;
        s11 = s11 + dy * dy; s12 = s12 + dy * dz; s22 = s22 + dz * dz;
        cnt++;
    });
    float s = 0.0f;
    if (cnt >= min_neighbors) {
        const double k = (double)cnt;
        double l1, l2, l3;
        eigvals3(s00 / k, s01 / k, s02 / k, s11 / k, s12 / k, s22 / k, l1, l2, l3);
        const float l3f = (float)l3;
        if (l2 < gamma21 * l1 && l3 < gamma32 * l2 && l3f > 0.0f) s = l3f;
    }
    const int row_me = __float_as_int(me.w);
    s_sorted[i] = s;
    s_rows[row_me] = s;
    k_rows[row_me] = cnt;
}

// flag_rows [n] by original row: 1 = keypoint
__global__ __launch_bounds__(kIssThreads) void k_iss_nms(TargetIndex ix, float r2, int32_t min_neighbors, const float *__restrict__ s_sorted,
                                                         uint32_t *flag_rows)
{
    __shared__ uint32_t loff[kMaxTreeLevels];
    stage_level_off(ix, loff);
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const int row_me = __float_as_int(me.w);
    const float s_me = s_sorted[i];
    uint32_t keep = 0u;
    if (s_me > 0.0f) {
        int32_t cnt = 0;
        bool beaten = false;
        radius_walk(ix, loff, i, me.x, me.y, me.z, r2, [&](uint32_t jj, const float4 &q, float) {
            cnt++;
            if (beaten) return;
            const float s_j = s_sorted[jj];
            beaten = s_j > s_me || (s_j == s_me && __float_as_int(q.w) < row_me);
        });
        keep = (!beaten && cnt >= min_neighbors) ? 1u : 0u;
    }
    flag_rows[row_me] = keep;
}

__global__ __launch_bounds__(kIssThreads) void k_iss_scatter(const uint32_t *__restrict__ flag_rows, const uint32_t *__restrict__ pos_rows,
                                                             uint32_t n, int32_t *rows_out)
{
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= n) return;
    if (flag_rows[row]) rows_out[pos_rows[row]] = (int32_t)row;
}

static dim3 iss_grid(uint32_t n) { return dim3((n + kIssThreads - 1) / kIssThreads); }

void launch_iss_saliency(const TargetIndex &ix, float r2, int32_t min_neighbors, float gamma21, float gamma32, float *s_sorted, float *s_rows,
                         int32_t *k_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_iss_saliency, iss_grid(ix.n), dim3(kIssThreads), 0, s, ix, r2, min_neighbors, (double)gamma21, (double)gamma32, s_sorted,
                       s_rows, k_rows);
}

void launch_iss_nms(const TargetIndex &ix, float r2, int32_t min_neighbors, const float *s_sorted, uint32_t *flag_rows, hipStream_t s)
{
    hipLaunchKernelGGL(k_iss_nms, iss_grid(ix.n), dim3(kIssThreads), 0, s, ix, r2, min_neighbors, s_sorted, flag_rows);
}

void launch_iss_scatter(const uint32_t *flag_rows, const uint32_t *pos_rows, uint32_t n, int32_t *rows_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_iss_scatter, iss_grid(n), dim3(kIssThreads), 0, s, flag_rows, pos_rows, n, rows_out);
}

}  // namespace symmicp
