// kernels_color.hip -- the per-point attributes of colored ICP (SYMMICP_MODE_COLOR) on gfx950: the intensity gradient on the tangent
// plane (symmicp_ctx_intensity_gradient; include/symmicp.h states its arithmetic) and the permutations of the attributes into the
// order the engine keeps its clouds in.  Off the pass loop: each runs once per cloud.  The rows themselves are acc_color in
// kernels_pass.hip.
#include "symmicp_internal.h"
#pragma clang fp contract(off)

namespace symmicp {

constexpr int kColorKnnMax = 16;

// dst[i] = (gradient, intensity) of the target point the index keeps at position i: its original row rides in tq[i].w (tq == null: the
// planar target of identity pairing, row i)
__global__ __launch_bounds__(256) void k_color_permute_target(const float *__restrict__ intensity, const float *__restrict__ grad3,
                                                              const float4 *__restrict__ tq, uint32_t n, float4 *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t row = tq ? (uint32_t)__float_as_int(tq[i].w) : i;
    if (row >= n) return;                                  // (cannot happen: the index holds a permutation of the rows)
    dst[i] = make_float4(grad3[3 * (size_t)row], grad3[3 * (size_t)row + 1], grad3[3 * (size_t)row + 2], intensity[row]);
}

// dst[i] = intensity of the caller's row behind share position i; `intensity` holds the caller's whole cloud
__global__ __launch_bounds__(256) void k_color_permute_source(const float *__restrict__ intensity, const uint32_t *__restrict__ order,
                                                              uint32_t off, uint32_t n, float *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    dst[i] = intensity[order ? order[i] : off + i];
}

__global__ __launch_bounds__(256) void k_color_unpermute_source(const float *__restrict__ src_int, const uint32_t *__restrict__ order,
                                                                uint32_t n, float *__restrict__ out_rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out_rows[order ? order[i] : i] = src_int[i];
}

// rec_rows[row] = (xyz, intensity) of every point by ORIGINAL row: the neighbour lists of launch_knn name rows
__global__ __launch_bounds__(256) void k_color_rows(const float4 *__restrict__ tq, const float *__restrict__ intensity_rows, uint32_t n,
                                                    float4 *__restrict__ rec_rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 me = tq[i];
    const uint32_t row = (uint32_t)__float_as_int(me.w);
    if (row >= n) return;
    rec_rows[row] = make_float4(me.x, me.y, me.z, intensity_rows[row]);
}

// One thread per sorted point: the moments of its neighbours on its tangent plane and the 3x3 solve, in fp64 (the neighbourhood is at
// most 16 gathers of 16 B; the walk that found it is k_normals_knn<true>'s, run just before: knn_rows [n][k] by original row, in
// ascending (d2, row) order).  Every step as include/symmicp.h writes it, so that a restatement in fp64 gives the same bits.
__global__ __launch_bounds__(256) void k_color_gradient(TargetIndex ix, const float4 *__restrict__ rec_rows, const int32_t *__restrict__ knn_rows,
                                                        int k, float *__restrict__ grad_rows)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ix.n) return;
    const float4 me = ix.tq[i];
    const int row_me = __float_as_int(me.w);
    if ((uint32_t)row_me >= ix.n) return;
    const float4 nm = ix.tn[2 * (size_t)i + 1];
    const double nx = (double)nm.x, ny = (double)nm.y, nz = (double)nm.z;
    const double x0 = (double)me.x, y0 = (double)me.y, z0 = (double)me.z, i0 = (double)rec_rows[row_me].w;
    double m00 = 0, m01 = 0, m02 = 0, m11 = 0, m12 = 0, m22 = 0, r0 = 0, r1 = 0, r2 = 0;
    for (int j = 0; j < k && j < kColorKnnMax; j++) {
        const int row = knn_rows[(size_t)row_me * k + j];
        if (row == row_me || (uint32_t)row >= ix.n) continue;       // the point itself is left out by ROW (a duplicate of it is a member)
        const float4 q = rec_rows[row];
        const double x = (double)q.x - x0, y = (double)q.y - y0, z = (double)q.z - z0;
        const double s = (x * nx + y * ny) + z * nz;
        const double ex = x - s * nx, ey = y - s * ny, ez = z - s * nz;
        const double di = (double)q.w - i0;
        m00 = m00 + ex * ex; m01 = m01 + ex * ey; m02 = m02 + ex * ez;
        m11 = m11 + ey * ey; m12 = m12 + ey * ez; m22 = m22 + ez * ez;
        r0 = r0 + ex * di; r1 = r1 + ey * di; r2 = r2 + ez * di;
    }
    const double mu = ((m00 + m11) + m22) / 2.0;
    const double a00 = m00 + (mu * nx) * nx, a01 = m01 + (mu * nx) * ny, a02 = m02 + (mu * nx) * nz;
    const double a11 = m11 + (mu * ny) * ny, a12 = m12 + (mu * ny) * nz, a22 = m22 + (mu * nz) * nz;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double t = ((a00 + a11) + a22) / 3.0;
    float gx = 0.0f, gy = 0.0f, gz = 0.0f;
    if (det > 1e-12 * ((t * t) * t)) {
        gx = (float)(((c00 * r0 + c01 * r1) + c02 * r2) / det);
        gy = (float)(((c01 * r0 + c11 * r1) + c12 * r2) / det);
        gz = (float)(((c02 * r0 + c12 * r1) + c22 * r2) / det);
    }
    grad_rows[3 * (size_t)row_me] = gx; grad_rows[3 * (size_t)row_me + 1] = gy; grad_rows[3 * (size_t)row_me + 2] = gz;
}

void launch_color_permute_target(const float *intensity, const float *grad3, const float4 *tq, uint32_t n, float4 *dst, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_color_permute_target, dim3((n + 255) / 256), dim3(256), 0, s, intensity, grad3, tq, n, dst);
}

void launch_color_permute_source(const float *intensity, const uint32_t *order, uint32_t off, uint32_t n, float *dst, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_color_permute_source, dim3((n + 255) / 256), dim3(256), 0, s, intensity, order, off, n, dst);
}

void launch_color_unpermute_source(const float *src_int, const uint32_t *order, uint32_t n, float *out_rows, hipStream_t s)
{
    if (n) hipLaunchKernelGGL(k_color_unpermute_source, dim3((n + 255) / 256), dim3(256), 0, s, src_int, order, n, out_rows);
}

void launch_color_gradient(const TargetIndex &ix, const float *intensity_rows, const int32_t *knn_rows, int k, float4 *rec_rows, float *grad_rows,
                           hipStream_t s)
{
    if (!ix.n) return;
    hipLaunchKernelGGL(k_color_rows, dim3((ix.n + 255) / 256), dim3(256), 0, s, ix.tq, intensity_rows, ix.n, rec_rows);
    hipLaunchKernelGGL(k_color_gradient, dim3((ix.n + 255) / 256), dim3(256), 0, s, ix, rec_rows, knn_rows, k, grad_rows);
}

}  // namespace symmicp
