// ndt_core.h -- the arithmetic SYMMICP_MODE_NDT shares between host and device (include/symmicp.h, "NDT registration"): the weight
// (symmicp_ndt_weight and k_pass_ndt form it from this one source) and the fp64 eigen-decomposition of a voxel's covariance.
//
// fp32 and fp64 expressions here must stay UNFUSED (the including file is compiled with -ffp-contract=off and carries
// `#pragma clang fp contract(off)`) and keep the association written: tests/_ndt_ref.py restates the weight bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "eig3.h"
#pragma clang fp contract(off)

namespace symmicp {

// exp(x) on (-64, 0] in plain fp32 arithmetic (Cephes' expf: Cody-Waite reduction by ln 2 in two pieces, a degree-5 polynomial, one
// exact scaling); 0 at and below -64 and for NaN, exp(0) above 0.  No expf, no __expf: every op is an IEEE fp32 op numpy has too.
__host__ __device__ inline float ndt_weight(float x)
{
    if (!(x > -64.0f)) return 0.0f;
    if (x > 0.0f) x = 0.0f;
    const float k = rintf(x * 1.44269504f);
    const float r = (x - k * 0.693359375f) - k * (-2.12194440e-4f);
    float p = 1.9875691500e-4f;
    p = p * r + 1.3981999507e-3f;
    p = p * r + 8.3334519073e-3f;
    p = p * r + 4.1665795894e-2f;
    p = p * r + 1.6666665459e-1f;
    p = p * r + 5.0000001201e-1f;
    const float y = (p * (r * r) + r) + 1.0f;
    return ldexpf(y, (int)k);
}

// The eigen-decomposition of a symmetric 3x3 in fp64 (jacobi3, eig3.h), keeping all three vectors: lam[r] ascending (ties keep the
// diagonal's order), vec[r] = the eigenvector of lam[r].
__host__ __device__ inline void ndt_eig3(double a00, double a01, double a02, double a11, double a12, double a22, double lam[3], double vec[3][3])
{
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    jacobi3<true>(A, V);
    double w0 = A[0][0], w1 = A[1][1], w2 = A[2][2];
    double v0[3] = {V[0][0], V[1][0], V[2][0]}, v1[3] = {V[0][1], V[1][1], V[2][1]}, v2[3] = {V[0][2], V[1][2], V[2][2]};
    // a stable three-element sort by static swaps (no indexed registers)
#define NDT_SWAP(wa, va, wb, vb)                                                                              \
    if (wb < wa) {                                                                                            \
        const double tw = wa; wa = wb; wb = tw;                                                               \
        for (int k = 0; k < 3; k++) { const double tv = va[k]; va[k] = vb[k]; vb[k] = tv; }                   \
    }
    NDT_SWAP(w0, v0, w1, v1)
    NDT_SWAP(w1, v1, w2, v2)
    NDT_SWAP(w0, v0, w1, v1)
#undef NDT_SWAP
    lam[0] = w0; lam[1] = w1; lam[2] = w2;
#pragma unroll
    for (int k = 0; k < 3; k++) { vec[0][k] = v0[k]; vec[1][k] = v1[k]; vec[2][k] = v2[k]; }
}

}  // namespace symmicp
