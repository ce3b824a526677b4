// ndt_core.h -- the arithmetic SYMMICP_MODE_NDT shares between host and device (include/symmicp.h, "NDT registration"): the weight
// (symmicp_ndt_weight and k_pass_ndt form it from this one source) and the fp64 eigen-decomposition of a voxel's covariance.
//
// fp32 and fp64 expressions here must stay UNFUSED (the including file is compiled with -ffp-contract=off and carries
// `#pragma clang fp contract(off)`) and keep the association written: tests/_ndt_ref.py restates the weight bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
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

// The cyclic Jacobi of the normals pre-step (kernels_normals.hip, smallest_eigvec3: the same sweeps, rotations and thresholds) on a
// symmetric 3x3 in fp64, keeping all three vectors: lam[r] ascending (ties keep the diagonal's order), vec[r] = the eigenvector of lam[r].
__host__ __device__ inline void ndt_eig3(double a00, double a01, double a02, double a11, double a12, double a22, double lam[3], double vec[3][3])
{
    double A[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}};
    double V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int sweep = 0; sweep < 12; sweep++) {
        const double off = A[0][1] * A[0][1] + A[0][2] * A[0][2] + A[1][2] * A[1][2];
        if (off < 1e-300) break;
#pragma unroll
        for (int pq = 0; pq < 3; pq++) {
            const int p = (pq == 2) ? 1 : 0, q = (pq == 0) ? 1 : 2;
            const double apq = A[p][q];
            if (fabs(apq) < 1e-300) continue;
            const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
            const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
            const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double kp = A[k][p], kq = A[k][q];
                A[k][p] = c * kp - s * kq; A[k][q] = s * kp + c * kq;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double pk = A[p][k], qk = A[q][k];
                A[p][k] = c * pk - s * qk; A[q][k] = s * pk + c * qk;
            }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double kp = V[k][p], kq = V[k][q];
                V[k][p] = c * kp - s * kq; V[k][q] = s * kp + c * kq;
            }
        }
    }
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
