// eig3.h -- the cyclic Jacobi on a symmetric 3x3 in fp64, for host and device: the one eigen-solver behind the normals pre-step
// (smallest_eigvec3, kernels_normals.hip), the ISS saliency (eigvals3, kernels_keypoints.hip) and the NDT voxel map (ndt_eig3,
// ndt_core.h).  Each of them sets up A, calls jacobi3 and selects or sorts in its own way.
// The expressions must stay UNFUSED and keep the association written (tests/_iss_ref.py and tests/_ndt_ref.py restate them).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#pragma clang fp contract(off)

namespace symmicp {

// At most 12 sweeps of the rotations (0,1), (0,2), (1,2) over A, until the off-diagonal is below 1e-300: A's diagonal ends up as the
// eigenvalues.  VEC: V (the identity on entry) collects the rotations, column j the eigenvector of A[j][j]; otherwise V is not touched
// and may be NULL.
// A by reference and both __restrict__: the compiler's first passes see this function on its own, where plain pointers may alias and
// may be null, and the kernels it is inlined into come out with more registers for it (k_normals_knn<false>: 75 VGPRs, one wave per
// SIMD fewer, against 70 this way; k_iss_saliency: 52 against 42).
template <bool VEC>
__host__ __device__ inline void jacobi3(double (&__restrict__ A)[3][3], double (*__restrict__ V)[3])
{
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
            if constexpr (VEC) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const double kp = V[k][p], kq = V[k][q];
                    V[k][p] = c * kp - s * kq; V[k][q] = s * kp + c * kq;
                }
            }
        }
    }
}

}  // namespace symmicp
