// kernels_posegraph.hip -- pose-graph optimisation on gfx950 (include/symmicp.h, "multiway registration"; DESIGN.md 4, "Pose-graph
// optimisation"): one Levenberg-Marquardt iteration per launch, all of it fp64.  tests/_posegraph_ref.py restates the arithmetic in numpy.
//
//   k_posegraph_iteration   ONE workgroup of 256 threads, as k_fgr_optimize: no grid barrier, no cooperative launch, no spinning on
//                           memory, no atomic of any kind; every loop is bounded by a count.  Phases, each behind a workgroup barrier:
//     edges    thread per edge (stride 256): E = X_t^-1 X_s T^-1, e, c, l, the cost term; W e and the two diagonal-block terms go to the
//              edge's two SLOTS of the incidence list (slot_s in the source's row, slot_t in the target's)
//     nodes    thread per node (stride 256): g_i and H_ii = the node's slots added in list order (ascending edge index), the 6x6 Cholesky
//              factor of H_ii + lambda I
//     solve    block-Jacobi PCG on (H + lambda I) d = -g.  The matvec is J^T W J p edge by edge -- per edge w = l L (Ad p_s - p_t), -w to
//              slot_t and Ad^T w to slot_s -- and then per node lambda p_i + its slots in order.  A node's rows of x, r, z, p belong
//              to one thread for the whole launch; only p and the slots cross threads, behind barriers.  Dot products: per-thread
//              partial sums over the thread's nodes in ascending order, a shuffle tree in the wave, the four waves added in order.
//     trial    X' = X Exp(d) per node, then F(X') per edge
//     record   thread 0
//   The vectors and the slots live in device memory, not LDS: five 6 n-double vectors are 240 KB at n = 1024 and the slots 1.5 MB at
//   m = 16384, against 160 KB of LDS; a second, LDS-resident path for small graphs would be a second kernel to test for the same
//   arithmetic.  One workgroup's working set stays in its CU's L1 and the XCD's L2.  Edge data is planar ([component][edge]) so that
//   consecutive lanes read consecutive doubles.
#include "symmicp_internal.h"
#include "posegraph_core.h"
#pragma clang fp contract(off)

namespace symmicp {

namespace {

// ---- reductions over the workgroup: lane 0 of each wave after a shuffle tree, then the waves in order.  Two LDS rows used in turn, so
// one barrier per reduction is enough: a row is written again only behind the barrier of the reduction after this one.
constexpr int kPgWaves = kPgThreads / 64;
constexpr int kPgRedN = 3;

struct PgRed {
    double v[2][kPgWaves][kPgRedN];
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}
__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o, 64));
    return v;
}

// v[k] <- over the workgroup: the sum for k < nsum, the maximum for the rest (N <= kPgRedN values)
template <int N>
__device__ __forceinline__ void block_reduce(PgRed &red, int &par, double (&v)[N], int nsum)
{
    const int t = threadIdx.x, w = t >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
        const double s = k < nsum ? wave_sum(v[k]) : wave_max(v[k]);
        if ((t & 63) == 0) red.v[par][w][k] = s;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
        double s = red.v[par][0][k];
#pragma unroll
        for (int j = 1; j < kPgWaves; j++) s = k < nsum ? s + red.v[par][j][k] : fmax(s, red.v[par][j][k]);
        v[k] = s;
    }
    par ^= 1;
}

struct PgEdge {
    double RT[9], tT[3];
    int32_t s, t;
};

__device__ __forceinline__ void load_edge(const PgArgs &a, uint32_t e, PgEdge &E)
{
    E.s = a.es[e]; E.t = a.et[e];
#pragma unroll
    for (int k = 0; k < 9; k++) E.RT[k] = a.T[(size_t)k * a.m + e];
#pragma unroll
    for (int k = 0; k < 3; k++) E.tT[k] = a.T[(size_t)(9 + k) * a.m + e];
}

__device__ __forceinline__ void load_info(const PgArgs &a, uint32_t e, double *L)
{
#pragma unroll
    for (int k = 0; k < 21; k++) L[k] = a.L[(size_t)k * a.m + e];
}

// y = L x for the symmetric L of the packed upper triangle, terms in ascending column order
__device__ __forceinline__ void sym_mul(const double *L, const double *x, double *y)
{
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = L[pg::tri(i, 0)] * x[0];
#pragma unroll
        for (int j = 1; j < 6; j++) s += L[pg::tri(i, j)] * x[j];
        y[i] = s;
    }
}

__device__ __forceinline__ void mat3_mul(const double *R, const double *x, double *y)
{
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = (R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2];
}
__device__ __forceinline__ void mat3t_mul(const double *R, const double *x, double *y)
{
#pragma unroll
    for (int i = 0; i < 3; i++) y[i] = (R[i] * x[0] + R[3 + i] * x[1]) + R[6 + i] * x[2];
}
__device__ __forceinline__ void cross3(const double *a, const double *b, double *y)
{
    y[0] = a[1] * b[2] - a[2] * b[1];
    y[1] = a[2] * b[0] - a[0] * b[2];
    y[2] = a[0] * b[1] - a[1] * b[0];
}

// y = Ad(T) x = (R w, t x (R w) + R tau)
__device__ __forceinline__ void ad_mul(const PgEdge &E, const double *x, double *y)
{
    double c[3], d[3];
    mat3_mul(E.RT, x, y);
    cross3(E.tT, y, c);
    mat3_mul(E.RT, x + 3, d);
#pragma unroll
    for (int i = 0; i < 3; i++) y[3 + i] = c[i] + d[i];
}
// y = Ad(T)^T x = (R^T (a - t x b), R^T b), x = (a, b)
__device__ __forceinline__ void adt_mul(const PgEdge &E, const double *x, double *y)
{
    double c[3], d[3];
    cross3(E.tT, x + 3, c);
#pragma unroll
    for (int i = 0; i < 3; i++) d[i] = x[i] - c[i];
    mat3t_mul(E.RT, d, y);
    mat3t_mul(E.RT, x + 3, y + 3);
}

// e and c of edge e at the poses X
__device__ __forceinline__ double edge_cost(const double *X, const PgEdge &E, const double *L, double *ev)
{
    double RE[9], Le[6];
    pg::edge_E(X + 12 * (size_t)E.s, X + 12 * (size_t)E.t, E.RT, E.tT, RE, ev + 3);
    pg::log_rot(RE, ev);
    sym_mul(L, ev, Le);
    double c = ev[0] * Le[0];
#pragma unroll
    for (int i = 1; i < 6; i++) c += ev[i] * Le[i];
    return c;
}

// the edge phase of the linearisation: e, c, l, the slots; returns the edge's cost term
__device__ __forceinline__ double edge_build(const PgArgs &a, uint32_t e)
{
    PgEdge E;
    double L[21], ev[6], We[6], y[6];
    load_edge(a, e, E);
    load_info(a, e, L);
    const double c = edge_cost(a.X, E, L, ev);
    const bool unc = a.eunc[e] != 0;
    const double l = unc ? pg::line_weight(a.mu, c) : 1.0;
#pragma unroll
    for (int i = 0; i < 6; i++) a.e[6 * (size_t)e + i] = ev[i];
    a.c[e] = c;
    a.l[e] = l;
#pragma unroll
    for (int k = 0; k < 21; k++) L[k] = l * L[k];                        // W
    sym_mul(L, ev, We);
    const size_t ss = a.slot_s[e], st = a.slot_t[e];
    adt_mul(E, We, y);
#pragma unroll
    for (int i = 0; i < 6; i++) { a.slot_v[6 * ss + i] = y[i]; a.slot_v[6 * st + i] = -We[i]; }
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j < 6; j++) a.slot_h[36 * st + 6 * i + j] = L[pg::tri(i, j)];
    }
    // Ad^T W Ad, column by column: Ad e_j, W of it, Ad^T of that
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double u[6], b[6], col[6];
#pragma unroll
        for (int i = 0; i < 6; i++) u[i] = i == j ? 1.0 : 0.0;
        ad_mul(E, u, b);
        sym_mul(L, b, u);
        adt_mul(E, u, col);
#pragma unroll
        for (int i = 0; i < 6; i++) a.slot_h[36 * ss + 6 * i + j] = col[i];
    }
    return unc ? a.mu * c / (a.mu + c) : c;
}

// position of (i, j), j <= i, in the row-major lower triangle
__device__ __forceinline__ constexpr int lo(int i, int j) { return i * (i + 1) / 2 + j; }

// the lower Cholesky factor of A (row-major 6x6, its lower triangle read) + lambda I, the diagonal stored as its reciprocal; false:
// not finite or not positive definite
__device__ __forceinline__ bool chol6(const double *A, double lambda, double *C)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
            double s = A[6 * i + j] + (i == j ? lambda : 0.0);
#pragma unroll
            for (int k = 0; k < j; k++) s -= C[lo(i, k)] * (j == i ? C[lo(i, k)] : C[lo(j, k)]);
            if (i == j) {
                if (!(s > 0.0) || !(s < 1.7e308)) { ok = false; s = 1.0; }
                C[lo(i, i)] = 1.0 / sqrt(s);
            } else {
                C[lo(i, j)] = s * C[lo(j, j)];
            }
        }
    }
    return ok;
}

// z = (C C^T)^-1 r
__device__ __forceinline__ void chol6_solve(const double *C, const double *r, double *z)
{
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = r[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= C[lo(i, k)] * y[k];
        y[i] = s * C[lo(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= C[lo(k, i)] * z[k];
        z[i] = s * C[lo(i, i)];
    }
}

__device__ __forceinline__ void load6(const double *p, size_t i, double *v)
{
#pragma unroll
    for (int k = 0; k < 6; k++) v[k] = p[6 * i + k];
}
__device__ __forceinline__ void store6(double *p, size_t i, const double *v)
{
#pragma unroll
    for (int k = 0; k < 6; k++) p[6 * i + k] = v[k];
}
__device__ __forceinline__ double dot6(const double *a, const double *b)
{
    double s = a[0] * b[0];
#pragma unroll
    for (int k = 1; k < 6; k++) s += a[k] * b[k];
    return s;
}

}  // namespace

__global__ __launch_bounds__(kPgThreads) void k_posegraph_iteration(PgArgs a)
{
    __shared__ PgRed s_red;
    const uint32_t t = threadIdx.x, n = a.n, m = a.m, ref = (uint32_t)a.ref;
    int par = 0;

    // ---- edges: errors, weights, cost terms, slots
    double fsum = 0.0;
    for (uint32_t e = t; e < m; e += kPgThreads) fsum += edge_build(a, e);
    __syncthreads();

    // ---- nodes: gradient and diagonal block, the slots in list order
    double gmax = 0.0, hmax = 0.0;
    for (uint32_t i = t; i < n; i += kPgThreads) {
        double g[6], H[36];
#pragma unroll
        for (int k = 0; k < 6; k++) g[k] = 0.0;
#pragma unroll
        for (int k = 0; k < 36; k++) H[k] = 0.0;
        if (i != ref) {
            for (uint32_t q = a.off[i]; q < a.off[i + 1]; q++) {
#pragma unroll
                for (int k = 0; k < 6; k++) g[k] += a.slot_v[6 * (size_t)q + k];
#pragma unroll
                for (int k = 0; k < 36; k++) H[k] += a.slot_h[36 * (size_t)q + k];
            }
        }
#pragma unroll
        for (int k = 0; k < 6; k++) { a.g[6 * (size_t)i + k] = g[k]; gmax = fmax(gmax, fabs(g[k])); hmax = fmax(hmax, H[7 * k]); }
#pragma unroll
        for (int k = 0; k < 36; k++) a.hdiag[36 * (size_t)i + k] = H[k];
    }
    double r3[3] = {fsum, gmax, hmax};
    block_reduce(s_red, par, r3, 1);
    const double cost = r3[0];
    gmax = r3[1]; hmax = r3[2];
    const double lambda = a.lambda >= 0.0 ? a.lambda : 1e-5 * hmax;

    // ---- the preconditioner; the solve's start: x = 0, r = -g, z = M^-1 r, p = z
    int bad = 0;
    double bb = 0.0, rz = 0.0;
    for (uint32_t i = t; i < n; i += kPgThreads) {
        double H[36], C[21], r[6], z[6];
#pragma unroll
        for (int k = 0; k < 6; k++) { r[k] = 0.0; z[k] = 0.0; }
        if (i != ref) {
#pragma unroll
            for (int k = 0; k < 36; k++) H[k] = a.hdiag[36 * (size_t)i + k];
            if (!chol6(H, lambda, C)) bad = 1;
#pragma unroll
            for (int k = 0; k < 21; k++) a.chol[21 * (size_t)i + k] = C[k];
#pragma unroll
            for (int k = 0; k < 6; k++) r[k] = -a.g[6 * (size_t)i + k];
            chol6_solve(C, r, z);
            bb += dot6(r, r);
            rz += dot6(r, z);
        }
        store6(a.r, i, r); store6(a.z, i, z); store6(a.p, i, z);
#pragma unroll
        for (int k = 0; k < 6; k++) a.x[6 * (size_t)i + k] = 0.0;
    }
    if (__syncthreads_or(bad)) {
        if (t == 0) {
            PgRecord rec{};
            rec.cost = cost; rec.grad_max = gmax; rec.hdiag_max = hmax; rec.lambda = lambda;
            rec.status = SYMMICP_ERR_DEGENERATE;
            *a.rec = rec;
        }
        return;
    }
    double r2[2] = {bb, rz};
    block_reduce(s_red, par, r2, 2);      // (its barrier also publishes p)
    bb = r2[0]; rz = r2[1];

    // ---- block-Jacobi PCG
    int it = 0;
    double rr = bb;
    if (bb > 0.0) {
        const double stop = (a.cg_tol * a.cg_tol) * bb;
        while (it < a.cg_max) {
            it++;
            // A p, edge by edge: w = l L (Ad p_s - p_t); -w to the target's slot, Ad^T w to the source's
            for (uint32_t e = t; e < m; e += kPgThreads) {
                PgEdge E;
                double L[21], ps[6], pt[6], u[6], w[6], y[6];
                load_edge(a, e, E);
                load_info(a, e, L);
                load6(a.p, (size_t)E.s, ps); load6(a.p, (size_t)E.t, pt);
                ad_mul(E, ps, u);
#pragma unroll
                for (int k = 0; k < 6; k++) u[k] -= pt[k];
                sym_mul(L, u, w);
                const double l = a.l[e];
#pragma unroll
                for (int k = 0; k < 6; k++) w[k] = l * w[k];
                adt_mul(E, w, y);
                const size_t ss = a.slot_s[e], st = a.slot_t[e];
#pragma unroll
                for (int k = 0; k < 6; k++) { a.slot_v[6 * ss + k] = y[k]; a.slot_v[6 * st + k] = -w[k]; }
            }
            __syncthreads();
            double pAp = 0.0;
            for (uint32_t i = t; i < n; i += kPgThreads) {
                if (i == ref) continue;
                double p[6], q[6];
                load6(a.p, i, p);
#pragma unroll
                for (int k = 0; k < 6; k++) q[k] = lambda * p[k];
                for (uint32_t s = a.off[i]; s < a.off[i + 1]; s++) {
#pragma unroll
                    for (int k = 0; k < 6; k++) q[k] += a.slot_v[6 * (size_t)s + k];
                }
                store6(a.z, i, q);                    // (z is free until the preconditioner writes it again below)
                pAp += dot6(p, q);
            }
            double r1[1] = {pAp};
            block_reduce(s_red, par, r1, 1);
            pAp = r1[0];
            if (!(pAp > 0.0)) { it--; break; }        // an information matrix that is not positive semidefinite: keep x (uniform: pAp is the workgroup's)
            const double alpha = rz / pAp;
            double rrp = 0.0, rzp = 0.0;
            for (uint32_t i = t; i < n; i += kPgThreads) {
                if (i == ref) continue;
                double p[6], q[6], x[6], r[6], z[6], C[21];
                load6(a.p, i, p); load6(a.z, i, q); load6(a.x, i, x); load6(a.r, i, r);
#pragma unroll
                for (int k = 0; k < 6; k++) { x[k] += alpha * p[k]; r[k] -= alpha * q[k]; }
#pragma unroll
                for (int k = 0; k < 21; k++) C[k] = a.chol[21 * (size_t)i + k];
                chol6_solve(C, r, z);
                store6(a.x, i, x); store6(a.r, i, r); store6(a.z, i, z);
                rrp += dot6(r, r);
                rzp += dot6(r, z);
            }
            double r2b[2] = {rrp, rzp};
            block_reduce(s_red, par, r2b, 2);
            rr = r2b[0];
            if (rr <= stop) break;
            const double beta = r2b[1] / rz;
            rz = r2b[1];
            for (uint32_t i = t; i < n; i += kPgThreads) {
                if (i == ref) continue;
                double p[6], z[6];
                load6(a.p, i, p); load6(a.z, i, z);
#pragma unroll
                for (int k = 0; k < 6; k++) p[k] = z[k] + beta * p[k];
                store6(a.p, i, p);
            }
            __syncthreads();
        }
    }

    // ---- trial poses and their cost
    double model = 0.0, dmax = 0.0;
    for (uint32_t i = t; i < n; i += kPgThreads) {
        double X[12], Xn[12], d[6], g[6];
#pragma unroll
        for (int k = 0; k < 12; k++) X[k] = a.X[12 * (size_t)i + k];
        if (i != ref) {
            load6(a.x, i, d); load6(a.g, i, g);
            pg::retract(X, d, Xn);
            double s = d[0] * (lambda * d[0] - g[0]);
#pragma unroll
            for (int k = 1; k < 6; k++) s += d[k] * (lambda * d[k] - g[k]);
            model += s;
#pragma unroll
            for (int k = 0; k < 6; k++) dmax = fmax(dmax, fabs(d[k]));
        } else {
#pragma unroll
            for (int k = 0; k < 12; k++) Xn[k] = X[k];
        }
#pragma unroll
        for (int k = 0; k < 12; k++) a.Xtrial[12 * (size_t)i + k] = Xn[k];
    }
    __syncthreads();
    double ftrial = 0.0;
    for (uint32_t e = t; e < m; e += kPgThreads) {
        PgEdge E;
        double L[21], ev[6];
        load_edge(a, e, E);
        load_info(a, e, L);
        const double c = edge_cost(a.Xtrial, E, L, ev);
        const bool unc = a.eunc[e] != 0;
        a.l_trial[e] = unc ? pg::line_weight(a.mu, c) : 1.0;
        ftrial += unc ? a.mu * c / (a.mu + c) : c;
    }
    double r3b[3] = {ftrial, model, dmax};
    block_reduce(s_red, par, r3b, 2);

    if (t == 0) {
        PgRecord rec{};
        rec.cost = cost; rec.cost_trial = r3b[0]; rec.model_decrease = r3b[1];
        rec.grad_max = gmax; rec.delta_max = r3b[2]; rec.hdiag_max = hmax; rec.lambda = lambda;
        rec.cg_residual = bb > 0.0 ? sqrt(rr / bb) : 0.0;
        rec.cg_iterations = it; rec.status = SYMMICP_OK;
        *a.rec = rec;
    }
}

void launch_posegraph_iteration(const PgArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_posegraph_iteration, dim3(1), dim3(kPgThreads), 0, s, a);
}

}  // namespace symmicp
