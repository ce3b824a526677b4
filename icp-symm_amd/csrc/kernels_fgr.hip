// kernels_fgr.hip -- Fast Global Registration on gfx950 (include/symmicp.h, "symmicp_ctx_fgr"; DESIGN.md 4, "Fast Global
// Registration"): the tuple test and the whole graduated-non-convexity loop.  tests/_fgr_ref.py restates the arithmetic in numpy.
//
//   k_fgr_tuples     one thread per trial: three SplitMix64 draws of (seed, stream 1), RANSAC's distinctness and EDGE checks
//                    (ransac_core.h, the same source), a flag.  The host scans the flags (kernels_build.hip's exclusive scan) and
//   k_fgr_scatter    writes the draws of the trials whose rank is below max_tuples at 3 * rank: the set comes out in trial order
//                    whatever the launch order was.  No atomic append: its order would leak into the result.
//   k_fgr_optimize   ONE workgroup runs every iteration in one launch, as k_batch_align does for a small ICP problem: there is no
//                    grid barrier, no cooperative launch, no spinning on memory and no global atomic; every loop is bounded by a count.
//                    A set of <= kFgrResident (4096) elements is gathered once into LDS (96 KB, planar) and stays there for the whole
//                    loop; a larger one is streamed from global memory every pass (32 MB at the 2^20-pair cap: L2 / MALL resident).
//                    Registers were the first choice and did not hold: whatever lives across the call of the __noinline__ solve
//                    competes with the sweep's 76 accumulator registers, and with 8 (or 6, or 4) elements per thread the compiler
//                    spilled them and reloaded them in every pass.  From LDS the kernel has no spill and no scratch
//                    instruction of its own; the scratch it reports is the solve's frame.
//                    Per pass: thread-private fp64 accumulators, acc_wave_reduce, the waves' rows summed through LDS in wave order
//                    (a fixed order: the result is bit-reproducible), then thread 0 runs the schedule and the solve
//                    (solve_core.h with the host's exact conditioning) and leaves X and `go` in LDS behind a barrier.
#include "symmicp_internal.h"
#include "device_common.h"
#include "solve_core.h"
#include "pass_rows.h"
#include "ransac_core.h"
#pragma clang fp contract(off)

namespace symmicp {

// ---- tuple test --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fgr_draws(unsigned long long base, uint32_t t, uint32_t m, uint32_t c[3])
{
#pragma unroll
    for (int j = 0; j < 3; j++) c[j] = ransac_draw(base, 3ull * t + j, m);
}

__global__ __launch_bounds__(256) void k_fgr_tuples(const float4 *__restrict__ pq, uint32_t m, uint32_t trials, unsigned long long base,
                                                    float edge2, uint32_t *flags)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > trials) return;
    if (t == trials) { flags[t] = 0u; return; }           // the scan's last word: rank[trials] = the accepted count
    uint32_t c[3];
    fgr_draws(base, t, m, c);
    bool ok = !(c[0] == c[1] || c[1] == c[2] || c[0] == c[2]);
    if (ok) {
        float P[3][3], Q[3][3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const float4 p = pq[2 * (size_t)c[k]], q = pq[2 * (size_t)c[k] + 1];
            P[k][0] = p.x; P[k][1] = p.y; P[k][2] = p.z;
            Q[k][0] = q.x; Q[k][1] = q.y; Q[k][2] = q.z;
        }
        ok = !ransac_edge_fails<float>(P, Q, edge2);
    }
    flags[t] = ok ? 1u : 0u;
}

// rank [trials + 1]: the exclusive scan of the flags
__global__ __launch_bounds__(256) void k_fgr_scatter(const uint32_t *__restrict__ rank, uint32_t m, uint32_t trials, unsigned long long base,
                                                     uint32_t max_tuples, int32_t *set)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= trials) return;
    const uint32_t r = rank[t];
    if (rank[t + 1] == r || r >= max_tuples) return;
    uint32_t c[3];
    fgr_draws(base, t, m, c);
#pragma unroll
    for (int j = 0; j < 3; j++) set[3 * (size_t)r + j] = (int32_t)c[j];
}

void launch_fgr_tuples(const float *pq8, uint32_t m, uint32_t trials, unsigned long long base, float edge2, uint32_t *flags, hipStream_t s)
{
    hipLaunchKernelGGL(k_fgr_tuples, dim3(trials / 256 + 1), dim3(256), 0, s, reinterpret_cast<const float4 *>(pq8), m, trials, base, edge2, flags);
}

void launch_fgr_scatter(const uint32_t *rank, uint32_t m, uint32_t trials, unsigned long long base, uint32_t max_tuples, int32_t *set, hipStream_t s)
{
    hipLaunchKernelGGL(k_fgr_scatter, dim3((trials + 255) / 256), dim3(256), 0, s, rank, m, trials, base, max_tuples, set);
}

// ---- the loop ----------------------------------------------------------------------------------------------------------------
typedef AccN<kNAccW> FgrAcc;

// loop state of the workgroup (LDS); thread 0 writes, every thread reads after a barrier
struct FgrLoop {
    float X[16];             // X_k: what the next pass applies
    float mu;                // ... and its mu
    int32_t go;              // 1: another pass follows
    int32_t iters, status;
};

// one element of the set at (X, mu): three rows of PLANE's form (acc_plane with n = e_x, e_y, e_z, whose fp32 terms are exact:
// p' x e_x = (0, pz, -py), p' x e_y = (-pz, 0, px), p' x e_z = (py, -px, 0); c = d . e) at the line-process weight l, which is returned
__device__ __forceinline__ float fgr_element(FgrAcc &acc, const float *X, float mu, float x, float y, float z, float qx, float qy, float qz)
{
    const float px = xf_row(X + 0, x, y, z, 1.0f), py = xf_row(X + 4, x, y, z, 1.0f), pz = xf_row(X + 8, x, y, z, 1.0f);
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float r2 = (dx * dx + dy * dy) + dz * dz;
    const float t = mu / (mu + r2);
    const float l = t * t;
    const double w = (double)l;
    const double vx[6] = {0.0, (double)pz, (double)(-py), 1.0, 0.0, 0.0};
    const double vy[6] = {(double)(-pz), 0.0, (double)px, 0.0, 1.0, 0.0};
    const double vz[6] = {(double)py, (double)(-px), 0.0, 0.0, 0.0, 1.0};
    acc_row(acc, vx, (double)dx, w);
    acc_row(acc, vy, (double)dy, w);
    acc_row(acc, vz, (double)dz, w);
    acc.v[27] = __builtin_fma(w, (double)px, acc.v[27]); acc.v[28] = __builtin_fma(w, (double)py, acc.v[28]); acc.v[29] = __builtin_fma(w, (double)pz, acc.v[29]);
    acc.v[30] = __builtin_fma(w, (double)qx, acc.v[30]); acc.v[31] = __builtin_fma(w, (double)qy, acc.v[31]); acc.v[32] = __builtin_fma(w, (double)qz, acc.v[32]);
    acc.v[34] += w;
    acc.v[36] += (double)r2;
    acc.v[37] += 1.0;
    return l;
}

// what thread 0's solve step reads of the arguments: scalars by value, so the kernel's argument block never has to live in memory
struct FgrSchedule {
    float delta2, division;
    int32_t iterations, decrease_every, pass_only;
};

// the schedule's step at the top of iteration k
__device__ __forceinline__ float fgr_schedule(const FgrSchedule &c, int k, float mu)
{
    if (k % c.decrease_every == 0 && mu > c.delta2) {
        mu = mu / c.division;
        if (mu < c.delta2) mu = c.delta2;
    }
    return mu;
}

// Thread 0 after pass k: PLANE's solve on the record in `sum`, X_{k+1} = increment * X_k, the schedule's step for pass k + 1.
// Not inlined: the solve's registers and arrays are its own, the sweep keeps the kernel's.
__device__ __noinline__ void fgr_solve_step(FgrSchedule c, int k, const double *sum, FgrLoop *L)
{
    int go = 0;
    if (!c.pass_only) {
        symmicp_sums rec;
        for (int i = 0; i < kNSum; i++) rec.s[i] = sum[i];
        float pbar[3], qbar[3], av[3], tv[3], rc = 0.f, Xi[16], Xn[16];
        const int st = solve::solve_mode(SYMMICP_MODE_PLANE, rec, nullptr, pbar, qbar, av, tv, &rc, Xi, true);
        if (st != SYMMICP_OK) L->status = SYMMICP_ERR_DEGENERATE;      // (iters stays: completed iterations; X stays X_k)
        else {
            solve::mat4_mul(Xi, L->X, Xn);
            for (int i = 0; i < 16; i++) L->X[i] = Xn[i];
            L->iters = k + 1;
            if (k + 1 < c.iterations) { L->mu = fgr_schedule(c, k + 1, L->mu); go = 1; }
        }
    }
    L->go = go;
}

__global__ __launch_bounds__(kFgrThreads) void k_fgr_optimize(FgrArgs a)
{
    __shared__ float s_set[6 * kFgrResident];              // 96 KB of the CU's 160: the one workgroup has the CU to itself
    __shared__ double s_red[(kFgrThreads / 64) * kNSum];
    __shared__ double s_sum[kNSum];
    __shared__ FgrLoop s_loop;

    const uint32_t t = threadIdx.x, M = a.M;
    const bool resident = M <= kFgrResident;
    FgrSchedule sch;
    sch.delta2 = a.delta2; sch.division = a.division;
    sch.iterations = a.iterations; sch.decrease_every = a.decrease_every; sch.pass_only = a.pass_only;

    // ---- once: the set into LDS (planar: element e of coordinate c at c * kFgrResident + e, consecutive lanes on consecutive banks), the
    // loop state
    if (resident) {
        for (uint32_t e = t; e < M; e += kFgrThreads) {
            const size_t row = a.set ? (size_t)a.set[e] : (size_t)e;
            const float4 p = a.pq[2 * row], q = a.pq[2 * row + 1];
            s_set[0 * kFgrResident + e] = p.x; s_set[1 * kFgrResident + e] = p.y; s_set[2 * kFgrResident + e] = p.z;
            s_set[3 * kFgrResident + e] = q.x; s_set[4 * kFgrResident + e] = q.y; s_set[5 * kFgrResident + e] = q.z;
        }
    }
    if (t < 16) s_loop.X[t] = a.X0[t];
    if (t == 0) {
        s_loop.mu = a.pass_only ? a.mu0 : fgr_schedule(sch, 0, a.mu0);
        s_loop.go = 0; s_loop.iters = 0; s_loop.status = SYMMICP_OK;
    }
    if (t < (uint32_t)kNSum) s_sum[t] = 0.0;
    __syncthreads();

    for (int k = 0; k < a.iterations; k++) {               // (pass k applies X_k; the loop state ends it earlier)
        float X[12];
#pragma unroll
        for (int i = 0; i < 12; i++) X[i] = s_loop.X[i];
        const float mu = s_loop.mu;
        FgrAcc acc;
        acc_zero(acc);
        if (resident) {
            for (uint32_t e = t; e < M; e += kFgrThreads) {
                const float l = fgr_element(acc, X, mu, s_set[0 * kFgrResident + e], s_set[1 * kFgrResident + e], s_set[2 * kFgrResident + e],
                                            s_set[3 * kFgrResident + e], s_set[4 * kFgrResident + e], s_set[5 * kFgrResident + e]);
                if (a.weight) a.weight[e] = l;
            }
        } else {
            for (uint32_t e = t; e < M; e += kFgrThreads) {
                const size_t row = a.set ? (size_t)a.set[e] : (size_t)e;
                const float4 p = a.pq[2 * row], q = a.pq[2 * row + 1];
                const float l = fgr_element(acc, X, mu, p.x, p.y, p.z, q.x, q.y, q.z);
                if (a.weight) a.weight[e] = l;
            }
        }
        // ---- the record: wave sums, then the waves in order
        acc_wave_reduce(acc, s_red + (t >> 6) * kNSum);
        __syncthreads();
        if (t < (uint32_t)kNSum) {
            double s = 0.0;
            if (t < (uint32_t)kNAccW) {
#pragma unroll
                for (int w = 0; w < kFgrThreads / 64; w++) s += s_red[w * kNSum + t];
            }
            s_sum[t] = s;
            if (a.sums_trace) a.sums_trace[(size_t)k * kNSum + t] = s;
        }
        if (t < 16 && a.X_trace) a.X_trace[(size_t)k * 16 + t] = s_loop.X[t];
        if (t == 0 && a.mu_trace) a.mu_trace[k] = mu;
        __syncthreads();
        if (t == 0) fgr_solve_step(sch, k, s_sum, &s_loop);
        __syncthreads();
        if (!s_loop.go) break;
    }
    // ---- the result, with ordinary stores
    FgrOut &o = *a.out;
    if (t < (uint32_t)kNSum) o.sums[t] = s_sum[t];
    if (t < 16) {
        o.X[t] = s_loop.X[t];
        if (a.X_trace) a.X_trace[(size_t)s_loop.iters * 16 + t] = s_loop.X[t];
    }
    if (t == 0) { o.mu = s_loop.mu; o.iters = s_loop.iters; o.status = s_loop.status; o.reserved = 0; }
}

void launch_fgr_optimize(const FgrArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_fgr_optimize, dim3(1), dim3(kFgrThreads), 0, s, a);
}

}  // namespace symmicp
