// kernels_batch.hip -- batched alignment for gfx950: many small ICP problems in one launch, ONE workgroup per problem, the whole
// loop of symmicp_align inside it (include/symmicp.h, "batched alignment"; DESIGN.md 4, "Batched alignment").
//
// A problem of a few thousand points needs none of what makes an iteration of the big pair cost 33 us whatever its size: its
// brute-force search, its rows, its 40-double record and its 6x6 solve fit in one workgroup, a workgroup barrier stands where the
// kernel boundary stood, and nothing crosses workgroups or returns to the host before the problem has ended.  So there is no grid
// barrier, no cooperative launch, no spinning on memory and no global atomic here; every loop is bounded by a count.
//
// Per pass:
//   search   the problem's target lies in LDS, planar, staged once before the loop (<= 4096 points: 3 x 16 KB; rows past the end are
//            NaN: every comparison with them is false).  Each thread keeps kBatchQ moved queries in registers and sweeps target rows
//            in ascending order with a strict '<' (ties -> lowest row); one 16-byte LDS read serves 4 target rows of one coordinate and
//            every lane reads the same address (broadcast).  A source of more than 2048 rows takes two sweeps.  A source of <= 1024
//            rows leaves threads idle, so the target is split over the spare waves (batch_splits) and the splits are merged by a
//            64-bit integer minimum of (d2 bits << 32 | row) in LDS: order independent, equal d2 resolves to the lowest row.
//   rows     pair_step of pass_rows.h -- the gates and rows of the pass kernels, the same source -- on the winner; its target normal
//            is gathered from global memory (L2-resident).
//   record   wave sums by acc_wave_reduce, then the 8 waves' rows summed through LDS in wave order: a fixed order, so a problem's
//            record does not depend on the batch around it.
//   solve    thread 0: symmicp_align's stop rule and solve_core.h with the host's exact conditioning, then X = increment * X in LDS.
#include "symmicp_internal.h"
#include "device_common.h"
#include "solve_core.h"
#include "pass_rows.h"
#pragma clang fp contract(off)

namespace symmicp {

// loop state of the workgroup's problem (LDS); thread 0 writes, every thread reads `go` after a barrier
struct BatchLoop {
    float X[16];             // cumulative transform: what the next pass applies
    int32_t go;              // 1: another pass follows
    int32_t iters, status, small_step;
    float diff_initial, diff, rcond;
};

// rows of one pair of problem pb: source row i (moved to p), target row j at fp32 squared distance d2
template <int OBJ>
__device__ __forceinline__ void batch_pair(Acc &acc, const HotParams &h, const BatchArgs &a, const BatchProblem &pb, const float *s_tx,
                                           const float *s_ty, const float *s_tz, uint32_t i, float px, float py, float pz, uint32_t j, float d2)
{
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (a.src_nrm) {
        const float *n = a.src_nrm + 3 * ((size_t)pb.src_first + i);
        nx = n[0]; ny = n[1]; nz = n[2];
    }
    const float *tn = a.tgt_nrm + 3 * ((size_t)pb.tgt_first + j);
    const float4 q = make_float4(s_tx[j], s_ty[j], s_tz[j], 0.f), nq = make_float4(tn[0], tn[1], tn[2], 0.f);
    pair_step<OBJ>(acc, h, nx, ny, nz, px, py, pz, q, nq, d2);
}

// Thread 0 after pass `pass`: myicp.cpp:123 and func.cpp:76-102 as symmicp_align runs them, on the record in `sum` and the loop state.
// Not inlined: the solve's registers and arrays are its own, the sweep keeps the kernel's.
__device__ __noinline__ void batch_stop_and_solve(const BatchArgs &a, const BatchProblem &pb, int pass, const double *sum, BatchLoop &L)
{
    const float diff = (float)sum[33];
    int go = 0;
    if (pass == 0) L.diff_initial = diff;
    L.diff = diff;
    if (!L.small_step && (a.fixed_iters || diff > a.diff_threshold) && L.iters < a.max_iters) {
        const int it = L.iters + 1;
        if (it <= 64) a.out[pb.slot].diffs[it - 1] = diff;
        symmicp_sums rec;
        for (int k = 0; k < kNSum; k++) rec.s[k] = sum[k];
        float pbar[3], qbar[3], av[3], tv[3], rc = 0.f, Xi[16], Xn[16];
        const int st = (a.mode == SYMMICP_MODE_P2P) ? solve::solve_p2p(rec, pb.pivot, &rc, Xi)
                                                    : solve::solve_mode(a.mode, rec, pb.pivot, pbar, qbar, av, tv, &rc, Xi, true);
        L.rcond = rc;
        if (st != SYMMICP_OK) L.status = SYMMICP_ERR_DEGENERATE;      // (iters stays: completed iterations)
        else {
            L.iters = it;
            solve::mat4_mul(Xi, L.X, Xn);                             // myicp.cpp:138
            for (int k = 0; k < 16; k++) L.X[k] = Xn[k];
            go = 1;
            // convergence on the increment (symmicp_align): the pass that applies this increment still runs
            if (a.eps_rotation > 0.f && a.eps_translation > 0.f && !a.fixed_iters && solve::small_increment(Xi, a.eps_rotation, a.eps_translation)) L.small_step = 1;
        }
    }
    L.go = go;
}

// OBJ: kObjSym (PAPER, and P2P through HotParams::p2p) or kObjPlane, an instantiation each as in the pass kernels
template <int OBJ>
__global__ __launch_bounds__(kBatchThreads, 4) void k_batch_align(BatchArgs a)
{
    __shared__ __attribute__((aligned(16))) float s_tx[kBatchTile];
    __shared__ __attribute__((aligned(16))) float s_ty[kBatchTile];
    __shared__ __attribute__((aligned(16))) float s_tz[kBatchTile];
    __shared__ unsigned long long s_best[kBatchChunk];
    __shared__ double s_red[(kBatchThreads / 64) * kNSum];
    __shared__ double s_sum[kNSum];
    __shared__ BatchLoop s_loop;

    const BatchProblem pb = a.problems[blockIdx.x];
    const uint32_t t = threadIdx.x;
    const uint32_t ns = pb.src_count, nt = pb.tgt_count, nt4 = (nt + 3u) & ~3u;      // (host: 1 <= ns, nt <= kBatchTile)
    const size_t slot = pb.slot, trace_rows = (size_t)a.max_iters + 1;

    // ---- once per problem: the target into LDS, the merge table, the loop state
    for (uint32_t j = t; j < nt4; j += kBatchThreads) {
        float x = __int_as_float(0x7fc00000), y = 0.f, z = 0.f;
        if (j < nt) { const float *q = a.tgt_xyz + 3 * ((size_t)pb.tgt_first + j); x = q[0]; y = q[1]; z = q[2]; }
        s_tx[j] = x; s_ty[j] = y; s_tz[j] = z;
    }
    for (uint32_t i = t; i < (uint32_t)kBatchChunk; i += kBatchThreads) s_best[i] = ~0ull;
    if (t < 16) s_loop.X[t] = a.guess ? a.guess[16 * slot + t] : ((t % 5u == 0u) ? 1.f : 0.f);
    if (t == 0) { s_loop.go = 0; s_loop.iters = 0; s_loop.status = SYMMICP_OK; s_loop.small_step = 0; s_loop.diff_initial = 0.f; s_loop.diff = 0.f; s_loop.rcond = 0.f; }

    // ---- how this workgroup sweeps: S splits of the target, threads_per_split threads each; split s sweeps rows [lo, hi)
    const uint32_t S = batch_splits(ns), threads_per_split = kBatchThreads / S;
    const uint32_t split = __builtin_amdgcn_readfirstlane(t / threads_per_split), u = t % threads_per_split;      // (whole waves per split)
    const uint32_t rows_per_split = ((nt4 / 4u + S - 1u) / S) * 4u;
    const uint32_t lo = min(split * rows_per_split, nt4), hi = min(lo + rows_per_split, nt4);
    const uint32_t sweeps = (S > 1u) ? 1u : (ns + kBatchChunk - 1u) / kBatchChunk;

    HotParams h;
    h.X.nrm_w = 0.f;
#pragma unroll
    for (int k = 0; k < 3; k++) h.pivot[k] = pb.pivot[k];
    h.max_d2 = a.max_d2; h.min_ndot = a.min_ndot;
    h.p2p = a.mode == SYMMICP_MODE_P2P ? 1 : 0;
    h.loss = SYMMICP_LOSS_NONE; h.loss_scale = 0.f; h.gicp_k = 0.f;
    __syncthreads();

    for (int pass = 0; pass <= a.max_iters; pass++) {      // (pass k applies X_k; the loop state ends it earlier)
#pragma unroll
        for (int k = 0; k < 12; k++) h.X.m[k] = s_loop.X[k];
        Acc acc;
        acc_zero(acc);
        for (uint32_t sweep = 0; sweep < sweeps; sweep++) {
            float px[kBatchQ], py[kBatchQ], pz[kBatchQ], bd[kBatchQ];
            uint32_t bj[kBatchQ];
#pragma unroll
            for (int k = 0; k < kBatchQ; k++) {
                const uint32_t i = sweep * kBatchChunk + k * threads_per_split + u;
                float x = 0.f, y = 0.f, z = 0.f;
                if (i < ns) { const float *p = a.src_xyz + 3 * ((size_t)pb.src_first + i); x = p[0]; y = p[1]; z = p[2]; }
                px[k] = xf_row(h.X.m + 0, x, y, z, 1.0f); py[k] = xf_row(h.X.m + 4, x, y, z, 1.0f); pz[k] = xf_row(h.X.m + 8, x, y, z, 1.0f);
                bd[k] = __int_as_float(0x7f800000); bj[k] = 0xFFFFFFFFu;
            }
            // rows ascend -> strict '<' keeps the lowest row on ties
            for (uint32_t j = lo; j < hi; j += 4u) {
                const float4 qx = *reinterpret_cast<const float4 *>(s_tx + j), qy = *reinterpret_cast<const float4 *>(s_ty + j),
                             qz = *reinterpret_cast<const float4 *>(s_tz + j);
                const float x4[4] = {qx.x, qx.y, qx.z, qx.w}, y4[4] = {qy.x, qy.y, qy.z, qy.w}, z4[4] = {qz.x, qz.y, qz.z, qz.w};
#pragma unroll
                for (int m = 0; m < 4; m++) {
#pragma unroll
                    for (int k = 0; k < kBatchQ; k++) {
                        const float d2 = dist2(px[k], py[k], pz[k], x4[m], y4[m], z4[m]);
                        if (d2 < bd[k]) { bd[k] = d2; bj[k] = j + (uint32_t)m; }
                    }
                }
            }
            // the sweep's winners into LDS: (d2 bits << 32 | row), merged over the splits by a 64-bit integer minimum
#pragma unroll
            for (int k = 0; k < kBatchQ; k++) {
                const uint32_t r = k * threads_per_split + u;
                if (sweep * kBatchChunk + r < ns && bj[k] != 0xFFFFFFFFu)
                    atomicMin(&s_best[r], ((unsigned long long)__float_as_uint(bd[k]) << 32) | (unsigned long long)bj[k]);
            }
            __syncthreads();
            // rows of the sweep's pairs, one row per thread and trip; the entry is reset for the next sweep
            const uint32_t first = sweep * kBatchChunk, count = min(ns - first, (uint32_t)kBatchChunk);
            for (uint32_t r = t; r < count; r += kBatchThreads) {
                const unsigned long long key = s_best[r];
                s_best[r] = ~0ull;
                if (key == ~0ull) continue;
                const uint32_t i = first + r;
                const float *p = a.src_xyz + 3 * ((size_t)pb.src_first + i);
                const float x = p[0], y = p[1], z = p[2];
                batch_pair<OBJ>(acc, h, a, pb, s_tx, s_ty, s_tz, i, xf_row(h.X.m + 0, x, y, z, 1.0f), xf_row(h.X.m + 4, x, y, z, 1.0f),
                                xf_row(h.X.m + 8, x, y, z, 1.0f), (uint32_t)(key & 0xFFFFFFFFull), __uint_as_float((uint32_t)(key >> 32)));
            }
            __syncthreads();
        }
        // ---- the record: wave sums, then the waves in order
        acc_wave_reduce(acc, s_red + (t >> 6) * kNSum);
        __syncthreads();
        if (t < (uint32_t)kNSum) {
            double s = 0.0;
            if (t < (uint32_t)kNAcc) {
#pragma unroll
                for (int w = 0; w < kBatchThreads / 64; w++) s += s_red[w * kNSum + t];
            }
            s_sum[t] = s;
            if (a.trace_sums) a.trace_sums[(slot * trace_rows + (size_t)pass) * kNSum + t] = s;
        }
        if (t < 16 && a.trace_X) a.trace_X[(slot * trace_rows + (size_t)pass) * 16 + t] = s_loop.X[t];
        __syncthreads();
        if (t == 0) batch_stop_and_solve(a, pb, pass, s_sum, s_loop);
        __syncthreads();
        if (!s_loop.go) break;
    }
    // ---- the result, with ordinary stores
    symmicp_batch_result &r = a.out[slot];
    if (t < (uint32_t)kNSum) r.sums.s[t] = s_sum[t];
    if (t < 16) r.transform[t] = s_loop.X[t];
    if (t < 3) r.pivot[t] = pb.pivot[t];
    if (t == 0) {
        r.status = s_loop.status; r.iters = s_loop.iters;
        r.diff_initial = s_loop.diff_initial; r.diff_final = s_loop.diff; r.rcond = s_loop.rcond;
        r.pairs = s_sum[34];
    }
}

void launch_batch_align(const BatchArgs &a, uint32_t n_problems, hipStream_t s)
{
    if (n_problems == 0) return;
    if (a.mode == SYMMICP_MODE_PLANE) hipLaunchKernelGGL(k_batch_align<kObjPlane>, dim3(n_problems), dim3(kBatchThreads), 0, s, a);
    else hipLaunchKernelGGL(k_batch_align<kObjSym>, dim3(n_problems), dim3(kBatchThreads), 0, s, a);
}

}  // namespace symmicp
