// kernels_reduce.hip -- the end of a pass: the blocks' partial records summed into the pass's record, and the device-driven loop.
//
//   k_final_reduce   partials -> the record, for the host loop (and the ranks' all-reduce); clears the append lists' counters
//   k_reduce_solve   the same without the host: reduce, loop test, solve (solve_core.h), the next pass's transform
//   k_solve_probe    test entry: solve_core.h on the device
//   k_loop_end, k_publish   what the host waits for
// The accumulating kernels that write the partial records are in kernels_pass.hip; the record's two feedback slots are coded by
// loop_plan.h.
#include "symmicp_internal.h"
#include "solve_core.h"
#include "loop_plan.h"       // the codec of the record's two feedback slots
#pragma clang fp contract(off)

namespace symmicp {

// The append lists' bookkeeping words, read by the 64 lanes of one wave at once (three independent loads per lane):
//   word 0 of shard t   entries in shard t of the work list          -> len      (summed over the shards)
//   word 1 of shard t   pairs searched this pass, counted per shard  -> searched
//   word 2 of a list    appends dropped because a shard was full     -> dropped  (work + retry list; must be 0)
//   word 3 of shard t   searched pairs their neighbourhood settled   -> scans = searched - that: the pairs that reached a scan, a probe or the walk
// Results are valid in every lane.
__device__ __forceinline__ void read_list_words(const uint32_t *cnt, int t, uint32_t &len, uint32_t &searched, uint32_t &dropped, uint32_t &scans)
{
    uint32_t v = cnt[t * kShardStride], u = cnt[t * kShardStride + 1], sc = cnt[t * kShardStride + 3];
    uint32_t d = (t < 2) ? cnt[t * kShards * kShardStride + 2] : 0u;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v += (uint32_t)__shfl_xor((int)v, off, 64);
        u += (uint32_t)__shfl_xor((int)u, off, 64);
        d += (uint32_t)__shfl_xor((int)d, off, 64);
        sc += (uint32_t)__shfl_xor((int)sc, off, 64);
    }
    len = v; searched = u; dropped = d; scans = u > sc ? u - sc : 0u;
}

// ---------------------------------------------------------------------------
// final reduce: partials[nblocks][40] -> 40 doubles.  One 256-thread block per sum: independent loads
// (8 bytes of every block's record: latency-bound, not bandwidth-bound), then a fixed pairwise tree in LDS (deterministic).  Writes the device record
// and, when given, a host-mapped copy (single-GPU read-back without a memcpy).
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_final_reduce(const double *__restrict__ partials, int nblocks,
                                                      double *out_dev, double *out_mapped, uint32_t *ticket,
                                                      unsigned long long seq, uint32_t *counters_to_clear, int keep_nonempty)
{
    __shared__ double red[256];
    const int k = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int j = t; j < nblocks; j += 256) s += partials[(size_t)j * kNSum + k];
    red[t] = s;
    __syncthreads();
#pragma unroll
    for (int off = 128; off > 0; off >>= 1) {
        if (t < off) red[t] += red[t + off];
        __syncthreads();
    }
    __shared__ int last;
    if (t == 0) {
        out_dev[k] = red[0];
        if (out_mapped) out_mapped[k] = red[0];
        // the block that takes the last ticket publishes the sequence number the host spins on
        __threadfence_system();
        last = (atomicAdd(ticket, 1u) == gridDim.x - 1);
    }
    __syncthreads();
    if (last) {
        // Shard counters of the pass's append lists.  The work list's length travels in the record's last slot (unused
        // by the sums; with several GPUs the all-reduce turns it into the total over ranks): it sizes the next pass's
        // walk grid and tells the host whether a pass that skipped the walk has to be repaired.  The counters are
        // zeroed for the next pass -- unless this pass skipped the walk and the list turned out non-empty.
        if (counters_to_clear) {
            __shared__ uint32_t s_len;
            if (t < 64) {
                uint32_t len, searched, dropped, scans;
                read_list_words(counters_to_clear, t, len, searched, dropped, scans);
                if (t == 0) {
                    s_len = len;
                    // the record's spare slots (feedback_encode, loop_plan.h): the list's length and whether appends were dropped (sl_push: must
                    // not happen); the pairs searched this pass (cells_tile) and those of them that reached a scan
                    // (feedback_encode written out: the call schedules this block's instructions differently)
                    const double lenw = (double)len + (dropped ? kListDropped : 0.0), srw = (double)searched + (double)scans * kScanUnit;
                    out_dev[kFeedbackListSlot] = lenw; out_dev[kFeedbackCountSlot] = srw;
                    if (out_mapped) { out_mapped[kFeedbackListSlot] = lenw; out_mapped[kFeedbackCountSlot] = srw; }
                }
            }
            __syncthreads();
            if (t < 2) counters_to_clear[t * kShards * kShardStride + 2] = 0;
            if (t < kShards) { counters_to_clear[t * kShardStride + 1] = 0; counters_to_clear[t * kShardStride + 3] = 0; }
            if (!(keep_nonempty && s_len > 0u))
                for (int c = t; c < 2 * kShards; c += 256) counters_to_clear[c * kShardStride] = 0;      // work list and retry list
        }
        if (t == 0) {
            *ticket = 0;
            if (out_mapped) {
                __threadfence_system();
                reinterpret_cast<volatile unsigned long long *>(out_mapped)[kNSum] = seq;
            }
        }
    }
}

// ---------------------------------------------------------------------------
// k_reduce_solve: the end of one pass and the start of the next WITHOUT the host (device-driven runs of passes).
//   reduce   partials[nblocks][40] -> the pass's record (one 512-thread block: wave w sums the records of blocks w, w+8, ...; fixed order).
//            Sharded runs reduce with k_final_reduce, all-reduce the record over the ranks and call this kernel with
//            REDUCE = false: the record is then read from out_dev.
//   check    a non-empty work list means the fused pass left queries to the tree walk: the pass has to be redone through
//            the separate kernels (LOOP_REDO_PASS, the host takes over)
//   loop     the reference's test `diff > threshold && iters++ < max_iters` (myicp.cpp:123) on the record's slot 33
//   solve    estimateTransformSymm (func.cpp:76-102) from the record: the SAME source as the host solve (solve_core.h),
//            run by one thread, with a guaranteed lower bound of the conditioning (SymSolver::solve, exact_rc = false); anything
//            but a clean solve -- a status other than OK, or a bound at or below 1e-6, so that the exact ratio is above 1e-6 on
//            every pass the device takes -- is handed back to the host's exact form (LOOP_HOST_SOLVE).  transform = increment * transform (myicp.cpp:138); the next pass
//            reads it from the loop state.
// Every pass leaves a LoopRecord in host-mapped memory (sums, increment, transform); the host reads them after the batch.
// ---------------------------------------------------------------------------
template <bool REDUCE>
__global__ __launch_bounds__(512) void k_reduce_solve(const double *__restrict__ partials, int nblocks, double *out_dev, int solve_only, LoopState *loop,
                                                       LoopConfig cfg, LoopRecord *ring, int ring_len, uint32_t *counters_to_clear)
{
    __shared__ double s_sum[kNSum];
    __shared__ uint32_t s_len, s_unc, s_scan;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#ifdef RS_STAMPS
    const unsigned long long ts0 = __builtin_amdgcn_s_memrealtime();
#endif
    // This block is one chain of dependent steps behind a kernel boundary: everything it reads from memory is requested up front, in one
    // round trip (the loop state, the work list's counters, the partial records), instead of one round trip per step (12 -> ~9 us).
    const LoopState ls = *loop;                       // (wave-uniform: scalar loads)
    uint32_t cw0 = 0, cw1 = 0, cw2 = 0, cw3 = 0;      // wave 0: the shard counters (see read_list_words)
    const bool want_counters = !solve_only && REDUCE && counters_to_clear && t < 64;
    if (want_counters) {
        cw0 = counters_to_clear[t * kShardStride]; cw1 = counters_to_clear[t * kShardStride + 1];
        cw2 = (t < 2) ? counters_to_clear[t * kShards * kShardStride + 2] : 0u;
        cw3 = counters_to_clear[t * kShardStride + 3];
    }
    // lane k < 40 of wave w sums slot k of the records of blocks w, w + 8, w + 16, ...: every load is one contiguous 320-byte record,
    // nothing has to cross lanes, the order is fixed.  All loads of a thread are issued before its first sum.
    __shared__ double s_part[8][kNSum];
    double accw = 0.0;
    if (!solve_only && REDUCE && lane < kNSum) {
        if (nblocks <= 512) {
            double c[64];
#pragma unroll
            for (int j = 0; j < 64; j++) { const int b = wave + 8 * j; c[j] = (b < nblocks) ? partials[(size_t)b * kNSum + lane] : 0.0; }
#pragma unroll
            for (int j = 0; j < 64; j++) accw += c[j];
        } else {
            for (int b = wave; b < nblocks; b += 8) accw += partials[(size_t)b * kNSum + lane];
        }
    }
    double rec = 0.0;
    if ((solve_only || !REDUCE) && t < kNSum) rec = out_dev[t];
    if (ls.stop) return;
#ifdef RS_STAMPS
    const unsigned long long tsA = __builtin_amdgcn_s_memrealtime();
#endif
    if (t == 0) { s_len = 0; s_unc = 0; s_scan = 0; }
    if (!solve_only && REDUCE) {
        if (lane < kNSum) s_part[wave][lane] = accw;
        __syncthreads();
        if (t < kNSum) {
            double x = 0.0;
#pragma unroll
            for (int w = 0; w < 8; w++) x += s_part[w][t];
            s_sum[t] = (t < kNAccW) ? x : 0.0;
        }
    } else if (t < kNSum) s_sum[t] = rec;
    __syncthreads();
    if (!solve_only && counters_to_clear) {
        if (REDUCE) {
            if (t < 64) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    cw0 += (uint32_t)__shfl_xor((int)cw0, off, 64);
                    cw1 += (uint32_t)__shfl_xor((int)cw1, off, 64);
                    cw2 += (uint32_t)__shfl_xor((int)cw2, off, 64);
                    cw3 += (uint32_t)__shfl_xor((int)cw3, off, 64);
                }
                if (t == 0) { s_len = cw2 ? 0xFFFFFFFFu : cw0; s_unc = cw1; s_scan = cw1 > cw3 ? cw1 - cw3 : 0u; }      // dropped appends: the host redoes the pass and reports
            }
            if (t < kShards) { counters_to_clear[t * kShardStride + 1] = 0; counters_to_clear[t * kShardStride + 3] = 0; }
            for (int c = t; c < 2 * kShards; c += 512) counters_to_clear[c * kShardStride] = 0;
        } else if (t == 0) {
            // summed over the ranks by the all-reduce (k_final_reduce put them in the record)
            // (feedback_decode written out: the call schedules this block's instructions differently)
            s_len = (s_sum[kFeedbackListSlot] >= kListDropped) ? 0xFFFFFFFFu : (uint32_t)s_sum[kFeedbackListSlot];
            const double sr = s_sum[kFeedbackCountSlot], sc = floor(sr / kScanUnit);
            s_unc = (uint32_t)(sr - sc * kScanUnit); s_scan = (uint32_t)sc;
        }
    }
    __syncthreads();
#ifdef RS_STAMPS
    const unsigned long long ts1 = __builtin_amdgcn_s_memrealtime();
#endif
    // (every thread takes the same decisions from the same words; the record is written by 40 lanes at once, not by one lane 40 times)
    int it = ls.iters;
    if (!solve_only) {
        const uint32_t len = s_len, unc = s_unc, scans = s_scan;
        // a non-empty work list: handled by the straggler stage of this very pass, or the pass has to be redone by the host; dropped
        // appends (0xFFFFFFFF) always go back
        if (cfg.tree && len > 0u && (!cfg.walk_in_loop || len == 0xFFFFFFFFu)) { if (t == 0) { loop->stop = 1; loop->reason = LOOP_REDO_PASS; } return; }
        it += 1;                                                        // this pass is complete
        LoopRecord &r = ring[it % ring_len];
        if (t < kNSum) { const double v = (t >= kNAccW) ? 0.0 : s_sum[t]; r.sums[t] = v; if (REDUCE) out_dev[t] = v; }
        if (t == 0) {
            loop->iters = it;
            r.solved = 0;
            r.searched = (int32_t)unc;
            r.list_len = (int32_t)len; r.scans = (int32_t)scans;
        }
        // many pairs had to be searched again (the cloud moved): the separate kernels do that faster; this pass is complete
        if (cfg.tree && (unc > cfg.uncertified_limit || (cfg.walk_in_loop && len > cfg.list_limit))) { if (t == 0) { loop->stop = 1; loop->reason = LOOP_SLOW; } return; }
    }
    if (t != 0) return;
    // ---- myicp.cpp:123
    const float diff = (float)s_sum[33];
    if (ls.small_step || !((cfg.fixed_iters || diff > cfg.diff_threshold) && it < cfg.max_iters)) {
        loop->stop = 1; loop->reason = LOOP_DONE;
        return;
    }
    // ---- func.cpp:76-102
    symmicp_sums S;
    for (int k = 0; k < kNSum; k++) S.s[k] = (k >= kNAccW) ? 0.0 : s_sum[k];
    float pbar[3], qbar[3], av[3], tv[3], rc = 0.f, Xi[16];
    const int st = solve::solve_mode(cfg.mode, S, cfg.pivot, pbar, qbar, av, tv, &rc, Xi, false);
    if (st != SYMMICP_OK || !(rc > 1e-6f)) { loop->stop = 1; loop->reason = LOOP_HOST_SOLVE; return; }
#ifdef RS_STAMPS
    const unsigned long long ts2 = __builtin_amdgcn_s_memrealtime();
#endif
    float Xn[16];
    solve::mat4_mul(Xi, ls.X, Xn);                                   // myicp.cpp:138
    for (int k = 0; k < 16; k++) loop->X[k] = Xn[k];
    const float *ap = cfg.incremental ? Xi : Xn;
    for (int k = 0; k < 12; k++) loop->Xapply.m[k] = ap[k];
    loop->Xapply.nrm_w = cfg.nrm_w;
    LoopRecord &r = ring[it % ring_len];
    for (int k = 0; k < 16; k++) { r.increment[k] = Xi[k]; r.X[k] = Xn[k]; }
    r.rcond = rc; r.status = st; r.solved = 1;
#ifdef RS_STAMPS2
    r.sums[37] = partials[(size_t)8191 * kNSum]; r.sums[38] = partials[(size_t)8191 * kNSum + 1]; r.sums[39] = partials[(size_t)8191 * kNSum + 2];
#elif defined(RS_STAMPS)
    r.sums[37] = (double)(ts1 - ts0) + 1e-4 * (double)(tsA - ts0); r.sums[38] = (double)(ts2 - ts1); r.sums[39] = (double)(__builtin_amdgcn_s_memrealtime() - ts2);      // 10 ns ticks: load + reduce, bookkeeping + solve, publish
#endif
    if (cfg.eps_rotation > 0.f && cfg.eps_translation > 0.f && !cfg.fixed_iters) {
        // convergence on the increment (engine.cpp, symmicp_align): the pass that applies this increment still runs
        // (solve::small_increment written out: the call turns the two compares into their negations)
        const double tr = ((double)Xi[0] + Xi[5] + Xi[10] - 1.0) * 0.5;
        const double ang = acos(tr > 1.0 ? 1.0 : (tr < -1.0 ? -1.0 : tr));
        const double tn = sqrt((double)Xi[3] * Xi[3] + (double)Xi[7] * Xi[7] + (double)Xi[11] * Xi[11]);
        if (ang < cfg.eps_rotation && tn < cfg.eps_translation) loop->small_step = 1;
    }
}

// Test entry (symmicp_ctx_solve_probe): the device's solve_core.h on a batch of records, one thread per record, with either
// conditioning estimate; then mat4_mul(increment, X_in) as k_reduce_solve composes it.  Off the hot path.
__global__ __launch_bounds__(64) void k_solve_probe(int mode, int exact_rc, const symmicp_sums *__restrict__ sums, int n, const float *pivot,
                                                    const float *__restrict__ X_in, int32_t *status, float *pbar, float *qbar, float *a, float *t,
                                                    float *rcond, float *out16, float *X_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const symmicp_sums S = sums[i];
    float pb[3] = {0.f, 0.f, 0.f}, qb[3] = {0.f, 0.f, 0.f}, av[3] = {0.f, 0.f, 0.f}, tv[3] = {0.f, 0.f, 0.f}, rc = 0.f, Xi[16], Xn[16];
    for (int k = 0; k < 16; k++) Xi[k] = 0.f;
    const bool ex = exact_rc != 0;
    const int st = solve::solve_mode(mode, S, pivot, pb, qb, av, tv, &rc, Xi, ex);
    status[i] = st;
    rcond[i] = rc;
    for (int k = 0; k < 3; k++) { pbar[3 * i + k] = pb[k]; qbar[3 * i + k] = qb[k]; a[3 * i + k] = av[k]; t[3 * i + k] = tv[k]; }
    for (int k = 0; k < 16; k++) out16[16 * (size_t)i + k] = Xi[k];
    if (X_in) {
        solve::mat4_mul(Xi, X_in + 16 * (size_t)i, Xn);
        for (int k = 0; k < 16; k++) X_out[16 * (size_t)i + k] = Xn[k];
    }
}

// last kernel of a batch: copy the loop state where the host can read it and publish the batch's sequence number
__global__ __launch_bounds__(64) void k_loop_end(const LoopState *loop, LoopState *host_copy, unsigned long long *done_flag, unsigned long long seq)
{
    if (threadIdx.x == 0) {
        *host_copy = *loop;
        __threadfence_system();
        *reinterpret_cast<volatile unsigned long long *>(done_flag) = seq;
    }
}

// multi-GPU: after the RCCL all-reduce, copy the record to host-mapped memory and publish the sequence number
__global__ __launch_bounds__(64) void k_publish(const double *__restrict__ sums_dev, double *out_mapped, unsigned long long seq)
{
    if (threadIdx.x < kNSum) out_mapped[threadIdx.x] = sums_dev[threadIdx.x];
    __threadfence_system();
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        reinterpret_cast<volatile unsigned long long *>(out_mapped)[kNSum] = seq;
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_final_reduce(const double *partials, int blocks, double *out_dev, double *out_host_mapped, uint32_t *ticket,
                         unsigned long long seq, uint32_t *counters_to_clear, int keep_nonempty, hipStream_t s)
{
    hipLaunchKernelGGL(k_final_reduce, dim3(kNSum), dim3(256), 0, s, partials, blocks, out_dev, out_host_mapped, ticket, seq,
                       counters_to_clear, keep_nonempty);
}

void launch_reduce_solve(const double *partials, int blocks, double *out_dev, int mode, LoopState *loop, LoopConfig cfg, LoopRecord *ring, int ring_len,
                         uint32_t *counters_to_clear, hipStream_t s)
{
    // mode 0: reduce + check + solve (single GPU); 1: record already in out_dev (after the all-reduce); 2: solve only (start of a batch)
    if (mode == 0) hipLaunchKernelGGL(k_reduce_solve<true>, dim3(1), dim3(512), 0, s, partials, blocks, out_dev, 0, loop, cfg, ring, ring_len, counters_to_clear);
    else hipLaunchKernelGGL(k_reduce_solve<false>, dim3(1), dim3(512), 0, s, partials, blocks, out_dev, mode == 2 ? 1 : 0, loop, cfg, ring, ring_len, counters_to_clear);
}

void launch_solve_probe(int mode, int exact_rc, const symmicp_sums *sums, int n, const float *pivot, const float *X_in, int32_t *status, float *pbar,
                        float *qbar, float *a, float *t, float *rcond, float *out16, float *X_out, hipStream_t s)
{
    if (n > 0) hipLaunchKernelGGL(k_solve_probe, dim3((n + 63) / 64), dim3(64), 0, s, mode, exact_rc, sums, n, pivot, X_in, status, pbar, qbar, a, t, rcond, out16, X_out);
}

void launch_loop_end(const LoopState *loop, LoopState *host_copy, unsigned long long *done_flag, unsigned long long seq, hipStream_t s)
{
    hipLaunchKernelGGL(k_loop_end, dim3(1), dim3(64), 0, s, loop, host_copy, done_flag, seq);
}

void launch_publish(const double *sums_dev, double *out_host_mapped, unsigned long long seq, hipStream_t s)
{
    hipLaunchKernelGGL(k_publish, dim3(1), dim3(64), 0, s, sums_dev, out_host_mapped, seq);
}

}  // namespace symmicp
