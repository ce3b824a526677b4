// kernels_pass.hip -- the accumulating kernels of the symmetric-ICP loop for gfx950: every kernel that turns pairs into a record.
//
// One "pass" = everything the reference does per trip of myicp.cpp:123-142 that touches all N points.  Per point:
//   applyTransform (func.cpp:104-121)  -> transform p, n_p on the fly (optionally write back)
//   calculateMatrixNotation (func.cpp:43-60) -> M_i, N_i, c_i in fp32 registers, never stored
//   the O(N) parts of solveLLS / means / evalDiff (func.cpp:19-32,64-73,85)
//                                     -> 37 fp64 sums per thread -> wave64 DPP sum
//                                        -> LDS across the 4 waves -> one record per block (pass_rows.h).
// The kernels differ in where a point's pair comes from:
//   k_pass_identity     row i of the target (what the reference does)
//   k_pass_indexed      the brute-force search's result (k_nn_brute, kernels_search.hip)
//   k_accumulate        the pairs k_search_cells / k_search_walk stored (kernels_search.hip); k_accumulate_list: the work list's only
//   k_pass_fused        search and record in one kernel, for a converged alignment: certificates, and cells_tile (pair_search.h) for the rest
//   k_pass_certified    the same with certificates alone
// The records are summed by kernels_reduce.hip.  The path is HBM/L2-bound integer+fp32 work; no MFMA.
//
// fp32 expressions here must stay UNFUSED (compiled with -ffp-contract=off) and
// keep the association written: the CPU oracle uses the same expressions, so
// nearest-neighbour choices compare bit for bit.
#include <type_traits>
#include "symmicp_internal.h"
#include "device_common.h"
#include "pass_rows.h"     // the accumulators, the rows of a pair, the gates and the sums (shared with kernels_batch.hip and kernels_ndt.hip)
#include "pair_search.h"   // the certificates and cells_tile (shared with kernels_search.hip)
#pragma clang fp contract(off)

namespace symmicp {

// ---------------------------------------------------------------------------
// pass, identity pairing (what the reference does: myicp.cpp:130)
// Streaming: 48 B/point read (+24 B/point written with write-back).
// ---------------------------------------------------------------------------
// VEC = 4: each thread handles 4 consecutive points per step with 16-byte loads/stores from the planar
// arrays (needs n, the target offset and the array lengths to be multiples of 4 so every column stays
// 16-byte aligned); VEC = 1 is the general form.
// OBJ: the record (acc_obj).  The PLANE instantiations read the source normals only to write them back or to gate on them.
template <int VEC, bool W, int OBJ, bool T>
__global__ __launch_bounds__(kPassThreads) void k_pass_identity(PassArgs a_in, CloudSoA tgt)
{
    if (a_in.loop && a_in.loop->stop) return;
    PassArgs a = a_in;
    if (a_in.loop) a.X = a_in.loop->Xapply;        // device-driven loop: the transform k_reduce_solve left behind
    AccT<W> acc; acc_zero(acc);
    const HotParams h = hot_params(a);
    const uint32_t tau = T ? a.rej.ws[kRejectTauWord] : 0u;
    const bool need_n = reads_src_normals<OBJ>(a.writeback, a.min_ndot);
    const uint32_t stride = gridDim.x * blockDim.x * VEC;
    for (uint32_t i0 = (blockIdx.x * blockDim.x + threadIdx.x) * VEC; i0 < a.n; i0 += stride) {
        float x[VEC], y[VEC], z[VEC], nx[VEC], ny[VEC], nz[VEC], qx[VEC], qy[VEC], qz[VEC], qnx[VEC], qny[VEC], qnz[VEC];
        const uint32_t j0 = a.tgt_offset + i0;
        if (VEC == 4) {
            *reinterpret_cast<float4 *>(x) = *reinterpret_cast<const float4 *>(a.in.x + i0);
            *reinterpret_cast<float4 *>(y) = *reinterpret_cast<const float4 *>(a.in.y + i0);
            *reinterpret_cast<float4 *>(z) = *reinterpret_cast<const float4 *>(a.in.z + i0);
            if (need_n) {
                *reinterpret_cast<float4 *>(nx) = *reinterpret_cast<const float4 *>(a.in.nx + i0);
                *reinterpret_cast<float4 *>(ny) = *reinterpret_cast<const float4 *>(a.in.ny + i0);
                *reinterpret_cast<float4 *>(nz) = *reinterpret_cast<const float4 *>(a.in.nz + i0);
            } else {
#pragma unroll
                for (int k = 0; k < VEC; k++) nx[k] = ny[k] = nz[k] = 0.0f;
            }
            *reinterpret_cast<float4 *>(qx) = *reinterpret_cast<const float4 *>(tgt.x + j0);
            *reinterpret_cast<float4 *>(qy) = *reinterpret_cast<const float4 *>(tgt.y + j0);
            *reinterpret_cast<float4 *>(qz) = *reinterpret_cast<const float4 *>(tgt.z + j0);
            *reinterpret_cast<float4 *>(qnx) = *reinterpret_cast<const float4 *>(tgt.nx + j0);
            *reinterpret_cast<float4 *>(qny) = *reinterpret_cast<const float4 *>(tgt.ny + j0);
            *reinterpret_cast<float4 *>(qnz) = *reinterpret_cast<const float4 *>(tgt.nz + j0);
        } else {
            x[0] = a.in.x[i0]; y[0] = a.in.y[i0]; z[0] = a.in.z[i0];
            if (need_n) { nx[0] = a.in.nx[i0]; ny[0] = a.in.ny[i0]; nz[0] = a.in.nz[i0]; }
            else nx[0] = ny[0] = nz[0] = 0.0f;
            qx[0] = tgt.x[j0]; qy[0] = tgt.y[j0]; qz[0] = tgt.z[j0];
            qnx[0] = tgt.nx[j0]; qny[0] = tgt.ny[j0]; qnz[0] = tgt.nz[j0];
        }
        float px[VEC], py[VEC], pz[VEC], npx[VEC], npy[VEC], npz[VEC], d2[VEC];
#pragma unroll
        for (int k = 0; k < VEC; k++) {
            px[k] = xf_row(a.X.m + 0, x[k], y[k], z[k], 1.0f); py[k] = xf_row(a.X.m + 4, x[k], y[k], z[k], 1.0f);
            pz[k] = xf_row(a.X.m + 8, x[k], y[k], z[k], 1.0f);
            npx[k] = xf_row(a.X.m + 0, nx[k], ny[k], nz[k], a.X.nrm_w); npy[k] = xf_row(a.X.m + 4, nx[k], ny[k], nz[k], a.X.nrm_w);
            npz[k] = xf_row(a.X.m + 8, nx[k], ny[k], nz[k], a.X.nrm_w);
            d2[k] = dist2(px[k], py[k], pz[k], qx[k], qy[k], qz[k]);
        }
        if (a.writeback) {
            if (VEC == 4) {
                *reinterpret_cast<float4 *>(a.out.x + i0) = *reinterpret_cast<float4 *>(px);
                *reinterpret_cast<float4 *>(a.out.y + i0) = *reinterpret_cast<float4 *>(py);
                *reinterpret_cast<float4 *>(a.out.z + i0) = *reinterpret_cast<float4 *>(pz);
                *reinterpret_cast<float4 *>(a.out.nx + i0) = *reinterpret_cast<float4 *>(npx);
                *reinterpret_cast<float4 *>(a.out.ny + i0) = *reinterpret_cast<float4 *>(npy);
                *reinterpret_cast<float4 *>(a.out.nz + i0) = *reinterpret_cast<float4 *>(npz);
            } else {
                a.out.x[i0] = px[0]; a.out.y[i0] = py[0]; a.out.z[i0] = pz[0];
                a.out.nx[i0] = npx[0]; a.out.ny[i0] = npy[0]; a.out.nz[i0] = npz[0];
            }
        }
        if (a.d2_out) {
            if (VEC == 4) *reinterpret_cast<float4 *>(a.d2_out + i0) = *reinterpret_cast<float4 *>(d2);
            else a.d2_out[i0] = d2[0];
        }
#pragma unroll
        for (int k = 0; k < VEC; k++)
            pair_step_at<OBJ, T>(acc, h, a, i0 + k, j0 + k, make_float3(nx[k], ny[k], nz[k]), make_float3(px[k], py[k], pz[k]),
                                 make_float4(qx[k], qy[k], qz[k], 0.0f), make_float4(qnx[k], qny[k], qnz[k], 0.0f), d2[k], tau);
    }
    acc_block_reduce_store(acc, a.partials, blockIdx.x);
}

// ---------------------------------------------------------------------------
// pass, pairs given by a previous search kernel (brute force): best64[i] holds
// (d2 bits << 32 | target row).  Target rows are gathered as float4.
// ---------------------------------------------------------------------------
template <bool W, int OBJ, bool T>
__global__ __launch_bounds__(kPassThreads) void k_pass_indexed(PassArgs a, const float4 *__restrict__ tn)
{
    AccT<W> acc; acc_zero(acc);
    const HotParams h = hot_params(a);
    const uint32_t tau = T ? a.rej.ws[kRejectTauWord] : 0u;
    const bool need_n = reads_src_normals<OBJ>(a.writeback, a.min_ndot);
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const SrcRow r = load_src_row(a.in, i, need_n);
        const float3 p = transform_point(a.X, r.p);
        if (a.writeback) write_back(a, i, p, r.n);
        unsigned long long b = a.best64[i];
        uint32_t j = (uint32_t)(b & 0xFFFFFFFFull);
        float d2 = __uint_as_float((uint32_t)(b >> 32));
        bool ok = (b != ~0ull);
        if (a.pos_out) a.pos_out[i] = ok ? (int32_t)j : -1;
        if (a.d2_out) a.d2_out[i] = ok ? d2 : __int_as_float(0x7f800000);
        if (!ok) continue;
        if (a.max_d2 > 0.0f && d2 > a.max_d2) continue;                  // (pair_step's gate, ahead of the gather it saves)
        if (T && a.rej.claim != kClaimNone && a.rej.keys[i] == 0xFFFFFFFFu) continue;      // one-to-one: the row lost its target (or is no candidate)
        pair_step_at<OBJ, T>(acc, h, a, i, j, r.n, p, tn[2 * (size_t)j], tn[2 * (size_t)j + 1], d2, tau);      // one 32-byte pair record
    }
    acc_block_reduce_store(acc, a.partials, blockIdx.x);
}

// ---------------------------------------------------------------------------
// k_pass_fused: the whole pass of a CONVERGED alignment in one kernel.  Once ICP has converged nearly every pair is
// certified, so the pass is a stream: per point 12 B position + 12 B normal + the pair's own 32-byte record copy + the
// 16-byte certificate, all coalesced; certified pairs are accumulated on the spot (rows of func.cpp:51-58, 37 fp64 sums).
// Separate search and accumulate kernels read the source twice and cost two launches.
//   stream   grid-stride over tiles of 256 points: certificate test (the expressions of cells_tile, phase 1: single, then the
//            neighbourhood); a pair that fails both goes to a list in LDS
//   scan     the listed queries run through cells_tile, 256 at a time: exact scan, new pair, certificate and record copy
//   settle   the listed queries once more: those that now have a pair are accumulated from their fresh record copy
// A query the scan has to hand to the tree walk is appended to the work list and NOT accumulated (its record copy is
// marked stale): the pass's record then reports a non-empty list and whoever drives the loop repeats the pass through
// the separate kernels.  So does a block whose LDS list overflows (the early passes of an alignment: they keep the
// separate kernels).  The transform comes from the device-resident loop state when there is one (a.loop): passes can be
// enqueued back to back without the host (k_reduce_solve writes the next transform); a stopped loop returns at once.
// ---------------------------------------------------------------------------
constexpr int kFusedList = 2048;      // (room for the uncertified points of several 256-point tiles between two flushes)

// (k_pass_fused holds what its streaming loop needs of its arguments in vector registers: in_vgpr, pass_rows.h)
typedef float f32x4_t __attribute__((ext_vector_type(4)));
template <typename T>
__device__ __forceinline__ __attribute__((address_space(1))) T *gcol(unsigned long long base)      // a global-memory pointer from its address (an opaque pointer would load as `flat`)
{
    return (__attribute__((address_space(1))) T *)base;
}
__device__ __forceinline__ float4 as_float4(f32x4_t v) { return make_float4(v.x, v.y, v.z, v.w); }

#ifndef FUSED_WAVES
#define FUSED_WAVES 2
#endif
#ifndef COMPACT_WAVES
#define COMPACT_WAVES 5
#endif
// ACC = true: the fused pass described above.  ACC = false: only the search part (stream + scan), for the passes of an alignment
// that is still settling: the separate k_search_cells lets every block of 256 queries pay the latency of the whole scan machinery
// for the dozen of them that need it; here a block streams several tiles and scans the failures 256 at a time (the walk and
// k_accumulate follow as usual).  No normals, no record copies read, no sums: registers for 5 waves per SIMD.
// W (with ACC): the weighted record of a robust loss.  OBJ (with ACC): the record (acc_obj); PLANE's reads source normals only for
// min_normal_dot.
template <bool ACC, bool W, int OBJ>
__global__ __launch_bounds__(kPassThreads, ACC ? FUSED_WAVES : COMPACT_WAVES) void k_pass_fused(PassArgs a, TargetIndex ix, WorkLists wl)
{
    static_assert(ACC || !W, "the search-only form has no sums to weight");
    static_assert(ACC || OBJ == kObjSym, "the search-only form has no rows");
    const bool need_n = reads_src_normals<OBJ>(false, a.min_ndot);      // (no write-back here)
    constexpr int kList = ACC ? kFusedList : kFusedList / 2;      // (the search-only form keeps 5 workgroups per CU: its tile is 256 points)
    __shared__ uint32_t s_list[kList];
    __shared__ uint32_t s_cnt, s_total, s_hood;      // (s_hood: listed pairs their neighbourhood settled)
    __shared__ unsigned long long s_col[ACC ? 10 : 1];      // base addresses of the streamed columns (read back at the top of every tile: see in_vgpr)
    // device-driven loop: stop flag and transform come from device memory, written by the kernel just before this one -- a cold round trip.
    // They are requested here and first LOOKED AT behind the first tile's loads (which do not depend on them): one round trip, not two
    // (behind the barrier: scalar loads and LDS stores share a counter, and the barrier waits for it)
    AccT<W> acc;
    if (ACC) acc_zero(acc);
    if (threadIdx.x == 0) { s_cnt = 0; s_total = 0; s_hood = 0; }
    if (ACC && threadIdx.x == 0) {
        s_col[0] = (unsigned long long)a.in.x; s_col[1] = (unsigned long long)a.in.y; s_col[2] = (unsigned long long)a.in.z;
        s_col[3] = (unsigned long long)a.in.nx; s_col[4] = (unsigned long long)a.in.ny; s_col[5] = (unsigned long long)a.in.nz;
        s_col[6] = (unsigned long long)a.pairrec; s_col[7] = (unsigned long long)a.cert;
    }
    __syncthreads();
    int stop = 0;
    HotParams h;
    if (ACC && a.loop) {
        stop = a.loop->stop;
        loop_transform(h, a.loop);      // (arrives in VGPRs, behind the first tile's loads like the flag)
    } else if (ACC) {
#pragma unroll
        for (int k = 0; k < 12; k++) h.X.m[k] = in_vgpr(a.X.m[k]);
        h.X.nrm_w = in_vgpr(a.X.nrm_w);
    } else {
        // (the search-only form runs at 5 waves per SIMD, 96 registers: no room for resident copies)
        h.X = a.X;
        if (a.loop) { stop = a.loop->stop; h.X = a.loop->Xapply; }
    }
    const Affine &X = h.X;
#pragma unroll
    for (int k = 0; k < 3; k++) h.pivot[k] = ACC ? in_vgpr(a.pivot[k]) : a.pivot[k];
    h.max_d2 = ACC ? in_vgpr(a.max_d2) : a.max_d2; h.min_ndot = ACC ? in_vgpr(a.min_ndot) : a.min_ndot;
    h.p2p = a.p2p;
    if (W) { h.loss = a.loss; h.loss_scale = in_vgpr(a.loss_scale); }
    if (OBJ == kObjGicp) h.gicp_k = in_vgpr(a.gicp_k);
#ifdef RS_STAMPS2
    const unsigned long long fs0 = __builtin_amdgcn_s_memrealtime();
    unsigned long long fs1 = 0;
#endif
    const uint32_t shard = blockIdx.x & (kShards - 1);

    // the listed queries (their single certificate has failed): (ACC) first the neighbourhood certificate -- the winner is a member of the set
    // the last scan kept: decided among 8 gathers, accumulated on the spot -- then the exact scan of the others 256 at a time, then (ACC) those
    // that now have a pair are accumulated from their fresh record copy.  (The neighbourhood test used to sit in the streaming loop; with 4
    // points per thread there it is 4 inlined copies and the kernel spills.)
    auto flush = [&]() {
        const uint32_t cnt = s_cnt;
        if (ACC && a.certk) {
            for (uint32_t base = 0; base < cnt; base += kPassThreads) {
                const uint32_t e = base + threadIdx.x;
                if (e >= cnt) continue;
                const uint32_t i = s_list[e];
                const float4 ce = a.cert[i];
                if (!(__float_as_uint(ce.w) & 1u)) continue;
                const float4 q = a.pairrec[2 * (size_t)i], nq = a.pairrec[2 * (size_t)i + 1];
                const int32_t pk = a.pos_prev[i];
                if (nq.w != 0.0f || (uint32_t)pk >= ix.n) continue;
                const float3 p = transform_point(X, make_float3(a.in.x[i], a.in.y[i], a.in.z[i]));
                const float d2 = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
                if (!(d2 <= __int_as_float(0x7f800000))) continue;
                int32_t pw; float d2w;
                if (hood_test(a, ix, i, p.x, p.y, p.z, dist2(p.x, p.y, p.z, ce.x, ce.y, ce.z), pk, d2, __float_as_int(q.w), pw, d2w)) {
                    float4 qw = q, nqw = nq;
                    if (pw != pk) { qw = ix.tn[2 * (size_t)pw]; nqw = ix.tn[2 * (size_t)pw + 1]; }
                    const float3 n = load_src_normal(a.in, i, need_n);      // (only now: most listed pairs do not get here)
                    pair_step<OBJ>(acc, h, n.x, n.y, n.z, p.x, p.y, p.z, qw, nqw, d2w);
                    s_list[e] = 0xFFFFFFFFu;                       // settled (an idle lane of the scan below)
                    atomicAdd(&s_hood, 1u);
                }
            }
            __syncthreads();
        }
        for (uint32_t base = 0; base < cnt; base += kPassThreads) {
            const uint32_t e = base + threadIdx.x;
            cells_tile<true>(a, ix, wl, X, e < cnt ? s_list[e] : 0xFFFFFFFFu, shard, true);
            __syncthreads();
        }
        if (ACC) {
            for (uint32_t base = 0; base < cnt; base += kPassThreads) {      // (each thread meets the entries it scanned itself)
                const uint32_t e = base + threadIdx.x;
                if (e >= cnt) continue;
                const uint32_t i = s_list[e];
                if (i == 0xFFFFFFFFu) continue;                        // settled by its neighbourhood above
                const float4 q = a.pairrec[2 * (size_t)i], nq = a.pairrec[2 * (size_t)i + 1];
                if (nq.w != 0.0f) continue;                            // no target at all, or handed to the walk
                const SrcRow r = load_src_row(a.in, i, need_n);
                const float3 p = transform_point(X, r.p);
                pair_step<OBJ>(acc, h, r.n.x, r.n.y, r.n.z, p.x, p.y, p.z, q, nq, dist2(p.x, p.y, p.z, q.x, q.y, q.z));
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) { s_total += cnt; s_cnt = 0; }
        __syncthreads();
    };

    // A tile = 256 consecutive points, one per thread (every load coalesced).  2 and 4 points per thread with everything requested up
    // front (144 / 288 B per lane in flight instead of 72) were measured in rounds 2 and 3 and are no faster at any size:
    // the loop is bound by its arithmetic and one round trip per tile, not by bytes in flight
    const uint32_t tiles = (a.n + kPassThreads - 1) / kPassThreads;
    // ACC: one contiguous eighth of the tiles per XCD (uniform work, best locality); search only: chunks of 16 tiles (the regions of a
    // cloud differ in cost: xcd_remap_chunked)
    constexpr uint32_t kTileChunk = 16;
    const uint32_t tiles_p = ACC ? ((tiles + 7u) / 8u) * 8u : ((tiles + 8u * kTileChunk - 1u) / (8u * kTileChunk)) * (8u * kTileChunk);
    // ---- stream (tile numbers are dealt so that each XCD works on one contiguous part of the sorted source)
    for (uint32_t t = blockIdx.x; t < tiles_p; t += gridDim.x) {
        const uint32_t i = (ACC ? xcd_remap(t, tiles_p) : xcd_remap_chunked(t, kTileChunk)) * kPassThreads + threadIdx.x;
        if (ACC) asm volatile("" ::: "memory");        // (the column table is read here, per tile: hoisted out of the loop it would be 24 more live registers)
        // one round trip: everything the common case (certified pair) needs.  (Measured and dropped: letting the last block to finish
        // reduce and solve in place of k_reduce_solve with device-scope fences -- every block then waits for an L2 write-back, 79 us
        // per pass instead of 27 + 12.)
        const bool live = i < a.n;
        float x = 0.f, y = 0.f, z = 0.f, nx = 0.f, ny = 0.f, nz = 0.f;      // (idle lanes carry zeros and a stale record, as in k_pass_certified)
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), nq = make_float4(0.f, 0.f, 0.f, 2.0f), ce = make_float4(0.f, 0.f, 0.f, 0.f);
        int32_t pa = -1;
        if (live) {
            if (ACC) {
                const size_t o = (size_t)i;
                x = gcol<float>(s_col[0])[o]; y = gcol<float>(s_col[1])[o]; z = gcol<float>(s_col[2])[o];
                if (need_n) { nx = gcol<float>(s_col[3])[o]; ny = gcol<float>(s_col[4])[o]; nz = gcol<float>(s_col[5])[o]; }
                else nx = ny = nz = 0.0f;
                q = as_float4(gcol<f32x4_t>(s_col[6])[2 * o]); nq = as_float4(gcol<f32x4_t>(s_col[6])[2 * o + 1]);      // a fresh copy (w = 0) has the bits of tq[prev]
                ce = as_float4(gcol<f32x4_t>(s_col[7])[o]);
            } else {
                x = a.in.x[i]; y = a.in.y[i]; z = a.in.z[i];
                pa = a.pos_prev[i];
                if ((uint32_t)pa < ix.n) { q = ix.tq[pa]; nq.w = 0.0f; }
                ce = a.cert[i];
            }
        }
        if (stop) return;                 // (uniform; nothing has been written yet)
#ifdef RS_STAMPS2
        if (fs1 == 0) fs1 = __builtin_amdgcn_s_memrealtime();       // loop state and the first tile's data are here
#endif
        if (live) {
            const float px = xf_row(X.m + 0, x, y, z, 1.0f), py = xf_row(X.m + 4, x, y, z, 1.0f), pz = xf_row(X.m + 8, x, y, z, 1.0f);
            bool certified = false;
            float d2 = 0.0f;
            if (nq.w == 0.0f) {
                d2 = dist2(px, py, pz, q.x, q.y, q.z);
                const float m2 = dist2(px, py, pz, ce.x, ce.y, ce.z);
                certified = cert_holds(d2, m2, ce.w);
                if (!ACC && !certified && d2 <= __int_as_float(0x7f800000) && (__float_as_uint(ce.w) & 1u) && a.certk) {
                    // the neighbourhood certificate: the winner is a member of the set the last scan kept (ACC: in the flush)
                    int32_t pw; float d2w;
                    if ((uint32_t)pa < ix.n && hood_test(a, ix, i, px, py, pz, m2, pa, d2, __float_as_int(q.w), pw, d2w)) {
                        certified = true;
                        d2 = d2w;
                    }
                }
            }
            if (certified) {
                // (the refreshed distance is not stored: 4 of the pass's 76 bytes per point; symmicp_get_correspondences evaluates it)
                if (ACC) pair_step<OBJ>(acc, h, nx, ny, nz, px, py, pz, q, nq, d2);
            } else {
                s_list[atomicAdd(&s_cnt, 1u)] = i;                 // (room for a whole tile: see the flush below)
            }
        }
        // room for another tile?  (uniform: everyone reads s_cnt after the barrier)
        __syncthreads();
        if (s_cnt > (uint32_t)(kList - kPassThreads)) flush();
    }
    __syncthreads();
    flush();
    // pairs that had to be searched (see cells_tile)
    if (threadIdx.x == 0 && s_total) atomicAdd(wl.work.counts + shard * kShardStride + 1, s_total);
    // ... and those of them that never reached a scan (word 3): "searched" counts every listed pair, but what run_batch needs to know before
    // it chooses k_pass_certified is whether any pair was really scanned, probed or walked: searched - settled
    if (ACC && threadIdx.x == 0 && s_hood) atomicAdd(wl.work.counts + shard * kShardStride + 3, s_hood);
#ifdef RS_STAMPS2
    const unsigned long long fs2 = __builtin_amdgcn_s_memrealtime();
#endif
    if (ACC) acc_block_reduce_store(acc, a.partials, blockIdx.x);
#ifdef RS_STAMPS2
    if (ACC && blockIdx.x == 0 && threadIdx.x == 0) {
        double *dbg = a.partials + (size_t)8191 * kNSum;
        dbg[0] = (double)(fs1 - fs0); dbg[1] = (double)(fs2 - fs1); dbg[2] = (double)(__builtin_amdgcn_s_memrealtime() - fs2);
    }
#endif
}

// ---------------------------------------------------------------------------
// k_pass_certified: the pass of a converged alignment in which NO pair needs a scan -- k_accumulate's loop plus the certificate.  In
// such a pass k_pass_fused carries its scan machinery for nothing (34 KB of LDS, ~240 registers, ~150 argument scalars live across
// the loop, a barrier and a counter check per tile).  Here the loop has no barrier, no LDS traffic and no store:
//   stream   the tiles in k_pass_fused<true>'s order; per point the single-certificate test (cert_holds)
//            and the pair step; a pair that fails goes to a small list in LDS
//   settle   after the loop, once: the neighbourhood certificate of the listed pairs (hood_test, as the first stage of
//            k_pass_fused's flush: record refresh when the winner changes, accumulation on success)
// There is no scan.  Every pair that is still unsettled -- no neighbourhood, a stale record copy, no target, a failed test, a list
// that overflowed -- makes the pass INCOMPLETE: the block adds their number to its shard's work-list count word (no entry is
// appended), so k_reduce_solve stops the loop with LOOP_REDO_PASS and the host repeats the pass through the search kernels, as for
// a work list that turns up without the straggler stage.  run_batch chooses this kernel for a chunk of passes after a complete pass
// that scanned nothing, and never again in an alignment once a pass of it came back incomplete.
// ---------------------------------------------------------------------------
constexpr uint32_t kCertList = kPassThreads;      // (one settle round; a converged 1M-point pass lists under one pair per block)

template <bool W, int OBJ>
__global__ __launch_bounds__(kPassThreads) void k_pass_certified(PassArgs a, TargetIndex ix, WorkLists wl)
{
    const bool need_n = reads_src_normals<OBJ>(false, a.min_ndot);      // (no write-back here)
    __shared__ uint32_t s_list[kCertList];
    __shared__ uint32_t s_cnt, s_bad;
    AccT<W> acc; acc_zero(acc);
    if (threadIdx.x == 0) { s_cnt = 0; s_bad = 0; }
    __syncthreads();
    // stop flag and transform of a device-driven loop: requested here, looked at behind the first tile's loads (see k_pass_fused)
    int stop = 0;
    HotParams h = hot_params(a);
    if (a.loop) {
        stop = a.loop->stop;
        loop_transform(h, a.loop);
    }
    const Affine &X = h.X;
    const uint32_t tiles = (a.n + kPassThreads - 1) / kPassThreads;
    const uint32_t tiles_p = ((tiles + 7u) / 8u) * 8u;
    for (uint32_t t = blockIdx.x; t < tiles_p; t += gridDim.x) {
        const uint32_t i = xcd_remap(t, tiles_p) * kPassThreads + threadIdx.x;
        const bool live = i < a.n;
        SrcRow r = {make_float3(0.f, 0.f, 0.f), make_float3(0.f, 0.f, 0.f)};
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f), nq = make_float4(0.f, 0.f, 0.f, 2.0f), ce = make_float4(0.f, 0.f, 0.f, 0.f);
        if (live) {
            r = load_src_row(a.in, i, need_n);
            q = a.pairrec[2 * (size_t)i]; nq = a.pairrec[2 * (size_t)i + 1];
            ce = a.cert[i];
        }
        if (stop) return;                 // (uniform; nothing has been written yet)
        if (!live) continue;
        const float3 p = transform_point(X, r.p);
        bool certified = false;
        float d2 = 0.0f;
        if (nq.w == 0.0f) {
            d2 = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
            certified = cert_holds(d2, dist2(p.x, p.y, p.z, ce.x, ce.y, ce.z), ce.w);
        }
        if (certified) pair_step<OBJ>(acc, h, r.n.x, r.n.y, r.n.z, p.x, p.y, p.z, q, nq, d2);
        else {
            const uint32_t e = atomicAdd(&s_cnt, 1u);
            if (e < kCertList) s_list[e] = i;
        }
    }
    __syncthreads();
    const uint32_t cnt = s_cnt;
    if (cnt) {                            // (uniform)
        const uint32_t m = min(cnt, kCertList);
        if (threadIdx.x < m) {
            const uint32_t i = s_list[threadIdx.x];
            bool settled = false;
            // one round trip for everything addressed by i (the set and its radius too, whether or not the test will run: the settle stage
            // is a chain of dependent loads at the end of the slowest blocks), a second one for the set's members
            const float4 ce = a.cert[i];
            const float4 q = a.pairrec[2 * (size_t)i], nq = a.pairrec[2 * (size_t)i + 1];
            const int32_t pk = a.pos_prev[i];
            const SrcRow r = load_src_row(a.in, i, need_n);
            uint4 w0 = make_uint4(kHoodNone, kHoodNone, kHoodNone, kHoodNone), w1 = w0;
            float T = 0.0f;
            if (a.certk) { w0 = a.certk[2 * (size_t)i]; w1 = a.certk[2 * (size_t)i + 1]; T = a.hoodr[i].x; }
            if (a.certk && (__float_as_uint(ce.w) & 1u)) {
                if (nq.w == 0.0f && (uint32_t)pk < ix.n) {
                    const float3 p = transform_point(X, r.p);
                    const float d2 = dist2(p.x, p.y, p.z, q.x, q.y, q.z);
                    int32_t pw; float d2w;
                    if (d2 <= __int_as_float(0x7f800000) &&
                        hood_test_set(a, ix, i, p.x, p.y, p.z, dist2(p.x, p.y, p.z, ce.x, ce.y, ce.z), pk, d2, __float_as_int(q.w), w0, w1, T, pw, d2w)) {
                        float4 qw = q, nqw = nq;
                        if (pw != pk) { qw = ix.tn[2 * (size_t)pw]; nqw = ix.tn[2 * (size_t)pw + 1]; }
                        pair_step<OBJ>(acc, h, r.n.x, r.n.y, r.n.z, p.x, p.y, p.z, qw, nqw, d2w);
                        settled = true;
                    }
                }
            }
            if (!settled) atomicAdd(&s_bad, 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t shard = blockIdx.x & (kShards - 1);
            const uint32_t bad = s_bad + (cnt - m);
            if (bad) atomicAdd(wl.work.counts + shard * kShardStride, bad);       // the pass is incomplete (no entry: nothing walks this "list")
            atomicAdd(wl.work.counts + shard * kShardStride + 1, cnt);            // pairs searched, as k_pass_fused counts them
            atomicAdd(wl.work.counts + shard * kShardStride + 3, cnt - bad);      // ... and those their neighbourhood settled
        }
    }
    acc_block_reduce_store(acc, a.partials, blockIdx.x);
}

// The pair's distance is recomputed from the gathered q (bit-identical to the stored one) instead of being read.
// (A 4-points-per-thread variant with 16-byte column loads was measured and is no faster: the two 16-byte gathers per
// pair bound this kernel, not the column loads.  Few blocks are: each one ends in a 40-value block reduction.)
template <bool W, int OBJ, bool T>
__global__ __launch_bounds__(kPassThreads) void k_accumulate(PassArgs a, const float4 *__restrict__ tn)
{
    AccT<W> acc; acc_zero(acc);
    const HotParams h = hot_params(a);
    const uint32_t tau = T ? a.rej.ws[kRejectTauWord] : 0u;
    const bool need_n = reads_src_normals<OBJ>(a.writeback, a.min_ndot);
    const uint32_t nbp = gridDim.x;
    // grid-stride over blocks of 256 points, XCD-contiguous
    const uint32_t total_blocks = (a.n + kPassThreads - 1) / kPassThreads;
    for (uint32_t lb = xcd_remap(blockIdx.x, nbp); lb < total_blocks; lb += nbp) {
        const uint32_t i = lb * kPassThreads + threadIdx.x;
        if (i >= a.n) continue;
        const SrcRow r = load_src_row(a.in, i, need_n);
        float4 q = a.pairrec[2 * (size_t)i], nq = a.pairrec[2 * (size_t)i + 1];            // the pair's own copy: coalesced
        if (nq.w == 2.0f) {
            // stale copy: the pair went through the tree walk this pass
            const int32_t pos = a.pos_out[i];
            if (pos >= 0) { q = tn[2 * (size_t)pos]; nq = tn[2 * (size_t)pos + 1]; }
            else nq = make_float4(0.f, 0.f, 0.f, 1.f);
            if (a.refresh_records) { a.pairrec[2 * (size_t)i] = q; a.pairrec[2 * (size_t)i + 1] = nq; }
        }
        const float3 p = transform_point(a.X, r.p);
        if (a.writeback) write_back(a, i, p, r.n);
        if (nq.w != 0.0f) continue;                       // no target for this point
        if (T && a.rej.claim != kClaimNone && a.rej.keys[i] == 0xFFFFFFFFu) continue;      // one-to-one: the row lost its target (or is no candidate)
        // (COLOR gathers by the pair's sorted position: the record copy holds no colour)
        pair_step_at<OBJ, T>(acc, h, a, i, OBJ == kObjColor ? (uint32_t)a.pos_out[i] : 0u, r.n, p, q, nq, dist2(p.x, p.y, p.z, q.x, q.y, q.z), tau);
    }
    acc_block_reduce_store(acc, a.partials, blockIdx.x);
}

// Straggler stage of a device-driven loop (after k_pass_fused and k_search_walk): the pairs of the work list's queries -- the fused pass
// left them out and marked their record copies stale -- are gathered, their copies refreshed, their rows summed into `gridDim.x` partial
// columns behind the fused pass's.  Launched whether or not the list is empty (the columns must be written).
template <bool W, int OBJ>
__global__ __launch_bounds__(kPassThreads) void k_accumulate_list(PassArgs a, const float4 *__restrict__ tn, ShardList list)
{
    if (a.loop) {
        if (a.loop->stop) return;
        a.X = a.loop->Xapply;
    }
    AccT<W> acc; acc_zero(acc);
    const HotParams h = hot_params(a);
    const bool need_n = reads_src_normals<OBJ>(false, a.min_ndot);      // (no write-back here)
    // block b: shards b, b + gridDim.x, ...; its waves take them in turn (a list is a handful of entries: what counts is that the
    // counters and entries of all shards are requested side by side, not one shard after the other)
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t shard = blockIdx.x + gridDim.x * wave; shard < (uint32_t)kShards; shard += gridDim.x * (kPassThreads / 64)) {
        const uint32_t cnt = min(list.counts[shard * kShardStride], list.cap);
        for (uint32_t e = lane; e < cnt; e += 64) {
            const uint32_t i = list.items[(size_t)shard * list.cap + e];
            const SrcRow r = load_src_row(a.in, i, need_n);
            const int32_t pos = a.pos_out[i];
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f), nq = make_float4(0.f, 0.f, 0.f, 1.f);
            if (pos >= 0) { q = tn[2 * (size_t)pos]; nq = tn[2 * (size_t)pos + 1]; }
            a.pairrec[2 * (size_t)i] = q; a.pairrec[2 * (size_t)i + 1] = nq;
            if (nq.w != 0.0f) continue;                   // no target for this point
            const float3 p = transform_point(a.X, r.p);
            pair_step<OBJ>(acc, h, r.n.x, r.n.y, r.n.z, p.x, p.y, p.z, q, nq, dist2(p.x, p.y, p.z, q.x, q.y, q.z));
        }
    }
    acc_block_reduce_store(acc, a.partials, a.partial_col0 + blockIdx.x);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
// Calls f(W, OBJ) with the pass's instantiation as compile-time constants (std::integral_constant): W, weighted (robust loss) or not;
// OBJ, the record (PassArgs::obj)
template <typename F>
static void with_instantiation(const PassArgs &a, F &&f)
{
    auto obj = [&](auto W) {
        if (a.obj == kObjGicp) f(W, std::integral_constant<int, kObjGicp>());
        else if (a.obj == kObjPlane) f(W, std::integral_constant<int, kObjPlane>());
        else f(W, std::integral_constant<int, kObjSym>());
    };
    if (a.loss != SYMMICP_LOSS_NONE) obj(std::true_type());
    else obj(std::false_type());
}

// ... and T: a rejecting pass (pass_rejects): the claim, the keys and the select (kernels_select.hip) run in front of its accumulating
// kernel, whose T instantiation reads the tau they leave.  The kernels of the device-driven loop have no such instantiation
// (batch_eligible keeps a trimming context in the host loop).
template <typename F>
static void with_trim(const PassArgs &a, F &&f)
{
    if (a.obj == kObjColor) {
        // COLOR's instantiations exist for the host loop's accumulating kernels only (with_instantiation, which also serves the fused
        // pass and the straggler stage, does not know them: batch_eligible keeps a COLOR context in the host loop)
        auto trim = [&](auto W) {
            if (pass_rejects(a)) f(W, std::integral_constant<int, kObjColor>(), std::true_type());
            else f(W, std::integral_constant<int, kObjColor>(), std::false_type());
        };
        if (a.loss != SYMMICP_LOSS_NONE) trim(std::true_type());
        else trim(std::false_type());
        return;
    }
    with_instantiation(a, [&](auto W, auto OBJ) {
        if (pass_rejects(a)) f(W, OBJ, std::true_type());
        else f(W, OBJ, std::false_type());
    });
}

void launch_pass_identity(const PassArgs &a, CloudSoA tgt, int blocks, bool vec4_ok, hipStream_t s)
{
    if (pass_rejects(a)) launch_reject(a, SYMMICP_CORR_IDENTITY, tgt, nullptr, s);
    with_trim(a, [&](auto W, auto OBJ, auto T) {
        if (vec4_ok) hipLaunchKernelGGL((k_pass_identity<4, W, OBJ, T>), dim3(blocks), dim3(kPassThreads), 0, s, a, tgt);
        else hipLaunchKernelGGL((k_pass_identity<1, W, OBJ, T>), dim3(blocks), dim3(kPassThreads), 0, s, a, tgt);
    });
}

void launch_pass_indexed(const PassArgs &a, const float4 *tn, int blocks, hipStream_t s)
{
    if (pass_rejects(a)) launch_reject(a, SYMMICP_CORR_BRUTE, CloudSoA{}, tn, s);
    with_trim(a, [&](auto W, auto OBJ, auto T) { hipLaunchKernelGGL((k_pass_indexed<W, OBJ, T>), dim3(blocks), dim3(kPassThreads), 0, s, a, tn); });
}

void launch_accumulate(const PassArgs &a, const float4 *tn, int blocks, hipStream_t s)
{
    if (pass_rejects(a)) launch_reject(a, SYMMICP_CORR_TREE, CloudSoA{}, tn, s);
    with_trim(a, [&](auto W, auto OBJ, auto T) { hipLaunchKernelGGL((k_accumulate<W, OBJ, T>), dim3(blocks), dim3(kPassThreads), 0, s, a, tn); });
}

// stage: 0 = whole pass (cells, walk, accumulate); 1 = cells and accumulate only (the host expects an empty work list
// and repairs the pass otherwise); 2 = the repair: walk and accumulate
// compact_blocks > 0: the search runs as k_pass_fused<false> on that many blocks (sparse scans), else as k_search_cells
void launch_pass_tree_split(const PassArgs &a_in, const TargetIndex &ix, const WorkLists &wl, int acc_blocks, uint32_t walk_blocks,
                            int stage, int compact_blocks, const PassTuning &tune, hipStream_t s, hipEvent_t *ev)
{
    PassArgs a = a_in;
    a.refresh_records = (stage != 1) ? 1 : 0;      // a stage-1 pass may still be repaired: its accumulate must not settle stale copies
    // all shard counters are zero here: cleared by the previous pass's final reduce
    const uint32_t nb = (a.n + kPassThreads - 1) / kPassThreads;
    const uint32_t nbp = ((nb + 7u) / 8u) * 8u;
    if (ev) hipEventRecord(ev[0], s);
    if (stage != 2 && nbp) {      // (nbp == 0: a rank whose share is empty)
        if (compact_blocks > 0) hipLaunchKernelGGL((k_pass_fused<false, false, kObjSym>), dim3(min((uint32_t)compact_blocks, nbp)), dim3(kPassThreads), 0, s, a, ix, wl);
        else launch_search_cells(a, ix, wl, tune, s);
    }
    if (ev) hipEventRecord(ev[1], s);
    if (ev) hipEventRecord(ev[2], s);
    if (stage != 1 && nbp) launch_search_walk(a, ix, wl, walk_blocks, tune, s);
    if (ev) hipEventRecord(ev[3], s);
    launch_accumulate(a, ix.tn, acc_blocks, s);
    if (ev) hipEventRecord(ev[4], s);
}

void launch_pass_fused(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int blocks, hipStream_t s)
{
    with_instantiation(a, [&](auto W, auto OBJ) { hipLaunchKernelGGL((k_pass_fused<true, W, OBJ>), dim3(blocks), dim3(kPassThreads), 0, s, a, ix, wl); });
}

void launch_pass_certified(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int blocks, hipStream_t s)
{
    with_instantiation(a, [&](auto W, auto OBJ) { hipLaunchKernelGGL((k_pass_certified<W, OBJ>), dim3(blocks), dim3(kPassThreads), 0, s, a, ix, wl); });
}

void launch_loop_stragglers(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, int list_blocks, const PassTuning &tune, hipStream_t s)
{
    launch_straggler_walk(a, ix, wl, tune, s);
    with_instantiation(a, [&](auto W, auto OBJ) {
        hipLaunchKernelGGL((k_accumulate_list<W, OBJ>), dim3(list_blocks), dim3(kPassThreads), 0, s, a, ix.tn, wl.work);
    });
}

}  // namespace symmicp
