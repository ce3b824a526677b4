// pass_rows.h -- the rows of one pair and the wave-level sum of a record: what every accumulating kernel shares.
//
// Included by kernels_pass.hip (the pass kernels of the big pair), kernels_batch.hip (one workgroup per small problem) and
// kernels_ndt.hip: the accumulators, the per-mode rows (acc_pair / acc_plane / acc_gicp / acc_color), the gates (pair_step), the
// source row of a pair (load_src_row, transform_point, write_back), the wave64 sum of the 37 accumulators and the block's record
// (acc_block_reduce_store) live here ONCE, so every translation unit forms a pair's terms from the same source.
//
// fp32 expressions here must stay UNFUSED (the including file is compiled with -ffp-contract=off and carries
// `#pragma clang fp contract(off)`) and keep the association written: the CPU oracle and tests/_record_ref.py use the same
// expressions, so records compare term for term.
#pragma once
#include <type_traits>
#include "symmicp_internal.h"
#include "device_common.h"
#include "robust_loss.h"
#pragma clang fp contract(off)

namespace symmicp {

// ---------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------
template <int NA>
struct AccN {
    double v[NA];
};
typedef AccN<kNAcc> Acc;
// W = true: the weighted instantiations of the accumulating kernels (robust loss), one accumulator more (slot 37: the pair count).
// A separate instantiation, not a branch: the unweighted kernels keep their registers and occupancy (the fused pass is register-bound).
template <bool W>
using AccT = AccN<W ? kNAccW : kNAcc>;

template <int NA>
__device__ __forceinline__ void acc_zero(AccN<NA> &a)
{
#pragma unroll
    for (int k = 0; k < NA; k++) a.v[k] = 0.0;
}

// One row v with residual c at weight w (1 in an unweighted record: 1 x = x and fma(1, x, s) = s + x exactly) into the Gram (slots
// 0..20, upper triangle row by row), the right-hand side (21..26) and the cost (35)
template <int NA>
__device__ __forceinline__ void acc_row(AccN<NA> &a, const double v[6], double c, double w)
{
    const double wc = w * c;
    int k = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) {
        const double wv = w * v[r];
#pragma unroll
        for (int s = r; s < 6; s++) { a.v[k] = __builtin_fma(wv, v[s], a.v[k]); k++; }
    }
#pragma unroll
    for (int r = 0; r < 6; r++) a.v[21 + r] = __builtin_fma(v[r], wc, a.v[21 + r]);
    a.v[35] = __builtin_fma(wc, c, a.v[35]);
}

// The per-pair slots of the row-based records: the weighted sums of p and q (27..32), sqrt(d2) (33), the weight (34), d2 (36) and, in
// the weighted record (NA = kNAccW), the pair count (37)
template <int NA>
__device__ __forceinline__ void acc_pair_sums(AccN<NA> &a, float px, float py, float pz, float qx, float qy, float qz, float d2, double w)
{
    a.v[27] = __builtin_fma(w, (double)px, a.v[27]); a.v[28] = __builtin_fma(w, (double)py, a.v[28]); a.v[29] = __builtin_fma(w, (double)pz, a.v[29]);
    a.v[30] = __builtin_fma(w, (double)qx, a.v[30]); a.v[31] = __builtin_fma(w, (double)qy, a.v[31]); a.v[32] = __builtin_fma(w, (double)qz, a.v[32]);
    a.v[33] += (double)sqrtf(d2);                                      // func.cpp:28
    a.v[34] += w;
    a.v[36] += (double)d2;
    if constexpr (NA == kNAccW) a.v[37] += 1.0;
}

// rows of func.cpp:51-58 for one pair, accumulated in fp64.  In the weighted record (NA = kNAccW) the pair is weighted by its robust-loss
// weight w (robust_loss.h) of r = c (PAPER) or |p - q| (P2P): every sum but 33 and 36 is scaled by w, slot 34 sums w, slot 37 counts the pairs
template <int NA>
__device__ __forceinline__ void acc_pair(AccN<NA> &a, float px, float py, float pz, float npx, float npy, float npz,
                                         float qx, float qy, float qz, float nqx, float nqy, float nqz,
                                         float d2, const float *pivot, int p2p, int loss, float scale)
{
    constexpr bool W = NA == kNAccW;
    px -= pivot[0]; py -= pivot[1]; pz -= pivot[2];
    qx -= pivot[0]; qy -= pivot[1]; qz -= pivot[2];
    if (p2p) {
        // point-to-point (regist.h:52): 3x3 cross-covariance sums, row-major in slots 0..8
        const float dist = sqrtf(d2);
        const double w = W ? (double)robust_weight(loss, scale, dist) : 1.0;
        const double P[3] = {(double)px, (double)py, (double)pz}, Q[3] = {(double)qx, (double)qy, (double)qz};
        const double WP[3] = {w * P[0], w * P[1], w * P[2]};
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) a.v[3 * r + c] = __builtin_fma(WP[r], Q[c], a.v[3 * r + c]);
#pragma unroll
        for (int k = 0; k < 3; k++) { a.v[27 + k] += WP[k]; a.v[30 + k] = __builtin_fma(w, Q[k], a.v[30 + k]); }
        a.v[33] += (double)dist;
        a.v[34] += w;
        a.v[36] += (double)d2;
        if constexpr (W) a.v[37] += 1.0;
        return;
    }
    float nx = npx + nqx, ny = npy + nqy, nz = npz + nqz;            // func.cpp:51
    float sx = px + qx, sy = py + qy, sz = pz + qz;
    float dx = px - qx, dy = py - qy, dz = pz - qz;
    float m0 = sy * nz - sz * ny;                                      // func.cpp:54
    float m1 = sz * nx - sx * nz;
    float m2 = sx * ny - sy * nx;
    float c = (dx * nx + dy * ny) + dz * nz;                           // func.cpp:58
    const double w = W ? (double)robust_weight(loss, scale, c) : 1.0;
    const double v[6] = {(double)m0, (double)m1, (double)m2, (double)nx, (double)ny, (double)nz};
    acc_row(a, v, (double)c, w);
    acc_pair_sums(a, px, py, pz, qx, qy, qz, d2, w);
}

// PLANE (point-to-plane): PAPER's slots with n_p = 0 and s = p + q replaced by p -- rows v = (p x n_q, n_q), c = (p - q) . n_q -- and,
// in the weighted record (NA = kNAccW), PAPER's weighting with r = c.  Needs no source normal.
template <int NA>
__device__ __forceinline__ void acc_plane(AccN<NA> &a, float px, float py, float pz, float qx, float qy, float qz,
                                          float nx, float ny, float nz, float d2, const float *pivot, int loss, float scale)
{
    px -= pivot[0]; py -= pivot[1]; pz -= pivot[2];
    qx -= pivot[0]; qy -= pivot[1]; qz -= pivot[2];
    float dx = px - qx, dy = py - qy, dz = pz - qz;
    float m0 = py * nz - pz * ny;
    float m1 = pz * nx - px * nz;
    float m2 = px * ny - py * nx;
    float c = (dx * nx + dy * ny) + dz * nz;
    const double w = NA == kNAccW ? (double)robust_weight(loss, scale, c) : 1.0;
    const double v[6] = {(double)m0, (double)m1, (double)m2, (double)nx, (double)ny, (double)nz};
    acc_row(a, v, (double)c, w);
    acc_pair_sums(a, px, py, pz, qx, qy, qz, d2, w);
}

// GICP (plane-to-plane, Segal et al. 2009): the pair's cost d^T M d with M = (C_p + C_q)^-1, C_x = I - k x x^T, k = 1 - eps, a = the
// moved source normal, b = the target normal, d = p - q.  With u = a + b, v = a - b and cs = a . b clamped to [-1, 1] (so both lambdas
// stay >= 2 eps whatever the normals), in closed form:
//   M = 1/2 I + gu u u^T + gv v v^T,   gu = k / (4 (2 - k (1 + cs))),   gv = k / (4 (2 - k (1 - cs))).
// Five rows of PLANE's form v = (p x l, l), c = l . d: u at weight gu, v at gv -- fp32, unfused, as acc_plane forms them -- and the three
// axes at weight 1/2, summed directly as 1/2 J^T J and 1/2 J^T d (J = [-[p]x, I]) in fp64 from p and d.  Slots 27..32 per pair, as
// PLANE's; slot 35 sums w d^T M d.  In the weighted record (NA = kNAccW) the pair's weight is that of r = sqrt(d^T M d) in fp32.
template <int NA>
__device__ __forceinline__ void acc_gicp(AccN<NA> &a, float px, float py, float pz, float ax, float ay, float az, float qx, float qy, float qz,
                                         float bx, float by, float bz, float d2, const float *pivot, float gk, int loss, float scale)
{
    px -= pivot[0]; py -= pivot[1]; pz -= pivot[2];
    qx -= pivot[0]; qy -= pivot[1]; qz -= pivot[2];
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float cs = fminf(fmaxf((ax * bx + ay * by) + az * bz, -1.0f), 1.0f);
    const float gu = gk / (4.0f * (2.0f - gk * (1.0f + cs)));
    const float gv = gk / (4.0f * (2.0f - gk * (1.0f - cs)));
    const float ux = ax + bx, uy = ay + by, uz = az + bz;
    const float vx = ax - bx, vy = ay - by, vz = az - bz;
    const float cu = (dx * ux + dy * uy) + dz * uz;
    const float cv = (dx * vx + dy * vy) + dz * vz;
    double w = 1.0;
    if constexpr (NA == kNAccW) {
        const float dd = (dx * dx + dy * dy) + dz * dz;
        w = (double)robust_weight(loss, scale, sqrtf((0.5f * dd + (gu * cu) * cu) + (gv * cv) * cv));
    }
    // the u row, then the v row
    const double U[6] = {(double)(py * uz - pz * uy), (double)(pz * ux - px * uz), (double)(px * uy - py * ux), (double)ux, (double)uy, (double)uz};
    acc_row(a, U, (double)cu, w * (double)gu);
    const double V[6] = {(double)(py * vz - pz * vy), (double)(pz * vx - px * vz), (double)(px * vy - py * vx), (double)vx, (double)vy, (double)vz};
    acc_row(a, V, (double)cv, w * (double)gv);
    // the axis rows: 1/2 J^T J = 1/2 [[|p|^2 I - p p^T, [p]x], [[p]x^T, I]] and 1/2 J^T d = 1/2 (p x d, d)
    const double Px = px, Py = py, Pz = pz, Dx = dx, Dy = dy, Dz = dz;
    const double hw = 0.5 * w, hx = hw * Px, hy = hw * Py, hz = hw * Pz;
    a.v[0] = __builtin_fma(hz, Pz, __builtin_fma(hy, Py, a.v[0]));
    a.v[1] = __builtin_fma(-hx, Py, a.v[1]);
    a.v[2] = __builtin_fma(-hx, Pz, a.v[2]);
    a.v[4] -= hz; a.v[5] += hy;
    a.v[6] = __builtin_fma(hz, Pz, __builtin_fma(hx, Px, a.v[6]));
    a.v[7] = __builtin_fma(-hy, Pz, a.v[7]);
    a.v[8] += hz; a.v[10] -= hx;
    a.v[11] = __builtin_fma(hy, Py, __builtin_fma(hx, Px, a.v[11]));
    a.v[12] -= hy; a.v[13] += hx;
    a.v[15] += hw; a.v[18] += hw; a.v[20] += hw;
    a.v[21] = __builtin_fma(hy, Dz, __builtin_fma(-hz, Dy, a.v[21]));
    a.v[22] = __builtin_fma(hz, Dx, __builtin_fma(-hx, Dz, a.v[22]));
    a.v[23] = __builtin_fma(hx, Dy, __builtin_fma(-hy, Dx, a.v[23]));
    a.v[24] = __builtin_fma(hw, Dx, a.v[24]); a.v[25] = __builtin_fma(hw, Dy, a.v[25]); a.v[26] = __builtin_fma(hw, Dz, a.v[26]);
    a.v[35] = __builtin_fma(hw, __builtin_fma(Dz, Dz, __builtin_fma(Dy, Dy, Dx * Dx)), a.v[35]);
    acc_pair_sums(a, px, py, pz, qx, qy, qz, d2, w);
}

// COLOR (colored ICP, Park et al. 2017): two rows of PLANE's form per pair -- the geometric row v = (p x n_q, n_q), c_G = (p - q) . n_q at
// weight lam, formed exactly as acc_plane forms it, and the photometric row v = (p x g, g), c_C = (p - q) . g + (I_q - I_p) at weight
// om = 1.0f - lam, g = the target's intensity gradient -- fp32, unfused.  Slots 27..34, 36, 37 once per pair, as PLANE's; slot 35 sums
// w (lam c_G^2 + om c_C^2).  In the weighted record (NA = kNAccW) the pair's weight is that of r = sqrtf((lam c_G) c_G + (om c_C) c_C) and
// scales both rows, as GICP's does.  At lam = 1 (om = 0) every photometric term is an exact zero: the record is PLANE's bit for bit.
template <int NA>
__device__ __forceinline__ void acc_color(AccN<NA> &a, float px, float py, float pz, float qx, float qy, float qz, float nx, float ny, float nz,
                                          const float4 &gi, float ip, float d2, const float *pivot, float lam, float om, int loss, float scale)
{
    px -= pivot[0]; py -= pivot[1]; pz -= pivot[2];
    qx -= pivot[0]; qy -= pivot[1]; qz -= pivot[2];
    const float dx = px - qx, dy = py - qy, dz = pz - qz;
    const float m0 = py * nz - pz * ny;
    const float m1 = pz * nx - px * nz;
    const float m2 = px * ny - py * nx;
    const float cg = (dx * nx + dy * ny) + dz * nz;
    const float gx = gi.x, gy = gi.y, gz = gi.z;
    const float k0 = py * gz - pz * gy;
    const float k1 = pz * gx - px * gz;
    const float k2 = px * gy - py * gx;
    const float cc = ((dx * gx + dy * gy) + dz * gz) + (gi.w - ip);
    const double w = NA == kNAccW ? (double)robust_weight(loss, scale, sqrtf((lam * cg) * cg + (om * cc) * cc)) : 1.0;
    const double G[6] = {(double)m0, (double)m1, (double)m2, (double)nx, (double)ny, (double)nz};
    acc_row(a, G, (double)cg, w * (double)lam);
    const double C[6] = {(double)k0, (double)k1, (double)k2, (double)gx, (double)gy, (double)gz};
    acc_row(a, C, (double)cc, w * (double)om);
    acc_pair_sums(a, px, py, pz, qx, qy, qz, d2, w);
}

// The record of an accumulating kernel's instantiation (its OBJ parameter, PassArgs::obj): the symmetric rows of PAPER / QUIRKS / P2P
// (acc_pair), PLANE's (acc_plane), GICP's (acc_gicp) or COLOR's (acc_color; `color` = the pair's extra data, read by that one only).
// Separate instantiations, not a branch, as W: each kernel keeps the registers its own record needs.
struct ColorPair {
    float4 gi;               // the target's (gradient xyz, intensity)
    float ip;                // the source point's intensity
    float lam, om;
};

template <int OBJ, int NA>
__device__ __forceinline__ void acc_obj(AccN<NA> &acc, float px, float py, float pz, float npx, float npy, float npz, float qx, float qy, float qz,
                                        float nqx, float nqy, float nqz, float d2, const float *pivot, int p2p, float gk, int loss, float scale,
                                        const ColorPair *color = nullptr)
{
    if constexpr (OBJ == kObjColor) acc_color(acc, px, py, pz, qx, qy, qz, nqx, nqy, nqz, color->gi, color->ip, d2, pivot, color->lam, color->om, loss, scale);
    else if constexpr (OBJ == kObjPlane) acc_plane(acc, px, py, pz, qx, qy, qz, nqx, nqy, nqz, d2, pivot, loss, scale);
    else if constexpr (OBJ == kObjGicp) acc_gicp(acc, px, py, pz, npx, npy, npz, qx, qy, qz, nqx, nqy, nqz, d2, pivot, gk, loss, scale);
    else acc_pair(acc, px, py, pz, npx, npy, npz, qx, qy, qz, nqx, nqy, nqz, d2, pivot, p2p, loss, scale);
}

// k_pass_fused holds what its streaming loop needs of its arguments (HotParams) in VECTOR registers.  The kernel's three argument structs are ~150
// scalars, all live across the loop (the scan behind it needs them); with 102 scalar registers per wave the compiler parked them in the
// lanes of a vector register and fetched them back one v_readlane at a time: 85 of the loop's 291 vector instructions per tile.  Values
// that pass through in_vgpr are opaque to it: they stay where they are (and VGPR operands issue faster than scalar ones).
template <typename T>
__device__ __forceinline__ T in_vgpr(T v)
{
    asm volatile("" : "+v"(v));
    return v;
}

// What the pair step reads of the pass's arguments.  k_pass_fused fills it through in_vgpr; the other kernels take it as
// it is (hot_params).
struct HotParams {
    Affine X;
    float pivot[3];
    float max_d2, min_ndot;
    int32_t p2p;
    int32_t loss;            // (set and read by the weighted instantiation only)
    float loss_scale;
    float gicp_k;            // (set and read by the GICP instantiation only)
};

__device__ __forceinline__ HotParams hot_params(const PassArgs &a)
{
    HotParams h;
    h.X = a.X;
#pragma unroll
    for (int k = 0; k < 3; k++) h.pivot[k] = a.pivot[k];
    h.max_d2 = a.max_d2; h.min_ndot = a.min_ndot;
    h.p2p = a.p2p; h.loss = a.loss; h.loss_scale = a.loss_scale; h.gicp_k = a.gicp_k;
    return h;
}

// The transform of a device-driven loop, as k_reduce_solve left it in the loop state, into h.X: vector loads through a pointer the
// compiler cannot see through, so that the transform arrives in VGPRs (in_vgpr).  The caller looks at it behind its first tile's loads.
__device__ __forceinline__ void loop_transform(HotParams &h, const LoopState *loop)
{
    const float4 *xp = reinterpret_cast<const float4 *>(&in_vgpr(loop)->Xapply);
    const float4 r0 = xp[0], r1 = xp[1], r2 = xp[2];
    h.X.m[0] = r0.x; h.X.m[1] = r0.y; h.X.m[2] = r0.z; h.X.m[3] = r0.w;
    h.X.m[4] = r1.x; h.X.m[5] = r1.y; h.X.m[6] = r1.z; h.X.m[7] = r1.w;
    h.X.m[8] = r2.x; h.X.m[9] = r2.y; h.X.m[10] = r2.z; h.X.m[11] = r2.w;
    h.X.nrm_w = reinterpret_cast<const float *>(xp)[12];
}

// Does an instantiation read the source normals?  Every record but PLANE's and COLOR's uses them; those read them only to write them
// back or to gate on them (min_normal_dot).
template <int OBJ>
__device__ __forceinline__ bool reads_src_normals(bool writeback, float min_ndot)
{
    return (OBJ != kObjPlane && OBJ != kObjColor) || writeback || min_ndot > -1.0f;
}

// A source row as stored: the position and the normal -- zeros where the instantiation does not read the normals (need_n =
// reads_src_normals): pair_step and write_back take them as they are
struct SrcRow {
    float3 p, n;
};

__device__ __forceinline__ float3 load_src_normal(const CloudSoA &in, uint32_t i, bool need_n)
{
    float3 n = make_float3(0.0f, 0.0f, 0.0f);
    if (need_n) { n.x = in.nx[i]; n.y = in.ny[i]; n.z = in.nz[i]; }
    return n;
}

__device__ __forceinline__ SrcRow load_src_row(const CloudSoA &in, uint32_t i, bool need_n)
{
    SrcRow r;
    r.p = make_float3(in.x[i], in.y[i], in.z[i]);
    r.n = load_src_normal(in, i, need_n);
    return r;
}

// applyTransform (func.cpp:104-121) of a position
__device__ __forceinline__ float3 transform_point(const Affine &X, float3 p)
{
    return make_float3(xf_row(X.m + 0, p.x, p.y, p.z, 1.0f), xf_row(X.m + 4, p.x, p.y, p.z, 1.0f), xf_row(X.m + 8, p.x, p.y, p.z, 1.0f));
}

// the optional write-back of a pass: the moved position p of row i, and its normal n_in moved by a.X
__device__ __forceinline__ void write_back(const PassArgs &a, uint32_t i, float3 p, float3 n_in)
{
    a.out.x[i] = p.x; a.out.y[i] = p.y; a.out.z[i] = p.z;
    a.out.nx[i] = xf_row(a.X.m + 0, n_in.x, n_in.y, n_in.z, a.X.nrm_w); a.out.ny[i] = xf_row(a.X.m + 4, n_in.x, n_in.y, n_in.z, a.X.nrm_w);
    a.out.nz[i] = xf_row(a.X.m + 8, n_in.x, n_in.y, n_in.z, a.X.nrm_w);
}

// The pair step of every accumulating kernel: the gates (max_correspondence_distance, then min_normal_dot), then the record.  (nx, ny, nz)
// is the source normal as stored (zeros where the instantiation does not read it); it is moved here, for the gate and the rows (PLANE's
// and COLOR's rows do not read it: there the compiler keeps it to the gate).  color: the COLOR instantiations' extra data (null elsewhere).
// T = true: the trimming instantiations (symmicp_set_trim_fraction below 1): a pair that passed the gates -- a candidate -- is kept only
// if its d2 bits are <= tau, the order statistic kernels_select.hip left for this pass (ties at tau are kept).  A separate instantiation,
// as W: the untrimmed kernels are the code they were.  tau has its own "off" (T = false), apart from max_d2, whose 0 means "keep all":
// tau = 0 keeps the pairs at distance 0 only.
// The one-to-one and median-distance rejectors run through the same instantiations: the median only derives tau differently, and with
// a claim in RejectArgs::claim (a runtime flag, not another template axis) the kernel drops the rows whose key is the sentinel before this step.
template <int OBJ, bool T = false, int NA>
__device__ __forceinline__ void pair_step(AccN<NA> &acc, const HotParams &h, float nx, float ny, float nz, float px, float py, float pz,
                                          const float4 &q, const float4 &nq, float d2, uint32_t tau = 0u, const ColorPair *color = nullptr)
{
    if (h.max_d2 > 0.0f && d2 > h.max_d2) return;
    const Affine &X = h.X;
    const float npx = xf_row(X.m + 0, nx, ny, nz, X.nrm_w), npy = xf_row(X.m + 4, nx, ny, nz, X.nrm_w), npz = xf_row(X.m + 8, nx, ny, nz, X.nrm_w);
    if (h.min_ndot > -1.0f && (npx * nq.x + npy * nq.y) + npz * nq.z < h.min_ndot) return;
    if (T && __float_as_uint(d2) > tau) return;
    acc_obj<OBJ>(acc, px, py, pz, npx, npy, npz, q.x, q.y, q.z, nq.x, nq.y, nq.z, d2, h.pivot, h.p2p, h.gicp_k, h.loss, h.loss_scale, color);
}

// The COLOR instantiations' extra data of one pair: the target's (gradient, intensity) at sorted position / row j, the source's at i
__device__ __forceinline__ ColorPair color_pair(const PassArgs &a, uint32_t i, uint32_t j)
{
    ColorPair c;
    c.gi = a.tgt_color[j];
    c.ip = a.src_int[i];
    c.lam = a.color_lam; c.om = a.color_om;
    return c;
}

// The pair step of source row i with target j (a row, or a sorted position: whatever the kernel's tgt_color is indexed by): COLOR's
// instantiations gather the pair's extra data here, the others take none
template <int OBJ, bool T = false, int NA>
__device__ __forceinline__ void pair_step_at(AccN<NA> &acc, const HotParams &h, const PassArgs &a, uint32_t i, uint32_t j, float3 n, float3 p,
                                             const float4 &q, const float4 &nq, float d2, uint32_t tau)
{
    if constexpr (OBJ == kObjColor) {
        const ColorPair cp = color_pair(a, i, j);
        pair_step<OBJ, T>(acc, h, n.x, n.y, n.z, p.x, p.y, p.z, q, nq, d2, tau, &cp);
    } else pair_step<OBJ, T>(acc, h, n.x, n.y, n.z, p.x, p.y, p.z, q, nq, d2, tau);
}

// one step of a sum on the VALU's DPP cross-lane network (no LDS traffic): row_shr 1,2,4,8 builds 16-lane row sums.  A double moves
// as two 32-bit DPP movs; lanes without a source read 0 (bound_ctrl), i.e. add +0.0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_f64(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROW_MASK, 0xf, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROW_MASK, 0xf, true);
    return x + __hiloint2double(hi, lo);
}

// wave64 sums of the 37 accumulators by halving: v_permlane32_swap puts the upper half-wave of value k next to the lower half-wave of
// value k + 20 (one add sums both values' halves: lanes 0..31 carry k, lanes 32..63 carry k + 20), v_permlane16_swap does the same
// with 16-lane rows for k and k + 10, and only the last four steps (row_shr 1, 2, 4, 8 inside a row of 16) touch every remaining
// register: 70 fp64 adds and 140 cross-lane moves per wave instead of the 222 + 444 of a full DPP reduction per value (2.4 us of the
// fused pass's 25 on its own stamps).  Lane 16 r + 15 then holds the wave's sum of value k + 10 r.
typedef unsigned u32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double swap32_add(double a, double b)
{
    const u32x2_t lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const u32x2_t hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi.x, (int)lo.x) + __hiloint2double((int)hi.y, (int)lo.y);
}
__device__ __forceinline__ double swap16_add(double a, double b)
{
    const u32x2_t lo = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
    const u32x2_t hi = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
    return __hiloint2double((int)hi.x, (int)lo.x) + __hiloint2double((int)hi.y, (int)lo.y);
}

// The wave's sums of a thread-private record into red_wave[0 .. kNSum) (LDS, this wave's row): the halving above, then the four DPP
// steps.  Slots NA .. 39 of red_wave are written as 0.  The caller sums the waves' rows in a fixed order after a barrier.
// (value 37 of the weighted record rides in the upper half-wave of h1[17], then in row 3 of h2[7])
template <int NA>
__device__ __forceinline__ void acc_wave_reduce(AccN<NA> &a, double *red_wave)
{
    static_assert(kNSum == 40 && NA <= 40, "the halving below pairs value k with k + 20, then k + 10");
    const int lane = threadIdx.x & 63;
    double h1[20], h2[10];
#pragma unroll
    for (int k = 0; k < 20; k++) h1[k] = swap32_add(k < NA ? a.v[k] : 0.0, k + 20 < NA ? a.v[k + 20] : 0.0);
#pragma unroll
    for (int k = 0; k < 10; k++) h2[k] = swap16_add(h1[k], h1[k + 10]);
#pragma unroll
    for (int k = 0; k < 10; k++) {
        double x = h2[k];
        x = dpp_add_f64<0x111, 0xf>(x);      // row_shr:1
        x = dpp_add_f64<0x112, 0xf>(x);      // row_shr:2
        x = dpp_add_f64<0x114, 0xf>(x);      // row_shr:4
        x = dpp_add_f64<0x118, 0xf>(x);      // row_shr:8  -> lane 15 of each row holds the row sum
        if ((lane & 15) == 15) red_wave[k + 10 * (lane >> 4)] = x;
    }
}

// block reduction: wave sums, then LDS across the 4 waves; fixed order -> deterministic.
// record k of block b lands at partials[b * kNSum + k]: one contiguous 320-byte burst per block.  (Round 2 stored it transposed,
// [k][block], so that the reduce could read along the blocks: 40 scattered 8-byte stores per block into lines shared with up to 15
// other blocks -- on other XCDs, i.e. other L2s -- and a reduce whose load phase alone took 5.9 us of k_reduce_solve's 11.5.)
template <int NA>
__device__ __forceinline__ void acc_block_reduce_store(AccN<NA> &a, double *partials, uint32_t col)
{
    __shared__ double red[(kPassThreads / 64) * kNSum];
    acc_wave_reduce(a, red + (threadIdx.x >> 6) * kNSum);
    __syncthreads();
    if (threadIdx.x < kNSum) {
        double s = 0.0;
        if (threadIdx.x < NA) {
#pragma unroll
            for (int w = 0; w < kPassThreads / 64; w++) s += red[w * kNSum + threadIdx.x];
        }
        partials[(size_t)col * kNSum + threadIdx.x] = s;
    }
}

}  // namespace symmicp
