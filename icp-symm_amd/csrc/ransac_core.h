// ransac_core.h -- the per-hypothesis arithmetic of symmicp_ctx_ransac (include/symmicp.h), shared by the kernels
// (kernels_global.hip, T = float) and the host (engine_global.cpp: the winner's inlier set).  Unfused, in the association written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "symmicp.h"

namespace symmicp {

__host__ __device__ inline unsigned long long ransac_mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the base of the SplitMix64 sequence of (seed, stream 0): symmicp.synth.splitmix64
__host__ __device__ inline unsigned long long ransac_base(unsigned long long seed)
{
    return ransac_mix64(seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull);
}

// draw number i of the sequence, mapped to 0 .. m - 1
__host__ __device__ inline uint32_t ransac_draw(unsigned long long base, unsigned long long i, uint32_t m)
{
    const unsigned long long u = ransac_mix64(base + (i + 1ull) * 0x9E3779B97F4A7C15ull);
    return (uint32_t)(((u >> 32) * (unsigned long long)m) >> 32);
}

template <class T> __host__ __device__ inline T rc_dot(const T a[3], const T b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
template <class T> __host__ __device__ inline void rc_cross(const T a[3], const T b[3], T o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__host__ __device__ inline float rc_sqrt(float x) { return sqrtf(x); }
__host__ __device__ inline double rc_sqrt(double x) { return sqrt(x); }

// |R p + t - q|^2 for Rt = R row-major, then t
template <class T> __host__ __device__ inline T ransac_residual2(const T Rt[12], const T p[3], const T q[3])
{
    const T dx = (((Rt[0] * p[0] + Rt[1] * p[1]) + Rt[2] * p[2]) + Rt[9]) - q[0];
    const T dy = (((Rt[3] * p[0] + Rt[4] * p[1]) + Rt[5] * p[2]) + Rt[10]) - q[1];
    const T dz = (((Rt[6] * p[0] + Rt[7] * p[1]) + Rt[8] * p[2]) + Rt[11]) - q[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the frame [e1 e2 e3] of a triangle a, b, c with u = b - a, v = c - a (the caller has checked that it is not degenerate)
template <class T> __host__ __device__ inline void rc_frame(const T u[3], const T v[3], T e1[3], T e2[3], T e3[3])
{
    const T lu = rc_sqrt(rc_dot(u, u));
    e1[0] = u[0] / lu; e1[1] = u[1] / lu; e1[2] = u[2] / lu;
    T w[3];
    rc_cross(e1, v, w);
    const T lw = rc_sqrt(rc_dot(w, w));
    e3[0] = w[0] / lw; e3[1] = w[1] / lw; e3[2] = w[2] / lw;
    rc_cross(e3, e1, e2);
}

// the base of the sequence of (seed, stream 1): the tuple trials of symmicp_ctx_fgr
__host__ __device__ inline unsigned long long ransac_base_stream1(unsigned long long seed)
{
    return ransac_mix64(seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull);
}

// the EDGE check: does an edge of the sample triangle (0-1, 1-2, 2-0) differ between the clouds by more than the ratio whose square is
// edge2?  Shared by the RANSAC hypotheses and the tuple test of symmicp_ctx_fgr.
template <class T>
__host__ __device__ inline bool ransac_edge_fails(const T P[3][3], const T Q[3][3], T edge2)
{
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int a = k, b = (k + 1) % 3;
        const T dp[3] = {P[a][0] - P[b][0], P[a][1] - P[b][1], P[a][2] - P[b][2]};
        const T dq[3] = {Q[a][0] - Q[b][0], Q[a][1] - Q[b][1], Q[a][2] - Q[b][2]};
        const T lp = rc_dot(dp, dp), lq = rc_dot(dq, dq);
        if (lp < edge2 * lq || lq < edge2 * lp) return true;
    }
    return false;
}

// status of the hypothesis drawn as c[0..2] with sample points P[k], Q[k]; Rt is written for EVALUATED and FAR
template <class T>
__host__ __device__ inline int ransac_hypothesis(const uint32_t c[3], const T P[3][3], const T Q[3][3], T edge2, T max_dist2, T Rt[12])
{
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return SYMMICP_RANSAC_REPEATED;
    if (edge2 > (T)0 && ransac_edge_fails<T>(P, Q, edge2)) return SYMMICP_RANSAC_EDGE;
    const T up[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, vp[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    const T uq[3] = {Q[1][0] - Q[0][0], Q[1][1] - Q[0][1], Q[1][2] - Q[0][2]}, vq[3] = {Q[2][0] - Q[0][0], Q[2][1] - Q[0][1], Q[2][2] - Q[0][2]};
    T wp[3], wq[3];
    rc_cross(up, vp, wp);
    rc_cross(uq, vq, wq);
    const T prod_p = rc_dot(up, up) * rc_dot(vp, vp), prod_q = rc_dot(uq, uq) * rc_dot(vq, vq);
    if (!(prod_p > (T)0) || !(prod_q > (T)0) || rc_dot(wp, wp) < (T)1e-4 * prod_p || rc_dot(wq, wq) < (T)1e-4 * prod_q)
        return SYMMICP_RANSAC_DEGENERATE;
    T fp[3][3], fq[3][3];
    rc_frame(up, vp, fp[0], fp[1], fp[2]);
    rc_frame(uq, vq, fq[0], fq[1], fq[2]);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = (fq[0][i] * fp[0][j] + fq[1][i] * fp[1][j]) + fq[2][i] * fp[2][j];
    T mp[3], mq[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        mp[i] = ((P[0][i] + P[1][i]) + P[2][i]) / (T)3;
        mq[i] = ((Q[0][i] + Q[1][i]) + Q[2][i]) / (T)3;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) Rt[9 + i] = mq[i] - ((Rt[3 * i] * mp[0] + Rt[3 * i + 1] * mp[1]) + Rt[3 * i + 2] * mp[2]);
#pragma unroll
    for (int k = 0; k < 3; k++)
        if (!(ransac_residual2<T>(Rt, P[k], Q[k]) <= max_dist2)) return SYMMICP_RANSAC_FAR;
    return SYMMICP_RANSAC_EVALUATED;
}

}  // namespace symmicp
