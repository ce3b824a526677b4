// plane_core.h -- the per-hypothesis arithmetic of symmicp_ctx_segment_plane (include/symmicp.h), shared by the kernels
// (kernels_plane.hip, T = float) and the host (tests/cpp/plane_core.cpp; engine_plane.cpp).  Unfused, in the association written.
#pragma once
#include "ransac_core.h"

namespace symmicp {

// the base of the SplitMix64 sequence of (seed, stream 2): the samples of symmicp_ctx_segment_plane
__host__ __device__ inline unsigned long long plane_base(unsigned long long seed)
{
    return ransac_mix64(seed * 0x9E3779B97F4A7C15ull + 2ull * 0xD1B54A32D192ED03ull + 0x2545F4914F6CDD1Dull);
}

template <class T> __host__ __device__ inline T plane_abs(T x) { return x < (T)0 ? -x : x; }

// signed offset of p from the plane nd = (n, d): ((n0 p0 + n1 p1) + n2 p2) + d
template <class T> __host__ __device__ inline T plane_offset(const T nd[4], const T p[3]) { return rc_dot(nd, p) + nd[3]; }

// status of the hypothesis drawn as c[0..2] with sample points P[k] (about the pivot); nd is written for EVALUATED and OFF_AXIS.
// have_axis: axis is the unit axis of the constraint, and cos_min bounds |n . axis| from below.
template <class T>
__host__ __device__ inline int plane_hypothesis(const uint32_t c[3], const T P[3][3], bool have_axis, const T axis[3], T cos_min, T nd[4])
{
    if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) return SYMMICP_PLANE_REPEATED;
    const T u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]}, v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
    T w[3];
    rc_cross(u, v, w);
    const T prod = rc_dot(u, u) * rc_dot(v, v), ww = rc_dot(w, w);
    if (!(prod > (T)0) || ww < (T)1e-4 * prod) return SYMMICP_PLANE_DEGENERATE;
    const T lw = rc_sqrt(ww);
    nd[0] = w[0] / lw; nd[1] = w[1] / lw; nd[2] = w[2] / lw;
    nd[3] = -rc_dot(nd, P[0]);
    if (have_axis && plane_abs(rc_dot(nd, axis)) < cos_min) return SYMMICP_PLANE_OFF_AXIS;
    return SYMMICP_PLANE_EVALUATED;
}

}  // namespace symmicp
