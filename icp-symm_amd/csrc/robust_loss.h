// robust_loss.h -- the M-estimator weights of the robust loop (symmicp_set_robust_loss).  ONE source for both sides, like
// solve_core.h: the weighted instantiations of the pass kernels (kernels_pass.hip) and symmicp_robust_weight on the host
// evaluate the same fp32 expressions.  With u = r / scale:
//   Huber          1 if |u| <= 1, else 1 / |u|
//   Tukey          (1 - u^2)^2 if |u| < 1, else 0
//   Cauchy         1 / (1 + u^2)
//   Geman-McClure  1 / (1 + u^2)^2
// Run as iteratively reweighted least squares: each pass weights every pair by w(r) of its residual at the pair's current
// position and the solve is the ordinary one on the weighted sums.
#pragma once
#include "symmicp.h"

#if defined(__HIPCC__)
#define SYMMICP_RW_HD __host__ __device__
#else
#define SYMMICP_RW_HD
#endif
#pragma clang fp contract(off)

namespace symmicp {

// loss is a validated SYMMICP_LOSS_* other than NONE and scale a finite positive number (the setter checks both)
SYMMICP_RW_HD inline float robust_weight(int loss, float scale, float r)
{
    const float u = r / scale;
    const float au = u < 0.0f ? -u : u;
    const float u2 = u * u;
    switch (loss) {
    case SYMMICP_LOSS_HUBER: return au <= 1.0f ? 1.0f : 1.0f / au;
    case SYMMICP_LOSS_TUKEY: { const float t = 1.0f - u2; return au < 1.0f ? t * t : 0.0f; }
    case SYMMICP_LOSS_CAUCHY: return 1.0f / (1.0f + u2);
    case SYMMICP_LOSS_GEMAN_MCCLURE: { const float t = 1.0f + u2; return 1.0f / (t * t); }
    default: return 1.0f;
    }
}

}  // namespace symmicp
