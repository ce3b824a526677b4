/*
 * symmicp.h -- C-ABI of libsymmicp, the MI355X (gfx950) symmetric-ICP engine.
 *
 * This is the drop-in boundary for the ONE hot path of StephenNG59/ICP-symm:
 * the MyICP::RegisterSymm() iteration loop (reference ICP/myicp.cpp:100-150)
 * and the free functions it calls (reference ICP/func.cpp:19-121).  Every
 * entry point below names the reference interface it replaces.  Plain
 * pointers and sizes only; no C++ or torch types.  The C++ class of the
 * reference (ICP/myicp.h:7-36) is mirrored on top of this ABI by
 * include/myicp.h.
 *
 * Threading: one ctx = one host thread = one GPU (one rank).  Multi-GPU runs
 * are one process (or thread) per GPU, joined by symmicp_comm_init_rank (RCCL)
 * or symmicp_comm_init_shm (ranks of one node).
 * Errors: every call returns SYMMICP_OK or an error code; the message is
 * available from symmicp_last_error().  The library never falls back to a
 * CPU path: without a usable HIP device symmicp_create fails.
 */
#ifndef SYMMICP_H
#define SYMMICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SYMMICP_NSUM 40            /* doubles per reduction record, see symmicp_sums layout */
#define SYMMICP_UNIQUE_ID_BYTES 128

typedef enum {
    SYMMICP_OK = 0,
    SYMMICP_ERR_ARG = 1,           /* null / out-of-range argument */
    SYMMICP_ERR_SIZE = 2,          /* empty cloud, or N_s != N_t with identity pairing (func.cpp:21 assert) */
    SYMMICP_ERR_DEGENERATE = 3,    /* rank-deficient system / non-finite transform (func.cpp:70,96 produce NaN) */
    SYMMICP_ERR_IO = 4,
    SYMMICP_ERR_HIP = 5,           /* HIP runtime error or no gfx950-capable device */
    SYMMICP_ERR_STATE = 6,         /* call out of order (e.g. step before begin) */
    SYMMICP_ERR_COMM = 7,          /* RCCL or shared-memory exchange error */
    SYMMICP_ERR_NO_CONSENSUS = 8,  /* symmicp_ctx_ransac: no hypothesis was evaluated, or the best one has fewer than 3 inliers;
                                      symmicp_ctx_fgr: no trial passed the tuple test */
    SYMMICP_ERR_INTERNAL = 9       /* a bound the library's own reasoning guarantees did not hold (symmicp_ctx_orient_normals: more than
                                      32 rounds, or a walk up the parents longer than the round's hooks) */
} symmicp_status;

/* Arithmetic mode.  QUIRKS reproduces the reference exactly as written:
 * un-centred rows (func.cpp:51-58), alternating a-then-t 3x3 solves seeded
 * with qbar-pbar (func.cpp:86-88), reversed composition (func.cpp:95-99) and
 * the full affine applied to the normals (myicp.cpp:137).  PAPER is the
 * formulation the reference's own comments intend (func.cpp:84,94;
 * Rusinkiewicz 2019): centred rows, joint 6x6 solve, T(q)RT(t)RT(-p),
 * normals rotated only.  P2P is the closed-form point-to-point fit of the reference's
 * regist.h:8-72 (registrateNPoint: centroids, 3x3 cross-covariance, SVD, reflection fix) run as an
 * ICP loop -- what the RegisterP2P stub (myicp.cpp:43-59) was heading for; record slots 0..8 then hold
 * sum p q^T instead of the symmetric-objective Gram matrix.  PLANE is point-to-plane ICP (Chen-Medioni):
 * minimise sum ((R p + t - q) . n_q)^2 with the TARGET's normals only; pivot, CUMULATIVE default and rotated-only normals
 * as PAPER.  Its record uses PAPER's slots with n_p = 0 and s = p + q replaced by p: v_i = (p_i x n_q, n_q),
 * c_i = (p_i - q_i) . n_q, both points about the pivot; the increment is T(pbar + t) R T(-pbar) with R = AngleAxis(|a|, a/|a|)
 * about the (weighted) source centroid.  PLANE alone needs no source normals: symmicp_set_source takes nrm == NULL then.
 * GICP is plane-to-plane ICP, the Generalized-ICP of Segal, Haehnel and Thrun (2009) with the usual regularised covariances
 * built from the normals: C_x = I - (1 - eps) x x^T for a normal x (eps: symmicp_set_gicp_epsilon, default 1e-3).  It minimises
 * sum d^T M d, d = R p + t - q, M = (C_q + R C_p R^T)^-1, linearised about the pivot as PLANE.  For the moved source normal a
 * and the target normal b, with u = a + b, v = a - b and cs = a . b, M has the closed form
 *   M = 1/2 I + gu u u^T + gv v v^T,  gu = (1 - eps) / (4 (2 - (1 - eps)(1 + cs))),  gv = (1 - eps) / (4 (2 - (1 - eps)(1 - cs)))
 * (exact for unit normals).  The mode is DEFINED by this formula with cs clamped to [-1, 1], so that it holds for any input:
 * zero normals give M = 1/2 I (a point-to-point pair), non-unit normals get the formula as stated.  GICP needs the normals of
 * both clouds; pivot, CUMULATIVE default, rotated-only normals and the solve (PLANE's, about the weighted source centroid) as
 * PLANE.  COLOR is colored ICP (Park, Zhou, Koltun 2017; Open3D's registration_colored_icp) on one scalar intensity per point: every
 * pair carries PLANE's geometric row at weight lambda and a photometric row at weight omega = 1.0f - lambda (fp32), the difference
 * between the source point's intensity I_p and a first-order model of the target's intensity on its tangent plane, I_q + g_q . (p - q)
 * with g_q the target's intensity gradient (tangent to the surface; symmicp_ctx_intensity_gradient estimates it).  The mode is
 * DEFINED by its rows (see symmicp_sums); pivot, CUMULATIVE default, rotated-only normals, the gates, trimming and the solve are
 * PLANE's, and only the target's normals enter the rows.  Source normals stay required (nrm == NULL is PLANE-only); they are read
 * under PLANE's rule (write-back or min_normal_dot).  lambda: symmicp_set_color_weight; the attributes: symmicp_set_source_intensity
 * and symmicp_set_target_intensity.  Out of scope, refused: sharded contexts (nranks > 1: SYMMICP_ERR_STATE), the fused pass and the
 * device-driven loop (symmicp_align runs the host loop, as it does for a trimming context).  NDT is the Normal Distributions
 * Transform (Biber and Strasser 2003, Magnusson 2009; pcl::NormalDistributionsTransform): a source point is paired with the Gaussian
 * of the target VOXEL it falls into, not with a target point -- no search, no normals, no index; its definition has a section of its
 * own below ("NDT registration").  Modes 4, 6 and 8 are unassigned and stay refused. */
typedef enum { SYMMICP_MODE_QUIRKS = 0, SYMMICP_MODE_PAPER = 1, SYMMICP_MODE_P2P = 2, SYMMICP_MODE_PLANE = 3,
               SYMMICP_MODE_GICP = 5, SYMMICP_MODE_COLOR = 7, SYMMICP_MODE_NDT = 9 } symmicp_mode;

/* Correspondence.  IDENTITY is what the reference does (myicp.cpp:130, the
 * search is a todo at :128-131).  BRUTE and TREE are exact nearest neighbour
 * (ties -> lowest target index) by LDS-tiled brute force, or by the index
 * built over the Morton-sorted target (cell table + sparse octree; once an
 * alignment has converged, per-pair certificates prove the pair unchanged and
 * the search is skipped). */
typedef enum { SYMMICP_CORR_IDENTITY = 0, SYMMICP_CORR_BRUTE = 1, SYMMICP_CORR_TREE = 2 } symmicp_corr;

/* How the source is advanced.  INCREMENTAL rewrites source points and normals
 * with each incremental transform, as applyTransform does (func.cpp:104-121,
 * myicp.cpp:136-137), so the fp32 rounding history matches the reference.
 * CUMULATIVE never rewrites the source: each pass applies the accumulated 4x4
 * to the original points (<= ~1e-6 relative drift, 24 B/point less traffic). */
typedef enum { SYMMICP_APPLY_DEFAULT = 0, SYMMICP_APPLY_INCREMENTAL = 1, SYMMICP_APPLY_CUMULATIVE = 2 } symmicp_apply;

/* Robust loss (symmicp_set_robust_loss): every pair is weighted by w(r / scale) of its residual r, run as iteratively
 * reweighted least squares (each pass weights the pairs at their current position; the solve is the usual one on the
 * weighted sums).  r is, in PAPER, c = (p - q) . (n_p + n_q), the quantity whose square the symmetric objective sums --
 * so `scale` is in units of c, about TWICE the point-to-plane distance when the two normals agree -- in PLANE
 * r = c = (p - q) . n_q, the signed point-to-plane distance itself (`scale` in plain length units), in GICP
 * r = sqrt(d^T M d), the pair's Mahalanobis distance (about 1/sqrt(2) of |p - q| across the planes, larger along the normals),
 * in COLOR r = sqrtf((lambda*c_G)*c_G + (omega*c_C)*c_C) (both rows are scaled by the pair's weight, as GICP scales its rows),
 * and in P2P r = |p - q|.  With u = r / scale:
 *   HUBER          1 if |u| <= 1, else 1/|u|
 *   TUKEY          (1 - u^2)^2 if |u| < 1, else 0
 *   CAUCHY         1 / (1 + u^2)
 *   GEMAN_MCCLURE  1 / (1 + u^2)^2
 * computed in fp32.  QUIRKS stays the reference as written: it takes no loss. */
typedef enum { SYMMICP_LOSS_NONE = 0, SYMMICP_LOSS_HUBER = 1, SYMMICP_LOSS_TUKEY = 2,
               SYMMICP_LOSS_CAUCHY = 3, SYMMICP_LOSS_GEMAN_MCCLURE = 4 } symmicp_loss;

typedef struct {
    int32_t struct_size;       /* = sizeof(symmicp_config), checked */
    int32_t device;            /* HIP device ordinal; -1 = current */
    int32_t mode;              /* symmicp_mode */
    int32_t corr;              /* symmicp_corr */
    int32_t apply;             /* symmicp_apply; DEFAULT = INCREMENTAL for QUIRKS, CUMULATIVE for PAPER */
    int32_t max_iters;         /* myicp.cpp:6   default 10 */
    float diff_threshold;      /* myicp.cpp:6   default 1.0, loop runs while diff > threshold (myicp.cpp:123) */
    float max_corr_dist;       /* <= 0: keep every pair; else pairs farther than this are dropped */
    int32_t fixed_iters;       /* != 0: ignore the threshold, run exactly max_iters iterations */
    int32_t sort_source;       /* != 0 (default for BRUTE/TREE): Morton-sort the source shard for locality */
    int32_t verbose;           /* != 0: print the reference's stdout lines (myicp.cpp:125-126,146-149) */
    /* robustness options of the paper-style loop; all off by default = reference behaviour */
    float min_normal_dot;      /* > -1: drop pairs whose (transformed) source normal . target normal is below this */
    float eps_rotation;        /* > 0 (radians) together with eps_translation > 0: also stop once an increment */
    float eps_translation;     /*   rotates by less than eps_rotation and translates by less than eps_translation */
    int32_t host_loop;         /* != 0: symmicp_align never hands runs of iterations to the device (every solve on the host, as symmicp_step does) */
    int32_t reserved[1];
} symmicp_config;

/* One reduction record = everything the host needs from one pass over the
 * source.  v_i = (M_i, N_i) is the 6-vector of
 * func.cpp:54,56 and c_i the scalar of func.cpp:58.
 *   [0..20]  upper triangle, row-major, of sum_i v_i v_i^T
 *   [21..26] sum_i v_i c_i
 *   [27..29] sum_i p_i        [30..32] sum_i q_i   (about `pivot`, see symmicp_get_pivot)
 *   [33] sum_i |p_i - q_i|   (evalDiff, func.cpp:19-32, over the current pairs)
 *   [34] number of pairs     [35] sum_i c_i^2      [36] sum_i |p_i - q_i|^2
 *   [37..39] reserved (0)
 * PLANE: v_i = (p_i x n_q, n_q) and c_i = (p_i - q_i) . n_q in fp32, unfused: m0 = py*nz - pz*ny, m1 = pz*nx - px*nz,
 *   m2 = px*ny - py*nx, c = (dx*nx + dy*ny) + dz*nz with n = n_q, d = p - q (p, q about the pivot); every other slot as above.
 * GICP: five rows per pair of PLANE's form v = (p x l, l), c = l . d, each with a weight o (M = sum o l l^T, see symmicp_mode):
 *   l = e_x, e_y, e_z at o = 1/2; l = u at gu; l = v at gv (u, v, gu, gv in fp32, unfused, cs clamped; rows as PLANE's with n = l)
 *   [0..20]  sum_i sum_l o v v^T  (the axis rows summed as 1/2 J^T J, J = [-[p]x, I])     [21..26] sum_i sum_l o v c
 *   [27..32] sum p, sum q once per PAIR, not per row (PLANE's solve centres on the source centroid)
 *   [35] sum_i d^T M d (= sum_i sum_l o c^2)                every other slot as above.
 *   The record has PLANE's shape: symmicp_solve(SYMMICP_MODE_GICP) is PLANE's solve.
 * COLOR: two rows per pair of PLANE's form, fp32, unfused, in the association written; p, q about the pivot, d = p - q, n = n_q, g = g_q:
 *   geometric    v = (p x n, n) formed exactly as PLANE's, c_G = (dx*nx + dy*ny) + dz*nz, at weight lambda
 *   photometric  v = (p x g, g) formed the same way,      c_C = ((dx*gx + dy*gy) + dz*gz) + (I_q - I_p), at weight omega = 1.0f - lambda
 *   [0..26] sum o v v^T and sum o v c over both rows     [35] sum (lambda c_G^2 + omega c_C^2)
 *   [27..34], [36], [37] once per pair, as PLANE.  symmicp_solve(SYMMICP_MODE_COLOR) is PLANE's solve.
 *   At lambda = 1 every photometric term is multiplied by an exact zero: for finite g and I the record is PLANE's, bit for bit.
 * With a robust loss set (symmicp_set_robust_loss), w_i = the pair's weight:
 *   [0..32], [35]  the same sums with every pair scaled by w_i: sum w v v^T, sum w v c, sum w p, sum w q, sum w c^2
 *                  (P2P: sum w p q^T and the weighted coordinate sums; GICP: every row of the pair scaled by w_i)
 *   [34] sum_i w_i (the solves centre on the weighted centroids)
 *   [33], [36]     unweighted, as above (the stop rule and `diff` keep their meaning)
 *   [37] number of pairs (what symmicp_iter_result.pairs reports then)
 * With SYMMICP_LOSS_NONE the record is exactly the unweighted one and [37] stays 0. */
typedef struct { double s[SYMMICP_NSUM]; } symmicp_sums;

typedef struct {
    int32_t status;            /* symmicp_status of this iteration */
    int32_t iter;              /* iterations completed so far */
    float diff;                /* sum |p-q| after this iteration's update (myicp.cpp:141) */
    float rcond;               /* smallest/largest eigenvalue of the solved system(s) */
    double pairs;              /* correspondences that entered the sums (slot 34, or slot 37 with a robust loss) */
    float increment[16];       /* row-major 4x4 of this iteration (func.cpp:91-101) */
    symmicp_sums sums;         /* record the NEXT solve will use (already all-reduced) */
} symmicp_iter_result;

typedef struct {
    int32_t status;
    int32_t iters;             /* iterations run */
    float diff_initial;        /* myicp.cpp:122 */
    float diff_final;
    float transform[16];       /* row-major 4x4, original source -> target (myicp.cpp:138,147) */
    float diffs[64];           /* diff printed at the top of each of the first 64 iterations (myicp.cpp:126) */
    double seconds_total;      /* wall time of the loop */
} symmicp_result;

typedef struct symmicp_ctx symmicp_ctx;

/* ---- lifetime ---------------------------------------------------------- */
void symmicp_config_default(symmicp_config *cfg);                 /* MyICP::MyICP, myicp.cpp:6 */
int symmicp_create(const symmicp_config *cfg, symmicp_ctx **out); /* MyICP::MyICP, myicp.cpp:6-14 */
void symmicp_destroy(symmicp_ctx *ctx);                           /* MyICP::~MyICP, myicp.cpp:16-18 */
const char *symmicp_last_error(const symmicp_ctx *ctx);           /* (reference has none: asserts / silent NaN) */
int symmicp_set_config(symmicp_ctx *ctx, const symmicp_config *cfg);   /* myicp.h:19 "todo add params" */
int symmicp_version(void);
/* Robust loss of the PAPER, PLANE and P2P loops (symmicp_loss above; off = SYMMICP_LOSS_NONE, the default).  SYMMICP_ERR_ARG for
 * an unknown loss, for a scale that is not finite and > 0 while loss != NONE, and for any loss in SYMMICP_MODE_QUIRKS
 * (symmicp_set_config refuses to switch a context with a loss into QUIRKS the same way).  Takes effect at the next pass:
 * it may be called between symmicp_step calls (e.g. to anneal the scale); a device-driven run inside symmicp_align keeps
 * the values it started with.  Sharded runs: every rank sets the same values. */
int symmicp_set_robust_loss(symmicp_ctx *ctx, int loss, float scale);
int symmicp_get_robust_loss(const symmicp_ctx *ctx, int *loss, float *scale);
/* The eps of SYMMICP_MODE_GICP's covariances C = I - (1 - eps) n n^T: 0 < eps <= 1, finite and 1.0f - eps != 1.0f (eps > 2^-25),
 * else SYMMICP_ERR_ARG and the eps set before stays; default 1e-3 (PCL's and Segal's).  The kernels use fl32(1 - eps): an eps that
 * rounds it to 1 would make a pair of equal normals singular, and an eps below ~1e-5 is quantised by up to 2^-25 / eps relative.
 * Accepted in every mode, read by GICP only.  eps = 1 makes every pair point-to-point (M = 1/2 I).  Takes
 * effect at the next pass; a device-driven run inside symmicp_align keeps the value it started with.  Sharded runs: every rank
 * sets the same value. */
int symmicp_set_gicp_epsilon(symmicp_ctx *ctx, float eps);
int symmicp_get_gicp_epsilon(const symmicp_ctx *ctx, float *eps);
/* The lambda of SYMMICP_MODE_COLOR: the geometric rows weigh lambda, the photometric ones 1.0f - lambda.  0 <= lambda <= 1 and
 * finite, else SYMMICP_ERR_ARG and the value set before stays; default 0.968f (Open3D's lambda_geometric).  Accepted in every mode,
 * read by COLOR only.  Takes effect at the next pass. */
int symmicp_set_color_weight(symmicp_ctx *ctx, float lambda);
int symmicp_get_color_weight(const symmicp_ctx *ctx, float *lambda);
/* Trimmed ICP (Chetverikov, Stepanov, Krsek 2002/2005; PCL's CorrespondenceRejectorTrimmed, libpointmatcher's
 * TrimmedDistOutlierFilter): each pass keeps the closest fraction rho of its pairs -- the rejection rule for clouds that overlap only
 * in part.  A pure function of the pass:
 *   Candidates  the pairs of the pass that exist (a target row >= 0) and pass the gates (max_corr_dist, then min_normal_dot), exactly
 *               as every accumulating kernel applies them; n_c = their number.
 *   Distance    d2 = the pair's fp32 squared distance (dx*dx + dy*dy) + dz*dz at the moved position: the same bits the accumulating
 *               kernels evaluate.
 *   Threshold   k = ceil((double)rho * (double)n_c) with rho the fp32 fraction, clamped to [1, n_c]; tau = the k-th smallest
 *               candidate d2.
 *   Kept set    the candidates with d2 <= tau.  Ties at tau are all kept, so the kept count is >= k.  n_c == 0: nothing is kept
 *               (tau is reported as 0) and the solve reports SYMMICP_ERR_DEGENERATE as it does for any empty record.
 *   Off         rho == 1, the default: nothing new is launched, every result is bit for bit that of a build without trimming.
 *   Record      the ordinary one over the kept set: slots 33, 34, 36 and 37 count kept pairs only, exactly as a pair dropped by
 *               max_corr_dist is left out; a robust loss weights the kept pairs.
 * All symmicp_corr values; modes PAPER, P2P, PLANE and GICP.  QUIRKS stays the reference as written: a fraction below 1 is
 * SYMMICP_ERR_ARG there, and symmicp_set_config refuses to switch a trimming context into QUIRKS the same way.
 * SYMMICP_ERR_ARG unless 0 < fraction <= 1 (NaN is refused too); the fraction set before stays.  Takes effect at the next pass: it may
 * be called between symmicp_step calls.  tau is an exact order statistic found on the device every pass (a radix select over the d2
 * bits); the fused pass and the device-driven loop are not extended: with a fraction below 1 symmicp_align runs every iteration in
 * the host loop (as cfg.host_loop does).  symmicp_get_correspondences then reports a pair that was trimmed away -- or gated: not a
 * candidate -- as rejected (-1).  Sharded contexts would need a quantile over all ranks and are out of scope: a fraction below 1 on a
 * context with nranks > 1, and symmicp_comm_init_rank / _shm with nranks > 1 on a trimming context, return SYMMICP_ERR_STATE. */
int symmicp_set_trim_fraction(symmicp_ctx *ctx, float fraction);
int symmicp_get_trim_fraction(const symmicp_ctx *ctx, float *fraction);
/* n_c, the kept count and tau of the most recent pass (each pointer may be NULL); SYMMICP_ERR_STATE if no pass has run or that pass
 * was not trimmed */
int symmicp_get_trim_state(const symmicp_ctx *ctx, uint64_t *candidates, uint64_t *kept, float *tau_d2);
/* One-to-one and median-distance rejection (PCL's CorrespondenceRejectorOneToOne and CorrespondenceRejectorMedianDistance): two more
 * rules for clouds that overlap only in part, neither of which needs to know the overlap.  Both are pure functions of the pass,
 * reproducible bit for bit, and off by default; with both off nothing new is launched and every result is bit for bit what it is
 * without them.
 *   Candidates  as for trimming: the pairs that exist (a target row >= 0) and pass max_corr_dist, then min_normal_dot; n_c = their
 *               number.  d2 = the fp32 (dx*dx + dy*dy) + dz*dz at the moved position, the bits the accumulating kernels evaluate.
 *   One-to-one  (symmicp_set_one_to_one, on != 0).  The key of candidate i is K(i) = ((uint64)bits(d2_i) << 32) | r_i with r_i the source
 *               point's row in the caller's numbering.  The winner of target row j is the candidate paired with j that has the smallest
 *               K: the closest one, ties in d2 going to the lowest caller row.  A candidate survives iff it is the winner of its target;
 *               n_u = the number of survivors = the number of distinct target rows among the candidates.  A gated pair claims nothing:
 *               the gates come first.  SYMMICP_CORR_IDENTITY pairs are one-to-one as they are: the option is accepted there, launches
 *               nothing and n_u = n_c.
 *   Median      (symmicp_set_median_factor; 0 = off, the default; else finite and > 0, otherwise SYMMICP_ERR_ARG and the factor set
 *               before stays).  Over the population below, of size n: med = the k-th smallest d2 with k = ceil(0.5 n), the threshold of a
 *               trim fraction 0.5; f2 = factor * factor and tau = f2 * med, two unfused fp32 products.  A pair is kept iff
 *               bits(d2) <= bits(tau); tau = +Inf keeps all (so does the NaN of f2 = +Inf times med = 0, which counts as +Inf).  n == 0:
 *               tau is reported as 0 and nothing is kept.
 *   Order       the gates, then one-to-one, then the quantile rule (trim fraction or median), whose population is the one-to-one
 *               survivors when one-to-one is on, else the candidates.  A trim fraction below 1 together with a median factor > 0 is
 *               refused: whichever setter comes second returns SYMMICP_ERR_ARG.  With one-to-one alone every survivor is kept and tau is
 *               reported as +Inf.
 *   Record      the ordinary one over the kept set, as for trimming: slots 33, 34, 36 and 37 count kept pairs only, a robust loss weights
 *               the kept pairs, and symmicp_get_correspondences reports every rejected row as -1.
 * Scope as for trimming: all symmicp_corr values; every mode but QUIRKS, which refuses both options with SYMMICP_ERR_ARG (and
 * symmicp_set_config refuses to switch such a context into QUIRKS); nranks > 1 is SYMMICP_ERR_STATE in both directions (the claim table
 * would need a minimum over all ranks); symmicp_align runs every iteration in the host loop, and a TREE pass that rejects never skips
 * its tree walk.  Both setters take effect at the next pass and may be called between symmicp_step calls.  On the device: a claim of
 * target rows by 64-bit integer minimum (order-independent), then the keys and the radix select of trimming. */
int symmicp_set_one_to_one(symmicp_ctx *ctx, int on);
int symmicp_get_one_to_one(const symmicp_ctx *ctx, int *on);
int symmicp_set_median_factor(symmicp_ctx *ctx, float factor);
int symmicp_get_median_factor(const symmicp_ctx *ctx, float *factor);
/* n_c, n_u (= n_c when one-to-one is off), the kept count and tau of the most recent pass (each pointer may be NULL);
 * SYMMICP_ERR_STATE if no pass has run or that pass ran neither of these two rejectors.  symmicp_get_trim_state keeps working for
 * trimmed passes; its `candidates` is the select's population (n_u with one-to-one on).  `unique` is the select's population too: on a
 * reciprocal pass (symmicp_set_reciprocal) it is n_r, and symmicp_get_reciprocal_state has n_u. */
int symmicp_get_rejection_state(const symmicp_ctx *ctx, uint64_t *gated, uint64_t *unique, uint64_t *kept, float *tau_d2);
/* Reciprocal correspondences (PCL's setUseReciprocalCorrespondences): a pair (p, q) counts only if q is the nearest target point of p
 * AND p is the nearest source point of q.  symmicp_set_reciprocal(on != 0; off by default) is a pure function of the pass and
 * reproducible bit for bit.  The moving cloud is never re-indexed: the source is indexed once, in the frame symmicp_set_source received
 * it in, and every target point is carried into that frame by the inverse of the pass's transform.
 *   Inverse     X = the cumulative row-major 4x4 of the pass: it takes the original source to the positions this pass pairs, and it is
 *               what symmicp_get_transform returns after the call that ran the pass.  With R_rc = X[4r + c] and t_r = X[4r + 3], row r of
 *               the 3x4 inverse is (R_0r, R_1r, R_2r, -((R_0r t_0 + R_1r t_1) + R_2r t_2)), formed in fp64 from the fp32 entries (the
 *               products of two fp32 values are exact in fp64, so contraction cannot change it), then each entry rounded to fp32.  X's
 *               bottom row is ignored.  The rule is defined by this arithmetic whatever X is: for a guess that is not rigid it is not an
 *               inverse, and that is the caller's business.  symmicp_inverse_rigid below is this function.
 *   Back-       y_j = the three inverse rows applied to target point q_j with w = 1, in fp32 and unfused:
 *   projection  ((m0 x + m1 y) + m2 z) + m3.
 *   Reverse     back(j) = the source row i that minimises (d2'(i, j), r_i) lexicographically, with d2'(i, j) the fp32
 *   neighbour   (dx dx + dy dy) + dz dz of d = y_j - p_i, p_i the ORIGINAL source point as symmicp_set_source received it (never the
 *               written-back copy, in either apply mode) and r_i the caller's row.  The minimum runs over ALL source rows of the context,
 *               not only the candidates.
 *   Rule        Candidates as for one-to-one (the pair exists and passes max_corr_dist, then min_normal_dot).  The one-to-one claim runs
 *               first -- reciprocal implies it, with the same key K -- and the winner i of target j survives iff back(j) == r_i.
 *               n_u = the number of claimed targets, n_r = the number of survivors.  The quantile rule (trim fraction or median factor)
 *               then runs over the survivors exactly as it does over one-to-one's; with no quantile rule every survivor is kept and
 *               tau = +Inf.  Turning symmicp_set_one_to_one on as well changes nothing.
 *   Properties  The kept set is a subset of what one-to-one alone keeps in the same pass (its survivors), whatever quantile rule runs.
 *               In exact arithmetic and for rigid X the survivors are PCL's reciprocal set; the forward search runs in the target's
 *               frame and the reverse one in the source's, so near-ties at rounding level may resolve differently.
 *   Off         nothing new is launched or allocated, and results are bit for bit what they are without it.
 * Scope: every mode but QUIRKS (SYMMICP_ERR_ARG from the setter, and symmicp_set_config refuses to switch a reciprocal context into
 * QUIRKS); BRUTE and TREE pairings -- SYMMICP_CORR_IDENTITY is refused the same way in both directions, because its pairs were never
 * searched; nranks > 1 is SYMMICP_ERR_STATE in both directions, as for one-to-one; symmicp_align runs the host loop, and a rejecting
 * TREE pass never skips its walk.  The setter takes effect at the next pass.  On the device: an octree over the source, built at the
 * first reciprocal pass after a symmicp_set_source and kept until the next one, and between the claim and the keys one exact
 * nearest-neighbour walk of it per claimed target, which vetoes the claim of a winner that is not the reverse neighbour. */
int symmicp_set_reciprocal(symmicp_ctx *ctx, int on);
int symmicp_get_reciprocal(const symmicp_ctx *ctx, int *on);
/* n_u (claimed targets) and n_r (reciprocal survivors) of the most recent pass (each pointer may be NULL); SYMMICP_ERR_STATE if no pass
 * has run or that pass was not reciprocal.  On a reciprocal pass symmicp_get_rejection_state's `unique` is the select's population,
 * so n_r. */
int symmicp_get_reciprocal_state(const symmicp_ctx *ctx, uint64_t *claimed, uint64_t *reciprocal);
/* the 3x4 inverse of the definition above (a pure host function); SYMMICP_ERR_ARG for a NULL pointer */
int symmicp_inverse_rigid(const float X16[16], float out12[12]);
/* the weight the kernels give a pair of residual r (the same fp32 source); NaN for an unknown loss, or for a scale that
 * is not finite and > 0 with loss != NONE; 1 for SYMMICP_LOSS_NONE */
float symmicp_robust_weight(int loss, float scale, float r);

/* ---- clouds (replaces pasteInMatrix, func.cpp:5-15, myicp.cpp:110-111) --
 * Host arrays, element (i,k) at base[i*row_stride + k*col_stride] (floats):
 *   packed xyz AoS        row_stride=3, col_stride=1
 *   pcl::PointXYZ (16 B)  row_stride=4, col_stride=1
 *   pcl::PointNormal      xyz: base=&pt[0].x, 12,1 ; normals: base=&pt[0].normal_x, 12,1
 *   Eigen::MatrixXf Nx3   row_stride=1, col_stride=N   (column-major)
 * Data is copied to the device; the caller keeps ownership.  With a
 * communicator attached every rank passes the FULL cloud (same pointer arithmetic on every rank) and uploads only its own
 * share: rows [begin, begin + count) of symmicp_shard_range, Morton-sorted on the device; the target is replicated.
 * set_target also builds the search index when corr != IDENTITY.
 * Source normals are optional in SYMMICP_MODE_PLANE, and only there: set_source with nrm == NULL (strides ignored) is
 * accepted when cfg.mode == PLANE and SYMMICP_ERR_ARG in every other mode.  The engine then holds zero source normals:
 * while such a source is set, symmicp_set_config refuses any other mode (SYMMICP_ERR_STATE), min_normal_dot > -1 is refused
 * (SYMMICP_ERR_ARG: there is no source normal to gate on) and symmicp_get_source returns zero normals. */
int symmicp_set_source(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                       const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride, size_t n);
int symmicp_set_target(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                       const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride, size_t n);

/* Per-point attributes of SYMMICP_MODE_COLOR: one scalar intensity per source point; one intensity and its gradient (3 floats,
 * tangent to the surface: symmicp_ctx_intensity_gradient, or the caller's own) per target point.  intensity[i * stride], grad
 * element (i, k) at grad[i * grad_row_stride + k * grad_col_stride], rows as the cloud's.  Each call follows the cloud's
 * symmicp_set_source / symmicp_set_target (SYMMICP_ERR_STATE before it); n must equal that cloud's count (SYMMICP_ERR_SIZE); a NULL
 * pointer or a non-finite value is SYMMICP_ERR_ARG.  The engine keeps the values in the order it keeps the cloud (the target index's
 * Morton order; the order of a sorted source share).  A new symmicp_set_source / symmicp_set_target drops that cloud's attribute.
 * Accepted in every mode, read by COLOR only: there symmicp_begin / symmicp_align without both is SYMMICP_ERR_STATE.
 * symmicp_get_source_intensity reads the source's values back in the caller's row order (cap >= the source's count; rows outside
 * this rank's share stay 0). */
int symmicp_set_source_intensity(symmicp_ctx *ctx, const float *intensity, size_t stride, size_t n);
int symmicp_set_target_intensity(symmicp_ctx *ctx, const float *intensity, size_t stride,
                                 const float *grad, size_t grad_row_stride, size_t grad_col_stride, size_t n);
int symmicp_get_source_intensity(symmicp_ctx *ctx, float *intensity, size_t cap);

/* ---- the loop (replaces MyICP::RegisterSymm, myicp.cpp:117-142) -------- */
/* align = begin + step until the stop rule of myicp.cpp:123. guess16 may be NULL (identity). */
int symmicp_align(symmicp_ctx *ctx, const float *guess16, symmicp_result *out);
/* begin: evaluate the initial pairs/sums/diff (myicp.cpp:122); no update yet. */
int symmicp_begin(symmicp_ctx *ctx, const float *guess16, symmicp_iter_result *out);
/* step: one trip of the loop body: solve (func.cpp:76-102) -> compose -> apply
 * (func.cpp:104-121) -> new pairs + sums + diff (myicp.cpp:128-141). */
int symmicp_step(symmicp_ctx *ctx, symmicp_iter_result *out);
int symmicp_get_transform(const symmicp_ctx *ctx, float out16[16]);           /* myicp.cpp:147 */
/* The result block exactly as the reference prints it (myicp.cpp:146-149: "Result transform:" + transform.matrix(), "  rotation:" +
 * transform.rotation(), "  translation:" + transform.translation(), each through Eigen's default IOFormat: precision 6, every
 * coefficient right-aligned to the widest one of its matrix, one space between columns).  Writes at most cap - 1 characters and a
 * terminating 0; returns the length of the whole text (buf may be NULL to query it).  symmicp_align prints this when cfg.verbose. */
size_t symmicp_format_result(const float transform16[16], char *buf, size_t cap);
int symmicp_get_pivot(const symmicp_ctx *ctx, float out3[3]);
/* current pairs in ORIGINAL numbering: idx[i] = target row paired with source row i
 * (rows of this rank's share; -1 = rejected), d2[i] = squared distance. Either may be NULL.
 * Where row i is written: a Morton-sorted source (BRUTE and TREE with cfg.sort_source) writes the share's pairs at the caller's rows,
 * so cap >= the whole source's count and rows outside the share stay -1 / 0; an unsorted source (IDENTITY, or sort_source == 0)
 * writes them at share rows 0 .. symmicp_local_source_count() - 1 (caller row = symmicp_local_source_offset() + i), cap >= the
 * share's count.  With a single rank the two coincide.  (SYMMICP_CORR_IDENTITY and _TREE evaluate
 * the distances here, at the positions the last pass gave the points: a pass stores them only for the pairs it searched.) */
int symmicp_get_correspondences(symmicp_ctx *ctx, int32_t *idx, float *d2, size_t cap);
/* current (transformed) source points / normals of this rank's share, original row order, packed AoS. */
int symmicp_get_source(symmicp_ctx *ctx, float *xyz, float *nrm, size_t cap);
/* diagnostic (SYMMICP_CORR_TREE): the pair certificates of this rank's share in its sorted order: cert4 [n_loc][4] = position of the
 * query when its pair was last searched + the clear radius L (<= 0: no single certificate; bit 0 of the word: the neighbourhood is
 * valid); hood8 (may be NULL) [n_loc][8]: the neighbourhood's members as target rows (0xFFFFFFFF: empty); hood_radius (may be NULL)
 * [n_loc]: its radius T; winner_row (may be NULL) [n_loc]: the pair's current target row (-1: none) */
int symmicp_get_certificates(symmicp_ctx *ctx, float *cert4, uint32_t *hood8, float *hood_radius, int32_t *winner_row, size_t cap);
size_t symmicp_local_source_count(const symmicp_ctx *ctx);
size_t symmicp_local_source_offset(const symmicp_ctx *ctx);

/* ---- host-side pieces of func.cpp:76-102, exposed for parity tests ----- */
/* PAPER, PLANE, GICP and COLOR (PLANE's solve): pbar / qbar = the (weighted) centroids in the caller's frame, (a, t) the solved 6-vector; P2P: zeros */
int symmicp_solve(int mode, const symmicp_sums *sums, const float pivot[3],
                  float pbar[3], float qbar[3], float a[3], float t[3], float *rcond, float out16[16]);

/* ---- test entry points of the device-driven loop (off the hot path; a test's view of what the device does with a record) ----- */
/* The device's solve: solve_core.h compiled for gfx950, one thread per record, mode QUIRKS / PAPER / PLANE / GICP, with the host's exact
 * conditioning (exact_rc = 1) or the device loop's lower bound (exact_rc = 0).  Per record i: status[i], pbar / qbar / a / t [i][3],
 * rcond[i], out16[i][16] (the increment); with X_in16 != NULL also X_out16[i][16] = increment * X_in16[i] (mat4_mul, as the loop
 * composes).  pivot may be NULL (PAPER / PLANE / GICP: zero). */
int symmicp_ctx_solve_probe(symmicp_ctx *ctx, int mode, int exact_rc, const symmicp_sums *sums, size_t n, const float pivot[3],
                            const float *X_in16, int32_t *status, float *pbar, float *qbar, float *a, float *t, float *rcond,
                            float *out16, float *X_out16);
/* One solve-only run of the device loop's end-of-pass kernel (the first launch of every device-driven batch) on a given record and
 * loop state.  in_i = {mode, fixed_iters, max_iters, iters, small_step, incremental}, in_f = {diff_threshold, eps_rotation,
 * eps_translation}, X_in16 the cumulative transform before it.  Read back: state_out = {stop, reason, iters, small_step} (LOOP_*:
 * 0 running, 1 done, 3 handed back to the host solve), X_out16, Xapply_out12 (what the next pass would apply), and the ring record
 * the kernel wrote (unwritten fields keep the pattern 0xFF bytes): ring_inc16, ring_X16, ring_rcond, ring_i2 = {status, solved}. */
int symmicp_ctx_loop_solve(symmicp_ctx *ctx, const symmicp_sums *sums, const float pivot[3], const float X_in16[16], const int32_t in_i[6],
                           const float in_f[3], int32_t state_out[4], float X_out16[16], float Xapply_out12[12], float ring_inc16[16],
                           float ring_X16[16], float *ring_rcond, int32_t ring_i2[2]);
/* One pass of a device-driven run, as symmicp_align's log keeps it: the pass's record, the increment solved from it and the
 * transform after it (when solved), the batch's stop reason. */
typedef struct {
    double sums[SYMMICP_NSUM];
    float increment[16], X[16];
    float rcond;
    int32_t iter;        /* iteration count after this pass (the reference's `iters`) */
    int32_t status;      /* status of the device solve from this record */
    int32_t solved;      /* 1: increment / X are valid (the device went on) */
    int32_t list_len;    /* TREE: work-list length of this pass */
    int32_t reason;      /* stop reason of the batch this pass belongs to (LOOP_* as above; 4: slow, 2: redo pass) */
    int32_t batch;       /* 0, 1, ...: batches of this align */
    int32_t reserved;    /* TREE: the kernel that ran this pass: 0 fused, 1 certified-only (SYMMICP_CERT_PASS); + 0x100 on a batch's last
                          * entry when the pass behind it ran certified-only and was handed back to the host incomplete */
} symmicp_loop_log_entry;
/* on != 0: every later symmicp_align keeps the log of its device-driven passes (off by default: nothing is copied) */
int symmicp_set_loop_log(symmicp_ctx *ctx, int on);
/* the log of the last symmicp_align: *count entries in all, min(cap, *count) of them copied to out (out may be NULL) */
int symmicp_get_loop_log(const symmicp_ctx *ctx, symmicp_loop_log_entry *out, size_t cap, size_t *count);

/* ---- test entry points of the index build (off the hot path; read-only: clouds, index, certificates and statistics stay as they
 * were).  What a test compares with its own restatement of the build (tests/_index_ref.py). ----- */
typedef struct {
    int32_t struct_size;        /* sizeof(symmicp_index_info), set by the caller */
    uint32_t n;                 /* target points */
    int32_t grid_level;         /* level of the cell table (0: none) */
    int32_t gdim;               /* 1 << grid_level (0 without a table) */
    float origin[3];            /* bounding-box minimum: the Morton frame */
    float h0, h, inv_h;         /* finest cell edge; cell edge at grid_level and its inverse (0 without a table) */
    int32_t tree_levels;        /* levels of the box tree: top + 1 */
    int32_t top;                /* index of its top level */
    uint32_t ntop;              /* nodes in the top level */
    uint32_t level_off[12];     /* first node of every box-tree level */
    uint32_t n_boxes;           /* nodes of the box tree in all, padding included: boxes holds 2 float4 per node */
    uint32_t olevel_off[12];    /* first node of octree level 0 .. 10, and their total */
    uint32_t n_onodes;          /* = olevel_off[11]: onodes holds 2 float4 per node */
    uint32_t n_blocks;          /* occupied super-cells: cells holds n_blocks * 512 (first, last + 1) pairs */
    uint32_t ctop_len;          /* length of ctop */
    uint32_t leaf_max;          /* octree leaf size in force */
    int32_t surface_like;       /* the first-pass regime decided for this target (1: packets) */
    uint32_t level_hist[16];    /* [l], l = 1 .. 10: adjacent sorted pairs whose keys first differ at octree level l */
} symmicp_index_info;
/* the target index of a SYMMICP_CORR_TREE context after symmicp_set_target (SYMMICP_ERR_STATE without one) */
int symmicp_ctx_index_info(symmicp_ctx *ctx, symmicp_index_info *info);
/* copies of its arrays, each may be NULL: tq [n][4], tn [n][2][4], boxes [n_boxes][2][4], ctop [ctop_len], cells [n_blocks * 512][2],
 * onodes [n_onodes][2][4] (floats as the device holds them: integer words keep their bits) */
int symmicp_ctx_index_arrays(symmicp_ctx *ctx, float *tq, float *tn, float *boxes, uint32_t *ctop, uint32_t *cells, float *onodes);
/* this rank's source share after symmicp_set_source.  Sizes: *n_local points, *pkt_count packets (0: no table, the first pass takes 64
 * queries as they lie), *sorted != 0: the share is in Morton order, *cost_keyed != 0: the packets are started by their distance to the
 * target.  Arrays, each may be NULL: order [n_local] = the caller's row of every share position (SYMMICP_ERR_STATE when asked of an
 * unsorted share), pkt_tab [pkt_count][2] = (first query, count) in start order.  Any size pointer may be NULL. */
int symmicp_ctx_source_share(symmicp_ctx *ctx, size_t *n_local, size_t *pkt_count, int32_t *sorted, int32_t *cost_keyed, uint32_t *order,
                             uint32_t *pkt_tab);
/* the build's primitives on host arrays, run on the context's stream with its scratch arena.  Stable ascending sort of (keys, vals) by
 * the low key_bits bits (0 .. 32, keys < 2^key_bits; the voxel sort passes 0 for a single voxel: no pass runs), in place; exclusive prefix sum of data (mod 2^32), in place.  n == 0 is OK and
 * launches nothing; n < 2^31. */
int symmicp_ctx_radix_sort_probe(symmicp_ctx *ctx, uint32_t *keys, uint32_t *vals, size_t n, int key_bits);
int symmicp_ctx_scan_probe(symmicp_ctx *ctx, uint32_t *data, size_t n);
/* the trimmed pass's exact radix select on a host array: *kth_out = the k-th smallest key (1 <= k <= n, n < 2^31), *n_le_out = the
 * number of keys <= it.  Same stream and scratch arena; the context's trim fraction and trim state stay as they were. */
int symmicp_ctx_select_probe(symmicp_ctx *ctx, const uint32_t *keys, size_t n, uint64_t k, uint32_t *kth_out, uint64_t *n_le_out);
/* the one-to-one claim on host arrays: row i (the array index is the caller row) claims target row tgt_row[i] with the key
 * (d2_bits[i] << 32 | i); tgt_row[i] < 0 (or >= n_t): no pair.  winner_out[i] = 1 iff row i wins its target.  n, n_t < 2^31.  Same
 * stream and scratch arena; the context's clouds, pairs, options and states stay as they were. */
int symmicp_ctx_unique_probe(symmicp_ctx *ctx, const int32_t *tgt_row, const uint32_t *d2_bits, size_t n, size_t n_t, uint8_t *winner_out);

/* the reverse search of a reciprocal pass on host arrays: builds the index over db [n_db][3] exactly as the pass builds the source's,
 * relabels it with the given distinct labels (< 2^31; NULL: the row), carries the queries q_xyz [n_q][3] through
 * symmicp_inverse_rigid(X16) (NULL: identity) and returns back() and d2' for every query.  n_db, n_q in 1 .. 2^31 - 1.  Same stream and
 * scratch arena; the context's clouds, indexes, options and states stay as they were. */
int symmicp_ctx_reverse_nn_probe(symmicp_ctx *ctx, const float *db_xyz, const int32_t *labels, size_t n_db, const float *q_xyz, size_t n_q,
                                 const float *X16, int32_t *label_out, float *d2_out);

/* what reciprocal correspondences hold on this context (each pointer may be NULL): *index_valid != 0: the source index exists;
 * *index_bytes: the device bytes of its arena (0: never built; the arena is kept across symmicp_set_source calls and reused);
 * *index_builds: the builds of it by passes since symmicp_create -- one per symmicp_set_source followed by a reciprocal pass, none
 * otherwise (the probe above builds an index of its own and is not counted); *table_words: the 64-bit words allocated for the
 * one-to-one claim table (0: none; the target's size for one-to-one passes; more, by the reverse search's arguments, once a
 * reciprocal pass has run). */
int symmicp_ctx_reciprocal_info(const symmicp_ctx *ctx, int32_t *index_valid, uint64_t *index_bytes, uint64_t *index_builds, uint64_t *table_words);
/* ---- normals pre-step (replaces MyICP::estimateNormals, myicp.cpp:152-172: PCL NormalEstimation,
 * setKSearch(10), viewpoint (0,0,0)).  Exact k-NN (the point itself included) + PCA on the GPU.
 * xyz strided as in set_source; nrm_out packed AoS [n][3]; curv_out (lambda_min / trace) may be NULL;
 * viewpoint may be NULL (origin); 3 <= k <= 16. */
int symmicp_estimate_normals(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k,
                             const float viewpoint[3], float *nrm_out, float *curv_out);
/* the same on a context the caller already owns (stream, arenas and code objects are reused; the context's own clouds are
 * left alone): what MyICP::estimateNormals calls for both clouds before every alignment (myicp.cpp:105) */
int symmicp_ctx_estimate_normals(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k,
                                 const float viewpoint[3], float *nrm_out, float *curv_out);
/* the k nearest points of the same cloud, the set the normals use: rows_out / d2_out [n][k] (row-major, both required), for every
 * point its neighbours' rows and fp32 squared distances (dx*dx + dy*dy) + dz*dz in ascending (d2, row) order, the point itself
 * included.  Same argument rules as symmicp_ctx_estimate_normals; the context's own clouds are left alone. */
int symmicp_ctx_knn(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n, int k,
                    int32_t *rows_out, float *d2_out);

/* ---- intensity gradient on the tangent plane (the target attribute of SYMMICP_MODE_COLOR) --------------------------------------
 * grad_out [n][3] packed (required); xyz, nrm (both required) strided as in symmicp_set_source; intensity[i * stride]; 3 <= k <= 16
 * and k <= n.  For row i with normal n, every step in fp64 from the fp32 inputs, unfused, sums in the order written:
 *   1. neighbours j = the k-NN set of symmicp_ctx_knn without row i itself, in its ascending (d2, row) order
 *   2. x = x_j - x_i;  s = (x.x*n.x + x.y*n.y) + x.z*n.z;  e_j = x - s n
 *   3. M = sum_j e_j e_j^T (upper triangle)      4. r = sum_j e_j (I_j - I_i)      5. mu = ((M00 + M11) + M22) / 2
 *   6. A = M + mu n n^T, A_ab = M_ab + (mu * n_a) * n_b
 *   7. g = adj(A) r / det A by the symmetric 3x3 adjugate: c00 = A11*A22 - A12*A12, c01 = A02*A12 - A01*A22, c02 = A01*A12 - A02*A11,
 *      c11 = A00*A22 - A02*A02, c12 = A01*A02 - A00*A12, c22 = A00*A11 - A01*A01, det = (A00*c00 + A01*c01) + A02*c02,
 *      g_x = ((c00*r0 + c01*r1) + c02*r2) / det, g_y = ((c01*r0 + c11*r1) + c12*r2) / det, g_z = ((c02*r0 + c12*r1) + c22*r2) / det
 *   8. g = 0 unless det > 1e-12 * t*t*t with t = ((A00 + A11) + A22) / 3 (collinear or duplicate neighbourhoods; a zero normal
 *      on a flat neighbourhood)
 *   9. g rounded to fp32.
 * mu stands in for the normal direction: r is orthogonal to n and M n = 0, so g is tangent and does not depend on mu in exact
 * arithmetic, and A's condition number is the ratio of the two tangent moments.
 * SYMMICP_ERR_ARG: NULL xyz / nrm / intensity / grad_out; n == 0 or n > 2^31 - 1; k outside 3 .. 16 or above n; non-finite
 * coordinates.  The ctx form runs on the context's stream and arenas like symmicp_ctx_knn: the context's source, target, index,
 * attributes and certificates stay exactly as they were. */
int symmicp_ctx_intensity_gradient(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                                   const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride,
                                   const float *intensity, size_t intensity_stride, size_t n, int k, float *grad_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_intensity_gradient(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                               const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride,
                               const float *intensity, size_t intensity_stride, size_t n, int k, float *grad_out);

/* ---- fixed-radius neighbour search (PCL's radiusSearch), exact, on the GPU ------------------------------------------------
 * For a cloud of n points and a radius r (finite, > 0): r2 = r * r in fp32, d2(i, j) = (dx*dx + dy*dy) + dz*dz in fp32,
 * unfused (the distance of symmicp_ctx_knn).  The neighbourhood of row i is
 *     N(i) = { j != i : d2(i, j) <= r2 }     compared in fp32.  The point itself is left out by ROW: a duplicate of it, at
 *                                             d2 == 0, is a member.
 * count_out [n] = |N(i)| (required).  With rows_out != NULL also the lists, in CSR form: offsets_out [n + 1] (int64, required
 * then; written whenever it is given), rows_out [total] and d2_out [total] (d2_out may be NULL); list i is
 * rows_out[offsets_out[i] .. offsets_out[i + 1]).  *total_out = the sum of the counts (required).
 * SYMMICP_ERR_SIZE when rows_out is given and total > cap: *total_out, count_out and offsets_out are set, the lists are not
 * written -- call again with room for *total_out entries.  Lists of more than 2^32 - 1 entries in all are refused the same way
 * whatever the cap (the device's offsets are 32-bit words); the counts are still right.
 * Order inside a list: ascending position in the index's sorted (Morton) order -- deterministic for a given cloud, not otherwise
 * specified; callers that need (d2, row) order sort (the Python wrapper does, on the host).
 * SYMMICP_ERR_ARG: NULL xyz / count_out / total_out; rows_out without offsets_out; n == 0 or n > 2^31 - 1; a radius that is not
 * finite and > 0; non-finite coordinates (the index build refuses them, as it does for symmicp_ctx_knn).
 * xyz strided as in symmicp_set_source.  The ctx form runs on the context's stream and arenas like symmicp_ctx_knn: the
 * context's source, target, index and certificates stay exactly as they were. */
int symmicp_ctx_radius_search(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n, float radius,
                              int32_t *count_out, int64_t *offsets_out, int32_t *rows_out, float *d2_out, size_t cap,
                              size_t *total_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_radius_search(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, float radius,
                          int32_t *count_out, int64_t *offsets_out, int32_t *rows_out, float *d2_out, size_t cap, size_t *total_out);

/* ---- Fast Point Feature Histograms (Rusu, Blodow, Beetz 2009; PCL's FPFHEstimation, Open3D's compute_fpfh_feature) --------
 * fpfh_out [n][33] (required), spfh_out [n][33] and count_out [n] (= |N(i)|) may be NULL; xyz and nrm (both required) strided as
 * in symmicp_set_source.  Neighbourhoods are N(i) of the radius search above.  Every operation below is fp32, unfused and in
 * the association written; sqrtf and / are correctly rounded, atan2f is the device library's.
 *   dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z        cross(a, b) = (a.y*b.z - a.z*b.y, a.z*b.x - a.x*b.z, a.x*b.y - a.y*b.x)
 * Pair features of row i (point p, normal n) with j in N(i) (point q, normal m):
 *   d = q - p;  f4 = sqrtf(d2(i, j));  a1 = dot(n, d) / f4;  a2 = dot(m, d) / f4;
 *   if fabsf(a1) < fabsf(a2):  A = m, B = n, d = -d, f3 = -a2      (PCL: the frame sits on the point whose normal makes the
 *   else:                      A = n, B = m,         f3 = a1        smaller angle with the line between the two)
 *   v = cross(d, A);  vn = sqrtf(dot(v, v));  v = (v.x / vn, v.y / vn, v.z / vn);  w = cross(A, v);
 *   f2 = dot(v, B);  f1 = atan2f(dot(w, B), dot(A, B)).
 *   The pair is VALID iff f4 > 0, vn > 0 and f1, f2, f3 are all finite; an invalid pair adds nothing (zero or NaN normals and
 *   duplicate points are thereby well defined: their histograms are emptier, or all zero).
 * Bins, 11 per feature, each clamped to [0, 10] (PI = 3.14159274f, INV_2PI = 0.159154937f):
 *   b1 = floorf((11.0f * (f1 + PI)) * INV_2PI);  b2 = floorf((11.0f * (f2 + 1.0f)) * 0.5f);  b3 = floorf((11.0f * (f3 + 1.0f)) * 0.5f).
 *   Layout of the 33 floats: [0..10] f1, [11..21] f2, [22..32] f3 (PCL's order).
 * SPFH: c_i[b] = the number of valid pairs of i in bin b (an integer: the order of the walk does not matter; 32-bit counters,
 *   exact for every count a cloud of n <= 2^31 - 1 points can give), spfh_i[b] = (100.0f * (float)c_i[b]) / (float)k_i with
 *   k_i = |N(i)| (invalid pairs count in k_i); all zero when k_i == 0.
 * FPFH: s_i[b] = the sum over j in N(i) with d2(i, j) > 0, in the list order of the radius search (ascending sorted position),
 *   of spfh_j[b] * w_ij, w_ij = 1.0f / d2(i, j), starting from 0.0f; per 11-bin block t = the sum of the block's s_i[b] in
 *   ascending b starting from 0.0f, and fpfh_i[b] = s_i[b] * (100.0f / t) if t > 0 and t is finite, else 0 for the whole block
 *   (near-duplicate points give weights that overflow fp32; the rule keeps NaN and Inf out of the output).  As in PCL the
 *   point's own SPFH enters only through its neighbours; each block sums to 100 (within rounding) or is exactly 0.
 * Cost grows with the neighbour count (there is no max_nn cap): two walks of the tree, |N(i)| pair features per point.
 * SYMMICP_ERR_ARG: NULL xyz / nrm / fpfh_out; n == 0 or n > 2^31 - 1; a radius that is not finite and > 0; non-finite
 * coordinates.  The ctx form leaves the context's source, target, index and certificates exactly as they were.  A sharded job
 * computes the features of the FULL cloud on every rank (the output is deterministic). */
int symmicp_ctx_fpfh(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                     const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride, size_t n, float radius,
                     float *fpfh_out, float *spfh_out, int32_t *count_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_fpfh(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                 const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride, size_t n, float radius,
                 float *fpfh_out, float *spfh_out, int32_t *count_out);

/* ---- Intrinsic Shape Signatures keypoints (Zhong 2009; PCL's ISSKeypoint3D, Open3D's compute_iss_keypoints) ----------------
 * The salient points of a cloud of n points: those whose neighbourhood spreads in all three directions, and that are the
 * most salient of their surroundings.  Global registration describes and matches these few instead of every point.  Defined by
 * its arithmetic; the result is a function of the inputs alone, bit for bit.
 * Neighbourhoods.  N_r(i) is N(i) of the radius search above at radius r: r2 = r * r in fp32, d2 the fp32
 *   (dx*dx + dy*dy) + dz*dz, members d2 <= r2; row i itself is left out by ROW (a duplicate of it is a member); list order =
 *   ascending position in the index's sorted order.  rs = cfg->salient_radius, rn = cfg->non_max_radius.
 * Saliency.  k = |N_rs(i)| (neighbors_out[i]).  If k < min_neighbors: s_i = 0.  Else, for j in N_rs(i) in list order,
 *   e = x_j - x_i per component in fp32; the six upper entries of S accumulate (double)e_a * (double)e_b in fp64, starting from
 *   0.0 (the products are exact, the sums run in list order); C = S / (double)k per entry.
 *   l1 >= l2 >= l3 = the eigenvalues of C in fp64 by cyclic Jacobi rotations (sweeps over the pairs (0,1), (0,2), (1,2), at most
 *   12, until the squared off-diagonal sum is below 1e-300; rotation angle from theta = (a_qq - a_pp) / (2 a_pq),
 *   t = sign(theta) / (|theta| + sqrt(theta^2 + 1)); eigenvalues only), for which |l - exact| <= 1e-13 * l1 holds.
 *   The point is SALIENT iff  l2 < (double)gamma21 * l1  and  l3 < (double)gamma32 * l2  and  (float)l3 > 0
 *   (products, not quotients: no division by zero; an exactly planar or collinear neighbourhood is never salient).
 *   s_i = (float)l3 if salient, else 0 (saliency_out[i]).  The paper's per-neighbour weights are not applied (as in Open3D).
 * Non-maximum suppression.  Row i is a keypoint iff  s_i > 0,  |N_rn(i)| >= min_neighbors,  and no j in N_rn(i) has
 *   s_j > s_i, or s_j == s_i with row j < row i.  A pure function of the fp32 array s and the exact neighbourhoods.
 *   Ties go to the LOWEST ROW: a deliberate departure from Open3D, which keeps both points of an exact tie (and so returns two
 *   keypoints one spacing apart on symmetric data).
 * Output.  rows_out [cap]: the keypoint rows in ascending order; *count_out their number (required).  SYMMICP_ERR_SIZE when the
 *   count exceeds cap: *count_out, saliency_out and neighbors_out are written, the rows are not -- call again with room
 *   (rows_out may be NULL with cap == 0 to ask for the count).  saliency_out [n] and neighbors_out [n] may be NULL.
 * Cost grows with the neighbour counts (there is no max_nn cap): one walk of the tree per radius; the second walk is skipped
 *   for points with s_i == 0.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed: NULL xyz / cfg / count_out; NULL rows_out with cap > 0;
 *   n == 0 or n > 2^31 - 1; cfg->struct_size != sizeof(symmicp_iss_config); a radius that is not finite and > 0; a gamma outside
 *   (0, 1] or NaN; min_neighbors < 1; non-finite coordinates.
 * xyz strided as in symmicp_set_source.  The ctx form runs on the context's stream and temporary arena: the context's clouds,
 * index, attributes, certificates and states stay exactly as they were.  A sharded job computes the keypoints of the FULL
 * cloud on every rank (the output is deterministic). */
typedef struct {
    uint32_t struct_size;     /* = sizeof(symmicp_iss_config), checked */
    float salient_radius;     /* finite, > 0 (the caller sets it; default 0) */
    float non_max_radius;     /* finite, > 0 (default 0) */
    float gamma21, gamma32;   /* each finite, in (0, 1]; default 0.975f */
    int32_t min_neighbors;    /* >= 1; default 5 */
    int32_t reserved;
} symmicp_iss_config;
void symmicp_iss_config_default(symmicp_iss_config *cfg);
int symmicp_ctx_iss_keypoints(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                              const symmicp_iss_config *cfg, int32_t *rows_out, size_t cap, size_t *count_out,
                              float *saliency_out, int32_t *neighbors_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_iss_keypoints(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                          const symmicp_iss_config *cfg, int32_t *rows_out, size_t cap, size_t *count_out,
                          float *saliency_out, int32_t *neighbors_out);

/* ---- statistical and radius outlier removal (PCL's StatisticalOutlierRemoval / RadiusOutlierRemoval, Open3D's
 * remove_statistical_outlier / remove_radius_outlier; DESIGN.md 4, "Outlier removal") ------------------------------------------
 * The rows of a cloud of n points that are NOT stray: the filter a pipeline runs between loading a scan and downsampling,
 * normals, keypoints and features.  Each filter is defined by its arithmetic; the result is a function of the inputs alone, bit
 * for bit.
 * Common.  xyz strided as in symmicp_set_source.  d2(i, j) is the fp32 (dx*dx + dy*dy) + dz*dz, unfused: the distance of
 *   symmicp_ctx_knn and of the radius search.  A point is never its own neighbour: it is left out by ROW, so a duplicate of it
 *   (d2 == 0) is a neighbour.
 * Statistical outlier removal.  1 <= k <= 64, k <= n - 1, std_mul finite.
 *   D_i = the multiset of the k smallest d2(i, j) over j != i (ties at the k-th value do not matter: only the values enter).
 *   m_i = ( sum of sqrt((double)d2) over D_i in ascending d2, starting from 0.0 ) / (double)k, in fp64 (mean_dist_out[i]).
 *   The statistics are PCL's formula, on the host, sequentially in ascending row order, unfused:
 *     S1 = sum m_i;  S2 = sum m_i * m_i;  mu = S1 / n;  var = (S2 - S1 * S1 / n) / (n - 1);  sd = sqrt(max(var, 0));
 *     thr = mu + (double)std_mul * sd.                                                  stats_out[3] = {mu, sd, thr}.
 *   Row i is KEPT iff m_i <= thr.  A NaN threshold keeps nothing; it can arise only when an fp32 d2 overflows (an infinite
 *   m_i makes var NaN, and max(var, 0) here passes a NaN on).
 * Radius outlier removal.  radius finite and > 0, min_neighbors >= 1.
 *   Row i is KEPT iff |N(i)| >= min_neighbors, N(i) exactly the neighbourhood of symmicp_ctx_radius_search: r2 = r * r in
 *   fp32, members d2 <= r2, the point itself excluded.  neighbors_out[i] = |N(i)|.
 *   PCL's RadiusOutlierRemoval and Open3D's remove_radius_outlier count the point itself among its neighbours (their radius
 *   search returns it).  PCL keeps a point with at least min_pts of them: min_neighbors = min_pts - 1 here.  Open3D keeps a
 *   point with MORE than nb_points of them: min_neighbors = nb_points here.
 * Output.  rows_out [cap]: the kept rows in ascending order; *count_out their number (required).  SYMMICP_ERR_SIZE when the
 *   count exceeds cap: *count_out and the per-point arrays (and stats_out) are written, the rows are not -- call again with room
 *   (rows_out may be NULL with cap == 0 to ask for the count).  mean_dist_out [n], stats_out [3], neighbors_out [n] may be NULL.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed: NULL xyz / count_out; NULL rows_out with cap > 0;
 *   n == 0 or n > 2^31 - 1; k outside 1 .. 64 or above n - 1; std_mul not finite; a radius that is not finite and > 0;
 *   min_neighbors < 1; non-finite coordinates.
 * The ctx forms run on the context's stream and arenas: the context's clouds, index, attributes, certificates and states stay
 * exactly as they were.  A sharded job filters the FULL cloud on every rank (the output is deterministic). */
int symmicp_ctx_statistical_outlier_removal(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                                            int k, float std_mul, int32_t *rows_out, size_t cap, size_t *count_out,
                                            double *mean_dist_out, double stats_out[3]);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_statistical_outlier_removal(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                                        int k, float std_mul, int32_t *rows_out, size_t cap, size_t *count_out,
                                        double *mean_dist_out, double stats_out[3]);
int symmicp_ctx_radius_outlier_removal(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                                       float radius, int min_neighbors, int32_t *rows_out, size_t cap, size_t *count_out,
                                       int32_t *neighbors_out);
int symmicp_radius_outlier_removal(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                                   float radius, int min_neighbors, int32_t *rows_out, size_t cap, size_t *count_out,
                                   int32_t *neighbors_out);

/* ---- DBSCAN and Euclidean cluster extraction (Ester et al. 1996; PCL's EuclideanClusterExtraction, Open3D's cluster_dbscan,
 * scikit-learn's DBSCAN; DESIGN.md 4, "Clustering") -------------------------------------------------------------------------
 * Splits a cloud of n points into its connected parts: the objects that symmicp_batch_align aligns pair by pair, and the small
 * floating blobs that the per-point outlier filters above cannot see.  Defined by its arithmetic; the result is a function of
 * the inputs alone, bit for bit (it does not depend on the order in which the device meets the edges).
 * Neighbourhoods.  N(i) is exactly the neighbourhood of symmicp_ctx_radius_search at radius eps: r2 = eps * eps in fp32, d2 the
 *   fp32 (dx*dx + dy*dy) + dz*dz, unfused, members d2 <= r2; row i itself is left out by ROW (a duplicate of it is a member).
 *   d2(i, j) == d2(j, i) exactly, so the graph i -- j iff j in N(i) is symmetric.  neighbors_out[i] = |N(i)|.
 * Core points.  Row i is CORE iff |N(i)| + 1 >= min_points (core_out[i] = 1): min_points counts the point itself, as Open3D and
 *   scikit-learn do.  min_points = 1 makes every point core: PCL's Euclidean clustering at tolerance eps.
 * Clusters.  A cluster is a connected component of that graph restricted to the core rows; its REPRESENTATIVE is its lowest core
 *   row.
 * Border points.  A non-core row with at least one core neighbour joins ONE cluster: among its core neighbours j the one with
 *   the smallest d2 (compared as fp32 bits), an exact tie going to the cluster whose representative row is lowest -- the minimum
 *   of the 64-bit key (d2 bits << 32) | representative(j).  A deliberate departure from PCL, Open3D and scikit-learn, where a
 *   border point goes to whichever cluster their scan order reaches first (a function of the row order, and for parallel
 *   implementations of the schedule).
 * Noise.  Every other row: label -1.
 * Labels.  The clusters are numbered 0 .. C - 1 in ascending order of their representative row.  On every core row and every noise
 *   row this is scikit-learn's DBSCAN(eps, min_samples = min_points).labels_; only border rows can differ.
 * Size filter.  A cluster's size is its core rows plus its border rows.  With min_cluster_size > 0 or max_cluster_size > 0 a
 *   cluster whose size lies outside [min, max] (0 = no bound on that side) becomes noise (-1), and the remaining clusters are
 *   renumbered in the same order.  core_out and neighbors_out describe the points BEFORE the size filter.
 * Output.  labels_out [n] and *clusters_out (the number of clusters after the filter) are required.  sizes_out [cap]: the sizes
 *   of clusters 0 .. C - 1.  SYMMICP_ERR_SIZE when C exceeds cap: the labels, the count and the per-point arrays are written,
 *   the sizes are not -- call again with room (sizes_out may be NULL with cap == 0).  core_out [n] and neighbors_out [n] may be
 *   NULL.
 * Cost grows with the neighbour counts (there is no max_nn cap): three walks of the tree for min_points > 1 (count, union,
 *   border), two for min_points == 1.  The radius graph is never stored.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed: NULL xyz / cfg / labels_out / clusters_out; NULL sizes_out
 *   with cap > 0; n == 0 or n > 2^31 - 1; cfg->struct_size != sizeof(symmicp_cluster_config); eps not finite or not > 0;
 *   min_points < 1; a negative size bound, or max_cluster_size < min_cluster_size with both > 0; non-finite coordinates.
 * xyz strided as in symmicp_set_source.  The ctx form runs on the context's stream and arenas: the context's clouds, index,
 * attributes, certificates and states stay exactly as they were.  A sharded job computes the full result on every rank (the
 * output is deterministic). */
typedef struct {
    uint32_t struct_size;       /* = sizeof(symmicp_cluster_config), checked */
    float    eps;               /* finite, > 0 (the caller sets it; default 0) */
    int32_t  min_points;        /* >= 1, counts the point itself; default 1 */
    int32_t  min_cluster_size;  /* >= 0, 0 = none */
    int32_t  max_cluster_size;  /* >= 0, 0 = none; if both > 0, max >= min */
    int32_t  reserved;
} symmicp_cluster_config;
void symmicp_cluster_config_default(symmicp_cluster_config *cfg);
int symmicp_ctx_cluster(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                        const symmicp_cluster_config *cfg, int32_t *labels_out, size_t *clusters_out, int32_t *sizes_out,
                        size_t cap, uint8_t *core_out, int32_t *neighbors_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_cluster(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                    const symmicp_cluster_config *cfg, int32_t *labels_out, size_t *clusters_out, int32_t *sizes_out,
                    size_t cap, uint8_t *core_out, int32_t *neighbors_out);

/* ---- region-growing segmentation (Rabbani et al. 2006; PCL's RegionGrowing; DESIGN.md 4, "Region growing") -------------------
 * Splits a cloud where its surface BENDS, not where it has a gap: a box on a table, or the three faces at a box corner, are one
 * Euclidean cluster and several regions.  The labels go where the clustering's go (symmicp_batch_align pair by pair, for example
 * the faces of an object).  Defined by its arithmetic; the result is a function of the inputs alone, bit for bit (it does not
 * depend on the order in which the device meets the edges, nor on the row order beyond the numbering).
 * Inputs: xyz [n]; nrm [n], required, of any sign, used as given (no normalisation: smoothness_cos is a bound on the dot product
 *   itself); curv [n] or NULL, element i at curv[i * curv_stride] (symmicp_ctx_estimate_normals' curv_out with stride 1).
 * Neighbourhoods.  N(i) is exactly the neighbourhood of symmicp_ctx_radius_search at radius eps: r2 = eps * eps in fp32, d2 the
 *   fp32 (dx*dx + dy*dy) + dz*dz, unfused, members d2 <= r2; row i itself is left out by ROW (a duplicate of it is a member).
 * Smooth edges.  smooth(i, j) iff j in N(i) and fabsf((nix*njx + niy*njy) + niz*njz) >= smoothness_cos, the dot product in fp32,
 *   unfused, in that association (a NaN from an overflow compares false).  Both halves are symmetric bit for bit, so the graph is
 *   undirected; inverting the sign of any normal changes nothing.  smooth_out[i] = |{ j : smooth(i, j) }|, over all rows.
 * Seeds.  Row i is a SEED iff curv == NULL or curv[i] <= curvature_threshold, compared in fp32 (seed_out[i] = 1).
 * Regions.  A region is a connected component of the smooth graph restricted to the seed rows; its REPRESENTATIVE is its lowest
 *   seed row.  A seed without a smooth seed neighbour is a region of one.
 * Border rows.  A non-seed row i joins ONE region: among the seed rows j with smooth(i, j) the one that minimises the 64-bit key
 *   (d2 bits << 32) | representative(j) -- the clustering's border rule with the smoothness test added.
 * Unlabelled rows.  Every other row: label -1.
 * Labels.  The regions are numbered 0 .. R - 1 in ascending order of their representative row.
 * Size filter, output, cap.  Exactly symmicp_ctx_cluster's: a region's size is its seed rows plus its border rows; a region whose
 *   size lies outside [min_region_size, max_region_size] (0 = no bound on that side) becomes -1 and the rest are renumbered in the
 *   same order.  labels_out [n] and *regions_out are required; sizes_out [cap]; SYMMICP_ERR_SIZE when R exceeds cap: the labels,
 *   the count and the per-point arrays are written, the sizes are not (sizes_out may be NULL with cap == 0).  seed_out [n] and
 *   smooth_out [n] may be NULL and describe the points BEFORE the size filter; smooth_out costs one more walk of the tree, which
 *   runs only when it is given.
 * Identity.  With smoothness_cos = 0 and curv == NULL the result is symmicp_ctx_cluster's at min_points = 1, label for label.
 * Departures from PCL's RegionGrowing, all deliberate: PCL takes k-nearest neighbourhoods, which are not symmetric; it grows in
 *   curvature order, so a point that two regions could claim goes to whichever reaches it first (a function of the scan order);
 *   and it opens a region from any leftover point, so nothing stays unlabelled.  Here the neighbourhood is the symmetric radius
 *   graph, a contested row goes by the key above, and a high-curvature row that no seed reaches smoothly stays -1.  PCL's residual
 *   test, a k-NN neighbourhood mode and colour-based growing are not provided.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed, the outputs untouched: NULL xyz / nrm / cfg / labels_out /
 *   regions_out; NULL sizes_out with cap > 0; n == 0 or n > 2^31 - 1; cfg->struct_size != sizeof(symmicp_region_config); eps not
 *   finite or not > 0; smoothness_cos not finite or outside [0, 1]; a NaN curvature_threshold (+-inf are allowed); a negative size
 *   bound, or max_region_size < min_region_size with both > 0; non-finite coordinates or normal components; a NaN in curv.
 * xyz and nrm strided as in symmicp_set_source.  The ctx form runs on the context's stream and arenas: the context's clouds, index,
 * attributes, certificates and states stay exactly as they were.  A sharded job computes the full result on every rank. */
typedef struct {
    uint32_t struct_size;          /* = sizeof(symmicp_region_config), checked */
    float    eps;                  /* neighbourhood radius, finite, > 0 (the caller sets it; default 0) */
    float    smoothness_cos;       /* in [0, 1]; default 0.8660254f (30 degrees, PCL's default) */
    float    curvature_threshold;  /* not NaN, +inf allowed; default 0.05f (PCL's default) */
    int32_t  min_region_size;      /* >= 0, 0 = none */
    int32_t  max_region_size;      /* >= 0, 0 = none; if both > 0, max >= min */
} symmicp_region_config;
void symmicp_region_config_default(symmicp_region_config *cfg);
int symmicp_ctx_region_growing(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                               size_t nrm_row_stride, size_t nrm_col_stride, const float *curv, size_t curv_stride, size_t n,
                               const symmicp_region_config *cfg, int32_t *labels_out, size_t *regions_out, int32_t *sizes_out,
                               size_t cap, uint8_t *seed_out, int32_t *smooth_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_region_growing(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                           size_t nrm_row_stride, size_t nrm_col_stride, const float *curv, size_t curv_stride, size_t n,
                           const symmicp_region_config *cfg, int32_t *labels_out, size_t *regions_out, int32_t *sizes_out,
                           size_t cap, uint8_t *seed_out, int32_t *smooth_out);

/* ---- consistent normal orientation (Hoppe et al. 1992; Open3D's orient_normals_consistent_tangent_plane; DESIGN.md 4, "Normal
 * orientation") ---------------------------------------------------------------------------------------------------------------
 * Gives the normals of a cloud one common side per connected part: a flip towards a viewpoint is right only where the viewpoint
 * sees the surface, so on a full model or a merged scan it is wrong for a good part of the rows, and two clouds of one surface
 * then disagree there.  One orientation is propagated along the minimum spanning forest of the neighbour graph, edges weighted by
 * how parallel the two normals are.  Defined by its arithmetic: fp32, unfused, in the association written; the result is a function
 * of the inputs alone, bit for bit (the forest is unique, so it does not depend on the order in which the device finds it).
 * Inputs: xyz [n], nrm [n] (unoriented; zero normals are allowed), cfg = {k, seed_rule, ref[3]}.
 *   1. Graph.  S(i) = the k-NN set of symmicp_ctx_knn without row i itself, left out by ROW as symmicp_ctx_intensity_gradient does (a
 *      duplicate of the point is a member; among more than k exact duplicates a row may be missing from its own set, and S(i) then has
 *      k members).  E = { {i, j} : j in S(i) or i in S(j) }: the symmetrised k-NN graph.  It is never stored symmetrised.
 *   2. Weight.  d(i,j) = (nx_i*nx_j + ny_i*ny_j) + nz_i*nz_j;  w = fmaxf(1.0f - fabsf(d), 0.0f);  s(i,j) = d < 0: "these two normals
 *      disagree".  d(i,j) == d(j,i) exactly.
 *   3. Order.  Edges are ordered by the triple (bits of w as uint32, lo = min(i,j), hi = max(i,j)): strict and total, so the minimum
 *      spanning forest F of (E, order) is unique.
 *   4. Components.  The connected components of E = the trees of F.  component_out[i] = the lowest row of i's component.
 *   5. Seed, one per component.
 *      SYMMICP_ORIENT_VIEWPOINT (the default, ref = the origin): the row with the smallest d2 = (dx*dx + dy*dy) + dz*dz, dx = x - ref.x
 *        and so on, compared as fp32 bits, ties to the lowest row.  It is flipped iff the flip test of the normals pre-step
 *        (symmicp_ctx_estimate_normals) flips it: in fp64 from the fp32 values,
 *        ((ref.x - x)*nx + (ref.y - y)*ny) + (ref.z - z)*nz < 0.
 *      SYMMICP_ORIENT_DIRECTION (Open3D's rule with ref = +z): the row with the largest p = ((x*ref.x + y*ref.y) + z*ref.z) + 0.0f (a
 *        NaN p, an overflow of both signs, counts as -inf), ties to the lowest row.  Flipped iff (nx*ref.x + ny*ref.y) + nz*ref.z < 0.
 *      The closest point to a viewpoint, or the extreme point along a direction, is where the surface's normal is parallel to the line
 *      of sight: the sign test is at its most reliable there.
 *   6. Propagation.  flip(i) = flip(seed) XOR (the number of edges with s = 1 on the tree path from i to its component's seed is odd).
 *   7. Output.  nrm_out [n][3] packed (required): nrm[i] with the sign bits of its three components inverted when flip(i); the bits
 *      are otherwise untouched.  Optional, each may be NULL: flip_out [n] (0 / 1); component_out [n]; tree_out [n - 1][2]: the edges
 *      (lo, hi) of F in an unspecified order, *tree_count their number = n - components (tree_count is required with tree_out and is
 *      always set when given); result (below).
 * nrm_out does not depend on the signs of the input normals: w uses |d|, and negating one normal inverts s on every edge at that row,
 * which inverts its own flip and nobody else's (the exception is an exact zero: a d, or a seed's test value, that is exactly 0 reads
 * as "agree" / "keep" under either sign).  So the stage is idempotent, and a normals pre-step with any viewpoint may precede it.
 * What remains the caller's part: every component is seeded on its own (result->components says how many there are; default k = 16:
 * the cat of tests/golden is one component at k = 16 and four at k = 10), and a viewpoint inside a closed object orients it inwards.
 * Method: Boruvka rounds over the lists of symmicp_ctx_knn with the sign carried as a parity (csrc/orient_core.h); rounds <=
 * ceil(log2 n).  SYMMICP_ERR_INTERNAL if a bound of that reasoning fails (more than 32 rounds; a walk longer than the round's hooks).
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed: NULL xyz / nrm / cfg / nrm_out; tree_out without tree_count;
 *   n == 0 or n > 2^31 - 1; cfg->struct_size != sizeof(symmicp_orient_config); k outside 3 .. 16 or above n; a seed_rule that is
 *   neither of the two; a non-finite ref, or a zero ref with SYMMICP_ORIENT_DIRECTION; non-finite coordinates; non-finite normals.
 * xyz and nrm strided as in symmicp_set_source.  The ctx form runs on the context's stream and arenas like symmicp_ctx_knn: the
 * context's source, target, index, attributes and certificates stay exactly as they were. */
typedef enum { SYMMICP_ORIENT_VIEWPOINT = 0, SYMMICP_ORIENT_DIRECTION = 1 } symmicp_orient_seed;
typedef struct {
    uint32_t struct_size;       /* = sizeof(symmicp_orient_config), checked */
    int32_t  k;                 /* 3 .. 16, <= n; default 16 (the cat of tests/golden: one component at 16, four at 10) */
    int32_t  seed_rule;         /* symmicp_orient_seed; default SYMMICP_ORIENT_VIEWPOINT */
    float    ref[3];            /* the viewpoint, or the direction; default 0 0 0 */
} symmicp_orient_config;
typedef struct {
    uint64_t graph_edges;       /* |E| */
    uint64_t tree_edges;        /* |F| = n - components */
    uint64_t components;
    uint64_t largest_component; /* rows of the largest component */
    uint64_t flipped;           /* rows with flip(i) = 1 */
    int32_t  rounds;            /* Boruvka rounds that joined something */
    int32_t  reserved;
} symmicp_orient_result;
void symmicp_orient_config_default(symmicp_orient_config *cfg);
int symmicp_ctx_orient_normals(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                               size_t nrm_row_stride, size_t nrm_col_stride, size_t n, const symmicp_orient_config *cfg, float *nrm_out,
                               uint8_t *flip_out, int32_t *component_out, int32_t *tree_out, size_t *tree_count,
                               symmicp_orient_result *result);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_orient_normals(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride, const float *nrm,
                           size_t nrm_row_stride, size_t nrm_col_stride, size_t n, const symmicp_orient_config *cfg, float *nrm_out,
                           uint8_t *flip_out, int32_t *component_out, int32_t *tree_out, size_t *tree_count, symmicp_orient_result *result);

/* ---- RANSAC plane segmentation (PCL's SACSegmentation with SACMODEL_PLANE / SACMODEL_PERPENDICULAR_PLANE, Open3D's
 * segment_plane; DESIGN.md 4, "Plane segmentation") ---------------------------------------------------------------------------
 * The plane with the most points of a cloud within max_dist: the floor or the table that joins every object standing on it into one
 * connected part, found and removed before the clustering above.  Defined by its arithmetic; the result is a function of the inputs
 * alone, bit for bit on the device part.
 *   Pivot.  c = the fp64 mean of the n points, summed in ascending row order, rounded to fp32; the device works on
 *     p_i = xyz_i - c (fp32).
 *   Samples.  Hypothesis h (0 <= h < hypotheses) draws the rows c_k = ((u(3h + k) >> 32) * n) >> 32, k = 0, 1, 2, where u is the
 *     SplitMix64 sequence of (seed, stream 2): symmicp_ctx_ransac's (stream 0; symmicp_ctx_fgr has stream 1) with
 *       base = mix64(seed * 0x9E3779B97F4A7C15 + 2 * 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D).
 *     No rejection loop; every hypothesis gets a status, the checks in this order, with a, b, c = the sample's p, u = b - a,
 *     v = c - a, w = u x v (fp32, unfused; dot(x, y) = (x0 y0 + x1 y1) + x2 y2):
 *       1 REPEATED    two draws are equal
 *       2 DEGENERATE  |w|^2 < 1e-4 |u|^2 |v|^2, or that product not > 0 (the sine bound of symmicp_ctx_ransac)
 *       3 OFF_AXIS    only with an axis (below): |dot(n, a^)| < cos_min
 *       0 EVALUATED
 *   Hypothesis.  n = w / sqrt(|w|^2),  d = -dot(n, a).
 *   Score.  inliers(h) = the number of rows i with fabsf(dot(n, p_i) + d) <= max_dist (fp32).  The winner is the evaluated
 *     hypothesis with the most inliers, ties to the lowest h.  None evaluated, or a winner with fewer than max(3, min_inliers)
 *     inliers: SYMMICP_ERR_NO_CONSENSUS, plane = 0, *count_out = 0 (result keeps best_hypothesis, evaluated and inliers_ransac;
 *     rows_out and distance_out are not written).
 *   Axis constraint (PCL's perpendicular-plane model: planes whose normal lies within max_angle_deg of an axis).  axis all zero:
 *     off.  Otherwise a^ = axis normalised in fp64 (length = sqrt((x x + y y) + z z)) and rounded to fp32, and
 *     cos_min = (float)cos(max_angle_deg * pi / 180) in fp64, 0 < max_angle_deg <= 90.
 *   Refit.  `refits` times (0 .. 8), on the host in fp64 over the current inlier set (at first the winner's fp32 set) in ascending
 *     row order, on x_i = xyz_i - (double)c, unfused: the mean m (sequential sums divided by the count k), the scatter matrix
 *     sum (x - m)(x - m)^T (sequential), its eigenvectors by the cyclic Jacobi of the normals pre-step (at most 12 sweeps), n = the
 *     eigenvector of the smallest eigenvalue (the lowest index among equal ones) divided by sqrt((n0 n0 + n1 n1) + n2 n2),
 *     d = -dot(n, m); then the inlier set is recomputed in fp64: |dot(n, x_i) + d| <= (double)max_dist.  Fewer than
 *     max(3, min_inliers) rows left: SYMMICP_ERR_NO_CONSENSUS as above.
 *   Result.  Oriented so that dot(n, a^) >= 0 with an axis; otherwise the component of n with the largest magnitude (the lowest
 *     axis among equal ones) is positive.  result->plane = (n, d - dot(n, (double)c)): the plane n . xyz + d = 0 in the caller's
 *     coordinates, composed in fp64; plane4_out is its rounding to fp32.  With refits == 0 it is the winner's fp32 (n, d) widened.
 *     distance_out[i] = dot(n, x_i) + d about the pivot, fp64, signed; rmse_final = sqrt of the mean of its square over the final
 *     inlier set (sequential).
 * Output.  plane4_out, result and *count_out are required.  rows_out [cap]: the final inlier rows in ascending order, *count_out
 *   their number.  SYMMICP_ERR_SIZE when the count exceeds cap: everything but the rows is written -- call again with room (rows_out
 *   may be NULL with cap == 0 to ask for the count).  distance_out [n], status_out [hypotheses] (uint8) and inliers_out
 *   [hypotheses] (int32, 0 unless evaluated) may be NULL.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed: NULL xyz / cfg / plane4_out / result / count_out; NULL
 *   rows_out with cap > 0; n < 3 or n > 2^31 - 1; cfg->struct_size != sizeof(symmicp_plane_config); hypotheses outside 1 .. 2^24;
 *   max_dist not finite and > 0; min_inliers < 0 or > n; refits outside 0 .. 8; a non-finite axis, or with an axis given a
 *   max_angle_deg outside (0, 90]; non-finite coordinates.
 * xyz strided as in symmicp_set_source.  The ctx form runs on the context's stream and arenas: the context's clouds, index,
 * attributes, certificates and states stay exactly as they were.  A sharded job computes the full result on every rank (the
 * output is deterministic). */
typedef struct {
    uint32_t struct_size;      /* = sizeof(symmicp_plane_config), checked */
    uint32_t hypotheses;       /* H, 1 .. 2^24; default 1 000 */
    uint64_t seed;
    float    max_dist;         /* finite, > 0 (the caller sets it; default 0) */
    int32_t  min_inliers;      /* 0 .. n; fewer than max(3, min_inliers) is no consensus; default 3 */
    int32_t  refits;           /* 0 .. 8, default 1 */
    float    axis[3];          /* all zero: no constraint */
    float    max_angle_deg;    /* (0, 90] with an axis */
    int32_t  reserved;
} symmicp_plane_config;
typedef struct {
    int32_t best_hypothesis;   /* -1: none */
    int32_t evaluated;         /* hypotheses with status EVALUATED */
    int32_t inliers_ransac;    /* the winner's inliers (fp32, on the device) */
    int32_t inliers_final;     /* after the refits */
    double  rmse_final;        /* over the final inliers */
    double  plane[4];          /* n, d in the caller's coordinates */
} symmicp_plane_result;
#define SYMMICP_PLANE_EVALUATED 0
#define SYMMICP_PLANE_REPEATED 1
#define SYMMICP_PLANE_DEGENERATE 2
#define SYMMICP_PLANE_OFF_AXIS 3
void symmicp_plane_config_default(symmicp_plane_config *cfg);
int symmicp_ctx_segment_plane(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                              const symmicp_plane_config *cfg, float plane4_out[4], symmicp_plane_result *result,
                              int32_t *rows_out, size_t cap, size_t *count_out, double *distance_out, uint8_t *status_out,
                              int32_t *inliers_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_segment_plane(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                          const symmicp_plane_config *cfg, float plane4_out[4], symmicp_plane_result *result,
                          int32_t *rows_out, size_t cap, size_t *count_out, double *distance_out, uint8_t *status_out,
                          int32_t *inliers_out);
/* test entry: the 4 floats (n, d about the pivot) the device computed for every hypothesis: hyp_out [hypotheses][4], written for
 * status EVALUATED and OFF_AXIS, zero otherwise; status_out [hypotheses] and pivot_out [3] = c may be NULL.  Arguments as above. */
int symmicp_ctx_plane_hypotheses(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n,
                                 const symmicp_plane_config *cfg, float *hyp_out, uint8_t *status_out, float pivot_out[3]);

/* ---- feature matching and RANSAC: global registration from FPFH features ("Feature matching and RANSAC") -------
 * All three run on the context's stream and temporary arena; the context's source, target, index and certificates stay exactly
 * as they were.  A sharded job computes the full result on every rank (the outputs are deterministic).
 *
 * FPFH matching relies on normals that are oriented alike in both clouds: two scans of one surface whose normals point to
 * different sides of it give unrelated histograms.  Estimated normals are flipped towards a viewpoint, which is right only where
 * the viewpoint sees the surface; symmicp_ctx_orient_normals then makes them consistent within every connected part of a cloud.
 * What remains the caller's part is a cloud in separate parts, each seeded on its own, and a viewpoint inside the object.
 *
 * symmicp_ctx_feature_nn: exact nearest neighbour in feature space.  fa [na][33] (queries) and fb [nb][33] (candidates), packed
 * fp32 as symmicp_ctx_fpfh writes them.  Defined by its arithmetic (fp32, unfused):
 *     D(i, j):    acc = 0.0f;  for b = 0 .. 32 ascending:  t = fa[i][b] - fb[j][b];  acc = acc + t * t
 *     nn(i)     = the j that minimises (D(i, j), j) lexicographically      (ties go to the lowest candidate row)
 *     second(i) = min over j != nn(i) of D(i, j); +INF when nb == 1
 * nn_out [na] (required), d2_out [na] = D(i, nn(i)) and d2_second_out [na] = second(i) (each may be NULL).  The result is a
 * function of the inputs alone.
 * SYMMICP_ERR_ARG: NULL fa / fb / nn_out; na or nb == 0 or > 2^31 - 1; a non-finite value in fa or fb. */
int symmicp_ctx_feature_nn(symmicp_ctx *ctx, const float *fa, size_t na, const float *fb, size_t nb,
                           int32_t *nn_out, float *d2_out, float *d2_second_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_feature_nn(int device, const float *fa, size_t na, const float *fb, size_t nb,
                       int32_t *nn_out, float *d2_out, float *d2_second_out);
/* The matches RANSAC consumes, defined by feature_nn: with nn_ab, d2, second = feature_nn(fa -> fb) and, if mutual != 0,
 * nn_ba = feature_nn(fb -> fa), pair (i, nn_ab(i)) is kept iff
 *     (mutual == 0 or nn_ba(nn_ab(i)) == i)  and  (max_ratio <= 0 or d2(i) <= (max_ratio * max_ratio) * second(i), in fp32).
 * pairs_out [cap][2] (row of fa, row of fb) in ascending i, d2_out [cap] (may be NULL), *count_out = the number kept.
 * SYMMICP_ERR_SIZE when the count exceeds cap: *count_out is set, nothing else is written (cap >= na always suffices;
 * pairs_out may be NULL with cap == 0 to ask for the count).
 * SYMMICP_ERR_ARG: as feature_nn; NULL count_out; NULL pairs_out with cap > 0; a max_ratio that is NaN. */
int symmicp_ctx_feature_correspondences(symmicp_ctx *ctx, const float *fa, size_t na, const float *fb, size_t nb, int mutual,
                                        float max_ratio, int32_t *pairs_out, float *d2_out, size_t cap, size_t *count_out);
int symmicp_feature_correspondences(int device, const float *fa, size_t na, const float *fb, size_t nb, int mutual,
                                    float max_ratio, int32_t *pairs_out, float *d2_out, size_t cap, size_t *count_out);

/* symmicp_ctx_ransac: a rigid transform from correspondences with outliers -- Open3D's
 * registration_ransac_based_on_correspondence (three-pair samples, edge-length pre-rejection, inliers counted over the
 * correspondence set, a least-squares refit on the winner's inliers), arranged as a pure function of its inputs.
 *   Pivots.  cs, ct = the fp64 means of the m source / target points of the pairs, rounded to fp32; the device works on
 *     p_k = src[pairs[k][0]] - cs, q_k = tgt[pairs[k][1]] - ct (fp32).  The returned transform is in the caller's coordinates
 *     (composed in fp64 on the host).
 *   Samples.  Hypothesis h (0 <= h < hypotheses) draws c_k = ((u(3h + k) >> 32) * m) >> 32, k = 0, 1, 2, where u(i) is value i
 *     of the SplitMix64 sequence of (seed, stream 0):
 *       mix64(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *       base = mix64(seed * 0x9E3779B97F4A7C15 + 0x2545F4914F6CDD1D);   u(i) = mix64(base + (i + 1) * 0x9E3779B97F4A7C15)
 *     (64-bit wrap-around arithmetic).  No rejection loop; every hypothesis gets a status, the checks in this order, with
 *     a, b, c = the sample's p (likewise q) and e = edge_ratio:
 *       1 REPEATED    two draws are equal
 *       2 EDGE        for an edge x-y of the triangle |p_x - p_y|^2 < e^2 |q_x - q_y|^2 or |q_x - q_y|^2 < e^2 |p_x - p_y|^2
 *                     (edges 0-1, 1-2, 2-0; off when e <= 0)
 *       3 DEGENERATE  |(b - a) x (c - a)|^2 < 1e-4 |b - a|^2 |c - a|^2, or that product not > 0, in either cloud (the sine of the
 *                     angle at a below 0.01: this bounds how much the frames amplify fp32 rounding)
 *       4 FAR         one of the three sample pairs is farther than max_dist under the hypothesis
 *       0 EVALUATED
 *   Hypothesis.  Orthonormal frames: e1 = (b - a) / |b - a|, e3 = (e1 x (c - a)) / |e1 x (c - a)|, e2 = e3 x e1, F = [e1 e2 e3];
 *     R = F_q F_p^T, t = mean(q) - R mean(p) (means of the three sample points).
 *   Score.  inliers(h) = the number of k with |R p_k + t - q_k|^2 <= max_dist^2 (fp32).  The winner is the evaluated hypothesis
 *     with the most inliers, ties to the lowest h.  None evaluated, or a winner with fewer than 3 inliers:
 *     SYMMICP_ERR_NO_CONSENSUS, transform = identity.
 *   Refit.  `refits` times: R, t = the least-squares rigid fit (Horn's quaternion method, a proper rotation) to the current
 *     inlier set, in fp64 on the host in ascending k and in the caller's coordinates; then the inlier set is recomputed under
 *     it in fp64 (|R x + t - y|^2 <= max_dist^2).  A refit that leaves fewer than 3 inliers is SYMMICP_ERR_NO_CONSENSUS.
 * src_xyz (ns points) and tgt_xyz (nt points) strided as in symmicp_set_source; pairs [m][2] int32 (source row, target row).
 * Outputs: transform16 (row-major 4x4, source -> target; required), result (required), inlier_mask_out [m] (uint8, the final
 * inlier set; with refits == 0 the winner's), status_out [hypotheses] (uint8) and inliers_out [hypotheses] (int32, 0 unless
 * evaluated); the last three may be NULL.
 * SYMMICP_ERR_ARG: NULL src_xyz / tgt_xyz / pairs / cfg / transform16 / result; ns, nt == 0 or > 2^31 - 1; m < 3 or > 2^31 - 1;
 * a pair row out of range; cfg->struct_size != sizeof(symmicp_ransac_config); hypotheses outside 1 .. 2^24; max_dist not finite
 * and > 0; edge_ratio > 1 or NaN; refits outside 0 .. 8; a non-finite coordinate among the paired points. */
typedef struct {
    uint32_t struct_size;      /* = sizeof(symmicp_ransac_config), checked */
    uint32_t hypotheses;       /* H, 1 .. 2^24 */
    uint64_t seed;
    float max_dist;            /* finite, > 0 */
    float edge_ratio;          /* 0 < e <= 1, default 0.9; <= 0: the edge check is off */
    int32_t refits;            /* 0 .. 8, default 1 */
    int32_t reserved;
} symmicp_ransac_config;
typedef struct {
    int32_t best_hypothesis;   /* -1: none */
    int32_t evaluated;         /* hypotheses with status EVALUATED */
    int32_t inliers_ransac;    /* the winner's inliers (fp32, on the device) */
    int32_t inliers_final;     /* after the refits */
    double rmse_final;         /* over the final inliers */
    double transform[16];      /* the result in fp64, row-major; transform16 is this matrix rounded to fp32 */
} symmicp_ransac_result;
#define SYMMICP_RANSAC_EVALUATED 0
#define SYMMICP_RANSAC_REPEATED 1
#define SYMMICP_RANSAC_EDGE 2
#define SYMMICP_RANSAC_DEGENERATE 3
#define SYMMICP_RANSAC_FAR 4
/* hypotheses 100 000, seed 0, max_dist 0 (the caller sets it), edge_ratio 0.9, refits 1 */
void symmicp_ransac_config_default(symmicp_ransac_config *cfg);
int symmicp_ctx_ransac(symmicp_ctx *ctx, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                       const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                       const int32_t *pairs, size_t m, const symmicp_ransac_config *cfg, float transform16[16],
                       symmicp_ransac_result *result, uint8_t *inlier_mask_out, uint8_t *status_out, int32_t *inliers_out);
int symmicp_ransac(int device, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                   const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                   const int32_t *pairs, size_t m, const symmicp_ransac_config *cfg, float transform16[16],
                   symmicp_ransac_result *result, uint8_t *inlier_mask_out, uint8_t *status_out, int32_t *inliers_out);
/* test entry: the 12 floats (R row-major, then t, about the pivots) the device computed for every hypothesis: hyp_out
 * [hypotheses][12], written for status EVALUATED and FAR, zero otherwise; pivots_out [6] = cs, ct.  Arguments as above. */
int symmicp_ctx_ransac_hypotheses(symmicp_ctx *ctx, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                                  const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                                  const int32_t *pairs, size_t m, const symmicp_ransac_config *cfg, float *hyp_out,
                                  uint8_t *status_out, float pivots_out[6]);

/* symmicp_ctx_fgr: Fast Global Registration (Zhou, Park, Koltun, ECCV 2016; Open3D's registration_fgr_based_on_correspondence):
 * a rigid transform from correspondences with outliers by a tuple test and a graduated-non-convexity (GNC) loop, the whole loop in
 * one launch.  A pure function of its inputs: no hypothesis count, no lucky sample.  Arguments and pivots as symmicp_ctx_ransac.
 *   Pivots.  cs, ct = the fp64 means of the m paired source / target points, rounded to fp32; the device works on
 *     p_k = src[pairs[k][0]] - cs, q_k = tgt[pairs[k][1]] - ct (fp32): FGR's centring, so the loop starts from the identity.
 *   Tuple test.  Trial t (0 <= t < tuple_trials; 0 means min(100 m, 2^24)) draws c_j = ((u(3t + j) >> 32) * m) >> 32, j = 0, 1, 2,
 *     u = the SplitMix64 sequence of (seed, stream 1): RANSAC's with
 *       base = mix64(seed * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03 + 0x2545F4914F6CDD1D).
 *     A trial is accepted iff its draws are distinct and no edge fails RANSAC's EDGE check with e = tuple_scale (e^2 in fp32).
 *     The optimisation set is the draws of the first min(accepted, max_tuples) accepted trials in ascending t, three per tuple,
 *     duplicates kept (a pair in several tuples counts several times); M = its length.  max_tuples == 0: the set is all m pairs
 *     in order, M = m.  No accepted trial: SYMMICP_ERR_NO_CONSENSUS, transform = identity.
 *   Schedule (fp32).  D2 = the maximum over all m pairs of max(|p|^2, |q|^2), |v|^2 = (x x + y y) + z z; mu = D2;
 *     d2 = max_dist * max_dist.  At the top of iteration k = 0 .. iterations - 1: if k % decrease_every == 0 and mu > d2 then
 *     mu = mu / division_factor, and if then mu < d2, mu = d2.
 *   Pass k at X_k (X_0 = I), for each element of the set (fp32, unfused):  p' = ((X0 x + X1 y) + X2 z) + X3 per row;
 *     d = p' - q; r2 = (dx dx + dy dy) + dz dz; t = mu / (mu + r2); l = t * t (the line-process weight: Geman-McClure at scale
 *     sqrt(mu)).  Three rows of PLANE's form with n = e_x, e_y, e_z -- v = (p' x n, n), c = d . n -- each at weight l, accumulated
 *     in fp64 into a record of PLANE's weighted shape about a zero pivot: [0..20] sum l v v^T, [21..26] sum l v c,
 *     [27..29] sum l p', [30..32] sum l q, [33] 0, [34] sum l, [35] sum l r2, [36] sum r2, [37] M.
 *   Solve.  symmicp_solve(SYMMICP_MODE_PLANE, ...) on that record, run on the device; X_{k+1} = increment * X_k (fp32).  A solve
 *     that fails ends the loop: SYMMICP_ERR_DEGENERATE with the iterations completed and X_k as the transform.
 *   Result.  T = T(ct) X T(-cs) in fp64 on the host, transform16 its fp32 rounding; inliers and rmse over all m pairs at
 *     |T x - y|^2 <= max_dist^2 (fp64).  There is no refit after the loop.
 * Outputs: transform16, result (required); set_out [3 * max_tuples, or m when max_tuples == 0] (int32 rows of `pairs`; the first
 * set_size are written); weight_out [same capacity]: l of the last pass run; X_trace [iterations + 1][16] (X_k; rows after the
 * last one reached are zero), sums_trace [iterations][40], mu_trace [iterations]; all five may be NULL.
 * SYMMICP_ERR_ARG: NULL src_xyz / tgt_xyz / pairs / cfg / transform16 / result; ns, nt == 0 or > 2^31 - 1; m < 3 or > 2^31 - 1;
 * m > 2^20 with max_tuples == 0; a pair row out of range; a non-finite paired coordinate; cfg->struct_size; max_dist not finite
 * and > 0; iterations outside 1 .. 1024; decrease_every < 1; division_factor not finite and > 1; tuple_scale outside (0, 1];
 * max_tuples > 2^18; tuple_trials > 2^24. */
typedef struct {
    uint32_t struct_size;      /* = sizeof(symmicp_fgr_config), checked */
    int32_t iterations;        /* 1 .. 1024, default 64 */
    int32_t decrease_every;    /* >= 1, default 4 */
    uint32_t max_tuples;       /* 0 .. 2^18, default 1000; 0: the tuple test is off */
    uint32_t tuple_trials;     /* 1 .. 2^24; default 0: min(100 m, 2^24) */
    float max_dist;            /* delta: finite, > 0 */
    float division_factor;     /* finite, > 1, default 1.4 */
    float tuple_scale;         /* 0 < s <= 1, default 0.95 */
    uint64_t seed;
} symmicp_fgr_config;
typedef struct {
    int32_t iterations;        /* iterations completed */
    int32_t inliers;           /* pairs within max_dist of the result, of all m */
    uint32_t tuples_accepted;  /* trials that passed the tuple test (0 with the test off) */
    uint32_t set_size;         /* M */
    float mu;                  /* of the last pass run */
    int32_t reserved;
    double weight_sum;         /* sum l of the last pass run */
    double rmse;               /* over the inliers */
    double transform[16];      /* the result in fp64, row-major; transform16 is this matrix rounded to fp32 */
} symmicp_fgr_result;
/* iterations 64, decrease_every 4, max_tuples 1000, tuple_trials 0, max_dist 0 (the caller sets it), division_factor 1.4,
 * tuple_scale 0.95, seed 0 */
void symmicp_fgr_config_default(symmicp_fgr_config *cfg);
int symmicp_ctx_fgr(symmicp_ctx *ctx, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                    const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                    const int32_t *pairs, size_t m, const symmicp_fgr_config *cfg, float transform16[16],
                    symmicp_fgr_result *result, int32_t *set_out, float *weight_out, float *X_trace, double *sums_trace,
                    float *mu_trace);
int symmicp_fgr(int device, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                const int32_t *pairs, size_t m, const symmicp_fgr_config *cfg, float transform16[16],
                symmicp_fgr_result *result, int32_t *set_out, float *weight_out, float *X_trace, double *sums_trace,
                float *mu_trace);
/* test entry: one pass of the loop on host arrays p, q [M][3] (already pivoted; 1 <= M <= 2^20) at X16 and mu, through the loop
 * kernel's own accumulation and reduction: sums_out [40] (required), weight_out [M] (may be NULL).
 * SYMMICP_ERR_ARG: NULL p / q / X16 / sums_out; M out of range; a non-finite value in p, q, X16 or mu. */
int symmicp_ctx_fgr_pass(symmicp_ctx *ctx, const float *p, const float *q, size_t M, const float X16[16], float mu,
                         double *sums_out, float *weight_out);

/* ---- voxel-grid downsampling (PCL's pcl::VoxelGrid, Open3D's voxel_down_sample), on the GPU -----------------------
 * Every point falls into the cubic voxel of edge `leaf` that holds it; each occupied voxel with at least min_points points
 * becomes one output point.  The arithmetic is exact and reproducible bit for bit ("Voxel downsampling"):
 *   inv = 1.0f / leaf; per axis lo = floorf(min * inv), hi = floorf(max * inv) over the cloud's box, n_axis = hi - lo + 1;
 *   a point's cell ix = (int)floorf(x * inv) - lo_x (likewise iy, iz), key = ix + nx * (iy + ny * iz) (x fastest, z slowest);
 *   output = the occupied voxels in ascending key; xyz_out = the members' fp32 sum taken one point at a time in ascending row
 *   order, divided by (float)count; nrm_out = the members' normal sum s in the same order divided by sqrtf((sx*sx + sy*sy) +
 *   sz*sz) when that is > 0, else (0, 0, 0).  Every op is fp32, unfused, correctly rounded.
 * xyz and nrm strided as in symmicp_set_source (nrm may be NULL, its strides ignored then).  Outputs: xyz_out / nrm_out packed
 * AoS [m][3], count_out [m] (points per output voxel), voxel_of [n] (the output row of every input row, -1 for the rows of
 * voxels dropped by min_points); count_out and voxel_of may be NULL; nrm_out requires nrm.  *n_out = m.
 * SYMMICP_ERR_SIZE when m > cap (*n_out = m is set, nothing else is written; cap >= n always suffices).
 * SYMMICP_ERR_ARG: NULL xyz / xyz_out / n_out; n == 0 or n > 2^31 - 1; a leaf that is not finite and > 0; min_points < 1;
 * nrm_out without nrm; non-finite coordinates; a leaf too small for the cloud (some lo or hi outside [-2^31, 2^31), or
 * nx * ny * nz > 2^32).
 * The ctx form runs on the context's stream and temporary arena, like symmicp_ctx_estimate_normals: the context's source,
 * target, index and certificates stay exactly as they were.  A sharded job downsamples the FULL cloud on every rank (the
 * output is deterministic, so all ranks get the same cloud) and hands it to symmicp_set_source, which shards it. */
int symmicp_ctx_voxel_downsample(symmicp_ctx *ctx, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                                 const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride, size_t n, float leaf, int min_points,
                                 float *xyz_out, float *nrm_out, int32_t *count_out, int32_t *voxel_of, size_t cap, size_t *n_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_voxel_downsample(int device, const float *xyz, size_t xyz_row_stride, size_t xyz_col_stride,
                             const float *nrm, size_t nrm_row_stride, size_t nrm_col_stride, size_t n, float leaf, int min_points,
                             float *xyz_out, float *nrm_out, int32_t *count_out, int32_t *voxel_of, size_t cap, size_t *n_out);

/* ---- NDT registration (SYMMICP_MODE_NDT): voxel Gaussians on the GPU --------------------------------------------------------------
 * The mode is DEFINED by the arithmetic below ("NDT"; tests/_ndt_ref.py is the same in numpy).  Every fp32 expression is
 * unfused, in the association written.
 *
 * Parameters (symmicp_ndt_config; symmicp_ndt_config_default: resolution 1, min_points 6, eig_ratio 0.01, outlier_ratio 0.55,
 * neighbors 7 -- PCL's values, 7 being its "direct 7" neighbourhood).  SYMMICP_ERR_ARG for a wrong struct_size, a resolution that is
 * not finite and > 0, min_points < 3, eig_ratio outside (0, 1], outlier_ratio outside (0, 1), neighbors other than 1 or 7; a refused
 * setter leaves the configuration as it was.
 *
 * Grid.  symmicp_ctx_voxel_downsample's, over the target's box, with leaf = resolution: inv = 1.0f / resolution; per axis
 *   lo = floorf(min * inv), hi = floorf(max * inv), n_axis = hi - lo + 1; key = ix + nx * (iy + ny * iz).  The same refusals, and one
 *   more: every |lo| and |hi| must be < 2^23 (cell coordinates are then exact as floats), else SYMMICP_ERR_ARG.
 * Map.  For every occupied voxel with count >= min_points, in ascending key:
 *   mu64 = the fp64 sum of the members, one point at a time in ascending caller row, divided by count; mean = (float)mu64.
 *   C = sum (x - mu64)(x - mu64)^T / (count - 1): fp64 products and sums, unfused, same order; its upper triangle (xx xy xz yy yz zz) is
 *   kept as 6 doubles.  Eigen-decomposition of C by the fp64 cyclic Jacobi of the normals pre-step.  The voxel is dropped unless
 *   lambda_max is finite and > 0.  lambda'_r = max(lambda_r, eig_ratio * lambda_max); axes l_r = the eigenvectors rounded to fp32, in
 *   ascending lambda; o_r = (float)(1 / lambda'_r); M = sum_r o_r l_r l_r^T is the voxel's inverse covariance.  Dropped voxels do not
 *   exist: a map row is a kept voxel, rows ascend with the key.
 * Gauss constants.  symmicp_ndt_gauss(outlier_ratio p_o, &d1, &d2), a pure host function in fp64 (a context calls it with its fp32
 *   outlier_ratio widened to fp64):
 *   c1 = 10 (1 - p_o), c2 = p_o, d3 = -log c2, d1 = -log(c1 + c2) - d3, d2 = -2 log((-log(c1 exp(-1/2) + c2) - d3) / d1).
 *   This is PCL's formula with c2 taken at resolution 1.  PCL divides c2 by resolution^3, which ties the weight to the unit of length;
 *   here the same cloud in other units, with the resolution scaled along, takes the same steps.  At 0.55: d1 = -2.217225244...,
 *   d2 = 0.433123004....  The pass's constant is h = (float)(0.5 * d2).  SYMMICP_ERR_ARG for a ratio outside (0, 1) or a NULL pointer.
 * Weight.  symmicp_ndt_weight(x), one source for host and device, a plain-arithmetic exp(x) on (-64, 0]:
 *   if !(x > -64.0f) return 0 (NaN too); if x > 0, x = 0; k = rintf(x * 1.44269504f); r = (x - k * 0.693359375f) - k * (-2.12194440e-4f);
 *   p = Horner over r with 1.9875691500e-4f, 1.3981999507e-3f, 8.3334519073e-3f, 4.1665795894e-2f, 1.6666665459e-1f, 5.0000001201e-1f;
 *   y = (p * (r * r) + r) + 1.0f; return ldexpf(y, (int)k).
 * A pass.  y_i = the three top rows of X applied to source row i in fp32 (as every mode moves a point); g = floorf(y * inv) per axis,
 *   kept as floats.  Candidate cells: g itself (neighbors = 1), and g +- 1 on each single axis as well (neighbors = 7).  A candidate is
 *   an ITEM iff lo <= g <= hi on all three axes (float compares) and the map holds that cell's voxel.  Per item, with p = y - pivot,
 *   mu = mean - pivot (fp32 subtractions), d = p - mu:
 *     c_r = (dx*lx + dy*ly) + dz*lz for each axis l_r; the row v_r = (p x l_r, l_r) formed exactly as PLANE forms (p x n, n);
 *     m = ((o0*c0)*c0 + (o1*c1)*c1) + (o2*c2)*c2;  w = symmicp_ndt_weight(-(h * m));  d2 = (dx*dx + dy*dy) + dz*dz.
 *     With max_corr_dist > 0 the item is dropped when d2 > max_corr_dist^2 (the rule of every mode).
 *   The three rows enter the record as PLANE rows at weight (double)w * (double)o_r:
 *     [0..26] sum w o v v^T, sum w o v c   [27..32] sum w p, sum w mu   [33] sum sqrtf(d2)   [34] sum w   [35] sum w m   [36] sum d2
 *     [37] the number of items (what symmicp_iter_result.pairs reports).
 * Solve.  symmicp_solve(SYMMICP_MODE_NDT) is PLANE's solve: each step is the Gauss-Newton (IRLS) step of the NDT score; the constant
 *   -d1 d2 cancels out of it.  The score of a pass is -d1 * [34]: symmicp_get_ndt_state reports it and the item count of the most recent
 *   pass (SYMMICP_ERR_STATE before one).
 * Engine.  cfg.corr is not read in this mode: symmicp_set_target builds the map instead of an index (and the N_s = N_t rule of identity
 *   pairing does not apply); nrm == NULL is accepted for both clouds; cfg.sort_source is honoured as BRUTE / TREE honour it.
 *   symmicp_align runs the host loop.  symmicp_set_ndt on an NDT context that holds a target rebuilds the map at once from the planar
 *   copy the context keeps -- bit for bit the map of a fresh symmicp_set_target -- and resets the loop state as symmicp_set_target does.
 *   symmicp_get_correspondences reports per caller row the map row of the point's OWN cell (-1: no voxel there) and d2 to that voxel's
 *   mean as a pass forms it (0 when there is none).  symmicp_evaluate builds a temporary index, as every non-TREE context does.
 * Refused: a robust loss, a trim fraction below 1, one-to-one, a median factor, reciprocal correspondences, min_normal_dot > -1 and
 *   SYMMICP_APPLY_INCREMENTAL (SYMMICP_ERR_ARG, from the setter on an NDT context and from symmicp_set_config into NDT alike);
 *   nranks > 1 (SYMMICP_ERR_STATE, both ways round); symmicp_set_config into or out of NDT while a cloud is set (SYMMICP_ERR_STATE);
 *   symmicp_batch_align in this mode (SYMMICP_ERR_ARG).
 *
 * symmicp_ctx_ndt_map builds the map of any cloud on a context the caller owns and leaves that context untouched; every output may be
 * NULL: key_out [m], count_out [m], mean_out [m][3], cov_out [m][6], axes_out [m][3][3] (axis r at [m][r][0..2]), inv_eig_out [m][3]
 * (o_r), grid_out = lo xyz, n xyz.  *m_out = m always (required); SYMMICP_ERR_SIZE when m > cap, nothing else is written then.  Its
 * argument checks (NULL xyz / cfg / m_out, n == 0 or > 2^31 - 1, the configuration's rules, non-finite coordinates) are decided on the
 * host before a device is needed.  symmicp_ndt_map is the same on a context of its own; symmicp_get_ndt_map reads the map an NDT context
 * holds (SYMMICP_ERR_STATE without one). */
typedef struct {
    int32_t struct_size;       /* = sizeof(symmicp_ndt_config), checked */
    float   resolution;        /* voxel edge */
    int32_t min_points;        /* voxels with fewer points have no Gaussian (>= 3) */
    float   eig_ratio;         /* eigenvalues are raised to eig_ratio * the largest */
    float   outlier_ratio;     /* p_o of the Gauss constants */
    int32_t neighbors;         /* 1: the point's own cell; 7: and its six face neighbours */
} symmicp_ndt_config;
void symmicp_ndt_config_default(symmicp_ndt_config *cfg);
int symmicp_set_ndt(symmicp_ctx *ctx, const symmicp_ndt_config *cfg);
int symmicp_get_ndt(const symmicp_ctx *ctx, symmicp_ndt_config *cfg);
int symmicp_ndt_gauss(double outlier_ratio, double *d1, double *d2);
float symmicp_ndt_weight(float x);
int symmicp_get_ndt_state(const symmicp_ctx *ctx, double *score, uint64_t *items);
int symmicp_ctx_ndt_map(symmicp_ctx *ctx, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_ndt_config *cfg,
                        uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out, float *axes_out, float *inv_eig_out,
                        int32_t grid_out[6], size_t cap, size_t *m_out);
int symmicp_ndt_map(int device, const float *xyz, size_t row_stride, size_t col_stride, size_t n, const symmicp_ndt_config *cfg,
                    uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out, float *axes_out, float *inv_eig_out,
                    int32_t grid_out[6], size_t cap, size_t *m_out);
int symmicp_get_ndt_map(symmicp_ctx *ctx, uint32_t *key_out, int32_t *count_out, float *mean_out, double *cov_out, float *axes_out,
                        float *inv_eig_out, int32_t grid_out[6], size_t cap, size_t *m_out);

/* ---- registration evaluation: fitness, inlier RMSE, information matrix (PCL's getFitnessScore, Open3D's evaluate_registration and
 * get_information_matrix_from_point_clouds) -----------------------------------------------------------------------------------------
 * How good an alignment is, as a pure function of (source, target, transform, distance): exact, reproducible bit for bit, and it leaves a
 * context exactly as it found it.  Several transforms are evaluated in one call, so that the results of a multi-start or a list of
 * RANSAC hypotheses are ranked on the full clouds at one common distance.  For a source of ns points, a target of nt points, a row-major
 * 4x4 X and max_dist:
 *   Moved point   y_i = the three top rows of X applied to source row i with w = 1, in fp32 and unfused: ((m0 x + m1 y) + m2 z) + m3.
 *                 X's bottom row is ignored.
 *   Neighbour     nn(i) = the target row j that minimises (d2(i, j), j) lexicographically, d2 the fp32 (dx dx + dy dy) + dz dz of
 *                 y_i - q_j (the distance of every pass; ties go to the lowest caller row).  The search is exact.
 *   Inlier        r2 = max_dist * max_dist in fp32.  Row i is an inlier iff max_dist <= 0 or d2_i <= r2 -- the rule by which the passes apply
 *                 max_corr_dist.
 *   Per point     nn_out[i], d2_out[i] (each may be NULL): nn(i) and d2_i for an inlier, -1 and +Inf otherwise.
 *   Sums          over the inliers: inliers = their count, sum_d2 = sum (double)d2_i, sum_q = sum q, sum_qq = the upper triangle
 *                 (xx, xy, xz, yy, yz, zz) of sum q q^T, q = q_nn(i) in the CALLER's coordinates widened to fp64 (the products are exact).
 *                 Order: a function of ns alone.  With T = 1024, B = min(ceil(ns / T), 4096): lane t (0 .. 255) of block b (0 .. B - 1)
 *                 adds the terms of the caller rows tile * T + 256 j + t, for tile = b, b + B, ... and j = 0 .. 3, in that order; the 256
 *                 lane sums of a block are added pairwise (t += t + 128, then + 64, ... + 1); the B block sums are added by lane t over
 *                 the blocks t, t + 256, ... ascending and then by the same pairwise tree.  No floating-point atomics.
 *   Derived       fitness = inliers / ns; mean_d2 = sum_d2 / inliers (PCL's getFitnessScore); rmse = sqrt(sum_d2 / inliers); rmse and
 *                 mean_d2 are 0 when there are no inliers.
 *   Information   information[36], row-major, rotation first, translation last: Open3D's GetInformationMatrixFromPointClouds,
 *                 L = sum G^T G over the inliers, where for q = (x, y, z) the rows of G are (0, z, -y, 1, 0, 0), (-z, 0, x, 0, 1, 0) and
 *                 (y, -x, 0, 0, 0, 1).  Computed in fp64 on the host from the sums by its closed form (symmicp_information_from_sums):
 *                 with S = sum_qq, s = sum_q, n = inliers, the rotation block is tr(S) I - S with the diagonal Syy + Szz, Sxx + Szz,
 *                 Sxx + Syy and the off-diagonals -Sxy, -Sxz, -Syz; the rotation-translation block is [s]x = (0, -sz, sy; sz, 0, -sx;
 *                 -sy, sx, 0), the translation-rotation block its transpose, the translation block n I.  The information is about the
 *                 CALLER's origin, as Open3D's is: a back end that linearises about another point moves it there itself.
 *   Purity        K is 1 .. 4096; result k is a function of X_k alone: bit for bit the same whatever K, whatever its place in the list,
 *                 and from run to run.
 * Target -> source (Chamfer's other half, the covered share of the target) is the same call with the clouds swapped and the rows of
 * symmicp_inverse_rigid(X) as the transform.
 * Out of scope: sharded contexts; point-to-plane residual statistics; a pose covariance from the record.  (The pose-graph optimiser that consumes the
 * information matrix is symmicp_ctx_posegraph_optimize, below.) */
typedef struct {
    uint64_t inliers;
    double fitness;            /* inliers / ns */
    double rmse;               /* sqrt(sum_d2 / inliers); 0 without inliers */
    double mean_d2;            /* sum_d2 / inliers (PCL's getFitnessScore); 0 without inliers */
    double sum_d2;
    double sum_q[3];
    double sum_qq[6];          /* xx, xy, xz, yy, yz, zz */
    double information[36];    /* row-major 6x6, rotation first */
} symmicp_evaluation;
/* the closed form above: a pure host function (SYMMICP_ERR_ARG for a NULL pointer) */
int symmicp_information_from_sums(uint64_t n, const double sum_q[3], const double sum_qq[6], double out36[36]);
/* On host arrays strided as in symmicp_set_source.  X16 [K][16] (NULL: the identity, K == 1); out [K]; nn_out / d2_out [K][ns] or NULL.
 * Runs on the context's stream and temporary memory, like symmicp_ctx_radius_search: the context's clouds, index, certificates, options
 * and states stay as they were.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed: a NULL cloud or out; ns or nt of 0 or above 2^31 - 1; K outside
 * 1 .. 4096; NULL X16 with K != 1; a non-finite entry in the top three rows of any X_k; a max_dist that is NaN or +-Inf; non-finite
 * coordinates.  (nn_out and d2_out are sized by the caller.) */
int symmicp_ctx_evaluate_registration(symmicp_ctx *ctx, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                                      const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                                      const float *X16, size_t K, float max_dist, symmicp_evaluation *out, int32_t *nn_out, float *d2_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_evaluate_registration(int device, const float *src_xyz, size_t src_row_stride, size_t src_col_stride, size_t ns,
                                  const float *tgt_xyz, size_t tgt_row_stride, size_t tgt_col_stride, size_t nt,
                                  const float *X16, size_t K, float max_dist, symmicp_evaluation *out, int32_t *nn_out, float *d2_out);
/* The same function on the clouds the context already holds; nothing is uploaded.  The source is the source as symmicp_set_source
 * received it -- never the written-back copy, in either apply mode and either source order -- and each X_k is applied to THAT source: it
 * is not composed with the context's transform.  X16 == NULL with K == 1 means the context's current cumulative transform, what
 * symmicp_get_transform returns.  Rows are in the caller's numbering for both clouds.  Every symmicp_corr is accepted: a TREE context
 * walks its own index, the others build a temporary one that is dropped before returning.  The result is bit for bit that of the
 * host-array form on the same clouds.  It may be called between two symmicp_step calls: pairs, certificates, rejection states, loop
 * state, loop log and the pass counts of symmicp_stats stay exactly as they were.
 * SYMMICP_ERR_ARG as above (out, K, X16, max_dist).  SYMMICP_ERR_STATE: before both clouds are set; on a sharded context (nranks > 1: the
 * sums would need an exchange; out of scope, as for the rejectors). */
int symmicp_evaluate(symmicp_ctx *ctx, const float *X16, size_t K, float max_dist, symmicp_evaluation *out, int32_t *nn_out, float *d2_out);

/* ---- multiway registration: pose-graph optimisation (Choi, Zhou, Koltun, CVPR 2015; Open3D's global_optimization is the inspiration,
 * the definitions below are the yardstick) --------------------------------------------------------------------------------------------
 * Makes the pairwise transforms of more than two scans consistent: Levenberg-Marquardt over the poses, with a line process that switches
 * false loop closures off.  It consumes the information matrix of symmicp_evaluation.  Everything is fp64.  A pure function of its
 * arguments, bit for bit the same from run to run; the context's clouds, index, options and states stay as they were.
 *   Graph        n nodes (2 .. 1024); node i has a pose X_i: row-major 4x4, the top three rows are read, taking node i's frame to the
 *                world.  m edges (1 .. 16384); edge (source s, target t, T, L, uncertain), s != t: T takes s's frame to t's frame --
 *                what symmicp_align returns with cloud s as source and cloud t as target; L = symmicp_evaluation.information of that
 *                pair (rotation first, about the target's origin; only the upper triangle is read); uncertain = 0 for odometry, anything
 *                else for a loop closure.  Several edges between the same two nodes are allowed, in either direction.
 *   Edge error   E = X_t^-1 X_s T^-1, both inverses the rigid ones (R^T, -R^T t): E acts on t's frame, a target point q lands at E q
 *                under the current poses, which is why L = sum G^T G of the evaluation applies to it.  e = (w, tau): tau = E's
 *                translation, w = the rotation vector of E's rotation R, angle in [0, pi]:
 *                  v = ((R21 - R12) / 2, (R02 - R20) / 2, (R10 - R01) / 2), c = clamp(((R00 + R11 + R22) - 1) / 2, -1, 1), s2 = v . v;
 *                  s2 >= 1e-8:            w = v * (atan2(sqrt(s2), c) / sqrt(s2));
 *                  s2 < 1e-8 and c > 0:   w = v * (1 + s2 / 6 + 3 s2^2 / 40)             (the series of asin(s) / s);
 *                  s2 < 1e-8 and c <= 0:  (near pi) w = atan2(sqrt(s2), c) * a, a the unit axis from the symmetric part: i = the largest
 *                                         diagonal entry (lowest i on ties), a_i = sqrt(max((R_ii - c) / (1 - c), 0)),
 *                                         a_j = (R_ij + R_ji) / (2 (1 - c) a_i), the whole of it negated if a . v < 0.
 *                c = e^T L e (L the symmetric matrix of the upper triangle).
 *   Line process l = 1 for a certain edge, l = (mu / (mu + c))^2 for an uncertain one.  Cost F = sum over certain edges of c + sum over
 *                uncertain edges of mu c / (mu + c): the line-process objective with l eliminated.  mu = line_process_weight if that is
 *                > 0; otherwise, with at least one uncertain edge, mu = preference_loop_closure * max_dist^2 * (the mean over ALL edges
 *                of L[35], the inlier count of the translation block), in fp64 on the host; a graph without uncertain edges has no mu
 *                (reported as line_process_weight).
 *   Update       X_i <- X_i Exp(d_i), d = (w, tau), Exp(d) = [exp([w]x) tau; 0 1]; exp([w]x) = I + A [w]x + B [w]x^2 with t2 = w . w,
 *                A = sin(t) / t, B = (1 - cos(t)) / t2, t = sqrt(t2), and below t2 = 1e-8 the series A = 1 - t2 / 6 + t2^2 / 120,
 *                B = 1 / 2 - t2 / 24 + t2^2 / 720.  The reference node takes no update: its pose comes back bit for bit (all 16 values).
 *                The other poses come back with the bottom row 0 0 0 1.
 *   Linearised   to first order about E = I (exact at a consistent graph): J_t = -I, J_s = Ad(T) = [R_T 0; [t_T]x R_T  R_T].  Per edge,
 *                with W = l L:  H_ss += Ad^T W Ad, H_tt += W, H_st -= Ad^T W, g_s += Ad^T W e, g_t -= W e.
 *   Step         (H + lambda I) d = -g over the free nodes, by a block-Jacobi preconditioned conjugate gradient on the device: the
 *                preconditioner is the 6x6 Cholesky factor of H_ii + lambda I of every node; the solve stops at
 *                r . r <= cg_tolerance^2 * g . g or after cg_max_iterations (0: 6 (n - 1)).
 *   Control      on the host, from one record per iteration.  lambda_0 = 1e-5 * the largest diagonal entry of H at the initial poses.
 *                Iteration: linearise at X, solve, X' = X Exp(d), F' = F(X').  Accepted iff F' < F; then X <- X',
 *                lambda <- lambda * max(1 / 3, 1 - (2 rho - 1)^3) with rho = (F - F') / (d . (lambda d - g)), nu = 2, and the loop
 *                stops if F - F' <= min_relative_decrease * F (stop reason 2).  Rejected: lambda <- lambda * nu, nu <- 2 nu.  After
 *                either: stop if max |d| <= min_increment (3), then if the iteration count has reached max_iterations (1).
 *   Pruning      after the loop an uncertain edge with l < edge_prune_threshold at the final poses is reported as pruned.  There is
 *                no second optimisation without them.
 *   Order        every sum has a fixed order: a node's blocks are added over its incident edges by ascending edge index; dot products
 *                and the cost are per-thread partial sums over a fixed stride followed by a pairwise tree.  No floating-point atomics.
 * SYMMICP_ERR_ARG, all decided on the host before a device is needed, with every output untouched: NULL poses_in / edges / cfg /
 * poses_out / result; a wrong struct_size; n outside 2 .. 1024 or m outside 1 .. 16384; a node index out of range or s == t; a graph that
 * is not connected; reference_node outside 0 .. n - 1; a non-finite entry in the top three rows of any X, of any T, or in the upper
 * triangle of any L; a rotation block of an X or a T with max |R^T R - I| > 1e-6; max_iterations outside 1 .. 10000; cg_max_iterations
 * outside 0 .. 100000; line_process_weight not finite or < 0; when mu has to be derived, max_dist or preference_loop_closure not finite
 * and > 0; edge_prune_threshold outside [0, 1]; min_relative_decrease or min_increment not finite or < 0; cg_tolerance outside (0, 1).
 * SYMMICP_ERR_DEGENERATE: a node block H_ii + lambda I that is not finite or not positive definite on the device; poses_out holds the
 * last accepted poses.
 * Out of scope: sharded contexts (nranks > 1: SYMMICP_ERR_STATE); graphs above the caps; re-optimisation after pruning; exact
 * (non-first-order) Jacobians. */
#define SYMMICP_POSEGRAPH_MAX_NODES 1024
#define SYMMICP_POSEGRAPH_MAX_EDGES 16384
typedef struct {
    int32_t source, target;    /* s, t */
    int32_t uncertain;         /* 0: odometry; else a loop closure */
    int32_t reserved;
    double transform[16];      /* T, row-major; the top three rows are read */
    double information[36];    /* L, row-major, rotation first; the upper triangle is read */
} symmicp_pose_edge;
typedef struct {
    uint32_t struct_size;          /* = sizeof(symmicp_posegraph_config), checked */
    int32_t max_iterations;        /* 1 .. 10000, default 100 */
    int32_t reference_node;        /* default 0 */
    int32_t cg_max_iterations;     /* default 0: 6 (n - 1) */
    double max_dist;               /* the distance the information matrices were evaluated at; read when mu is derived */
    double preference_loop_closure;/* default 1.0 */
    double line_process_weight;    /* mu; default 0: derived */
    double edge_prune_threshold;   /* default 0.25 */
    double min_relative_decrease;  /* default 1e-6 */
    double min_increment;          /* default 1e-9 */
    double cg_tolerance;           /* default 1e-10 */
} symmicp_posegraph_config;
typedef struct {
    int32_t status;                /* what the call returned */
    int32_t iterations;            /* linearisations = launches of the iteration kernel */
    int32_t accepted_steps;
    int32_t stop_reason;           /* 1 max_iterations, 2 relative decrease, 3 increment; 0: the call failed */
    int32_t pruned;                /* uncertain edges with l < edge_prune_threshold */
    int32_t cg_iterations;         /* over all iterations */
    double cost_initial, cost_final;
    double mu;
    double lambda_final;           /* lambda after the last iteration's update */
    double grad_max;               /* max |g| at the last linearisation */
} symmicp_posegraph_result;
/* one record per iteration, as the device left it and the host judged it (trace_out) */
typedef struct {
    double cost, cost_trial;       /* F(X), F(X') */
    double model_decrease;         /* d . (lambda d - g) */
    double grad_max, delta_max;    /* max |g|, max |d| */
    double hdiag_max;              /* the largest diagonal entry of H */
    double lambda;                 /* of this iteration's solve */
    double cg_residual;            /* sqrt(r . r / g . g) when the solve stopped */
    int32_t cg_iterations;
    int32_t accepted;              /* 1: F' < F */
    int32_t status;                /* SYMMICP_OK or SYMMICP_ERR_DEGENERATE */
    int32_t reserved;
} symmicp_posegraph_iteration;
/* max_iterations 100, reference_node 0, cg_max_iterations 0, max_dist 0 (the caller sets it), preference_loop_closure 1,
 * line_process_weight 0, edge_prune_threshold 0.25, min_relative_decrease 1e-6, min_increment 1e-9, cg_tolerance 1e-10 */
void symmicp_posegraph_config_default(symmicp_posegraph_config *cfg);
/* poses_in, poses_out [n][16] (they may be the same array); result (required); weight_out [m]: l at the final poses; pruned_out [m]: 1 for
 * a pruned edge; trace_out [max_iterations]: the first result->iterations records are written; the three may be NULL.  Runs on the
 * context's stream and temporary memory. */
int symmicp_ctx_posegraph_optimize(symmicp_ctx *ctx, const double *poses_in, size_t n, const symmicp_pose_edge *edges, size_t m,
                                   const symmicp_posegraph_config *cfg, double *poses_out, symmicp_posegraph_result *result,
                                   double *weight_out, uint8_t *pruned_out, symmicp_posegraph_iteration *trace_out);
/* the same on a context of its own, created on `device` (-1 = current) and destroyed again */
int symmicp_posegraph_optimize(int device, const double *poses_in, size_t n, const symmicp_pose_edge *edges, size_t m,
                               const symmicp_posegraph_config *cfg, double *poses_out, symmicp_posegraph_result *result,
                               double *weight_out, uint8_t *pruned_out, symmicp_posegraph_iteration *trace_out);
/* test entry: one launch of the iteration kernel at the given poses, mu (finite, > 0) and lambda (finite, >= 0), with the solve's
 * cg_tolerance (in (0, 1)) and cg_max_iterations (0: 6 (n - 1)).  Outputs, each may be NULL: e_out [m][6], c_out [m], l_out [m],
 * g_out [n][6], hdiag_out [n][36] (H_ii without lambda), delta_out [n][6] -- the rows of the reference node are zero in the three --
 * and record_out: cost, cost_trial = F(X Exp(d)), the solve's iterations and residual (accepted = 0).
 * SYMMICP_ERR_ARG as for the optimiser (graph, poses, reference_node), and for mu, lambda, cg_tolerance, cg_max_iterations out of range. */
int symmicp_ctx_posegraph_pass(symmicp_ctx *ctx, const double *poses, size_t n, const symmicp_pose_edge *edges, size_t m,
                               int32_t reference_node, double mu, double lambda, double cg_tolerance, int32_t cg_max_iterations,
                               double *e_out, double *c_out, double *l_out, double *g_out, double *hdiag_out, double *delta_out,
                               symmicp_posegraph_iteration *record_out);
/* pure host helpers: e of one edge by the definition above (e6_out = (w, tau); SYMMICP_ERR_ARG for a NULL pointer), and l of an
 * uncertain edge */
int symmicp_posegraph_edge_error(const double Xs16[16], const double Xt16[16], const double T16[16], double e6_out[6]);
double symmicp_posegraph_line_weight(double mu, double c);

/* ---- multi-GPU (new: the reference is single-threaded) ----- */
/* rank 0 creates an id, the application ships it to the other ranks (any channel),
 * then every rank calls comm_init_rank BEFORE set_source.  One RCCL all-reduce of
 * SYMMICP_NSUM doubles per pass. */
int symmicp_comm_get_unique_id(void *out128);
/* the share of the source `rank` of `nranks` owns: rows [begin, begin+count) of the caller's cloud;
 * pure host arithmetic, the same partition symmicp_set_source applies. */
int symmicp_shard_range(size_t n, int nranks, int rank, size_t *begin, size_t *count);
int symmicp_comm_init_rank(symmicp_ctx *ctx, int nranks, int rank, const void *unique_id128);
/* External exchange: with unique_id128 == NULL and nranks > 1 the context is sharded as above but owns no
 * communicator; every pass then ends with THIS RANK's record (symmicp_iter_result.sums).  The application sums the
 * records over the ranks however it likes (MPI, gloo, shared memory, ...) and hands the total back before the next
 * step; all ranks must pass the same 40 doubles so that their solves agree.  (symmicp_align is not available in this
 * mode: it would solve from the local record.) */
int symmicp_set_sums(symmicp_ctx *ctx, const symmicp_sums *total_over_ranks);
/* Ranks of ONE node can also exchange the record through POSIX shared memory instead of RCCL (a 320-byte, purely
 * latency-bound exchange: no collective kernel, no extra launch).  job_name must be the same on all ranks and unique
 * per job (it names the segment /symmicp_<job_name>; rank 0 creates and, on destroy, removes it).  Call it instead of
 * symmicp_comm_init_rank, before symmicp_set_source; everything else (align, step, ...) works as with RCCL. */
int symmicp_comm_init_shm(symmicp_ctx *ctx, int nranks, int rank, const char *job_name);

/* ---- measurement helpers ------------------------------------------------ */
typedef struct {
    double last_pass_ms;       /* HIP-event time of the most recent pass kernel(s), on the ctx stream */
    double sum_pass_ms;        /* accumulated since the last reset */
    int64_t passes;
    double build_ms;           /* target index build (sort + grid + tree) */
    double upload_ms;
    int32_t grid_level;        /* cells per axis = 2^grid_level */
    int32_t tree_levels;
    int64_t pass_blocks;
    int64_t bytes_algorithmic_per_pass;  /* N_s*(48+4+4)+N_t*12 (NN) or N_s*48 (identity) [+24 N_s write-back]
                                            [-12 N_s: PLANE and COLOR read no source normals without write-back and min_normal_dot]
                                            [+20 N_s in COLOR: 4 B of source intensity per point, 16 B of target (gradient, intensity) per pair] */
    /* per-kernel HIP-event time since the last reset (timing mode), slots:
     * 0 k_search_cells, 1 idle gap between cells and walk, 2 k_search_walk, 3 k_accumulate, 4 k_final_reduce,
     * 5 the single pass kernel of the IDENTITY / BRUTE modes (k_pass_identity, or k_nn_brute + k_pass_indexed),
     * 6 the whole pass bracketed by two events (timing mode 1);
     * kernel_launches[7] counts passes that skipped the tree walk and had to be repaired */
    double kernel_ms[8];
    int64_t kernel_launches[8];
    /* timing on: duration of each of the first 8 passes since symmicp_reset_stats (pass 0 = the correspondence pass of
     * symmicp_begin, myicp.cpp:122), and how many passes were timed in all (timing mode 3: a pass that carried events counts, in
     * sum_pass_ms / passes_timed / pass_ms_head, for itself and the up to three passes behind it that carried none) */
    double pass_ms_head[8];
    int64_t passes_timed;
    /* passes that ran inside device-driven runs of iterations (symmicp_align), and those of them that carried the straggler stage
     * (tree walk over a non-empty work list inside the run) */
    int64_t loop_passes, loop_straggler_passes;
    /* first passes run as 64-query packets (kernels_packet.hip): packets whose breadth-first frontier outgrew its LDS slot and that
     * finished depth-first instead (exact either way; 0 on the BASELINE workloads), since symmicp_create */
    int64_t packet_fallbacks;
    /* sharded runs with the library's own RCCL communicator, timing on: HIP-event time spent in the per-pass all-reduce of the record
     * (events on the ctx stream around the collective) and the number of all-reduces that carried events */
    double allreduce_ms;
    int64_t allreduce_timed;
} symmicp_stats;
int symmicp_get_stats(symmicp_ctx *ctx, symmicp_stats *out);
int symmicp_reset_stats(symmicp_ctx *ctx);
/* HIP events on the ctx stream: 0 off, 1 two events bracketing each pass, 2 events around every kernel of a pass, 3 as 1 but only
 * every 4th pass of a device-driven run of iterations carries events and stands for its neighbours in the sums (each record costs ~2.5 us of GPU timeline: two per pass are 13 % of a converged
 * 1M-point iteration; mode 2 is for profiling, not for throughput runs) */
int symmicp_enable_timing(symmicp_ctx *ctx, int on);

/* ---- batched alignment: many small ICP problems in one launch ------------------------------------------------------------------
 * B independent problems of at most SYMMICP_BATCH_MAX_POINTS points per cloud, each run to its end by ONE workgroup: its brute-force
 * search, its rows, its record and its solve never leave the workgroup, and nothing returns to the host before every problem has
 * ended.  Multi-start refinement (one pair, many guesses), many object pairs, keypoint-sized scan pairs.
 *   Clouds      packed [n][3] pools src_xyz / src_nrm [ns_total][3] and tgt_xyz / tgt_nrm [nt_total][3].  Problem b reads the source
 *               rows [src_first, src_first + src_count) and the target rows [tgt_first, tgt_first + tgt_count); the ranges of different
 *               problems may overlap or coincide.  src_nrm may be NULL in PLANE only (with min_normal_dot <= -1), as for
 *               symmicp_set_source: the source normals are zeros then.
 *   Pivot       the mean of the problem's target rows, summed in fp64 in row order, divided by the count and rounded to fp32; reported.
 *   Start       X_0 = guess16 + 16 b (row-major 4x4), or the identity when guess16 is NULL; iters = 0.
 *   Pass k      moves the ORIGINAL source rows by X_k in fp32, unfused: ((m0 x + m1 y) + m2 z) + m3 w, points with w = 1, normals with
 *               w = 0.  Row i pairs with the target row j that minimises (d2, j) over the problem's target rows in the caller's order,
 *               d2 = (dx dx + dy dy) + dz dz in fp32 -- exact brute force, ties to the lowest row.  The gates: the pair is dropped when
 *               max_corr_dist > 0 and d2 > max_corr_dist * max_corr_dist (the fp32 square), then when min_normal_dot > -1 and the moved
 *               source normal . target normal < min_normal_dot.  The mode's record (symmicp_sums: PAPER's, P2P's or PLANE's rows in fp32
 *               about `pivot`, summed in fp64) is formed by the same source the pass kernels of a context use.
 *   Loop        diff = (float)record[33]; diff_initial = the diff of pass 0.  Then symmicp_align's loop:
 *                 while ((fixed_iters || diff > diff_threshold) && iters < max_iters) {
 *                     iters++; if (iters <= 64) diffs[iters - 1] = diff;
 *                     increment = the solve of the record: symmicp_solve's arithmetic (exact conditioning) and acceptance; on failure
 *                                 iters--, status = SYMMICP_ERR_DEGENERATE, stop
 *                     X = increment * X (4x4 product in fp32);  run the next pass with X;  diff = (float)record[33]
 *                     if (eps_rotation > 0 && eps_translation > 0 && !fixed_iters && the increment rotates by less than eps_rotation
 *                         and translates by less than eps_translation) stop
 *                 }
 *   Result      status (SYMMICP_OK or SYMMICP_ERR_DEGENERATE: that problem alone; the call still returns SYMMICP_OK and no other
 *               problem is affected), iters, diff_initial, diff_final, rcond of the last solve (0 if none ran), pivot, transform = the
 *               last X, diffs, and the last pass's record with its pair count (slot 34).
 *   Traces      trace_X [B][max_iters + 1][16] and trace_sums [B][max_iters + 1][40] (each may be NULL): X_k and the record of pass k
 *               for every pass that ran; rows not reached stay zero.
 *   Purity      a problem's outputs are a function of its own rows, guess and the configuration only: bit for bit the same whatever
 *               B, the problem's place in the batch, the other problems, or the run (fixed-order sums, no floating-point atomics).
 * SYMMICP_ERR_ARG, decided on the host before a device is needed: NULL src_xyz, tgt_xyz, tgt_nrm, problems, cfg or out; a wrong
 * struct_size; a mode other than PAPER, P2P and PLANE; B == 0 or B > 2^20; a count of 0; a range outside its pool; max_iters outside
 * 0 .. 1000; a non-finite diff_threshold, max_corr_dist, min_normal_dot, eps_rotation or eps_translation; NULL src_nrm outside PLANE,
 * or together with min_normal_dot > -1; a non-finite coordinate (or normal component) in a row some problem uses.  SYMMICP_ERR_SIZE: a
 * count above SYMMICP_BATCH_MAX_POINTS (the message names the limit): above it the tree search of a context wins.
 * Out of scope, refused or absent: QUIRKS, GICP and COLOR (SYMMICP_ERR_ARG); robust losses, trimming, one-to-one, median and
 * reciprocal rejection, tree search (the configuration has no field for them); sharding one batch over ranks (each rank may run its
 * own).  The ctx form runs on the context's stream and scratch arena: its clouds, index, certificates, options and loop state stay
 * exactly as they were, so it may be called between two symmicp_step calls.  The other form creates a context on `device`
 * (-1 = current) and destroys it again. */
#define SYMMICP_BATCH_MAX_POINTS 4096      /* per cloud of a problem; above it the tree search wins: use a context */
typedef struct { uint32_t src_first, src_count, tgt_first, tgt_count; } symmicp_batch_problem;
typedef struct {
    uint32_t struct_size;         /* = sizeof(symmicp_batch_config), checked */
    int32_t mode;                 /* SYMMICP_MODE_PAPER, _P2P or _PLANE */
    int32_t max_iters;            /* 0 .. 1000; default 10 */
    int32_t fixed_iters;          /* != 0: ignore the threshold (and the eps rule), run exactly max_iters iterations */
    float diff_threshold, max_corr_dist, min_normal_dot, eps_rotation, eps_translation;   /* as symmicp_config */
    int32_t reserved[3];
} symmicp_batch_config;
typedef struct {
    int32_t status, iters;
    float diff_initial, diff_final, rcond;    /* rcond of the last solve */
    float pivot[3];
    float transform[16];
    float diffs[64];
    double pairs;                             /* slot 34 of the last record */
    symmicp_sums sums;                        /* the last pass's record */
} symmicp_batch_result;
void symmicp_batch_config_default(symmicp_batch_config *cfg);      /* PAPER, 10 iterations, threshold 1, every gate and the eps rule off */
int symmicp_ctx_batch_align(symmicp_ctx *ctx, const float *src_xyz, const float *src_nrm, size_t ns_total,
                            const float *tgt_xyz, const float *tgt_nrm, size_t nt_total,
                            const symmicp_batch_problem *problems, const float *guess16, size_t B,
                            const symmicp_batch_config *cfg, symmicp_batch_result *out, float *trace_X, double *trace_sums);
int symmicp_batch_align(int device, const float *src_xyz, const float *src_nrm, size_t ns_total,
                        const float *tgt_xyz, const float *tgt_nrm, size_t nt_total,
                        const symmicp_batch_problem *problems, const float *guess16, size_t B,
                        const symmicp_batch_config *cfg, symmicp_batch_result *out, float *trace_X, double *trace_sums);

/* ---- PCD I/O (replaces pcl::PCDReader use in MyICP::LoadCloud, myicp.cpp:20-31) */
/* returns point count (>=0) or -symmicp_status.  xyz/nrm packed AoS (3 floats per point); pass
 * xyz==NULL to query the count.  nrm may be NULL.  *has_normals reports normal_x/y/z fields. */
long symmicp_pcd_read(const char *path, float *xyz, float *nrm, size_t cap, int *has_normals);
int symmicp_pcd_write(const char *path, const float *xyz, const float *nrm, size_t n, int binary);
/* One scalar intensity per point of a PCD file, in file order.  A field named `intensity` (any scalar type the reader loads):
 * *kind = 1.  Else a field named `rgb` or `rgba`, PCL's packed 0x00RRGGBB in a 4-byte U or F field (an ASCII F value is parsed as
 * a float and its bits are taken): I = (float)(r + g + b) / 765.0f, *kind = 2.  Neither: *kind = 0 and the count returned is 0.
 * Returns the point count (>= 0) or -symmicp_status; out == NULL queries the count; kind may be NULL. */
long symmicp_pcd_read_intensity(const char *path, float *out, size_t cap, int *kind);

#ifdef __cplusplus
}
#endif
#endif /* SYMMICP_H */
