// posegraph_core.h -- the fp64 arithmetic of the pose-graph optimiser that the host and the device share (include/symmicp.h,
// "multiway registration", has the definitions; tests/_posegraph_ref.py restates them in numpy): the edge error and its log, the
// exponential of the update, the line-process weight.  One source for symmicp_posegraph_edge_error and for kernels_posegraph.hip.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define PG_HD __host__ __device__ __forceinline__
#else
#define PG_HD inline
#endif

namespace symmicp {
namespace pg {

constexpr double kSmall2 = 1e-8;      // the series of log and exp below this squared size

// E = X_t^-1 X_s T^-1 from the top three rows of X_s, X_t (row-major 3x4) and T = (RT row-major 3x3, tT): RE row-major, tE
PG_HD void edge_E(const double *Xs, const double *Xt, const double *RT, const double *tT, double *RE, double *tE)
{
    double A[9], a[3];      // A = R_t^T R_s, a = R_t^T (t_s - t_t)
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) A[3 * i + j] = (Xt[i] * Xs[j] + Xt[4 + i] * Xs[4 + j]) + Xt[8 + i] * Xs[8 + j];
        a[i] = (Xt[i] * (Xs[3] - Xt[3]) + Xt[4 + i] * (Xs[7] - Xt[7])) + Xt[8 + i] * (Xs[11] - Xt[11]);
    }
    // T^-1 = (RT^T, -RT^T tT): RE = A RT^T, tE = a - RE tT
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) RE[3 * i + j] = (A[3 * i] * RT[3 * j] + A[3 * i + 1] * RT[3 * j + 1]) + A[3 * i + 2] * RT[3 * j + 2];
    }
#pragma unroll
    for (int i = 0; i < 3; i++) tE[i] = a[i] - ((RE[3 * i] * tT[0] + RE[3 * i + 1] * tT[1]) + RE[3 * i + 2] * tT[2]);
}

// the rotation vector of R (row-major), angle in [0, pi]
PG_HD void log_rot(const double *R, double *w)
{
    const double v[3] = {0.5 * (R[7] - R[5]), 0.5 * (R[2] - R[6]), 0.5 * (R[3] - R[1])};
    double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    c = c > 1.0 ? 1.0 : (c < -1.0 ? -1.0 : c);
    const double s2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (s2 >= kSmall2) {
        const double s = sqrt(s2), k = atan2(s, c) / s;
        w[0] = v[0] * k; w[1] = v[1] * k; w[2] = v[2] * k;
        return;
    }
    if (c > 0.0) {
        const double k = (1.0 + s2 / 6.0) + 3.0 * (s2 * s2) / 40.0;
        w[0] = v[0] * k; w[1] = v[1] * k; w[2] = v[2] * k;
        return;
    }
    const double th = atan2(sqrt(s2), c);
    const double d[3] = {R[0], R[4], R[8]};
    int i = 0;
    if (d[1] > d[i]) i = 1;
    if (d[2] > d[i]) i = 2;
    double a[3];
    const double q = (d[i] - c) / (1.0 - c);
    a[i] = sqrt(q > 0.0 ? q : 0.0);
    for (int j = 0; j < 3; j++)
        if (j != i) a[j] = (R[3 * i + j] + R[3 * j + i]) / ((2.0 * (1.0 - c)) * a[i]);
    const double sg = ((a[0] * v[0] + a[1] * v[1]) + a[2] * v[2]) < 0.0 ? -1.0 : 1.0;
    w[0] = th * (sg * a[0]); w[1] = th * (sg * a[1]); w[2] = th * (sg * a[2]);
}

// exp([w]x), row-major
PG_HD void exp_rot(const double *w, double *R)
{
    const double t2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    double A, B;
    if (t2 < kSmall2) {
        A = (1.0 - t2 / 6.0) + (t2 * t2) / 120.0;
        B = (0.5 - t2 / 24.0) + (t2 * t2) / 720.0;
    } else {
        const double t = sqrt(t2);
        A = sin(t) / t;
        B = (1.0 - cos(t)) / t2;
    }
    // [w]x^2 = w w^T - t2 I
    R[0] = 1.0 + B * (w[0] * w[0] - t2); R[1] = B * (w[0] * w[1]) - A * w[2]; R[2] = B * (w[0] * w[2]) + A * w[1];
    R[3] = B * (w[0] * w[1]) + A * w[2]; R[4] = 1.0 + B * (w[1] * w[1] - t2); R[5] = B * (w[1] * w[2]) - A * w[0];
    R[6] = B * (w[0] * w[2]) - A * w[1]; R[7] = B * (w[1] * w[2]) + A * w[0]; R[8] = 1.0 + B * (w[2] * w[2] - t2);
}

// X' = X Exp(d) on the top three rows (row-major 3x4), d = (w, tau)
PG_HD void retract(const double *X, const double *d, double *Xn)
{
    double R[9];
    exp_rot(d, R);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Xn[4 * i + j] = (X[4 * i] * R[j] + X[4 * i + 1] * R[3 + j]) + X[4 * i + 2] * R[6 + j];
        Xn[4 * i + 3] = ((X[4 * i] * d[3] + X[4 * i + 1] * d[4]) + X[4 * i + 2] * d[5]) + X[4 * i + 3];
    }
}

PG_HD double line_weight(double mu, double c)
{
    const double t = mu / (mu + c);
    return t * t;
}

// position of (i, j), i <= j, in the row-major upper triangle of a 6x6
PG_HD constexpr int tri(int i, int j) { return i <= j ? i * 6 - (i * (i - 1)) / 2 + (j - i) : j * 6 - (j * (j - 1)) / 2 + (i - j); }

}  // namespace pg
}  // namespace symmicp
