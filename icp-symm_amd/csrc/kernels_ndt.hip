// kernels_ndt.hip -- SYMMICP_MODE_NDT on gfx950 (include/symmicp.h, "NDT registration"; DESIGN.md 4, "NDT"):
//   k_ndt_voxels   one thread per voxel with >= min_points points: the fp64 mean and covariance in two sequential passes over its
//                  members (ascending caller row: the stable sort of kernels_voxel.hip), the Jacobi, the inverse covariance's factors
//   k_ndt_compact  the voxels that survived, dense in ascending key
//   k_ndt_insert   the lookup table key -> map row
//   k_pass_ndt     one pass: per source point its 1 or 7 candidate cells, per (point, voxel) item three PLANE rows into the record
//   k_ndt_corr     symmicp_get_correspondences: the map row of every point's own cell
// The arithmetic is the specification (tests/_ndt_ref.py is the same in numpy): nothing here is reassociated, fused or approximated.
// No floating-point atomics: two runs give the same bits.
#include "symmicp_internal.h"
#include "device_common.h"
#include "pass_rows.h"
#include "ndt_core.h"
#pragma clang fp contract(off)

namespace symmicp {

// A heavy voxel is one lane's chain of loads, as in k_voxel_mean ("NDT")
__global__ __launch_bounds__(256) void k_ndt_voxels(CloudSoA s, const uint32_t *__restrict__ skeys, const uint32_t *__restrict__ kfirst,
                                                    const uint32_t *__restrict__ kcount, uint32_t m, float eig_ratio, float4 *__restrict__ rec,
                                                    double *__restrict__ cov, uint32_t *__restrict__ key, uint32_t *__restrict__ valid)
{
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= m) return;
    const uint32_t f = kfirst[o], c = kcount[o], e = f + c;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t j = f; j < e; j++) { sx += (double)s.x[j]; sy += (double)s.y[j]; sz += (double)s.z[j]; }
    const double dc = (double)c;
    const double mx = sx / dc, my = sy / dc, mz = sz / dc;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (uint32_t j = f; j < e; j++) {
        const double dx = (double)s.x[j] - mx, dy = (double)s.y[j] - my, dz = (double)s.z[j] - mz;
        c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    const double dn = (double)(c - 1u);      // (min_points >= 3)
    c00 /= dn; c01 /= dn; c02 /= dn; c11 /= dn; c12 /= dn; c22 /= dn;
    double lam[3], vec[3][3];
    ndt_eig3(c00, c01, c02, c11, c12, c22, lam, vec);
    const double lmax = lam[2];
    const bool ok = isfinite(lmax) && lmax > 0.0;
    valid[o] = ok ? 1u : 0u;
    key[o] = skeys[f];
    double *cv = cov + 6 * (size_t)o;
    cv[0] = c00; cv[1] = c01; cv[2] = c02; cv[3] = c11; cv[4] = c12; cv[5] = c22;
    const double floor_l = (double)eig_ratio * lmax;
    float4 *r = rec + 4 * (size_t)o;
    r[0] = make_float4((float)mx, (float)my, (float)mz, __int_as_float((int)c));
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double l = lam[k] > floor_l ? lam[k] : floor_l;      // max(lambda, eig_ratio * lambda_max)
        r[1 + k] = make_float4((float)vec[k][0], (float)vec[k][1], (float)vec[k][2], (float)(1.0 / l));
    }
}

__global__ __launch_bounds__(256) void k_ndt_compact(const float4 *__restrict__ rec, const double *__restrict__ cov, const uint32_t *__restrict__ key,
                                                     const uint32_t *__restrict__ valid, const uint32_t *__restrict__ pos, uint32_t m,
                                                     float4 *__restrict__ rec_out, double *__restrict__ cov_out, uint32_t *__restrict__ key_out)
{
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= m || !valid[o]) return;
    const size_t d = pos[o];
#pragma unroll
    for (int k = 0; k < 4; k++) rec_out[4 * d + k] = rec[4 * (size_t)o + k];
#pragma unroll
    for (int k = 0; k < 6; k++) cov_out[6 * d + k] = cov[6 * (size_t)o + k];
    key_out[d] = key[o];
}

__device__ __forceinline__ uint32_t ndt_hash(uint32_t key, uint32_t shift) { return (key * 0x9E3779B1u) >> shift; }

// Keys are distinct and the table is at most half full: every insert finds an empty entry within `mask + 1` probes.  Which entry a key
// lands in depends on the order of the inserts; what a lookup returns does not.
__global__ __launch_bounds__(256) void k_ndt_insert(const uint32_t *__restrict__ key, uint32_t m, unsigned long long *__restrict__ table,
                                                    uint32_t shift, uint32_t mask)
{
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= m) return;
    const uint32_t k = key[o];
    const unsigned long long entry = ((unsigned long long)k << 32) | (unsigned long long)(o + 1u);
    uint32_t h = ndt_hash(k, shift) & mask;
    for (uint32_t t = 0; t <= mask; t++) {
        if (atomicCAS(table + h, 0ull, entry) == 0ull) return;
        h = (h + 1u) & mask;
    }
}

// the map row of cell `key`, or -1: one 8-byte load per probe, an empty entry ends the probe
__device__ __forceinline__ int32_t ndt_find(const NdtGrid &g, uint32_t key)
{
    uint32_t h = ndt_hash(key, g.shift) & g.mask;
    for (uint32_t t = 0; t <= g.mask; t++) {
        const unsigned long long e = g.table[h];
        if (e == 0ull) return -1;
        if ((uint32_t)(e >> 32) == key) return (int32_t)((uint32_t)e - 1u);
        h = (h + 1u) & g.mask;
    }
    return -1;
}

// the map row of the cell (cx, cy, cz) (floats holding integers), or -1 when it lies outside the box or holds no voxel
__device__ __forceinline__ int32_t ndt_cell_row(const NdtGrid &g, float cx, float cy, float cz)
{
    // (a NaN or infinite coordinate fails these compares: no item)
    if (!(cx >= g.lo[0] && cx <= g.hi[0] && cy >= g.lo[1] && cy <= g.hi[1] && cz >= g.lo[2] && cz <= g.hi[2])) return -1;
    const uint64_t ix = (uint64_t)((int64_t)(int)cx - g.lo_i[0]);
    const uint64_t iy = (uint64_t)((int64_t)(int)cy - g.lo_i[1]);
    const uint64_t iz = (uint64_t)((int64_t)(int)cz - g.lo_i[2]);
    return ndt_find(g, (uint32_t)(ix + (uint64_t)g.nx * (iy + (uint64_t)g.ny * iz)));
}

// One source point per thread per trip.  Streaming: 12 B per point; per item one table probe (8 B, mostly one) and the voxel's record as
// four 16-byte loads -- a Morton-sorted share keeps neighbouring lanes in the same few voxels, so the records come out of L1 / L2 --
// and 84 fp64 FMAs (three acc_row of 28).
__global__ __launch_bounds__(kPassThreads) void k_pass_ndt(NdtPassArgs a)
{
    AccN<kNAccW> acc; acc_zero(acc);
    const uint32_t stride = gridDim.x * blockDim.x;
    const int ncand = a.neighbors == 7 ? 7 : 1;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const float x = a.x[i], y = a.y[i], z = a.z[i];
        const float yx = xf_row(a.X.m + 0, x, y, z, 1.0f), yy = xf_row(a.X.m + 4, x, y, z, 1.0f), yz = xf_row(a.X.m + 8, x, y, z, 1.0f);
        const float gx = floorf(yx * a.g.inv), gy = floorf(yy * a.g.inv), gz = floorf(yz * a.g.inv);
        const float px = yx - a.pivot[0], py = yy - a.pivot[1], pz = yz - a.pivot[2];
        for (int k = 0; k < ncand; k++) {
            // k = 0: the point's own cell; 1, 2: x + 1, x - 1; 3, 4: y; 5, 6: z
            float cx = gx, cy = gy, cz = gz;
            if (k) {
                const float sgn = (k & 1) ? 1.0f : -1.0f;
                const int axis = (k - 1) >> 1;
                if (axis == 0) cx += sgn; else if (axis == 1) cy += sgn; else cz += sgn;
            }
            const int32_t row = ndt_cell_row(a.g, cx, cy, cz);
            if (row < 0) continue;
            const float4 *r = a.g.rec + 4 * (size_t)row;
            const float4 r0 = r[0], l0 = r[1], l1 = r[2], l2 = r[3];
            const float mx = r0.x - a.pivot[0], my = r0.y - a.pivot[1], mz = r0.z - a.pivot[2];
            const float dx = px - mx, dy = py - my, dz = pz - mz;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if (a.max_d2 > 0.0f && d2 > a.max_d2) continue;
            const float c0 = (dx * l0.x + dy * l0.y) + dz * l0.z;
            const float c1 = (dx * l1.x + dy * l1.y) + dz * l1.z;
            const float c2 = (dx * l2.x + dy * l2.y) + dz * l2.z;
            const float mm = ((l0.w * c0) * c0 + (l1.w * c1) * c1) + (l2.w * c2) * c2;
            const double w = (double)ndt_weight(-(a.h * mm));
            {
                const double v[6] = {(double)(py * l0.z - pz * l0.y), (double)(pz * l0.x - px * l0.z), (double)(px * l0.y - py * l0.x),
                                     (double)l0.x, (double)l0.y, (double)l0.z};
                acc_row(acc, v, (double)c0, w * (double)l0.w);
            }
            {
                const double v[6] = {(double)(py * l1.z - pz * l1.y), (double)(pz * l1.x - px * l1.z), (double)(px * l1.y - py * l1.x),
                                     (double)l1.x, (double)l1.y, (double)l1.z};
                acc_row(acc, v, (double)c1, w * (double)l1.w);
            }
            {
                const double v[6] = {(double)(py * l2.z - pz * l2.y), (double)(pz * l2.x - px * l2.z), (double)(px * l2.y - py * l2.x),
                                     (double)l2.x, (double)l2.y, (double)l2.z};
                acc_row(acc, v, (double)c2, w * (double)l2.w);
            }
            acc_pair_sums(acc, px, py, pz, mx, my, mz, d2, w);
        }
    }
    acc_block_reduce_store(acc, a.partials, blockIdx.x);      // (pass_rows.h: the weighted record, as the pass kernels sum it)
}

__global__ __launch_bounds__(256) void k_ndt_corr(NdtPassArgs a, const uint32_t *__restrict__ order, int32_t *__restrict__ idx_out,
                                                  float *__restrict__ d2_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const float x = a.x[i], y = a.y[i], z = a.z[i];
    const float yx = xf_row(a.X.m + 0, x, y, z, 1.0f), yy = xf_row(a.X.m + 4, x, y, z, 1.0f), yz = xf_row(a.X.m + 8, x, y, z, 1.0f);
    const int32_t row = ndt_cell_row(a.g, floorf(yx * a.g.inv), floorf(yy * a.g.inv), floorf(yz * a.g.inv));
    float d2 = 0.0f;
    if (row >= 0) {
        const float4 r0 = a.g.rec[4 * (size_t)row];
        const float dx = (yx - a.pivot[0]) - (r0.x - a.pivot[0]), dy = (yy - a.pivot[1]) - (r0.y - a.pivot[1]),
                    dz = (yz - a.pivot[2]) - (r0.z - a.pivot[2]);
        d2 = (dx * dx + dy * dy) + dz * dz;
    }
    const size_t at = order ? order[i] : i;
    idx_out[at] = row;
    d2_out[at] = d2;
}

static inline uint32_t nblk(uint32_t n) { return (n + 255) / 256; }

void launch_ndt_voxels(const CloudSoA &sorted, const uint32_t *skeys, const uint32_t *kfirst, const uint32_t *kcount, uint32_t m, float eig_ratio,
                       float4 *rec, double *cov, uint32_t *key, uint32_t *valid, hipStream_t s)
{
    if (m == 0) return;
    hipLaunchKernelGGL(k_ndt_voxels, dim3(nblk(m)), dim3(256), 0, s, sorted, skeys, kfirst, kcount, m, eig_ratio, rec, cov, key, valid);
}

void launch_ndt_compact(const float4 *rec, const double *cov, const uint32_t *key, const uint32_t *valid, const uint32_t *pos, uint32_t m,
                        float4 *rec_out, double *cov_out, uint32_t *key_out, hipStream_t s)
{
    if (m == 0) return;
    hipLaunchKernelGGL(k_ndt_compact, dim3(nblk(m)), dim3(256), 0, s, rec, cov, key, valid, pos, m, rec_out, cov_out, key_out);
}

void launch_ndt_insert(const uint32_t *key, uint32_t m, unsigned long long *table, uint32_t shift, uint32_t mask, hipStream_t s)
{
    if (m == 0) return;
    hipLaunchKernelGGL(k_ndt_insert, dim3(nblk(m)), dim3(256), 0, s, key, m, table, shift, mask);
}

void launch_pass_ndt(const NdtPassArgs &a, int blocks, hipStream_t s)
{
    hipLaunchKernelGGL(k_pass_ndt, dim3(blocks), dim3(kPassThreads), 0, s, a);
}

void launch_ndt_corr(const NdtPassArgs &a, const uint32_t *order, int32_t *idx_out, float *d2_out, hipStream_t s)
{
    if (a.n == 0) return;
    hipLaunchKernelGGL(k_ndt_corr, dim3(nblk(a.n)), dim3(256), 0, s, a, order, idx_out, d2_out);
}

}  // namespace symmicp
