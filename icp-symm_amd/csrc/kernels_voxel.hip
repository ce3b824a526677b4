// kernels_voxel.hip -- voxel-grid downsampling of one cloud (gfx950), the device half of symmicp_ctx_voxel_downsample:
//   k_voxel_keys    linear voxel key per point (x fastest, z slowest: PCL's divb_mul order) + the point's row as value
//   (radix_sort_pairs, kernels_build.hip: stable, so the rows of one voxel stay ascending)
//   k_voxel_heads   1 where a run of equal keys starts                       (then launch_exclusive_scan)
//   k_voxel_first   first sorted position of every voxel, the sentinel n, the voxel count
//   k_voxel_keep    1 for voxels with at least min_points points             (then launch_exclusive_scan)
//   k_voxel_compact (first, count) of the kept voxels, dense in ascending key, and their number
//   k_voxel_mean    one thread per kept voxel: sequential fp32 sums in ascending row order, mean and normalised normal sum
//   k_voxel_of      per sorted position: the output id of the point's voxel (-1: dropped) at the point's row
// The arithmetic is the specification ("Voxel downsampling"; tests/_voxel_ref.py is the same in numpy):
// nothing here is reassociated, fused or approximated.
#include "symmicp_internal.h"
#pragma clang fp contract(off)

namespace symmicp {

__global__ __launch_bounds__(256) void k_voxel_keys(const float *__restrict__ x, const float *__restrict__ y, const float *__restrict__ z,
                                                    uint32_t n, float inv, int lo_x, int lo_y, int lo_z, uint64_t nx, uint64_t ny,
                                                    uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // floorf(v * inv) lies in [lo, hi] (the host checked both ends fit an int): the cell offsets fit uint32, the key fits uint32
    const uint64_t ix = (uint64_t)((int64_t)(int)floorf(x[i] * inv) - lo_x);
    const uint64_t iy = (uint64_t)((int64_t)(int)floorf(y[i] * inv) - lo_y);
    const uint64_t iz = (uint64_t)((int64_t)(int)floorf(z[i] * inv) - lo_z);
    keys[i] = (uint32_t)(ix + nx * (iy + ny * iz));
    vals[i] = i;
}

__global__ __launch_bounds__(256) void k_voxel_heads(const uint32_t *__restrict__ keys, uint32_t n, uint32_t *__restrict__ head)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// vid_excl = the exclusive scan of the heads: position i belongs to voxel vid_excl[i] + head(i) - 1
__global__ __launch_bounds__(256) void k_voxel_first(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ vid_excl, uint32_t n,
                                                     uint32_t *__restrict__ first, uint32_t *__restrict__ m0_out)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    if (h) first[vid_excl[i]] = i;
    if (i == n - 1) {
        const uint32_t m0 = vid_excl[i] + h;
        first[m0] = n;
        *m0_out = m0;
    }
}

__global__ __launch_bounds__(256) void k_voxel_keep(const uint32_t *__restrict__ first, uint32_t m0, uint32_t min_points, uint32_t *__restrict__ keep)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m0) return;
    keep[v] = (first[v + 1] - first[v] >= min_points) ? 1u : 0u;
}

// kid_excl = the exclusive scan of the keep flags: a kept voxel v becomes output kid_excl[v]
__global__ __launch_bounds__(256) void k_voxel_compact(const uint32_t *__restrict__ first, const uint32_t *__restrict__ kid_excl, uint32_t m0,
                                                       uint32_t min_points, uint32_t *__restrict__ kfirst, uint32_t *__restrict__ kcount,
                                                       uint32_t *__restrict__ m_out)
{
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= m0) return;
    const uint32_t cnt = first[v + 1] - first[v];
    const uint32_t kept = cnt >= min_points ? 1u : 0u;
    if (kept) { kfirst[kid_excl[v]] = first[v]; kcount[kid_excl[v]] = cnt; }
    if (v == m0 - 1) *m_out = kid_excl[v] + kept;
}

// One thread per kept voxel: its members are the sorted positions [f, f + c), ascending in the caller's row order (stable sort
// of the iota rows), and are summed in that order, one fp32 add at a time.  Point: sum / (float)c.  Normal: the sum divided by
// its length sqrtf((sx*sx + sy*sy) + sz*sz) when that squared length is > 0, else (0, 0, 0).  hipcc's default fp32 division
// and sqrtf are correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt; note that __fsqrt_rn is NOT, it maps to the native
// approximation unless OCML_BASIC_ROUNDED_OPERATIONS is defined).  The loads of kVoxUnroll members are issued before their
// dependent adds: a heavy voxel is one lane's chain of memory round trips (16 instead of 4 per trip: 200k points in one voxel
// 8.6 -> 7.9 ms, 18.4 -> 14.5 ms with normals).
constexpr int kVoxUnroll = 16;
__global__ __launch_bounds__(256) void k_voxel_mean(CloudSoA s, const uint32_t *__restrict__ kfirst, const uint32_t *__restrict__ kcount,
                                                    uint32_t m, int with_normals, float *__restrict__ xyz_out, float *__restrict__ nrm_out,
                                                    int32_t *__restrict__ count_out)
{
    const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= m) return;
    const uint32_t f = kfirst[o], c = kcount[o], e = f + c;
    float px = 0.f, py = 0.f, pz = 0.f;
    uint32_t j = f;
    for (; j + kVoxUnroll <= e; j += kVoxUnroll) {
        float vx[kVoxUnroll], vy[kVoxUnroll], vz[kVoxUnroll];
#pragma unroll
        for (int k = 0; k < kVoxUnroll; k++) { vx[k] = s.x[j + k]; vy[k] = s.y[j + k]; vz[k] = s.z[j + k]; }
#pragma unroll
        for (int k = 0; k < kVoxUnroll; k++) { px += vx[k]; py += vy[k]; pz += vz[k]; }
    }
    for (; j < e; j++) { px += s.x[j]; py += s.y[j]; pz += s.z[j]; }
    const float fc = (float)c;
    xyz_out[3 * (size_t)o] = px / fc;
    xyz_out[3 * (size_t)o + 1] = py / fc;
    xyz_out[3 * (size_t)o + 2] = pz / fc;
    count_out[o] = (int32_t)c;
    if (!with_normals) return;
    float nx = 0.f, ny = 0.f, nz = 0.f;
    j = f;
    for (; j + kVoxUnroll <= e; j += kVoxUnroll) {
        float vx[kVoxUnroll], vy[kVoxUnroll], vz[kVoxUnroll];
#pragma unroll
        for (int k = 0; k < kVoxUnroll; k++) { vx[k] = s.nx[j + k]; vy[k] = s.ny[j + k]; vz[k] = s.nz[j + k]; }
#pragma unroll
        for (int k = 0; k < kVoxUnroll; k++) { nx += vx[k]; ny += vy[k]; nz += vz[k]; }
    }
    for (; j < e; j++) { nx += s.nx[j]; ny += s.ny[j]; nz += s.nz[j]; }
    const float len2 = (nx * nx + ny * ny) + nz * nz;
    float rx = 0.f, ry = 0.f, rz = 0.f;
    if (len2 > 0.f) {
        const float len = sqrtf(len2);
        rx = nx / len; ry = ny / len; rz = nz / len;
    }
    nrm_out[3 * (size_t)o] = rx;
    nrm_out[3 * (size_t)o + 1] = ry;
    nrm_out[3 * (size_t)o + 2] = rz;
}

__global__ __launch_bounds__(256) void k_voxel_of(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ rows,
                                                  const uint32_t *__restrict__ vid_excl, const uint32_t *__restrict__ first,
                                                  const uint32_t *__restrict__ kid_excl, uint32_t n, uint32_t min_points,
                                                  int32_t *__restrict__ voxel_of)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t h = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    const uint32_t v = vid_excl[i] + h - 1u;
    const bool kept = first[v + 1] - first[v] >= min_points;
    voxel_of[rows[i]] = kept ? (int32_t)kid_excl[v] : -1;
}

static inline uint32_t nblk(uint32_t n) { return (n + 255) / 256; }

void launch_voxel_keys(const CloudSoA &cl, uint32_t n, float inv, const int lo[3], uint64_t nx, uint64_t ny, uint32_t *keys, uint32_t *vals,
                       hipStream_t s)
{
    hipLaunchKernelGGL(k_voxel_keys, dim3(nblk(n)), dim3(256), 0, s, cl.x, cl.y, cl.z, n, inv, lo[0], lo[1], lo[2], nx, ny, keys, vals);
}

void launch_voxel_segments(const uint32_t *keys, uint32_t n, uint32_t *vid_excl, uint32_t *first, uint32_t *scan_ws, uint32_t *m0_out,
                           hipStream_t s)
{
    hipLaunchKernelGGL(k_voxel_heads, dim3(nblk(n)), dim3(256), 0, s, keys, n, vid_excl);
    launch_exclusive_scan(vid_excl, n, scan_ws, s);
    hipLaunchKernelGGL(k_voxel_first, dim3(nblk(n)), dim3(256), 0, s, keys, (const uint32_t *)vid_excl, n, first, m0_out);
}

void launch_voxel_keep(const uint32_t *first, uint32_t m0, uint32_t min_points, uint32_t *kid_excl, uint32_t *scan_ws, uint32_t *kfirst,
                       uint32_t *kcount, uint32_t *m_out, hipStream_t s)
{
    hipLaunchKernelGGL(k_voxel_keep, dim3(nblk(m0)), dim3(256), 0, s, first, m0, min_points, kid_excl);
    launch_exclusive_scan(kid_excl, m0, scan_ws, s);
    hipLaunchKernelGGL(k_voxel_compact, dim3(nblk(m0)), dim3(256), 0, s, first, (const uint32_t *)kid_excl, m0, min_points, kfirst, kcount, m_out);
}

void launch_voxel_mean(const CloudSoA &sorted, const uint32_t *kfirst, const uint32_t *kcount, uint32_t m, int with_normals, float *xyz_out,
                       float *nrm_out, int32_t *count_out, hipStream_t s)
{
    if (m == 0) return;             // (min_points dropped every voxel)
    hipLaunchKernelGGL(k_voxel_mean, dim3(nblk(m)), dim3(256), 0, s, sorted, kfirst, kcount, m, with_normals, xyz_out, nrm_out, count_out);
}

void launch_voxel_of(const uint32_t *keys, const uint32_t *rows, const uint32_t *vid_excl, const uint32_t *first, const uint32_t *kid_excl,
                     uint32_t n, uint32_t min_points, int32_t *voxel_of, hipStream_t s)
{
    hipLaunchKernelGGL(k_voxel_of, dim3(nblk(n)), dim3(256), 0, s, keys, rows, vid_excl, first, kid_excl, n, min_points, voxel_of);
}

}  // namespace symmicp
