// pair_search.h -- the exact nearest neighbour of a query through the target's cell table, and the certificates that let later
// passes skip the search: cells_tile (one tile of 256 queries) and what it is made of.
//
// Included by kernels_search.hip (k_search_cells: tile = block) and kernels_pass.hip (k_pass_fused: the queries its streaming phase
// could not certify; k_pass_certified: the certificates alone).  Force-inlined, like pass_rows.h and oct_walk.h.
//
//   phase 0: the pair found by the previous pass bounds the search (temporal coherence);
//   phase 1: the 27 Morton cells around the query in the dense cell table ("grid"),
//            skipping cells farther than the current best;
//   phase 2: only if phase 1 cannot prove its answer: stackless pre-order walk of the
//            implicit 8-ary box tree ("linear BVH"), pruned by the current best (k_search_walk).
// Result = argmin over ALL target points of (d2, original row), identical to brute force.
//
// fp32 expressions here must stay UNFUSED (the including file is compiled with -ffp-contract=off) and keep the association
// written: the CPU oracle uses the same expressions, so nearest-neighbour choices compare bit for bit.
//
// ---------------------------------------------------------------------------
// cells_tile: the common case of a pass, load-balanced at (query, cell) granularity.
//   phase 1  thread = query (plan_query): transform, previous-pair bound, the <= 3x3x3 cells its ball overlaps, and which of
//            them can still hold something not farther than the bound.  Each surviving (query, cell) pair becomes
//            a 13-bit work item in LDS (block-wide prefix sum gives the slots).  Queries without a previous pair or
//            with a wider ball go to the work list of the tree-walk kernels.
//   phase 2  thread = work item (scan_round): one cell range, its points four at a time, result merged per query with an LDS
//            64-bit atomicMin on (d2 bits << 32 | row)  -- min is order independent, ties resolve to the lowest row.
//   phase 3  thread = query (store_pair): store the pair.
// A wave's cost is now the largest single CELL in it, not the largest sum over a query's cells, and queries with 27
// cells no longer drag their whole wave through 27 steps.
//
// Pair certificates.  The search ball is padded by D = kSlackFrac * h beyond the previous pair's distance, so after
// the scan every target point other than the winner is known to be at least L = min(second-nearest scanned, bound + D)
// away from the query position p_ref (the "clear radius", stored in PassArgs::cert[i].w; 0 = no certificate).  If the
// query later sits at p with |p - p_ref| = delta, any other point is >= L - delta away from it, so while the winner's
// current distance d1' satisfies d1' + delta < L the nearest neighbour is provably the same point and the scan is
// skipped; only the distance is refreshed (cert_holds).  Once ICP has converged almost every pair is certified and the kernel is
// little more than phase 1.  Margins: every fp32 distance here is good to ~2.5e-7 relative (three differences, three
// squares, two sums, one 1-ulp root), so with D(p,x) >= second (1 - 2.5e-7) - delta (1 + 2.5e-7) for every other point x
// the test (d1' + delta) (1 + 2e-6) < second (1 - 1e-6) leaves D(p,x) > D(p,winner) (1 + 2e-6): the fp32 comparison the
// oracle makes cannot come out the other way (it needs 3.5e-7).  Bounds that come from cell faces (lim) carry the
// grid's own absolute margin and keep 1e-5.  Pairs whose two nearest points are closer together than that - a few
// dozen per million - have no certificate and are searched again in every pass.
// ---------------------------------------------------------------------------
// Neighbourhood certificates.  The single certificate above has only the room between the two nearest points, L - d1; while an
// alignment still drifts (the scan-like pair keeps moving by a fraction of its point spacing for a dozen passes) that room is used
// up within a pass or two and the query is scanned again, and a pair whose two nearest points are (nearly) equally far can never be
// certified at all -- at convergence the transform still jitters in its last bits, and ~70 pairs per million fail in every pass.
// So a scan also keeps the whole neighbourhood it saw: S = every target point closer to p_ref than a radius T <= lim, if these are
// at most 8.  Every point outside S is then >= T from p_ref, and while
//     min over S of d(p, s) + delta < T
// the nearest neighbour of p is a member of S: decided by the same fp32 (d2, row) comparison brute force makes, over <= 8 gathers
// instead of a scan.  The room is now T - d1, several times L - d1.  Stored per pair: the sorted positions of S (PassArgs::certk,
// 8 words, 0xFFFFFFFF: empty slot; the winner is one of them) and (T, hint) in PassArgs::hoodr.  Bit 0 of cert.w says that they are
// valid, so every writer of a certificate invalidates them by writing an even word (cert_word).  A successful test moves the
// reference to the current position: T <- T - delta and a fresh single certificate L = min(second nearest of S, T), exact bounds.
// T follows the local point spacing: a scan counts ALL points within its T, kept or not, and leaves hint = T (6.5 / count)^0.4 for the
// pair's next scan (the count grows with T^2 on a surface, T^3 in a noisy slab); a first scan starts from 2 x the previous pair's
// distance.
#pragma once
#include "symmicp_internal.h"
#include "device_common.h"
#include "oct_walk.h"        // Best
#pragma clang fp contract(off)

namespace symmicp {

__device__ __forceinline__ uint2 cell_range(const TargetIndex &ix, uint32_t morton)
{
    const uint32_t blk = ix.ctop[morton >> 9];
    if (blk == 0xFFFFFFFFu) return make_uint2(0u, 0u);
    return ix.cells[(size_t)blk * 512u + (morton & 511u)];
}

__device__ __forceinline__ uint32_t spread3(uint32_t v)
{
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// squared gap (minus the safety margin) between the query coordinate and the cell [lo, lo+h) on one axis
__device__ __forceinline__ float axis_gap2(float p, float origin, int c, float h, float margin)
{
    const float lo = origin + (float)c * h;
    const float g = fmaxf(fmaxf(lo - p, p - (lo + h)) - margin, 0.0f);
    return g * g;
}

#ifndef SLACK_FRAC
#define SLACK_FRAC 0.0625f
#endif
// (with the grid at ~4 points per cell: 0.5 / 0.25 / 0.125 / 0.0625 / 0.031 / 0.016 of a cell edge give pass 3 of the 1M surface pair in
// 0.240 / 0.178 / 0.153 / 0.139 / 0.135 / 0.128 ms; the 8M scan pair holds 2 780 iter/s down to 0.0625 and drops to 2 645 / 2 543 below:
// its settling passes want some room.  At ~1 point per cell, rounds 1-2, 0.125 .. 1.0 were within noise.)
constexpr float kSlackFrac = SLACK_FRAC;
constexpr int kHoodSlots = 8;            // |S| <= 8, the winner included
constexpr uint32_t kHoodNone = 0xFFFFFFFFu;

// The certificate test, single (L = the clear radius) or neighbourhood (L = T): the winner at squared distance d2 from the query, the
// query m2 = delta^2 from the certificate's reference; see the margins above.  1-ulp roots, inside the margin.  L <= 0: no
// certificate, never holds.  ONE definition: every kernel has to take the same decision for the same pair.
__device__ __forceinline__ bool cert_holds(float d2, float m2, float L)
{
    return (__builtin_amdgcn_sqrtf(d2) + __builtin_amdgcn_sqrtf(m2)) * 1.000002f < L;
}

// cert.w for clear radius L (> 0; 0: none) and the neighbourhood flag: never above L
__device__ __forceinline__ float cert_word(float L, bool hood)
{
    const uint32_t u = __float_as_uint(L);
    if (!(L > 0.0f)) return hood ? __uint_as_float(0xBF800001u) : 0.0f;      // -1 with the flag: neighbourhood only
    return __uint_as_float(hood ? ((u - 1u) | 1u) : (u & ~1u));
}

// Neighbourhood test of pair i (its single certificate has failed or does not exist).  In: the query's position, delta^2 = m2 to the
// reference, the current winner (sorted position, d2, row).  True: the nearest neighbour is provably a member of S; pos_w / d2w are
// the winner's, and everything the change needs is stored (position, record copy, moved reference).
// hood_test_set: the same with the pair's set (w0, w1 = certk[2 i], certk[2 i + 1]) and radius (T = hoodr[i].x) already loaded -- a caller
// that requests them together with everything else addressed by i saves a round trip (k_pass_certified).
__device__ __forceinline__ bool hood_test_set(const PassArgs &a, const TargetIndex &ix, uint32_t i, float px, float py, float pz, float m2,
                                              int32_t pos_a, float d2a, int32_t rowa, const uint4 &w0, const uint4 &w1, const float T,
                                              int32_t &pos_w, float &d2w)
{
    const uint32_t cand[kHoodSlots] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    float4 q[kHoodSlots];
#pragma unroll
    for (int k = 0; k < kHoodSlots; k++) q[k] = ix.tq[min(cand[k], ix.n - 1u)];       // all gathers in flight at once
    unsigned long long kw = ((unsigned long long)__float_as_uint(d2a) << 32) | (unsigned long long)(uint32_t)rowa;
    uint32_t sec = 0x7f800000u;              // d2 bits of the second nearest of S
    pos_w = pos_a;
#pragma unroll
    for (int k = 0; k < kHoodSlots; k++) {
        const float d2 = dist2(px, py, pz, q[k].x, q[k].y, q[k].z);
        if (cand[k] < ix.n && cand[k] != (uint32_t)pos_a && d2 == d2) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned long long)(uint32_t)__float_as_int(q[k].w);
            if (key < kw) { sec = (uint32_t)(kw >> 32); kw = key; pos_w = (int32_t)cand[k]; }
            else sec = min(sec, __float_as_uint(d2));
        }
    }
    d2w = __uint_as_float((uint32_t)(kw >> 32));
    const float dl = __builtin_amdgcn_sqrtf(m2);
    if (!cert_holds(d2w, m2, T)) return false;
    if (pos_w != pos_a) {
        a.pos_out[i] = pos_w;
        store_pair_record(a, ix, i, pos_w);
    }
    // move the reference to p: everything outside S is >= T - delta from here
    const float d1 = sqrtf(d2w) * 1.000001f;
    const float Tn = (T - dl * 1.000001f) * 0.999999f;
    const float L = fminf(sqrtf(__uint_as_float(sec)) * 0.999999f, Tn);
    if (Tn > d1 * 1.001f) {
        a.cert[i] = make_float4(px, py, pz, cert_word((L > d1) ? L : 0.0f, true));
        a.hoodr[i].x = Tn;
    } else if (pos_w != pos_a) {
        a.cert[i].w = cert_word(0.0f, true);       // the moved radius would leave no room: reference and T stay, the old single certificate goes
    }
    return true;
}

__device__ __forceinline__ bool hood_test(const PassArgs &a, const TargetIndex &ix, uint32_t i, float px, float py, float pz, float m2,
                                          int32_t pos_a, float d2a, int32_t rowa, int32_t &pos_w, float &d2w)
{
    const uint4 w0 = a.certk[2 * (size_t)i], w1 = a.certk[2 * (size_t)i + 1];
    const float T = a.hoodr[i].x;
    return hood_test_set(a, ix, i, px, py, pz, m2, pos_a, d2a, rowa, w0, w1, T, pos_w, d2w);
}

// ---------------------------------------------------------------------------
// cells_tile and its phases
// ---------------------------------------------------------------------------
// What a query (a thread of the tile) carries from phase to phase
struct CellQuery {
    Best b;                    // the best pair so far: the previous pass's at first
    uint32_t mask;             // cells of this query to scan this round, bit = kx + 3*ky + 9*kz
    uint32_t mask_rest;        // probe: the other cells of the 3x3x3 block, scanned only if the 2x2x2 block cannot prove its best
    float lim, lim_full;       // everything outside the scanned cells is at least this far from the query
    float reach;               // T of the neighbourhood this scan collects (0: none)
    // handed to the walk / bounded scan / probe / not certified / settled by its neighbourhood.  (int, not bool: the struct travels by
    // value, a bool in it is a byte, and the compiler then carries the five as 8-bit values in vector registers through the scan rounds;
    // as ints they end up as lane masks in scalar registers, like the locals they replace.  k_pass_fused<false> has 96 registers.)
    int defer, searched, probe, uncert, hood_ok;
};

// The tile's LDS arrays as the phases address them (cells_tile declares them one by one: their order fixes the LDS offsets)
struct TileLds {
    float *px, *py, *pz;
    unsigned long long *key;
    uint32_t *second;
    int32_t *pos;
    uint32_t *cell0;
    uint16_t *items;
    uint32_t *wsum, *anyw, *nmore;
    float *reach;
    uint32_t *hcnt, *qi;
};

constexpr int kTileItems = kPassThreads * 27;

// The previous pair bounds the scan: the ball of the bound, padded by kSlackFrac * h, and the cells it reaches.  If they are at most
// 3x3x3 the query scans those of them that reach into the ball (searched); else it stays deferred.  cell0: the block's first cell.
// (The phases take and return the query BY VALUE: it then lives in registers from the first compiler pass on, as the locals it replaces did.)
__device__ __forceinline__ CellQuery plan_bounded_scan(const TargetIndex &ix, float px, float py, float pz, CellQuery c, uint32_t &cell0)
{
    const float inf = __int_as_float(0x7f800000);
    const float margin = 2e-3f * ix.h;
    const float gmax = (float)ix.gdim;
    // any rb >= sqrt(d2) is valid: the hardware square root (1 ulp) with a relative pad
    const float rb = __builtin_amdgcn_sqrtf(c.b.d2) * 1.00001f;
    c.lim = rb + kSlackFrac * ix.h;
    const float r = c.lim + margin;
    const float lx = (px - r - ix.ox) * ix.inv_h, hx = (px + r - ix.ox) * ix.inv_h;
    const float ly = (py - r - ix.oy) * ix.inv_h, hy = (py + r - ix.oy) * ix.inv_h;
    const float lz = (pz - r - ix.oz) * ix.inv_h, hz = (pz + r - ix.oz) * ix.inv_h;
    const int x0 = (int)floorf(fminf(fmaxf(lx, 0.0f), gmax - 1.0f)), x1 = (int)floorf(fminf(fmaxf(hx, 0.0f), gmax - 1.0f));
    const int y0 = (int)floorf(fminf(fmaxf(ly, 0.0f), gmax - 1.0f)), y1 = (int)floorf(fminf(fmaxf(hy, 0.0f), gmax - 1.0f));
    const int z0 = (int)floorf(fminf(fmaxf(lz, 0.0f), gmax - 1.0f)), z1 = (int)floorf(fminf(fmaxf(hz, 0.0f), gmax - 1.0f));
    const int nx = x1 - x0, ny = y1 - y0, nz = z1 - z0;      // extra cells per axis
    if (nx <= 2 && ny <= 2 && nz <= 2) {
        c.defer = false;
        c.searched = true;
        const float thr2 = c.lim * c.lim * 1.00001f;             // keep every cell that reaches into the padded ball
        float gx[3], gy[3], gz[3];
        uint32_t mask = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            gx[k] = (k <= nx) ? axis_gap2(px, ix.ox, x0 + k, ix.h, margin) : inf;
            gy[k] = (k <= ny) ? axis_gap2(py, ix.oy, y0 + k, ix.h, margin) : inf;
            gz[k] = (k <= nz) ? axis_gap2(pz, ix.oz, z0 + k, ix.h, margin) : inf;
        }
#pragma unroll
        for (int kz = 0; kz < 3; kz++)
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    const float g2 = (gx[kx] + gy[ky]) + gz[kz];
                    if (g2 <= thr2) mask |= 1u << (kx + 3 * ky + 9 * kz);
                }
        c.mask = mask;
        cell0 = (uint32_t)x0 | ((uint32_t)y0 << 10) | ((uint32_t)z0 << 20);
        c.reach = rb;            // (marks a scan; the radius is chosen by hood_radius)
    }
    return c;
}

// The previous pair is too far to bound the scan (the cloud has just moved a lot).  Probe the 27 cells
// around the query instead: if the best point found there is closer than the nearest outer face of that
// block, nothing outside the block can beat it and the answer is exact; otherwise it still tightens the
// bound the tree walk starts from.  Only queries inside the grid probe.
__device__ __forceinline__ CellQuery plan_probe(const TargetIndex &ix, float px, float py, float pz, CellQuery c, uint32_t &cell0)
{
    const float inf = __int_as_float(0x7f800000);
    const float fx = (px - ix.ox) * ix.inv_h, fy = (py - ix.oy) * ix.inv_h, fz = (pz - ix.oz) * ix.inv_h;
    const float gmax = (float)ix.gdim;
    if (fx >= 0.0f && fy >= 0.0f && fz >= 0.0f && fx < gmax && fy < gmax && fz < gmax) {
        const int cx = (int)fx, cy = (int)fy, cz = (int)fz;
        const int x0 = max(cx - 1, 0), y0 = max(cy - 1, 0), z0 = max(cz - 1, 0);
        const int x1 = min(cx + 1, ix.gdim - 1), y1 = min(cy + 1, ix.gdim - 1), z1 = min(cz + 1, ix.gdim - 1);
        // first round: the 2x2x2 cells nearest to the query (the query's cell and, per axis, the neighbour on
        // the side of the nearer face); bits are relative to (x0, y0, z0) like those of the full block
        const int ax = max(cx - ((fx - (float)cx) < 0.5f ? 1 : 0), 0), bx = min(ax + 1, ix.gdim - 1);
        const int ay = max(cy - ((fy - (float)cy) < 0.5f ? 1 : 0), 0), by = min(ay + 1, ix.gdim - 1);
        const int az = max(cz - ((fz - (float)cz) < 0.5f ? 1 : 0), 0), bz = min(az + 1, ix.gdim - 1);
        uint32_t mask = 0, mask_rest = 0;
#pragma unroll
        for (int kz = 0; kz < 3; kz++)
#pragma unroll
            for (int ky = 0; ky < 3; ky++)
#pragma unroll
                for (int kx = 0; kx < 3; kx++) {
                    const int X = x0 + kx, Y = y0 + ky, Z = z0 + kz;
                    const uint32_t bit = 1u << (kx + 3 * ky + 9 * kz);
                    if (X <= x1 && Y <= y1 && Z <= z1) {
                        if (X >= ax && X <= bx && Y >= ay && Y <= by && Z >= az && Z <= bz) mask |= bit;
                        else mask_rest |= bit;
                    }
                }
        c.mask = mask; c.mask_rest = mask_rest;
        cell0 = (uint32_t)x0 | ((uint32_t)y0 << 10) | ((uint32_t)z0 << 20);
        // distance from the query to the nearest face, with cells beyond it, of the small and of the full block
        float face = inf, face8 = inf;
        if (x0 > 0) face = fminf(face, px - (ix.ox + (float)x0 * ix.h));
        if (y0 > 0) face = fminf(face, py - (ix.oy + (float)y0 * ix.h));
        if (z0 > 0) face = fminf(face, pz - (ix.oz + (float)z0 * ix.h));
        if (x1 < ix.gdim - 1) face = fminf(face, (ix.ox + (float)(x1 + 1) * ix.h) - px);
        if (y1 < ix.gdim - 1) face = fminf(face, (ix.oy + (float)(y1 + 1) * ix.h) - py);
        if (z1 < ix.gdim - 1) face = fminf(face, (ix.oz + (float)(z1 + 1) * ix.h) - pz);
        if (ax > 0) face8 = fminf(face8, px - (ix.ox + (float)ax * ix.h));
        if (ay > 0) face8 = fminf(face8, py - (ix.oy + (float)ay * ix.h));
        if (az > 0) face8 = fminf(face8, pz - (ix.oz + (float)az * ix.h));
        if (bx < ix.gdim - 1) face8 = fminf(face8, (ix.ox + (float)(bx + 1) * ix.h) - px);
        if (by < ix.gdim - 1) face8 = fminf(face8, (ix.oy + (float)(by + 1) * ix.h) - py);
        if (bz < ix.gdim - 1) face8 = fminf(face8, (ix.oz + (float)(bz + 1) * ix.h) - pz);
        c.lim = face8 - 2e-3f * ix.h;          // everything outside the scanned block is at least this far away
        c.lim_full = face - 2e-3f * ix.h;
        c.probe = true;
        c.defer = false;
        c.reach = __builtin_amdgcn_sqrtf(c.b.d2) * 1.00001f;
    }
    return c;
}

// Phase 1 of query i (active = false: an idle lane, which scans nothing): its position (px, py, pz), the bound from its previous pair, the
// certificates, and what it scans.  A query that can do neither a bounded scan nor a probe is pushed to the work list (shard push_shard)
// with its provisional pair.
__device__ __forceinline__ CellQuery plan_query(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const Affine &X, uint32_t i, bool active,
                                                uint32_t push_shard, bool from_list, float &px, float &py, float &pz, uint32_t &cell0)
{
    const float inf = __int_as_float(0x7f800000);
    CellQuery c;
    c.b.d2 = inf; c.b.pos = -1; c.b.row = 0x7fffffff;
    c.mask = c.mask_rest = 0;
    c.lim = c.lim_full = c.reach = 0.f;
    c.defer = c.searched = c.probe = c.uncert = c.hood_ok = false;
    if (active) {
        // Two memory round trips decide a certified pair: everything addressed by i first (the certificate is loaded
        // whether or not it will be needed), then the previous winner as one 16-byte load.
        const float x = a.in.x[i], y = a.in.y[i], z = a.in.z[i];
        const int32_t prev = a.pos_prev ? a.pos_prev[i] : -1;
        float clear = 0.0f, rx = 0.0f, ry = 0.0f, rz = 0.0f;                              // L (0: no certificate), p_ref
        if (a.use_slack) { const float4 ce = a.cert[i]; rx = ce.x; ry = ce.y; rz = ce.z; clear = ce.w; }      // one 16-byte load (bit 0 of w: neighbourhood flag)
        px = xf_row(X.m + 0, x, y, z, 1.0f); py = xf_row(X.m + 4, x, y, z, 1.0f); pz = xf_row(X.m + 8, x, y, z, 1.0f);
        if (prev >= 0 && (uint32_t)prev < ix.n) {
            const float4 q = ix.tq[prev];
            const float d2 = dist2(px, py, pz, q.x, q.y, q.z);
            const int32_t row = __float_as_int(q.w);
            if (d2 <= inf) { c.b.d2 = d2; c.b.pos = prev; c.b.row = row; }                // (not NaN)
        }
        bool certified = false;
        if (a.use_slack && c.b.pos >= 0 && !from_list) {
            const float m2 = dist2(px, py, pz, rx, ry, rz);                               // delta^2
            certified = cert_holds(c.b.d2, m2, clear);
            if (!certified && (__float_as_uint(clear) & 1u) && a.certk) {
                int32_t pw; float d2w;
                if (hood_test(a, ix, i, px, py, pz, m2, c.b.pos, c.b.d2, c.b.row, pw, d2w)) {
                    certified = c.hood_ok = true; c.b.pos = pw; c.b.d2 = d2w;
                }
            }
        }
        if (!certified) {               // (certified: same pair, nothing stored -- its distance is evaluated when someone asks: k_pairs_d2)
            c.uncert = true;
            c.defer = true;
            if (c.b.pos >= 0 && ix.glevel > 0) c = plan_bounded_scan(ix, px, py, pz, c, cell0);
            if (c.defer && c.b.pos >= 0 && ix.glevel > 0) c = plan_probe(ix, px, py, pz, c, cell0);
            if (c.defer) {
                a.pos_out[i] = c.b.pos;      // provisional: the tree walk starts from this bound
                a.d2_out[i] = c.b.d2;
                a.cert[i].w = 0.0f;           // pairs found by the walk carry no certificate
                a.pairrec[2 * (size_t)i + 1].w = 2.0f;      // ... and k_accumulate has to fetch their record again
                sl_push(wl.work, push_shard, i);
            }
        }
    }
    return c;
}

// radius of the neighbourhood a scan collects: the pair's hint from its last scan (but beyond the bound on the winner's distance), else
// twice the previous pair's distance; never beyond what the scan covers
template <bool HOOD>
__device__ __forceinline__ float hood_radius(const PassArgs &a, uint32_t i, CellQuery c)
{
    if (HOOD && c.reach > 0.0f && a.certk) {
        const float hint = a.hoodr[i].y;
        return fminf(c.probe ? c.lim_full : c.lim, hint > 0.0f ? fmaxf(hint, 1.01f * c.reach) : 2.0f * c.reach);      // (a probe: cut to what it has scanned in the end)
    }
    return 0.0f;
}

// Scan target points [j0, j1) for query q of the tile and merge the result into the query's (nearest, second nearest, position).
// EVERY thread of the block calls it (have = false: nothing to scan): it contains a barrier.
template <bool HOOD>
__device__ __forceinline__ void scan_merge(const PassArgs &a, const TargetIndex &ix, const TileLds &s, bool have, int q, uint32_t j0, uint32_t j1)
{
    unsigned long long mykey = ~0ull;
    uint32_t my2nd = 0x7f800000u;          // d2 bits of this range's second-nearest point
    int32_t mypos = -1;
    if (have) {
        const float qx = s.px[q], qy = s.py[q], qz = s.pz[q];
        const float t2 = HOOD ? s.reach[q] * s.reach[q] : 0.0f;
        for (uint32_t j = j0; j < j1; j += 4) {
            float4 t4[4];
#pragma unroll
            for (int k = 0; k < 4; k++) t4[k] = ix.tq[min(j + (uint32_t)k, j1 - 1)];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (j + (uint32_t)k < j1) {
                    const float d2 = dist2(qx, qy, qz, t4[k].x, t4[k].y, t4[k].z);
                    if (HOOD && d2 < t2) {                         // a member of the query's neighbourhood
                        const uint32_t hs = atomicAdd(&s.hcnt[q], 1u);
                        if (hs < (uint32_t)kHoodSlots) reinterpret_cast<uint32_t *>(a.certk)[(size_t)s.qi[q] * kHoodSlots + hs] = j + (uint32_t)k;
                    }
                    if (d2 == d2) {
                        const unsigned long long key = ((unsigned long long)__float_as_uint(d2) << 32) |
                                                       (unsigned long long)(uint32_t)__float_as_int(t4[k].w);
                        if (key < mykey) { my2nd = (uint32_t)(mykey >> 32); mykey = key; mypos = (int32_t)(j + k); }
                        else my2nd = min(my2nd, __float_as_uint(d2));
                    }
                }
            }
        }
        if (mypos >= 0) {
            // Every key that loses against the running minimum -- ours, or the one we displace -- is a candidate for
            // the query's second-nearest distance; the final winner is the only key never offered.  (Deciding
            // "am I the winner" per round would be wrong: a later round can still displace this round's winner.)
            const unsigned long long old = atomicMin(&s.key[q], mykey);
            uint32_t offer;
            if (mykey < old) offer = min((uint32_t)(old >> 32), my2nd);
            else if (mykey == old) offer = my2nd;              // the previous pair found again in its cell
            else offer = (uint32_t)(mykey >> 32);
            atomicMin(&s.second[q], offer);
        }
    }
    __syncthreads();
    if (mypos >= 0 && s.key[q] == mykey) s.pos[q] = mypos;
}

// One round of scans: the queries' cells in `mask` become (query, cell) items in LDS (block-wide prefix sum of the counts), then one
// thread scans one item.  EVERY thread of the block calls it.  False (round 0 only): no query of the tile scans or probes anything --
// the common block of a converged pass: every pair certified (or handed to the walk), nothing to scan or store.
// scans: this query does a bounded scan or a probe; total_all: the items so far, for the debug counters.
template <bool HOOD>
__device__ __forceinline__ bool scan_round(const PassArgs &a, const TargetIndex &ix, const TileLds &s, int round, uint32_t mask, bool scans, uint32_t &total_all)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // block-wide exclusive prefix sum of the item counts
    const uint32_t cnt = (uint32_t)__popc(mask);
    uint32_t incl = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(incl, off, 64);
        if (lane >= off) incl += u;
    }
    if (lane == 63) s.wsum[wave] = incl;
    if (round == 0) {
        const unsigned long long any3 = __ballot(scans);
        if (lane == 0) s.anyw[wave] = (any3 != 0ull);
    }
    __syncthreads();
    uint32_t base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kPassThreads / 64; w++) {
        const uint32_t ws = s.wsum[w];
        if (w < wave) base += ws;
        total += ws;
    }
    total_all += total;
    if (round == 0 && !ix.dbg) {
        uint32_t any = 0;
#pragma unroll
        for (int w = 0; w < kPassThreads / 64; w++) any |= s.anyw[w];
        if (!any) return false;
    }
    {
        uint32_t slot = base + incl - cnt;
        uint32_t m = mask;
        while (m) {
            const int bit = __ffs((int)m) - 1;
            m &= m - 1;
            s.items[slot++] = (uint16_t)((tid << 5) | bit);
        }
        if (tid == 0) *s.nmore = 0;
    }
    __syncthreads();
    // One thread scans one (query, cell) item -- at most kItemMax points of it: the rest of a crowded cell (the inner rings of a scan hold
    // ~100 points per finest cell) is handed over in chunks of kItemMax points, as sub-items in the free tail of the item array that the
    // whole block scans afterwards.  A wave's cost is then bounded by kItemMax points per lane, not by the most crowded cell among its 64 items.
    constexpr uint32_t kItemMax = 16;          // (8 / 32: the same within noise on the 2M scan pair)
    uint2 *s_more = reinterpret_cast<uint2 *>(s.items + ((total + 3u) & ~3u));          // (8-byte aligned: 4 uint16)
    const uint32_t more_cap = (uint32_t)(kTileItems - ((total + 3u) & ~3u)) / 4u;
    for (uint32_t it0 = 0; it0 < total; it0 += kPassThreads) {
        const uint32_t it = it0 + tid;
        int q = 0;
        uint32_t j0 = 0, j1 = 0;
        if (it < total) {
            const uint32_t item = s.items[it];
            q = (int)(item >> 5);
            const int bit = (int)(item & 31u);
            const int kz = bit / 9, ky = (bit - 9 * kz) / 3, kx = bit - 9 * kz - 3 * ky;
            const uint32_t c0 = s.cell0[q];
            const uint32_t cx = (c0 & 1023u) + (uint32_t)kx, cy = ((c0 >> 10) & 1023u) + (uint32_t)ky, cz = (c0 >> 20) + (uint32_t)kz;
            const uint2 rng = cell_range(ix, (spread3(cz) << 2) | (spread3(cy) << 1) | spread3(cx));
            if (ix.dbg) atomicAdd(ix.dbg + 3, (unsigned long long)(rng.y - rng.x));
            j0 = rng.x; j1 = rng.y;
            // a crowded cell: chunks are handed over from the end while the tail has room; what is left stays with this thread
            while (j1 > j0 && j1 - j0 > kItemMax) {
                const uint32_t js = j0 + ((j1 - j0 - 1u) / kItemMax) * kItemMax;      // start of the last chunk
                const uint32_t e = atomicAdd(s.nmore, 1u);
                if (e >= more_cap) break;
                s_more[e] = make_uint2((uint32_t)q | ((j1 - js) << 8), js);
                j1 = js;
            }
        }
        scan_merge<HOOD>(a, ix, s, it < total && j1 > j0, q, j0, j1);
    }
    __syncthreads();
    // sub-items of crowded cells
    {
        const uint32_t nmore = min(*s.nmore, more_cap);
        for (uint32_t e0 = 0; e0 < nmore; e0 += kPassThreads) {
            const uint32_t e = e0 + tid;
            int q = 0;
            uint32_t j0 = 0, j1 = 0;
            if (e < nmore) { const uint2 m = s_more[e]; q = (int)(m.x & 255u); j0 = m.y; j1 = m.y + (m.x >> 8); }
            scan_merge<HOOD>(a, ix, s, e < nmore && j1 > j0, q, j0, j1);
        }
    }
    __syncthreads();
    return true;
}

// Phase 3 of a query that scanned or probed: the pair, and its certificates for the following passes -- or, for a probe that could
// not prove its best, the work list: the tree walk takes over from this (tighter) bound
template <bool HOOD>
__device__ __forceinline__ void store_pair(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const TileLds &s, uint32_t i, uint32_t push_shard,
                                           float px, float py, float pz, CellQuery c)
{
    const int tid = threadIdx.x;
    const unsigned long long key = s.key[tid];
    const float d1sq = __uint_as_float((uint32_t)(key >> 32));
    const float d1 = sqrtf(d1sq) * 1.000001f;
    a.pos_out[i] = s.pos[tid];
    a.d2_out[i] = d1sq;
    if (c.probe && !(d1 < c.lim)) {
        a.cert[i].w = 0.0f;
        a.pairrec[2 * (size_t)i + 1].w = 2.0f;
        sl_push(wl.work, push_shard, i);
        return;
    }
    // certificate for the following passes
    const float second = sqrtf(__uint_as_float(s.second[tid])) * 0.999999f;
    const float L = fminf(second, c.lim * 0.99999f);
    // the neighbourhood: everything the scan saw closer than T, if it fits (the winner is inside: T > d1)
    bool hood = false;
    const float Tq = HOOD ? fminf(s.reach[tid], c.lim) : 0.0f;         // (a probe collected up to its full block's bound: cut to what it scanned)
    if (Tq > 0.0f) {
        const uint32_t hc = s.hcnt[tid];
        const float T = Tq * 0.99999f;
        hood = T > d1 && hc >= 1u && hc <= (uint32_t)kHoodSlots;
        if (hood) {
            uint32_t *slots = reinterpret_cast<uint32_t *>(a.certk) + (size_t)i * kHoodSlots;
#pragma unroll
            for (int k = 1; k < kHoodSlots; k++) if ((uint32_t)k >= hc) slots[k] = kHoodNone;
        }
        // the radius that would have held ~6.5 points: count ~ T^2.5 between a surface and a slab
        const float scale = fminf(fmaxf(__powf(6.5f / ((float)hc + 0.5f), 0.4f), 0.4f), 1.5f);
        a.hoodr[i] = make_float2(hood ? T : 0.0f, Tq * scale);
        if (ix.dbg) atomicAdd(ix.dbg + (hood ? 9 : 10), 1ull);
    }
    const float Lw = cert_word((L > d1) ? L : 0.0f, hood);
    a.cert[i] = make_float4(px, py, pz, Lw);
    store_pair_record(a, ix, i, s.pos[tid]);
}

// debug counters of a tile: [0] (query,cell) items, [1] certified, [2] cell scans, [6] probes, [7] handed to the walk in phase 1,
// [8] settled by their neighbourhood
__device__ __forceinline__ void count_tile_debug(const TargetIndex &ix, bool active, CellQuery c, uint32_t total_all)
{
    if (threadIdx.x == 0) atomicAdd(ix.dbg + 0, (unsigned long long)total_all);
    const unsigned long long mc = __ballot(active && !c.defer && !c.searched && !c.probe), ms = __ballot(c.searched), mp = __ballot(c.probe), md = __ballot(c.defer);
    const unsigned long long mh = __ballot(c.hood_ok);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(ix.dbg + 8, (unsigned long long)__popcll(mh));
        atomicAdd(ix.dbg + 1, (unsigned long long)__popcll(mc)); atomicAdd(ix.dbg + 2, (unsigned long long)__popcll(ms));
        atomicAdd(ix.dbg + 6, (unsigned long long)__popcll(mp)); atomicAdd(ix.dbg + 7, (unsigned long long)__popcll(md));
    }
}

// One tile of 256 queries (i >= a.n: idle lane).  Called by k_search_cells (tile = block) and by k_pass_fused (the queries its
// streaming phase could not certify).
// from_list: the queries come from k_pass_fused's list -- their certificates have just failed there and are not tried again.
// HOOD: this scan also keeps neighbourhoods (off in the passes right after the first big move, whose certificates the next
// move invalidates anyway: the kernel then runs without the extra LDS and the scattered member stores).
template <bool HOOD>
__device__ __forceinline__ void cells_tile(const PassArgs &a, const TargetIndex &ix, const WorkLists &wl, const Affine &X, const uint32_t i,
                                           const uint32_t shard, const bool from_list)
{
    __shared__ float s_px[kPassThreads], s_py[kPassThreads], s_pz[kPassThreads];
    __shared__ unsigned long long s_key[kPassThreads];
    __shared__ uint32_t s_second[kPassThreads];        // d2 bits of the second-nearest scanned point
    __shared__ int32_t s_pos[kPassThreads];
    __shared__ uint32_t s_cell0[kPassThreads];
    __shared__ __align__(8) uint16_t s_items[kTileItems];       // (the free tail also holds the 8-byte sub-items of crowded cells)
    __shared__ uint32_t s_wsum[kPassThreads / 64 + 1];
    __shared__ uint32_t s_anyw[kPassThreads / 64];     // per-wave flags for block-wide "any" votes
    __shared__ uint32_t s_nmore;                       // sub-items of crowded cells (phase 2)
    constexpr int kHoodLds = HOOD ? kPassThreads : 1;
    __shared__ float s_reach[kHoodLds];                // T of the query's neighbourhood (0: none wanted)
    __shared__ uint32_t s_hcnt[kHoodLds];              // scanned points closer than T (the first 8 go straight to certk)
    __shared__ uint32_t s_qi[kHoodLds];                // the query's index
    const TileLds s = {s_px, s_py, s_pz, s_key, s_second, s_pos, s_cell0, s_items, s_wsum, s_anyw, &s_nmore, s_reach, s_hcnt, s_qi};

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool active = i < a.n;
    // the shard a query is appended to follows the QUERY's own tile of 256, whoever scans it: a block of the streaming kernels strides over
    // many tiles, and a shard's capacity (shard_capacity) only covers the tiles with (tile & 63) == shard
    const uint32_t push_shard = from_list ? ((i / kPassThreads) & (uint32_t)(kShards - 1)) : shard;

    // ---- phase 1 ----
    float px = 0.f, py = 0.f, pz = 0.f;
    CellQuery c = plan_query(a, ix, wl, X, i, active, push_shard, from_list, px, py, pz, s_cell0[tid]);
    if (!from_list) {
        // how many pairs had to be searched this pass: tells the host when the alignment has converged far enough for the fused
        // pass (engine.cpp, batch_eligible); word 1 behind each shard counter of the work list is free (counters sit 16 words apart)
        const unsigned long long mu = __ballot(c.uncert);
        if (lane == 0 && mu) atomicAdd(wl.work.counts + shard * kShardStride + 1, (uint32_t)__popcll(mu));      // (one word per shard: a single word saturates near 88 atomics per microsecond)
    }
    s_px[tid] = px; s_py[tid] = py; s_pz[tid] = pz;
    s_pos[tid] = c.b.pos;
    s_key[tid] = (c.b.pos >= 0) ? (((unsigned long long)__float_as_uint(c.b.d2) << 32) | (unsigned long long)(uint32_t)c.b.row) : ~0ull;
    s_second[tid] = 0x7f800000u;
    c.reach = hood_radius<HOOD>(a, i, c);
    if (HOOD) { s_reach[tid] = c.reach; s_hcnt[tid] = 0; s_qi[tid] = i; }

    // ---- phase 2: scan; if any probe needs its outer cells, scan those ----
    uint32_t total_all = 0;
    for (int round = 0; round < 2; round++) {
        if (!scan_round<HOOD>(a, ix, s, round, c.mask, c.searched || c.probe, total_all)) return;
        // A probe that scanned its 2x2x2 block: done if the best point is closer than the nearest outer face of that block,
        // else the other cells of the 3x3x3 block are scanned in a second round (about one query in ten on a surface cloud).
        bool more = false;
        if (round == 0 && c.probe) {
            const float d1 = sqrtf(__uint_as_float((uint32_t)(s_key[tid] >> 32))) * 1.00001f;
            // (2 % of room at least: a best that only just clears the small block's face would hold a certificate no jitter survives)
            if (!(d1 * 1.02f < c.lim)) { more = (c.mask_rest != 0); c.lim = c.lim_full; }
        }
        c.mask = more ? c.mask_rest : 0u;
        if (round == 1) break;
        const unsigned long long anym = __ballot(more);
        if (lane == 0) s_anyw[wave] = (anym != 0ull);
        __syncthreads();
        uint32_t any = 0;
#pragma unroll
        for (int w = 0; w < kPassThreads / 64; w++) any |= s_anyw[w];
        if (!any) break;
    }
    if (ix.dbg) count_tile_debug(ix, active, c, total_all);

    // ---- phase 3 ----
    if (active && (c.searched || c.probe)) store_pair<HOOD>(a, ix, wl, s, i, push_shard, px, py, pz, c);
}

}  // namespace symmicp
