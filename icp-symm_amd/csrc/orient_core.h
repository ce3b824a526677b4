// orient_core.h -- what the kernels of symmicp_ctx_orient_normals (kernels_orient.hip; include/symmicp.h, "Normal orientation", defines
// the result) share with a host program (tests/cpp/orient_core.cpp): the weight word of an edge, the packing of a row's state, the
// candidate key, the hook rule, the bounded walk up the parents -- and a host Boruvka over an explicit edge list built from them.
//
// State.  One 32-bit word per row: (parent << 1) | parity, parity = the sign relation between the row's normal and its parent's
// (1: they disagree).  A root is a row whose parent is itself, with parity 0.  Parent and parity share the word so that one load
// sees both.
// Edge.  The weight word of {i, j}: bits 0..30 = the bits of w = fmaxf(1 - |d|, 0) (w >= 0: its sign bit is free), bit 31 = s = d < 0.
// Order.  (w bits, lo, hi), strict and total; the candidate of a component is the minimum over its outgoing edges, taken in two
// integer-minimum passes: key64 = (w bits << 32) | lo first, then hi among the edges whose key64 is the minimum.
// Hook.  Root a, whose component chose {u in A, v in B}, hangs itself under b = root(B) -- unless B chose the same edge and a < b.
// Under a strict total order the chosen edges form no cycle longer than two, and both members of a 2-cycle chose the same edge, so
// the rule is acyclic with every root writing its own word only.
// NO loop here waits for another thread: walk_up follows parents for at most `bound` steps and reports when that was not enough.
#pragma once
#include <stdint.h>
#include <string.h>
#if !defined(__HIPCC__) && !defined(__CUDACC__)
#include <math.h>
#include <vector>
#endif

#if defined(__HIPCC__) || defined(__CUDACC__)
#define ORIENT_HD __host__ __device__
#else
#define ORIENT_HD
#endif

namespace symmicp {
namespace orient {

constexpr uint32_t kSignBit = 0x80000000u;
constexpr uint64_t kNoKey = ~0ull;
constexpr uint32_t kNoRow = 0xffffffffu;
constexpr int kMaxRounds = 32;

ORIENT_HD inline uint32_t bits_of(float f)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(f);
#else
    uint32_t u;
    memcpy(&u, &f, sizeof(u));
    return u;
#endif
}

// fp32, unfused (every file that includes this is built with -ffp-contract=off), in the association written
ORIENT_HD inline uint32_t weight_word(float nxi, float nyi, float nzi, float nxj, float nyj, float nzj)
{
    const float d = (nxi * nxj + nyi * nyj) + nzi * nzj;
    const float w = fmaxf(1.0f - fabsf(d), 0.0f);
    // (fmaxf(NaN, 0) is 0 and cannot arise from finite normals anyway; -0 cannot arise: 1 - |d| is +0 when it is zero)
    return (bits_of(w) & ~kSignBit) | (d < 0.0f ? kSignBit : 0u);
}

ORIENT_HD inline uint32_t pack(uint32_t parent, uint32_t parity) { return (parent << 1) | (parity & 1u); }
ORIENT_HD inline uint32_t parent_of(uint32_t word) { return word >> 1; }
ORIENT_HD inline uint32_t parity_of(uint32_t word) { return word & 1u; }

ORIENT_HD inline uint64_t key64(uint32_t weight_word_, uint32_t lo) { return ((uint64_t)(weight_word_ & ~kSignBit) << 32) | (uint64_t)lo; }

// does root a (which chose an edge into the component of root b) write its word?  same_edge: b's component chose the same edge
ORIENT_HD inline bool hook_writes(uint32_t a, uint32_t b, bool same_edge) { return !(same_edge && a < b); }

// the word root a writes: u in A, v in B, word_u / word_v their words of the FLAT state the round began with
ORIENT_HD inline uint32_t hook_word(uint32_t word_u, uint32_t word_v, uint32_t weight_word_)
{
    return pack(parent_of(word_v), parity_of(word_u) ^ (weight_word_ >> 31) ^ parity_of(word_v));
}

// follows parents from row i until a root, at most `bound` links: *root_word = pack(root, parity of i relative to the root).
// false: more than `bound` links (the state is not the forest the caller believes it to be); *root_word is what was reached.
ORIENT_HD inline bool walk_up(const uint32_t *words, uint32_t i, uint32_t bound, uint32_t *root_word)
{
    uint32_t p = i, par = 0;
    for (uint32_t step = 0;; step++) {
        const uint32_t w = words[p];
        if (parent_of(w) == p) { *root_word = pack(p, par); return true; }
        if (step >= bound) { *root_word = pack(p, par); return false; }
        par ^= parity_of(w);
        p = parent_of(w);
    }
}

// a float's bits as an unsigned word in the floats' order (-inf lowest; -0 below +0: callers add +0.0f first where that matters)
ORIENT_HD inline uint32_t ordered_bits(float f)
{
    const uint32_t u = bits_of(f);
    return (u & kSignBit) ? ~u : (u | kSignBit);
}

#if !defined(__HIPCC__) && !defined(__CUDACC__)
struct Edge { uint32_t u, v, ww; };      // ww = weight_word

struct Forest {
    std::vector<uint32_t> words;          // flat: pack(root, parity relative to the root)
    std::vector<uint32_t> tree;           // (lo, hi) pairs in the order they were hooked
    int rounds = 0;                       // rounds that hooked something
    bool ok = true;                       // false: a walk exceeded its bound, or more than kMaxRounds rounds
};

// the rounds of the kernels, one after another on the host: candidates (two minimum passes), hooks from the flat state into a copy,
// flatten by bounded walks.  Self-loops are ignored; an edge may be listed any number of times, from either end.
inline Forest boruvka(uint32_t n, const std::vector<Edge> &edges)
{
    Forest f;
    f.words.resize(n);
    for (uint32_t i = 0; i < n; i++) f.words[i] = pack(i, 0);
    std::vector<uint64_t> best(n);
    std::vector<uint32_t> best_hi(n), mid(n);
    for (int round = 0;; round++) {
        if (round > kMaxRounds) { f.ok = false; return f; }
        for (uint32_t i = 0; i < n; i++) { best[i] = kNoKey; best_hi[i] = kNoRow; }
        for (const Edge &e : edges) {
            const uint32_t ru = parent_of(f.words[e.u]), rv = parent_of(f.words[e.v]);
            if (ru == rv) continue;
            const uint64_t key = key64(e.ww, e.u < e.v ? e.u : e.v);
            if (key < best[ru]) best[ru] = key;
            if (key < best[rv]) best[rv] = key;
        }
        for (const Edge &e : edges) {
            const uint32_t ru = parent_of(f.words[e.u]), rv = parent_of(f.words[e.v]);
            if (ru == rv) continue;
            const uint32_t lo = e.u < e.v ? e.u : e.v, hi = e.u < e.v ? e.v : e.u;
            const uint64_t key = key64(e.ww, lo);
            if (key == best[ru] && hi < best_hi[ru]) best_hi[ru] = hi;
            if (key == best[rv] && hi < best_hi[rv]) best_hi[rv] = hi;
        }
        // the sign bit of the chosen edge: any listing of {lo, hi} with that weight carries it
        uint32_t hooks = 0;
        mid = f.words;
        for (uint32_t a = 0; a < n; a++) {
            if (parent_of(f.words[a]) != a || best[a] == kNoKey) continue;
            const uint32_t lo = (uint32_t)(best[a] & 0xffffffffull), hi = best_hi[a];
            uint32_t ww = 0;
            for (const Edge &e : edges)
                if (((e.u == lo && e.v == hi) || (e.u == hi && e.v == lo)) && (e.ww & ~kSignBit) == (uint32_t)(best[a] >> 32)) { ww = e.ww; break; }
            const bool lo_mine = parent_of(f.words[lo]) == a;
            const uint32_t u = lo_mine ? lo : hi, v = lo_mine ? hi : lo;
            const uint32_t b = parent_of(f.words[v]);
            if (!hook_writes(a, b, best[b] == best[a] && best_hi[b] == best_hi[a])) continue;
            mid[a] = hook_word(f.words[u], f.words[v], ww);
            f.tree.push_back(lo);
            f.tree.push_back(hi);
            hooks++;
        }
        if (hooks == 0) return f;
        f.rounds++;
        for (uint32_t i = 0; i < n; i++)
            if (!walk_up(mid.data(), i, hooks + 1, &f.words[i])) f.ok = false;
        if (!f.ok) return f;
    }
}
#endif

}  // namespace orient
}  // namespace symmicp
