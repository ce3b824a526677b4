// cluster_core.h -- the concurrent union-find of symmicp_ctx_cluster (include/symmicp.h, "DBSCAN"), shared by the kernels
// (kernels_cluster.hip, kernels_region.hip: agent-scope atomics) and a host program (tests/cpp/cluster_core.cpp: plain loads and stores).
//
// parent[] is indexed by CALLER ROW and starts as parent[x] == x.  One invariant carries everything:
//
//     parent[x] <= x   for every x, at every moment, and a word only ever changes to a LOWER value.
//
//   - A root is a row with parent[x] == x.  Only a root is ever hooked (by compare-and-swap against its own value), and always under
//     a LOWER row; path halving replaces a parent by the grandparent, which is lower or equal.  So every link points to a lower or
//     equal row, and a row that has stopped being a root never becomes one again.
//   - find() therefore strictly descends until it meets a root: at most x steps from row x, whatever other threads do meanwhile.
//   - A failed compare-and-swap in unite() means that somebody else lowered the root's parent: the value it returns is a row strictly
//     below the failed root, and the next round starts there.  The larger of the two rows in hand strictly decreases from round to
//     round, so unite() ends after a bounded number of rounds by itself.
//   - NO loop here waits for another thread: each iteration follows a link that strictly descends or ends the loop.  A lane whose
//     compare-and-swap loses has lost to a lane that made progress.
//   - Once all unions are done the root of a component is its MINIMUM row (a root is never hooked under a higher one), so the result
//     does not depend on the order in which the unions arrived.
//
// Ops: uint32_t load(const uint32_t *p);  uint32_t cas(uint32_t *p, uint32_t expected, uint32_t desired) -> the value found at p
// (== expected iff the swap happened).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CLUSTER_HD __host__ __device__
#else
#define CLUSTER_HD
#endif

namespace symmicp {
namespace cluster {

// plain loads and stores: one thread
struct SerialOps {
    static inline uint32_t load(const uint32_t *p) { return *p; }
    static inline uint32_t cas(uint32_t *p, uint32_t expected, uint32_t desired)
    {
        const uint32_t old = *p;
        if (old == expected) *p = desired;
        return old;
    }
};

#if defined(__HIPCC__)
// relaxed agent-scope atomics: parent[] words are read and swapped by lanes of every XCD within one launch
struct AgentOps {
    __device__ static __forceinline__ uint32_t load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ static __forceinline__ uint32_t cas(uint32_t *p, uint32_t expected, uint32_t desired)
    {
        (void)__hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return expected;      // the value found (unchanged when the swap happened)
    }
};
#endif

// the root of x, halving the path on the way (every second link is cut to the grandparent; a lost swap only means somebody else
// cut it first)
template <class Ops>
CLUSTER_HD inline uint32_t find(uint32_t *parent, uint32_t x)
{
    while (true) {
        const uint32_t p = Ops::load(parent + x);
        if (p == x) return x;
        const uint32_t g = Ops::load(parent + p);      // g <= p < x
        if (g == p) return p;
        (void)Ops::cas(parent + x, p, g);
        x = g;
    }
}

// joins the sets of a and b: the LARGER root goes under the SMALLER.  Returns the row the joined set hung from when last seen (an
// ancestor of a and of b for good: the place to start the next find from); *lost, when given, += the lost compare-and-swaps (a statistic).
template <class Ops>
CLUSTER_HD inline uint32_t unite(uint32_t *parent, uint32_t a, uint32_t b, uint32_t *lost = nullptr)
{
    while (true) {
        a = find<Ops>(parent, a);
        b = find<Ops>(parent, b);
        if (a == b) return a;
        if (a < b) { const uint32_t t = a; a = b; b = t; }      // a > b
        const uint32_t old = Ops::cas(parent + a, a, b);
        if (old == a) return b;
        if (lost) (*lost)++;
        a = old;      // < the failed root: find again from there
    }
}

}  // namespace cluster
}  // namespace symmicp
