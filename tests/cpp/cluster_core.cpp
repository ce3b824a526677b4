// tests/cpp/cluster_core.cpp -- the host instantiation of cluster_core.h (find, unite) over edge lists in adversarial orders.
//
//   cluster_core          (no arguments; built and run by tests/test_cluster_ref.py, plain or with -fsanitize=address,undefined)
// After EVERY union it checks the invariant parent[x] <= x for every x; at the end of a list it checks that the root of every row is the
// MINIMUM row of its component (components from a reference label-spreading pass over the same edges) and that find() leaves
// the roots alone.  Two policies drive the same code: SerialOps (plain loads and stores), and MeddlingOps, whose compare-and-swap
// first lets "another thread" complete a union of its own on the same array -- the interleaving that makes a swap fail on the
// device -- so that the retry path (find again from the value the failed swap returned) runs on the host too.
// Prints one line per case; exit code != 0 on the first failure.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "cluster_core.h"

using namespace symmicp::cluster;
typedef std::vector<std::pair<uint32_t, uint32_t>> Edges;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t m)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % m);
}

// what the meddling thread will unite next, and how often a swap lost to it
static uint32_t *med_parent = nullptr;
static const Edges *med_edges = nullptr;
static size_t med_at = 0;
static uint64_t med_lost = 0;

struct MeddlingOps {
    static uint32_t load(const uint32_t *p) { return *p; }
    static uint32_t cas(uint32_t *p, uint32_t expected, uint32_t desired)
    {
        if (med_edges) {
            // a burst of the other thread's own unions ...
            for (uint32_t k = rnd(8); k > 0 && med_at < med_edges->size(); k--) {
                const std::pair<uint32_t, uint32_t> e = (*med_edges)[med_at++];
                (void)unite<SerialOps>(med_parent, e.first, e.second);
            }
            // ... and now and then it gets to THIS root first: it joins the two sets the swap at hand is about to join (they belong
            // to one component whatever the order), so the swap at hand finds the word changed
            if (p == med_parent + expected && desired < expected && rnd(4) == 0) (void)unite<SerialOps>(med_parent, expected, desired);
        }
        const uint32_t old = SerialOps::cas(p, expected, desired);
        if (old != expected) med_lost++;
        return old;
    }
};

static void check_invariant(const std::vector<uint32_t> &parent)
{
    for (uint32_t x = 0; x < parent.size(); x++) CHECK(parent[x] <= x);
}

// the minimum row of every row's component, by spreading minima over the edges until nothing changes
static std::vector<uint32_t> component_min(uint32_t n, const Edges &a, const Edges &b)
{
    std::vector<uint32_t> m(n);
    for (uint32_t i = 0; i < n; i++) m[i] = i;
    bool changed = true;
    while (changed) {
        changed = false;
        for (const Edges *es : {&a, &b})
            for (const auto &e : *es) {
                const uint32_t lo = std::min(m[e.first], m[e.second]);
                if (m[e.first] != lo || m[e.second] != lo) { m[e.first] = m[e.second] = lo; changed = true; }
            }
    }
    return m;
}

template <class Ops>
static void run(const char *name, uint32_t n, const Edges &edges, const Edges &meddle)
{
    std::vector<uint32_t> parent(n);
    for (uint32_t i = 0; i < n; i++) parent[i] = i;
    med_parent = parent.data(); med_edges = &meddle; med_at = 0; med_lost = 0;
    uint64_t lost = 0;
    // the full check after every union is O(n): on the long lists it runs after every union of the first 256 and then every 64th
    size_t k = 0;
    for (const auto &e : edges) {
        uint32_t l = 0;
        const uint32_t top = unite<Ops>(parent.data(), e.first, e.second, &l);
        lost += l;
        // what it returns is an ancestor of both rows: at or below both, and in their set
        CHECK(top <= e.first && top <= e.second && find<SerialOps>(parent.data(), top) == find<SerialOps>(parent.data(), e.first));
        CHECK(find<SerialOps>(parent.data(), e.first) == find<SerialOps>(parent.data(), e.second));
        if (k < 256 || k % 64 == 0 || n <= 512) check_invariant(parent);
        k++;
    }
    while (med_at < meddle.size()) { const auto e = meddle[med_at++]; (void)unite<SerialOps>(parent.data(), e.first, e.second); }
    check_invariant(parent);
    CHECK(lost <= med_lost);      // (med_lost counts the lost path-halving swaps too)
    const std::vector<uint32_t> want = component_min(n, edges, meddle);
    for (uint32_t x = 0; x < n; x++) CHECK(find<Ops>(parent.data(), x) == want[x]);
    check_invariant(parent);
    for (uint32_t x = 0; x < n; x++) CHECK(parent[want[x]] == want[x]);      // a component's minimum is a root
    med_edges = nullptr;
    std::printf("%-28s n %5u  edges %6zu + %5zu  lost swaps %llu  ok\n", name, n, edges.size(), meddle.size(), (unsigned long long)lost);
}

static Edges shuffled(Edges e)
{
    for (size_t i = e.size(); i > 1; i--) std::swap(e[i - 1], e[rnd((uint32_t)i)]);
    return e;
}

int main()
{
    const uint32_t n = 2000;
    const Edges none;
    Edges up, down, star_lo, star_hi, random, twice, lattice;
    for (uint32_t i = 0; i + 1 < n; i++) up.push_back({i, i + 1});
    for (uint32_t i = n - 1; i > 0; i--) down.push_back({i, i - 1});
    for (uint32_t i = 1; i < n; i++) star_lo.push_back({0, i});
    for (uint32_t i = 0; i + 1 < n; i++) star_hi.push_back({i, n - 1});
    for (uint32_t k = 0; k < 1500; k++) random.push_back({rnd(n), rnd(n)});      // below n edges: several components, self-loops included
    for (const auto &e : random) { twice.push_back(e); twice.push_back({e.second, e.first}); }
    for (uint32_t y = 0; y < 40; y++)
        for (uint32_t x = 0; x < 40; x++) {
            if (x + 1 < 40) lattice.push_back({y * 40 + x, y * 40 + x + 1});
            if (y + 1 < 40) lattice.push_back({y * 40 + x, (y + 1) * 40 + x});
        }

    run<SerialOps>("one row", 1, none, none);
    run<SerialOps>("no edges", 7, none, none);
    run<SerialOps>("ascending chain", n, up, none);
    run<SerialOps>("descending chain", n, down, none);
    run<SerialOps>("shuffled chain", n, shuffled(up), none);
    run<SerialOps>("star at row 0", n, star_lo, none);
    run<SerialOps>("star at the last row", n, star_hi, none);
    run<SerialOps>("random graph", n, random, none);
    run<SerialOps>("every edge twice", n, twice, none);
    run<SerialOps>("lattice 40 x 40", 1600, shuffled(lattice), none);

    // the same lists against a second thread that unites the SAME component in another order in the middle of the swaps
    run<MeddlingOps>("meddled ascending chain", n, up, down);
    run<MeddlingOps>("meddled descending chain", n, down, shuffled(up));
    run<MeddlingOps>("meddled star", n, star_hi, shuffled(star_lo));
    run<MeddlingOps>("meddled random graph", n, shuffled(twice), shuffled(random));
    run<MeddlingOps>("meddled lattice", 1600, shuffled(lattice), shuffled(lattice));
    std::printf("cluster_core: ok\n");
    return 0;
}
