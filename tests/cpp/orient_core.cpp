// The host side of orient_core.h, on its own (g++, no HIP): orient::boruvka -- the rounds of kernels_orient.hip one after another --
// against Kruskal over the same edges in the total order (w bits, lo, hi), trees AND parities, on the edge lists that stress each
// part: all-equal weights (the row tie-break decides everything), mutual choices (2-cycles: one of the two roots must stand still),
// chains that make the hook graph deep (the flatten walk is as long as its bound allows), isolated vertices, duplicate and two-sided
// listings, self-loops; and the guard of orient::walk_up on states that are not a forest.  Prints "orient_core: ok" at the end.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <tuple>
#include <vector>

#include "orient_core.h"

using namespace symmicp::orient;

static int failures = 0;
#define CHECK(x) do { if (!(x)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); failures++; } } while (0)

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

// a weight word from a weight given as a float and a sign bit (what weight_word packs)
static uint32_t ww_of(float w, bool s) { return (bits_of(w) & ~kSignBit) | (s ? kSignBit : 0u); }

struct Ref {
    std::vector<std::pair<uint32_t, uint32_t>> tree;      // sorted (lo, hi)
    std::vector<uint32_t> comp;                           // lowest row of the component
    std::vector<uint32_t> par;                            // parity against the component's lowest row
};

static Ref kruskal(uint32_t n, const std::vector<Edge> &edges)
{
    std::vector<std::tuple<uint32_t, uint32_t, uint32_t, uint32_t>> order;      // (w bits, lo, hi, s)
    for (const Edge &e : edges)
        if (e.u != e.v) order.emplace_back(e.ww & ~kSignBit, std::min(e.u, e.v), std::max(e.u, e.v), e.ww >> 31);
    std::sort(order.begin(), order.end());
    std::vector<uint32_t> parent(n);
    for (uint32_t i = 0; i < n; i++) parent[i] = i;
    auto find = [&](uint32_t x) { while (parent[x] != x) x = parent[x]; return x; };
    Ref r;
    std::vector<std::vector<std::pair<uint32_t, uint32_t>>> adj(n);
    for (auto &[w, lo, hi, s] : order) {
        (void)w;
        const uint32_t a = find(lo), b = find(hi);
        if (a == b) continue;
        parent[std::max(a, b)] = std::min(a, b);
        r.tree.emplace_back(lo, hi);
        adj[lo].emplace_back(hi, s);
        adj[hi].emplace_back(lo, s);
    }
    std::sort(r.tree.begin(), r.tree.end());
    r.comp.assign(n, kNoRow);
    r.par.assign(n, 0);
    for (uint32_t root = 0; root < n; root++) {
        if (r.comp[root] != kNoRow) continue;
        std::vector<uint32_t> stack{root};
        r.comp[root] = root;
        while (!stack.empty()) {
            const uint32_t x = stack.back();
            stack.pop_back();
            for (auto &[y, s] : adj[x])
                if (r.comp[y] == kNoRow) { r.comp[y] = root; r.par[y] = r.par[x] ^ s; stack.push_back(y); }
        }
    }
    return r;
}

static void compare(const char *name, uint32_t n, const std::vector<Edge> &edges, int max_rounds)
{
    const Forest f = boruvka(n, edges);
    const Ref r = kruskal(n, edges);
    CHECK(f.ok);
    std::vector<std::pair<uint32_t, uint32_t>> tree;
    for (size_t t = 0; t + 1 < f.tree.size(); t += 2) tree.emplace_back(f.tree[t], f.tree[t + 1]);
    std::sort(tree.begin(), tree.end());
    CHECK(tree == r.tree);
    CHECK(f.rounds <= max_rounds);
    bool flat = true, same = true;
    for (uint32_t i = 0; i < n && f.ok; i++) {
        const uint32_t root = parent_of(f.words[i]);
        flat &= root < n && parent_of(f.words[root]) == root && parity_of(f.words[root]) == 0;
        if (!flat) break;
        // same component, and the same parity between any row and the component's lowest row
        same &= r.comp[i] == r.comp[root];
        same &= (parity_of(f.words[i]) ^ parity_of(f.words[r.comp[i]])) == r.par[i];
    }
    CHECK(flat);
    CHECK(same);
    std::printf("%-28s n %5u, %6zu listed edges, %5zu tree edges, %2d rounds %s\n", name, n, edges.size(), tree.size(), f.rounds,
                failures ? "FAILED" : "ok");
}

static int ceil_log2(uint32_t n) { int b = 0; while ((1u << b) < n) b++; return b; }

int main()
{
    // all-equal weights on a grid graph, signs at random: the forest is decided by (lo, hi) alone
    {
        const uint32_t side = 24, n = side * side;
        std::vector<Edge> e;
        for (uint32_t y = 0; y < side; y++)
            for (uint32_t x = 0; x < side; x++) {
                if (x + 1 < side) e.push_back({y * side + x, y * side + x + 1, ww_of(0.0f, rnd() & 1)});
                if (y + 1 < side) e.push_back({(y + 1) * side + x, y * side + x, ww_of(0.0f, rnd() & 1)});
            }
        compare("equal weights, grid", n, e, ceil_log2(n));
    }
    // mutual choices: disjoint pairs whose cheapest edge is each other's, then the pairs joined by dearer edges
    {
        const uint32_t n = 512;
        std::vector<Edge> e;
        for (uint32_t i = 0; i + 1 < n; i += 2) e.push_back({i + 1, i, ww_of(0.001f, (i >> 1) & 1)});
        for (uint32_t i = 0; i + 2 < n; i += 2) e.push_back({i, i + 2, ww_of(0.5f + 0.0001f * (float)(rnd() % 1000), rnd() & 1)});
        compare("mutual choices", n, e, ceil_log2(n));
    }
    // a chain with strictly increasing weights: in round one every row chooses the edge below it, the hook graph is one path of n - 1
    // links and the flatten walk uses all of its bound
    {
        const uint32_t n = 300;
        std::vector<Edge> e;
        for (uint32_t i = 0; i + 1 < n; i++) e.push_back({i, i + 1, ww_of(0.001f * (float)(i + 1), i % 3 == 0)});
        compare("deep chain, ascending", n, e, 1);
        for (Edge &x : e) x.ww = ww_of(0.5f - 0.001f * (float)x.u, x.u % 5 == 0);
        compare("deep chain, descending", n, e, 1);
    }
    // isolated vertices, self-loops, edges listed twice and from both ends
    {
        const uint32_t n = 200;
        std::vector<Edge> e;
        for (uint32_t t = 0; t < 300; t++) {
            const uint32_t u = 2 * (rnd() % 80), v = 2 * (rnd() % 80);      // odd rows and rows >= 160 stay isolated
            const uint32_t ww = ww_of(0.01f * (float)(rnd() % 7), rnd() & 1);
            e.push_back({u, v, ww});
        }
        // one sign per undirected pair: the first listing's, as a real graph has
        for (size_t a = 0; a < e.size(); a++)
            for (size_t b = 0; b < a; b++)
                if ((e[a].u == e[b].u && e[a].v == e[b].v) || (e[a].u == e[b].v && e[a].v == e[b].u)) { e[a].ww = e[b].ww; break; }
        const size_t m = e.size();
        for (size_t a = 0; a < m; a += 3) e.push_back({e[a].v, e[a].u, e[a].ww});
        for (uint32_t i = 0; i < n; i += 7) e.push_back({i, i, ww_of(0.0f, true)});
        compare("isolated, loops, duplicates", n, e, ceil_log2(n));
    }
    // random graphs with few distinct weights (many ties) and random signs
    for (int rep = 0; rep < 6; rep++) {
        const uint32_t n = 64 + 97 * (uint32_t)rep;
        std::vector<Edge> e;
        for (uint32_t i = 0; i < n; i++)
            for (int t = 0; t < 3; t++) {
                const uint32_t j = rnd() % n;
                if (j == i) continue;
                bool seen = false;
                for (const Edge &x : e) seen |= (x.u == i && x.v == j) || (x.u == j && x.v == i);
                if (!seen) e.push_back({i, j, ww_of(0.25f * (float)(rnd() % 4), rnd() & 1)});
            }
        compare("random, tied weights", n, e, ceil_log2(n));
    }
    // the weight word: |d| decides the weight, the sign of d the bit; clamped at zero
    {
        const uint32_t a = weight_word(1.f, 0.f, 0.f, 1.f, 0.f, 0.f), b = weight_word(1.f, 0.f, 0.f, -1.f, 0.f, 0.f);
        CHECK(a == 0u && b == kSignBit);
        CHECK(weight_word(0.f, 2.f, 0.f, 0.f, 2.f, 0.f) == 0u);                       // 1 - 4 < 0 -> 0
        CHECK((weight_word(0.f, 0.f, 0.f, 1.f, 0.f, 0.f) & ~kSignBit) == bits_of(1.0f));      // a zero normal: the dearest edge
        CHECK(weight_word(0.6f, 0.f, 0.8f, 0.f, 1.f, 0.f) == bits_of(1.0f));
        CHECK(key64(b, 7u) == 7ull && key64(bits_of(1.0f), 3u) == (((uint64_t)bits_of(1.0f) << 32) | 3ull));
        CHECK(ordered_bits(-1.0f) < ordered_bits(-0.0f) && ordered_bits(-0.0f) < ordered_bits(0.0f) && ordered_bits(0.0f) < ordered_bits(2.0f));
        CHECK(hook_writes(3, 5, false) && hook_writes(5, 3, true) && !hook_writes(3, 5, true));
    }
    // the guard of walk_up: a path of L links needs bound >= L; a cycle is reported at any bound and never loops
    {
        const uint32_t n = 50;
        std::vector<uint32_t> w(n);
        w[0] = pack(0, 0);
        for (uint32_t i = 1; i < n; i++) w[i] = pack(i - 1, i & 1);
        uint32_t out = 0, par = 0;
        for (uint32_t i = 1; i <= 30; i++) par ^= i & 1;
        CHECK(walk_up(w.data(), 30, 30, &out) && out == pack(0, par));
        CHECK(walk_up(w.data(), 30, 1000, &out) && out == pack(0, par));
        CHECK(!walk_up(w.data(), 30, 29, &out) && parent_of(out) == 1);
        CHECK(walk_up(w.data(), 0, 0, &out) && out == pack(0, 0));
        w[0] = pack(n - 1, 1);                                                        // a cycle through every row
        for (uint32_t bound : {0u, 1u, 49u, 50u, 51u, 100000u}) CHECK(!walk_up(w.data(), 7, bound, &out));
        std::printf("%-28s %s\n", "walk guard", failures ? "FAILED" : "ok");
    }
    if (failures) { std::printf("orient_core: %d FAILED\n", failures); return 1; }
    std::printf("orient_core: ok\n");
    return 0;
}
