// tests/cpp/plane_core.cpp -- the host instantiation of plane_core.h (the draws of stream 2, plane_hypothesis, plane_offset) against
// values written down here.
//
//   plane_core          (no arguments; built and run by tests/test_segplane_abi.py, plain or with -fsanitize=address,undefined)
// Prints one line per group; exit code != 0 on the first failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "plane_core.h"

using namespace symmicp;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

template <class T>
static int hyp(const uint32_t c[3], const T (&a)[3], const T (&b)[3], const T (&cc)[3], const T *axis, T cos_min, T nd[4])
{
    const T P[3][3] = {{a[0], a[1], a[2]}, {b[0], b[1], b[2]}, {cc[0], cc[1], cc[2]}};
    const T none[3] = {0, 0, 0};
    for (int k = 0; k < 4; k++) nd[k] = (T)77;      // (what a status without a plane must leave alone)
    return plane_hypothesis<T>(c, P, axis != nullptr, axis ? axis : none, cos_min, nd);
}

template <class T>
static void hypotheses(const char *name)
{
    const uint32_t ok[3] = {5, 9, 2};
    T nd[4];
    // the draws decide REPEATED before any arithmetic
    const T o[3] = {0, 0, 0}, ex[3] = {1, 0, 0}, ey[3] = {0, 1, 0};
    for (int k = 0; k < 3; k++) {
        uint32_t c[3] = {5, 9, 2};
        c[k] = c[(k + 1) % 3];
        CHECK(hyp<T>(c, o, ex, ey, nullptr, (T)0, nd) == SYMMICP_PLANE_REPEATED && nd[0] == (T)77 && nd[3] == (T)77);
    }
    // the unit triangle: n = +z, d = -0; its mirror image: n = -z
    CHECK(hyp<T>(ok, o, ex, ey, nullptr, (T)0, nd) == SYMMICP_PLANE_EVALUATED);
    CHECK(nd[0] == 0 && nd[1] == 0 && nd[2] == 1 && nd[3] == 0);
    CHECK(hyp<T>(ok, o, ey, ex, nullptr, (T)0, nd) == SYMMICP_PLANE_EVALUATED && nd[2] == -1);
    // u = (1, 0, 0), v = (0, 3, 4): w = (0, -4, 3), |w| = 5; through a = (0, 5, 0): d = -(-0.8 * 5) = 4
    const T a[3] = {0, 5, 0}, b[3] = {1, 5, 0}, c345[3] = {0, 8, 4};
    CHECK(hyp<T>(ok, a, b, c345, nullptr, (T)0, nd) == SYMMICP_PLANE_EVALUATED);
    CHECK(nd[0] == 0 && nd[1] == (T)-4 / (T)5 && nd[2] == (T)3 / (T)5 && nd[3] == (T)4);
    const T on[3] = {7, 5, 0}, above[3] = {-2, 5, 10}, below[3] = {3, 10, 0};
    CHECK(plane_offset<T>(nd, on) == 0 && plane_offset<T>(nd, a) == 0);
    CHECK(plane_offset<T>(nd, above) == (T)10 * ((T)3 / (T)5) && plane_offset<T>(nd, below) == ((T)-4 / (T)5) * (T)10 + (T)4);
    // collinear and coincident samples
    const T two[3] = {2, 0, 0};
    CHECK(hyp<T>(ok, o, ex, two, nullptr, (T)0, nd) == SYMMICP_PLANE_DEGENERATE && nd[0] == (T)77);
    CHECK(hyp<T>(ok, ex, ex, ey, nullptr, (T)0, nd) == SYMMICP_PLANE_DEGENERATE);
    CHECK(hyp<T>(ok, ex, ex, ex, nullptr, (T)0, nd) == SYMMICP_PLANE_DEGENERATE);
    // the sine bound: sin^2 = s^2 / (1 + s^2) against 1e-4
    const T thin[3] = {1, (T)0.01, 0}, wide[3] = {1, (T)0.02, 0};
    CHECK(hyp<T>(ok, o, ex, thin, nullptr, (T)0, nd) == SYMMICP_PLANE_DEGENERATE);
    CHECK(hyp<T>(ok, o, ex, wide, nullptr, (T)0, nd) == SYMMICP_PLANE_EVALUATED && nd[2] == 1);
    // the axis: |n . z| = 0.6 for the 3-4-5 plane; equal to cos_min passes, the next number up does not, and the sign of the axis is ignored
    const T up[3] = {0, 0, 1}, down[3] = {0, 0, -1}, side[3] = {1, 0, 0};
    const T c06 = (T)3 / (T)5;
    CHECK(hyp<T>(ok, a, b, c345, up, c06, nd) == SYMMICP_PLANE_EVALUATED);
    CHECK(hyp<T>(ok, a, b, c345, down, c06, nd) == SYMMICP_PLANE_EVALUATED);
    CHECK(hyp<T>(ok, a, b, c345, up, std::nextafter(c06, (T)1), nd) == SYMMICP_PLANE_OFF_AXIS);
    CHECK(nd[1] == (T)-4 / (T)5 && nd[2] == c06 && nd[3] == (T)4);                     // OFF_AXIS keeps n, d
    CHECK(hyp<T>(ok, a, b, c345, down, std::nextafter(c06, (T)1), nd) == SYMMICP_PLANE_OFF_AXIS);
    CHECK(hyp<T>(ok, a, b, c345, side, (T)1e-30, nd) == SYMMICP_PLANE_OFF_AXIS);     // n . x = 0 exactly
    CHECK(hyp<T>(ok, a, b, c345, side, (T)0, nd) == SYMMICP_PLANE_EVALUATED);
    // REPEATED and DEGENERATE come before the axis
    const uint32_t rep[3] = {4, 4, 1};
    CHECK(hyp<T>(rep, a, b, c345, side, (T)1, nd) == SYMMICP_PLANE_REPEATED);
    CHECK(hyp<T>(ok, o, ex, two, side, (T)1, nd) == SYMMICP_PLANE_DEGENERATE);
    std::printf("%-28s ok\n", name);
}

int main()
{
    // stream 2 of the seed (a pure-Python SplitMix64 gave these)
    CHECK(plane_base(0) == 0x64e497afb5544359ull && plane_base(7) == 0xe7b0d3fdcd6db8b7ull);
    CHECK(plane_base(0) != ransac_base(0) && plane_base(0) != ransac_base_stream1(0));
    const uint32_t d0[9] = {439, 475, 323, 342, 736, 252, 702, 409, 469}, d7[9] = {625, 985, 307, 143, 83, 459, 716, 508, 772};
    for (int i = 0; i < 9; i++) CHECK(ransac_draw(plane_base(0), i, 1000) == d0[i] && ransac_draw(plane_base(7), i, 1000) == d7[i]);
    const uint32_t h1[3] = {1, 2, 0};                      // hypothesis 1 of (seed 0, n = 3): a permutation
    for (int k = 0; k < 3; k++) CHECK(ransac_draw(plane_base(0), 3 + k, 3) == h1[k]);
    for (uint32_t n : {3u, 4u, 2047u, 0x7fffffffu})
        for (int i = 0; i < 2000; i++) CHECK(ransac_draw(plane_base(11), i, n) < n);
    std::printf("%-28s ok\n", "draws");
    hypotheses<float>("hypotheses, float");
    hypotheses<double>("hypotheses, double");
    CHECK(plane_abs(-0.5f) == 0.5f && plane_abs(0.25) == 0.25 && plane_abs(-0.0f) == 0.0f);
    std::printf("plane_core: ok\n");
    return 0;
}
