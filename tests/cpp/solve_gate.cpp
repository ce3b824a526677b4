// solve_gate.cpp -- solve_core.h compiled on the host with both conditioning estimates (test_solve_ref.py builds and runs it).
// stdin: n, then per record: mode, pivot[3], 40 doubles.  stdout per record, for exact_rc = 1 then 0:
//   status rcond pbar[3] qbar[3] a[3] t[3]  (floats as hexadecimal bit patterns, so that "bit-identical" means what it says)
#include <cstdio>
#include <cstring>
#include <cstdint>
#include <initializer_list>
#include "solve_core.h"

static unsigned bits(float v) { unsigned u; std::memcpy(&u, &v, 4); return u; }

int main()
{
    int n = 0;
    if (std::scanf("%d", &n) != 1) return 1;
    for (int i = 0; i < n; i++) {
        int mode;
        float pivot[3];
        symmicp_sums S;
        if (std::scanf("%d %a %a %a", &mode, &pivot[0], &pivot[1], &pivot[2]) != 4) return 1;
        for (int k = 0; k < SYMMICP_NSUM; k++)
            if (std::scanf("%la", &S.s[k]) != 1) return 1;
        for (int ex = 1; ex >= 0; ex--) {
            float pb[3] = {0, 0, 0}, qb[3] = {0, 0, 0}, a[3] = {0, 0, 0}, t[3] = {0, 0, 0}, rc = 0.f, out16[16];
            const int st = mode == SYMMICP_MODE_QUIRKS ? symmicp::solve::solve_quirks(S, pb, qb, a, t, &rc, out16, ex != 0)
                         : mode == SYMMICP_MODE_PLANE  ? symmicp::solve::solve_plane(S, pivot, pb, qb, a, t, &rc, out16, ex != 0)
                                                       : symmicp::solve::solve_paper(S, pivot, pb, qb, a, t, &rc, out16, ex != 0);
            std::printf("%d %08x", st, bits(rc));
            for (const float *v : {pb, qb, a, t})
                for (int k = 0; k < 3; k++) std::printf(" %08x", bits(v[k]));
            std::printf("\n");
        }
    }
    return 0;
}
