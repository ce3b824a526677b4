// tests/cpp/myicp_multistart.cpp -- MyICP::alignMultiStart (batched multi-start refinement) through the C++ class.
//
//   myicp_multistart <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_batch.py)
//         <dir>/guesses.f32                             B row-major 4x4 guesses
// writes  <dir>/out_best.f32       the adopted 4x4
//         <dir>/out_all.f32        B x (status, iters, pairs, diff_final) as floats, then B x 16 transforms
// and checks by itself (exit code != 0 on failure): one result per guess, the adopted one is the OK result with the most pairs
// (ties: smaller diff_final, then lowest index) and is what getFinalTransformation returns, a second call gives the same bits, and
// QUIRKS, GICP and clouds above SYMMICP_BATCH_MAX_POINTS are refused with the batch call's error (no fallback to a loop).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "myicp.h"

static std::vector<float> slurp(const std::string &path)
{
    std::vector<float> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(float));
    if (std::fread(v.data(), sizeof(float), v.size(), f) != v.size()) { std::fprintf(stderr, "short read on %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
    return v;
}

static void dump(const std::string &path, const float *p, size_t n)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(float), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 64; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<float> src = slurp(dir + "src.f32"), src_n = slurp(dir + "src_n.f32"), tgt = slurp(dir + "tgt.f32"), tgt_n = slurp(dir + "tgt_n.f32"),
                             guesses = slurp(dir + "guesses.f32");
    CHECK(src.size() % 3 == 0 && src.size() == src_n.size() && tgt.size() == tgt_n.size() && guesses.size() % 16 == 0 && !guesses.empty());
    const size_t B = guesses.size() / 16;

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setMaximumIterations(10);
    icp.setDiffThreshold(0.f);                       // every iteration runs
    icp.setInputSource(src.data(), src_n.data(), src.size() / 3);
    icp.setInputTarget(tgt.data(), tgt_n.data(), tgt.size() / 3);
    float best[16], again[16];
    CHECK(icp.alignMultiStart(guesses.data(), B, best) == SYMMICP_OK);
    const std::vector<symmicp_batch_result> res = icp.multiStartResults();
    CHECK(res.size() == B);
    int want = -1;
    for (size_t k = 0; k < B; k++) {
        if (res[k].status != SYMMICP_OK) continue;
        if (want < 0 || res[k].pairs > res[(size_t)want].pairs || (res[k].pairs == res[(size_t)want].pairs && res[k].diff_final < res[(size_t)want].diff_final)) want = (int)k;
    }
    CHECK(want >= 0 && icp.bestStart() == want);
    CHECK(std::memcmp(best, res[(size_t)want].transform, sizeof(best)) == 0);
    CHECK(std::memcmp(best, icp.getFinalTransformation(), sizeof(best)) == 0);
    CHECK(icp.lastResult().iters == res[(size_t)want].iters && icp.lastResult().status == SYMMICP_OK);
    CHECK(icp.alignMultiStart(guesses.data(), B, again) == SYMMICP_OK);
    CHECK(std::memcmp(best, again, sizeof(best)) == 0);
    CHECK(std::memcmp(res.data(), icp.multiStartResults().data(), sizeof(symmicp_batch_result) * B) == 0);

    // refusals: the batch call's error, the final transformation stays, the object goes on
    icp.setMode(SYMMICP_MODE_QUIRKS);
    CHECK(icp.alignMultiStart(guesses.data(), B, nullptr) == SYMMICP_ERR_ARG);
    CHECK(std::strlen(icp.lastError()) > 0 && icp.multiStartResults().empty() && icp.bestStart() == -1);
    icp.setMode(SYMMICP_MODE_GICP);
    CHECK(icp.alignMultiStart(guesses.data(), B, nullptr) == SYMMICP_ERR_ARG);
    icp.setMode(SYMMICP_MODE_PAPER);
    CHECK(icp.alignMultiStart(guesses.data(), 0, nullptr) == SYMMICP_ERR_ARG);
    CHECK(std::memcmp(best, icp.getFinalTransformation(), sizeof(best)) == 0);
    {
        std::vector<float> big(3 * (size_t)(SYMMICP_BATCH_MAX_POINTS + 1));
        for (size_t i = 0; i < big.size(); i++) big[i] = (float)(i % 97) * 0.25f;
        MyICP too_big;
        too_big.setVerbose(false);
        too_big.setMode(SYMMICP_MODE_PAPER);
        too_big.setInputSource(big.data(), big.data(), big.size() / 3);
        too_big.setInputTarget(tgt.data(), tgt_n.data(), tgt.size() / 3);
        CHECK(too_big.alignMultiStart(guesses.data(), B, nullptr) == SYMMICP_ERR_SIZE);
        CHECK(std::strstr(too_big.lastError(), "4096") != nullptr);
    }
    CHECK(icp.alignMultiStart(guesses.data(), B, again) == SYMMICP_OK);
    CHECK(std::memcmp(best, again, sizeof(best)) == 0);

    std::vector<float> all(4 * B + 16 * B);
    for (size_t k = 0; k < B; k++) {
        all[4 * k] = (float)res[k].status; all[4 * k + 1] = (float)res[k].iters; all[4 * k + 2] = (float)res[k].pairs; all[4 * k + 3] = res[k].diff_final;
        std::memcpy(&all[4 * B + 16 * k], res[k].transform, sizeof(float) * 16);
    }
    dump(dir + "out_best.f32", best, 16);
    dump(dir + "out_all.f32", all.data(), all.size());
    return 0;
}
