// tests/cpp/myicp_eval.cpp -- registration evaluation through the C++ class: MyICP::evaluate, getFitnessScore, evaluateStarts.
//
//   myicp_eval <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_eval.py)
//         <dir>/guesses.f32                             B row-major 4x4 starts for alignMultiStart
//         <dir>/dist.f32                                the evaluation distance
// writes  <dir>/out_align.f64      after a PAPER + tree align(): inliers, fitness, rmse, mean_d2, getFitnessScore(D), getFitnessScore(),
//                                  getFitnessScore(0.1) before the alignment, then the 36 entries of the information matrix
//         <dir>/out_starts.f64     B x (inliers, fitness, rmse) of evaluateStarts
//         <dir>/out_X.f32          the aligned 4x4, then the B transforms of the starts
// and checks by itself (exit code != 0 on failure): evaluateStarts before an alignMultiStart is SYMMICP_ERR_STATE, its results are bit
// for bit those of B single evaluate calls, an evaluation changes neither the final transformation nor the multi-start results, and
// the information matrix is symmicp_information_from_sums of the returned sums.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
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

template <typename T>
static void dump(const std::string &path, const T *p, size_t n)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(p, sizeof(T), n, f) != n) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
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
                             guesses = slurp(dir + "guesses.f32"), dist = slurp(dir + "dist.f32");
    CHECK(src.size() % 3 == 0 && src.size() == src_n.size() && tgt.size() == tgt_n.size() && guesses.size() % 16 == 0 && !guesses.empty() && dist.size() == 1);
    const size_t B = guesses.size() / 16;
    const float D = dist[0];

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations(30);
    icp.setInputSource(src.data(), src_n.data(), src.size() / 3);
    icp.setInputTarget(tgt.data(), tgt_n.data(), tgt.size() / 3);
    // before any alignment the final transformation is the identity: the closest pair of the test's clouds is 0.18 apart
    const double unaligned = icp.getFitnessScore(0.1);
    float X[16];
    CHECK(icp.align(X) == SYMMICP_OK);
    symmicp_evaluation e, e2;
    CHECK(icp.evaluate(D, &e) == SYMMICP_OK);
    CHECK(std::memcmp(X, icp.getFinalTransformation(), sizeof(X)) == 0);
    CHECK(icp.evaluate(D, &e2, X) == SYMMICP_OK && std::memcmp(&e, &e2, sizeof(e)) == 0);      // the default transform is the final one
    double L[36];
    CHECK(symmicp_information_from_sums(e.inliers, e.sum_q, e.sum_qq, L) == SYMMICP_OK && std::memcmp(L, e.information, sizeof(L)) == 0);
    std::vector<double> out = {(double)e.inliers, e.fitness, e.rmse, e.mean_d2, icp.getFitnessScore(D), icp.getFitnessScore(), unaligned};
    out.insert(out.end(), e.information, e.information + 36);
    CHECK(out[4] == e.mean_d2);
    CHECK(out[6] == std::numeric_limits<double>::max());          // nothing within range
    CHECK(icp.evaluate(std::numeric_limits<float>::quiet_NaN(), &e2) == SYMMICP_ERR_ARG && std::strlen(icp.lastError()) > 0);

    // multi-start: every start scored at one distance in one call, equal to single calls
    std::vector<symmicp_evaluation> starts;
    CHECK(icp.evaluateStarts(D, starts) == SYMMICP_ERR_STATE && starts.empty());
    icp.setMaximumIterations(10);
    icp.setDiffThreshold(0.f);
    float best[16];
    CHECK(icp.alignMultiStart(guesses.data(), B, best) == SYMMICP_OK);
    const std::vector<symmicp_batch_result> res = icp.multiStartResults();
    const int winner = icp.bestStart();
    CHECK(icp.evaluateStarts(D, starts) == SYMMICP_OK && starts.size() == B);
    CHECK(icp.bestStart() == winner && std::memcmp(best, icp.getFinalTransformation(), sizeof(best)) == 0);
    CHECK(std::memcmp(res.data(), icp.multiStartResults().data(), sizeof(symmicp_batch_result) * B) == 0);
    std::vector<double> so;
    std::vector<float> xs(X, X + 16);
    for (size_t k = 0; k < B; k++) {
        symmicp_evaluation one;
        CHECK(icp.evaluate(D, &one, res[k].transform) == SYMMICP_OK);
        CHECK(std::memcmp(&one, &starts[k], sizeof(one)) == 0);
        so.push_back((double)starts[k].inliers); so.push_back(starts[k].fitness); so.push_back(starts[k].rmse);
        xs.insert(xs.end(), res[k].transform, res[k].transform + 16);
    }
    dump(dir + "out_align.f64", out.data(), out.size());
    dump(dir + "out_starts.f64", so.data(), so.size());
    dump(dir + "out_X.f32", xs.data(), xs.size());
    return 0;
}
