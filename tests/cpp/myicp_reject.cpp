// tests/cpp/myicp_reject.cpp -- MyICP::setOneToOne / setMedianFactor (one-to-one and median-distance rejection) through the C++ class.
//
//   myicp_reject <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_reject.py)
//         <dir>/levels.f32                              K triples (leaf, max_iters, max_corr_dist)
// writes  <dir>/out_plain.f32    the 4x4 of PLANE + TREE, 30 iterations, every pair
//         <dir>/out_unique.f32   ... with setOneToOne(true)
//         <dir>/out_median.f32   ... with setMedianFactor(2)
//         <dir>/out_both.f32     ... with both
//         <dir>/out_levels.f32   ... with both and the voxel levels
// and checks by itself (exit code != 0 on failure): a bad factor, a factor with a trim fraction below 1 and either option with
// SYMMICP_MODE_QUIRKS are SYMMICP_ERR_ARG, the object recovers from each, off (false / 0) gives the bits of the run that never set
// them, and a rejecting run repeated on the same object gives the same bits.
#include <cmath>
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
                             lv = slurp(dir + "levels.f32");
    CHECK(src.size() % 3 == 0 && src.size() == src_n.size() && tgt.size() == tgt_n.size() && lv.size() % 3 == 0 && !lv.empty());
    std::vector<MyICP::VoxelLevel> levels;
    for (size_t k = 0; k < lv.size(); k += 3) levels.push_back({lv[k], (int)lv[k + 1], lv[k + 2]});

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PLANE);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations(30);
    icp.setDiffThreshold(0.f);                       // every iteration runs
    icp.setInputSource(src.data(), src_n.data(), src.size() / 3);
    icp.setInputTarget(tgt.data(), tgt_n.data(), tgt.size() / 3);
    float plain[16], off[16], uniq[16], med[16], both[16], again[16], lev[16];
    CHECK(icp.align(plain) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    icp.setOneToOne(false);                          // off: the same bits
    icp.setMedianFactor(0.f);
    CHECK(icp.align(off) == SYMMICP_OK);
    CHECK(std::memcmp(plain, off, sizeof(plain)) == 0);

    // refusals, and the object goes on afterwards
    const float bad[] = {-1.f, std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()};
    for (float b : bad) {
        icp.setMedianFactor(b);
        CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
        CHECK(std::strlen(icp.lastError()) > 0);
    }
    icp.setMedianFactor(2.f);
    icp.setTrimFraction(0.5f);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);     // the two quantile rules exclude each other
    icp.setTrimFraction(1.f);
    icp.setMode(SYMMICP_MODE_QUIRKS);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setMedianFactor(0.f);
    icp.setOneToOne(true);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setMode(SYMMICP_MODE_PLANE);

    CHECK(icp.align(uniq) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    CHECK(std::memcmp(uniq, icp.getFinalTransformation(), sizeof(uniq)) == 0);
    CHECK(std::memcmp(uniq, plain, sizeof(uniq)) != 0);
    CHECK(icp.align(again) == SYMMICP_OK);
    CHECK(std::memcmp(uniq, again, sizeof(uniq)) == 0);

    icp.setOneToOne(false);
    icp.setMedianFactor(2.f);
    CHECK(icp.align(med) == SYMMICP_OK);
    CHECK(std::memcmp(med, plain, sizeof(med)) != 0 && std::memcmp(med, uniq, sizeof(med)) != 0);

    icp.setOneToOne(true);
    CHECK(icp.align(both) == SYMMICP_OK);
    CHECK(std::memcmp(both, med, sizeof(med)) != 0 && std::memcmp(both, uniq, sizeof(med)) != 0);

    // every level of a coarse-to-fine run rejects
    icp.setVoxelLevels(levels);
    CHECK(icp.align(lev) == SYMMICP_OK);
    CHECK(icp.levelResults().size() == levels.size());

    dump(dir + "out_plain.f32", plain, 16);
    dump(dir + "out_unique.f32", uniq, 16);
    dump(dir + "out_median.f32", med, 16);
    dump(dir + "out_both.f32", both, 16);
    dump(dir + "out_levels.f32", lev, 16);
    return 0;
}
