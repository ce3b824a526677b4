// tests/cpp/myicp_trim.cpp -- MyICP::setTrimFraction (trimmed ICP) through the C++ class.
//
//   myicp_trim <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_trim.py)
//         <dir>/levels.f32                              K triples (leaf, max_iters, max_corr_dist)
// writes  <dir>/out_plain.f32    the 4x4 of PLANE + TREE, 30 iterations, every pair
//         <dir>/out_trim.f32     ... with setTrimFraction(0.5)
//         <dir>/out_levels.f32   ... with setTrimFraction(0.5) and the voxel levels
// and checks by itself (exit code != 0 on failure): a fraction outside (0, 1] and a fraction below 1 with SYMMICP_MODE_QUIRKS are
// SYMMICP_ERR_ARG, the object recovers from both, setTrimFraction(1) gives the bits of the run that never set it, and a trimmed
// run repeated on the same object gives the same bits.
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
    float plain[16], one[16], trim[16], again[16], lev[16];
    CHECK(icp.align(plain) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    icp.setTrimFraction(1.f);                        // off: the same bits
    CHECK(icp.align(one) == SYMMICP_OK);
    CHECK(std::memcmp(plain, one, sizeof(plain)) == 0);

    // refusals, and the object goes on afterwards
    icp.setTrimFraction(0.f);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    CHECK(std::strlen(icp.lastError()) > 0);
    icp.setTrimFraction(1.5f);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setTrimFraction(0.5f);
    icp.setMode(SYMMICP_MODE_QUIRKS);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setMode(SYMMICP_MODE_PLANE);

    CHECK(icp.align(trim) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    CHECK(std::memcmp(trim, icp.getFinalTransformation(), sizeof(trim)) == 0);
    CHECK(std::memcmp(trim, plain, sizeof(trim)) != 0);
    CHECK(icp.align(again) == SYMMICP_OK);
    CHECK(std::memcmp(trim, again, sizeof(trim)) == 0);

    // every level of a coarse-to-fine run is trimmed
    icp.setVoxelLevels(levels);
    CHECK(icp.align(lev) == SYMMICP_OK);
    CHECK(icp.levelResults().size() == levels.size());

    dump(dir + "out_plain.f32", plain, 16);
    dump(dir + "out_trim.f32", trim, 16);
    dump(dir + "out_levels.f32", lev, 16);
    return 0;
}
