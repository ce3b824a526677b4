// tests/cpp/myicp_recip.cpp -- MyICP::setReciprocalCorrespondences (reciprocal correspondences) through the C++ class.
//
//   myicp_recip <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_recip.py)
//         <dir>/levels.f32                              K triples (leaf, max_iters, max_corr_dist)
// writes  <dir>/out_plain.f32    the 4x4 of PLANE + TREE, 30 iterations, every pair
//         <dir>/out_recip.f32    ... with setReciprocalCorrespondences(true)
//         <dir>/out_median.f32   ... and setMedianFactor(2)
//         <dir>/out_levels.f32   ... reciprocal alone with the voxel levels
// and checks by itself (exit code != 0 on failure): the option with SYMMICP_MODE_QUIRKS or SYMMICP_CORR_IDENTITY is SYMMICP_ERR_ARG, the
// object recovers from each, off gives the bits of the run that never set it, setOneToOne on top changes nothing, and a reciprocal run
// repeated on the same object gives the same bits.
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
    float plain[16], off[16], recip[16], again[16], with_o2o[16], med[16], lev[16];
    CHECK(icp.align(plain) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    icp.setReciprocalCorrespondences(false);         // off: the same bits
    CHECK(icp.align(off) == SYMMICP_OK);
    CHECK(std::memcmp(plain, off, sizeof(plain)) == 0);

    // refusals, and the object goes on afterwards
    icp.setReciprocalCorrespondences(true);
    icp.setMode(SYMMICP_MODE_QUIRKS);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    CHECK(std::strlen(icp.lastError()) > 0);
    icp.setMode(SYMMICP_MODE_PLANE);
    icp.setCorrespondence(SYMMICP_CORR_IDENTITY);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setCorrespondence(SYMMICP_CORR_TREE);

    CHECK(icp.align(recip) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    CHECK(std::memcmp(recip, icp.getFinalTransformation(), sizeof(recip)) == 0);
    CHECK(std::memcmp(recip, plain, sizeof(recip)) != 0);
    CHECK(icp.align(again) == SYMMICP_OK);
    CHECK(std::memcmp(recip, again, sizeof(recip)) == 0);
    icp.setOneToOne(true);                           // reciprocal implies it
    CHECK(icp.align(with_o2o) == SYMMICP_OK);
    CHECK(std::memcmp(recip, with_o2o, sizeof(recip)) == 0);
    icp.setOneToOne(false);

    icp.setMedianFactor(2.f);
    CHECK(icp.align(med) == SYMMICP_OK);
    CHECK(std::memcmp(med, recip, sizeof(med)) != 0);
    icp.setMedianFactor(0.f);

    // every level of a coarse-to-fine run is reciprocal
    icp.setVoxelLevels(levels);
    CHECK(icp.align(lev) == SYMMICP_OK);
    CHECK(icp.levelResults().size() == levels.size());

    dump(dir + "out_plain.f32", plain, 16);
    dump(dir + "out_recip.f32", recip, 16);
    dump(dir + "out_median.f32", med, 16);
    dump(dir + "out_levels.f32", lev, 16);
    return 0;
}
