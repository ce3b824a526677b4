// tests/cpp/myicp_voxel.cpp -- MyICP::setVoxelLevels (coarse-to-fine alignment) through the C++ class.
//
//   myicp_voxel <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_multiscale.py)
//         <dir>/guess.f32                               16 floats, row-major 4x4
//         <dir>/levels.f32                              K triples (leaf, max_iters, max_corr_dist)
// writes  <dir>/out.f32          the 4x4 align() returned (PAPER + TREE, the levels, the guess)
//         <dir>/levels_out.f32   K x 16: the transform of every level (levelResults())
//         <dir>/iters.f32        K: the iterations of every level
// and checks by itself (exit code != 0 on failure): out == getFinalTransformation() == lastResult().transform == the last level's,
// a second align on the same object gives the same bits, SYMMICP_CORR_IDENTITY with levels is SYMMICP_ERR_ARG, and clearing the
// levels gives align() without them.
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
                             guess = slurp(dir + "guess.f32"), lv = slurp(dir + "levels.f32");
    CHECK(src.size() % 3 == 0 && src.size() == src_n.size() && tgt.size() == tgt_n.size() && guess.size() == 16 && lv.size() % 3 == 0 && !lv.empty());
    std::vector<MyICP::VoxelLevel> levels;
    for (size_t k = 0; k < lv.size(); k += 3) levels.push_back({lv[k], (int)lv[k + 1], lv[k + 2]});

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setInputSource(src.data(), src_n.data(), src.size() / 3);
    icp.setInputTarget(tgt.data(), tgt_n.data(), tgt.size() / 3);
    icp.setVoxelLevels(levels);
    float out[16];
    CHECK(icp.align(out, guess.data()) == SYMMICP_OK);
    CHECK(std::memcmp(out, icp.getFinalTransformation(), sizeof(out)) == 0);
    CHECK(std::memcmp(out, icp.lastResult().transform, sizeof(out)) == 0);
    const std::vector<symmicp_result> &lr = icp.levelResults();
    CHECK(lr.size() == levels.size());
    CHECK(std::memcmp(out, lr.back().transform, sizeof(out)) == 0);
    std::vector<float> per(16 * lr.size()), iters(lr.size());
    for (size_t k = 0; k < lr.size(); k++) {
        CHECK(lr[k].status == SYMMICP_OK);
        std::memcpy(&per[16 * k], lr[k].transform, sizeof(float) * 16);
        iters[k] = (float)lr[k].iters;
    }
    dump(dir + "out.f32", out, 16);
    dump(dir + "levels_out.f32", per.data(), per.size());
    dump(dir + "iters.f32", iters.data(), iters.size());

    // the same object again: the same bits
    float again[16];
    CHECK(icp.align(again, guess.data()) == SYMMICP_OK);
    CHECK(std::memcmp(out, again, sizeof(out)) == 0);

    // identity pairing cannot pair downsampled clouds
    icp.setCorrespondence(SYMMICP_CORR_IDENTITY);
    CHECK(icp.align(nullptr, guess.data()) == SYMMICP_ERR_ARG);
    CHECK(std::strlen(icp.lastError()) > 0);

    // no levels: align() as without them (one run, max_iters of the object, every pair)
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setVoxelLevels({});
    icp.setMaximumIterations(30);
    CHECK(icp.align(out, guess.data()) == SYMMICP_OK);
    CHECK(icp.levelResults().empty());
    dump(dir + "out_plain.f32", out, 16);
    return 0;
}
