// tests/cpp/myicp_ndt.cpp -- SYMMICP_MODE_NDT through the C++ class: MyICP::setNdt and MyICP::setNdtLevels.
//
//   myicp_ndt <dir>
// reads   <dir>/src.f32 tgt.f32        packed float32 [n][3] (written by tests/test_gpu_ndt.py)
//         <dir>/guess.f32              16 floats, row-major 4x4
//         <dir>/levels.f32             K pairs (resolution, max_iters)
// writes  <dir>/out.f32          the 4x4 align() returned (NDT, the levels, the guess)
//         <dir>/levels_out.f32   K x 16: the transform of every level (levelResults())
//         <dir>/iters.f32        K: the iterations of every level
//         <dir>/out_single.f32   the 4x4 of one alignment at the last level's resolution (setNdt, no levels), 12 iterations, neighbours 1
// and checks by itself (exit code != 0 on failure): out == getFinalTransformation() == lastResult().transform == the last level's, a
// second align on the same object gives the same bits, the mode's refusals (a robust loss, a trim fraction, voxel levels, bad setNdt
// values) are SYMMICP_ERR_ARG, and the object goes on to other modes and back.
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
    const std::vector<float> src = slurp(dir + "src.f32"), tgt = slurp(dir + "tgt.f32"), guess = slurp(dir + "guess.f32"), lv = slurp(dir + "levels.f32");
    CHECK(src.size() % 3 == 0 && tgt.size() % 3 == 0 && guess.size() == 16 && lv.size() % 2 == 0 && !lv.empty());
    std::vector<MyICP::NdtLevel> levels;
    for (size_t k = 0; k < lv.size(); k += 2) levels.push_back({lv[k], (int)lv[k + 1]});

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_NDT);
    icp.setInputSource(src.data(), nullptr, src.size() / 3);      // no normals: none are estimated in this mode
    icp.setInputTarget(tgt.data(), nullptr, tgt.size() / 3);
    icp.setNdt(levels[0].resolution);
    icp.setNdtLevels(levels);
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

    // what the mode refuses, each followed by a run that works
    icp.setRobustLoss(SYMMICP_LOSS_HUBER, 0.01f);
    CHECK(icp.align(nullptr, guess.data()) == SYMMICP_ERR_ARG);
    CHECK(std::strlen(icp.lastError()) > 0);
    icp.setRobustLoss(SYMMICP_LOSS_NONE, 0.f);
    icp.setTrimFraction(0.5f);
    CHECK(icp.align(nullptr, guess.data()) == SYMMICP_ERR_ARG);
    icp.setTrimFraction(1.f);
    icp.setVoxelLevels({{0.05f, 5, 0.f}});
    CHECK(icp.align(nullptr, guess.data()) == SYMMICP_ERR_ARG);
    icp.setVoxelLevels({});
    icp.setNdt(levels[0].resolution, 3);
    CHECK(icp.align(nullptr, guess.data()) == SYMMICP_ERR_ARG);
    icp.setNdt(levels[0].resolution, 7, 2);
    CHECK(icp.align(nullptr, guess.data()) == SYMMICP_ERR_ARG);
    icp.setNdt(levels[0].resolution);
    CHECK(icp.align(again, guess.data()) == SYMMICP_OK);
    CHECK(std::memcmp(out, again, sizeof(out)) == 0);

    // another mode on the same object (a context of its own kind), then NDT again without levels
    icp.setMode(SYMMICP_MODE_PLANE);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations(3);
    CHECK(icp.align(again, out) == SYMMICP_OK);
    icp.setMode(SYMMICP_MODE_NDT);
    icp.setNdtLevels({});
    icp.setNdt(levels.back().resolution, 1);
    icp.setMaximumIterations(12);
    icp.setDiffThreshold(0.f);
    CHECK(icp.align(again, nullptr) == SYMMICP_OK);
    CHECK(icp.levelResults().size() == 1 && icp.lastResult().iters == 12);
    dump(dir + "out_single.f32", again, 16);
    return 0;
}
