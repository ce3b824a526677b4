// tests/cpp/myicp_color.cpp -- colored ICP (SYMMICP_MODE_COLOR) through the C++ class.
//
//   myicp_color <dir>
// reads   <dir>/src.f32 src_n.f32 tgt.f32 tgt_n.f32     packed float32 [n][3] (written by tests/test_gpu_color.py)
//         <dir>/src_i.f32 tgt_i.f32                     float32 [n]: one intensity per point
// writes  <dir>/out_color.f32    the 4x4 of COLOR + TREE, 30 iterations, lambda = 0.968 (the default)
//         <dir>/out_half.f32     ... with setColorWeight(0.5)
// and checks by itself (exit code != 0 on failure): COLOR without intensities is SYMMICP_ERR_STATE, with voxel levels and with a
// lambda outside [0, 1] SYMMICP_ERR_ARG, the object recovers from each, setInput* drops the cloud's intensities, a run repeated on
// the same object gives the same bits, and intensities and a colour weight set on a PLANE run change no bit of it.
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
                             src_i = slurp(dir + "src_i.f32"), tgt_i = slurp(dir + "tgt_i.f32");
    CHECK(src.size() % 3 == 0 && src.size() == src_n.size() && tgt.size() == tgt_n.size() && src_i.size() * 3 == src.size() && tgt_i.size() * 3 == tgt.size());
    const size_t ns = src_i.size(), nt = tgt_i.size();

    MyICP icp;
    icp.setVerbose(false);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations(30);
    icp.setDiffThreshold(0.f);                       // every iteration runs
    icp.setInputSource(src.data(), src_n.data(), ns);
    icp.setInputTarget(tgt.data(), tgt_n.data(), nt);

    // off means off: a PLANE run with intensities and a colour weight set is the PLANE run without them
    float plane[16], plane_i[16];
    icp.setMode(SYMMICP_MODE_PLANE);
    const int st_plane = icp.align(plane);
    icp.setSourceIntensity(src_i.data(), ns);
    icp.setTargetIntensity(tgt_i.data(), nt);
    icp.setColorWeight(0.25f);
    CHECK(icp.align(plane_i) == st_plane);
    CHECK(std::memcmp(plane, plane_i, sizeof(plane)) == 0);
    icp.setColorWeight(0.968f);

    // refusals, and the object goes on afterwards
    icp.setMode(SYMMICP_MODE_COLOR);
    icp.setInputSource(src.data(), src_n.data(), ns);            // drops the source's intensities
    CHECK(!icp.haveIntensities());
    CHECK(icp.align(nullptr) == SYMMICP_ERR_STATE);
    CHECK(std::strlen(icp.lastError()) > 0);
    icp.setSourceIntensity(src_i.data(), ns - 1);                // wrong count
    CHECK(icp.align(nullptr) == SYMMICP_ERR_STATE);
    icp.setSourceIntensity(src_i.data(), ns);
    CHECK(icp.haveIntensities());
    icp.setColorWeight(1.5f);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setColorWeight(-0.1f);
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setColorWeight(0.968f);
    icp.setVoxelLevels({{0.05f, 5, 0.f}, {0.f, 5, 0.f}});
    CHECK(icp.align(nullptr) == SYMMICP_ERR_ARG);
    icp.setVoxelLevels({});

    float color[16], again[16], half[16];
    CHECK(icp.align(color) == SYMMICP_OK);
    CHECK(icp.lastResult().iters == 30);
    CHECK(std::memcmp(color, icp.getFinalTransformation(), sizeof(color)) == 0);
    CHECK(icp.align(again) == SYMMICP_OK);
    CHECK(std::memcmp(color, again, sizeof(color)) == 0);
    icp.setColorWeight(0.5f);
    CHECK(icp.align(half) == SYMMICP_OK);
    CHECK(std::memcmp(color, half, sizeof(color)) != 0);

    dump(dir + "out_color.f32", color, 16);
    dump(dir + "out_half.f32", half, 16);
    return 0;
}
