// tests/cpp/myicp_keypoints.cpp -- MyICP::GlobalInit::iss (ISS keypoints in the global initialisation) through the C++ class.
//
//   myicp_keypoints <dir>
// reads   <dir>/src.f32 tgt.f32                  packed float32 [n][3] (written by tests/test_gpu_iss.py)
//         <dir>/truth.f32                        16 floats, row-major 4x4: the true source -> target transform
//         <dir>/params.f32                       fpfh_radius, max_dist, hypotheses, seed, max_corr_dist, max_iters, iss_salient_radius,
//                                                iss_non_max_radius, a salient radius below the point spacing
// writes  <dir>/out_off.f32        17 floats: the status and the 4x4 of align() with setGlobalInit, iss off
//         <dir>/out_iss.f32        17 floats: the same with iss on
//         <dir>/out_truth.f32      17 floats: align() without initialisation, started from the truth
//         <dir>/init_off.f32 init_iss.f32   16 + 4 floats: the initialisation's transform, its correspondences, source and target
//                                  keypoints, inliers after the refit
// PAPER + TREE throughout, MyICP estimates the normals.  Checks by itself (exit code != 0 on failure): the run with keypoints
// succeeds and reports the counts symmicp_iss_keypoints gives when called directly, its pairs are fewer than the keypoints, a
// second run gives the same bits, the off path reports no keypoints, and radii that leave fewer than 3 keypoints are returned as
// SYMMICP_ERR_NO_CONSENSUS with lastError() naming the step (no silent fall-back to the full cloud).
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

static void dump(const std::string &path, const std::vector<float> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(float), v.size(), f) != v.size()) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

static std::vector<float> status_and(int st, const float *T)
{
    std::vector<float> v(17);
    v[0] = (float)st;
    std::memcpy(&v[1], T, 16 * sizeof(float));
    return v;
}

static std::vector<float> init_record(const MyICP::GlobalResult &gr)
{
    std::vector<float> v(gr.transform, gr.transform + 16);
    v.push_back((float)gr.correspondences);
    v.push_back((float)gr.source_keypoints);
    v.push_back((float)gr.target_keypoints);
    v.push_back((float)gr.ransac.inliers_final);
    return v;
}

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 64; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<float> src = slurp(dir + "src.f32"), tgt = slurp(dir + "tgt.f32"), truth = slurp(dir + "truth.f32"), par = slurp(dir + "params.f32");
    CHECK(src.size() % 3 == 0 && tgt.size() % 3 == 0 && truth.size() == 16 && par.size() == 9);

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations((int)par[5]);
    icp.setMaxCorrespondenceDistance(par[4]);
    icp.setInputSource(src.data(), nullptr, src.size() / 3);
    icp.setInputTarget(tgt.data(), nullptr, tgt.size() / 3);

    MyICP::GlobalInit g;
    g.fpfh_radius = par[0]; g.max_dist = par[1]; g.hypotheses = (unsigned)par[2]; g.seed = (unsigned long long)par[3];
    icp.setGlobalInit(g);                                        // iss off: the path as it was
    float T0[16];
    int st = icp.align(T0);
    CHECK(st == SYMMICP_OK && icp.globalResult().source_keypoints == 0 && icp.globalResult().target_keypoints == 0);
    dump(dir + "out_off.f32", status_and(st, T0));
    dump(dir + "init_off.f32", init_record(icp.globalResult()));

    g.iss = true; g.iss_salient_radius = par[6]; g.iss_non_max_radius = par[7];
    icp.setGlobalInit(g);
    float T1[16];
    st = icp.align(T1);
    if (st != SYMMICP_OK) std::fprintf(stderr, "align with iss: status %d, %s\n", st, icp.lastError());
    CHECK(st == SYMMICP_OK);
    const MyICP::GlobalResult gr = icp.globalResult();
    CHECK(gr.status == SYMMICP_OK && gr.correspondences >= 3 && gr.ransac.inliers_final >= 3);
    CHECK(gr.source_points == src.size() / 3 && gr.target_points == tgt.size() / 3);
    CHECK(gr.correspondences <= gr.source_keypoints && gr.correspondences <= gr.target_keypoints);
    dump(dir + "out_iss.f32", status_and(st, T1));
    dump(dir + "init_iss.f32", init_record(gr));

    // the counts are those of the detector called directly
    symmicp_iss_config ic;
    symmicp_iss_config_default(&ic);
    ic.salient_radius = par[6]; ic.non_max_radius = par[7];
    size_t ks = 0, kt = 0;
    CHECK(symmicp_iss_keypoints(-1, src.data(), 3, 1, src.size() / 3, &ic, nullptr, 0, &ks, nullptr, nullptr) == SYMMICP_ERR_SIZE);
    CHECK(symmicp_iss_keypoints(-1, tgt.data(), 3, 1, tgt.size() / 3, &ic, nullptr, 0, &kt, nullptr, nullptr) == SYMMICP_ERR_SIZE);
    CHECK(ks == gr.source_keypoints && kt == gr.target_keypoints && ks >= 3 && kt >= 3);

    float T2[16];
    CHECK(icp.align(T2) == SYMMICP_OK && std::memcmp(T1, T2, sizeof(T1)) == 0);          // the same bits again
    CHECK(std::memcmp(gr.transform, icp.globalResult().transform, sizeof(gr.transform)) == 0);

    // switching iss off again gives the bits of the first run
    g.iss = false;
    icp.setGlobalInit(g);
    float T3[16];
    CHECK(icp.align(T3) == SYMMICP_OK && std::memcmp(T0, T3, sizeof(T0)) == 0);

    // fewer than 3 keypoints: a salient radius below the spacing leaves every point without neighbours
    g.iss = true; g.iss_salient_radius = par[8]; g.iss_non_max_radius = par[8];
    icp.setGlobalInit(g);
    float C[16];
    st = icp.align(C);
    CHECK(st == SYMMICP_ERR_NO_CONSENSUS && icp.lastResult().status == SYMMICP_ERR_NO_CONSENSUS);
    CHECK(std::strstr(icp.lastError(), "global initialisation") && std::strstr(icp.lastError(), "ISS keypoints"));
    CHECK(icp.globalResult().status == SYMMICP_ERR_NO_CONSENSUS);
    g.iss_salient_radius = -1.f;
    icp.setGlobalInit(g);
    CHECK(icp.align(C) == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "ISS keypoints"));

    icp.clearGlobalInit();
    float B[16];
    st = icp.align(B, truth.data());
    CHECK(st == SYMMICP_OK);
    dump(dir + "out_truth.f32", status_and(st, B));
    std::printf("myicp_keypoints: ok (%zu and %zu keypoints, %zu correspondences, %d inliers)\n", gr.source_keypoints, gr.target_keypoints,
                gr.correspondences, gr.ransac.inliers_final);
    return 0;
}
