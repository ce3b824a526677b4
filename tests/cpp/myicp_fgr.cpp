// tests/cpp/myicp_fgr.cpp -- MyICP::setGlobalInit with GlobalInit::FGR (feature matching and Fast Global Registration before the
// alignment) through the C++ class.
//
//   myicp_fgr <dir>
// reads   <dir>/src.f32 tgt.f32                  packed float32 [n][3] (written by tests/test_gpu_fgr.py)
//         <dir>/src_n.f32 tgt_n.f32              the same for the normals; absent: MyICP estimates them
//         <dir>/truth.f32                        16 floats, row-major 4x4: the true source -> target transform
//         <dir>/params.f32                       fpfh_radius, max_dist, fgr_iterations, seed, voxel_leaf, max_corr_dist, max_iters
// writes  <dir>/out_identity.f32   17 floats: the status and the 4x4 of align() started from the identity (no initialisation)
//         <dir>/out_global.f32     17 floats: the same with setGlobalInit (method FGR)
//         <dir>/out_truth.f32      17 floats: the same without it, started from the truth
//         <dir>/init.f32           16 + 5 floats: the initialisation's transform, its correspondences, accepted tuples, set size,
//                                  iterations, inliers
// PAPER + TREE throughout.  Checks by itself (exit code != 0 on failure): the initialised align succeeds and reports its result,
// RANSAC did not run, a second one gives the same bits, a caller's guess switches the initialisation off, clearGlobalInit does too,
// and an initialisation that cannot succeed is returned from align() with lastError() naming it (no silent identity).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "myicp.h"

static std::vector<float> slurp(const std::string &path, bool optional = false)
{
    std::vector<float> v;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) {
        if (optional) return v;
        std::fprintf(stderr, "cannot open %s\n", path.c_str());
        std::exit(2);
    }
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

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 64; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<float> src = slurp(dir + "src.f32"), tgt = slurp(dir + "tgt.f32"), src_n = slurp(dir + "src_n.f32", true),
                             tgt_n = slurp(dir + "tgt_n.f32", true), truth = slurp(dir + "truth.f32"), par = slurp(dir + "params.f32");
    CHECK(src.size() % 3 == 0 && tgt.size() % 3 == 0 && truth.size() == 16 && par.size() == 7);
    CHECK(src_n.empty() || src_n.size() == src.size());
    CHECK(tgt_n.empty() || tgt_n.size() == tgt.size());

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations((int)par[6]);
    icp.setMaxCorrespondenceDistance(par[5]);
    icp.setInputSource(src.data(), src_n.empty() ? nullptr : src_n.data(), src.size() / 3);
    icp.setInputTarget(tgt.data(), tgt_n.empty() ? nullptr : tgt_n.data(), tgt.size() / 3);

    float T[16];
    int st = icp.align(T);                                      // from the identity: the test expects this to fail or to end far away
    dump(dir + "out_identity.f32", status_and(st, T));

    MyICP::GlobalInit g;
    g.fpfh_radius = par[0]; g.max_dist = par[1]; g.fgr_iterations = (int)par[2]; g.seed = (unsigned long long)par[3]; g.voxel_leaf = par[4];
    g.method = MyICP::GlobalInit::FGR;
    g.hypotheses = 1;                                           // RANSAC's own settings are ignored: one hypothesis would not do
    icp.setGlobalInit(g);
    float G1[16];
    st = icp.align(G1);
    if (st != SYMMICP_OK) std::fprintf(stderr, "align with setGlobalInit: status %d, %s\n", st, icp.lastError());
    CHECK(st == SYMMICP_OK);
    const MyICP::GlobalResult gr = icp.globalResult();
    CHECK(gr.status == SYMMICP_OK && gr.correspondences >= 3 && gr.fgr.inliers >= 3 && gr.fgr.iterations == g.fgr_iterations);
    CHECK(gr.fgr.tuples_accepted >= 1 && gr.fgr.set_size == 3 * (gr.fgr.tuples_accepted < g.fgr_max_tuples ? gr.fgr.tuples_accepted : g.fgr_max_tuples));
    CHECK(gr.ransac.evaluated == 0 && gr.ransac.inliers_final == 0);      // RANSAC was not run
    CHECK(std::memcmp(G1, icp.getFinalTransformation(), sizeof(G1)) == 0 && std::memcmp(G1, icp.lastResult().transform, sizeof(G1)) == 0);
    dump(dir + "out_global.f32", status_and(st, G1));
    std::vector<float> init(gr.transform, gr.transform + 16);
    init.push_back((float)gr.correspondences);
    init.push_back((float)gr.fgr.tuples_accepted);
    init.push_back((float)gr.fgr.set_size);
    init.push_back((float)gr.fgr.iterations);
    init.push_back((float)gr.fgr.inliers);
    dump(dir + "init.f32", init);

    float G2[16];
    CHECK(icp.align(G2) == SYMMICP_OK && std::memcmp(G1, G2, sizeof(G1)) == 0);          // the same bits again
    CHECK(std::memcmp(gr.transform, icp.globalResult().transform, sizeof(gr.transform)) == 0);

    // a caller's guess switches the initialisation off; so does clearGlobalInit
    float A[16], B[16];
    CHECK(icp.align(A, truth.data()) == SYMMICP_OK);
    icp.clearGlobalInit();
    st = icp.align(B, truth.data());
    CHECK(st == SYMMICP_OK && std::memcmp(A, B, sizeof(A)) == 0);
    dump(dir + "out_truth.f32", status_and(st, B));
    float I2[16];
    const int st_id = icp.align(I2);
    const std::vector<float> first = slurp(dir + "out_identity.f32");
    CHECK((float)st_id == first[0] && std::memcmp(I2, &first[1], sizeof(I2)) == 0);

    // an initialisation that cannot succeed: a setting FGR refuses
    MyICP::GlobalInit bad = g;
    bad.fgr_division_factor = 1.0f;
    icp.setGlobalInit(bad);
    float C[16];
    st = icp.align(C);
    CHECK(st == SYMMICP_ERR_ARG && icp.lastResult().status == SYMMICP_ERR_ARG);
    CHECK(std::strstr(icp.lastError(), "global initialisation") && std::strstr(icp.lastError(), "FGR"));
    CHECK(icp.globalResult().status == SYMMICP_ERR_ARG);
    bad = g;
    bad.fpfh_radius = -1.f;
    icp.setGlobalInit(bad);
    CHECK(icp.align(C) == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "FPFH"));
    std::printf("myicp_fgr: ok (%zu correspondences, %u tuples accepted, %u set elements, %d inliers)\n", gr.correspondences, gr.fgr.tuples_accepted,
                gr.fgr.set_size, gr.fgr.inliers);
    return 0;
}
