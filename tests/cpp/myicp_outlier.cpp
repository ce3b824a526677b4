// tests/cpp/myicp_outlier.cpp -- MyICP::removeStatisticalOutliers / removeRadiusOutliers / outliersRemoved through the C++ class.
//
//   myicp_outlier <dir>
// reads   <dir>/src.f32 tgt.f32                  packed float32 [n][3] (written by tests/test_gpu_outlier.py): clouds with stray points
//         <dir>/src_nrm.f32                      packed float32 [n][3]: normals the caller supplies for the source
//         <dir>/src_int.f32 tgt_int.f32          float32 [n]: intensities
//         <dir>/params.f32                       k, std_mul, radius, min_neighbors
// writes  <dir>/sor_src.i32 sor_tgt.i32          int32: the rows symmicp_statistical_outlier_removal keeps, called directly
//         <dir>/out_src.f32 out_tgt.f32          packed [m][3]: the clouds the class holds after removeStatisticalOutliers
//         <dir>/out_T.f32                        17 floats: status and 4x4 of align() (PAPER, TREE) on the filtered clouds
//         <dir>/ror_src.f32                      packed [m2][3]: the source after removeRadiusOutliers on top
// Checks by itself (exit code != 0 on failure): the held clouds are the kept rows of the direct call, in order; the counts are
// reported; bad arguments are returned with the clouds unchanged; identity pairing reports SYMMICP_ERR_SIZE for unequal counts.
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

template <class T>
static void dump(const std::string &path, const std::vector<T> &v)
{
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(v.data(), sizeof(T), v.size(), f) != v.size()) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(2); }
    std::fclose(f);
}

static std::vector<float> packed(const pcl::PointCloud<PointT> &c)
{
    std::vector<float> v(3 * c.points.size());
    for (size_t i = 0; i < c.points.size(); i++) { v[3 * i] = c.points[i].x; v[3 * i + 1] = c.points[i].y; v[3 * i + 2] = c.points[i].z; }
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
    const std::vector<float> src = slurp(dir + "src.f32"), tgt = slurp(dir + "tgt.f32"), nrm = slurp(dir + "src_nrm.f32"),
                             si = slurp(dir + "src_int.f32"), ti = slurp(dir + "tgt_int.f32"), par = slurp(dir + "params.f32");
    CHECK(src.size() % 3 == 0 && tgt.size() % 3 == 0 && nrm.size() == src.size() && par.size() == 4);
    const size_t ns = src.size() / 3, nt = tgt.size() / 3;
    CHECK(si.size() == ns && ti.size() == nt);
    const int k = (int)par[0], min_nb = (int)par[3];
    const float mul = par[1], radius = par[2];

    // the filter called directly
    std::vector<int32_t> ks(ns), kt(nt);
    size_t cs = 0, ct = 0;
    CHECK(symmicp_statistical_outlier_removal(-1, src.data(), 3, 1, ns, k, mul, ks.data(), ns, &cs, nullptr, nullptr) == SYMMICP_OK);
    CHECK(symmicp_statistical_outlier_removal(-1, tgt.data(), 3, 1, nt, k, mul, kt.data(), nt, &ct, nullptr, nullptr) == SYMMICP_OK);
    ks.resize(cs); kt.resize(ct);
    CHECK(cs < ns && ct < nt && cs > 0 && ct > 0);
    dump(dir + "sor_src.i32", ks);
    dump(dir + "sor_tgt.i32", kt);

    MyICP icp;
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations(30);
    icp.setInputSource(src.data(), nrm.data(), ns);
    icp.setInputTarget(tgt.data(), nullptr, nt);
    icp.setSourceIntensity(si.data(), ns);
    icp.setTargetIntensity(ti.data(), nt);
    size_t rs = 7, rt = 7;
    icp.outliersRemoved(&rs, &rt);
    CHECK(rs == 0 && rt == 0);

    // bad arguments: the status comes back, lastError() says why, the clouds stay
    CHECK(icp.removeStatisticalOutliers(0, mul) == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "statistical_outlier_removal"));
    CHECK(icp.removeStatisticalOutliers(65, mul) == SYMMICP_ERR_ARG);
    CHECK(icp.removeRadiusOutliers(-1.f, 3) == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "radius_outlier_removal"));
    CHECK(icp.removeRadiusOutliers(radius, 0) == SYMMICP_ERR_ARG);
    CHECK(icp.GetSrcCloud()->points.size() == ns && icp.GetTgtCloud()->points.size() == nt);

    CHECK(icp.removeStatisticalOutliers(k, mul) == SYMMICP_OK);
    icp.outliersRemoved(&rs, &rt);
    CHECK(rs == ns - cs && rt == nt - ct);
    icp.outliersRemoved(nullptr, nullptr);                        // tolerated
    const pcl::PointCloud<PointT> &a = *icp.GetSrcCloud(), &b = *icp.GetTgtCloud();
    CHECK(a.points.size() == cs && b.points.size() == ct && a.width == cs && b.width == ct);
    for (size_t j = 0; j < cs; j++) CHECK(std::memcmp(&a.points[j].x, &src[3 * (size_t)ks[j]], 3 * sizeof(float)) == 0);
    for (size_t j = 0; j < ct; j++) CHECK(std::memcmp(&b.points[j].x, &tgt[3 * (size_t)kt[j]], 3 * sizeof(float)) == 0);
    dump(dir + "out_src.f32", packed(a));
    dump(dir + "out_tgt.f32", packed(b));

    // the intensities followed (COLOR would refuse clouds and intensities of different lengths), and so did the supplied normals:
    // a PAPER alignment runs on them
    CHECK(icp.haveIntensities());
    float T[16];
    const int st = icp.align(T);
    if (st != SYMMICP_OK) std::fprintf(stderr, "align: status %d, %s\n", st, icp.lastError());
    CHECK(st == SYMMICP_OK);
    std::vector<float> rec(17);
    rec[0] = (float)st;
    std::memcpy(&rec[1], T, sizeof(T));
    dump(dir + "out_T.f32", rec);

    // identity pairing: unequal counts are SYMMICP_ERR_SIZE from align(), as for any two clouds of different sizes
    if (cs != ct) {
        MyICP id;
        id.setVerbose(false);
        id.setInputSource(src.data(), nullptr, ns);
        id.setInputTarget(tgt.data(), nullptr, nt);
        CHECK(id.removeStatisticalOutliers(k, mul) == SYMMICP_OK);
        CHECK(id.align(nullptr) == SYMMICP_ERR_SIZE);
    }

    // the radius filter on top: the counts of the direct call on the clouds as they are now
    const std::vector<float> a0 = packed(a), b0 = packed(b);
    size_t c2s = 0, c2t = 0;
    const int q1 = symmicp_radius_outlier_removal(-1, a0.data(), 3, 1, cs, radius, min_nb, nullptr, 0, &c2s, nullptr);      // count queries
    const int q2 = symmicp_radius_outlier_removal(-1, b0.data(), 3, 1, ct, radius, min_nb, nullptr, 0, &c2t, nullptr);
    CHECK(q1 == (c2s ? SYMMICP_ERR_SIZE : SYMMICP_OK) && q2 == (c2t ? SYMMICP_ERR_SIZE : SYMMICP_OK));
    CHECK(icp.removeRadiusOutliers(radius, min_nb) == SYMMICP_OK);
    icp.outliersRemoved(&rs, &rt);
    CHECK(rs == cs - c2s && rt == ct - c2t);
    CHECK(icp.GetSrcCloud()->points.size() == c2s && icp.GetTgtCloud()->points.size() == c2t);
    dump(dir + "ror_src.f32", packed(*icp.GetSrcCloud()));
    std::printf("myicp_outlier: ok (source %zu -> %zu -> %zu, target %zu -> %zu -> %zu)\n", ns, cs, c2s, nt, ct, c2t);
    return 0;
}
