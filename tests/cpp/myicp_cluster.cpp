// tests/cpp/myicp_cluster.cpp -- MyICP::removeSmallClusters / outliersRemoved through the C++ class.
//
//   myicp_cluster <dir>
// reads   <dir>/src.f32 tgt.f32                  packed float32 [n][3] (written by tests/test_gpu_cluster.py): clouds with stray points
//         <dir>/src_nrm.f32                      packed float32 [n][3]: normals the caller supplies for the source
//         <dir>/src_int.f32 tgt_int.f32          float32 [n]: intensities
//         <dir>/params.f32                       eps, min_size
// writes  <dir>/keep_src.i32 keep_tgt.i32        int32: the rows whose label symmicp_cluster (min_points 1, min_cluster_size) leaves >= 0
//         <dir>/sizes_src.i32                    int32: the sizes of the source's clusters WITHOUT the size filter
//         <dir>/out_src.f32 out_tgt.f32          packed [m][3]: the clouds the class holds after removeSmallClusters
//         <dir>/out_T.f32                        17 floats: status and 4x4 of align() (PAPER, TREE) on the filtered clouds
// Checks by itself (exit code != 0 on failure): the held clouds are the kept rows of the direct call, in order; the counts are
// reported; bad arguments are returned with the clouds unchanged; a second call removes nothing.
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

// the rows the filter keeps, by the C entry called directly
static int kept_rows(const std::vector<float> &xyz, float eps, int min_size, std::vector<int32_t> &rows)
{
    const size_t n = xyz.size() / 3;
    symmicp_cluster_config cfg;
    symmicp_cluster_config_default(&cfg);
    CHECK(cfg.struct_size == sizeof(cfg) && cfg.min_points == 1 && cfg.min_cluster_size == 0 && cfg.max_cluster_size == 0);
    cfg.eps = eps;
    cfg.min_cluster_size = min_size;
    std::vector<int32_t> labels(n), sizes(n);
    size_t clusters = 0;
    CHECK(symmicp_cluster(-1, xyz.data(), 3, 1, n, &cfg, labels.data(), &clusters, sizes.data(), n, nullptr, nullptr) == SYMMICP_OK);
    size_t sum = 0;
    for (size_t k = 0; k < clusters; k++) { CHECK(sizes[k] >= min_size); sum += (size_t)sizes[k]; }
    rows.clear();
    for (size_t i = 0; i < n; i++) if (labels[i] >= 0) rows.push_back((int32_t)i);
    CHECK(sum == rows.size());
    return 0;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 64; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<float> src = slurp(dir + "src.f32"), tgt = slurp(dir + "tgt.f32"), nrm = slurp(dir + "src_nrm.f32"),
                             si = slurp(dir + "src_int.f32"), ti = slurp(dir + "tgt_int.f32"), par = slurp(dir + "params.f32");
    CHECK(src.size() % 3 == 0 && tgt.size() % 3 == 0 && nrm.size() == src.size() && par.size() == 2);
    const size_t ns = src.size() / 3, nt = tgt.size() / 3;
    CHECK(si.size() == ns && ti.size() == nt);
    const float eps = par[0];
    const int min_size = (int)par[1];

    // the entry called directly: the kept rows, and the source's cluster sizes without the filter
    std::vector<int32_t> ks, kt;
    if (kept_rows(src, eps, min_size, ks) || kept_rows(tgt, eps, min_size, kt)) return 1;
    const size_t cs = ks.size(), ct = kt.size();
    CHECK(cs < ns && ct < nt && cs > 0 && ct > 0);
    dump(dir + "keep_src.i32", ks);
    dump(dir + "keep_tgt.i32", kt);
    {
        symmicp_cluster_config cfg;
        symmicp_cluster_config_default(&cfg);
        cfg.eps = eps;
        std::vector<int32_t> labels(ns), sizes;
        size_t clusters = 0;
        CHECK(symmicp_cluster(-1, src.data(), 3, 1, ns, &cfg, labels.data(), &clusters, nullptr, 0, nullptr, nullptr) == SYMMICP_ERR_SIZE);      // the count query
        CHECK(clusters > 0);
        sizes.resize(clusters);
        CHECK(symmicp_cluster(-1, src.data(), 3, 1, ns, &cfg, labels.data(), &clusters, sizes.data(), sizes.size(), nullptr, nullptr) == SYMMICP_OK);
        CHECK(clusters == sizes.size());
        dump(dir + "sizes_src.i32", sizes);
    }

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
    CHECK(icp.removeSmallClusters(0.f, min_size) == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "cluster"));
    CHECK(icp.removeSmallClusters(-1.f, min_size) == SYMMICP_ERR_ARG);
    CHECK(icp.removeSmallClusters(eps, 0) == SYMMICP_ERR_ARG);
    CHECK(icp.removeSmallClusters(eps, -2) == SYMMICP_ERR_ARG);
    CHECK(icp.GetSrcCloud()->points.size() == ns && icp.GetTgtCloud()->points.size() == nt);

    CHECK(icp.removeSmallClusters(eps, min_size) == SYMMICP_OK);
    icp.outliersRemoved(&rs, &rt);
    CHECK(rs == ns - cs && rt == nt - ct);
    const pcl::PointCloud<PointT> &a = *icp.GetSrcCloud(), &b = *icp.GetTgtCloud();
    CHECK(a.points.size() == cs && b.points.size() == ct && a.width == cs && b.width == ct);
    for (size_t j = 0; j < cs; j++) CHECK(std::memcmp(&a.points[j].x, &src[3 * (size_t)ks[j]], 3 * sizeof(float)) == 0);
    for (size_t j = 0; j < ct; j++) CHECK(std::memcmp(&b.points[j].x, &tgt[3 * (size_t)kt[j]], 3 * sizeof(float)) == 0);
    dump(dir + "out_src.f32", packed(a));
    dump(dir + "out_tgt.f32", packed(b));

    // the intensities and the supplied normals followed: a PAPER alignment runs on them
    CHECK(icp.haveIntensities());
    float T[16];
    const int st = icp.align(T);
    if (st != SYMMICP_OK) std::fprintf(stderr, "align: status %d, %s\n", st, icp.lastError());
    CHECK(st == SYMMICP_OK);
    std::vector<float> rec(17);
    rec[0] = (float)st;
    std::memcpy(&rec[1], T, sizeof(T));
    dump(dir + "out_T.f32", rec);

    // again: what is left is made of parts of at least min_size points
    CHECK(icp.removeSmallClusters(eps, min_size) == SYMMICP_OK);
    icp.outliersRemoved(&rs, &rt);
    CHECK(rs == 0 && rt == 0 && icp.GetSrcCloud()->points.size() == cs && icp.GetTgtCloud()->points.size() == ct);
    std::printf("myicp_cluster: ok (source %zu -> %zu, target %zu -> %zu)\n", ns, cs, nt, ct);
    return 0;
}
