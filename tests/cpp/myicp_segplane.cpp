// tests/cpp/myicp_segplane.cpp -- MyICP::removePlane / planeRemoved / outliersRemoved through the C++ class.
//
//   myicp_segplane <dir>
// reads   <dir>/src.f32 tgt.f32                  packed float32 [n][3] (written by tests/test_gpu_segplane.py): an object standing on a floor
//         <dir>/src_nrm.f32                      packed float32 [n][3]: normals the caller supplies for the source
//         <dir>/src_int.f32 tgt_int.f32          float32 [n]: intensities
//         <dir>/params.f32                       max_dist, hypotheses
// writes  <dir>/keep_src.i32 keep_tgt.i32        int32: the rows that are NOT final inliers of symmicp_segment_plane (seed 0, one refit)
//         <dir>/planes.f64                       8 doubles: planeRemoved()
//         <dir>/out_src.f32 out_tgt.f32          packed [m][3]: the clouds the class holds after removePlane
//         <dir>/out_T.f32                        17 floats: status and 4x4 of align() (PAPER, TREE) on the edited clouds
// Checks by itself (exit code != 0 on failure): the held clouds are the kept rows of the direct call, in order; the counts and the
// planes are reported; bad arguments are returned with the clouds unchanged; a cloud without a plane of min_inliers points loses nothing.
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

// the rows the edit keeps and the plane, by the C entry called directly
static int kept_rows(const std::vector<float> &xyz, float max_dist, int hypotheses, std::vector<int32_t> &rows, double plane[4])
{
    const size_t n = xyz.size() / 3;
    symmicp_plane_config cfg;
    symmicp_plane_config_default(&cfg);
    CHECK(cfg.struct_size == sizeof(cfg) && cfg.hypotheses == 1000 && cfg.min_inliers == 3 && cfg.refits == 1 && cfg.seed == 0);
    cfg.max_dist = max_dist;
    cfg.hypotheses = (uint32_t)hypotheses;
    float plane4[4];
    symmicp_plane_result res;
    size_t count = 0;
    CHECK(symmicp_segment_plane(-1, xyz.data(), 3, 1, n, &cfg, plane4, &res, nullptr, 0, &count, nullptr, nullptr, nullptr) == SYMMICP_ERR_SIZE);      // the count query
    CHECK(count >= 3 && count < n && (size_t)res.inliers_final == count);
    std::vector<int32_t> on(count);
    CHECK(symmicp_segment_plane(-1, xyz.data(), 3, 1, n, &cfg, plane4, &res, on.data(), count, &count, nullptr, nullptr, nullptr) == SYMMICP_OK);
    for (int a = 0; a < 4; a++) { plane[a] = res.plane[a]; CHECK(plane4[a] == (float)res.plane[a]); }
    rows.clear();
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        if (at < count && (size_t)on[at] == i) at++;
        else rows.push_back((int32_t)i);
    }
    CHECK(at == count && rows.size() == n - count);
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
    const float max_dist = par[0];
    const int hypotheses = (int)par[1];

    std::vector<int32_t> ks, kt;
    double want[2][4];
    if (kept_rows(src, max_dist, hypotheses, ks, want[0]) || kept_rows(tgt, max_dist, hypotheses, kt, want[1])) return 1;
    const size_t cs = ks.size(), ct = kt.size();
    dump(dir + "keep_src.i32", ks);
    dump(dir + "keep_tgt.i32", kt);

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
    double ps[4] = {7, 7, 7, 7}, pt[4] = {7, 7, 7, 7};
    icp.planeRemoved(ps, pt);
    for (int a = 0; a < 4; a++) CHECK(ps[a] == 0.0 && pt[a] == 0.0);

    // bad arguments: the status comes back, lastError() says why, the clouds stay
    const float up[3] = {0.f, 0.f, 1.f};
    CHECK(icp.removePlane(0.f, hypotheses) == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "segment_plane"));
    CHECK(icp.removePlane(-1.f, hypotheses) == SYMMICP_ERR_ARG);
    CHECK(icp.removePlane(max_dist, 0) == SYMMICP_ERR_ARG);
    CHECK(icp.removePlane(max_dist, -5) == SYMMICP_ERR_ARG);
    CHECK(icp.removePlane(max_dist, hypotheses, -1) == SYMMICP_ERR_ARG);
    CHECK(icp.removePlane(max_dist, hypotheses, 3, up, 0.f) == SYMMICP_ERR_ARG);
    CHECK(icp.removePlane(max_dist, hypotheses, 3, up, 91.f) == SYMMICP_ERR_ARG);
    CHECK(icp.GetSrcCloud()->points.size() == ns && icp.GetTgtCloud()->points.size() == nt);

    // no plane of that many points: nothing goes, and that is not an error
    CHECK(icp.removePlane(max_dist, hypotheses, (int)(ns < nt ? ns : nt)) == SYMMICP_OK);
    icp.outliersRemoved(&rs, &rt);
    icp.planeRemoved(ps, pt);
    CHECK(rs == 0 && rt == 0 && icp.GetSrcCloud()->points.size() == ns && icp.GetTgtCloud()->points.size() == nt);
    for (int a = 0; a < 4; a++) CHECK(ps[a] == 0.0 && pt[a] == 0.0);

    // the floor is horizontal: the constraint to 10 degrees about +z finds the same plane
    CHECK(icp.removePlane(max_dist, hypotheses, 3, up, 10.f) == SYMMICP_OK);
    icp.outliersRemoved(&rs, &rt);
    CHECK(rs == ns - cs && rt == nt - ct);
    icp.planeRemoved(ps, pt);
    for (int a = 0; a < 4; a++) CHECK(ps[a] == want[0][a] && pt[a] == want[1][a]);
    CHECK(ps[2] > 0.99 && pt[2] > 0.99);
    dump(dir + "planes.f64", std::vector<double>{ps[0], ps[1], ps[2], ps[3], pt[0], pt[1], pt[2], pt[3]});
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
    std::printf("myicp_segplane: ok (source %zu -> %zu, target %zu -> %zu)\n", ns, cs, nt, ct);
    return 0;
}
