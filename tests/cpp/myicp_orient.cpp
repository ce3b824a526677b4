// tests/cpp/myicp_orient.cpp -- MyICP::setOrientNormals and GlobalInit::orient_k through the C++ class.
//
//   myicp_orient <dir>
// reads   <dir>/src.f32 tgt.f32      packed float32 [n][3] (written by tests/test_gpu_orient.py): two clouds of one surface
// writes  <dir>/src_nrm.f32 tgt_nrm.f32   packed [n][3]: the normals align() ran on with setOrientNormals(16)
// Checks by itself (exit code != 0 on failure): with setOrientNormals(k) the normals the class estimates are the normals pre-step's
// followed by symmicp_orient_normals (bit for bit the two entries called directly), some rows differ in sign from the plain estimate
// and none in anything else; normals the caller supplies stay exactly as supplied; an out-of-range k is SYMMICP_ERR_ARG from align(),
// for setOrientNormals and for GlobalInit::orient_k alike.
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

static std::vector<float> normals_of(const pcl::PointCloud<pcl::PointNormal> &c)
{
    std::vector<float> v(3 * c.points.size());
    for (size_t i = 0; i < c.points.size(); i++) { v[3 * i] = c.points[i].normal_x; v[3 * i + 1] = c.points[i].normal_y; v[3 * i + 2] = c.points[i].normal_z; }
    return v;
}

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); return 1; } \
    } while (0)

static bool same_bits(const std::vector<float> &a, const std::vector<float> &b)
{
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(float)) == 0;
}

// the two entries called directly: k = 10 normals towards the origin, then the orientation over the k-NN graph
static int direct(const std::vector<float> &xyz, int k, std::vector<float> &plain, std::vector<float> &oriented, symmicp_orient_result &res)
{
    const size_t n = xyz.size() / 3;
    plain.assign(3 * n, 0.f);
    oriented.assign(3 * n, 0.f);
    CHECK(symmicp_estimate_normals(-1, xyz.data(), 3, 1, n, 10, nullptr, plain.data(), nullptr) == SYMMICP_OK);
    symmicp_orient_config cfg;
    symmicp_orient_config_default(&cfg);
    CHECK(cfg.struct_size == sizeof(cfg) && cfg.k == 16 && cfg.seed_rule == SYMMICP_ORIENT_VIEWPOINT && cfg.ref[0] == 0.f && cfg.ref[1] == 0.f && cfg.ref[2] == 0.f);
    cfg.k = k;
    CHECK(symmicp_orient_normals(-1, xyz.data(), 3, 1, plain.data(), 3, 1, n, &cfg, oriented.data(), nullptr, nullptr, nullptr, nullptr, &res) == SYMMICP_OK);
    return 0;
}

static void new_icp(MyICP &icp)
{
    icp.setVerbose(false);
    icp.setMode(SYMMICP_MODE_PAPER);
    icp.setCorrespondence(SYMMICP_CORR_TREE);
    icp.setMaximumIterations(2);
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: %s <dir>\n", argv[0]); return 64; }
    const std::string dir = std::string(argv[1]) + "/";
    const std::vector<float> src = slurp(dir + "src.f32"), tgt = slurp(dir + "tgt.f32");
    CHECK(src.size() % 3 == 0 && tgt.size() % 3 == 0 && src.size() >= 60 && tgt.size() >= 60);
    const size_t ns = src.size() / 3, nt = tgt.size() / 3;

    std::vector<float> ps, os, pt, ot;
    symmicp_orient_result rs, rt;
    if (direct(src, 16, ps, os, rs) || direct(tgt, 16, pt, ot, rt)) return 1;
    CHECK(rs.tree_edges + rs.components == ns && rt.tree_edges + rt.components == nt && rs.rounds > 0 && rt.rounds > 0);
    CHECK(rs.flipped > 0 && rs.flipped < ns);                      // (a full model: the viewpoint flip is wrong for part of it)
    for (size_t i = 0; i < 3 * ns; i++) CHECK(os[i] == ps[i] || os[i] == -ps[i]);

    // off (the default): the plain estimate
    {
        MyICP icp;
        new_icp(icp);
        icp.setInputSource(src.data(), nullptr, ns);
        icp.setInputTarget(tgt.data(), nullptr, nt);
        CHECK(icp.align() == SYMMICP_OK);
        CHECK(same_bits(normals_of(*icp.GetSrcPointNormals()), ps) && same_bits(normals_of(*icp.GetTgtPointNormals()), pt));
        icp.setOrientNormals(0);
        CHECK(icp.align() == SYMMICP_OK && same_bits(normals_of(*icp.GetSrcPointNormals()), ps));
    }
    // on: estimated normals are oriented, bit for bit the direct calls
    {
        MyICP icp;
        new_icp(icp);
        icp.setOrientNormals(16);
        icp.setInputSource(src.data(), nullptr, ns);
        icp.setInputTarget(tgt.data(), nullptr, nt);
        CHECK(icp.align() == SYMMICP_OK);
        const std::vector<float> a = normals_of(*icp.GetSrcPointNormals()), b = normals_of(*icp.GetTgtPointNormals());
        CHECK(same_bits(a, os) && same_bits(b, ot) && !same_bits(a, ps));
        dump(dir + "src_nrm.f32", a);
        dump(dir + "tgt_nrm.f32", b);
        // supplied normals stay as supplied (here: the plain estimate, which the orientation would change), the other cloud's are oriented
        icp.setInputSource(src.data(), ps.data(), ns);
        CHECK(icp.align() == SYMMICP_OK);
        CHECK(same_bits(normals_of(*icp.GetSrcPointNormals()), ps) && same_bits(normals_of(*icp.GetTgtPointNormals()), ot));
        icp.setInputSource(src.data(), nullptr, ns);
        icp.setInputTarget(tgt.data(), pt.data(), nt);
        CHECK(icp.align() == SYMMICP_OK);
        CHECK(same_bits(normals_of(*icp.GetSrcPointNormals()), os) && same_bits(normals_of(*icp.GetTgtPointNormals()), pt));
        // an out-of-range k comes back from align()
        icp.setInputTarget(tgt.data(), nullptr, nt);
        for (int bad : {1, 2, 17, -3}) {
            icp.setOrientNormals(bad);
            CHECK(icp.align() == SYMMICP_ERR_ARG && icp.lastResult().status == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "orient"));
        }
        icp.setOrientNormals(16);
        CHECK(icp.align() == SYMMICP_OK);
    }
    // GlobalInit::orient_k: checked by align() the same way
    {
        MyICP icp;
        new_icp(icp);
        icp.setInputSource(src.data(), nullptr, ns);
        icp.setInputTarget(tgt.data(), nullptr, nt);
        MyICP::GlobalInit g;
        CHECK(g.orient_k == 0);
        g.fpfh_radius = 11.05f;
        g.max_dist = 11.05f / 4;
        g.hypotheses = 4000;
        g.orient_k = 17;
        icp.setGlobalInit(g);
        CHECK(icp.align() == SYMMICP_ERR_ARG && icp.globalResult().status == SYMMICP_ERR_ARG && std::strstr(icp.lastError(), "orient"));
    }
    std::printf("myicp_orient: ok (%zu / %zu rows, %llu / %llu flipped, %d / %d rounds)\n", ns, nt, (unsigned long long)rs.flipped,
                (unsigned long long)rt.flipped, rs.rounds, rt.rounds);
    return 0;
}
