// examples/icp_align.cpp -- command-line registration of two PCD files on one MI355X through the MyICP class.
//
//   icp_align [options] [source.pcd target.pcd]
//     --mode quirks|paper|plane|gicp|color|ndt  arithmetic: the reference as written (default), the paper-correct symmetric form,
//                              point-to-plane (target normals only: the source's are not estimated), plane-to-plane
//                              (Generalized-ICP, covariances from the normals of both clouds), colored ICP (point-to-plane rows
//                              plus intensity rows: both files need an `intensity` or `rgb` field; no --scale levels), or the
//                              Normal Distributions Transform (source points against the Gaussians of the target's voxels: no
//                              normals, no search; needs --ndt-resolution; no --loss, --trim, rejectors, --scale or --init global)
//     --ndt-resolution L       NDT: the voxel edge, L > 0 (required with --mode ndt)
//     --ndt-neighbors 1|7      NDT: a point meets its own voxel, or that and its six face neighbours (default 7)
//     --ndt-min-points N       NDT: voxels with fewer points carry no Gaussian, N >= 3 (default 6)
//     --ndt-level L:ITERS      NDT: one level of a coarse-to-fine run (repeat it, coarse first): resolution L, at most ITERS
//                              iterations, each level started from the one before (replaces --ndt-resolution and --iters)
//     --color-weight L         colored ICP: the weight of the geometric rows, 0 <= L <= 1 (default 0.968; --mode color only)
//     --gicp-epsilon E         the covariances' eps, 2^-25 < E <= 1: 1 - E must differ from 1 in fp32 (default 1e-3; --mode gicp only)
//     --corr identity|tree     pairing: by row (default, what the reference does) or exact nearest neighbours
//     --iters N                iteration cap            (default 10, ICP/myicp.cpp:6)
//     --loss none|huber|tukey|cauchy|gm   robust loss of the paper loop (default none; not with --mode quirks)
//     --loss-scale S           its scale (PAPER: in units of c = (p - q).(n_p + n_q), about twice the point-to-plane distance;
//                              PLANE: the point-to-plane distance itself; GICP: the pair's Mahalanobis distance)
//     --threshold D            stop once the summed pair distance is <= D   (default 1.0, ICP/myicp.cpp:6)
//     --max-dist D             drop pairs farther apart than D (default 0: keep every pair)
//     --trim F                 trimmed ICP: every pass keeps the closest fraction F of its pairs, 0 < F <= 1 (default 1: all of them;
//                              for clouds that overlap only in part; not with --mode quirks)
//     --one-to-one             of the source points paired with one target point only the closest is kept (not with --mode quirks)
//     --median-factor F        drop pairs farther apart than F times the median pair distance, F > 0 (default 0: off; not with --trim
//                              below 1, not with --mode quirks)
//     --reciprocal             keep a pair only if the source point is also the nearest source point of its target point (implies
//                              --one-to-one; needs --corr tree, not with --mode quirks)
//     --scale LEAF:ITERS[:MAXDIST]   one level of a coarse-to-fine alignment (repeat it, coarse first): both clouds
//                              voxel-downsampled with edge LEAF (0: as given), at most ITERS iterations, pairs farther than
//                              MAXDIST dropped (default 0: none); each level starts from the one before.  Needs --corr tree
//     --init global            start from a global registration instead of the identity: FPFH features of both clouds, their mutual
//                              nearest neighbours in feature space, RANSAC on those matches (clouds any angle apart)
//     --fpfh-radius R          its feature radius (required with --init global; some 8 to 12 point spacings)
//     --ransac-dist D          its inlier distance (required; some 2 point spacings)
//     --ransac-iters H         hypotheses drawn (default 100000)      --seed S   of the draws (default 0)
//     --init fgr               the same with Fast Global Registration in RANSAC's place (a tuple test and a graduated-non-convexity
//                              loop on those matches: no hypothesis count, no lucky sample); takes --fpfh-radius, --seed, --init-voxel and
//                              --init-keypoints as --init global does, and
//     --fgr-dist D             its inlier distance (required; some 2 point spacings)
//     --fgr-iters N            iterations of the loop (default 64)    --fgr-tuples N   tuples kept (default 1000; 0: the tuple test off)
//     --init-voxel L           both clouds voxel-downsampled with edge L for the initialisation (default 0: as given)
//     --init-keypoints iss     match and run RANSAC on the ISS keypoints of both clouds only (features still come from the full clouds)
//     --iss-radius R           their salient radius (required with --init-keypoints iss; some 6 point spacings)
//     --iss-nms-radius R2      their non-maximum radius (default: two thirds of R)   --iss-min-neighbors K   (default 5)
//     --orient-normals K       the normals this program estimates (for the alignment, and for --init global / fgr) are oriented consistently
//                              over each cloud's K-NN graph (3 .. 16; symmicp_ctx_orient_normals, viewpoint at the origin): two scans of one
//                              surface then agree on the side their normals point to, which FPFH matching needs
//     --evaluate D             after the result block, one line with the result's fitness, inlier RMSE and inliers / source points at
//                              distance D (> 0) on the full clouds: the share of source points with a target point within D
//     --information            with --evaluate: also the six rows of the 6x6 information matrix (rotation first, about the origin)
//     --sor K:S                statistical outlier removal of both clouds right after loading: a point goes when its mean distance to
//                              its K nearest neighbours (1 .. 64) exceeds the cloud's mean + S standard deviations
//     --ror R:M                radius outlier removal of both clouds (after --sor when both are given): a point goes with fewer than
//                              M other points within R.  Unless --quiet each filter prints one line with the counts before and after
//     --min-cluster EPS:M      small-cluster removal of both clouds (after --sor and --ror): every connected part of a cloud (points
//                              closer than EPS) with fewer than M points goes -- floating blobs that pass both point filters
//     --remove-plane D[:H[:MIN]]  plane removal of both clouds (after --sor and --ror, before --min-cluster): the points within D of each
//                              cloud's dominant plane go -- the floor or table that joins the objects on it into one cluster.  H RANSAC
//                              hypotheses (default 1000); a plane with fewer than MIN points (default 3) is left alone
//     --plane-axis X,Y,Z:DEG   with --remove-plane: only planes whose normal lies within DEG degrees (0 < DEG <= 90) of the axis
//     --out aligned.pcd        write the source moved by the result (the reference only prints its result; after --sor / --ror / --remove-plane /
//                              --min-cluster the filtered source)
//     --quiet                  no per-iteration lines
//   Without file names it registers cat.pcd to cat_out.pcd from the working directory: the reference's own run.
// Exit code: the symmicp status of the alignment (0 = ok).
//
// The drop-in property itself -- the reference's ICP/main.cpp compiling byte-unchanged against include/myicp.h -- is
// checked in the build container by tests/test_abi.py; this program is the repo's own driver for the same class.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "myicp.h"

static int usage(const char *argv0, const char *complaint)
{
    std::fprintf(stderr, "%s\nusage: %s [--mode quirks|paper|plane|gicp|color|ndt] [--ndt-resolution L] [--ndt-neighbors 1|7] [--ndt-min-points N] [--ndt-level L:ITERS]... [--color-weight L] [--corr identity|tree] [--iters N] [--threshold D] [--loss none|huber|tukey|cauchy|gm]"
                 " [--loss-scale S] [--gicp-epsilon E] [--max-dist D] [--trim F] [--one-to-one] [--reciprocal] [--median-factor F] [--scale LEAF:ITERS[:MAXDIST]]... [--init global --fpfh-radius R --ransac-dist D [--ransac-iters H] [--seed S] [--init-voxel L] [--init-keypoints iss --iss-radius R [--iss-nms-radius R2] [--iss-min-neighbors K]]] [--init fgr --fpfh-radius R --fgr-dist D [--fgr-iters N] [--fgr-tuples N] [--seed S] [--init-voxel L] [--init-keypoints iss ...]] [--orient-normals K] [--evaluate D [--information]] [--sor K:S] [--ror R:M] [--remove-plane D[:H[:MIN]] [--plane-axis X,Y,Z:DEG]] [--min-cluster EPS:M] [--out file.pcd] [--quiet] [source.pcd target.pcd]\n",
                 complaint, argv0);
    return 64;
}

int main(int argc, char **argv)
{
    std::vector<std::string> files;
    std::string out_path;
    MyICP icp;
    bool quirks = true;                      // (the class default)
    int orient_k = 0;
    symmicp_loss loss = SYMMICP_LOSS_NONE;
    float loss_scale = 0.f;
    bool have_scale = false;
    bool gicp = false, have_eps = false;
    float gicp_eps = 0.f;
    bool tree = false;
    bool color = false, have_color_weight = false;
    float color_weight = 0.f;
    float trim = 1.f;
    bool one_to_one = false, reciprocal = false;
    float median_factor = 0.f;
    std::vector<MyICP::VoxelLevel> levels;
    bool init_global = false, have_init_option = false, have_iss_option = false, have_fgr_option = false, have_ransac_option = false;
    MyICP::GlobalInit ginit;
    bool evaluate = false, information = false;
    float eval_dist = 0.f;
    int sor_k = 0, ror_min = 0;              // 0: the filter is off
    float sor_mul = 0.f, ror_radius = 0.f;
    int cluster_min = 0;
    float cluster_eps = 0.f;
    float plane_dist = 0.f, plane_axis[3] = {0.f, 0.f, 0.f}, plane_deg = 0.f;
    int plane_hyp = 1000, plane_min = 3;
    bool have_plane_axis = false;
    bool quiet = false;
    bool ndt = false, have_ndt_option = false;
    float ndt_resolution = 0.f;
    int ndt_neighbors = 7, ndt_min_points = 6;
    std::vector<MyICP::NdtLevel> ndt_levels;
    auto number = [&](const char *what, const char *v, float &out) {
        char *end = nullptr;
        out = std::strtof(v, &end);
        if (end == v || *end || !std::isfinite(out)) { std::fprintf(stderr, "%s needs a number\n", what); std::exit(64); }
    };
    for (int k = 1; k < argc; k++) {
        const std::string a = argv[k];
        auto value = [&](const char *what) -> const char * {
            if (k + 1 >= argc) { std::fprintf(stderr, "%s needs a value\n", what); std::exit(64); }
            return argv[++k];
        };
        if (a == "--mode") {
            const std::string v = value("--mode");
            color = false;
            ndt = false;
            if (v == "ndt") { icp.setMode(SYMMICP_MODE_NDT); quirks = false; gicp = false; ndt = true; }
            else if (v == "quirks") { icp.setMode(SYMMICP_MODE_QUIRKS); quirks = true; gicp = false; }
            else if (v == "paper") { icp.setMode(SYMMICP_MODE_PAPER); quirks = false; gicp = false; }
            else if (v == "plane") { icp.setMode(SYMMICP_MODE_PLANE); quirks = false; gicp = false; }
            else if (v == "gicp") { icp.setMode(SYMMICP_MODE_GICP); quirks = false; gicp = true; }
            else if (v == "color") { icp.setMode(SYMMICP_MODE_COLOR); quirks = false; gicp = false; color = true; }
            else return usage(argv[0], "unknown --mode");
        } else if (a == "--corr") {
            const std::string v = value("--corr");
            if (v == "identity") { icp.setCorrespondence(SYMMICP_CORR_IDENTITY); tree = false; }
            else if (v == "tree") { icp.setCorrespondence(SYMMICP_CORR_TREE); tree = true; }
            else return usage(argv[0], "unknown --corr");
        } else if (a == "--ndt-resolution") {
            number("--ndt-resolution", value("--ndt-resolution"), ndt_resolution);
            if (!(ndt_resolution > 0.f)) return usage(argv[0], "--ndt-resolution needs a length L > 0");
            have_ndt_option = true;
        } else if (a == "--ndt-neighbors") {
            ndt_neighbors = std::atoi(value("--ndt-neighbors"));
            if (ndt_neighbors != 1 && ndt_neighbors != 7) return usage(argv[0], "--ndt-neighbors needs 1 or 7");
            have_ndt_option = true;
        } else if (a == "--ndt-min-points") {
            ndt_min_points = std::atoi(value("--ndt-min-points"));
            if (ndt_min_points < 3) return usage(argv[0], "--ndt-min-points needs N >= 3");
            have_ndt_option = true;
        } else if (a == "--ndt-level") {
            const char *v = value("--ndt-level");
            char *end = nullptr;
            MyICP::NdtLevel lv{0.f, 0};
            lv.resolution = std::strtof(v, &end);
            bool ok = end != v && *end == ':' && std::isfinite(lv.resolution) && lv.resolution > 0.f;
            if (ok) {
                const char *w = end + 1;
                const long it = std::strtol(w, &end, 10);
                ok = end != w && !*end && it >= 0 && it <= 1000000;
                lv.max_iters = (int)it;
            }
            if (!ok) return usage(argv[0], "--ndt-level needs L:ITERS with L > 0 and ITERS >= 0");
            ndt_levels.push_back(lv);
            have_ndt_option = true;
        } else if (a == "--iters") icp.setMaximumIterations(std::atoi(value("--iters")));
        else if (a == "--threshold") icp.setDiffThreshold((float)std::atof(value("--threshold")));
        else if (a == "--loss") {
            const std::string v = value("--loss");
            if (v == "none") loss = SYMMICP_LOSS_NONE;
            else if (v == "huber") loss = SYMMICP_LOSS_HUBER;
            else if (v == "tukey") loss = SYMMICP_LOSS_TUKEY;
            else if (v == "cauchy") loss = SYMMICP_LOSS_CAUCHY;
            else if (v == "gm") loss = SYMMICP_LOSS_GEMAN_MCCLURE;
            else return usage(argv[0], "unknown --loss");
        } else if (a == "--loss-scale") {
            char *end = nullptr;
            const char *v = value("--loss-scale");
            loss_scale = std::strtof(v, &end);
            if (end == v || *end) return usage(argv[0], "--loss-scale needs a number");
            have_scale = true;
        } else if (a == "--gicp-epsilon") {
            char *end = nullptr;
            const char *v = value("--gicp-epsilon");
            gicp_eps = std::strtof(v, &end);
            if (end == v || *end || !std::isfinite(gicp_eps) || !(gicp_eps > 0.f) || gicp_eps > 1.f || 1.0f - gicp_eps == 1.0f)
                return usage(argv[0], "--gicp-epsilon needs a number E with 2^-25 < E <= 1 (1 - E must differ from 1 in fp32)");
            have_eps = true;
        }
        else if (a == "--color-weight") {
            char *end = nullptr;
            const char *v = value("--color-weight");
            color_weight = std::strtof(v, &end);
            if (end == v || *end || !(color_weight >= 0.f) || color_weight > 1.f) return usage(argv[0], "--color-weight needs a number L with 0 <= L <= 1");
            have_color_weight = true;
        }
        else if (a == "--max-dist") {
            char *end = nullptr;
            const char *v = value("--max-dist");
            const float d = std::strtof(v, &end);
            if (end == v || *end || !std::isfinite(d)) return usage(argv[0], "--max-dist needs a number");
            icp.setMaxCorrespondenceDistance(d);
        } else if (a == "--trim") {
            char *end = nullptr;
            const char *v = value("--trim");
            trim = std::strtof(v, &end);
            if (end == v || *end || !(trim > 0.f) || trim > 1.f) return usage(argv[0], "--trim needs a fraction F with 0 < F <= 1");
        } else if (a == "--one-to-one") {
            one_to_one = true;
        } else if (a == "--reciprocal") {
            reciprocal = true;
        } else if (a == "--median-factor") {
            char *end = nullptr;
            const char *v = value("--median-factor");
            median_factor = std::strtof(v, &end);
            if (end == v || *end || !std::isfinite(median_factor) || !(median_factor > 0.f)) return usage(argv[0], "--median-factor needs a number F > 0");
        } else if (a == "--scale") {
            // LEAF:ITERS[:MAXDIST]
            const char *v = value("--scale");
            char *end = nullptr;
            MyICP::VoxelLevel lv{0.f, 0, 0.f};
            lv.leaf = std::strtof(v, &end);
            bool ok = end != v && *end == ':' && std::isfinite(lv.leaf) && lv.leaf >= 0.f;
            if (ok) {
                const char *w = end + 1;
                const long it = std::strtol(w, &end, 10);
                ok = end != w && it >= 0 && it <= 1000000 && (*end == 0 || *end == ':');
                lv.max_iters = (int)it;
            }
            if (ok && *end == ':') {
                const char *w = end + 1;
                lv.max_corr_dist = std::strtof(w, &end);
                ok = end != w && *end == 0 && std::isfinite(lv.max_corr_dist);
            }
            if (!ok) return usage(argv[0], "--scale needs LEAF:ITERS[:MAXDIST] with LEAF >= 0 and ITERS >= 0");
            levels.push_back(lv);
        }
        else if (a == "--init") {
            const std::string v = value("--init");
            if (v == "global") { init_global = true; ginit.method = MyICP::GlobalInit::RANSAC; }
            else if (v == "fgr") { init_global = true; ginit.method = MyICP::GlobalInit::FGR; }
            else if (v == "identity") init_global = false;
            else return usage(argv[0], "unknown --init (global, fgr or identity)");
        }
        else if (a == "--fgr-dist") { number("--fgr-dist", value("--fgr-dist"), ginit.max_dist); have_init_option = true; have_fgr_option = true; }
        else if (a == "--fgr-iters") {
            ginit.fgr_iterations = std::atoi(value("--fgr-iters"));
            if (ginit.fgr_iterations < 1 || ginit.fgr_iterations > 1024) return usage(argv[0], "--fgr-iters needs 1 .. 1024");
            have_init_option = true; have_fgr_option = true;
        }
        else if (a == "--fgr-tuples") {
            const long n = std::atol(value("--fgr-tuples"));
            if (n < 0 || n > (1l << 18)) return usage(argv[0], "--fgr-tuples needs 0 .. 262144 (0: the tuple test off)");
            ginit.fgr_max_tuples = (unsigned)n; have_init_option = true; have_fgr_option = true;
        }
        else if (a == "--fpfh-radius") { number("--fpfh-radius", value("--fpfh-radius"), ginit.fpfh_radius); have_init_option = true; }
        else if (a == "--ransac-dist") { number("--ransac-dist", value("--ransac-dist"), ginit.max_dist); have_init_option = true; have_ransac_option = true; }
        else if (a == "--init-voxel") { number("--init-voxel", value("--init-voxel"), ginit.voxel_leaf); have_init_option = true; }
        else if (a == "--ransac-iters") {
            const long h = std::atol(value("--ransac-iters"));
            if (h < 1 || h > (1l << 24)) return usage(argv[0], "--ransac-iters needs 1 .. 16777216");
            ginit.hypotheses = (unsigned)h; have_init_option = true; have_ransac_option = true;
        }
        else if (a == "--init-keypoints") {
            const std::string v = value("--init-keypoints");
            if (v == "iss") ginit.iss = true;
            else if (v == "none") ginit.iss = false;
            else return usage(argv[0], "unknown --init-keypoints (iss or none)");
            have_init_option = true;
        }
        else if (a == "--iss-radius") { number("--iss-radius", value("--iss-radius"), ginit.iss_salient_radius); have_iss_option = true; }
        else if (a == "--iss-nms-radius") { number("--iss-nms-radius", value("--iss-nms-radius"), ginit.iss_non_max_radius); have_iss_option = true; }
        else if (a == "--iss-min-neighbors") { ginit.iss_min_neighbors = std::atoi(value("--iss-min-neighbors")); have_iss_option = true; }
        else if (a == "--orient-normals") {
            orient_k = std::atoi(value("--orient-normals"));
            if (orient_k < 3 || orient_k > 16) return usage(argv[0], "--orient-normals needs K in 3 .. 16");
        }
        else if (a == "--seed") { ginit.seed = std::strtoull(value("--seed"), nullptr, 10); have_init_option = true; }
        else if (a == "--evaluate") {
            number("--evaluate", value("--evaluate"), eval_dist);
            if (!(eval_dist > 0.f)) return usage(argv[0], "--evaluate needs a distance D > 0");
            evaluate = true;
        }
        else if (a == "--information") information = true;
        else if (a == "--out") out_path = value("--out");
        else if (a == "--sor") {
            // K:S
            const char *v = value("--sor");
            char *end = nullptr;
            const long kk = std::strtol(v, &end, 10);
            bool ok = end != v && *end == ':' && kk >= 1 && kk <= 64;
            if (ok) {
                const char *w = end + 1;
                sor_mul = std::strtof(w, &end);
                ok = end != w && *end == 0 && std::isfinite(sor_mul);
            }
            if (!ok) return usage(argv[0], "--sor needs K:S with 1 <= K <= 64 neighbours and a finite multiplier S");
            sor_k = (int)kk;
        }
        else if (a == "--ror") {
            // R:M
            const char *v = value("--ror");
            char *end = nullptr;
            ror_radius = std::strtof(v, &end);
            bool ok = end != v && *end == ':' && std::isfinite(ror_radius) && ror_radius > 0.f;
            if (ok) {
                const char *w = end + 1;
                const long m = std::strtol(w, &end, 10);
                ok = end != w && *end == 0 && m >= 1 && m <= 0x7fffffffl;
                ror_min = (int)m;
            }
            if (!ok) return usage(argv[0], "--ror needs R:M with a radius R > 0 and M >= 1 neighbours");
        }
        else if (a == "--min-cluster") {
            // EPS:M
            const char *v = value("--min-cluster");
            char *end = nullptr;
            cluster_eps = std::strtof(v, &end);
            bool ok = end != v && *end == ':' && std::isfinite(cluster_eps) && cluster_eps > 0.f;
            if (ok) {
                const char *w = end + 1;
                const long m = std::strtol(w, &end, 10);
                ok = end != w && *end == 0 && m >= 1 && m <= 0x7fffffffl;
                cluster_min = (int)m;
            }
            if (!ok) return usage(argv[0], "--min-cluster needs EPS:M with a distance EPS > 0 and M >= 1 points");
        }
        else if (a == "--remove-plane") {
            // D[:H[:MIN]]
            const char *v = value("--remove-plane");
            char *end = nullptr;
            plane_dist = std::strtof(v, &end);
            bool ok = end != v && (*end == ':' || *end == 0) && std::isfinite(plane_dist) && plane_dist > 0.f;
            if (ok && *end == ':') {
                const char *w = end + 1;
                const long h = std::strtol(w, &end, 10);
                ok = end != w && (*end == ':' || *end == 0) && h >= 1 && h <= (1l << 24);
                plane_hyp = (int)h;
                if (ok && *end == ':') {
                    w = end + 1;
                    const long m = std::strtol(w, &end, 10);
                    ok = end != w && *end == 0 && m >= 0 && m <= 0x7fffffffl;
                    plane_min = (int)m;
                }
            }
            if (!ok) return usage(argv[0], "--remove-plane needs D[:H[:MIN]] with a distance D > 0, 1 <= H <= 16777216 hypotheses and MIN >= 0 points");
        }
        else if (a == "--plane-axis") {
            // X,Y,Z:DEG
            const char *v = value("--plane-axis");
            char *end = nullptr;
            bool ok = true;
            for (int k = 0; k < 3 && ok; k++) {
                plane_axis[k] = std::strtof(v, &end);
                ok = end != v && *end == (k < 2 ? ',' : ':') && std::isfinite(plane_axis[k]);
                v = end + 1;
            }
            if (ok) {
                plane_deg = std::strtof(v, &end);
                ok = end != v && *end == 0 && plane_deg > 0.f && plane_deg <= 90.f;
            }
            ok = ok && (plane_axis[0] != 0.f || plane_axis[1] != 0.f || plane_axis[2] != 0.f);
            if (!ok) return usage(argv[0], "--plane-axis needs X,Y,Z:DEG with a non-zero axis and 0 < DEG <= 90");
            have_plane_axis = true;
        }
        else if (a == "--quiet") { icp.setVerbose(false); quiet = true; }
        else if (!a.empty() && a[0] == '-') return usage(argv[0], ("unknown option " + a).c_str());
        else files.push_back(a);
    }
    if (files.empty()) files = {"cat.pcd", "cat_out.pcd"};
    if (files.size() != 2) return usage(argv[0], "expected two PCD files");
    if (have_plane_axis && !(plane_dist > 0.f)) return usage(argv[0], "--plane-axis needs --remove-plane");
    if (have_ndt_option && !ndt) return usage(argv[0], "--ndt-resolution, --ndt-neighbors, --ndt-min-points and --ndt-level need --mode ndt");
    if (ndt) {
        if (ndt_levels.empty() && !(ndt_resolution > 0.f)) return usage(argv[0], "--mode ndt needs --ndt-resolution L (or --ndt-level L:ITERS)");
        if (loss != SYMMICP_LOSS_NONE || trim < 1.f || one_to_one || reciprocal || median_factor > 0.f)
            return usage(argv[0], "--mode ndt takes no --loss, --trim, --one-to-one, --reciprocal or --median-factor (its weights are the voxel Gaussians')");
        if (!levels.empty() || init_global) return usage(argv[0], "--mode ndt runs neither --scale levels (--ndt-level is its coarse-to-fine) nor --init global");
        icp.setNdt(ndt_levels.empty() ? ndt_resolution : ndt_levels[0].resolution, ndt_neighbors, ndt_min_points);
        icp.setNdtLevels(ndt_levels);
    }
    if (loss != SYMMICP_LOSS_NONE) {
        if (quirks) return usage(argv[0], "--loss needs --mode paper, plane or gicp (quirks is the reference as written)");
        if (!have_scale || !(loss_scale > 0.f) || !std::isfinite(loss_scale)) return usage(argv[0], "--loss needs --loss-scale S with S > 0");
        icp.setRobustLoss(loss, loss_scale);
    }
    if (trim < 1.f) {
        if (quirks) return usage(argv[0], "--trim below 1 needs --mode paper, plane or gicp (quirks is the reference as written)");
        icp.setTrimFraction(trim);
    }
    if (have_color_weight) {
        if (!color) return usage(argv[0], "--color-weight needs --mode color");
        icp.setColorWeight(color_weight);
    }
    if (color && !levels.empty()) return usage(argv[0], "--mode color does not run --scale levels (intensities are not averaged per voxel yet)");
    if (one_to_one || median_factor > 0.f) {
        if (quirks) return usage(argv[0], "--one-to-one and --median-factor need --mode paper, plane or gicp (quirks is the reference as written)");
        if (median_factor > 0.f && trim < 1.f) return usage(argv[0], "--median-factor and --trim below 1 exclude each other");
        icp.setOneToOne(one_to_one);
        icp.setMedianFactor(median_factor);
    }
    if (reciprocal) {
        if (quirks) return usage(argv[0], "--reciprocal needs --mode paper, plane, gicp or color (quirks is the reference as written)");
        if (!tree) return usage(argv[0], "--reciprocal needs --corr tree (identity pairs were never searched)");
        icp.setReciprocalCorrespondences(true);
    }
    if (!levels.empty()) {
        if (!tree) return usage(argv[0], "--scale needs --corr tree (identity pairing cannot pair clouds of different sizes)");
        icp.setVoxelLevels(levels);
    }
    icp.setOrientNormals(orient_k);
    ginit.orient_k = orient_k;
    if (init_global) {
        const bool fgr = ginit.method == MyICP::GlobalInit::FGR;
        if (have_fgr_option && !fgr) return usage(argv[0], "--fgr-dist, --fgr-iters and --fgr-tuples need --init fgr");
        if (have_ransac_option && fgr) return usage(argv[0], "--ransac-dist and --ransac-iters need --init global (--init fgr takes --fgr-dist)");
        if (fgr && !(ginit.fpfh_radius > 0.f && ginit.max_dist > 0.f)) return usage(argv[0], "--init fgr needs --fpfh-radius R and --fgr-dist D, both > 0");
        if (!(ginit.fpfh_radius > 0.f) || !(ginit.max_dist > 0.f)) return usage(argv[0], "--init global needs --fpfh-radius R and --ransac-dist D, both > 0");
        if (ginit.voxel_leaf < 0.f) return usage(argv[0], "--init-voxel needs L >= 0");
        if (!tree) return usage(argv[0], "--init global needs --corr tree (identity pairing assumes the clouds correspond row by row)");
        if (have_iss_option && !ginit.iss) return usage(argv[0], "--iss-radius, --iss-nms-radius and --iss-min-neighbors need --init-keypoints iss");
        if (ginit.iss) {
            if (!(ginit.iss_salient_radius > 0.f)) return usage(argv[0], "--init-keypoints iss needs --iss-radius R > 0");
            if (ginit.iss_non_max_radius == 0.f) ginit.iss_non_max_radius = ginit.iss_salient_radius * (2.0f / 3.0f);
            if (!(ginit.iss_non_max_radius > 0.f)) return usage(argv[0], "--iss-nms-radius needs R2 > 0");
            if (ginit.iss_min_neighbors < 1) return usage(argv[0], "--iss-min-neighbors needs K >= 1");
        }
        icp.setGlobalInit(ginit);
    } else if (have_init_option || have_iss_option) return usage(argv[0], "--fpfh-radius, --ransac-dist, --ransac-iters, --fgr-dist, --fgr-iters, --fgr-tuples, --seed, --init-voxel and --init-keypoints need --init global or --init fgr");
    if (information && !evaluate) return usage(argv[0], "--information needs --evaluate D");
    if (have_eps) {
        if (!gicp) return usage(argv[0], "--gicp-epsilon needs --mode gicp");
        icp.setGicpEpsilon(gicp_eps);
    }

    icp.LoadCloud(files[0], files[1]);
    if (icp.GetSrcCloud()->points.empty() || icp.GetTgtCloud()->points.empty()) {
        std::fprintf(stderr, "%s\n", icp.lastError()[0] ? icp.lastError() : "empty cloud");
        return SYMMICP_ERR_IO;
    }
    if (color && !icp.haveIntensities()) {
        std::fprintf(stderr, "--mode color needs colours in both files: an `intensity` or an `rgb` field per point\n");
        return SYMMICP_ERR_STATE;
    }
    // outlier removal right after loading, the statistical filter first
    for (int f = 0; f < 2; f++) {
        if (f == 0 ? sor_k == 0 : ror_min == 0) continue;
        const size_t ns = icp.GetSrcCloud()->points.size(), nt = icp.GetTgtCloud()->points.size();
        const int st = f == 0 ? icp.removeStatisticalOutliers(sor_k, sor_mul) : icp.removeRadiusOutliers(ror_radius, ror_min);
        if (st != SYMMICP_OK) { std::fprintf(stderr, "%s\n", icp.lastError()); return st; }
        if (!quiet)
            std::printf("%s outlier removal: source %zu -> %zu, target %zu -> %zu\n", f == 0 ? "statistical" : "radius", ns,
                        icp.GetSrcCloud()->points.size(), nt, icp.GetTgtCloud()->points.size());
    }
    if (plane_dist > 0.f) {
        const size_t ns = icp.GetSrcCloud()->points.size(), nt = icp.GetTgtCloud()->points.size();
        const int st = icp.removePlane(plane_dist, plane_hyp, plane_min, plane_axis, plane_deg);
        if (st != SYMMICP_OK) { std::fprintf(stderr, "%s\n", icp.lastError()); return st; }
        if (!quiet) {
            double ps[4], pt[4];
            icp.planeRemoved(ps, pt);
            std::printf("plane removal: source %zu -> %zu, target %zu -> %zu\n", ns, icp.GetSrcCloud()->points.size(), nt,
                        icp.GetTgtCloud()->points.size());
            std::printf("  source plane %.6f %.6f %.6f %.6f  target plane %.6f %.6f %.6f %.6f\n", ps[0], ps[1], ps[2], ps[3], pt[0], pt[1], pt[2], pt[3]);
        }
    }
    if (cluster_min > 0) {
        const size_t ns = icp.GetSrcCloud()->points.size(), nt = icp.GetTgtCloud()->points.size();
        const int st = icp.removeSmallClusters(cluster_eps, cluster_min);
        if (st != SYMMICP_OK) { std::fprintf(stderr, "%s\n", icp.lastError()); return st; }
        if (!quiet)
            std::printf("small cluster removal: source %zu -> %zu, target %zu -> %zu\n", ns, icp.GetSrcCloud()->points.size(), nt,
                        icp.GetTgtCloud()->points.size());
    }
    icp.RegisterSymm();
    const symmicp_result &r = icp.lastResult();
    if (r.status != SYMMICP_OK) return r.status;          // (RegisterSymm has printed lastError(): a failed initialisation among them)

    if (evaluate) {
        symmicp_evaluation e;
        const int st = icp.evaluate(eval_dist, &e);
        if (st != SYMMICP_OK) { std::fprintf(stderr, "%s\n", icp.lastError()); return st; }
        std::printf("Evaluation at %g: fitness %.6f  inlier rmse %.6g  inliers %llu / %zu\n", (double)eval_dist, e.fitness, e.rmse,
                    (unsigned long long)e.inliers, icp.GetSrcCloud()->points.size());
        if (information) {
            std::printf("  information:\n");
            for (int r6 = 0; r6 < 6; r6++) {
                for (int c6 = 0; c6 < 6; c6++) std::printf("%s%.9g", c6 ? " " : "", e.information[6 * r6 + c6]);
                std::printf("\n");
            }
        }
    }

    if (!out_path.empty()) {
        pcl::PointCloud<PointT>::Ptr moved = icp.GetAlignedSrcCloud();
        std::vector<float> xyz(3 * moved->points.size());
        for (size_t i = 0; i < moved->points.size(); i++) { xyz[3 * i] = moved->points[i].x; xyz[3 * i + 1] = moved->points[i].y; xyz[3 * i + 2] = moved->points[i].z; }
        if (symmicp_pcd_write(out_path.c_str(), xyz.data(), nullptr, moved->points.size(), 0) != 0) {
            std::fprintf(stderr, "cannot write %s\n", out_path.c_str());
            return SYMMICP_ERR_IO;
        }
    }
    return 0;
}
