// myicp.cpp -- MyICP on top of the libsymmicp C-ABI (drop-in for reference ICP/myicp.cpp:6-172).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "myicp.h"

MyICP::MyICP() : max_iters(10), diff_threshold(1.f),                       // myicp.cpp:6
                 mode_(SYMMICP_MODE_QUIRKS), corr_(SYMMICP_CORR_IDENTITY), verbose_(true),
                 have_src_normals_(false), have_tgt_normals_(false), loss_(SYMMICP_LOSS_NONE), loss_scale_(0.f), gicp_eps_(1e-3f), trim_fraction_(1.f), one_to_one_(false), reciprocal_(false), median_factor_(0.f), max_corr_dist_(0.f), ctx_(nullptr), ctx_corr_(-1), ctx_no_src_normals_(false)
{
	cloud_src = pcl::PointCloud<PointT>::Ptr(new pcl::PointCloud<PointT>);
	cloud_tgt = pcl::PointCloud<PointT>::Ptr(new pcl::PointCloud<PointT>);
	cloud_pn_src = pcl::PointCloud<pcl::PointNormal>::Ptr(new pcl::PointCloud<pcl::PointNormal>);
	cloud_pn_tgt = pcl::PointCloud<pcl::PointNormal>::Ptr(new pcl::PointCloud<pcl::PointNormal>);
	for (int k = 0; k < 16; k++) transform_[k] = (k % 5 == 0) ? 1.f : 0.f;
	std::memset(&result_, 0, sizeof(result_));
}

MyICP::~MyICP()
{
	if (ctx_) symmicp_destroy(ctx_);
}

// The context is created on first use and kept: a second RegisterSymm / align on the same object reuses its stream, its
// arenas and the loaded code objects.  The correspondence kind decides device layouts, so changing it means a new context.
symmicp_ctx *MyICP::context()
{
	const bool ndt = mode_ == SYMMICP_MODE_NDT;      // (the mode cannot change into or out of NDT on a context that holds clouds)
	if (ctx_ && (ctx_corr_ != (int)corr_ || ctx_ndt_ != ndt)) { symmicp_destroy(ctx_); ctx_ = nullptr; }
	if (!ctx_) {
		symmicp_config cfg;
		symmicp_config_default(&cfg);
		cfg.corr = corr_;
		if (ndt) cfg.mode = SYMMICP_MODE_NDT;
		if (symmicp_create(&cfg, &ctx_) != SYMMICP_OK) { ctx_ = nullptr; return nullptr; }
		ctx_corr_ = (int)corr_;
		ctx_ndt_ = ndt;
		ctx_no_src_normals_ = false;
	}
	return ctx_;
}

static bool load_one(const std::string &path, pcl::PointCloud<PointT> &out)
{
	long n = symmicp_pcd_read(path.c_str(), nullptr, nullptr, 0, nullptr);
	out.points.clear();
	if (n < 0) return false;
	std::vector<float> xyz(3 * (size_t)n);
	if (symmicp_pcd_read(path.c_str(), xyz.data(), nullptr, (size_t)n, nullptr) != n) return false;
	out.points.resize((size_t)n);
	for (long i = 0; i < n; i++) { out.points[i].x = xyz[3 * i]; out.points[i].y = xyz[3 * i + 1]; out.points[i].z = xyz[3 * i + 2]; }
	out.width = (uint32_t)n; out.height = 1;
	return true;
}

// the file's intensities (an `intensity` or `rgb` field), empty when it has none
static void load_intensity(const std::string &path, size_t n, std::vector<float> &out)
{
	out.clear();
	int kind = 0;
	const long m = symmicp_pcd_read_intensity(path.c_str(), nullptr, 0, &kind);
	if (m <= 0 || kind == 0 || (size_t)m != n) return;
	out.resize(n);
	if (symmicp_pcd_read_intensity(path.c_str(), out.data(), n, &kind) != m) out.clear();
}

int MyICP::LoadCloud(std::string src_path, std::string tgt_path)
{
	// myicp.cpp:20-31: x,y,z are kept, other fields dropped; the reference ignores reader status and returns 0
	if (!load_one(src_path, *cloud_src)) error_ = "cannot read " + src_path;
	if (!load_one(tgt_path, *cloud_tgt)) error_ = "cannot read " + tgt_path;
	load_intensity(src_path, cloud_src->points.size(), src_int_);
	load_intensity(tgt_path, cloud_tgt->points.size(), tgt_int_);
	have_src_normals_ = have_tgt_normals_ = false;
	return 0;
}

pcl::PointCloud<PointT>::Ptr MyICP::GetSrcCloud()
{
	return this->cloud_src;
}

pcl::PointCloud<PointT>::Ptr MyICP::GetTgtCloud()
{
	return this->cloud_tgt;
}

void MyICP::RegisterP2P()
{
	// myicp.cpp:43-59: the reference stub prints an identity guess and applies it (a no-op)
	std::cout << "guess matrix:\n1 0 0 0\n0 1 0 0\n0 0 1 0\n0 0 0 1" << std::endl;
}

static void fill_pn(const pcl::PointCloud<PointT> &c, const float *nrm, pcl::PointCloud<pcl::PointNormal> &pn)
{
	pn.points.resize(c.points.size());
	for (size_t i = 0; i < c.points.size(); i++) {
		pcl::PointNormal &p = pn.points[i];
		p.x = c.points[i].x; p.y = c.points[i].y; p.z = c.points[i].z;
		if (nrm) { p.normal_x = nrm[3 * i]; p.normal_y = nrm[3 * i + 1]; p.normal_z = nrm[3 * i + 2]; }
	}
	pn.width = (uint32_t)pn.points.size(); pn.height = 1;
}

void MyICP::setInputSource(const float *xyz, const float *normals, size_t n)
{
	cloud_src->points.resize(n);
	for (size_t i = 0; i < n; i++) { cloud_src->points[i].x = xyz[3 * i]; cloud_src->points[i].y = xyz[3 * i + 1]; cloud_src->points[i].z = xyz[3 * i + 2]; }
	cloud_src->width = (uint32_t)n;
	have_src_normals_ = normals != nullptr;
	src_int_.clear();
	fill_pn(*cloud_src, normals, *cloud_pn_src);
}

void MyICP::setInputTarget(const float *xyz, const float *normals, size_t n)
{
	cloud_tgt->points.resize(n);
	for (size_t i = 0; i < n; i++) { cloud_tgt->points[i].x = xyz[3 * i]; cloud_tgt->points[i].y = xyz[3 * i + 1]; cloud_tgt->points[i].z = xyz[3 * i + 2]; }
	cloud_tgt->width = (uint32_t)n;
	have_tgt_normals_ = normals != nullptr;
	tgt_int_.clear();
	fill_pn(*cloud_tgt, normals, *cloud_pn_tgt);
}

int MyICP::estimateNormals()
{
	int orient_status = SYMMICP_OK;
	// myicp.cpp:152-172: NormalEstimation, KdTree, setKSearch(10), viewpoint (0,0,0), then concatenateFields -- from the
	// clouds as they are NOW, on every call (GetSrcCloud / GetTgtCloud hand out the clouds themselves: a caller may have
	// edited them).  Normals the caller supplied through setInput* are kept.
	struct Job { pcl::PointCloud<PointT> *c; pcl::PointCloud<pcl::PointNormal> *pn; bool have; };
	Job jobs[2] = {{cloud_src.get(), cloud_pn_src.get(), have_src_normals_}, {cloud_tgt.get(), cloud_pn_tgt.get(), have_tgt_normals_}};
	for (Job &j : jobs) {
		const size_t n = j.c->points.size();
		// point-to-plane reads the target's normals only: the source's are not estimated (align() passes none unless the caller did)
		if (mode_ == SYMMICP_MODE_PLANE && j.pn == cloud_pn_src.get() && !j.have) {
			fill_pn(*j.c, nullptr, *j.pn);
			continue;
		}
		if (j.have && j.pn->points.size() == n) {
			for (size_t i = 0; i < n; i++) { j.pn->points[i].x = j.c->points[i].x; j.pn->points[i].y = j.c->points[i].y; j.pn->points[i].z = j.c->points[i].z; }
			continue;
		}
		std::vector<float> nrm(3 * n, 0.f);
		if (n >= 10) {
			symmicp_ctx *ctx = context();
			int st = ctx ? symmicp_ctx_estimate_normals(ctx, &j.c->points[0].x, sizeof(PointT) / sizeof(float), 1, n, 10, nullptr, nrm.data(), nullptr) : SYMMICP_ERR_HIP;
			if (st != SYMMICP_OK) error_ = "symmicp_estimate_normals failed";
			// setOrientNormals: the estimate's signs made consistent along the cloud (never a caller's normals: those took the branch above)
			if (st == SYMMICP_OK && orient_k_ != 0) {
				symmicp_orient_config oc;
				symmicp_orient_config_default(&oc);
				oc.k = orient_k_;
				std::vector<float> out(3 * n);
				st = symmicp_ctx_orient_normals(ctx, &j.c->points[0].x, sizeof(PointT) / sizeof(float), 1, nrm.data(), 3, 1, n, &oc, out.data(), nullptr, nullptr,
				                                nullptr, nullptr, nullptr);
				if (st == SYMMICP_OK) nrm.swap(out);
				else { error_ = std::string("normal orientation: ") + symmicp_last_error(ctx); orient_status = st; }
			}
		}
		fill_pn(*j.c, nrm.data(), *j.pn);
	}
	return orient_status;
}

// Outlier removal: the kept rows of both clouds first (an error leaves both as they were), then every per-point array of each cloud
// compacted in row order.  The point-normal clouds follow only while they still match their clouds row for row.
int MyICP::removeOutliers(int filter, int k, float std_mul, float radius, int min_neighbors)
{
	assert(cloud_src && cloud_tgt);
	removed_src_ = removed_tgt_ = 0;
	symmicp_ctx *ctx = context();
	if (!ctx) { error_ = "symmicp_create failed: no usable gfx950 HIP device (there is no CPU fallback)"; return SYMMICP_ERR_HIP; }
	pcl::PointCloud<PointT> *clouds[2] = {cloud_src.get(), cloud_tgt.get()};
	std::vector<int32_t> rows[2];
	double planes[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
	for (int s = 0; s < 2; s++) {
		const size_t n = clouds[s]->points.size();
		if (n == 0) { error_ = "outlier removal: a cloud is empty"; return SYMMICP_ERR_SIZE; }
		rows[s].resize(n);
		size_t count = 0;
		const float *xyz = &clouds[s]->points[0].x;
		const size_t fs = sizeof(PointT) / sizeof(float);
		int st;
		if (filter == 2) {
			// small clusters: the rows whose label survives the size filter (the labels land in rows[s] and are compacted in place)
			symmicp_cluster_config cfg;
			symmicp_cluster_config_default(&cfg);
			cfg.eps = radius;
			cfg.min_cluster_size = min_neighbors;
			size_t clusters = 0;
			if (min_neighbors < 1) { error_ = "cluster: min_size must be >= 1"; return SYMMICP_ERR_ARG; }
			st = symmicp_ctx_cluster(ctx, xyz, fs, 1, n, &cfg, rows[s].data(), &clusters, nullptr, 0, nullptr, nullptr);
			if (st == SYMMICP_ERR_SIZE) st = SYMMICP_OK;      // (the sizes were not asked for: the labels are written)
			if (st == SYMMICP_OK)
				for (size_t i = 0; i < n; i++) if (rows[s][i] >= 0) rows[s][count++] = (int32_t)i;
		} else if (filter == 3) {
			// the dominant plane: the rows that are NOT among its final inliers; a cloud without a plane keeps every row
			std::vector<int32_t> on(n);
			float plane4[4];
			symmicp_plane_result res;
			size_t on_count = 0;
			st = symmicp_ctx_segment_plane(ctx, xyz, fs, 1, n, &plane_cfg_, plane4, &res, on.data(), n, &on_count, nullptr, nullptr, nullptr);
			if (st == SYMMICP_ERR_NO_CONSENSUS) { st = SYMMICP_OK; on_count = 0; }
			if (st == SYMMICP_OK) {
				for (int a = 0; a < 4; a++) planes[s][a] = res.plane[a];
				size_t at = 0;
				for (size_t i = 0; i < n; i++) {
					if (at < on_count && (size_t)on[at] == i) at++;
					else rows[s][count++] = (int32_t)i;
				}
			}
		} else {
			st = filter == 0 ? symmicp_ctx_statistical_outlier_removal(ctx, xyz, fs, 1, n, k, std_mul, rows[s].data(), n, &count, nullptr, nullptr)
			                 : symmicp_ctx_radius_outlier_removal(ctx, xyz, fs, 1, n, radius, min_neighbors, rows[s].data(), n, &count, nullptr);
		}
		if (st != SYMMICP_OK) { error_ = symmicp_last_error(ctx); return st; }
		rows[s].resize(count);
	}
	pcl::PointCloud<pcl::PointNormal> *pns[2] = {cloud_pn_src.get(), cloud_pn_tgt.get()};
	std::vector<float> *ints[2] = {&src_int_, &tgt_int_};
	for (int s = 0; s < 2; s++) {
		const size_t n = clouds[s]->points.size(), m = rows[s].size();
		const bool with_pn = pns[s]->points.size() == n, with_int = ints[s]->size() == n;
		for (size_t j = 0; j < m; j++) {      // rows ascend: rows[j] >= j, so the copy never reads a slot it has written
			const size_t i = (size_t)rows[s][j];
			clouds[s]->points[j] = clouds[s]->points[i];
			if (with_pn) pns[s]->points[j] = pns[s]->points[i];
			if (with_int) (*ints[s])[j] = (*ints[s])[i];
		}
		clouds[s]->points.resize(m);
		clouds[s]->width = (uint32_t)m; clouds[s]->height = 1;
		if (with_pn) { pns[s]->points.resize(m); pns[s]->width = (uint32_t)m; pns[s]->height = 1; }
		if (with_int) ints[s]->resize(m);
		(s == 0 ? removed_src_ : removed_tgt_) = n - m;
	}
	if (filter == 3) std::memcpy(planes_, planes, sizeof(planes_));
	return SYMMICP_OK;
}

int MyICP::removeStatisticalOutliers(int k, float std_mul)
{
	return removeOutliers(0, k, std_mul, 0.f, 0);
}

int MyICP::removeRadiusOutliers(float radius, int min_neighbors)
{
	return removeOutliers(1, 0, 0.f, radius, min_neighbors);
}

int MyICP::removeSmallClusters(float eps, int min_size)
{
	return removeOutliers(2, 0, 0.f, eps, min_size);
}

int MyICP::removePlane(float max_dist, int hypotheses, int min_inliers, const float axis[3], float max_angle_deg)
{
	symmicp_plane_config_default(&plane_cfg_);
	plane_cfg_.max_dist = max_dist;
	plane_cfg_.hypotheses = hypotheses < 0 ? 0u : (uint32_t)hypotheses;
	plane_cfg_.min_inliers = min_inliers;
	for (int a = 0; a < 3; a++) plane_cfg_.axis[a] = axis ? axis[a] : 0.f;
	plane_cfg_.max_angle_deg = max_angle_deg;
	return removeOutliers(3, 0, 0.f, 0.f, 0);
}

int MyICP::align(float out4x4[16], const float *guess4x4)
{
	assert(cloud_src && cloud_tgt);                                        // myicp.cpp:102
	if (mode_ == SYMMICP_MODE_NDT) return alignNdt(out4x4, guess4x4);       // (no normals pre-step, no index)
	const bool source_normals = mode_ != SYMMICP_MODE_PLANE || have_src_normals_;
	if (ctx_ && ctx_no_src_normals_ && mode_ != SYMMICP_MODE_PLANE) { symmicp_destroy(ctx_); ctx_ = nullptr; }   // (it would refuse the mode)
	symmicp_ctx *ctx = context();
	if (!ctx) { error_ = "symmicp_create failed: no usable gfx950 HIP device (there is no CPU fallback)"; result_.status = SYMMICP_ERR_HIP; return SYMMICP_ERR_HIP; }
	if (int ost = estimateNormals()) { result_.status = ost; return ost; }  // myicp.cpp:105 (only setOrientNormals can fail it)
	symmicp_config cfg;
	symmicp_config_default(&cfg);
	cfg.mode = mode_; cfg.corr = corr_; cfg.max_iters = max_iters; cfg.diff_threshold = diff_threshold;
	cfg.verbose = verbose_ ? 1 : 0;
	cfg.max_corr_dist = max_corr_dist_;
	int st = symmicp_set_robust_loss(ctx, SYMMICP_LOSS_NONE, 0.f);        // (the context may carry a loss into a QUIRKS config)
	if (st == SYMMICP_OK) st = symmicp_set_trim_fraction(ctx, 1.f);        // (... or a trim fraction)
	if (st == SYMMICP_OK) st = symmicp_set_one_to_one(ctx, 0);             // (... or a rejector)
	if (st == SYMMICP_OK) st = symmicp_set_median_factor(ctx, 0.f);
	if (st == SYMMICP_OK) st = symmicp_set_reciprocal(ctx, 0);
	if (st == SYMMICP_OK) st = symmicp_set_config(ctx, &cfg);
	if (st == SYMMICP_OK) st = symmicp_set_trim_fraction(ctx, trim_fraction_);        // ERR_ARG: outside (0, 1], or below 1 with QUIRKS
	if (st == SYMMICP_OK) st = symmicp_set_one_to_one(ctx, one_to_one_ ? 1 : 0);      // ERR_ARG: with QUIRKS
	if (st == SYMMICP_OK) st = symmicp_set_reciprocal(ctx, reciprocal_ ? 1 : 0);      // ERR_ARG: with QUIRKS or identity pairing
	if (st == SYMMICP_OK) st = symmicp_set_median_factor(ctx, median_factor_);        // ERR_ARG: not 0 or finite and > 0, with QUIRKS, or with a trim fraction below 1
	if (st == SYMMICP_OK) st = symmicp_set_robust_loss(ctx, loss_, loss_scale_);      // ERR_ARG: a loss with QUIRKS, or a bad scale
	if (st == SYMMICP_OK) st = symmicp_set_gicp_epsilon(ctx, gicp_eps_);              // ERR_ARG: eps outside (0, 1]
	if (st == SYMMICP_OK) st = symmicp_set_color_weight(ctx, color_weight_);          // ERR_ARG: lambda outside [0, 1]
	if (st == SYMMICP_OK && mode_ == SYMMICP_MODE_COLOR && !levels_.empty()) {
		error_ = "SYMMICP_MODE_COLOR does not run voxel levels (intensities are not averaged per voxel yet)";
		result_.status = SYMMICP_ERR_ARG;
		return SYMMICP_ERR_ARG;
	}
	const size_t fs = sizeof(pcl::PointNormal) / sizeof(float);            // pasteInMatrix, func.cpp:5-15
	level_results_.clear();
	if (st == SYMMICP_OK && have_global_ && !guess4x4) {
		st = globalInit(ctx);
		if (st != SYMMICP_OK) {
			result_.status = st;
			if (out4x4) std::memcpy(out4x4, transform_, sizeof(transform_));
			return st;
		}
		guess4x4 = global_result_.transform;
	}
	if (st == SYMMICP_OK && !levels_.empty()) {
		st = alignLevels(cfg, source_normals, guess4x4);
		if (result_.iters > 0 || st == SYMMICP_OK) std::memcpy(transform_, result_.transform, sizeof(transform_));
		if (out4x4) std::memcpy(out4x4, transform_, sizeof(transform_));
		return st;
	}
	if (st == SYMMICP_OK) {
		if (!cloud_pn_tgt->points.empty() && !cloud_pn_src->points.empty()) {
			st = symmicp_set_target(ctx, &cloud_pn_tgt->points[0].x, fs, 1, &cloud_pn_tgt->points[0].normal_x, fs, 1, cloud_pn_tgt->points.size());
			if (st == SYMMICP_OK) {
				st = symmicp_set_source(ctx, &cloud_pn_src->points[0].x, fs, 1, source_normals ? &cloud_pn_src->points[0].normal_x : nullptr, fs, 1,
				                        cloud_pn_src->points.size());
				ctx_no_src_normals_ = st == SYMMICP_OK && !source_normals;
			}
			if (st == SYMMICP_OK && mode_ == SYMMICP_MODE_COLOR) {
				st = setColorAttributes(ctx);
				if (st != SYMMICP_OK) {
					result_.status = st;
					if (out4x4) std::memcpy(out4x4, transform_, sizeof(transform_));
					return st;
				}
			}
		} else {
			st = SYMMICP_ERR_SIZE;
		}
	}
	if (st == SYMMICP_OK) st = symmicp_align(ctx, guess4x4, &result_);
	else result_.status = st;
	if (st != SYMMICP_OK) error_ = symmicp_last_error(ctx);
	if (result_.iters > 0 || st == SYMMICP_OK) std::memcpy(transform_, result_.transform, sizeof(transform_));
	if (out4x4) std::memcpy(out4x4, transform_, sizeof(transform_));
	return st;
}

// SYMMICP_MODE_NDT: the clouds as they are (no normals), the options the mode refuses applied so that the library says so, then one
// alignment per level -- symmicp_set_ndt, symmicp_set_config (the level's iterations), symmicp_align from the level before.
int MyICP::alignNdt(float out4x4[16], const float *guess4x4)
{
	auto done = [&](int st) {
		if (st != SYMMICP_OK) result_.status = st;
		if (out4x4) std::memcpy(out4x4, transform_, sizeof(transform_));
		return st;
	};
	level_results_.clear();
	symmicp_ctx *ctx = context();
	if (!ctx) { error_ = "symmicp_create failed: no usable gfx950 HIP device (there is no CPU fallback)"; return done(SYMMICP_ERR_HIP); }
	if (!levels_.empty() || have_global_) {
		error_ = "SYMMICP_MODE_NDT runs neither voxel levels (setNdtLevels is its coarse-to-fine) nor the global initialisation";
		return done(SYMMICP_ERR_ARG);
	}
	if (cloud_src->points.empty() || cloud_tgt->points.empty()) { error_ = "a cloud is empty"; return done(SYMMICP_ERR_SIZE); }
	std::vector<NdtLevel> levels = ndt_levels_;
	if (levels.empty()) levels.push_back(NdtLevel{ndt_resolution_, max_iters});
	symmicp_config cfg;
	symmicp_config_default(&cfg);
	cfg.mode = SYMMICP_MODE_NDT; cfg.corr = corr_; cfg.diff_threshold = diff_threshold;
	cfg.max_corr_dist = max_corr_dist_;
	cfg.max_iters = levels[0].max_iters; cfg.verbose = 0;
	symmicp_ndt_config ncfg;
	symmicp_ndt_config_default(&ncfg);
	ncfg.resolution = levels[0].resolution; ncfg.neighbors = ndt_neighbors_; ncfg.min_points = ndt_min_points_;
	int st = symmicp_set_config(ctx, &cfg);
	if (st == SYMMICP_OK) st = symmicp_set_trim_fraction(ctx, trim_fraction_);        // ERR_ARG below 1: NDT takes none of these
	if (st == SYMMICP_OK) st = symmicp_set_one_to_one(ctx, one_to_one_ ? 1 : 0);
	if (st == SYMMICP_OK) st = symmicp_set_reciprocal(ctx, reciprocal_ ? 1 : 0);
	if (st == SYMMICP_OK) st = symmicp_set_median_factor(ctx, median_factor_);
	if (st == SYMMICP_OK) st = symmicp_set_robust_loss(ctx, loss_, loss_scale_);
	if (st == SYMMICP_OK) st = symmicp_set_ndt(ctx, &ncfg);                           // ERR_ARG: setNdt's values
	const size_t fs = sizeof(PointT) / sizeof(float);
	if (st == SYMMICP_OK) st = symmicp_set_target(ctx, &cloud_tgt->points[0].x, fs, 1, nullptr, 0, 0, cloud_tgt->points.size());
	if (st == SYMMICP_OK) st = symmicp_set_source(ctx, &cloud_src->points[0].x, fs, 1, nullptr, 0, 0, cloud_src->points.size());
	if (st != SYMMICP_OK) { error_ = symmicp_last_error(ctx); return done(st); }
	float prev[16];                       // (symmicp_align clears result_ before it reads its guess: the level before is kept apart)
	const float *guess = guess4x4;
	for (size_t k = 0; k < levels.size(); k++) {
		if (k) {
			ncfg.resolution = levels[k].resolution;
			st = symmicp_set_ndt(ctx, &ncfg);
		}
		if (verbose_ && !ndt_levels_.empty())
			std::printf("NDT level %zu/%zu: resolution %g, %d iterations\n", k + 1, levels.size(), (double)levels[k].resolution, levels[k].max_iters);
		cfg.max_iters = levels[k].max_iters;
		cfg.verbose = (verbose_ && k + 1 == levels.size()) ? 1 : 0;
		if (st == SYMMICP_OK) st = symmicp_set_config(ctx, &cfg);
		if (st == SYMMICP_OK) st = symmicp_align(ctx, guess, &result_);
		else result_.status = st;
		level_results_.push_back(result_);
		if (st != SYMMICP_OK) { error_ = symmicp_last_error(ctx); break; }
		std::memcpy(prev, result_.transform, sizeof(prev));
		guess = prev;
	}
	if (result_.iters > 0 || st == SYMMICP_OK) std::memcpy(transform_, result_.transform, sizeof(transform_));
	return done(st);
}

// Multi-start refinement: one problem per guess on the object's clouds, one batch (symmicp_ctx_batch_align)
int MyICP::alignMultiStart(const float *guesses4x4, size_t n_guesses, float out4x4[16])
{
	assert(cloud_src && cloud_tgt);
	multi_results_.clear();
	best_start_ = -1;
	symmicp_ctx *ctx = context();
	if (!ctx) { error_ = "symmicp_create failed: no usable gfx950 HIP device (there is no CPU fallback)"; return SYMMICP_ERR_HIP; }
	const size_t ns = cloud_src->points.size(), nt = cloud_tgt->points.size();
	symmicp_batch_config cfg;
	symmicp_batch_config_default(&cfg);
	cfg.mode = mode_; cfg.max_iters = max_iters; cfg.diff_threshold = diff_threshold; cfg.max_corr_dist = max_corr_dist_;
	const bool in_scope = (mode_ == SYMMICP_MODE_PAPER || mode_ == SYMMICP_MODE_P2P || mode_ == SYMMICP_MODE_PLANE) &&
	                      ns <= SYMMICP_BATCH_MAX_POINTS && nt <= SYMMICP_BATCH_MAX_POINTS;
	if (in_scope) { if (int ost = estimateNormals()) return ost; }      // (a call the batch refuses needs none)
	else { fill_pn(*cloud_src, nullptr, *cloud_pn_src); fill_pn(*cloud_tgt, nullptr, *cloud_pn_tgt); }
	const bool source_normals = mode_ != SYMMICP_MODE_PLANE || have_src_normals_;
	// the packed pools of the batch call
	std::vector<float> sx(3 * ns), sn(3 * ns), tx(3 * nt), tn(3 * nt);
	for (size_t i = 0; i < ns; i++) {
		const pcl::PointNormal &p = cloud_pn_src->points[i];
		sx[3 * i] = p.x; sx[3 * i + 1] = p.y; sx[3 * i + 2] = p.z; sn[3 * i] = p.normal_x; sn[3 * i + 1] = p.normal_y; sn[3 * i + 2] = p.normal_z;
	}
	for (size_t i = 0; i < nt; i++) {
		const pcl::PointNormal &p = cloud_pn_tgt->points[i];
		tx[3 * i] = p.x; tx[3 * i + 1] = p.y; tx[3 * i + 2] = p.z; tn[3 * i] = p.normal_x; tn[3 * i + 1] = p.normal_y; tn[3 * i + 2] = p.normal_z;
	}
	std::vector<symmicp_batch_problem> problems(n_guesses, symmicp_batch_problem{0u, (uint32_t)ns, 0u, (uint32_t)nt});
	multi_results_.resize(n_guesses);
	int st = symmicp_ctx_batch_align(ctx, sx.data(), source_normals ? sn.data() : nullptr, ns, tx.data(), tn.data(), nt, problems.data(), guesses4x4,
	                                 n_guesses, &cfg, multi_results_.data(), nullptr, nullptr);
	if (st != SYMMICP_OK) { error_ = symmicp_last_error(ctx); multi_results_.clear(); return st; }
	for (size_t k = 0; k < n_guesses; k++) {
		const symmicp_batch_result &r = multi_results_[k];
		if (r.status != SYMMICP_OK) continue;
		if (best_start_ < 0) { best_start_ = (int)k; continue; }
		const symmicp_batch_result &b = multi_results_[(size_t)best_start_];
		if (r.pairs > b.pairs || (r.pairs == b.pairs && r.diff_final < b.diff_final)) best_start_ = (int)k;
	}
	if (best_start_ < 0) { error_ = "alignMultiStart: no start ended with SYMMICP_OK"; st = SYMMICP_ERR_DEGENERATE; }
	else {
		const symmicp_batch_result &b = multi_results_[(size_t)best_start_];
		std::memcpy(transform_, b.transform, sizeof(transform_));
		std::memset(&result_, 0, sizeof(result_));
		result_.status = b.status; result_.iters = b.iters; result_.diff_initial = b.diff_initial; result_.diff_final = b.diff_final;
		std::memcpy(result_.transform, b.transform, sizeof(b.transform));
		std::memcpy(result_.diffs, b.diffs, sizeof(b.diffs));
		if (verbose_) {
			char buf[1024];
			symmicp_format_result(transform_, buf, sizeof(buf));
			std::fputs(buf, stdout);
		}
	}
	if (out4x4) std::memcpy(out4x4, transform_, sizeof(transform_));
	return st;
}

// Registration evaluation on the full clouds as the object holds them (pcl::PointXYZ rows of 4 floats), K transforms in one call
static int evaluate_clouds(symmicp_ctx *ctx, const pcl::PointCloud<PointT> &src, const pcl::PointCloud<PointT> &tgt, const float *X16, size_t K,
                           float max_dist, symmicp_evaluation *out)
{
	const size_t stride = sizeof(PointT) / sizeof(float);
	return symmicp_ctx_evaluate_registration(ctx, src.points.empty() ? nullptr : &src.points[0].x, stride, 1, src.points.size(),
	                                         tgt.points.empty() ? nullptr : &tgt.points[0].x, stride, 1, tgt.points.size(), X16, K, max_dist, out,
	                                         nullptr, nullptr);
}

int MyICP::evaluate(float max_dist, symmicp_evaluation *out, const float *transform4x4)
{
	assert(cloud_src && cloud_tgt);
	symmicp_ctx *ctx = context();
	if (!ctx) { error_ = "symmicp_create failed: no usable gfx950 HIP device (there is no CPU fallback)"; return SYMMICP_ERR_HIP; }
	const int st = evaluate_clouds(ctx, *cloud_src, *cloud_tgt, transform4x4 ? transform4x4 : transform_, 1, max_dist, out);
	if (st != SYMMICP_OK) error_ = symmicp_last_error(ctx);
	return st;
}

double MyICP::getFitnessScore(double max_range)
{
	// (a range that fp32 cannot hold is no limit)
	const float d = max_range >= (double)std::numeric_limits<float>::max() ? 0.f : (float)max_range;
	symmicp_evaluation e;
	if (evaluate(d, &e) != SYMMICP_OK || e.inliers == 0) return std::numeric_limits<double>::max();
	return e.mean_d2;
}

int MyICP::evaluateStarts(float max_dist, std::vector<symmicp_evaluation> &out)
{
	assert(cloud_src && cloud_tgt);
	out.clear();
	if (multi_results_.empty()) { error_ = "evaluateStarts: alignMultiStart comes first"; return SYMMICP_ERR_STATE; }
	symmicp_ctx *ctx = context();
	if (!ctx) { error_ = "symmicp_create failed: no usable gfx950 HIP device (there is no CPU fallback)"; return SYMMICP_ERR_HIP; }
	std::vector<float> X(16 * multi_results_.size());
	for (size_t k = 0; k < multi_results_.size(); k++) std::memcpy(&X[16 * k], multi_results_[k].transform, sizeof(float) * 16);
	out.resize(multi_results_.size());
	const int st = evaluate_clouds(ctx, *cloud_src, *cloud_tgt, X.data(), multi_results_.size(), max_dist, out.data());
	if (st != SYMMICP_OK) { error_ = symmicp_last_error(ctx); out.clear(); }
	return st;
}

// SYMMICP_MODE_COLOR: the target's intensity gradient on its tangent planes (k = 10, the normals align() uses), then both attributes
int MyICP::setColorAttributes(symmicp_ctx *ctx)
{
	const size_t ns = cloud_pn_src->points.size(), nt = cloud_pn_tgt->points.size();
	if (src_int_.size() != ns || tgt_int_.size() != nt) {
		error_ = "SYMMICP_MODE_COLOR needs an intensity per point of both clouds (setSourceIntensity / setTargetIntensity, or files with an intensity or rgb field)";
		return SYMMICP_ERR_STATE;
	}
	const size_t fs = sizeof(pcl::PointNormal) / sizeof(float);
	std::vector<float> grad(3 * nt);
	int st = symmicp_ctx_intensity_gradient(ctx, &cloud_pn_tgt->points[0].x, fs, 1, &cloud_pn_tgt->points[0].normal_x, fs, 1, tgt_int_.data(), 1, nt, 10,
	                                        grad.data());
	if (st == SYMMICP_OK) st = symmicp_set_target_intensity(ctx, tgt_int_.data(), 1, grad.data(), 3, 1, nt);
	if (st == SYMMICP_OK) st = symmicp_set_source_intensity(ctx, src_int_.data(), 1, ns);
	if (st != SYMMICP_OK) error_ = symmicp_last_error(ctx);
	return st;
}

// setGlobalInit's steps on the object's context: downsample, normals, FPFH, correspondences, RANSAC -> global_result_
int MyICP::globalInit(symmicp_ctx *ctx)
{
	const GlobalInit &g = global_;
	std::memset(&global_result_, 0, sizeof(global_result_));
	for (int k = 0; k < 16; k++) global_result_.transform[k] = (k % 5 == 0) ? 1.f : 0.f;
	global_result_.ransac.best_hypothesis = -1;
	auto failed = [&](int st, const std::string &what) {
		const char *msg = symmicp_last_error(ctx);
		error_ = "global initialisation: " + what + (msg && msg[0] ? std::string(": ") + msg : std::string());
		global_result_.status = st;
		return st;
	};
	if (cloud_pn_src->points.empty() || cloud_pn_tgt->points.empty()) return failed(SYMMICP_ERR_SIZE, "empty cloud");
	const size_t fs = sizeof(pcl::PointNormal) / sizeof(float);
	struct Cloud { pcl::PointCloud<pcl::PointNormal> *pn; bool have; std::vector<float> xyz, n, f; size_t m; };
	Cloud cl[2] = {{cloud_pn_src.get(), have_src_normals_, {}, {}, {}, 0}, {cloud_pn_tgt.get(), have_tgt_normals_, {}, {}, {}, 0}};
	for (Cloud &c : cl) {
		const size_t n = c.pn->points.size();
		const pcl::PointNormal *p = &c.pn->points[0];
		c.xyz.resize(3 * n);
		c.n.resize(3 * n);
		if (g.voxel_leaf > 0.f) {
			int st = symmicp_ctx_voxel_downsample(ctx, &p->x, fs, 1, c.have ? &p->normal_x : nullptr, fs, 1, n, g.voxel_leaf, 1, c.xyz.data(),
			                                      c.have ? c.n.data() : nullptr, nullptr, nullptr, n, &c.m);
			if (st != SYMMICP_OK) return failed(st, "voxel downsampling");
		} else {
			for (size_t i = 0; i < n; i++) {
				c.xyz[3 * i] = p[i].x; c.xyz[3 * i + 1] = p[i].y; c.xyz[3 * i + 2] = p[i].z;
				if (c.have) { c.n[3 * i] = p[i].normal_x; c.n[3 * i + 1] = p[i].normal_y; c.n[3 * i + 2] = p[i].normal_z; }
			}
			c.m = n;
		}
		if (!c.have) {
			int st = symmicp_ctx_estimate_normals(ctx, c.xyz.data(), 3, 1, c.m, g.normal_k, nullptr, c.n.data(), nullptr);
			if (st != SYMMICP_OK) return failed(st, "normals of the downsampled cloud");
			if (g.orient_k != 0) {
				symmicp_orient_config oc;
				symmicp_orient_config_default(&oc);
				oc.k = g.orient_k;
				std::vector<float> out(3 * c.m);
				st = symmicp_ctx_orient_normals(ctx, c.xyz.data(), 3, 1, c.n.data(), 3, 1, c.m, &oc, out.data(), nullptr, nullptr, nullptr, nullptr, nullptr);
				if (st != SYMMICP_OK) return failed(st, "normal orientation");
				c.n.swap(out);
			}
		}
		c.f.resize(33 * c.m);
		int st = symmicp_ctx_fpfh(ctx, c.xyz.data(), 3, 1, c.n.data(), 3, 1, c.m, g.fpfh_radius, c.f.data(), nullptr, nullptr);
		if (st != SYMMICP_OK) return failed(st, "FPFH features");
	}
	global_result_.source_points = cl[0].m;
	global_result_.target_points = cl[1].m;
	// with iss: the features were computed on the full (downsampled) clouds, whose neighbourhoods stay dense; only the keypoints' rows
	// of them are matched, and the pairs are mapped back to rows of the downsampled clouds for RANSAC
	std::vector<int32_t> kp[2];
	std::vector<float> kf[2];
	if (g.iss) {
		symmicp_iss_config ic;
		symmicp_iss_config_default(&ic);
		ic.salient_radius = g.iss_salient_radius; ic.non_max_radius = g.iss_non_max_radius;
		ic.gamma21 = g.iss_gamma21; ic.gamma32 = g.iss_gamma32; ic.min_neighbors = g.iss_min_neighbors;
		for (int w = 0; w < 2; w++) {
			kp[w].resize(cl[w].m);
			size_t k = 0;
			int st = symmicp_ctx_iss_keypoints(ctx, cl[w].xyz.data(), 3, 1, cl[w].m, &ic, kp[w].data(), cl[w].m, &k, nullptr, nullptr);
			if (st != SYMMICP_OK) return failed(st, "ISS keypoints");
			kp[w].resize(k);
			(w == 0 ? global_result_.source_keypoints : global_result_.target_keypoints) = k;
			kf[w].resize(33 * k);
			for (size_t i = 0; i < k; i++) std::memcpy(&kf[w][33 * i], &cl[w].f[33 * (size_t)kp[w][i]], 33 * sizeof(float));
		}
		if (kp[0].size() < 3 || kp[1].size() < 3)
			return failed(SYMMICP_ERR_NO_CONSENSUS, "ISS keypoints: fewer than 3 keypoints (" + std::to_string(kp[0].size()) + " in the source, " +
			                                            std::to_string(kp[1].size()) + " in the target)");
	}
	const size_t na = g.iss ? kp[0].size() : cl[0].m, nb = g.iss ? kp[1].size() : cl[1].m;
	std::vector<int32_t> pairs(2 * na);
	size_t count = 0;
	int st = symmicp_ctx_feature_correspondences(ctx, g.iss ? kf[0].data() : cl[0].f.data(), na, g.iss ? kf[1].data() : cl[1].f.data(), nb,
	                                             g.mutual ? 1 : 0, g.max_ratio, pairs.data(), nullptr, na, &count);
	if (st != SYMMICP_OK) return failed(st, "feature correspondences");
	if (g.iss) for (size_t k = 0; k < count; k++) { pairs[2 * k] = kp[0][(size_t)pairs[2 * k]]; pairs[2 * k + 1] = kp[1][(size_t)pairs[2 * k + 1]]; }
	global_result_.correspondences = count;
	if (count < 3) return failed(SYMMICP_ERR_NO_CONSENSUS, "fewer than 3 feature correspondences");
	if (g.method == GlobalInit::FGR) {
		symmicp_fgr_config fc;
		symmicp_fgr_config_default(&fc);
		fc.max_dist = g.max_dist; fc.seed = g.seed; fc.iterations = g.fgr_iterations; fc.division_factor = g.fgr_division_factor;
		fc.tuple_scale = g.fgr_tuple_scale; fc.max_tuples = g.fgr_max_tuples;
		st = symmicp_ctx_fgr(ctx, cl[0].xyz.data(), 3, 1, cl[0].m, cl[1].xyz.data(), 3, 1, cl[1].m, pairs.data(), count, &fc, global_result_.transform,
		                     &global_result_.fgr, nullptr, nullptr, nullptr, nullptr, nullptr);
		if (verbose_)
			std::printf("global init: %zu -> %zu source and %zu -> %zu target points, %zu and %zu ISS keypoints, %zu correspondences, FGR: %u tuples accepted, "
			            "%u set elements, %d iterations, %d inliers\n",
			            cloud_pn_src->points.size(), cl[0].m, cloud_pn_tgt->points.size(), cl[1].m, g.iss ? kp[0].size() : (size_t)0,
			            g.iss ? kp[1].size() : (size_t)0, count, global_result_.fgr.tuples_accepted, global_result_.fgr.set_size,
			            global_result_.fgr.iterations, global_result_.fgr.inliers);
		if (st != SYMMICP_OK) {
			for (int k = 0; k < 16; k++) global_result_.transform[k] = (k % 5 == 0) ? 1.f : 0.f;      // (a degenerate loop leaves its X_k: not a guess)
			return failed(st, "FGR");
		}
		global_result_.status = SYMMICP_OK;
		return SYMMICP_OK;
	}
	symmicp_ransac_config rc;
	symmicp_ransac_config_default(&rc);
	rc.hypotheses = g.hypotheses; rc.seed = g.seed; rc.max_dist = g.max_dist; rc.edge_ratio = g.edge_ratio; rc.refits = g.refits;
	st = symmicp_ctx_ransac(ctx, cl[0].xyz.data(), 3, 1, cl[0].m, cl[1].xyz.data(), 3, 1, cl[1].m, pairs.data(), count, &rc, global_result_.transform,
	                        &global_result_.ransac, nullptr, nullptr, nullptr);
	if (verbose_ && g.iss)
		std::printf("global init: %zu -> %zu source and %zu -> %zu target points, %zu and %zu ISS keypoints, %zu correspondences, %d of %u hypotheses evaluated, %d -> %d inliers\n",
		            cloud_pn_src->points.size(), cl[0].m, cloud_pn_tgt->points.size(), cl[1].m, kp[0].size(), kp[1].size(), count,
		            global_result_.ransac.evaluated, rc.hypotheses, global_result_.ransac.inliers_ransac, global_result_.ransac.inliers_final);
	else if (verbose_)
		std::printf("global init: %zu -> %zu source and %zu -> %zu target points, %zu correspondences, %d of %u hypotheses evaluated, %d -> %d inliers\n",
		            cloud_pn_src->points.size(), cl[0].m, cloud_pn_tgt->points.size(), cl[1].m, count, global_result_.ransac.evaluated, rc.hypotheses,
		            global_result_.ransac.inliers_ransac, global_result_.ransac.inliers_final);
	if (st != SYMMICP_OK) return failed(st, "RANSAC");
	global_result_.status = SYMMICP_OK;
	return SYMMICP_OK;
}

// the levels of setVoxelLevels on the object's context (cfg: align()'s configuration, already set on it)
int MyICP::alignLevels(const symmicp_config &cfg0, bool source_normals, const float *guess4x4)
{
	symmicp_ctx *ctx = ctx_;
	if (corr_ == SYMMICP_CORR_IDENTITY) {
		error_ = "voxel levels need nearest-neighbour pairs (SYMMICP_CORR_IDENTITY pairs by row, and downsampled counts differ)";
		result_.status = SYMMICP_ERR_ARG;
		return SYMMICP_ERR_ARG;
	}
	if (cloud_pn_tgt->points.empty() || cloud_pn_src->points.empty()) { result_.status = SYMMICP_ERR_SIZE; return SYMMICP_ERR_SIZE; }
	const size_t fs = sizeof(pcl::PointNormal) / sizeof(float);
	struct Cloud { pcl::PointCloud<pcl::PointNormal> *pn; bool nrm; std::vector<float> xyz, n; size_t m; };
	Cloud cl[2] = {{cloud_pn_src.get(), source_normals, {}, {}, 0}, {cloud_pn_tgt.get(), true, {}, {}, 0}};
	float X[16];
	const float *guess = guess4x4;
	const size_t K = levels_.size();
	for (size_t k = 0; k < K; k++) {
		const VoxelLevel &lv = levels_[k];
		for (Cloud &c : cl) {
			const size_t n = c.pn->points.size();
			const pcl::PointNormal *p = &c.pn->points[0];
			c.xyz.resize(3 * n);
			c.n.resize(c.nrm ? 3 * n : 0);
			if (lv.leaf > 0.f) {
				int st = symmicp_ctx_voxel_downsample(ctx, &p->x, fs, 1, c.nrm ? &p->normal_x : nullptr, fs, 1, n, lv.leaf, 1, c.xyz.data(),
				                                      c.nrm ? c.n.data() : nullptr, nullptr, nullptr, n, &c.m);
				if (st != SYMMICP_OK) { result_.status = st; error_ = symmicp_last_error(ctx); return st; }
			} else {
				for (size_t i = 0; i < n; i++) {
					c.xyz[3 * i] = p[i].x; c.xyz[3 * i + 1] = p[i].y; c.xyz[3 * i + 2] = p[i].z;
					if (c.nrm) { c.n[3 * i] = p[i].normal_x; c.n[3 * i + 1] = p[i].normal_y; c.n[3 * i + 2] = p[i].normal_z; }
				}
				c.m = n;
			}
		}
		if (verbose_)
			std::printf("level %zu/%zu: leaf %g, source %zu -> %zu, target %zu -> %zu\n", k + 1, K, (double)lv.leaf, cloud_pn_src->points.size(), cl[0].m,
			            cloud_pn_tgt->points.size(), cl[1].m);
		symmicp_config cfg = cfg0;
		cfg.max_iters = lv.max_iters;
		cfg.max_corr_dist = lv.max_corr_dist;
		cfg.verbose = (verbose_ && k + 1 == K) ? 1 : 0;
		int st = symmicp_set_config(ctx, &cfg);
		if (st == SYMMICP_OK) st = symmicp_set_target(ctx, cl[1].xyz.data(), 3, 1, cl[1].n.data(), 3, 1, cl[1].m);
		if (st == SYMMICP_OK) {
			st = symmicp_set_source(ctx, cl[0].xyz.data(), 3, 1, cl[0].nrm ? cl[0].n.data() : nullptr, 3, 1, cl[0].m);
			ctx_no_src_normals_ = st == SYMMICP_OK && !cl[0].nrm;
		}
		if (st == SYMMICP_OK) st = symmicp_align(ctx, guess, &result_);
		else result_.status = st;
		level_results_.push_back(result_);
		if (st != SYMMICP_OK) { error_ = symmicp_last_error(ctx); return st; }
		std::memcpy(X, result_.transform, sizeof(X));
		guess = X;
	}
	return SYMMICP_OK;
}

pcl::PointCloud<PointT>::Ptr MyICP::GetAlignedSrcCloud() const
{
	pcl::PointCloud<PointT>::Ptr out(new pcl::PointCloud<PointT>);
	const float *X = transform_;
	out->points.resize(cloud_src->points.size());
	for (size_t i = 0; i < cloud_src->points.size(); i++) {
		const PointT &p = cloud_src->points[i];
		PointT &q = out->points[i];
		q.x = ((X[0] * p.x + X[1] * p.y) + X[2] * p.z) + X[3];
		q.y = ((X[4] * p.x + X[5] * p.y) + X[6] * p.z) + X[7];
		q.z = ((X[8] * p.x + X[9] * p.y) + X[10] * p.z) + X[11];
	}
	out->width = (uint32_t)out->points.size(); out->height = 1;
	return out;
}

void MyICP::RegisterSymm()
{
	// myicp.cpp:100-150; the loop itself (and its stdout lines) runs inside symmicp_align
	int st = align(nullptr, nullptr);
	if (st != SYMMICP_OK) std::cerr << "RegisterSymm: " << error_ << " (status " << st << ")" << std::endl;
}
