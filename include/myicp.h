/*
 * myicp.h -- drop-in for the reference's ICP/myicp.h:7-36.
 *
 * Same class name, same five public methods with the same signatures and observable behaviour
 * (LoadCloud returns 0; RegisterSymm prints "iters#k / diff: v" per iteration and the final
 * "Result transform / rotation / translation" block, ICP/myicp.cpp:125-126,146-149; defaults
 * max_iters = 10, diff_threshold = 1.0, ICP/myicp.cpp:6), so the reference's main.cpp call
 * sequence (ICP/main.cpp:7-10,16-31) compiles against it unchanged.  The work is done by
 * libsymmicp (include/symmicp.h) on one MI355X: normals (ICP/myicp.cpp:152-172) and the
 * iteration loop (ICP/myicp.cpp:117-142) both run as HIP kernels.
 *
 * Additive surface (BASELINE.json north_star: "align()/setInput*"): setInputSource,
 * setInputTarget, align, getFinalTransformation, and setters for what the reference hard-codes
 * ("todo add params to specify iters & diff", ICP/myicp.h:19).
 */
#pragma once
#include <limits>
#include <vector>
#include "stdafx.h"
#include "symmicp.h"

typedef pcl::PointXYZ PointT;

class MyICP
{
public:
	MyICP();
	~MyICP();

public:
	int LoadCloud(std::string src_path, std::string tgt_path);
	pcl::PointCloud<PointT>::Ptr GetSrcCloud();
	pcl::PointCloud<PointT>::Ptr GetTgtCloud();

	void RegisterP2P();
	void RegisterSymm();

	// ---- additive ----
	void setInputSource(const float *xyz, const float *normals, size_t n);   // packed [n][3]; normals may be null
	void setInputTarget(const float *xyz, const float *normals, size_t n);
	int align(float out4x4[16] = nullptr, const float *guess4x4 = nullptr);   // returns symmicp_status
	const float *getFinalTransformation() const { return transform_; }       // row-major 4x4
	// the source cloud moved by the final transform (the reference never writes its result back: myicp.cpp:109-111,146-149)
	pcl::PointCloud<PointT>::Ptr GetAlignedSrcCloud() const;
	MyICP(const MyICP &) = delete;
	MyICP &operator=(const MyICP &) = delete;
	void setMaximumIterations(int n) { max_iters = n; }
	void setDiffThreshold(float d) { diff_threshold = d; }
	void setMode(symmicp_mode m) { mode_ = m; }                    // default SYMMICP_MODE_QUIRKS (= the reference); PLANE estimates no source normals,
	                                                               // GICP the normals of both clouds (as PAPER)
	void setCorrespondence(symmicp_corr c) { corr_ = c; }          // default SYMMICP_CORR_IDENTITY (= the reference)
	void setVerbose(bool v) { verbose_ = v; }
	// consistent normal orientation (symmicp_ctx_orient_normals; k = 0, the default: off): the normals pre-step of each cloud is followed
	// by the orientation over the k-NN graph, viewpoint at the origin, so that two clouds of one surface get normals on the same side
	// where a flip towards the viewpoint alone would not.  Applies to normals the class estimates itself, never to supplied ones;
	// checked by align(), which returns SYMMICP_ERR_ARG for a k outside 3 .. 16 or above a cloud's count.
	void setOrientNormals(int k) { orient_k_ = k; }
	// the point-normal clouds the last align() ran on (x y z and the normal it used per point: supplied, or estimated and, with
	// setOrientNormals, oriented); empty before the first align()
	pcl::PointCloud<pcl::PointNormal>::Ptr GetSrcPointNormals() const { return cloud_pn_src; }
	pcl::PointCloud<pcl::PointNormal>::Ptr GetTgtPointNormals() const { return cloud_pn_tgt; }
	// robust loss of the PAPER loop (symmicp_set_robust_loss; default SYMMICP_LOSS_NONE): checked by align(), which
	// returns SYMMICP_ERR_ARG for a loss with SYMMICP_MODE_QUIRKS or a scale that is not finite and > 0
	void setRobustLoss(symmicp_loss loss, float scale) { loss_ = loss; loss_scale_ = scale; }
	// the covariance eps of SYMMICP_MODE_GICP (symmicp_set_gicp_epsilon; default 1e-3): checked by align(), which returns
	// SYMMICP_ERR_ARG unless 0 < eps <= 1 and 1 - eps != 1 in fp32 (eps > 2^-25)
	void setGicpEpsilon(float eps) { gicp_eps_ = eps; }
	// trimmed ICP (symmicp_set_trim_fraction; default 1 = off): every pass keeps the closest `fraction` of its pairs -- for clouds that
	// overlap only in part.  Applies to single-level runs and to every level of setVoxelLevels; checked by align(), which returns
	// SYMMICP_ERR_ARG unless 0 < fraction <= 1, and for a fraction below 1 with SYMMICP_MODE_QUIRKS
	void setTrimFraction(float fraction) { trim_fraction_ = fraction; }
	// one-to-one and median-distance rejection (symmicp_set_one_to_one / symmicp_set_median_factor; default off / 0 = off): of the source
	// points paired with one target point only the closest is kept; pairs farther than factor x the median pair distance are dropped.
	// Apply like setTrimFraction, every level of setVoxelLevels included; checked by align(), which returns SYMMICP_ERR_ARG with
	// SYMMICP_MODE_QUIRKS, for a factor that is neither 0 nor finite and > 0, and for a factor > 0 with a trim fraction below 1
	void setOneToOne(bool on) { one_to_one_ = on; }
	void setMedianFactor(float factor) { median_factor_ = factor; }
	// reciprocal correspondences (symmicp_set_reciprocal; default off; PCL's setUseReciprocalCorrespondences): a pair (p, q) is kept only
	// if p is also the nearest source point of q; implies one-to-one.  Applies like setOneToOne, every level of setVoxelLevels included;
	// checked by align(), which returns SYMMICP_ERR_ARG with SYMMICP_MODE_QUIRKS and with SYMMICP_CORR_IDENTITY
	void setReciprocalCorrespondences(bool on) { reciprocal_ = on; }
	// Colored ICP (SYMMICP_MODE_COLOR): one scalar intensity per point of each cloud, n = the cloud's count, set after setInput* /
	// LoadCloud (LoadCloud keeps the intensities of files that carry an `intensity` or `rgb` field; setInput* drops the cloud's).
	// align() estimates the target's intensity gradient itself (symmicp_ctx_intensity_gradient, k = 10).  In COLOR align() returns
	// SYMMICP_ERR_STATE when either cloud has no intensities, and SYMMICP_ERR_ARG with voxel levels (not supported yet).
	void setSourceIntensity(const float *intensity, size_t n) { src_int_.assign(intensity, intensity + n); }
	void setTargetIntensity(const float *intensity, size_t n) { tgt_int_.assign(intensity, intensity + n); }
	// lambda of the geometric rows (symmicp_set_color_weight; default 0.968): checked by align(), SYMMICP_ERR_ARG outside [0, 1]
	void setColorWeight(float lambda) { color_weight_ = lambda; }
	bool haveIntensities() const { return !src_int_.empty() && !tgt_int_.empty(); }   // both clouds carry one (set, or loaded from the files)
	// pairs farther apart than d are dropped (symmicp_config.max_corr_dist; <= 0, the default: every pair is kept)
	void setMaxCorrespondenceDistance(float d) { max_corr_dist_ = d; }
	// Coarse-to-fine alignment.  With levels set, align() estimates (or takes) the normals of the full clouds as before, then runs
	// one alignment per level in the order given: both clouds voxel-downsampled with the level's leaf (symmicp_ctx_voxel_downsample,
	// normals averaged; leaf 0: the clouds as given), max_iters and max_corr_dist from the level, started from the previous level's
	// transform (the first from the caller's guess).  The result is the last level's: source -> target in original coordinates.
	// Coarse levels run quiet; verbose prints one line per level and the last level's iterations and Result block.
	// SYMMICP_CORR_IDENTITY is SYMMICP_ERR_ARG with levels (the downsampled counts differ).  Empty (the default): align() as without.
	struct VoxelLevel { float leaf; int max_iters; float max_corr_dist; };
	void setVoxelLevels(const std::vector<VoxelLevel> &levels) { levels_ = levels; }
	// NDT registration (SYMMICP_MODE_NDT, include/symmicp.h): the voxel edge, the neighbourhood (1: the point's own voxel, 7: and its six
	// face neighbours) and the fewest points a voxel needs; checked by align() (SYMMICP_ERR_ARG as symmicp_set_ndt).  In this mode
	// align() skips both normals pre-steps (the clouds go in without normals) and builds no index; robust losses, the rejectors, voxel
	// levels and the global initialisation are SYMMICP_ERR_ARG.
	void setNdt(float resolution, int neighbors = 7, int min_points = 6) { ndt_resolution_ = resolution; ndt_neighbors_ = neighbors; ndt_min_points_ = min_points; }
	// Coarse-to-fine NDT, coarse first: per level symmicp_set_ndt with the level's resolution (the target's map is rebuilt at once) and an
	// alignment of max_iters iterations started from the level before (the first from the caller's guess) -- bit for bit the transform
	// of the same calls made by hand.  levelResults() has one result per level.  Empty (the default): one alignment at setNdt's resolution.
	struct NdtLevel { float resolution; int max_iters; };
	void setNdtLevels(const std::vector<NdtLevel> &levels) { ndt_levels_ = levels; }
	const std::vector<symmicp_result> &levelResults() const { return level_results_; }   // one per level run by the last align()
	// Global initialisation (feature matching and RANSAC, include/symmicp.h): with it set and no guess4x4 given, align() first
	// voxel-downsamples both clouds with voxel_leaf (0: the clouds as given), estimates normals on the downsampled clouds when the
	// caller supplied none (normal_k neighbours, viewpoint at the origin), computes FPFH features of both at fpfh_radius, their
	// correspondences (mutual, max_ratio) and a RANSAC transform (max_dist, hypotheses, seed, edge_ratio, refits), and starts the
	// ordinary alignment (voxel levels included) from it.  A failure of any step -- SYMMICP_ERR_NO_CONSENSUS from RANSAC among
	// them -- is returned from align() with lastError() saying so; there is no silent fall-back to the identity.  FPFH matching
	// needs normals oriented alike in both clouds: with estimated normals orient_k > 0 arranges that within every connected part of
	// each cloud (symmicp_ctx_orient_normals, viewpoint at the origin); what remains the caller's part is a cloud in separate parts,
	// each seeded on its own, and a viewpoint inside the object.
	struct GlobalInit {
		float voxel_leaf = 0.f;
		int normal_k = 10;
		int orient_k = 0;             // > 0: the estimated normals are oriented consistently over the orient_k-NN graph (3 .. 16); 0: off
		float fpfh_radius = 0.f;      // required: finite, > 0
		float max_dist = 0.f;         // required: finite, > 0
		unsigned hypotheses = 100000;
		unsigned long long seed = 0;
		bool mutual = true;
		float max_ratio = 0.f;
		float edge_ratio = 0.9f;
		int refits = 1;
		// ISS keypoints (symmicp_ctx_iss_keypoints; off by default): the features are still computed on the full (downsampled) clouds,
		// but only the keypoints' rows of them are matched, and RANSAC runs on those pairs (mapped back to rows of the downsampled
		// clouds).  Matching cost falls from quadratic in the cloud to quadratic in the keypoint count.  Fewer than 3 keypoints in
		// either cloud is SYMMICP_ERR_NO_CONSENSUS from align(); there is no fall-back to the full cloud.
		bool iss = false;
		float iss_salient_radius = 0.f;   // required with iss: finite, > 0
		float iss_non_max_radius = 0.f;   // required with iss: finite, > 0
		float iss_gamma21 = 0.975f, iss_gamma32 = 0.975f;
		int iss_min_neighbors = 5;
		// The estimator the correspondences go to: RANSAC (the default) or Fast Global Registration (symmicp_ctx_fgr: a tuple test and a
		// graduated-non-convexity loop, no hypothesis count to tune).  FGR shares max_dist and seed with RANSAC and ignores hypotheses,
		// edge_ratio and refits; with it RANSAC is not run, every other step is the same, and a failure is returned as RANSAC's is.
		enum Method { RANSAC = 0, FGR = 1 };
		Method method = RANSAC;
		int fgr_iterations = 64;
		float fgr_division_factor = 1.4f;
		float fgr_tuple_scale = 0.95f;
		unsigned fgr_max_tuples = 1000;
	};
	struct GlobalResult {
		symmicp_ransac_result ransac;  // of the last align() that ran the initialisation
		float transform[16];           // row-major 4x4, source -> target: the guess the alignment started from
		size_t correspondences;
		size_t source_points, target_points;   // after downsampling
		size_t source_keypoints, target_keypoints;   // with GlobalInit::iss: the ISS keypoints of each (0 without)
		int status;                    // symmicp_status of the initialisation
		symmicp_fgr_result fgr;        // with GlobalInit::FGR: its result (ransac stays zero), else zero
	};
	void setGlobalInit(const GlobalInit &g) { global_ = g; have_global_ = true; }
	void clearGlobalInit() { have_global_ = false; }
	const GlobalResult &globalResult() const { return global_result_; }
	const symmicp_result &lastResult() const { return result_; }
	// Multi-start refinement: ONE batch on the object's clouds and context (symmicp_ctx_batch_align, include/symmicp.h), a problem per
	// guess (n_guesses row-major 4x4 matrices), with the object's mode, max_iters, diff_threshold and max correspondence distance;
	// normals are estimated as align() does.  Every result stays available through multiStartResults().  Adopted as final
	// transformation: the result with status SYMMICP_OK and the most pairs; ties go to the smaller diff_final, then to the lowest
	// index (bestStart(); -1 and the final transformation unchanged when no problem ended OK: the call then returns
	// SYMMICP_ERR_DEGENERATE).  Clouds above SYMMICP_BATCH_MAX_POINTS points, or a mode other than PAPER, P2P and PLANE, return the
	// batch call's error: there is no fallback to a loop of align() calls.
	int alignMultiStart(const float *guesses4x4, size_t n_guesses, float out4x4[16] = nullptr);
	const std::vector<symmicp_batch_result> &multiStartResults() const { return multi_results_; }
	int bestStart() const { return best_start_; }
	// Registration evaluation (symmicp_ctx_evaluate_registration, include/symmicp.h) on the object's FULL clouds: fitness, inlier RMSE,
	// the inlier sums and the 6x6 information matrix of transform4x4 (row-major; null: the final transformation) at max_dist (<= 0:
	// every point counts).  Returns a symmicp_status; the object's context and results stay as they were.
	int evaluate(float max_dist, symmicp_evaluation *out, const float *transform4x4 = nullptr);
	// PCL's getFitnessScore for the final transformation: the mean squared distance from the moved source points to their nearest
	// target points, over those within max_range (a distance, rounded to fp32; the default: no limit), and
	// std::numeric_limits<double>::max() when none is within range or the evaluation fails (lastError() says why).
	double getFitnessScore(double max_range = std::numeric_limits<double>::max());
	// every multiStartResults() transform scored on the full clouds at one common distance, in ONE call: out[k] belongs to guess k.
	// alignMultiStart's own choice of winner does not change.  SYMMICP_ERR_STATE before an alignMultiStart.
	int evaluateStarts(float max_dist, std::vector<symmicp_evaluation> &out);
	// Outlier removal (symmicp_ctx_statistical_outlier_removal / symmicp_ctx_radius_outlier_removal, include/symmicp.h): a one-shot
	// edit of BOTH held clouds, the same as a user running PCL's filter before RegisterSymm -- not a stored option.  Each cloud is
	// filtered by its own statistics; the point clouds, the point-normal clouds (normals the caller supplied included: they stay
	// "supplied") and the per-point intensities keep the surviving rows, in row order.  Returns a symmicp_status; on an error
	// neither cloud is changed.  outliersRemoved reports how many points the last call took from each cloud (either may be null).
	// With SYMMICP_CORR_IDENTITY a later align() returns SYMMICP_ERR_SIZE if the two counts end up unequal, as it does for any
	// two clouds of different sizes.
	int removeStatisticalOutliers(int k, float std_mul);
	int removeRadiusOutliers(float radius, int min_neighbors);
	// The same edit by connectivity (symmicp_ctx_cluster with min_points = 1 and min_cluster_size = min_size): every connected part of a
	// cloud -- points closer than eps -- with fewer than min_size points goes.  A floating blob of a dozen points passes both filters
	// above, because each of its points has close neighbours; this one removes it.
	int removeSmallClusters(float eps, int min_size);
	// The same edit for the dominant plane (symmicp_ctx_segment_plane: seed 0, one refit): the final inliers of the plane with the most
	// points within max_dist go from EACH held cloud -- the floor or the table that joins the objects standing on it into one cluster.
	// axis (null or all zero: none) and max_angle_deg restrict the planes to those whose normal lies within that angle of the axis.
	// A cloud in which no plane reaches max(3, min_inliers) points loses nothing; that is not an error.  planeRemoved reports the two
	// planes (n, d with n . x + d = 0 in the cloud's own coordinates; zeros for a cloud without one; either may be null).
	int removePlane(float max_dist, int hypotheses = 1000, int min_inliers = 3, const float axis[3] = nullptr, float max_angle_deg = 0.f);
	void planeRemoved(double src[4], double tgt[4]) const
	{
		for (int a = 0; a < 4; a++) { if (src) src[a] = planes_[0][a]; if (tgt) tgt[a] = planes_[1][a]; }
	}
	void outliersRemoved(size_t *src, size_t *tgt) const { if (src) *src = removed_src_; if (tgt) *tgt = removed_tgt_; }
	const char *lastError() const { return error_.c_str(); }

private:
	int max_iters;
	float diff_threshold;

	pcl::PointCloud<PointT>::Ptr cloud_src, cloud_tgt;
	pcl::PointCloud<pcl::PointNormal>::Ptr cloud_pn_src, cloud_pn_tgt;

	int estimateNormals();               // SYMMICP_OK, or what setOrientNormals' step returned
	int orient_k_ = 0;

	symmicp_ctx *context();              // one libsymmicp context for the life of the object (stream, arenas, code objects)

	symmicp_mode mode_;
	symmicp_corr corr_;
	bool verbose_, have_src_normals_, have_tgt_normals_;   // have_*: normals supplied by the caller through setInput*
	symmicp_loss loss_;
	float loss_scale_;
	float gicp_eps_;
	float trim_fraction_;
	bool one_to_one_;
	bool reciprocal_;
	float median_factor_;
	float max_corr_dist_;
	float color_weight_ = 0.968f;
	std::vector<float> src_int_, tgt_int_;
	int setColorAttributes(symmicp_ctx *ctx);   // COLOR: the target's gradient and both intensities, after set_target / set_source
	std::vector<VoxelLevel> levels_;
	std::vector<symmicp_result> level_results_;
	int alignLevels(const symmicp_config &cfg, bool source_normals, const float *guess4x4);
	float ndt_resolution_ = 1.f;
	int ndt_neighbors_ = 7, ndt_min_points_ = 6;
	std::vector<NdtLevel> ndt_levels_;
	int alignNdt(float out4x4[16], const float *guess4x4);
	GlobalInit global_;
	bool have_global_ = false;
	GlobalResult global_result_{};
	int globalInit(symmicp_ctx *ctx);
	symmicp_ctx *ctx_;
	int ctx_corr_;
	bool ctx_ndt_ = false;               // the context was created for SYMMICP_MODE_NDT (it holds a voxel map, not an index: no other mode runs on it)
	bool ctx_no_src_normals_;            // the context holds a source set without normals (PLANE): no other mode can run on it
	float transform_[16];
	symmicp_result result_;
	std::vector<symmicp_batch_result> multi_results_;
	int best_start_ = -1;
	size_t removed_src_ = 0, removed_tgt_ = 0;
	int removeOutliers(int filter, int k, float std_mul, float radius, int min_neighbors);      // filter: 0 statistical, 1 radius, 2 small clusters, 3 the plane of plane_cfg_
	symmicp_plane_config plane_cfg_{};
	double planes_[2][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}};
	std::string error_;
};
