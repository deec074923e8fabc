// mvgx_relative_pose_robust.h — sfm::robustRelativePose (sfm/pipelines/sfm_robust_model_estimation.cpp:29-120) from start to end on the
// device. Included at the end of mvgx_geofilter.hip: the first half IS the geometric filter's E a-contrario stage (geofilter_run with
// the five-point model on pixels, or the eight-point model on bearing vectors), the second half the cheirality stage of
// mvgx_relative_pose.h (mvgx_ba.hip's unit), enqueued on the same stream on the filter's own device buffers - bearings, mask, models and
// inlier counts are read where the a-contrario kernel left them. One download at the end.
//
// Where this route parts from the filter entries (both through GeoSource, neither changes what those entries compute):
//   the bound      robustRelativePose hands RelativePose_Info::initial_residual_tolerance to ACRANSAC as it is (:63-66: squared pixels),
//                  GeometricFilter_EMatrix_AC hands Square(m_dPrecision) - here opt->residual_tolerance IS the loop's threshold, no
//                  root and square on the way. The angular form takes degrees on both routes (:89-92 = E_ACRobust_Angular.hpp:117-119).
//   acceptance     !(n < 2.5 x MINIMUM_SAMPLES) (:70-74, :101-105), not the functors' n > 2.5 x MINIMUM_SAMPLES: the same for five points
//                  (13), not for eight (20 inliers pass here). The kernel keeps mask and model by the rule of the route; the decision
//                  reported here is taken from n_inliers.
#pragma once

#include "mvgx_relative_pose_internal.h"

extern "C" int mvgx_relative_pose_robust(int device, const double* xI, const double* xJ, const double* bearingI, const double* bearingJ,
                                         const uint64_t* match_start, const uint32_t* image_wh, const double* K, uint64_t n_pairs,
                                         const mvgx_relative_pose_options* opt, uint8_t* inlier_mask, mvgx_relative_pose_result* results,
                                         uint64_t* out_selected_start, uint32_t* out_selected, double* out_X, mvgx_relative_pose_stats* stats) {
  using clock = std::chrono::steady_clock;
  const auto t_begin = clock::now();
  const char* const entry = "mvgx_relative_pose_robust";
  MVGX_REQUIRE(opt && match_start, MVGX_ERR_ARG, "%s: NULL options or match_start", entry);
  MVGX_REQUIRE(opt->kind == MVGX_RELPOSE_PINHOLE || opt->kind == MVGX_RELPOSE_ANGULAR, MVGX_ERR_ARG, "%s: kind %d", entry, opt->kind);
  MVGX_REQUIRE(opt->method >= 0 && opt->method <= 3, MVGX_ERR_ARG, "%s: method %d", entry, opt->method);
  MVGX_REQUIRE(opt->positive_depth_ratio > 0.0 && opt->positive_depth_ratio <= 1.0, MVGX_ERR_ARG, "%s: positive_depth_ratio %g is outside (0, 1]", entry,
               opt->positive_depth_ratio);
  MVGX_REQUIRE(!std::isinf(opt->residual_tolerance), MVGX_ERR_UNSUPPORTED,
               "%s: an unbounded residual_tolerance (the exhaustive NFA form) has no essential-matrix path on the device", entry);
  MVGX_REQUIRE(std::isfinite(opt->residual_tolerance) && opt->residual_tolerance > 0.0, MVGX_ERR_ARG, "%s: residual_tolerance %g", entry, opt->residual_tolerance);
  MVGX_REQUIRE(n_pairs < (1ull << 32), MVGX_ERR_ARG, "%s: %llu pairs", entry, (unsigned long long)n_pairs);
  const bool pinhole = opt->kind == MVGX_RELPOSE_PINHOLE;
  const int model = pinhole ? kModelE : kModelEA8;
  GeoSource src{entry};
  src.bI = bearingI; src.bJ = bearingJ;
  if (pinhole) { src.xI = xI; src.xJ = xJ; src.K = K; }
  src.bound_as_given = true; src.accept_at_bound = true;
  mvgx_geofilter_options gopt;
  gopt.precision = opt->residual_tolerance; gopt.max_iterations = opt->max_iterations;
  // every argument error of the a-contrario stage before anything is written
  std::vector<mvgx_geofilter_result> gres(std::max<uint64_t>(n_pairs, 1));
  int rc;
  if ((rc = geo_check_arguments(geo_model(model), src, match_start, pinhole ? image_wh : nullptr, n_pairs, &gopt, inlier_mask, gres.data()))) return rc;
  MVGX_REQUIRE(!n_pairs || results, MVGX_ERR_ARG, "%s: NULL results", entry);
  const uint64_t n_total = match_start[n_pairs];
  const bool want_lists = out_selected_start && (out_selected || out_X);

  // the second stage on the first one's buffers
  mvgx::DevBuf<uint64_t> d_start;
  mvgx::DevBuf<mvgx_relative_pose_result> d_res;
  mvgx::DevBuf<uint32_t> d_sel;
  mvgx::DevBuf<double> d_X;
  std::vector<mvgx_relative_pose_result> h_res(n_pairs);
  std::vector<uint32_t> h_sel(out_selected && want_lists ? n_total : 0);
  std::vector<double> h_X(out_X && want_lists ? 3 * n_total : 0);
  hipEvent_t e0 = nullptr, e1 = nullptr;
  struct Events { hipEvent_t& a; hipEvent_t& b; ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); } } events{e0, e1};
  const GeoNextStage next = [&](GeoDevice& dev, hipStream_t stream) -> int {
    if (!n_pairs) return MVGX_OK;
    int rc2;
    if ((rc2 = alloc(d_start, n_pairs + 1)) || (rc2 = alloc(d_res, n_pairs)) || (rc2 = alloc(d_sel, h_sel.size())) || (rc2 = alloc(d_X, h_X.size()))) return rc2;
    MVGX_HIP(hipMemcpyAsync(d_start.p, match_start, (n_pairs + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    MVGX_HIP(hipEventCreate(&e0));
    MVGX_HIP(hipEventCreate(&e1));
    mvgx::RelPoseLaunch a{};
    a.n_pairs = (uint32_t)n_pairs; a.start = d_start.p; a.bI = dev.b1.p; a.bJ = dev.b2.p;
    a.E = dev.res.p->F; a.e_stride = (uint32_t)(sizeof(GeoResult) / sizeof(double)); a.normalize_e = pinhole ? 0 : 1;
    a.use_start = nullptr; a.use_index = nullptr; a.mask = dev.mask.p;
    a.n_inliers = &dev.res.p->n_inliers; a.n_inliers_stride = (uint32_t)(sizeof(GeoResult) / sizeof(uint32_t));
    a.min_inliers = 2.5 * geo_model(model).min_samples;
    a.method = opt->method; a.ratio = opt->positive_depth_ratio;
    a.results = d_res.p; a.out_selected = h_sel.empty() ? nullptr : d_sel.p; a.out_X = h_X.empty() ? nullptr : d_X.p;
    MVGX_HIP(hipEventRecord(e0, stream));
    if ((rc2 = mvgx::relative_pose_launch(a, stream))) return rc2;
    MVGX_HIP(hipEventRecord(e1, stream));
    MVGX_HIP(hipMemcpyAsync(h_res.data(), d_res.p, n_pairs * sizeof(mvgx_relative_pose_result), hipMemcpyDeviceToHost, stream));
    if (!h_sel.empty()) MVGX_HIP(hipMemcpyAsync(h_sel.data(), d_sel.p, h_sel.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    if (!h_X.empty()) MVGX_HIP(hipMemcpyAsync(h_X.data(), d_X.p, h_X.size() * sizeof(double), hipMemcpyDeviceToHost, stream));
    return MVGX_OK;
  };
  static_assert(sizeof(GeoResult) % sizeof(double) == 0 && offsetof(GeoResult, F) == 0, "the stride arithmetic above");
  mvgx_geofilter_stats gstats;
  memset(&gstats, 0, sizeof(gstats));
  if ((rc = geofilter_run(device, model, src, match_start, pinhole ? image_wh : nullptr, n_pairs, &gopt, inlier_mask, gres.data(), &gstats, &next))) return rc;

  uint64_t at = 0, n_ok = 0;
  if (out_selected_start) out_selected_start[0] = 0;
  for (uint64_t p = 0; p < n_pairs; ++p) {
    mvgx_relative_pose_result& r = results[p];
    r = h_res[p];
    memcpy(r.E, gres[p].F, sizeof(r.E));
    r.found_precision = pinhole ? gres[p].precision_robust : gres[p].precision_robust * 180.0 / M_PI;   // (:68, :98-99: R2D)
    r.n_acransac_inliers = gres[p].n_inliers;
    const uint64_t k = r.n_selected;
    if (k && want_lists) {
      if (out_selected) memcpy(out_selected + at, h_sel.data() + match_start[p], k * sizeof(uint32_t));
      if (out_X) memcpy(out_X + 3 * at, h_X.data() + 3 * match_start[p], 3 * k * sizeof(double));
    }
    at += k; n_ok += r.ok;
    if (out_selected_start) out_selected_start[p + 1] = at;
  }
  if (stats) {
    memset(stats, 0, sizeof(*stats));
    float kernel_ms = 0.f;
    if (e0 && e1) (void)hipEventElapsedTime(&kernel_ms, e0, e1);
    stats->n_pairs = n_pairs; stats->n_pairs_ok = n_ok; stats->n_selected = at;
    stats->kernel_ms = kernel_ms; stats->acransac_kernel_ms = gstats.kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(clock::now() - t_begin).count();
  }
  return MVGX_OK;
}
