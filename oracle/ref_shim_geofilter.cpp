// ref_shim_geofilter.cpp - TEST INFRASTRUCTURE ONLY (never linked into the product).
//
// Thin extern "C" wrapper (our code) around the REFERENCE's own a-contrario fundamental-matrix filter, compiled in place from
// /root/reference/src by oracle/Makefile (target ref_geofilter) into oracle/_ref/libref_geofilter.so. It runs, per image pair, what
// GeometricFilter_FMatrix_AC::Robust_estimation (matching_image_collection/F_ACRobust.hpp:65-122) runs:
//   robust::ACKernelAdaptor<fundamental::kernel::SevenPointSolver, fundamental::kernel::EpipolarDistanceError, UnnormalizerT, Mat3>
//     (robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:104-202, multiview/solver_fundamental_kernel.cpp:37-93,157-166)
//   robust::ACRANSAC (robust_estimation/robust_estimator_ACRansac.hpp:339-489)
// with the pairs spread over OpenMP threads as ImageCollectionGeometricFilter::Robust_model_estimation does
// (matching_image_collection/GeometricFilter.hpp:80-131). The feature positions arrive as the Mat2X pair MatchesPairToMat would
// build (Geometric_Filter_utils.hpp:56-64); the container bookkeeping around it is not part of this checker.
// Used (a) to pin oracle/geofilter_oracle.cpp and the device path, (b) as the "reference" CPU baseline of bench_geofilter.py.
#include <chrono>
#include <cstdint>
#include <cstring>
#include <exception>
#include <limits>
#include <vector>

#include <omp.h>

#include "openMVG/cameras/Camera_Pinhole.hpp"
#include "openMVG/multiview/solver_essential_five_point.hpp"
#include "openMVG/multiview/solver_essential_kernel.hpp"
#include "openMVG/multiview/solver_fundamental_kernel.hpp"
#include "openMVG/multiview/motion_from_essential.hpp"
#include "openMVG/multiview/solver_essential_eight_point.hpp"
#include "openMVG/multiview/solver_essential_three_point.hpp"
#include "openMVG/multiview/solver_homography_kernel.hpp"
#include "openMVG/numeric/numeric.h"
#include "openMVG/robust_estimation/robust_estimator_ACRansac.hpp"
#include "openMVG/robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp"

using namespace openMVG;

// One robust estimation per pair with the given kernel adaptor (F: point-to-line, H: point-to-point), as the functors'
// Robust_estimation members run it.
template <typename KernelType>
static double run_acransac(const double* xI, const double* xJ, const uint64_t* start, const uint32_t* wh, uint64_t n_pairs, double precision,
                           uint32_t max_iterations, int num_threads, bool point_to_line, uint8_t* inlier_mask, uint8_t* ok, double* F, double* prec,
                           double* nfa) {
  const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic) num_threads(num_threads > 0 ? num_threads : omp_get_max_threads())
  for (int64_t p = 0; p < (int64_t)n_pairs; ++p) {
    const uint64_t lo = start[p], n = start[p + 1] - lo;
    Mat2X x1(2, n), x2(2, n);
    for (uint64_t i = 0; i < n; ++i) {
      x1.col(i) << xI[2 * (lo + i)], xI[2 * (lo + i) + 1];
      x2.col(i) << xJ[2 * (lo + i)], xJ[2 * (lo + i) + 1];
    }
    std::memset(inlier_mask + lo, 0, n);
    Mat3 model = Mat3::Identity();
    const KernelType kernel(x1, wh[4 * p], wh[4 * p + 1], x2, wh[4 * p + 2], wh[4 * p + 3], point_to_line);
    const double upper_bound_precision = Square(precision);   // F_ACRobust.hpp:98, H_ACRobust.hpp:92
    std::vector<uint32_t> vec_inliers;
    const std::pair<double, double> out = robust::ACRANSAC(kernel, vec_inliers, max_iterations, &model, upper_bound_precision);
    const bool good = vec_inliers.size() > KernelType::MINIMUM_SAMPLES * 2.5;   // F_ACRobust.hpp:103, H_ACRobust.hpp:98
    ok[p] = good ? 1 : 0;
    prec[p] = out.first; nfa[p] = out.second;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) F[9 * p + 3 * r + c] = model(r, c);
    if (good)
      for (const uint32_t idx : vec_inliers) inlier_mask[lo + idx] = 1;
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

extern "C" {

// pairs: for pair p the correspondences [start[p], start[p + 1]) of xI / xJ (2 doubles each, pixels), image sizes wh[4 p ..] =
// {w_I, h_I, w_J, h_J}. Outputs: inlier_mask per correspondence (1: geometric inlier of a pair whose estimation succeeded),
// ok[p] (Robust_estimation returned true), F[9 p ..] row-major (m_F), prec[p] (m_dPrecision_robust = ACRansacOut.first),
// nfa[p] (ACRansacOut.second). Returns the seconds spent.
double ref_geofilter_f_acransac(const double* xI, const double* xJ, const uint64_t* start, const uint32_t* wh, uint64_t n_pairs,
                                double precision, uint32_t max_iterations, int num_threads, uint8_t* inlier_mask, uint8_t* ok, double* F,
                                double* prec, double* nfa) {
  using KernelType = robust::ACKernelAdaptor<fundamental::kernel::SevenPointSolver, fundamental::kernel::EpipolarDistanceError, UnnormalizerT, Mat3>;
  return run_acransac<KernelType>(xI, xJ, start, wh, n_pairs, precision, max_iterations, num_threads, true, inlier_mask, ok, F, prec, nfa);
}

// the same for GeometricFilter_HMatrix_AC::Robust_estimation (matching_image_collection/H_ACRobust.hpp:49-113): the homography
// kernel, "configure as point to point error model"; F receives m_H
double ref_geofilter_h_acransac(const double* xI, const double* xJ, const uint64_t* start, const uint32_t* wh, uint64_t n_pairs,
                                double precision, uint32_t max_iterations, int num_threads, uint8_t* inlier_mask, uint8_t* ok, double* F,
                                double* prec, double* nfa) {
  using KernelType = robust::ACKernelAdaptor<homography::kernel::FourPointSolver, homography::kernel::AsymmetricError, UnnormalizerI, Mat3>;
  return run_acransac<KernelType>(xI, xJ, start, wh, n_pairs, precision, max_iterations, num_threads, false, inlier_mask, ok, F, prec, nfa);
}

// GeometricFilter_EMatrix_AC::Robust_estimation (matching_image_collection/E_ACRobust.hpp:57-150) per pair:
// ACKernelAdaptorEssential<FivePointSolver, EpipolarDistanceError, Mat3> on the pixels + the cameras' bearing vectors, ACRANSAC, more than
// 2.5 x 5 inliers. K: 18 doubles per pair {K_I, K_J} row-major (the cameras are Pinhole_Intrinsic(w, h, K)); F receives m_E.
double ref_geofilter_e_acransac(const double* xI, const double* xJ, const uint64_t* start, const uint32_t* wh, const double* K, uint64_t n_pairs,
                                double precision, uint32_t max_iterations, int num_threads, uint8_t* inlier_mask, uint8_t* ok, double* F,
                                double* prec, double* nfa) {
  using KernelType = robust::ACKernelAdaptorEssential<essential::kernel::FivePointSolver, fundamental::kernel::EpipolarDistanceError, Mat3>;
  const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic) num_threads(num_threads > 0 ? num_threads : omp_get_max_threads())
  for (int64_t p = 0; p < (int64_t)n_pairs; ++p) {
    const uint64_t lo = start[p], n = start[p + 1] - lo;
    Mat2X x1(2, n), x2(2, n);
    for (uint64_t i = 0; i < n; ++i) {
      x1.col(i) << xI[2 * (lo + i)], xI[2 * (lo + i) + 1];
      x2.col(i) << xJ[2 * (lo + i)], xJ[2 * (lo + i) + 1];
    }
    std::memset(inlier_mask + lo, 0, n);
    Mat3 K1, K2;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { K1(r, c) = K[18 * p + 3 * r + c]; K2(r, c) = K[18 * p + 9 + 3 * r + c]; }
    const cameras::Pinhole_Intrinsic camI(wh[4 * p], wh[4 * p + 1], K1), camJ(wh[4 * p + 2], wh[4 * p + 3], K2);
    Mat3 model = Mat3::Identity();
    const KernelType kernel(x1, camI(x1), wh[4 * p], wh[4 * p + 1], x2, camJ(x2), wh[4 * p + 2], wh[4 * p + 3], camI.K(), camJ.K());
    const double upper_bound_precision = Square(precision);   // E_ACRobust.hpp:127
    std::vector<uint32_t> vec_inliers;
    const std::pair<double, double> out = robust::ACRANSAC(kernel, vec_inliers, max_iterations, &model, upper_bound_precision);
    const bool good = vec_inliers.size() > KernelType::MINIMUM_SAMPLES * 2.5;   // E_ACRobust.hpp:132
    ok[p] = good ? 1 : 0;
    prec[p] = out.first; nfa[p] = out.second;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) F[9 * p + 3 * r + c] = model(r, c);
    if (good)
      for (const uint32_t idx : vec_inliers) inlier_mask[lo + idx] = 1;
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// GeometricFilter_ESphericalMatrix_AC_Angular<upright>::Robust_estimation (matching_image_collection/E_ACRobust_Angular.hpp:53-160) per pair
// on the bearing vectors bI / bJ (3 doubles per correspondence): ACKernelAdaptor_AngularRadianError<EightPointRelativePoseSolver |
// ThreePointUprightRelativePoseSolver, AngularError> + ACRANSAC with the bound D2R(precision_deg) (:117-122). pose_stage = 0 stops after
// ACRANSAC (its inliers, more than 2.5 x MINIMUM_SAMPLES of them: what the device entry returns), 1 continues like the functor with
// RelativePoseFromEssential on those inliers (:126-143) and reports the functor's geometric inliers.
extern "C++" {
template <typename Solver>
static double run_angular(const double* bI, const double* bJ, const uint64_t* start, uint64_t n_pairs, double precision_deg, uint32_t max_iterations,
                          int num_threads, int pose_stage, uint8_t* inlier_mask, uint8_t* ok, double* F, double* prec, double* nfa) {
  using KernelType = robust::ACKernelAdaptor_AngularRadianError<Solver, AngularError, Mat3>;
  const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic) num_threads(num_threads > 0 ? num_threads : omp_get_max_threads())
  for (int64_t p = 0; p < (int64_t)n_pairs; ++p) {
    const uint64_t lo = start[p], n = start[p + 1] - lo;
    Mat3X x1(3, n), x2(3, n);
    for (uint64_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) { x1(k, i) = bI[3 * (lo + i) + k]; x2(k, i) = bJ[3 * (lo + i) + k]; }
    std::memset(inlier_mask + lo, 0, n);
    Mat3 model = Mat3::Identity();
    const KernelType kernel(x1, x2);
    const double upper_bound_precision = D2R(precision_deg);
    std::vector<uint32_t> vec_inliers;
    const std::pair<double, double> out = robust::ACRANSAC(kernel, vec_inliers, max_iterations, &model, upper_bound_precision);
    if (pose_stage) {
      geometry::Pose3 relative_pose;
      std::vector<uint32_t> inliers_indexes;
      std::vector<Vec3> inliers_X;
      if (RelativePoseFromEssential(x1, x2, model, vec_inliers, &relative_pose, &inliers_indexes, &inliers_X)) vec_inliers = inliers_indexes;
      else vec_inliers.clear();
    }
    const bool good = vec_inliers.size() > KernelType::MINIMUM_SAMPLES * 2.5;
    ok[p] = good ? 1 : 0;
    prec[p] = out.first; nfa[p] = out.second;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) F[9 * p + 3 * r + c] = model(r, c);
    if (good)
      for (const uint32_t idx : vec_inliers) inlier_mask[lo + idx] = 1;
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
}  // extern "C++"
double ref_geofilter_e_angular_acransac(const double* bI, const double* bJ, const uint64_t* start, uint64_t n_pairs, double precision_deg,
                                        uint32_t max_iterations, int num_threads, int upright, int pose_stage, uint8_t* inlier_mask, uint8_t* ok,
                                        double* F, double* prec, double* nfa) {
  return upright ? run_angular<essential::kernel::ThreePointUprightRelativePoseSolver>(bI, bJ, start, n_pairs, precision_deg, max_iterations, num_threads,
                                                                                        pose_stage, inlier_mask, ok, F, prec, nfa)
                 : run_angular<EightPointRelativePoseSolver>(bI, bJ, start, n_pairs, precision_deg, max_iterations, num_threads, pose_stage, inlier_mask,
                                                             ok, F, prec, nfa);
}

// GeometricFilter_EOMatrix_RA::Robust_estimation (matching_image_collection/Eo_Robust.hpp:50-144) per pair: the cameras are
// Pinhole_Intrinsic(w, h, K) (K: 18 doubles per pair), the bound becomes the mean of imagePlane_toCameraPlaneError(precision^2) (:96-100),
// ACKernelAdaptorEssentialOrtho<ThreePointKernel, OrthographicSymmetricEpipolarDistanceError> on the cameras' bearing vectors, ACRANSAC,
// more than 2.5 x 3 inliers. F receives m_E.
double ref_geofilter_eo_acransac(const double* xI, const double* xJ, const uint64_t* start, const uint32_t* wh, const double* K, uint64_t n_pairs,
                                 double precision, uint32_t max_iterations, int num_threads, uint8_t* inlier_mask, uint8_t* ok, double* F,
                                 double* prec, double* nfa) {
  using KernelType = robust::ACKernelAdaptorEssentialOrtho<essential::kernel::ThreePointKernel,
                                                           essential::kernel::OrthographicSymmetricEpipolarDistanceError, Mat3>;
  const auto t0 = std::chrono::steady_clock::now();
#pragma omp parallel for schedule(dynamic) num_threads(num_threads > 0 ? num_threads : omp_get_max_threads())
  for (int64_t p = 0; p < (int64_t)n_pairs; ++p) {
    const uint64_t lo = start[p], n = start[p + 1] - lo;
    Mat2X x1(2, n), x2(2, n);
    for (uint64_t i = 0; i < n; ++i) {
      x1.col(i) << xI[2 * (lo + i)], xI[2 * (lo + i) + 1];
      x2.col(i) << xJ[2 * (lo + i)], xJ[2 * (lo + i) + 1];
    }
    std::memset(inlier_mask + lo, 0, n);
    Mat3 K1, K2;
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { K1(r, c) = K[18 * p + 3 * r + c]; K2(r, c) = K[18 * p + 9 + 3 * r + c]; }
    const cameras::Pinhole_Intrinsic camI(wh[4 * p], wh[4 * p + 1], K1), camJ(wh[4 * p + 2], wh[4 * p + 3], K2);
    const double bound = (camI.imagePlane_toCameraPlaneError(Square(precision)) + camJ.imagePlane_toCameraPlaneError(Square(precision))) / 2.;
    Mat3 model = Mat3::Identity();
    const KernelType kernel(camI(x1), wh[4 * p], wh[4 * p + 1], camJ(x2), wh[4 * p + 2], wh[4 * p + 3]);
    std::vector<uint32_t> vec_inliers;
    const std::pair<double, double> out = robust::ACRANSAC(kernel, vec_inliers, max_iterations, &model, bound);
    const bool good = vec_inliers.size() > KernelType::MINIMUM_SAMPLES * 2.5;   // Eo_Robust.hpp:128
    ok[p] = good ? 1 : 0;
    prec[p] = out.first; nfa[p] = out.second;
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) F[9 * p + 3 * r + c] = model(r, c);
    if (good)
      for (const uint32_t idx : vec_inliers) inlier_mask[lo + idx] = 1;
  }
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the bearing vectors Pinhole_Intrinsic(w, h, K)(x) the essential kernel receives (Camera_Pinhole.hpp:136-139): n points, 3 doubles each
void ref_pinhole_bearings(const double* K, const double* x, uint64_t n, double* out) {
  Mat3 Km;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Km(r, c) = K[3 * r + c];
  const cameras::Pinhole_Intrinsic cam(1, 1, Km);
  Mat2X pts(2, n);
  for (uint64_t i = 0; i < n; ++i) pts.col(i) << x[2 * i], x[2 * i + 1];
  const Mat3X b = cam(pts);
  for (uint64_t i = 0; i < n; ++i) for (int k = 0; k < 3; ++k) out[3 * i + k] = b(k, i);
}

// FivePointsRelativePose (multiview/solver_essential_five_point.cpp:170-230) on five bearing pairs (5 x 3 doubles each): up to ten
// essential matrices, row-major
void ref_five_point(const double* b1, const double* b2, double* Es_out, int* n_out) {
  Mat3X x1(3, 5), x2(3, 5);
  for (int i = 0; i < 5; ++i) for (int k = 0; k < 3; ++k) { x1(k, i) = b1[3 * i + k]; x2(k, i) = b2[3 * i + k]; }
  std::vector<Mat3> Es;
  FivePointsRelativePose(x1, x2, &Es);
  *n_out = (int)Es.size();
  for (size_t m = 0; m < Es.size(); ++m) for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) Es_out[9 * m + 3 * r + c] = Es[m](r, c);
}

}  // extern "C"

// ---- container level: ImageCollectionGeometricFilter::Robust_model_estimation on an in-memory scene --------------------------
// The same caller code is compiled twice: into oracle/_ref/libref_geofilter.so against the reference headers alone (the member
// template of GeometricFilter.hpp is instantiated), and into the adapter harness with -include mvgx_geometric_filter.hpp, where
// the explicit specialisation of openmvg_amd/adapter/mvgx_geometric_filter.cpp is linked instead (oracle/adapter_harness.mk).
#include "openMVG/cameras/Camera_Pinhole_Radial.hpp"
#include "openMVG/features/regions_factory.hpp"
#include "openMVG/matching_image_collection/E_ACRobust.hpp"
#include "openMVG/matching_image_collection/E_ACRobust_Angular.hpp"
#include "openMVG/matching_image_collection/Eo_Robust.hpp"
#include "openMVG/matching_image_collection/F_ACRobust.hpp"
#include "openMVG/matching_image_collection/H_ACRobust.hpp"
#include "openMVG/matching_image_collection/GeometricFilter.hpp"
#include "openMVG/sfm/pipelines/sfm_regions_provider.hpp"
#include "openMVG/sfm/sfm_data.hpp"

namespace {
struct InMemoryRegionsProvider : public sfm::Regions_Provider {
  void set(IndexT id, std::shared_ptr<features::Regions> r) { cache_[id] = std::move(r); }
  void set_type(features::Regions* t) { region_type_.reset(t); }
};
}  // namespace

extern "C" typedef void (*geo_sink)(void* user, uint32_t I, uint32_t J, const uint32_t* ij, uint32_t n);

// the region type the container entries below build: 0 SIFT_Regions (128 bytes per feature, the default), 1 AKAZE_Float_Regions (64 floats),
// 2 AKAZE_Binary_Regions (64 bytes) - `descs` is read with that row size
static int g_container_region_type = 0;
extern "C" void ref_geofilter_container_region_type(int t) { g_container_region_type = t; }
namespace {
template <class RegionsT>
std::shared_ptr<features::Regions> make_regions(const float* feat_xy, const uint8_t* descs, uint64_t lo, uint64_t n) {
  auto r = std::make_shared<RegionsT>();
  r->Features().resize(n);
  r->Descriptors().resize(n);
  constexpr size_t kRowBytes = sizeof(typename RegionsT::DescriptorT);
  for (uint64_t i = 0; i < n; ++i) {
    r->Features()[i] = features::SIOPointFeature(feat_xy[2 * (lo + i)], feat_xy[2 * (lo + i) + 1], 1.f, 0.f);
    if (descs) std::memcpy(r->Descriptors()[i].data(), descs + (lo + i) * kRowBytes, kRowBytes);
    else std::memset(r->Descriptors()[i].data(), 0, kRowBytes);
  }
  return r;
}
}  // namespace

// images: feat_xy (2 floats per feature, image k owning [feat_start[k], feat_start[k + 1])), descs (128 bytes per feature or NULL),
// image_wh (w, h per image); k1 != 0: all views share one Pinhole_Intrinsic_Radial_K1 (the positions are then undistorted by
// MatchesPairToMat). putative matches: pairs_IJ, match_start, matches_ij (feature indices). The geometric matches are handed to
// `sink` in container order. Returns the number of pairs in the result.
template <class Functor>
static uint64_t container_impl(const float* feat_xy, const uint8_t* descs, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                               const uint32_t* pairs_IJ, const uint64_t* match_start, const uint32_t* matches_ij, uint64_t n_pairs,
                               double precision, uint32_t max_iterations, int guided, double distance_ratio, double k1, geo_sink sink, void* user,
                               double pinhole_focal = 0.0) {
  sfm::SfM_Data scene;
  auto provider = std::make_shared<InMemoryRegionsProvider>();
  if (g_container_region_type == 1) provider->set_type(new features::AKAZE_Float_Regions());
  else if (g_container_region_type == 2) provider->set_type(new features::AKAZE_Binary_Regions());
  else provider->set_type(new features::SIFT_Regions());
  for (uint32_t k = 0; k < n_images; ++k) {
    // pinhole_focal > 0: every view has its own Pinhole_Intrinsic (focal given, principal point at the centre) - except the LAST view, which
    // keeps no intrinsic, so that the essential functor's "no intrinsic information" branch is exercised by its pairs
    const bool own_pinhole = pinhole_focal > 0.0 && (k + 1 < n_images || n_images < 3);
    scene.views[k] = std::make_shared<sfm::View>("", k, k1 != 0.0 ? 0 : own_pinhole ? k : UndefinedIndexT, UndefinedIndexT, image_wh[2 * k], image_wh[2 * k + 1]);
    if (own_pinhole)
      scene.intrinsics[k] = std::make_shared<cameras::Pinhole_Intrinsic>(image_wh[2 * k], image_wh[2 * k + 1], pinhole_focal, image_wh[2 * k] / 2.0, image_wh[2 * k + 1] / 2.0);
    const uint64_t lo = feat_start[k], n = feat_start[k + 1] - lo;
    provider->set(k, g_container_region_type == 1   ? make_regions<features::AKAZE_Float_Regions>(feat_xy, descs, lo, n)
                     : g_container_region_type == 2 ? make_regions<features::AKAZE_Binary_Regions>(feat_xy, descs, lo, n)
                                                    : make_regions<features::SIFT_Regions>(feat_xy, descs, lo, n));
  }
  if (k1 != 0.0)
    scene.intrinsics[0] = std::make_shared<cameras::Pinhole_Intrinsic_Radial_K1>(image_wh[0], image_wh[1], 0.9 * image_wh[0], image_wh[0] / 2.0, image_wh[1] / 2.0, k1);
  matching::PairWiseMatches putative;
  for (uint64_t p = 0; p < n_pairs; ++p) {
    matching::IndMatches m;
    for (uint64_t i = match_start[p]; i < match_start[p + 1]; ++i) m.emplace_back(matches_ij[2 * i], matches_ij[2 * i + 1]);
    putative.insert({{pairs_IJ[2 * p], pairs_IJ[2 * p + 1]}, std::move(m)});
  }
  std::shared_ptr<sfm::Regions_Provider> base = provider;
  matching_image_collection::ImageCollectionGeometricFilter filter(&scene, base);
  try {   // (the reference's filter never throws; a replacement asked to - MVGX_ON_DEVICE_ERROR=throw - must not unwind into ctypes)
    filter.Robust_model_estimation(Functor(precision, max_iterations), putative, guided != 0, distance_ratio);
  } catch (const std::exception&) {
    return UINT64_MAX;
  }
  const matching::PairWiseMatches& out = filter.Get_geometric_matches();
  std::vector<uint32_t> buf;
  for (const auto& kv : out) {
    buf.clear();
    for (const auto& m : kv.second) { buf.push_back(m.i_); buf.push_back(m.j_); }
    sink(user, kv.first.first, kv.first.second, buf.data(), (uint32_t)kv.second.size());
  }
  return out.size();
}

extern "C" {
uint64_t ref_geofilter_container(const float* feat_xy, const uint8_t* descs, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                 const uint32_t* pairs_IJ, const uint64_t* match_start, const uint32_t* matches_ij, uint64_t n_pairs,
                                 double precision, uint32_t max_iterations, int guided, double distance_ratio, double k1, geo_sink sink, void* user) {
  return container_impl<matching_image_collection::GeometricFilter_FMatrix_AC>(feat_xy, descs, feat_start, image_wh, n_images, pairs_IJ, match_start, matches_ij,
                                                                               n_pairs, precision, max_iterations, guided, distance_ratio, k1, sink, user);
}
// the same caller with the homography functor (H_ACRobust.hpp)
uint64_t ref_geofilter_container_h(const float* feat_xy, const uint8_t* descs, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                   const uint32_t* pairs_IJ, const uint64_t* match_start, const uint32_t* matches_ij, uint64_t n_pairs,
                                   double precision, uint32_t max_iterations, int guided, double distance_ratio, double k1, geo_sink sink, void* user) {
  return container_impl<matching_image_collection::GeometricFilter_HMatrix_AC>(feat_xy, descs, feat_start, image_wh, n_images, pairs_IJ, match_start, matches_ij,
                                                                               n_pairs, precision, max_iterations, guided, distance_ratio, k1, sink, user);
}
// the essential functor (E_ACRobust.hpp): every view but the last carries a Pinhole_Intrinsic of the given focal
uint64_t ref_geofilter_container_e(const float* feat_xy, const uint8_t* descs, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                   const uint32_t* pairs_IJ, const uint64_t* match_start, const uint32_t* matches_ij, uint64_t n_pairs,
                                   double precision, uint32_t max_iterations, int guided, double distance_ratio, double focal, geo_sink sink, void* user) {
  return container_impl<matching_image_collection::GeometricFilter_EMatrix_AC>(feat_xy, descs, feat_start, image_wh, n_images, pairs_IJ, match_start, matches_ij,
                                                                               n_pairs, precision, max_iterations, guided, distance_ratio, 0.0, sink, user, focal);
}
// the angular essential functors (E_ACRobust_Angular.hpp; -g a / -g u): pinhole views as above, bearing vectors by the cameras' operator()
uint64_t ref_geofilter_container_ea(const float* feat_xy, const uint8_t* descs, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                    const uint32_t* pairs_IJ, const uint64_t* match_start, const uint32_t* matches_ij, uint64_t n_pairs,
                                    double precision, uint32_t max_iterations, int upright, double focal, geo_sink sink, void* user) {
  if (upright)
    return container_impl<matching_image_collection::GeometricFilter_ESphericalMatrix_AC_Angular<true>>(
        feat_xy, descs, feat_start, image_wh, n_images, pairs_IJ, match_start, matches_ij, n_pairs, precision, max_iterations, 0, 0.8, 0.0, sink, user, focal);
  return container_impl<matching_image_collection::GeometricFilter_ESphericalMatrix_AC_Angular<false>>(
      feat_xy, descs, feat_start, image_wh, n_images, pairs_IJ, match_start, matches_ij, n_pairs, precision, max_iterations, 0, 0.8, 0.0, sink, user, focal);
}
// the orthographic essential functor (Eo_Robust.hpp; -g o): pinhole views as above
uint64_t ref_geofilter_container_eo(const float* feat_xy, const uint8_t* descs, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                    const uint32_t* pairs_IJ, const uint64_t* match_start, const uint32_t* matches_ij, uint64_t n_pairs,
                                    double precision, uint32_t max_iterations, int guided, double distance_ratio, double focal, geo_sink sink, void* user) {
  return container_impl<matching_image_collection::GeometricFilter_EOMatrix_RA>(feat_xy, descs, feat_start, image_wh, n_images, pairs_IJ, match_start, matches_ij,
                                                                                n_pairs, precision, max_iterations, guided, distance_ratio, 0.0, sink, user, focal);
}
}  // extern "C"

// Guided matching: the reference's own template (robust_estimation/guided_matching.hpp:178-227, the Regions overload that
// {F,H,E}_ACRobust.hpp's Geometry_guided_matching call) for ONE image pair. cam = nullptr on both sides: the positions are compared as
// they are stored (SIOPointFeature holds floats: pass positions that are exact in float). kind 0: EpipolarDistanceError, 1: AsymmetricError.
// out_ij: capacity 2 nI; returns the number of matches.
#include "openMVG/robust_estimation/guided_matching.hpp"
#include "openMVG/multiview/solver_fundamental_kernel.hpp"
#include "openMVG/multiview/solver_homography_kernel.hpp"
extern "C" uint64_t ref_guided_match(int kind, const double* M, const float* xyI, const uint8_t* descI, uint64_t nI, const float* xyJ, const uint8_t* descJ,
                                     uint64_t nJ, double error_th, double dist_ratio, uint32_t* out_ij) {
  auto make = [](const float* xy, const uint8_t* d, uint64_t n) {
    auto r = std::make_shared<features::SIFT_Regions>();
    r->Features().resize(n);
    r->Descriptors().resize(n);
    for (uint64_t i = 0; i < n; ++i) {
      r->Features()[i] = features::SIOPointFeature(xy[2 * i], xy[2 * i + 1], 1.f, 0.f);
      std::memcpy(r->Descriptors()[i].data(), d + i * 128, 128);
    }
    return r;
  };
  const auto rI = make(xyI, descI, nI), rJ = make(xyJ, descJ, nJ);
  Mat3 mod;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) mod(r, c) = M[3 * r + c];
  matching::IndMatches out;
  if (kind == 0)
    geometry_aware::GuidedMatching<Mat3, openMVG::fundamental::kernel::EpipolarDistanceError>(mod, nullptr, *rI, nullptr, *rJ, error_th, dist_ratio, out);
  else
    geometry_aware::GuidedMatching<Mat3, openMVG::homography::kernel::AsymmetricError>(mod, nullptr, *rI, nullptr, *rJ, error_th, dist_ratio, out);
  for (size_t k = 0; k < out.size(); ++k) { out_ij[2 * k] = out[k].i_; out_ij[2 * k + 1] = out[k].j_; }
  return out.size();
}

// ... and on the other region types the functors can meet (round 6): desc_type 1 = AKAZE_Float_Regions (64 floats per row), 2 =
// AKAZE_Binary_Regions (64 bytes per row) - the regions' own virtual SquaredDescriptorDistance decides the metric (guided_matching.hpp:213).
template <class RegionsT, class ElemT>
static uint64_t ref_guided_match_on(int kind, const double* M, const float* xyI, const ElemT* descI, uint64_t nI, const float* xyJ, const ElemT* descJ, uint64_t nJ,
                                    double error_th, double dist_ratio, uint32_t* out_ij) {
  auto make = [](const float* xy, const ElemT* d, uint64_t n) {
    auto r = std::make_shared<RegionsT>();
    r->Features().resize(n);
    r->Descriptors().resize(n);
    constexpr size_t L = RegionsT::DescriptorT::static_size;
    for (uint64_t i = 0; i < n; ++i) {
      r->Features()[i] = features::SIOPointFeature(xy[2 * i], xy[2 * i + 1], 1.f, 0.f);
      std::memcpy(r->Descriptors()[i].data(), d + i * L, L * sizeof(ElemT));
    }
    return r;
  };
  const auto rI = make(xyI, descI, nI), rJ = make(xyJ, descJ, nJ);
  Mat3 mod;
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) mod(r, c) = M[3 * r + c];
  matching::IndMatches out;
  if (kind == 0)
    geometry_aware::GuidedMatching<Mat3, openMVG::fundamental::kernel::EpipolarDistanceError>(mod, nullptr, *rI, nullptr, *rJ, error_th, dist_ratio, out);
  else
    geometry_aware::GuidedMatching<Mat3, openMVG::homography::kernel::AsymmetricError>(mod, nullptr, *rI, nullptr, *rJ, error_th, dist_ratio, out);
  for (size_t k = 0; k < out.size(); ++k) { out_ij[2 * k] = out[k].i_; out_ij[2 * k + 1] = out[k].j_; }
  return out.size();
}
extern "C" uint64_t ref_guided_match_typed(int kind, int desc_type, const double* M, const float* xyI, const void* descI, uint64_t nI, const float* xyJ,
                                           const void* descJ, uint64_t nJ, double error_th, double dist_ratio, uint32_t* out_ij) {
  if (desc_type == 1)
    return ref_guided_match_on<features::AKAZE_Float_Regions, float>(kind, M, xyI, static_cast<const float*>(descI), nI, xyJ, static_cast<const float*>(descJ), nJ,
                                                                     error_th, dist_ratio, out_ij);
  if (desc_type == 2)
    return ref_guided_match_on<features::AKAZE_Binary_Regions, unsigned char>(kind, M, xyI, static_cast<const unsigned char*>(descI), nI, xyJ,
                                                                              static_cast<const unsigned char*>(descJ), nJ, error_th, dist_ratio, out_ij);
  return ref_guided_match_on<features::SIFT_Regions, unsigned char>(kind, M, xyI, static_cast<const unsigned char*>(descI), nI, xyJ,
                                                                    static_cast<const unsigned char*>(descJ), nJ, error_th, dist_ratio, out_ij);
}
