// The cheirality stage of the relative pose on DEVICE pointers: what mvgx_relative_pose_from_essential (mvgx_relative_pose.h, in
// mvgx_ba.hip's unit beside the two-view triangulation it calls) and mvgx_relative_pose_robust (mvgx_relative_pose_robust.h, in
// mvgx_geofilter.hip's unit beside the a-contrario stage it chains) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mvgx.h"

namespace mvgx {

struct RelPoseLaunch {
  uint32_t n_pairs;
  const uint64_t* start;       // n_pairs + 1: the pair's correspondences in bI / bJ (3 doubles each)
  const double *bI, *bJ;
  const double* E;             // the pair's matrix at E + p * e_stride (row-major)
  uint32_t e_stride;           // doubles
  int normalize_e;             // scale E to unit Frobenius norm first (what the angular filter's result carries)
  // the list of a pair, one of: use_index rows [use_start[p], use_start[p + 1]) | every correspondence (use_index == nullptr), of
  // which, where mask != nullptr, those with mask[start[p] + i] != 0
  const uint64_t* use_start;
  const uint32_t* use_index;
  const uint8_t* mask;
  // a pair is voted on only if !(n_inliers[p * n_inliers_stride] < min_inliers) (n_inliers == nullptr: every pair)
  const uint32_t* n_inliers;
  uint32_t n_inliers_stride;   // words
  double min_inliers;
  int method;                  // ETriangulationMethod 0..3
  double ratio;
  // outputs: the pair's slots of out_selected / out_X start where its list does (use_start[p], or start[p]); the first n_selected are written
  mvgx_relative_pose_result* results;
  uint32_t* out_selected;      // may be nullptr
  double* out_X;               // may be nullptr
};

// enqueues the kernel on `stream`; every pointer is device memory
int relative_pose_launch(const RelPoseLaunch& a, hipStream_t stream);

}  // namespace mvgx
