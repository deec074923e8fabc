// mvgx_relative_pose.h — from an essential matrix to (R, t) by cheirality, a batch of pairs on the device: the kernel, its launch on
// device pointers (mvgx_relative_pose_internal.h) and the host entry mvgx_relative_pose_from_essential.
// Included at the end of mvgx_ba.hip after mvgx_triangulate.h: it calls that header's two-view triangulation (tri_two_view_closed,
// tri_dlt_point / tri_dlt_in_front) and is compiled under the same contraction mode.
//
// What the reference does on the host, per pair (paths under src/openMVG of the reference):
//   multiview/essential.cpp:79-113              MotionFromEssential: JacobiSVD of E, U.col(2) / Vt.row(2) negated where the determinant
//                                               is negative, R in {U W V^T, U W^T V^T}, t = +-U.col(2); the four poses in the order
//                                               (R0, t0) (R1, t1) (R0, t1) (R1, t0)
//   multiview/motion_from_essential.cpp:20-95   RelativePoseFromEssential: Triangulate2View of every listed correspondence under each of
//                                               the four, std::max_element (the first maximum), 0 points -> false, the two largest
//                                               counts of the sorted accumulator: second / best < ratio
//
// Exact: the decisions (first maximum, the ratio in double arithmetic), the order of the selected list. To rounding: R, t and the points
// (one-sided Jacobi iteration instead of Eigen's two-sided one; fused multiply-adds). The order of the four candidates follows the sign
// choices of this iteration and is not always Eigen's (include/mvgx.h says what that can and cannot change).
//
// One wave per pair. The SVD of E runs redundantly in every lane (named scalars, no cross-lane traffic: a 3 x 3 iteration is some
// hundred operations, and the wave has nothing else to do meanwhile). Pass 1: the four 16-lane rows of the wave take the four candidates,
// lane l of row r the list entries l, l + 16, ...; one ballot per step counts all four. The decision is wave-uniform. Pass 2: all 64
// lanes triangulate the list under the winner - whose R | t they fetch from a lane of its row, not compute again - and compact
// positions and points in list order by ballot + prefix count. The two passes are ONE loop body run twice (never unrolled), so the
// triangulation exists once in the code object and a correspondence gets the same verdict in both: n_selected == cheirality[winner].
#pragma once

#include "mvgx_relative_pose_internal.h"

namespace {

constexpr int kRelPoseSweeps = 15;

struct RelPoseDev {
  const uint64_t* start;
  const double *bI, *bJ, *E;
  const uint64_t* use_start;
  const uint32_t* use_index;
  const uint8_t* mask;
  const uint32_t* n_inliers;
  mvgx_relative_pose_result* results;
  uint32_t* out_selected;
  double* out_X;
  double min_inliers, ratio;
  uint32_t e_stride, n_inliers_stride;
  int normalize_e, method;
};

// columns p and q of a 3 x 3 matrix and of V: the plane rotation from the right that makes the two columns orthogonal (tri_hestenes_rot
// with three rows)
__device__ __forceinline__ bool relpose_rot(double& a0p, double& a0q, double& a1p, double& a1q, double& a2p, double& a2q,
                                            double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
  const double app = a0p * a0p + a1p * a1p + a2p * a2p, aqq = a0q * a0q + a1q * a1q + a2q * a2q;
  const double apq = a0p * a0q + a1p * a1q + a2p * a2q;
  if (!(fabs(apq) > 2.220446049250313e-16 * sqrt(app * aqq))) return false;   // orthogonal at this precision (a zero column, a NaN included)
  const double th = (aqq - app) / (2.0 * apq);
  const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));   // th^2 = inf -> t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  double x, y;
  x = a0p; y = a0q; a0p = c * x - s * y; a0q = s * x + c * y;
  x = a1p; y = a1q; a1p = c * x - s * y; a1q = s * x + c * y;
  x = a2p; y = a2q; a2p = c * x - s * y; a2q = s * x + c * y;
  x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
  x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
  x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
  return true;
}
// columns a and b of the rotated matrix and of V change places where b is the longer one (strictly: equal columns keep their order)
__device__ __forceinline__ void relpose_order(double& na, double& nb, double& a0, double& b0, double& a1, double& b1, double& a2, double& b2,
                                              double& v0a, double& v0b, double& v1a, double& v1b, double& v2a, double& v2b) {
  const bool sw = nb > na;
  double x;
  x = sw ? nb : na; nb = sw ? na : nb; na = x;
  x = sw ? b0 : a0; b0 = sw ? a0 : b0; a0 = x;
  x = sw ? b1 : a1; b1 = sw ? a1 : b1; a1 = x;
  x = sw ? b2 : a2; b2 = sw ? a2 : b2; a2 = x;
  x = sw ? v0b : v0a; v0b = sw ? v0a : v0b; v0a = x;
  x = sw ? v1b : v1a; v1b = sw ? v1a : v1b; v1a = x;
  x = sw ? v2b : v2a; v2b = sw ? v2a : v2b; v2a = x;
}
// E scaled to unit Frobenius norm as the host side of the angular filter does it (products and sums rounded one by one: the same bits)
__device__ __forceinline__ void relpose_unit_norm(double E[9]) {
#pragma clang fp contract(off)
  double n2 = 0.0;
#pragma unroll
  for (int u = 0; u < 9; ++u) n2 += E[u] * E[u];
  if (n2 > 0.0) {
    const double len = sqrt(n2);
#pragma unroll
    for (int u = 0; u < 9; ++u) E[u] /= len;
  }
}
// MotionFromEssential (essential.cpp:79-113). E = U S V^T with S descending: a one-sided Jacobi iteration on the columns of E (E V = U S),
// the columns ordered by length; u3 = u1 x u2 and v3 = v1 x v2 are the third columns the two determinant fixes leave (det U = det V = +1;
// the third column of E V is zero for a true essential matrix and carries no direction). With W = [0 -1 0; 1 0 0; 0 0 1]:
// U W V^T = u2 v1^T - u1 v2^T + u3 v3^T and U W^T V^T = u1 v2^T - u2 v1^T + u3 v3^T. Out: A = u2 v1^T - u1 v2^T, B = u3 v3^T, u3.
// The iteration works on E times the power of two that brings its largest entry to [1, 2): its tests compare products of squared column
// lengths, fourth powers of the scale of E, which overflow above 1e77 and vanish below 1e-81 while E itself is an ordinary double - and
// the decomposition does not depend on the scale (the reference's JacobiSVD divides by the largest entry). A power of two changes no
// mantissa, so E and 2^k E give the same bits by construction. (Against the iteration on E as given, the results are the same bits in
// IEEE arithmetic; on the device they move by a unit or two in the last place)
// An E with an entry that is not finite becomes all NaN here (no comparison with a NaN holds: no rotation, no point in front, every count
// 0) - a NaN confined to one column would otherwise leave the two other columns to pass for a motion.
__device__ __forceinline__ void relpose_motion(const double E[9], double A[9], double B[9], double u3[3]) {
  double big = 0.0;
  bool finite = true;
#pragma unroll
  for (int u = 0; u < 9; ++u) { big = fmax(big, fabs(E[u])); finite = finite && fabs(E[u]) < INFINITY; }
  int ex = 1;
  if (finite && big > 0.0) (void)frexp(big, &ex);   // big = f 2^ex, f in [0.5, 1) (a subnormal included)
  double W[9];
#pragma unroll
  for (int u = 0; u < 9; ++u) W[u] = finite ? ldexp(E[u], 1 - ex) : NAN;   // (a select, not a sum: -0.0 stays -0.0)
  double a00 = W[0], a01 = W[1], a02 = W[2], a10 = W[3], a11 = W[4], a12 = W[5], a20 = W[6], a21 = W[7], a22 = W[8];   // a_rc
  double v00 = 1, v01 = 0, v02 = 0, v10 = 0, v11 = 1, v12 = 0, v20 = 0, v21 = 0, v22 = 1;
#pragma unroll 1
  for (int sweep = 0; sweep < kRelPoseSweeps; ++sweep) {
    bool any = relpose_rot(a00, a01, a10, a11, a20, a21, v00, v01, v10, v11, v20, v21);          // (0, 1)
    any = relpose_rot(a00, a02, a10, a12, a20, a22, v00, v02, v10, v12, v20, v22) || any;        // (0, 2)
    any = relpose_rot(a01, a02, a11, a12, a21, a22, v01, v02, v11, v12, v21, v22) || any;        // (1, 2)
    if (!any) break;
  }
  double n0 = a00 * a00 + a10 * a10 + a20 * a20, n1 = a01 * a01 + a11 * a11 + a21 * a21, n2 = a02 * a02 + a12 * a12 + a22 * a22;
  relpose_order(n0, n1, a00, a01, a10, a11, a20, a21, v00, v01, v10, v11, v20, v21);
  relpose_order(n1, n2, a01, a02, a11, a12, a21, a22, v01, v02, v11, v12, v21, v22);
  relpose_order(n0, n1, a00, a01, a10, a11, a20, a21, v00, v01, v10, v11, v20, v21);
  const double l0 = n0 > 0.0 ? sqrt(n0) : 1.0, l1 = n1 > 0.0 ? sqrt(n1) : 1.0;
  const double u1[3] = {a00 / l0, a10 / l0, a20 / l0}, u2[3] = {a01 / l1, a11 / l1, a21 / l1};
  const double v1[3] = {v00, v10, v20}, v2[3] = {v01, v11, v21};
  double v3[3];
  tri_cross(u1, u2, u3);
  tri_cross(v1, v2, v3);
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      A[3 * i + j] = u2[i] * v1[j] - u1[i] * v2[j];
      B[3 * i + j] = u3[i] * v3[j];
    }
}

// kDlt: Triangulate2View by the DLT (method 0) - a kernel of its own, so that its Jacobi iteration costs the closed forms no register
template <bool kDlt>
__global__ __launch_bounds__(64) void relpose_cheirality_kernel(RelPoseDev d) {
  const uint32_t p = blockIdx.x;
  const int lane = threadIdx.x & 63, row = lane >> 4;
  const uint64_t c0 = d.start[p];
  const uint32_t n = (uint32_t)(d.start[p + 1] - c0);
  const uint64_t u0 = d.use_index ? d.use_start[p] : c0;   // where the pair's list, and its output slots, start
  uint32_t m = d.use_index ? (uint32_t)(d.use_start[p + 1] - u0) : n;
  if (d.n_inliers && (double)d.n_inliers[(size_t)p * d.n_inliers_stride] < d.min_inliers) m = 0;   // not voted on: every count stays 0

  double E[9];
#pragma unroll
  for (int u = 0; u < 9; ++u) E[u] = d.E[(size_t)p * d.e_stride + u];
  if (d.normalize_e) relpose_unit_norm(E);
  // this lane's candidate: row 0 (R0, +u3), 1 (R1, -u3), 2 (R0, -u3), 3 (R1, +u3) - by selects on the row, never an array indexed by it
  double Rt[12];
  {
    double A[9], B[9], u3[3];
    relpose_motion(E, A, B, u3);
    const bool second = (row & 1) != 0, plus = row == 0 || row == 3;
#pragma unroll
    for (int k = 0; k < 9; ++k) Rt[k] = second ? B[k] - A[k] : B[k] + A[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) Rt[9 + k] = plus ? u3[k] : -u3[k];
  }
  const double Rt0[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};   // pose1: the identity at the origin

  uint32_t cnt0 = 0, cnt1 = 0, cnt2 = 0, cnt3 = 0, n_sel = 0;
  int win = 0;
  bool ok = false;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    if (pass) {
      // the decision (motion_from_essential.cpp:72-94): the first maximum; the two largest of the sorted counts
      uint32_t best = cnt0;
      if (cnt1 > best) { best = cnt1; win = 1; }
      if (cnt2 > best) { best = cnt2; win = 2; }
      if (cnt3 > best) { best = cnt3; win = 3; }
      const uint32_t hi01 = cnt0 > cnt1 ? cnt0 : cnt1, lo01 = cnt0 > cnt1 ? cnt1 : cnt0, hi23 = cnt2 > cnt3 ? cnt2 : cnt3, lo23 = cnt2 > cnt3 ? cnt3 : cnt2;
      const uint32_t mid_a = hi01 < hi23 ? hi01 : hi23, mid_b = lo01 > lo23 ? lo01 : lo23;
      const uint32_t second = mid_a > mid_b ? mid_a : mid_b;
      ok = best > 0 && (double)second / static_cast<double>(best) < d.ratio;
      if (!ok) break;   // (wave-uniform)
#pragma unroll
      for (int k = 0; k < 12; ++k) Rt[k] = __shfl(Rt[k], 16 * win);
    }
    const uint32_t step = pass ? 64u : 16u, mine = pass ? (uint32_t)lane : (uint32_t)(lane & 15);
#pragma unroll 1
    for (uint32_t base = 0; base < m; base += step) {
      const uint32_t e = base + mine;
      bool valid = e < m;
      uint32_t idx = 0;
      if (valid) idx = d.use_index ? d.use_index[u0 + e] : e;
      if (valid && d.mask) valid = d.mask[c0 + idx] != 0;
      double X[3] = {0.0, 0.0, 0.0};
      bool front = false;
      if (valid) {
        const double* pi = d.bI + 3 * (size_t)(c0 + idx);
        const double* pj = d.bJ + 3 * (size_t)(c0 + idx);
        const double x0[3] = {pi[0], pi[1], pi[2]}, x1[3] = {pj[0], pj[1], pj[2]};
        if constexpr (kDlt) {
          tri_dlt_point(Rt0, x0, Rt, x1, X);
          front = tri_dlt_in_front(Rt0, Rt, X);
        } else {
          front = tri_two_view_closed(d.method, Rt0, x0, Rt, x1, X);
        }
      }
      const unsigned long long bal = __ballot(front);
      if (!pass) {
        cnt0 += (uint32_t)__popcll(bal & 0xffffull); cnt1 += (uint32_t)__popcll((bal >> 16) & 0xffffull);
        cnt2 += (uint32_t)__popcll((bal >> 32) & 0xffffull); cnt3 += (uint32_t)__popcll(bal >> 48);
      } else {
        if (front) {
          const uint64_t slot = u0 + n_sel + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
          if (d.out_selected) d.out_selected[slot] = idx;
          if (d.out_X) { d.out_X[3 * slot] = X[0]; d.out_X[3 * slot + 1] = X[1]; d.out_X[3 * slot + 2] = X[2]; }
        }
        n_sel += (uint32_t)__popcll(bal);
      }
    }
  }
  if (lane == 0) {
    mvgx_relative_pose_result& r = d.results[p];
#pragma unroll
    for (int k = 0; k < 12; ++k) r.pose[(k < 9 ? 4 * (k / 3) + k % 3 : 4 * (k - 9) + 3)] = ok ? Rt[k] : 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) r.pose[12 + j] = ok ? -(Rt[j] * Rt[9] + Rt[3 + j] * Rt[10] + Rt[6 + j] * Rt[11]) : 0.0;   // C = -R^T t
#pragma unroll
    for (int u = 0; u < 9; ++u) r.E[u] = E[u];
    r.found_precision = 0.0;
    r.cheirality[0] = cnt0; r.cheirality[1] = cnt1; r.cheirality[2] = cnt2; r.cheirality[3] = cnt3;
    r.n_acransac_inliers = 0;
    r.n_selected = ok ? n_sel : 0;
    r.ok = ok ? 1u : 0u;
  }
}

template <typename T>
int relpose_upload(mvgx::DevBuf<T>& dst, const T* src, size_t n, hipStream_t stream) {
  const int rc = dst.ensure(std::max<size_t>(n, 1));
  if (rc) return rc;
  if (n) MVGX_HIP(hipMemcpyAsync(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
  return MVGX_OK;
}

}  // namespace

namespace mvgx {

int relative_pose_launch(const RelPoseLaunch& a, hipStream_t stream) {
  if (!a.n_pairs) return MVGX_OK;
  MVGX_REQUIRE(a.method >= 0 && a.method <= 3, MVGX_ERR_ARG, "relative pose: method %d", a.method);
  RelPoseDev d;
  d.start = a.start; d.bI = a.bI; d.bJ = a.bJ; d.E = a.E; d.use_start = a.use_start; d.use_index = a.use_index; d.mask = a.mask;
  d.n_inliers = a.n_inliers; d.results = a.results; d.out_selected = a.out_selected; d.out_X = a.out_X; d.min_inliers = a.min_inliers;
  d.ratio = a.ratio; d.e_stride = a.e_stride; d.n_inliers_stride = a.n_inliers_stride; d.normalize_e = a.normalize_e; d.method = a.method;
  if (a.method == 0) hipLaunchKernelGGL(relpose_cheirality_kernel<true>, dim3(a.n_pairs), dim3(64), 0, stream, d);
  else hipLaunchKernelGGL(relpose_cheirality_kernel<false>, dim3(a.n_pairs), dim3(64), 0, stream, d);
  BA_LAUNCH_CHECK();
  return MVGX_OK;
}

}  // namespace mvgx

extern "C" {

void mvgx_relative_pose_default_options(mvgx_relative_pose_options* o) {
  if (!o) return;
  // RelativePoseFromEssential's defaults (motion_from_essential.hpp: 0.7, ETriangulationMethod::DEFAULT); Relative_Pose_Engine's bound and count
  o->kind = MVGX_RELPOSE_PINHOLE; o->method = 3; o->positive_depth_ratio = 0.7; o->residual_tolerance = 2.5 * 2.5; o->max_iterations = 256;
}

int mvgx_relative_pose_from_essential(int device, uint32_t n_pairs, const uint64_t* start, const double* bearingI, const double* bearingJ, const double* E,
                                      const uint64_t* use_start, const uint32_t* use_index, const mvgx_relative_pose_options* opt,
                                      mvgx_relative_pose_result* results, uint64_t* out_selected_start, uint32_t* out_selected, double* out_X,
                                      mvgx_relative_pose_stats* stats) {
  using clock = std::chrono::steady_clock;
  const auto t_begin = clock::now();
  MVGX_REQUIRE(opt && start && out_selected_start, MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: NULL options, start or out_selected_start");
  MVGX_REQUIRE(opt->method >= 0 && opt->method <= 3, MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: method %d", opt->method);
  MVGX_REQUIRE(opt->positive_depth_ratio > 0.0 && opt->positive_depth_ratio <= 1.0, MVGX_ERR_ARG,
               "mvgx_relative_pose_from_essential: positive_depth_ratio %g is outside (0, 1]", opt->positive_depth_ratio);
  MVGX_REQUIRE(!n_pairs || (results && E), MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: NULL results or E");
  MVGX_REQUIRE(!use_index || use_start, MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: use_index without use_start");
  for (uint32_t p = 0; p < n_pairs; ++p) {
    MVGX_REQUIRE(start[p] <= start[p + 1] && start[p + 1] - start[p] < (1ull << 31), MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: start is not monotone at pair %u", p);
    if (!use_index) continue;
    MVGX_REQUIRE(use_start[p] <= use_start[p + 1] && use_start[p + 1] - use_start[p] < (1ull << 31), MVGX_ERR_ARG,
                 "mvgx_relative_pose_from_essential: use_start is not monotone at pair %u", p);
    const uint64_t n = start[p + 1] - start[p];
    for (uint64_t u = use_start[p]; u < use_start[p + 1]; ++u)
      MVGX_REQUIRE(use_index[u] < n, MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: pair %u lists position %u of %llu", p, use_index[u], (unsigned long long)n);
  }
  // correspondences are addressed from start[0], list entries from use_start[0]: the arrays are taken from there
  const uint64_t c_base = start[0], n_corr = start[n_pairs] - c_base;
  const uint64_t u_base = use_index ? use_start[0] : c_base, n_list = use_index ? use_start[n_pairs] - u_base : n_corr;
  MVGX_REQUIRE(!n_corr || (bearingI && bearingJ), MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: NULL bearing vectors");
  MVGX_REQUIRE(!n_list || (out_selected && out_X), MVGX_ERR_ARG, "mvgx_relative_pose_from_essential: NULL output list");
  if (stats) memset(stats, 0, sizeof(*stats));
  out_selected_start[0] = 0;
  if (!n_pairs) return MVGX_OK;
  int rc;
  if ((rc = mvgx::select_device(device < 0 ? -1 : device))) return rc;

  std::vector<uint64_t> h_start((size_t)n_pairs + 1), h_ustart(use_index ? (size_t)n_pairs + 1 : 0);
  for (uint32_t p = 0; p <= n_pairs; ++p) h_start[p] = start[p] - c_base;
  for (uint32_t p = 0; use_index && p <= n_pairs; ++p) h_ustart[p] = use_start[p] - u_base;
  std::vector<mvgx_relative_pose_result> h_res(n_pairs);
  std::vector<uint32_t> h_sel(n_list);
  std::vector<double> h_X(3 * n_list);

  mvgx::DevBuf<double> d_bI, d_bJ, d_E, d_X;   // (before the stream guard: drained first, freed after)
  mvgx::DevBuf<uint64_t> d_start, d_ustart;
  mvgx::DevBuf<uint32_t> d_uidx, d_sel;
  mvgx::DevBuf<mvgx_relative_pose_result> d_res;
  hipStream_t stream = nullptr;
  if ((rc = mvgx::acquire_stream(&stream))) return rc;
  int stream_device = 0;
  MVGX_HIP(hipGetDevice(&stream_device));
  mvgx::StreamGuard sg{stream_device, stream};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  MVGX_HIP(hipEventCreate(&e0));
  MVGX_HIP(hipEventCreate(&e1));
  mvgx::EventGuard eg{e0, e1};

  if ((rc = relpose_upload(d_start, h_start.data(), h_start.size(), stream)) || (rc = relpose_upload(d_ustart, h_ustart.data(), h_ustart.size(), stream)) ||
      (rc = relpose_upload(d_uidx, use_index ? use_index + u_base : nullptr, use_index ? n_list : 0, stream)) ||
      (rc = relpose_upload(d_bI, n_corr ? bearingI + 3 * c_base : nullptr, 3 * n_corr, stream)) ||
      (rc = relpose_upload(d_bJ, n_corr ? bearingJ + 3 * c_base : nullptr, 3 * n_corr, stream)) || (rc = relpose_upload(d_E, E, (size_t)n_pairs * 9, stream)))
    return rc;
  if ((rc = d_res.ensure(n_pairs)) || (rc = d_sel.ensure(std::max<size_t>(n_list, 1))) || (rc = d_X.ensure(std::max<size_t>(3 * n_list, 1)))) return rc;

  mvgx::RelPoseLaunch a{};
  a.n_pairs = n_pairs; a.start = d_start.p; a.bI = d_bI.p; a.bJ = d_bJ.p; a.E = d_E.p; a.e_stride = 9; a.normalize_e = 0;
  a.use_start = use_index ? d_ustart.p : nullptr; a.use_index = use_index ? d_uidx.p : nullptr; a.mask = nullptr;
  a.n_inliers = nullptr; a.n_inliers_stride = 0; a.min_inliers = 0.0; a.method = opt->method; a.ratio = opt->positive_depth_ratio;
  a.results = d_res.p; a.out_selected = d_sel.p; a.out_X = d_X.p;
  MVGX_HIP(hipEventRecord(e0, stream));
  if ((rc = mvgx::relative_pose_launch(a, stream))) return rc;
  MVGX_HIP(hipEventRecord(e1, stream));
  MVGX_HIP(hipMemcpyAsync(h_res.data(), d_res.p, (size_t)n_pairs * sizeof(mvgx_relative_pose_result), hipMemcpyDeviceToHost, stream));
  if (n_list) {
    MVGX_HIP(hipMemcpyAsync(h_sel.data(), d_sel.p, n_list * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipMemcpyAsync(h_X.data(), d_X.p, 3 * n_list * sizeof(double), hipMemcpyDeviceToHost, stream));
  }
  MVGX_HIP(hipStreamSynchronize(stream));
  // the lists of the accepted pairs, one after the other
  uint64_t at = 0, n_ok = 0;
  for (uint32_t p = 0; p < n_pairs; ++p) {
    results[p] = h_res[p];
    const uint64_t from = use_index ? h_ustart[p] : h_start[p], k = h_res[p].n_selected;
    if (k) {
      memcpy(out_selected + at, h_sel.data() + from, k * sizeof(uint32_t));
      memcpy(out_X + 3 * at, h_X.data() + 3 * from, 3 * k * sizeof(double));
    }
    at += k; n_ok += h_res[p].ok;
    out_selected_start[p + 1] = at;
  }
  if (stats) {
    float kernel_ms = 0.f;
    (void)hipEventElapsedTime(&kernel_ms, e0, e1);
    stats->n_pairs = n_pairs; stats->n_pairs_ok = n_ok; stats->n_selected = at;
    stats->kernel_ms = kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(clock::now() - t_begin).count();
  }
  return MVGX_OK;
}

}  // extern "C"
