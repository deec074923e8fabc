// mvgx_triangulate.h — triangulation of the tracks of a scene on the device: kernels and host entry of mvgx_triangulate_tracks.
// Included at the end of mvgx_ba.hip (it shares ba_math.h and the unnamed namespace of the track filters there).
//
// What the reference does on the host, per track (paths under src/openMVG of the reference):
//   sfm/sfm_data_triangulation.cpp:45-101   track_triangulation: bearings cam(cam.get_ud_pixel(x)) (:67); more than two ->
//                                           TriangulateNViewAlgebraic, exactly two -> Triangulate2View(method)
//   sfm/sfm_data_triangulation.cpp:107-164  track_check_predicate, cheirality_predicate, ResidualAndCheiralityPredicate: the bearing
//                                           of every cheirality test is cam(x) of the RAW position (:142, :161, :400)
//   sfm/sfm_data_triangulation.cpp:166-222  SfM_Data_Structure_Computation_Blind::triangulate
//   sfm/sfm_data_triangulation.cpp:319-434  SfM_Data_Structure_Computation_Robust::robust_triangulation
//   multiview/triangulation_nview.cpp:39-61 TriangulateNViewAlgebraic (AtA = sum cost^T cost, cost = P - b b^T P)
//   multiview/triangulation.cpp:52-248      TriangulateDLT, L1 / Linfinity angular, inverse-depth-weighted midpoint, Triangulate2View
//   multiview/triangulation_method.hpp:15-22 ETriangulationMethod: 0 DLT, 1 L1 angular, 2 Linfinity angular, 3 IDW midpoint (DEFAULT)
//   cameras/Camera_Intrinsics.hpp:293-301   CheiralityTest: bearing . pose(X) > 0
//   robust_estimation/rand_sampling.hpp:36-58 UniformSample (draw, reject duplicates)
//
// Exact: the sample sequence (a fresh std::mt19937(default_seed) per track, :371, so the samples of a track depend on (min_sample_index, n)
// alone: a host-built table per (k, n), no generator on the device), the order of every sum over observations, every decision rule.
// To rounding: the points (the eigenvector of AtA comes from a cyclic Jacobi iteration instead of Eigen's tridiagonal QL; the DLT's null
// vector from a one-sided (Hestenes) Jacobi iteration on the columns of D instead of a two-sided JacobiSVD of D - never from D^T D, whose
// error grows with the SQUARED condition number of D; fused multiply-adds), R | t = the BA kernels' rotation terms instead of Pose3's
// matrix, pose(X) = R X + t instead of R (X - C).
#pragma once

#include <map>

#include "mvgx_buffers.h"

namespace {

constexpr int kTriRec = 29;      // doubles of one staged observation record: R | t (12), b_ud (3), b_raw (3), xy (2), intrinsic row (8), model
constexpr int kTriLdsObs = 64;   // longest track whose records a whole-wave group keeps in LDS; also the width of the inlier mask
constexpr int kTriSmallObs = 8;  // longest track of a 16-lane group (2 n <= 16 hypotheses)
constexpr int kTriJacobiSweeps = 12;

struct TriDev {
  const double* Rt;         // n_poses x 12: R row-major | t
  const double* intr;       // n_intrinsics x 8
  const int32_t* model;
  const uint64_t* track_start;
  const uint32_t* obs_pose;
  const uint32_t* obs_intr;
  const double* obs_xy;
  const uint8_t* obs_def;   // nullptr: every view is defined
  const double* bear;       // 6 x n_obs, structure of arrays: b_ud (3 rows), b_raw (3 rows)
  uint64_t n_obs;
  const uint32_t* tab;      // sample tables: for a track of n observations 2 n samples of k ascending observation positions
  const uint32_t* tab_off;  // per track: where its table starts
  double* X;
  uint8_t* ok;
  uint8_t* inl;
  double bound2;            // Square(max_reprojection_error)
  uint32_t min_inl, k;
  int method;
};

__device__ __forceinline__ void tri_cross(const double a[3], const double b[3], double c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double tri_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void tri_normalized(const double a[3], double n[3]) {   // Eigen's normalized(): a / sqrt(squaredNorm), a itself at 0
  const double s = tri_dot(a, a);
  const double len = s > 0.0 ? sqrt(s) : 1.0;
  n[0] = a[0] / len; n[1] = a[1] / len; n[2] = a[2] / len;
}
// pose(X) as R X + t
__device__ __forceinline__ void tri_to_camera(const double* Rt, const double X[3], double p[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = Rt[3 * i] * X[0] + Rt[3 * i + 1] * X[1] + Rt[3 * i + 2] * X[2] + Rt[9 + i];
}
// R^T (x - t): camera frame to world
__device__ __forceinline__ void tri_to_world(const double* Rt, const double x[3], double X[3]) {
  const double d[3] = {x[0] - Rt[9], x[1] - Rt[10], x[2] - Rt[11]};
#pragma unroll
  for (int j = 0; j < 3; ++j) X[j] = Rt[j] * d[0] + Rt[3 + j] * d[1] + Rt[6 + j] * d[2];
}

// ---- the 4 x 4 symmetric eigenproblem: cyclic Jacobi with a fixed bound on the sweeps, every entry a named scalar ----
// a: upper triangle {00, 01, 02, 03, 11, 12, 13, 22, 23, 33}; v: eigenvectors in columns, row-major.
__device__ __forceinline__ void tri_jacobi_rot(double& app, double& aqq, double& apq, double& apr, double& aqr, double& aps, double& aqs,
                                               double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q, double& v3p, double& v3q) {
  const double g = 100.0 * fabs(apq);
  if (fabs(app) + g == fabs(app) && fabs(aqq) + g == fabs(aqq)) { apq = 0.0; return; }   // nothing left to rotate away at this precision
  const double th = (aqq - app) / (2.0 * apq);
  const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));   // th^2 = inf -> t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq; aqq += t * apq; apq = 0.0;
  double x, y;
  x = apr; y = aqr; apr = c * x - s * y; aqr = s * x + c * y;
  x = aps; y = aqs; aps = c * x - s * y; aqs = s * x + c * y;
  x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
  x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
  x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
  x = v3p; y = v3q; v3p = c * x - s * y; v3q = s * x + c * y;
}
// hnormalized eigenvector of the smallest eigenvalue (SelfAdjointEigenSolver::eigenvectors().col(0), then Vec4::hnormalized)
__device__ __forceinline__ void tri_smallest_eigenvector(const double a[10], double X[3]) {
  double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0, v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
  double a00 = a[0], a01 = a[1], a02 = a[2], a03 = a[3], a11 = a[4], a12 = a[5], a13 = a[6], a22 = a[7], a23 = a[8], a33 = a[9];
#pragma unroll 1
  for (int sweep = 0; sweep < kTriJacobiSweeps; ++sweep) {
    if (a01 == 0.0 && a02 == 0.0 && a03 == 0.0 && a12 == 0.0 && a13 == 0.0 && a23 == 0.0) break;
    tri_jacobi_rot(a00, a11, a01, a02, a12, a03, a13, v00, v01, v10, v11, v20, v21, v30, v31);   // (0, 1)
    tri_jacobi_rot(a00, a22, a02, a01, a12, a03, a23, v00, v02, v10, v12, v20, v22, v30, v32);   // (0, 2)
    tri_jacobi_rot(a00, a33, a03, a01, a13, a02, a23, v00, v03, v10, v13, v20, v23, v30, v33);   // (0, 3)
    tri_jacobi_rot(a11, a22, a12, a01, a02, a13, a23, v01, v02, v11, v12, v21, v22, v31, v32);   // (1, 2)
    tri_jacobi_rot(a11, a33, a13, a01, a03, a12, a23, v01, v03, v11, v13, v21, v23, v31, v33);   // (1, 3)
    tri_jacobi_rot(a22, a33, a23, a02, a03, a12, a13, v02, v03, v12, v13, v22, v23, v32, v33);   // (2, 3)
  }
  // the column of the smallest diagonal entry (the first among equals), picked pairwise: a chain of four `if (a_cc < e)` was compiled
  // into a 16-entry table in scratch and an indexed load
  const bool lo1 = a11 < a00, hi1 = a33 < a22;
  const double elo = lo1 ? a11 : a00, ehi = hi1 ? a33 : a22;
  const double l0 = lo1 ? v01 : v00, l1 = lo1 ? v11 : v10, l2 = lo1 ? v21 : v20, l3 = lo1 ? v31 : v30;
  const double h0 = hi1 ? v03 : v02, h1 = hi1 ? v13 : v12, h2 = hi1 ? v23 : v22, h3 = hi1 ? v33 : v32;
  const bool hi = ehi < elo;
  const double x3 = hi ? h3 : l3;
  X[0] = (hi ? h0 : l0) / x3; X[1] = (hi ? h1 : l1) / x3; X[2] = (hi ? h2 : l2) / x3;
}
// a += r^T r for one row r of a matrix with four columns (every index a constant: the entries stay in registers)
__device__ __forceinline__ void tri_add_row(double r0, double r1, double r2, double r3, double a[10]) {
  a[0] += r0 * r0; a[1] += r0 * r1; a[2] += r0 * r2; a[3] += r0 * r3;
  a[4] += r1 * r1; a[5] += r1 * r2; a[6] += r1 * r3;
  a[7] += r2 * r2; a[8] += r2 * r3;
  a[9] += r3 * r3;
}
// one view of TriangulateNViewAlgebraic (triangulation_nview.cpp:49-56): AtA += cost^T cost, cost = P - b b^T P, b = bearing.normalized()
__device__ __forceinline__ void tri_nview_add(const double* Rt, const double bearing[3], double a[10]) {
  double b[3];
  tri_normalized(bearing, b);
  // w = b^T P, one row of cost at a time
  const double w0 = b[0] * Rt[0] + b[1] * Rt[3] + b[2] * Rt[6], w1 = b[0] * Rt[1] + b[1] * Rt[4] + b[2] * Rt[7];
  const double w2 = b[0] * Rt[2] + b[1] * Rt[5] + b[2] * Rt[8], w3 = b[0] * Rt[9] + b[1] * Rt[10] + b[2] * Rt[11];
#pragma unroll
  for (int i = 0; i < 3; ++i) tri_add_row(Rt[3 * i] - b[i] * w0, Rt[3 * i + 1] - b[i] * w1, Rt[3 * i + 2] - b[i] * w2, Rt[9 + i] - b[i] * w3, a);
}

// Compute3DPoint (triangulation.cpp:95-114)
__device__ __forceinline__ bool tri_point_from_rays(const double m0[3], const double m1[3], const double t[3], const double* Rt1, double X[3]) {
  double z[3], c0[3], c1[3];
  tri_cross(m1, m0, z);
  const double z2 = tri_dot(z, z);
  tri_cross(t, m1, c0);
  tri_cross(t, m0, c1);
  const double l0 = tri_dot(z, c0) / z2, l1 = tri_dot(z, c1) / z2;
  const double xp[3] = {t[0] + l0 * m0[0], t[1] + l0 * m0[1], t[2] + l0 * m0[2]};
  tri_to_world(Rt1, xp, X);
  return l0 > 0.0 && l1 > 0.0;
}
// TriangulateDLT (triangulation.cpp:16-70): the point is the right singular vector of the smallest singular value of the 4 x 4 design
// matrix D, rows x[0] P.row(2) - x[2] P.row(0) and x[1] P.row(2) - x[2] P.row(1) per view (:29-32). One-sided (Hestenes) Jacobi: plane
// rotations from the right make the columns of D orthogonal, V collects them, D V = U S; the column of the smallest norm names the null
// vector. Its error grows with the condition number of D (as that of the reference's JacobiSVD), not with its square (as that of an
// eigenvector of D^T D: three orders worse at half a degree of parallax). Every entry a named scalar, as in tri_smallest_eigenvector.
__device__ __forceinline__ void tri_dlt_row(const double* Rt, double xa, double xc, int r, double& d0, double& d1, double& d2, double& d3) {
  d0 = xa * Rt[6] - xc * Rt[3 * r]; d1 = xa * Rt[7] - xc * Rt[3 * r + 1]; d2 = xa * Rt[8] - xc * Rt[3 * r + 2]; d3 = xa * Rt[11] - xc * Rt[9 + r];
}
// columns p and q of D (four rows each) and of V; returns whether it rotated
__device__ __forceinline__ bool tri_hestenes_rot(double& d0p, double& d0q, double& d1p, double& d1q, double& d2p, double& d2q, double& d3p, double& d3q,
                                                 double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q, double& v3p, double& v3q) {
  const double app = d0p * d0p + d1p * d1p + d2p * d2p + d3p * d3p, aqq = d0q * d0q + d1q * d1q + d2q * d2q + d3q * d3q;
  const double apq = d0p * d0q + d1p * d1q + d2p * d2q + d3p * d3q;
  if (fabs(apq) <= 2.220446049250313e-16 * sqrt(app * aqq)) return false;   // orthogonal at this precision (a zero column included)
  const double th = (aqq - app) / (2.0 * apq);
  const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));   // th^2 = inf -> t = 0
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  double x, y;
  x = d0p; y = d0q; d0p = c * x - s * y; d0q = s * x + c * y;
  x = d1p; y = d1q; d1p = c * x - s * y; d1q = s * x + c * y;
  x = d2p; y = d2q; d2p = c * x - s * y; d2q = s * x + c * y;
  x = d3p; y = d3q; d3p = c * x - s * y; d3q = s * x + c * y;
  x = v0p; y = v0q; v0p = c * x - s * y; v0q = s * x + c * y;
  x = v1p; y = v1q; v1p = c * x - s * y; v1q = s * x + c * y;
  x = v2p; y = v2q; v2p = c * x - s * y; v2q = s * x + c * y;
  x = v3p; y = v3q; v3p = c * x - s * y; v3q = s * x + c * y;
  return true;
}
__device__ __forceinline__ void tri_dlt_point(const double* Rt0, const double x0[3], const double* Rt1, const double x1[3], double X[3]) {
  double d00, d01, d02, d03, d10, d11, d12, d13, d20, d21, d22, d23, d30, d31, d32, d33;   // d_rc: row r, column c
  tri_dlt_row(Rt0, x0[0], x0[2], 0, d00, d01, d02, d03);
  tri_dlt_row(Rt0, x0[1], x0[2], 1, d10, d11, d12, d13);
  tri_dlt_row(Rt1, x1[0], x1[2], 0, d20, d21, d22, d23);
  tri_dlt_row(Rt1, x1[1], x1[2], 1, d30, d31, d32, d33);
  double v00 = 1, v01 = 0, v02 = 0, v03 = 0, v10 = 0, v11 = 1, v12 = 0, v13 = 0, v20 = 0, v21 = 0, v22 = 1, v23 = 0, v30 = 0, v31 = 0, v32 = 0, v33 = 1;
#pragma unroll 1
  for (int sweep = 0; sweep < kTriJacobiSweeps; ++sweep) {
    bool any = tri_hestenes_rot(d00, d01, d10, d11, d20, d21, d30, d31, v00, v01, v10, v11, v20, v21, v30, v31);   // (0, 1)
    any = tri_hestenes_rot(d00, d02, d10, d12, d20, d22, d30, d32, v00, v02, v10, v12, v20, v22, v30, v32) || any;  // (0, 2)
    any = tri_hestenes_rot(d00, d03, d10, d13, d20, d23, d30, d33, v00, v03, v10, v13, v20, v23, v30, v33) || any;  // (0, 3)
    any = tri_hestenes_rot(d01, d02, d11, d12, d21, d22, d31, d32, v01, v02, v11, v12, v21, v22, v31, v32) || any;  // (1, 2)
    any = tri_hestenes_rot(d01, d03, d11, d13, d21, d23, d31, d33, v01, v03, v11, v13, v21, v23, v31, v33) || any;  // (1, 3)
    any = tri_hestenes_rot(d02, d03, d12, d13, d22, d23, d32, d33, v02, v03, v12, v13, v22, v23, v32, v33) || any;  // (2, 3)
    if (!any) break;
  }
  // the column of the smallest norm (the first among equals), picked pairwise as in tri_smallest_eigenvector
  const double n0 = d00 * d00 + d10 * d10 + d20 * d20 + d30 * d30, n1 = d01 * d01 + d11 * d11 + d21 * d21 + d31 * d31;
  const double n2 = d02 * d02 + d12 * d12 + d22 * d22 + d32 * d32, n3 = d03 * d03 + d13 * d13 + d23 * d23 + d33 * d33;
  const bool lo1 = n1 < n0, hi1 = n3 < n2;
  const double elo = lo1 ? n1 : n0, ehi = hi1 ? n3 : n2;
  const double l0 = lo1 ? v01 : v00, l1 = lo1 ? v11 : v10, l2 = lo1 ? v21 : v20, l3 = lo1 ? v31 : v30;
  const double h0 = hi1 ? v03 : v02, h1 = hi1 ? v13 : v12, h2 = hi1 ? v23 : v22, h3 = hi1 ? v33 : v32;
  const bool hi = ehi < elo;
  const double x3 = hi ? h3 : l3;
  X[0] = (hi ? h0 : l0) / x3; X[1] = (hi ? h1 : l1) / x3; X[2] = (hi ? h2 : l2) / x3;
}
// D^T D += the two rows of one view (the form the DLT had before the one-sided iteration; see tri_robust_kernel for why it is still here)
__device__ __forceinline__ void tri_dtd_add(const double* Rt, const double x[3], double a[10]) {
  tri_add_row(x[0] * Rt[6] - x[2] * Rt[0], x[0] * Rt[7] - x[2] * Rt[1], x[0] * Rt[8] - x[2] * Rt[2], x[0] * Rt[11] - x[2] * Rt[9], a);
  tri_add_row(x[1] * Rt[6] - x[2] * Rt[3], x[1] * Rt[7] - x[2] * Rt[4], x[1] * Rt[8] - x[2] * Rt[5], x[1] * Rt[11] - x[2] * Rt[10], a);
}
// ... and its verdict (:69): positive depth in both views
__device__ __forceinline__ bool tri_dlt_in_front(const double* Rt0, const double* Rt1, const double X[3]) {
  double p0[3], p1[3];
  tri_to_camera(Rt0, X, p0);
  tri_to_camera(Rt1, X, p1);
  return p0[2] > 0.0 && p1[2] > 0.0;
}
// The three closed forms of Triangulate2View (triangulation.cpp:218-248; method 1, 2 or 3) on two views' R | t and bearings
__device__ __forceinline__ bool tri_two_view_closed(int method, const double* Rt0, const double x0[3], const double* Rt1, const double x1[3], double X[3]) {
  // AbsoluteToRelative (:75-89): R = R1 R0^T, t = t1 - R t0, Rx0 = R x0
  double R[9], t[3], Rx0[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[3 * i + j] = Rt1[3 * i] * Rt0[3 * j] + Rt1[3 * i + 1] * Rt0[3 * j + 1] + Rt1[3 * i + 2] * Rt0[3 * j + 2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t[i] = Rt1[9 + i] - (R[3 * i] * Rt0[9] + R[3 * i + 1] * Rt0[10] + R[3 * i + 2] * Rt0[11]);
    Rx0[i] = R[3 * i] * x0[0] + R[3 * i + 1] * x0[1] + R[3 * i + 2] * x0[2];
  }
  if (method == 1) {   // TriangulateL1Angular (:116-147)
    double rn[3], xn[3], ca[3], cb[3];
    tri_normalized(Rx0, rn);
    tri_normalized(x1, xn);
    tri_cross(rn, t, ca);
    tri_cross(xn, t, cb);
    if (tri_dot(ca, ca) <= tri_dot(cb, cb)) {
      double c[3], n1[3];
      tri_cross(x1, t, c);
      tri_normalized(c, n1);
      const double s = tri_dot(Rx0, n1);
      const double m0[3] = {Rx0[0] - s * n1[0], Rx0[1] - s * n1[1], Rx0[2] - s * n1[2]};
      return tri_point_from_rays(m0, x1, t, Rt1, X);
    }
    double c[3], n0[3];
    tri_cross(Rx0, t, c);
    tri_normalized(c, n0);
    const double s = tri_dot(x1, n0);
    const double m1[3] = {x1[0] - s * n0[0], x1[1] - s * n0[1], x1[2] - s * n0[2]};
    return tri_point_from_rays(Rx0, m1, t, Rt1, X);
  }
  if (method == 2) {   // TriangulateLInfinityAngular (:149-177)
    double rn[3], xn[3], na[3], nb[3], np[3];
    tri_normalized(Rx0, rn);
    tri_normalized(x1, xn);
    const double sum[3] = {rn[0] + xn[0], rn[1] + xn[1], rn[2] + xn[2]}, dif[3] = {rn[0] - xn[0], rn[1] - xn[1], rn[2] - xn[2]};
    tri_cross(sum, t, na);
    tri_cross(dif, t, nb);
    if (tri_dot(na, na) >= tri_dot(nb, nb)) tri_normalized(na, np); else tri_normalized(nb, np);
    const double s0 = tri_dot(Rx0, np), s1 = tri_dot(x1, np);
    const double m0[3] = {Rx0[0] - s0 * np[0], Rx0[1] - s0 * np[1], Rx0[2] - s0 * np[2]};
    const double m1[3] = {x1[0] - s1 * np[0], x1[1] - s1 * np[1], x1[2] - s1 * np[2]};
    return tri_point_from_rays(m0, m1, t, Rt1, X);
  }
  // TriangulateIDWMidpoint (:179-216)
  double cp[3], cq[3], cr[3];
  tri_cross(Rx0, x1, cp);
  tri_cross(Rx0, t, cq);
  tri_cross(x1, t, cr);
  const double pn = sqrt(tri_dot(cp, cp)), qn = sqrt(tri_dot(cq, cq)), rn = sqrt(tri_dot(cr, cr));
  const double w = qn / (qn + rn), rp = rn / pn, qp = qn / pn;
  const double xp[3] = {w * (t[0] + rp * (Rx0[0] + x1[0])), w * (t[1] + rp * (Rx0[1] + x1[1])), w * (t[2] + rp * (Rx0[2] + x1[2]))};
  tri_to_world(Rt1, xp, X);
  double mm = 0.0, pp = 0.0, nn = 0.0, mp = 0.0;   // |t + l0 - l1|^2, |t + l0 + l1|^2, |t - l0 - l1|^2, |t - l0 + l1|^2
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double l0 = rp * Rx0[i], l1 = qp * x1[i];
    const double e0 = t[i] + l0 - l1, e1 = t[i] + l0 + l1, e2 = t[i] - l0 - l1, e3 = t[i] - l0 + l1;
    mm += e0 * e0; pp += e1 * e1; nn += e2 * e2; mp += e3 * e3;
  }
  const double m01 = pp < nn ? pp : nn;
  return mm < (m01 < mp ? m01 : mp);
}

// ---- where a track's observation records are read from: the group's LDS image (kLds) or the scene arrays ----
template <bool kLds>
__device__ __forceinline__ int tri_obs_model(const TriDev& d, const double* rec, uint64_t o, uint32_t j) {   // < 0: view without pose or intrinsic
  if constexpr (kLds) return (int)rec[j * kTriRec + 28];
  if (d.obs_def && !d.obs_def[o]) return -1;
  return d.model[d.obs_intr[o]];
}
template <bool kLds>
__device__ __forceinline__ const double* tri_obs_Rt(const TriDev& d, const double* rec, uint64_t o, uint32_t j) {
  if constexpr (kLds) return rec + j * kTriRec;
  return d.Rt + 12 * (size_t)d.obs_pose[o];
}
template <bool kLds>
__device__ __forceinline__ const double* tri_obs_intr(const TriDev& d, const double* rec, uint64_t o, uint32_t j) {
  if constexpr (kLds) return rec + j * kTriRec + 20;
  return d.intr + 8 * (size_t)d.obs_intr[o];
}
template <bool kLds>
__device__ __forceinline__ void tri_obs_bearing(const TriDev& d, const double* rec, uint64_t o, uint32_t j, int raw, double b[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if constexpr (kLds) b[c] = rec[j * kTriRec + 12 + 3 * raw + c];
    else b[c] = d.bear[(size_t)(3 * raw + c) * d.n_obs + o];
  }
}
template <bool kLds>
__device__ __forceinline__ void tri_obs_xy(const TriDev& d, const double* rec, uint64_t o, uint32_t j, double xy[2]) {
  if constexpr (kLds) { xy[0] = rec[j * kTriRec + 18]; xy[1] = rec[j * kTriRec + 19]; }
  else { xy[0] = d.obs_xy[2 * o]; xy[1] = d.obs_xy[2 * o + 1]; }
}

// One observation against a point, as the scoring loop of :393-412 and ResidualAndCheiralityPredicate (:152-163) see it.
// 0: not counted (view undefined, or the point fails CheiralityTest(cam(x), pose, X)); 1: residual^2 < bound; 2: not below the bound.
template <bool kLds>
__device__ __forceinline__ int tri_score(const TriDev& d, const double* rec, uint64_t o, uint32_t j, const double X[3], double& r2) {
  const int model = tri_obs_model<kLds>(d, rec, o, j);
  if (model < 0) return 0;
  double p[3], br[3], xy[2], r[2];
  tri_to_camera(tri_obs_Rt<kLds>(d, rec, o, j), X, p);
  tri_obs_bearing<kLds>(d, rec, o, j, 1, br);
  if (!(tri_dot(br, p) > 0.0)) return 0;
  tri_obs_xy<kLds>(d, rec, o, j, xy);
  project_residual(model, tri_obs_intr<kLds>(d, rec, o, j), p, xy, r);
  r2 = r[0] * r[0] + r[1] * r[1];
  return r2 < d.bound2 ? 1 : 2;
}

// ---- prepare pass ----
// R | t of every pose from its angle-axis row: the rotation terms of the BA kernels (transform_point)
__global__ __launch_bounds__(256) void tri_pose_kernel(const double* __restrict__ poses, uint32_t n_poses, double* __restrict__ Rt) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_poses) return;
  double pose[6], p[3], R[9], A[9];
#pragma unroll
  for (int k = 0; k < 6; ++k) pose[k] = poses[(size_t)i * 6 + k];
  const double zero[3] = {0.0, 0.0, 0.0};
  transform_point<true>(pose, zero, p, R, A);
#pragma unroll
  for (int k = 0; k < 9; ++k) Rt[(size_t)i * 12 + k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) Rt[(size_t)i * 12 + 9 + k] = pose[3 + k];
}
// b_ud = cam(get_ud_pixel(x)) and b_raw = cam(x) of every observation: the iterative undistortions run here, once
__global__ __launch_bounds__(256) void tri_bearing_kernel(TriDev d, double* __restrict__ bear) {
  const uint64_t o = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= d.n_obs) return;
  double bu[3] = {0.0, 0.0, 0.0}, br[3] = {0.0, 0.0, 0.0};
  if (!d.obs_def || d.obs_def[o]) {
    const uint32_t ii = d.obs_intr[o];
    double pin[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) pin[k] = d.intr[(size_t)ii * 8 + k];
    const double xy[2] = {d.obs_xy[2 * o], d.obs_xy[2 * o + 1]};
    camera_bearing(d.model[ii], pin, xy, true, bu);
    camera_bearing(d.model[ii], pin, xy, false, br);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) { bear[(size_t)c * d.n_obs + o] = bu[c]; bear[(size_t)(3 + c) * d.n_obs + o] = br[c]; }
}

// ---- one lane per track: track_triangulation on ALL observations, then track_check_predicate ----
// robust == 0: SfM_Data_Structure_Computation_Blind::triangulate (:193-206; the default method, cheirality of every observation).
// robust == 1: the all-observations case of robust_triangulation (:344-357; the caller's method, cheirality and residual).
// perm lists the tracks in order of length, so the lanes of a wave run similar trip counts.
// kDlt: the caller's method is the DLT (robust only): the form with the one-sided Jacobi, kept out of the code the other methods run.
template <bool kDlt>
__global__ __launch_bounds__(256) void tri_track_kernel(TriDev d, const uint32_t* __restrict__ perm, uint32_t count, int robust) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint32_t t = perm[i];
  const uint64_t o0 = d.track_start[t];
  const uint32_t n = (uint32_t)(d.track_start[t + 1] - o0);
  bool ok = n >= 2;
  for (uint32_t j = 0; j < n && ok; ++j) ok = tri_obs_model<false>(d, nullptr, o0 + j, j) >= 0;   // :63-64
  double X[3] = {0.0, 0.0, 0.0};
  if (ok) {
    const int method = robust ? d.method : 3;   // (kDlt: not read)
    if (n == 2) {
      double b0[3], b1[3];
      tri_obs_bearing<false>(d, nullptr, o0, 0, 0, b0);
      tri_obs_bearing<false>(d, nullptr, o0 + 1, 1, 0, b1);
      const double *Rt0 = tri_obs_Rt<false>(d, nullptr, o0, 0), *Rt1 = tri_obs_Rt<false>(d, nullptr, o0 + 1, 1);
      if constexpr (kDlt) {
        tri_dlt_point(Rt0, b0, Rt1, b1, X);
        ok = tri_dlt_in_front(Rt0, Rt1, X);
      } else {
        ok = tri_two_view_closed(method, Rt0, b0, Rt1, b1, X);
      }
    } else {
      double a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll 1
      for (uint32_t j = 0; j < n; ++j) {
        double b[3];
        tri_obs_bearing<false>(d, nullptr, o0 + j, j, 0, b);
        tri_nview_add(tri_obs_Rt<false>(d, nullptr, o0 + j, j), b, a);
      }
      tri_smallest_eigenvector(a, X);
    }
  }
#pragma unroll 1
  for (uint32_t j = 0; j < n && ok; ++j) {
    double r2;
    const int s = tri_score<false>(d, nullptr, o0 + j, j, X, r2);
    ok = robust ? s == 1 : s != 0;
  }
  d.ok[t] = ok ? 1 : 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) d.X[3 * (size_t)t + c] = ok ? X[c] : 0.0;
  for (uint32_t j = 0; j < n; ++j) d.inl[o0 + j] = ok ? 1 : 0;
}

// ---- the RANSAC of robust_triangulation (:362-433): one group of G lanes per track, one hypothesis per lane ----
// Lane l of the group takes the iterations l, l + G, ... of the reference's loop and keeps the best of them (strictly smaller error: the
// earliest wins among its own); a shuffle reduction then takes the smallest (error, iteration) over the group - the iteration the
// reference's `current_error < best_error` would have ended with. G = 16: four tracks of at most 8 observations per wave; G = 64: one.
// kLds: the track's records are staged in LDS once (tracks up to kTriLdsObs observations; above, every lane reads the scene arrays).
// Tracks up to 64 observations carry their inlier set as a mask; longer ones are scored once more with the winning point.
// kDlt: two-view samples by the DLT (min_sample_index == 2, method 0) - a form of its own, so that the one-sided Jacobi costs the forms of
// the other methods no register; a kernel holds ONE of the two iterations.
template <int G, bool kLds, bool kDlt>
__global__ __launch_bounds__(64) void tri_robust_kernel(TriDev d, const uint32_t* __restrict__ perm, uint32_t count) {
  constexpr int kGroups = 64 / G;
  constexpr int kCap = G == 16 ? kTriSmallObs : kTriLdsObs;
  __shared__ double lds_rec[kLds ? kGroups * kCap * kTriRec : 1];
  const int lane = threadIdx.x & 63, g = lane / G, lg = lane % G;
  const uint32_t slot = blockIdx.x * kGroups + g;
  const uint32_t t = slot < count ? perm[slot] : 0;
  const uint64_t o0 = slot < count ? d.track_start[t] : 0;
  uint32_t n = slot < count ? (uint32_t)(d.track_start[t + 1] - o0) : 0;
  if (kLds && n > (uint32_t)kCap) n = 0;   // (the host never sends such a track here)
  const double* rec = lds_rec + (kLds ? g * kCap * kTriRec : 0);
  if constexpr (kLds) {
    double* w = lds_rec + g * kCap * kTriRec;
    for (uint32_t e = lg; e < n * kTriRec; e += G) {
      const uint32_t j = e / kTriRec, f = e % kTriRec;
      const uint64_t o = o0 + j;
      const bool def = !d.obs_def || d.obs_def[o];
      double val = 0.0;
      if (f == 28) val = def ? (double)d.model[d.obs_intr[o]] : -1.0;
      else if (!def) val = 0.0;
      else if (f < 12) val = d.Rt[12 * (size_t)d.obs_pose[o] + f];
      else if (f < 18) val = d.bear[(size_t)(f - 12) * d.n_obs + o];
      else if (f < 20) val = d.obs_xy[2 * o + (f - 18)];
      else val = d.intr[8 * (size_t)d.obs_intr[o] + (f - 20)];
      w[e] = val;
    }
    __syncthreads();
  }
  const uint32_t k = d.k;
  const uint32_t* tab = d.tab + (slot < count ? d.tab_off[t] : 0);
  double best_err = INFINITY, bX[3] = {0.0, 0.0, 0.0};
  uint32_t best_h = 0xffffffffu;
  unsigned long long best_mask = 0;
  for (uint32_t h = lg; h < 2 * n; h += G) {
    const uint32_t s0 = tab[(size_t)h * k], s1 = tab[(size_t)h * k + 1], s2 = k == 3 ? tab[(size_t)h * k + 2] : s1;
    // track_triangulation of the sample (:383): every view defined, then two views or three
    if (tri_obs_model<kLds>(d, rec, o0 + s0, s0) < 0 || tri_obs_model<kLds>(d, rec, o0 + s1, s1) < 0 || tri_obs_model<kLds>(d, rec, o0 + s2, s2) < 0) continue;
    double X[3];
    {
      double b0[3], b1[3];
      tri_obs_bearing<kLds>(d, rec, o0 + s0, s0, 0, b0);
      tri_obs_bearing<kLds>(d, rec, o0 + s1, s1, 0, b1);
      const double *Rt0 = tri_obs_Rt<kLds>(d, rec, o0 + s0, s0), *Rt1 = tri_obs_Rt<kLds>(d, rec, o0 + s1, s1);
      if constexpr (kDlt) {
        tri_dlt_point(Rt0, b0, Rt1, b1, X);
        if (!tri_dlt_in_front(Rt0, Rt1, X)) continue;
      } else if (k == 2 && d.method != 0) {
        if (!tri_two_view_closed(d.method, Rt0, b0, Rt1, b1, X)) continue;
      } else {
        double a[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (k == 2) {   // (never taken: the host launches the kDlt form for two-view samples by the DLT. The branch is what this form had
                        // when it served the DLT too, through D^T D; with it the form compiles to the code it had - measured, not argued)
          tri_dtd_add(Rt0, b0, a);
          tri_dtd_add(Rt1, b1, a);
        } else {
          double b2[3];
          tri_obs_bearing<kLds>(d, rec, o0 + s2, s2, 0, b2);
          tri_nview_add(Rt0, b0, a);
          tri_nview_add(Rt1, b1, a);
          tri_nview_add(tri_obs_Rt<kLds>(d, rec, o0 + s2, s2), b2, a);
        }
        tri_smallest_eigenvector(a, X);
        if (k == 2 && !tri_dlt_in_front(Rt0, Rt1, X)) continue;
      }
    }
    // the sample's own predicate (:387)
    double r2;
    if (tri_score<kLds>(d, rec, o0 + s0, s0, X, r2) != 1 || tri_score<kLds>(d, rec, o0 + s1, s1, X, r2) != 1) continue;
    if (k == 3 && tri_score<kLds>(d, rec, o0 + s2, s2, X, r2) != 1) continue;
    // score over all observations in order (:393-412)
    double err = 0.0;
    uint32_t cnt = 0;
    unsigned long long mask = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < n; ++j) {
      const int s = tri_score<kLds>(d, rec, o0 + j, j, X, r2);
      if (s == 1) { err += r2; ++cnt; if (j < 64) mask |= 1ull << j; }
      else if (s == 2) err += d.bound2;
    }
    if (err < best_err && err < 1.7976931348623157e308 && cnt >= d.min_inl) {   // (:416-417; best_error starts at the largest double)
      best_err = err; best_h = h; best_mask = mask;
      bX[0] = X[0]; bX[1] = X[1]; bX[2] = X[2];
    }
  }
  // the smallest (error, iteration) of the group
  double win_err = best_err;
  uint32_t win_h = best_h;
#pragma unroll
  for (int off = G / 2; off >= 1; off >>= 1) {
    const double e = __shfl_xor(win_err, off);
    const uint32_t hh = (uint32_t)__shfl_xor((int)win_h, off);
    if (e < win_err || (e == win_err && hh < win_h)) { win_err = e; win_h = hh; }
  }
  const bool kept = win_h != 0xffffffffu;
  const int src = g * G + (kept ? (int)(win_h % G) : lg);   // the lane that owns the winning iteration
  const double X0 = __shfl(bX[0], src), X1 = __shfl(bX[1], src), X2 = __shfl(bX[2], src);
  const unsigned long long wmask = ((unsigned long long)(uint32_t)__shfl((int)(best_mask >> 32), src) << 32) | (uint32_t)__shfl((int)(uint32_t)best_mask, src);
  if (slot >= count) return;
  if (lg == 0) {
    d.ok[t] = kept ? 1 : 0;
    d.X[3 * (size_t)t] = kept ? X0 : 0.0; d.X[3 * (size_t)t + 1] = kept ? X1 : 0.0; d.X[3 * (size_t)t + 2] = kept ? X2 : 0.0;
  }
  const double Xw[3] = {X0, X1, X2};
  for (uint32_t j = lg; j < n; j += G) {
    uint8_t in = 0;
    if (kept) {
      if (n <= 64) in = (uint8_t)((wmask >> j) & 1ull);
      else { double r2; in = tri_score<kLds>(d, rec, o0 + j, j, Xw, r2) == 1 ? 1 : 0; }
    }
    d.inl[o0 + j] = in;
  }
}

// ---- host ----
// The sample sequence of a track: std::mt19937(default_seed), then per iteration UniformSample(k, n) = draws of
// std::uniform_int_distribution<uint32_t>(0, n - 1), duplicates rejected (rand_sampling.hpp:46-57), sorted because ObservationsSampler
// (:300-314) inserts into a map. The bounded draw is written out in the form of libstdc++ 11 (bits/uniform_int_dist.h, _S_nd; the form
// mvgx_geofilter.hip states for the device) - the standard does not fix the distribution's algorithm.
struct TriMt19937 {
  uint32_t mt[624];
  int idx = 624;
  TriMt19937() {
    mt[0] = 5489u;
    for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
  }
  uint32_t next() {
    if (idx >= 624) {
      for (int i = 0; i < 624; ++i) {
        const uint32_t y = (mt[i] & 0x80000000u) | (mt[(i + 1) % 624] & 0x7fffffffu);
        mt[i] = mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      idx = 0;
    }
    uint32_t y = mt[idx++];
    y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18;
    return y;
  }
  uint32_t below(uint32_t range) {   // uniform in [0, range)
    uint64_t product = (uint64_t)next() * range;
    uint32_t low = (uint32_t)product;
    if (low < range) {
      const uint32_t threshold = (0u - range) % range;
      while (low < threshold) { product = (uint64_t)next() * range; low = (uint32_t)product; }
    }
    return (uint32_t)(product >> 32);
  }
};

std::mutex g_tri_tables_mutex;
std::map<uint64_t, std::vector<uint32_t>> g_tri_tables;   // (k, n) -> 2 n samples of k ascending positions; entries are never removed

const std::vector<uint32_t>* tri_sample_table(uint32_t k, uint32_t n) {
  std::lock_guard<std::mutex> lock(g_tri_tables_mutex);
  std::vector<uint32_t>& tab = g_tri_tables[((uint64_t)k << 32) | n];
  if (tab.empty()) {
    tab.reserve((size_t)2 * n * k);
    TriMt19937 gen;
    for (uint32_t it = 0; it < 2 * n; ++it) {
      uint32_t s[3], m = 0;
      while (m < k) {
        const uint32_t v = gen.below(n);
        bool found = false;
        for (uint32_t q = 0; q < m; ++q) found = found || s[q] == v;
        if (!found) s[m++] = v;
      }
      std::sort(s, s + k);
      tab.insert(tab.end(), s, s + k);
    }
  }
  return &tab;
}

int tri_check_arguments(const double* poses, uint32_t n_poses, const double* intrinsics, const int32_t* intr_model, uint32_t n_intrinsics,
                        const uint64_t* track_start, uint32_t n_tracks, const uint32_t* obs_pose, const uint32_t* obs_intr, const double* obs_xy,
                        const uint8_t* obs_defined, const mvgx_triangulate_options* opt, double* X, uint8_t* track_ok, uint8_t* obs_inlier) {
  MVGX_REQUIRE(opt && track_start, MVGX_ERR_ARG, "mvgx_triangulate_tracks: NULL options or track_start");
  MVGX_REQUIRE(opt->mode == MVGX_TRI_BLIND || opt->mode == MVGX_TRI_ROBUST, MVGX_ERR_ARG, "mvgx_triangulate_tracks: mode %d", opt->mode);
  if (opt->mode == MVGX_TRI_ROBUST) {
    MVGX_REQUIRE(opt->method >= 0 && opt->method <= 3, MVGX_ERR_ARG, "mvgx_triangulate_tracks: method %d", opt->method);
    MVGX_REQUIRE(opt->min_sample_index == 2 || opt->min_sample_index == 3, MVGX_ERR_UNSUPPORTED,
                 "mvgx_triangulate_tracks: min_sample_index %u (2 and 3 are what the callers of the reference use)", opt->min_sample_index);
    MVGX_REQUIRE(opt->min_required_inliers >= 1, MVGX_ERR_UNSUPPORTED, "mvgx_triangulate_tracks: min_required_inliers 0");
  }
  for (uint32_t t = 0; t < n_tracks; ++t)
    MVGX_REQUIRE(track_start[t] <= track_start[t + 1] && track_start[t + 1] - track_start[t] < (1ull << 30), MVGX_ERR_ARG,
                 "mvgx_triangulate_tracks: track_start is not monotone at track %u", t);
  const uint64_t o_begin = track_start[0], o_end = track_start[n_tracks];
  MVGX_REQUIRE(!n_tracks || (X && track_ok), MVGX_ERR_ARG, "mvgx_triangulate_tracks: NULL output");
  MVGX_REQUIRE(o_begin == o_end || (obs_pose && obs_intr && obs_xy && obs_inlier && poses && intrinsics && intr_model), MVGX_ERR_ARG,
               "mvgx_triangulate_tracks: NULL array");
  for (uint32_t i = 0; i < n_intrinsics && intr_model; ++i)
    MVGX_REQUIRE(intr_param_count(intr_model[i]) >= 0, MVGX_ERR_UNSUPPORTED, "mvgx_triangulate_tracks: camera model %d of intrinsic %u", intr_model[i], i);
  for (uint64_t o = o_begin; o < o_end; ++o) {
    if (obs_defined && !obs_defined[o]) continue;
    MVGX_REQUIRE(obs_pose[o] < n_poses && obs_intr[o] < n_intrinsics, MVGX_ERR_ARG, "mvgx_triangulate_tracks: observation %llu names pose %u / intrinsic %u",
                 (unsigned long long)o, obs_pose[o], obs_intr[o]);
  }
  return MVGX_OK;
}

// the launches of one call, by class of track
struct TriPlan {
  std::vector<uint32_t> all;      // blind: every track of two or more observations, by length
  std::vector<uint32_t> whole;    // robust: the all-observations case
  std::vector<uint32_t> small, wave, global;   // robust loop: n <= kTriSmallObs | <= kTriLdsObs | above
  std::vector<uint32_t> tab_off;  // per track
  std::vector<uint32_t> tables;
  uint64_t n_hypotheses = 0;
};

int tri_plan(const uint64_t* track_start, uint32_t n_tracks, const mvgx_triangulate_options* opt, TriPlan& pl) {
  if (opt->mode == MVGX_TRI_BLIND) {
    for (uint32_t t = 0; t < n_tracks; ++t)
      if (track_start[t + 1] - track_start[t] >= 2) pl.all.push_back(t);
    std::stable_sort(pl.all.begin(), pl.all.end(), [&](uint32_t a, uint32_t b) { return track_start[a + 1] - track_start[a] < track_start[b + 1] - track_start[b]; });
    return MVGX_OK;
  }
  const uint32_t k = opt->min_sample_index, need = opt->min_required_inliers;
  pl.tab_off.assign(n_tracks, 0);
  std::map<uint32_t, uint32_t> off_of_n;
  for (uint32_t t = 0; t < n_tracks; ++t) {
    const uint32_t n = (uint32_t)(track_start[t + 1] - track_start[t]);
    if (n < need || n < k) continue;                                  // :327-330
    if (need == k && n == need) { pl.whole.push_back(t); continue; }  // :344-357
    auto it = off_of_n.find(n);
    if (it == off_of_n.end()) {
      const std::vector<uint32_t>* tab = tri_sample_table(k, n);
      MVGX_REQUIRE(pl.tables.size() + tab->size() < (1ull << 32), MVGX_ERR_UNSUPPORTED, "mvgx_triangulate_tracks: sample tables beyond 2^32 entries");
      it = off_of_n.emplace(n, (uint32_t)pl.tables.size()).first;
      pl.tables.insert(pl.tables.end(), tab->begin(), tab->end());
    }
    pl.tab_off[t] = it->second;
    pl.n_hypotheses += 2ull * n;
    (n <= (uint32_t)kTriSmallObs ? pl.small : n <= (uint32_t)kTriLdsObs ? pl.wave : pl.global).push_back(t);
  }
  return MVGX_OK;
}

template <typename T>
int tri_upload(mvgx::DevBuf<T>& dst, const T* src, size_t n, hipStream_t stream) {
  const int rc = dst.ensure(std::max<size_t>(n, 1));
  if (rc) return rc;
  if (n) MVGX_HIP(hipMemcpyAsync(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
  return MVGX_OK;
}

}  // namespace

extern "C" {

void mvgx_triangulate_default_options(mvgx_triangulate_options* o) {
  if (!o) return;
  // SfM_Data_Structure_Computation_Robust's constructor defaults (sfm/sfm_data_triangulation.hpp): 4.0, 3, 3, ETriangulationMethod::DEFAULT
  o->mode = MVGX_TRI_ROBUST; o->method = 3; o->max_reprojection_error = 4.0; o->min_required_inliers = 3; o->min_sample_index = 3;
}

int mvgx_triangulate_tracks(int device, const double* poses, uint32_t n_poses, const double* intrinsics, const int32_t* intr_model, uint32_t n_intrinsics,
                            const uint64_t* track_start, uint32_t n_tracks, const uint32_t* obs_pose, const uint32_t* obs_intr, const double* obs_xy,
                            const uint8_t* obs_defined, const mvgx_triangulate_options* opt, double* X, uint8_t* track_ok, uint8_t* obs_inlier,
                            mvgx_triangulate_stats* stats) {
  using clock = std::chrono::steady_clock;
  const auto t_begin = clock::now();
  int rc;
  if ((rc = tri_check_arguments(poses, n_poses, intrinsics, intr_model, n_intrinsics, track_start, n_tracks, obs_pose, obs_intr, obs_xy, obs_defined, opt,
                                X, track_ok, obs_inlier)))
    return rc;
  if (stats) memset(stats, 0, sizeof(*stats));
  if (!n_tracks) return MVGX_OK;
  // observations are addressed from track_start[0]: the arrays are taken from there
  const uint64_t o_base = track_start[0], n_obs = track_start[n_tracks] - o_base;
  TriPlan pl;
  if ((rc = tri_plan(track_start, n_tracks, opt, pl))) return rc;
  if ((rc = mvgx::select_device(device < 0 ? -1 : device))) return rc;

  // one page-locked staging buffer for what the host built: track offsets from zero | launch lists | table offsets | tables
  const size_t n_lists = pl.all.size() + pl.whole.size() + pl.small.size() + pl.wave.size() + pl.global.size();
  mvgx::PinnedBuf<uint64_t> stage;
  const size_t stage_u32 = n_lists + pl.tab_off.size() + pl.tables.size();
  if ((rc = stage.ensure((size_t)n_tracks + 1 + (stage_u32 + 1) / 2))) return rc;
  for (uint32_t t = 0; t <= n_tracks; ++t) stage.p[t] = track_start[t] - o_base;
  uint32_t* s32 = reinterpret_cast<uint32_t*>(stage.p + n_tracks + 1);
  size_t at = 0;
  const auto put = [&](const std::vector<uint32_t>& v) { const size_t o = at; if (!v.empty()) memcpy(s32 + at, v.data(), v.size() * sizeof(uint32_t)); at += v.size(); return o; };
  const size_t at_all = put(pl.all), at_whole = put(pl.whole), at_small = put(pl.small), at_wave = put(pl.wave), at_global = put(pl.global);
  const size_t at_off = put(pl.tab_off), at_tab = put(pl.tables);

  mvgx::DevBuf<double> d_poses, d_intr, d_xy, d_Rt, d_bear, d_X;   // (before the stream guard: drained first, freed after)
  mvgx::DevBuf<int32_t> d_model;
  mvgx::DevBuf<uint64_t> d_start;
  mvgx::DevBuf<uint32_t> d_opose, d_ointr, d_u32;
  mvgx::DevBuf<uint8_t> d_def, d_ok, d_inl;
  hipStream_t stream = nullptr;
  if ((rc = mvgx::acquire_stream(&stream))) return rc;
  int stream_device = 0;
  MVGX_HIP(hipGetDevice(&stream_device));
  mvgx::StreamGuard sg{stream_device, stream};
  hipEvent_t e0 = nullptr, e1 = nullptr;
  MVGX_HIP(hipEventCreate(&e0));
  MVGX_HIP(hipEventCreate(&e1));
  mvgx::EventGuard eg{e0, e1};

  if ((rc = tri_upload(d_poses, poses, (size_t)n_poses * 6, stream)) || (rc = tri_upload(d_intr, intrinsics, (size_t)n_intrinsics * 8, stream)) ||
      (rc = tri_upload(d_model, intr_model, n_intrinsics, stream)) || (rc = tri_upload(d_start, stage.p, (size_t)n_tracks + 1, stream)) ||
      (rc = tri_upload(d_u32, s32, stage_u32, stream)) || (rc = tri_upload(d_opose, n_obs ? obs_pose + o_base : nullptr, n_obs, stream)) ||
      (rc = tri_upload(d_ointr, n_obs ? obs_intr + o_base : nullptr, n_obs, stream)) || (rc = tri_upload(d_xy, n_obs ? obs_xy + 2 * o_base : nullptr, 2 * n_obs, stream)) ||
      (rc = tri_upload(d_def, obs_defined && n_obs ? obs_defined + o_base : nullptr, obs_defined ? n_obs : 0, stream)))
    return rc;
  if ((rc = d_Rt.ensure(std::max<size_t>((size_t)n_poses * 12, 1))) || (rc = d_bear.ensure(std::max<size_t>(6 * n_obs, 1))) ||
      (rc = d_X.ensure((size_t)n_tracks * 3)) || (rc = d_ok.ensure(n_tracks)) || (rc = d_inl.ensure(std::max<size_t>(n_obs, 1))))
    return rc;
  // rejected tracks, and tracks no kernel visits: zeros
  MVGX_HIP(hipMemsetAsync(d_X.p, 0, (size_t)n_tracks * 3 * sizeof(double), stream));
  MVGX_HIP(hipMemsetAsync(d_ok.p, 0, n_tracks, stream));
  if (n_obs) MVGX_HIP(hipMemsetAsync(d_inl.p, 0, n_obs, stream));

  TriDev d;
  d.Rt = d_Rt.p; d.intr = d_intr.p; d.model = d_model.p; d.track_start = d_start.p; d.obs_pose = d_opose.p; d.obs_intr = d_ointr.p; d.obs_xy = d_xy.p;
  d.obs_def = obs_defined ? d_def.p : nullptr; d.bear = d_bear.p; d.n_obs = n_obs; d.tab = d_u32.p + at_tab; d.tab_off = d_u32.p + at_off;
  d.X = d_X.p; d.ok = d_ok.p; d.inl = d_inl.p;
  d.bound2 = opt->max_reprojection_error * opt->max_reprojection_error;
  d.min_inl = opt->min_required_inliers; d.k = opt->min_sample_index; d.method = opt->method;

  MVGX_HIP(hipEventRecord(e0, stream));
  // (launch arguments are plain pointers and counts: the test-suite's emulation captures them by value)
  const double* const p_poses = d_poses.p;
  double* const p_Rt = d_Rt.p;
  double* const p_bear = d_bear.p;
  const uint32_t* const lists = d_u32.p;
  if (n_poses && n_obs) {
    hipLaunchKernelGGL(tri_pose_kernel, dim3((n_poses + 255) / 256), dim3(256), 0, stream, p_poses, n_poses, p_Rt);
    BA_LAUNCH_CHECK();
  }
  if (n_obs) {
    hipLaunchKernelGGL(tri_bearing_kernel, dim3((unsigned)((n_obs + 255) / 256)), dim3(256), 0, stream, d, p_bear);
    BA_LAUNCH_CHECK();
  }
  const auto blocks = [](uint32_t count, uint32_t per_block) { return dim3((count + per_block - 1) / per_block); };
  const uint32_t n_all = (uint32_t)pl.all.size(), n_whole = (uint32_t)pl.whole.size(), n_small = (uint32_t)pl.small.size();
  const uint32_t n_wave = (uint32_t)pl.wave.size(), n_global = (uint32_t)pl.global.size();
  // the DLT forms: only where a two-view solve by the caller's method 0 can happen (the robust lists are empty in blind mode)
  const bool dlt_whole = opt->method == 0, dlt_samples = opt->method == 0 && opt->min_sample_index == 2;
  if (n_all) {
    hipLaunchKernelGGL(tri_track_kernel<false>, blocks(n_all, 256), dim3(256), 0, stream, d, lists + at_all, n_all, 0);
    BA_LAUNCH_CHECK();
  }
  if (n_whole) {
    if (dlt_whole) hipLaunchKernelGGL(tri_track_kernel<true>, blocks(n_whole, 256), dim3(256), 0, stream, d, lists + at_whole, n_whole, 1);
    else hipLaunchKernelGGL(tri_track_kernel<false>, blocks(n_whole, 256), dim3(256), 0, stream, d, lists + at_whole, n_whole, 1);
    BA_LAUNCH_CHECK();
  }
  if (n_small) {
    if (dlt_samples) hipLaunchKernelGGL((tri_robust_kernel<16, true, true>), blocks(n_small, 4), dim3(64), 0, stream, d, lists + at_small, n_small);
    else hipLaunchKernelGGL((tri_robust_kernel<16, true, false>), blocks(n_small, 4), dim3(64), 0, stream, d, lists + at_small, n_small);
    BA_LAUNCH_CHECK();
  }
  if (n_wave) {
    if (dlt_samples) hipLaunchKernelGGL((tri_robust_kernel<64, true, true>), blocks(n_wave, 1), dim3(64), 0, stream, d, lists + at_wave, n_wave);
    else hipLaunchKernelGGL((tri_robust_kernel<64, true, false>), blocks(n_wave, 1), dim3(64), 0, stream, d, lists + at_wave, n_wave);
    BA_LAUNCH_CHECK();
  }
  if (n_global) {
    if (dlt_samples) hipLaunchKernelGGL((tri_robust_kernel<64, false, true>), blocks(n_global, 1), dim3(64), 0, stream, d, lists + at_global, n_global);
    else hipLaunchKernelGGL((tri_robust_kernel<64, false, false>), blocks(n_global, 1), dim3(64), 0, stream, d, lists + at_global, n_global);
    BA_LAUNCH_CHECK();
  }
  MVGX_HIP(hipEventRecord(e1, stream));
  MVGX_HIP(hipMemcpyAsync(X, d_X.p, (size_t)n_tracks * 3 * sizeof(double), hipMemcpyDeviceToHost, stream));
  MVGX_HIP(hipMemcpyAsync(track_ok, d_ok.p, n_tracks, hipMemcpyDeviceToHost, stream));
  if (n_obs) MVGX_HIP(hipMemcpyAsync(obs_inlier + o_base, d_inl.p, n_obs, hipMemcpyDeviceToHost, stream));
  MVGX_HIP(hipStreamSynchronize(stream));
  if (stats) {
    float kernel_ms = 0.f;
    (void)hipEventElapsedTime(&kernel_ms, e0, e1);
    stats->n_tracks = n_tracks; stats->n_hypotheses = pl.n_hypotheses;
    for (uint32_t t = 0; t < n_tracks; ++t) stats->n_kept += track_ok[t];
    for (uint64_t o = 0; o < n_obs; ++o) stats->n_inlier_obs += obs_inlier[o_base + o];
    stats->kernel_ms = kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(clock::now() - t_begin).count();
  }
  return MVGX_OK;
}

}  // extern "C"
