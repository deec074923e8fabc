// mvgx_resection.h - robust camera resection on the device: AC-RANSAC over a P3P solver, a batch of independent problems per call, in
// the reference's two forms: the exhaustive NFA of an unbounded precision (mvgx_resection_localize) and the quantified NFA with the
// max-consensus warm-up of a bounded one (mvgx_resection_localize_bounded). Included at the end of mvgx_geofilter.hip, after
// mvgx_resection_loop.h and under that header's `#pragma clang fp contract(off)`: the a-contrario loop, its storage, its sampling and
// the exhaustive kernel are that header's. Here: the two P3P solvers, the form they give the exhaustive loop (ResP3PForm), the bounded
// loop, and the host side of all three entries (ResCall and the res_* stages; mvgx_resection_dlt.h calls them with its own record).
// What is restated here (paths under src/openMVG of the reference; the loop's own list is in mvgx_resection_loop.h):
//   sfm/pipelines/localization/SfM_Localizer.cpp:31-343          ACKernelAdaptorResection_Intrinsics, SfM_Localizer::Localize
//   robust_estimation/robust_estimator_ACRansac.hpp:205-256      the quantified NFA of one model (third_party/histogram/histogram.hpp)
//   robust_estimation/robust_estimator_ACRansac.hpp:326-489      the bounded loop's warm-up and early exit
//   robust_estimation/rand_sampling.hpp:36-58                    UniformSample(3, nData, ...) of the warm-up (rejection)
//   multiview/solver_resection_p3p_ding.cpp:33-325               P3PSolver_Ding
//   multiview/solver_resection_p3p_nordberg.cpp:31-454           P3PSolver_Nordberg
//   multiview/projection.cpp:40-132                              KRt_From_P (host)
#pragma once

namespace {

constexpr uint32_t kResLdsMaxN = 1024;        // largest n whose sort slices and tables live in LDS (DESIGN.md derives it)
constexpr int kResSolverNordberg = 3, kResSolverDing = 4;   // resection::SolverType (multiview/solver_resection.hpp:15-24)

struct ResProblem {       // per problem, prepared on the host (glibc's log10: the reference's value)
  uint64_t start;         // first correspondence, counted from the first problem's
  uint64_t scratch;       // global form: byte offset of the problem's scratch
  uint32_t n, model;
  double intr[8];
  double n1, loge0;       // imagePlane_toCameraPlaneError(1), log10(MAX_MODELS (n - 3))
};

struct ResV3 { double x, y, z; };
__device__ __forceinline__ ResV3 res_sub(ResV3 a, ResV3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ ResV3 res_neg(ResV3 a) { return {-a.x, -a.y, -a.z}; }
__device__ __forceinline__ ResV3 res_scale(ResV3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ double res_dot(ResV3 a, ResV3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ ResV3 res_cross(ResV3 a, ResV3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ ResV3 res_load(const double* p) { return {p[0], p[1], p[2]}; }

// P3PSolver_Nordberg::root2real (solver_resection_p3p_nordberg.hpp:22-38)
__device__ __forceinline__ bool res_root2real(double b, double c, double& r1, double& r2) {
  const double v = b * b - 4.0 * c;
  if (v <= 0.0) {
    r1 = r2 = -0.5 * b;
    return v >= 0.0;
  }
  const double y = sqrt(v);
  if (b < 0.0) {
    r1 = 0.5 * (-b + y);
    r2 = 0.5 * (-b - y);
  } else {
    r1 = 2.0 * c / (-b + y);
    r2 = 2.0 * c / (-b - y);
  }
  return true;
}

// What both solvers end with: R = [v1 v2 v1 x v2] [c0 c1 c0 x c1]^-1 (the inverse by cofactors, rows i0 i1 i2), t = base - R X0; the model
// is stored as the row-major 3 x 4 matrix [R | t]
struct ResFrame { ResV3 i0, i1, i2, X0; };
__device__ __forceinline__ ResFrame res_frame(ResV3 c0, ResV3 c1, ResV3 X0) {
  const ResV3 c2 = res_cross(c0, c1);
  const ResV3 r0 = res_cross(c1, c2), r1 = res_cross(c2, c0), r2 = res_cross(c0, c1);
  const double inv_det = 1.0 / res_dot(c0, r0);
  return {res_scale(r0, inv_det), res_scale(r1, inv_det), res_scale(r2, inv_det), X0};
}
__device__ __forceinline__ void res_emit(const ResFrame& f, ResV3 v1, ResV3 v2, ResV3 base, double* __restrict__ Rt) {
  const ResV3 v3 = res_cross(v1, v2);
  const double r00 = v1.x * f.i0.x + v2.x * f.i1.x + v3.x * f.i2.x, r01 = v1.x * f.i0.y + v2.x * f.i1.y + v3.x * f.i2.y, r02 = v1.x * f.i0.z + v2.x * f.i1.z + v3.x * f.i2.z;
  const double r10 = v1.y * f.i0.x + v2.y * f.i1.x + v3.y * f.i2.x, r11 = v1.y * f.i0.y + v2.y * f.i1.y + v3.y * f.i2.y, r12 = v1.y * f.i0.z + v2.y * f.i1.z + v3.y * f.i2.z;
  const double r20 = v1.z * f.i0.x + v2.z * f.i1.x + v3.z * f.i2.x, r21 = v1.z * f.i0.y + v2.z * f.i1.y + v3.z * f.i2.y, r22 = v1.z * f.i0.z + v2.z * f.i1.z + v3.z * f.i2.z;
  Rt[0] = r00; Rt[1] = r01; Rt[2] = r02; Rt[3] = base.x - (r00 * f.X0.x + r01 * f.X0.y + r02 * f.X0.z);
  Rt[4] = r10; Rt[5] = r11; Rt[6] = r12; Rt[7] = base.y - (r10 * f.X0.x + r11 * f.X0.y + r12 * f.X0.z);
  Rt[8] = r20; Rt[9] = r21; Rt[10] = r22; Rt[11] = base.z - (r20 * f.X0.x + r21 * f.X0.y + r22 * f.X0.z);
}

// ---- P3PSolver_Ding (solver_resection_p3p_ding.cpp) ----
__device__ __forceinline__ void ding_refine(double& l1, double& l2, double& l3, double a12, double a13, double a23, double b12, double b13, double b23) {
  for (int it = 0; it < 5; ++it) {
    const double r1 = (l1 * l1 - 2.0 * l1 * l2 * b12 + l2 * l2 - a12);
    const double r2 = (l1 * l1 - 2.0 * l1 * l3 * b13 + l3 * l3 - a13);
    const double r3 = (l2 * l2 - 2.0 * l2 * l3 * b23 + l3 * l3 - a23);
    if (fabs(r1) + fabs(r2) + fabs(r3) < 1e-10) return;
    const double x11 = l1 - l2 * b12, x12 = l2 - l1 * b12, x21 = l1 - l3 * b13, x23 = l3 - l1 * b13, x32 = l2 - l3 * b23, x33 = l3 - l2 * b23;
    const double detJ = 0.5 / (x11 * x23 * x32 + x12 * x21 * x33);
    const double n1 = l1 + (-x23 * x32 * r1 - x12 * x33 * r2 + x12 * x23 * r3) * detJ;
    const double n2 = l2 + (-x21 * x33 * r1 + x11 * x33 * r2 - x11 * x23 * r3) * detJ;
    const double n3 = l3 + (x21 * x32 * r1 - x11 * x32 * r2 - x12 * x21 * r3) * detJ;
    l1 = n1; l2 = n2; l3 = n3;
  }
}
__device__ __forceinline__ bool ding_cubic_single_real(double c2, double c1, double c0, double& root) {
  const double a = c1 - c2 * c2 / 3.0;
  double b = (2.0 * c2 * c2 * c2 - 9.0 * c2 * c1) / 27.0 + c0;
  double c = b * b / 4.0 + a * a * a / 27.0;
  if (c != 0) {
    if (c > 0) {
      c = sqrt(c);
      b *= -0.5;
      root = cbrt(b + c) + cbrt(b - c) - c2 / 3.0;
      return true;
    }
    c = 3.0 * b / (2.0 * a) * sqrt(-3.0 / a);
    root = 2.0 * sqrt(-a / 3.0) * cos(acos(c) / 3.0) - c2 / 3.0;
  } else {
    root = -c2 / 3.0 + (a != 0 ? (3.0 * b / a) : 0);
  }
  return false;
}
struct DingCtx {
  double a, b, a01, a02, a12, m01, m02, m12;
  ResV3 x0, x1, x2;
  ResFrame f;
};
// one positive tau of one line: depths, the refinement, the pose
__device__ __forceinline__ void ding_tau(const DingCtx& c, bool switch_12, double tau, double w0, double w1, double* __restrict__ Rt, int& n_sols) {
  if (tau <= 0) return;
  double d0, d1, d2;
  if (switch_12) {
    d2 = sqrt(c.a12 / (tau * (tau - 2.0 * c.m12) + 1.0));
    d1 = tau * d2;
    d0 = (w0 * d2 + w1 * d1);
    if (d0 < 0) return;
  } else {
    d0 = sqrt(c.a01 / (tau * (tau - 2.0 * c.m01) + 1.0));
    d1 = tau * d0;
    d2 = w0 * d0 + w1 * d1;
    if (d2 < 0) return;
  }
  ding_refine(d0, d1, d2, c.a01, c.a02, c.a12, c.m01, c.m02, c.m12);
  const ResV3 base = res_scale(c.x0, d0);
  res_emit(c.f, res_sub(base, res_scale(c.x1, d1)), res_sub(base, res_scale(c.x2, d2)), base, Rt + 12 * n_sols);
  ++n_sols;
}
__device__ __forceinline__ void ding_line(const DingCtx& c, double p0, double p1, double p2, double* __restrict__ Rt, int& n_sols) {
  const bool switch_12 = fabs(p0) <= fabs(p1);
  double w0, w1, cb, cc, tau0, tau1;
  if (switch_12) {
    w0 = -p0 / p1;
    w1 = -p2 / p1;
    const double ca = 1.0 / (w1 * w1 - c.b);
    cb = 2.0 * (c.b * c.m12 - c.m02 * w1 + w0 * w1) * ca;
    cc = (w0 * w0 - 2 * c.m02 * w0 - c.b + 1.0) * ca;
  } else {
    w0 = -p1 / p0;
    w1 = -p2 / p0;
    const double ca = 1.0 / (-c.a * w1 * w1 + 2 * c.a * c.m12 * w1 - c.a + 1);
    cb = 2 * (c.a * c.m12 * w0 - c.m01 - c.a * w0 * w1) * ca;
    cc = (1 - c.a * w0 * w0) * ca;
  }
  if (!res_root2real(cb, cc, tau0, tau1)) return;
  ding_tau(c, switch_12, tau0, w0, w1, Rt, n_sols);
  ding_tau(c, switch_12, tau1, w0, w1, Rt, n_sols);
}
// bear, X: three vectors each (3 x 3 doubles, one vector after the other); Rt: up to four [R | t]; returns their number
__device__ __forceinline__ int p3p_ding(const double* __restrict__ bear, const double* __restrict__ X, double* __restrict__ Rt) {
  ResV3 X0 = res_load(X), X1 = res_load(X + 3), X2 = res_load(X + 6);
  ResV3 X01 = res_sub(X0, X1), X02 = res_sub(X0, X2);
  const ResV3 X12 = res_sub(X1, X2);
  double a01 = res_dot(X01, X01), a02 = res_dot(X02, X02), a12 = res_dot(X12, X12);
  ResV3 x0 = res_load(bear), x1 = res_load(bear + 3), x2 = res_load(bear + 6);
  // the columns are switched so that |X1 - X2| is the largest of the three distances
  if (a01 > a02) {
    if (a01 > a12) {
      ResV3 t = X0; X0 = X2; X2 = t;
      t = x0; x0 = x2; x2 = t;
      const double s = a01; a01 = a12; a12 = s;
      X01 = res_neg(X12);
      X02 = res_neg(X02);
    }
  } else if (a02 > a12) {
    ResV3 t = X0; X0 = X1; X1 = t;
    t = x0; x0 = x1; x1 = t;
    const double s = a02; a02 = a12; a12 = s;
    X01 = res_neg(X01);
    X02 = X12;
  }
  const double a12d = 1.0 / a12;
  const double a = a01 * a12d, b = a02 * a12d;
  const double m01 = res_dot(x0, x1), m02 = res_dot(x0, x2), m12 = res_dot(x1, x2);
  const double m12sq = -m12 * m12 + 1.0, m02sq = -1.0 + m02 * m02, m01sq = -1.0 + m01 * m01;
  const double ab = a * b, bsq = b * b, asq = a * a;
  const double m013 = -2.0 + 2.0 * m01 * m02 * m12;
  const double bsqm12sq = bsq * m12sq, asqm12sq = asq * m12sq, abm12sq = 2.0 * ab * m12sq;
  const double k3_inv = 1.0 / (bsqm12sq + b * m02sq);
  const double k2 = k3_inv * ((-1.0 + a) * m02sq + abm12sq + bsqm12sq + b * m013);
  const double k1 = k3_inv * (asqm12sq + abm12sq + a * m013 + (-1.0 + b) * m01sq);
  const double k0 = k3_inv * (asqm12sq + a * m01sq);
  double s;
  const bool G = ding_cubic_single_real(k2, k1, k0, s);
  // the degenerate conic C = C1 + s C2 (symmetric) and its split into two lines (compute_pq)
  const double C00 = -a + s * (1 - b), C01 = -m02 * s, C02 = a * m12 + b * m12 * s, C11 = s + 1, C12 = -m01, C22 = -a - b * s + 1;
  const double A00 = C12 * C12 - C11 * C22, A11 = C02 * C02 - C00 * C22, A22 = C01 * C01 - C00 * C11;
  const double A01 = C01 * C22 - C02 * C12, A02 = C02 * C11 - C01 * C12, A12 = C00 * C12 - C02 * C01;
  double v0, v1, v2;
  if (A00 > A11) {
    if (A00 > A22) { const double q = sqrt(A00); v0 = A00 / q; v1 = A01 / q; v2 = A02 / q; }
    else { const double q = sqrt(A22); v0 = A02 / q; v1 = A12 / q; v2 = A22 / q; }
  } else if (A11 > A22) {
    const double q = sqrt(A11); v0 = A01 / q; v1 = A11 / q; v2 = A12 / q;
  } else {
    const double q = sqrt(A22); v0 = A02 / q; v1 = A12 / q; v2 = A22 / q;
  }
  (void)v0;   // (v(0) only moves C(1,2) / C(2,1), which neither line reads)
  DingCtx c{a, b, a01, a02, a12, m01, m02, m12, x0, x1, x2, res_frame(X01, X02, X0)};
  int n_sols = 0;
  ding_line(c, C00, C01 + v2, C02 - v1, Rt, n_sols);   // pq[0] = C.col(0)
  if (n_sols > 0 && G) return n_sols;                  // only one line of the pair meets the conic
  ding_line(c, C00, C01 - v2, C02 + v1, Rt, n_sols);   // pq[1] = C.row(0)
  return n_sols;
}

// ---- P3PSolver_Nordberg (solver_resection_p3p_nordberg.cpp) ----
__device__ __forceinline__ void nordberg_refine(double& L1, double& L2, double& L3, double a12, double a13, double a23, double b12, double b13, double b23) {
  for (int i = 0; i < 5; ++i) {
    const double l1 = L1, l2 = L2, l3 = L3;
    const double r1 = l1 * l1 + l2 * l2 + b12 * l1 * l2 - a12;
    const double r2 = l1 * l1 + l3 * l3 + b13 * l1 * l3 - a13;
    const double r3 = l2 * l2 + l3 * l3 + b23 * l2 * l3 - a23;
    if (fabs(r1) + fabs(r2) + fabs(r3) < 1e-10) break;
    const double v0 = 2.0 * l1 + b12 * l2, v1 = 2.0 * l2 + b12 * l1, v3 = 2.0 * l1 + b13 * l3, v5 = 2.0 * l3 + b13 * l1;
    const double v7 = 2.0 * l2 + b23 * l3, v8 = 2.0 * l3 + b23 * l2;
    const double det = 1.0 / (-v0 * v5 * v7 - v1 * v3 * v8);
    const double n1 = l1 - det * (-v5 * v7 * r1 + -v1 * v8 * r2 + v1 * v5 * r3);
    const double n2 = l2 - det * (-v3 * v8 * r1 + v0 * v8 * r2 + -v0 * v5 * r3);
    const double n3 = l3 - det * (v3 * v7 * r1 + -v0 * v7 * r2 + -v1 * v3 * r3);
    const double r11 = n1 * n1 + n2 * n2 + b12 * n1 * n2 - a12;
    const double r12 = n1 * n1 + n3 * n3 + b13 * n1 * n3 - a13;
    const double r13 = n2 * n2 + n3 * n3 + b23 * n2 * n3 - a23;
    if (fabs(r11) + fabs(r12) + fabs(r13) > fabs(r1) + fabs(r2) + fabs(r3)) break;
    L1 = n1; L2 = n2; L3 = n3;
  }
}
__device__ __forceinline__ double nordberg_cubick(double b, double c, double d) {
  double r0;
  if (b * b >= 3.0 * c) {
    const double v = sqrt(b * b - 3.0 * c);
    const double t1 = (-b - v) / (3.0);
    double k = ((t1 + b) * t1 + c) * t1 + d;
    if (k > 0.0) {
      r0 = t1 - sqrt(-k / (3.0 * t1 + b));
    } else {
      const double t2 = (-b + v) / 3.0;
      k = ((t2 + b) * t2 + c) * t2 + d;
      r0 = t2 + sqrt(-k / (3.0 * t2 + b));
    }
  } else {
    r0 = -b / 3.0;
    if (fabs(((3.0 * r0 + 2.0 * b) * r0 + c)) < 1e-4) r0 += 1;
  }
  for (unsigned int cnt = 0; cnt < 50; ++cnt) {
    const double fx = (((r0 + b) * r0 + c) * r0 + d);
    if ((cnt < 7 || fabs(fx) > 1e-13)) {
      const double fpx = ((3.0 * r0 + 2.0 * b) * r0 + c);
      r0 -= fx / fpx;
    } else {
      break;
    }
  }
  return r0;
}
struct NordbergCtx {
  double a12, a13, a23, b12, b13, b23;
  ResV3 f1, f2, f3;
  ResFrame f;
};
__device__ __forceinline__ void nordberg_pose(const NordbergCtx& c, double l1, double l2, double l3, double* __restrict__ Rt, int& valid) {
  nordberg_refine(l1, l2, l3, c.a12, c.a13, c.a23, c.b12, c.b13, c.b23);
  const ResV3 ry1 = res_scale(c.f1, l1), ry2 = res_scale(c.f2, l2), ry3 = res_scale(c.f3, l3);
  res_emit(c.f, res_sub(ry1, ry2), res_sub(ry1, ry3), ry1, Rt + 12 * valid);
  ++valid;
}
__device__ __forceinline__ void nordberg_sign(const NordbergCtx& c, ResV3 U, double* __restrict__ Rt, int& valid) {
  const double u1 = U.x, u2 = U.y, u3 = U.z;
  const double a12 = c.a12, a13 = c.a13, a23 = c.a23, b12 = c.b12, b13 = c.b13, b23 = c.b23;
  double tau0, tau1;
  if (fabs(u1) < fabs(u2)) {   // solve for l2
    const double a = (a23 - a12) * u3 * u3 - a12 * u2 * u2 + a12 * b23 * u2 * u3;
    const double b = (2. * a23 * u1 * u3 - 2. * a12 * u1 * u3 + a12 * b23 * u1 * u2 - a23 * b12 * u2 * u3) / a;
    const double cq = (a23 * u1 * u1 - a12 * u1 * u1 + a23 * u2 * u2 - a23 * b12 * u1 * u2) / a;
    if (!res_root2real(b, cq, tau0, tau1)) return;
    for (int r = 0; r < 2; ++r) {
      const double tau = r == 0 ? tau0 : tau1;
      if (tau <= 0) continue;
      const double l1 = sqrt(a13 / (tau * (tau + b13) + 1.));
      const double l3 = tau * l1;
      const double l2 = -(u1 * l1 + u3 * l3) / u2;
      if (l2 <= 0.) continue;
      nordberg_pose(c, l1, l2, l3, Rt, valid);
    }
  } else {   // solve for l1
    const double w2 = 1. / (-u1);
    const double w0 = u2 * w2, w1 = u3 * w2;
    const double a = 1.0 / ((a13 - a12) * w1 * w1 - a12 * b13 * w1 - a12);
    const double b = (a13 * b12 * w1 - a12 * b13 * w0 - 2. * w0 * w1 * (a12 - a13)) * a;
    const double cq = ((a13 - a12) * w0 * w0 + a13 * b12 * w0 + a13) * a;
    if (!res_root2real(b, cq, tau0, tau1)) return;
    for (int r = 0; r < 2; ++r) {
      const double tau = r == 0 ? tau0 : tau1;
      if (tau <= 0.) continue;
      const double d = a23 / (tau * (b23 + tau) + 1.0);
      const double l2 = sqrt(d);
      const double l3 = tau * l2;
      const double l1 = w0 * l2 + w1 * l3;
      if (l1 <= 0.) continue;
      nordberg_pose(c, l1, l2, l3, Rt, valid);
    }
  }
}
// (The reference collects the up to four depth triples, refines them all, then forms the poses: each triple's refinement and pose depend
// on that triple alone, so they are formed here as the triples are found - the same models in the same order.)
__device__ __forceinline__ int p3p_nordberg(const double* __restrict__ bear, const double* __restrict__ X, double* __restrict__ Rt) {
  const ResV3 P1 = res_load(X), P2 = res_load(X + 3), P3 = res_load(X + 6);
  const ResV3 f1 = res_load(bear), f2 = res_load(bear + 3), f3 = res_load(bear + 6);
  const double b12 = -2.0 * (res_dot(f1, f2)), b13 = -2.0 * (res_dot(f1, f3)), b23 = -2.0 * (res_dot(f2, f3));
  const ResV3 d12 = res_sub(P1, P2), d13 = res_sub(P1, P3), d23 = res_sub(P2, P3);
  const double a12 = res_dot(d12, d12), a13 = res_dot(d13, d13), a23 = res_dot(d23, d23);
  const double c31 = -0.5 * b13, c23 = -0.5 * b23, c12 = -0.5 * b12;
  const double blob = (c12 * c23 * c31 - 1.0);
  const double s31_squared = 1.0 - c31 * c31, s23_squared = 1.0 - c23 * c23, s12_squared = 1.0 - c12 * c12;
  double p3 = a13 * (a23 * s31_squared - a13 * s23_squared);
  double p2 = 2.0 * blob * a23 * a13 + a13 * (2.0 * a12 + a13) * s23_squared + a23 * (a23 - a12) * s31_squared;
  double p1 = a23 * (a13 - a23) * s12_squared - a12 * a12 * s23_squared - 2.0 * a12 * (blob * a23 + a13 * s23_squared);
  double p0 = a12 * (a12 * s23_squared - a23 * s12_squared);
  p3 = 1.0 / p3;
  p2 *= p3; p1 *= p3; p0 *= p3;
  const double g = nordberg_cubick(p2, p1, p0);
  const double A00 = a23 * (1.0 - g), A01 = (a23 * b12) * 0.5, A02 = (a23 * b13 * g) * (-0.5);
  const double A11 = a23 - a12 + a13 * g, A12 = b23 * (a13 * g - a12) * 0.5, A22 = g * (a13 - a23) - a12;
  // eigwithknown0: A has a zero eigenvalue; the other two from the characteristic quadratic, the larger in magnitude first, and their
  // vectors (the vector of the zero eigenvalue is computed by the reference and never read: left out)
  const double x01_squared = A01 * A01;
  const double qb = -A00 - A11 - A22;
  const double qc = -x01_squared - A02 * A02 - A12 * A12 + A00 * (A11 + A22) + A11 * A22;
  double e1, e2;
  (void)res_root2real(qb, qc, e1, e2);
  if (fabs(e1) < fabs(e2)) { const double t = e1; e1 = e2; e2 = t; }
  const double mx0011 = -A00 * A11;
  const double prec_0 = A01 * A12 - A02 * A11, prec_1 = A01 * A02 - A00 * A12;
  const double tmp = 1.0 / (e1 * (A00 + A11) + mx0011 - e1 * e1 + x01_squared);
  double a1 = -(e1 * A02 + prec_0) * tmp, a2 = -(e1 * A12 + prec_1) * tmp;
  const double rnorm = 1.0 / sqrt(a1 * a1 + a2 * a2 + 1.0);
  a1 *= rnorm; a2 *= rnorm;
  const double tmp2 = 1.0 / (e2 * (A00 + A11) + mx0011 - e2 * e2 + x01_squared);
  double a21 = -(e2 * A02 + prec_0) * tmp2, a22 = -(e2 * A12 + prec_1) * tmp2;
  const double rnorm2 = 1.0 / sqrt(a21 * a21 + a22 * a22 + 1.0);
  a21 *= rnorm2; a22 *= rnorm2;
  const double q = -e2 / e1;
  const double v = sqrt(0.0 < q ? q : 0.0);   // std::max(0.0, q): 0 for a NaN
  NordbergCtx c{a12, a13, a23, b12, b13, b23, f1, f2, f3, res_frame(d12, d13, P1)};
  int valid = 0;
  nordberg_sign(c, ResV3{a1 - v * a21, a2 - v * a22, rnorm - v * rnorm2}, Rt, valid);
  nordberg_sign(c, ResV3{a1 - (-v) * a21, a2 - (-v) * a22, rnorm - (-v) * rnorm2}, Rt, valid);
  return valid;
}

__device__ __forceinline__ int res_solve(int solver, const double* __restrict__ bear, const double* __restrict__ X, double* __restrict__ Rt) {
  return solver == kResSolverNordberg ? p3p_nordberg(bear, X, Rt) : p3p_ding(bear, X, Rt);
}

// Test hook: one lane per sample
__global__ __launch_bounds__(64) void resection_p3p_debug_kernel(int solver, const double* __restrict__ bear, const double* __restrict__ X, uint32_t n_samples,
                                                                 double* __restrict__ Rt_out, int* __restrict__ n_out) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n_samples) return;
  n_out[i] = res_solve(solver, bear + 9 * (size_t)i, X + 9 * (size_t)i, Rt_out + 48 * (size_t)i);
}

// ---- prepare pass: the bearing of every correspondence, once per problem ----
__global__ __launch_bounds__(256) void resection_bearing_kernel(const ResProblem* __restrict__ problems, uint32_t n_problems, uint64_t n_total,
                                                                const double* __restrict__ x2d, double* __restrict__ bear) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_total) return;
  const ResProblem& P = res_problem_of(problems, n_problems, i);
  double b[3];
  mvgx_ba::camera_bearing((int)P.model, P.intr, x2d + 2 * i, /*undistort=*/false, b);
  bear[3 * i] = b[0]; bear[3 * i + 1] = b[1]; bear[3 * i + 2] = b[2];
}

// ---- what the P3P solvers give the loop (both the exhaustive kernel of mvgx_resection_loop.h and the bounded one below) ----
struct ResP3PForm {
  using Problem = ResProblem;
  using Layout = ResLayout<3, kResVerdict, 48, 0, true>;   // a wave's work: up to four [R | t]
  static constexpr int kSample = 3, kMaxModels = 4, kModelAt = 0;
  const double2* px;
  const double *pX, *pb, *intr;
  double n1norm;
  int res_model, solver;
  __device__ __forceinline__ ResP3PForm(const ResProblem& P, const double* __restrict__ x2d, const double* __restrict__ X3d, const double* __restrict__ bear, int solver_)
      : px(reinterpret_cast<const double2*>(x2d) + P.start), pX(X3d + 3 * P.start), pb(bear + 3 * P.start), intr(P.intr), n1norm(P.n1),
        res_model(P.model == (uint32_t)mvgx_ba::kCamSpherical ? mvgx_ba::kCamSpherical : mvgx_ba::kCamPinhole),   // ignore_distortion
        solver(solver_) {}
  // the sample's vectors go to the wave's verdict slot (its first 18 doubles), read by lane 0's solve before the verdict is written
  __device__ __forceinline__ void load_sample(const uint32_t* sample, double*, double* verdict, int lane) const {
    if (lane < 3) {
      const uint32_t s = sample[lane];
      verdict[3 * lane] = pb[3 * s]; verdict[3 * lane + 1] = pb[3 * s + 1]; verdict[3 * lane + 2] = pb[3 * s + 2];
      verdict[9 + 3 * lane] = pX[3 * s]; verdict[9 + 3 * lane + 1] = pX[3 * s + 1]; verdict[9 + 3 * lane + 2] = pX[3 * s + 2];
    }
  }
  __device__ __forceinline__ int solve(double* work, const double* verdict, uint32_t* count, int lane) const {
    if (lane == 0) *count = (uint32_t)res_solve(solver, verdict, verdict + 9, work);
    wave_sync();
    return (int)*count;
  }
  // the normalised squared residual of correspondence i under M (every pass of both loops goes through here, so a residual has the
  // same bits wherever it is compared)
  __device__ __forceinline__ double residual(const ResRt& M, uint32_t i) const {
    const double X = pX[3 * i], Y = pX[3 * i + 1], Z = pX[3 * i + 2];
    const double pc[3] = {M.m0 * X + M.m1 * Y + M.m2 * Z + M.m3, M.m4 * X + M.m5 * Y + M.m6 * Z + M.m7, M.m8 * X + M.m9 * Y + M.m10 * Z + M.m11};
    const double2 obs = px[i];
    const double ob[2] = {obs.x, obs.y};
    double r[2];
    mvgx_ba::project_residual(res_model, intr, pc, ob, r);
    const double rx = mul_rn(r[0], n1norm), ry = mul_rn(r[1], n1norm);
    return add_rn(mul_rn(rx, rx), mul_rn(ry, ry));
  }
};
static_assert(4 * ResP3PForm::Layout::words(kResLdsMaxN) <= 160 * 1024, "the LDS form must fit a workgroup's 160 KiB");

// ---- the bounded form (mvgx_resection_localize_bounded): a finite precision ----
// robust_estimator_ACRansac.hpp:205-256 (the NFA read off a 20-bin histogram), :351-358, :375, :386-389 (the warm-up's rejection sampler,
// rand_sampling.hpp:36-58), :402-413 (max-consensus until a model has more than 2.5 x 3 residuals inside the bound), :446-452 (the early
// exit). No sort: per model n residuals, 20 counters and, for a model that lowers minNFA, one list in index order. The mapping is the
// exhaustive loop's - one workgroup per problem, one wave per iteration evaluated ahead - and the kernel is built from the pieces of
// mvgx_resection_loop.h (layout, tables, draw and rewind, budget, result) and ResP3PForm's sample, solver and residual. Its own: the
// verdicts, with two more kinds of event - the switch to the a-contrario mode, and a list that was rebuilt but came out too short to
// count as a better model (:243-255) -, the warm-up's sampler and the early exit.
// Deliberate differences: a model with a non-finite entry is skipped (as in the exhaustive loop); an adopted pool of fewer than three entries stops the
// problem with its current result (the reference's sampler returns false there, unchecked, and the stale sample is evaluated again).
constexpr uint32_t kResBLdsMaxN = 8192;       // largest n whose four tables live in LDS (DESIGN.md derives it)
constexpr int kResBVerdict = 32;              // doubles per wave: flags | nfa | threshold | unused | P[12] | models evaluated | list threshold | list P[12] | unused
constexpr int kResBBetter = 1, kResBRebuilt = 2, kResBSwitched = 4;   // a verdict's flags
struct ResBound {         // per problem, prepared on the host (glibc's log10)
  double max_threshold, bins_by_interval;   // error_max^2 n1^2; 20 / max_threshold
  double bin_value[kBins];                  // (max_threshold / 19) b: histogram.hpp:105-112, not the bins' edges
  double logalpha_bin[kBins];               // logalpha0 + log10(bin_value + FLT_EPSILON)
};
// the layout's extra words: histograms (kBins counters per wave) | resb_rebuild_list's counts (two sets); no sort slices
using ResBLayout = ResLayout<3, kResBVerdict, 48, kResWaves * kBins + 2 * kResWaves, false>;
static_assert(4 * ResBLayout::words(kResBLdsMaxN) <= 160 * 1024, "the LDS form must fit a workgroup's 160 KiB");

// UniformSample(3, nData, ...) (rand_sampling.hpp:36-58): three distinct indices of [0, n - 1], a repeated one drawn again (n > 3 here)
__device__ __forceinline__ void resb_draw_distinct(uint32_t* mt, int& mt_idx, int lane, uint32_t n, uint32_t& c0, uint32_t& c1, uint32_t& c2) {
  c0 = uniform_u32(mt, mt_idx, lane, 0, n - 1);
  do { c1 = uniform_u32(mt, mt_idx, lane, 0, n - 1); } while (c1 == c0);
  do { c2 = uniform_u32(mt, mt_idx, lane, 0, n - 1); } while (c2 == c0 || c2 == c1);
}
// the inlier list of (M, thr) by the whole workgroup: the indices with e <= thr in index order. 512 consecutive indices per round: a
// ballot and a count per wave, the prefix over the eight waves' counts (two sets of counts: one barrier per round). Returns the length.
__device__ __forceinline__ uint32_t resb_rebuild_list(const ResP3PForm& F, const ResRt& M, double thr, uint32_t n, uint32_t* inliers, uint32_t* wcount, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  uint32_t total = 0, set = 0;
  for (uint32_t base = 0; base < n; base += 64 * kResWaves, set ^= (uint32_t)kResWaves) {
    const uint32_t i = base + (uint32_t)tid;
    const bool in = i < n && F.residual(M, i) <= thr;   // (a NaN is no inlier)
    const unsigned long long bal = __ballot(in);
    if (lane == 0) wcount[set + wave] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kResWaves; ++w) {
      const uint32_t c = wcount[set + w];
      before += w < wave ? c : 0u;
      all += c;
    }
    if (in) inliers[total + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = i;
    total += all;
  }
  __syncthreads();
  return total;
}

// (n_lds_max is not read: without slices nothing is sized for the launch's largest problem; the launcher passes it to every loop kernel)
template <bool kGlobal>
__global__ __launch_bounds__(64 * kResWaves) void resection_acransac_bounded_kernel(const uint32_t* __restrict__ order, uint32_t n_work, uint32_t /*n_lds_max*/,
                                                                                    const ResProblem* __restrict__ problems, const ResBound* __restrict__ bounds,
                                                                                    const double* __restrict__ x2d, const double* __restrict__ X3d, const double* __restrict__ bear,
                                                                                    const float* __restrict__ l10, const uint32_t* __restrict__ mt_init, uint32_t max_iteration, int solver,
                                                                                    uint32_t waves_ahead, unsigned char* __restrict__ scratch, ResResult* __restrict__ results,
                                                                                    uint32_t* __restrict__ inliers_out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_u32[];
  if (blockIdx.x >= n_work) return;
  using L = ResBLayout;
  const uint32_t pi = order[blockIdx.x];
  const ResProblem& P = problems[pi];
  const ResBound& B = bounds[pi];
  const uint32_t n = P.n;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  const L lds(lds_u32);
  const ResTables T = res_tables(kGlobal ? reinterpret_cast<uint32_t*>(scratch + P.scratch) : lds.tables, n, n, L::kHasSlices);
  uint32_t* const hists = lds.extra;                          // kBins counters per wave
  uint32_t* const wcount = hists + kResWaves * kBins;         // resb_rebuild_list's counts
  uint32_t* const my_hist = hists + kBins * wave;

  const ResP3PForm F(P, x2d, X3d, bear, solver);   // the exhaustive loop's sample, solver and residual
  const double loge0 = P.loge0;
  const double max_threshold = B.max_threshold, bins_by_interval = B.bins_by_interval;
  const double my_bin_value = lane < kBins ? B.bin_value[lane] : 0.0, my_logalpha = lane < kBins ? B.logalpha_bin[lane] : 0.0;

  ResGen gen{lds.mt, lds.mt_saved, kMtN, kMtN};
  res_tables_init<3>(T, gen, mt_init, l10, n, tid);

  const uint32_t Wa = waves_ahead ? waves_ahead : (uint32_t)kResWaves;
  double minNFA = INFINITY, errorMax = INFINITY;
  if (tid == 0)
    for (int e = 0; e < 12; ++e) lds.best_model[e] = 0.0;
  bool ac = false, stop = false;   // bACRansacMode; an adopted pool was too small to sample from
  uint32_t n_inl = 0, pool_n = n;  // the length of vec_inliers, of vec_index
  uint32_t n_models_total = 0;
  ResBudget it(max_iteration);

  while (!stop && it.running()) {
    uint32_t nb = it.block(Wa);
    // the warm-up gives up after iteration 2 nIterReserve + 1 (:448): nothing is evaluated ahead past it
    if (!ac) nb = min(nb, 2u * (uint32_t)it.nIterReserve + 2u - it.iter);
    const bool ac_at_start = ac;
    // ---- the samples of the block, drawn in iteration order from the one generator (wave 0), in the block's mode ----
    if (wave == 0) {
      if (ac) res_draw_block<3>(gen, T.pool, pool_n, lds.swaps, lds.samples, nb, lane);
      else {   // the warm-up never touches the pool
        gen.save(lane);
        for (uint32_t j = 0; j < nb; ++j) {
          uint32_t c0, c1, c2;
          resb_draw_distinct(gen.mt, gen.idx, lane, n, c0, c1, c2);
          if (lane == 0) { lds.samples[3 * j] = c0; lds.samples[3 * j + 1] = c1; lds.samples[3 * j + 2] = c2; }
        }
      }
    }
    __syncthreads();

    // ---- one wave, one iteration ----
    if ((uint32_t)wave < nb) {
      double* const my_models = lds.works + L::kWork * wave;
      double* const my_verdict = lds.verdicts + L::kVerdict * wave;
      F.load_sample(lds.samples + 3 * wave, my_models, my_verdict, lane);
      wave_sync();
      const int nm = F.solve(my_models, my_verdict, lds.n_mod + wave, lane);
      bool my_ac = ac;
      double run_min = minNFA, win_thr = 0.0, list_thr = 0.0;
      int winner = -1, lister = -1;
      uint32_t evaluated = 0, flags = 0;
      for (int m = 0; m < nm; ++m) {
        const ResRt M = res_rt_load(my_models + 12 * m);
        if (!res_rt_finite(M)) continue;
        ++evaluated;
        if (lane < kBins) my_hist[lane] = 0;
        wave_sync();
        uint32_t n_le = 0;
        for (uint32_t base = 0; base < n; base += 64) {
          const uint32_t i = base + lane;
          const double e = i < n ? F.residual(M, i) : INFINITY;
          if (!my_ac) n_le += (uint32_t)__popcll(__ballot(i < n && e <= max_threshold));
          // Histogram::Add (histogram.hpp:74-86): a NaN or a huge value ends in no bin, like the cast to size_t on x86-64
          const double t = mul_rn(e, bins_by_interval);
          if (i < n && t >= 0.0 && t < (double)kBins) atomicAdd(&my_hist[(int)t], 1u);
        }
        if (!my_ac && (double)n_le > 2.5 * 3) { my_ac = true; flags |= (uint32_t)kResBSwitched; }   // for this model and every later one
        wave_sync();
        if (my_ac) {   // ComputeNFA_and_inliers, quantified form: lane b holds bin b (the geometric filter's scan and selection)
          uint32_t cum = lane < kBins ? my_hist[lane] : 0u;
          cum += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cum, 0x111, 0xF, 0xF, true);
          cum += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cum, 0x112, 0xF, 0xF, true);
          cum += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cum, 0x114, 0xF, 0xF, true);
          cum += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)cum, 0x118, 0xF, 0xF, true);
          {
            const uint32_t row0 = (uint32_t)__builtin_amdgcn_readlane((int)cum, 15);
            if (lane >= 16) cum += row0;
          }
          double cur = INFINITY;
          if (lane < kBins && cum > 3u && my_bin_value > kResFltEps) {
            cur = add_rn(add_rn(add_rn(loge0, mul_rn(my_logalpha, (double)(cum - 3u))), (double)T.logc_n[cum]), (double)T.logc_k[cum]);
            if (!(cur < 0)) cur = INFINITY;
          }
          // the first bin of strictly smallest NFA among the negative ones: wave maxima of an order-reversing key of the value's bits
          double cb_nfa = INFINITY, cb_thr = 0.0;
          {
            const bool cand = lane < kBins && cur < INFINITY;
            unsigned long long bits = (unsigned long long)__double_as_longlong(cur);
            bits = (bits >> 63) ? bits : ~(bits | 0x8000000000000000ull);
            const uint32_t hi = cand ? (uint32_t)(bits >> 32) : 0u;
            const uint32_t best_hi = wave_max_u32(hi);
            if (best_hi != 0u) {   // (wave-uniform; 0: no candidate)
              const bool top = cand && hi == best_hi;
              const uint32_t lo = top ? (uint32_t)bits : 0u;
              const uint32_t best_lo = wave_max_u32(lo);
              const unsigned long long holders = __ballot(top && lo == best_lo);
              const int b = (int)__builtin_ctzll(holders);
              cb_nfa = lane_value_f64(cur, b);
              cb_thr = lane_value_f64(my_bin_value, b);
            }
          }
          if (cb_nfa < run_min) {   // the list is rebuilt (by the workgroup, once the verdicts are read) before its size decides (:243-255)
            uint32_t cnt = 0;
            for (uint32_t base = 0; base < n; base += 64) {
              const uint32_t i = base + lane;
              cnt += (uint32_t)__popcll(__ballot(i < n && F.residual(M, i) <= cb_thr));
            }
            lister = m; list_thr = cb_thr; flags |= (uint32_t)kResBRebuilt;
            if (cnt > 3u) { run_min = cb_nfa; winner = m; win_thr = cb_thr; flags |= (uint32_t)kResBBetter; }
          }
        }
        wave_sync();   // (the histogram has been read before the next model clears it)
      }
      wave_sync();   // every lane has read the sample's vectors before the verdict overwrites the slot
      if (lane == 0) {
        my_verdict[0] = (double)flags;
        my_verdict[1] = run_min; my_verdict[2] = win_thr; my_verdict[3] = 0.0;
        const double* const Mw = my_models + 12 * (winner >= 0 ? winner : 0);
        const double* const Ml = my_models + 12 * (lister >= 0 ? lister : 0);
        for (int e = 0; e < 12; ++e) { my_verdict[4 + e] = Mw[e]; my_verdict[18 + e] = Ml[e]; }
        my_verdict[16] = (double)evaluated; my_verdict[17] = list_thr;
      }
    }
    __syncthreads();

    // ---- the verdicts in iteration order: the first event is applied, what follows it is void ----
    uint32_t done = nb;
    bool event = false;
    for (uint32_t j = 0; j < nb && !event; ++j) {
      const double* const v = lds.verdicts + L::kVerdict * j;
      n_models_total += (uint32_t)v[16];
      const uint32_t flags = (uint32_t)v[0];
      const bool better = (flags & (uint32_t)kResBBetter) != 0, rebuilt = (flags & (uint32_t)kResBRebuilt) != 0;
      if (flags & (uint32_t)kResBSwitched) ac = true;
      if (rebuilt) {   // vec_inliers of the iteration's last rebuild; a better model's is the last one or the size test failed after it
        n_inl = resb_rebuild_list(F, res_rt_load(v + 18), v[17], n, T.inliers, wcount, tid);
        if (better) {
          minNFA = v[1]; errorMax = v[2];
          res_keep_model(lds.best_model, v + 4, tid);
        }
      }
      // loop control (:446-474)
      bool take_pool = false, branch = false, early = false;
      if (!ac && (it.iter + j) > (uint32_t)(it.nIterReserve * 2)) { it.nIter = 0; early = true; }
      else if (ac) branch = it.reserve_event(better && minNFA < 0, j, n_inl, take_pool);
      if (rebuilt || ac != ac_at_start || branch || early) {
        event = true;
        done = j + 1;
        __syncthreads();   // the inlier list is complete; wave 0 may touch the pool
        if (done < nb && !early && wave == 0) {
          // the generator and the pool as they stood after iteration j, in the mode the block was drawn in (a switch voids what was
          // drawn ahead in the warm-up's mode)
          if (ac_at_start) res_rewind_block<3>(gen, T.pool, pool_n, lds.swaps, nb, done, lane);
          else {
            gen.restore(lane);
            for (uint32_t jj = 0; jj < done; ++jj) {
              uint32_t c0, c1, c2;
              resb_draw_distinct(gen.mt, gen.idx, lane, n, c0, c1, c2);
            }
          }
        }
        __syncthreads();
        if (take_pool) {   // (in index order)
          res_adopt_pool(T.pool, T.inliers, n_inl, pool_n, tid);
          if (pool_n < 3) stop = true;
        }
      }
    }
    it.iter += done;
    __syncthreads();
  }
  res_write_result(results[pi], inliers_out + P.start, T.inliers, lds.best_model, minNFA, errorMax, n_inl, it.iter, n_models_total, tid);
}

// ---- host ----
// KRt_From_P (multiview/projection.cpp:40-132) of P = [R | t]: RQ of the left block by three Givens rotations, the signs fixed, t = K^-1 p4
inline void res_mul3(const double* A, const double* B, double* C) {
  double T[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  memcpy(C, T, sizeof(T));
}
inline void res_krt_from_p(const double* P, double* K, double* R, double* t) {
  double Q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K[3 * i + j] = P[4 * i + j];
  const auto rotate = [&](const double* Qr) {
    double Qt[9];
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) Qt[3 * i + j] = Qr[3 * j + i];
    res_mul3(K, Qr, K);
    res_mul3(Qt, Q, Q);
  };
  if (K[7] != 0) {
    double c = -K[8], s = K[7];
    const double l = std::hypot(c, s);
    c /= l; s /= l;
    const double Qx[9] = {1, 0, 0, 0, c, -s, 0, s, c};
    rotate(Qx);
  }
  if (K[6] != 0) {
    double c = K[8], s = K[6];
    const double l = std::hypot(c, s);
    c /= l; s /= l;
    const double Qy[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    rotate(Qy);
  }
  if (K[3] != 0) {
    double c = -K[4], s = K[3];
    const double l = std::hypot(c, s);
    c /= l; s /= l;
    const double Qz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    rotate(Qz);
  }
  memcpy(R, Q, sizeof(Q));
  if (K[8] < 0)
    for (int e = 0; e < 9; ++e) { K[e] = -K[e]; R[e] = -R[e]; }
  if (K[4] < 0) {
    const double S[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
    res_mul3(K, S, K);
    res_mul3(S, R, R);
  }
  if (K[0] < 0) {
    const double S[9] = {-1, 0, 0, 0, 1, 0, 0, 0, 1};
    res_mul3(K, S, K);
    res_mul3(S, R, R);
  }
  // t = K^-1 p4 by elimination with partial pivoting (Eigen::PartialPivLU)
  double A[12];
  for (int i = 0; i < 3; ++i) { A[4 * i] = K[3 * i]; A[4 * i + 1] = K[3 * i + 1]; A[4 * i + 2] = K[3 * i + 2]; A[4 * i + 3] = P[4 * i + 3]; }
  for (int c = 0; c < 3; ++c) {
    int piv = c;
    for (int r = c + 1; r < 3; ++r)
      if (std::fabs(A[4 * r + c]) > std::fabs(A[4 * piv + c])) piv = r;
    if (piv != c)
      for (int e = 0; e < 4; ++e) std::swap(A[4 * c + e], A[4 * piv + e]);
    for (int r = c + 1; r < 3; ++r) {
      const double f = A[4 * r + c] / A[4 * c + c];
      for (int e = c; e < 4; ++e) A[4 * r + e] -= f * A[4 * c + e];
    }
  }
  t[2] = A[11] / A[10];
  t[1] = (A[7] - A[6] * t[2]) / A[5];
  t[0] = (A[3] - A[1] * t[1] - A[2] * t[2]) / A[0];
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  if (det < 0) {
    for (int e = 0; e < 9; ++e) R[e] = -R[e];
    for (int e = 0; e < 3; ++e) t[e] = -t[e];
  }
  const double k22 = K[8];
  for (int e = 0; e < 9; ++e) K[e] /= k22;
}

// What the three entries (mvgx_resection_localize, _bounded, _uncalibrated) share: the checks of a batch, the problem table and the
// staging, the uploads, the trace, the launches and the unpacking of the results. The buffers of one call; on scope exit the stream is
// drained and handed back before any of them is freed.
struct ResCall {
  const char* entry = "";
  uint32_t n_problems = 0, n_max = 0, n_lds_max = 0;   // n_lds_max: the largest problem of the LDS form
  uint64_t base = 0, n_total = 0;
  std::vector<uint32_t> in_lds, in_global;   // problems that reach the loop (n > the minimum sample), the largest first; the two storage forms
  // one page-locked staging buffer: problems | (bounded) bounds | launch lists | log10 table | generator state
  mvgx::PinnedBuf<uint64_t> stage;
  size_t stage_words = 0, prob_words = 0, bound_words = 0, n_lists = 0, l10_n = 0, scratch_bytes = 0;
  uint32_t* h_lists = nullptr;
  mvgx::DevBuf<uint64_t> d_stage;
  mvgx::DevBuf<double> d_x2d, d_X, d_bear;   // d_bear: what the prepare pass writes (bearings, or the normalised pixels in 2 of its 3 doubles)
  mvgx::DevBuf<unsigned char> d_scratch;
  mvgx::DevBuf<ResResult> d_res;
  mvgx::DevBuf<uint32_t> d_inl, d_trace;
  mvgx::PinnedBuf<ResResult> h_res;
  uint32_t* host_trace = nullptr;            // test hook: where this call's trace goes, its events per problem, its words
  uint32_t trace_events = 0;
  size_t trace_words = 0;
  hipStream_t stream = nullptr;
  int stream_device = 0;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ResCall() = default;
  ResCall(const ResCall&) = delete;
  ResCall& operator=(const ResCall&) = delete;
  ~ResCall() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) { (void)hipStreamSynchronize(stream); mvgx::release_stream(stream_device, stream); }
  }
  template <class Problem> Problem* h_prob() { return reinterpret_cast<Problem*>(stage.p); }
  template <class T> T* h_bound() { return reinterpret_cast<T*>(reinterpret_cast<uint32_t*>(stage.p) + prob_words); }
  // (launch arguments are plain pointers and counts: the test-suite's emulation captures them by value)
  template <class Problem> const Problem* p_prob() const { return reinterpret_cast<const Problem*>(d_stage.p); }
  template <class T> const T* p_bound() const { return reinterpret_cast<const T*>(reinterpret_cast<const uint32_t*>(d_stage.p) + prob_words); }
  const uint32_t* p_lists() const { return reinterpret_cast<const uint32_t*>(d_stage.p) + prob_words + bound_words; }
  const float* p_l10() const { return reinterpret_cast<const float*>(p_lists() + n_lists); }
  const uint32_t* p_mt() const { return reinterpret_cast<const uint32_t*>(p_l10() + l10_n); }
  uint32_t* p_trace() const { return host_trace ? d_trace.p : nullptr; }
};

// The checks every entry makes of its batch, after those of its own options: waves_ahead, then per problem the start, the size and
// check_problem(p) (returns an error code); sets c.n_problems and c.n_max
template <class CheckProblem>
int res_check_batch(ResCall& c, uint32_t n_problems, const uint64_t* start, const mvgx_resection_options* opt, CheckProblem check_problem) {
  const char* const fn = c.entry;
  MVGX_REQUIRE(opt->waves_ahead <= (uint32_t)kResWaves, MVGX_ERR_ARG, "%s: waves_ahead %u exceeds the build's %d", fn, opt->waves_ahead, kResWaves);
  c.n_problems = n_problems;
  c.n_max = 0;
  for (uint32_t p = 0; p < n_problems; ++p) {
    MVGX_REQUIRE(start[p + 1] >= start[p], MVGX_ERR_ARG, "%s: start decreases at problem %u", fn, p);
    const uint64_t n = start[p + 1] - start[p];
    MVGX_REQUIRE(n <= kResMaxN, MVGX_ERR_ARG, "%s: problem %u has %llu correspondences, the supported maximum is %u", fn, p, (unsigned long long)n, kResMaxN);
    if (const int rc = check_problem(p)) return rc;
    c.n_max = std::max(c.n_max, (uint32_t)n);
  }
  return MVGX_OK;
}

// The checks of the two calibrated entries, in one order
int res_check_arguments(ResCall& c, bool bounded, uint32_t n_problems, const uint64_t* start, const int32_t* intr_model, const double* intrinsics,
                        const mvgx_resection_options* opt, const uint8_t* out_ok, const double* out_pose, const double* out_P, const double* out_error_max,
                        const double* out_min_nfa, const uint64_t* out_inlier_start) {
  const char* const fn = c.entry;
  MVGX_REQUIRE(opt && start && out_ok && out_pose && out_P && out_error_max && out_min_nfa && out_inlier_start, MVGX_ERR_ARG, "%s: NULL argument", fn);
  MVGX_REQUIRE(n_problems == 0 || (intr_model && intrinsics), MVGX_ERR_ARG, "%s: NULL camera arrays", fn);
  MVGX_REQUIRE(opt->solver >= 0 && opt->solver <= 5, MVGX_ERR_ARG, "%s: solver %d is no resection::SolverType", fn, opt->solver);
  MVGX_REQUIRE(opt->solver == MVGX_RESECTION_P3P_DING || opt->solver == MVGX_RESECTION_P3P_NORDBERG, MVGX_ERR_UNSUPPORTED,
               "%s: solver %d has no device path (P3P_DING_CVPR23 = 4 and P3P_NORDBERG_ECCV18 = 3 have)", fn, opt->solver);
  if (bounded)
    MVGX_REQUIRE(std::isfinite(opt->error_max) && opt->error_max > 0, MVGX_ERR_ARG,
                 "%s: error_max must be a finite bound in pixels, > 0 (infinity - the exhaustive NFA - is mvgx_resection_localize's form)", fn);
  else
    MVGX_REQUIRE(std::isinf(opt->error_max) && opt->error_max > 0, MVGX_ERR_UNSUPPORTED,
                 "%s: a finite error_max selects the quantified NFA with the max-consensus early exit: that form is mvgx_resection_localize_bounded", fn);
  return res_check_batch(c, n_problems, start, opt, [&](uint32_t p) -> int {
    const int m = intr_model[p];
    MVGX_REQUIRE(mvgx_ba::intr_param_count(m) >= 0, MVGX_ERR_UNSUPPORTED, "%s: problem %u: camera model %d is not supported", fn, p, m);
    return MVGX_OK;
  });
}

// Clears the outputs and sorts the problems with more than min_sample correspondences (ACRANSAC returns early below that) into the two
// storage forms: the LDS form up to global_above, capped by lds_max_n; *work = whether any problem reaches the loop
int res_classify(ResCall& c, uint32_t min_sample, const uint64_t* start, const double* x2d, const double* X3d, const uint32_t* out_inliers, uint32_t global_above,
                 uint32_t lds_max_n, uint8_t* out_ok, double* out_error_max, double* out_min_nfa, uint64_t* out_inlier_start, mvgx_resection_stats* stats, bool* work) {
  const uint32_t n_problems = c.n_problems;
  const uint32_t lds_bound = global_above ? std::min(global_above, lds_max_n) : lds_max_n;
  *work = false;
  if (stats) memset(stats, 0, sizeof(*stats));
  for (uint32_t p = 0; p < n_problems; ++p) { out_ok[p] = 0; out_error_max[p] = 0.0; out_min_nfa[p] = 0.0; }
  for (uint32_t p = 0; p <= n_problems; ++p) out_inlier_start[p] = 0;
  if (!n_problems) return MVGX_OK;
  c.base = start[0];
  c.n_total = start[n_problems] - c.base;
  MVGX_REQUIRE(c.n_total == 0 || (x2d && X3d && out_inliers), MVGX_ERR_ARG, "%s: NULL correspondence arrays", c.entry);
  for (uint32_t p = 0; p < n_problems; ++p) {
    const uint64_t n = start[p + 1] - start[p];
    if (n > min_sample) (n <= lds_bound ? c.in_lds : c.in_global).push_back(p);
  }
  const auto by_n = [&](uint32_t a, uint32_t b) { const uint64_t na = start[a + 1] - start[a], nb = start[b + 1] - start[b]; return na != nb ? na > nb : a < b; };
  std::sort(c.in_lds.begin(), c.in_lds.end(), by_n);
  std::sort(c.in_global.begin(), c.in_global.end(), by_n);
  c.n_lds_max = c.in_lds.empty() ? 0 : (uint32_t)(start[c.in_lds[0] + 1] - start[c.in_lds[0]]);
  *work = !(c.in_lds.empty() && c.in_global.empty());
  return MVGX_OK;
}

// The staging buffer: the problem table (start, n and scratch offset here, the rest by fill(p, n, record)), bound_words for a second
// per-problem table behind it, the launch lists, the log10 table and the generator's initial state. glibc's log10: the reference's values.
template <class Problem, class Fill>
int res_stage(ResCall& c, const uint64_t* start, size_t bound_words, size_t (*scratch_bytes_of)(uint32_t), Fill fill) {
  const uint32_t n_problems = c.n_problems;
  int rc;
  c.n_lists = c.in_lds.size() + c.in_global.size();
  c.prob_words = (size_t)n_problems * sizeof(Problem) / 4;
  c.bound_words = bound_words;
  c.l10_n = (size_t)c.n_max + 2;
  c.stage_words = c.prob_words + c.bound_words + c.n_lists + c.l10_n + kMtN;
  if ((rc = c.stage.ensure((c.stage_words + 1) / 2))) return rc;
  Problem* const hp = c.h_prob<Problem>();
  c.h_lists = reinterpret_cast<uint32_t*>(c.stage.p) + c.prob_words + c.bound_words;
  float* const h_l10 = reinterpret_cast<float*>(c.h_lists + c.n_lists);
  uint32_t* const h_mt = reinterpret_cast<uint32_t*>(h_l10 + c.l10_n);
  for (uint32_t p = 0; p < n_problems; ++p) {
    Problem& g = hp[p];
    g.start = start[p] - c.base; g.n = (uint32_t)(start[p + 1] - start[p]); g.scratch = 0;
    fill(p, g.n, g);
  }
  c.scratch_bytes = 0;
  for (uint32_t p : c.in_global) { hp[p].scratch = c.scratch_bytes; c.scratch_bytes += scratch_bytes_of(hp[p].n); }
  if (!c.in_lds.empty()) memcpy(c.h_lists, c.in_lds.data(), c.in_lds.size() * 4);
  if (!c.in_global.empty()) memcpy(c.h_lists + c.in_lds.size(), c.in_global.data(), c.in_global.size() * 4);
  for (size_t i = 0; i < c.l10_n; ++i) h_l10[i] = (float)::log10((double)static_cast<float>(i));
  h_mt[0] = 5489u;   // std::mt19937::default_seed
  for (int i = 1; i < kMtN; ++i) h_mt[i] = 1812433253u * (h_mt[i - 1] ^ (h_mt[i - 1] >> 30)) + (uint32_t)i;
  return MVGX_OK;
}
// The record of a calibrated problem; bounded: the histogram constants of error_max too
void res_fill_calibrated(ResCall& c, bool bounded, const int32_t* intr_model, const double* intrinsics, double error_max, uint32_t p, uint32_t n, ResProblem& g) {
  g.model = (uint32_t)intr_model[p];
  memcpy(g.intr, intrinsics + 8 * (size_t)p, sizeof(g.intr));
  // imagePlane_toCameraPlaneError(1): 1 / focal (pinhole family), 1 / max(w, h) (spherical)
  g.n1 = intr_model[p] == mvgx_ba::kCamSpherical ? 1.0 / std::max(g.intr[0], g.intr[1]) : 1.0 / g.intr[0];
  g.loge0 = n > 3 ? std::log10(4.0 * (double)(n - 3)) : 0.0;   // MAX_MODELS = 4, MINIMUM_SAMPLES = 3
  if (bounded) {
    // maxThreshold = precision N(0,0)^2 with precision = Square(error_max) (SfM_Localizer.cpp:125-128, robust_estimator_ACRansac.hpp:351-353);
    // Histogram(0, maxThreshold, 20): nBins_by_interval and GetXbinsValue (histogram.hpp:49-61, :105-112); logalpha per bin value (:229-231)
    ResBound& b = c.h_bound<ResBound>()[p];
    b.max_threshold = error_max * error_max * g.n1 * g.n1;
    b.bins_by_interval = kBins / (b.max_threshold - 0.0);
    const double val = (b.max_threshold - 0.0) / static_cast<double>(kBins - 1);
    for (int k = 0; k < kBins; ++k) {
      b.bin_value[k] = val * static_cast<double>(k) + 0.0;
      b.logalpha_bin[k] = std::log10(M_PI) + 1.0 * std::log10(b.bin_value[k] + std::numeric_limits<float>::epsilon());
    }
  }
}

// Stream, events and device buffers; the uploads
int res_upload(ResCall& c, const double* x2d, const double* X3d) {
  int rc;
  if ((rc = mvgx::acquire_stream(&c.stream))) return rc;
  MVGX_HIP(hipGetDevice(&c.stream_device));
  MVGX_HIP(hipEventCreate(&c.e0));
  MVGX_HIP(hipEventCreate(&c.e1));
  const uint64_t n_total = c.n_total;
  if ((rc = c.d_stage.ensure((c.stage_words + 1) / 2)) || (rc = c.d_x2d.ensure(2 * n_total)) || (rc = c.d_X.ensure(3 * n_total)) || (rc = c.d_bear.ensure(3 * n_total)) ||
      (rc = c.d_scratch.ensure(std::max<size_t>(c.scratch_bytes, 1))) || (rc = c.d_res.ensure(c.n_problems)) || (rc = c.d_inl.ensure(n_total)) ||
      (rc = c.h_res.ensure(c.n_problems)))
    return rc;
  MVGX_HIP(hipMemcpyAsync(c.d_stage.p, c.stage.p, (c.stage_words + 1) / 2 * 8, hipMemcpyHostToDevice, c.stream));
  MVGX_HIP(hipMemcpyAsync(c.d_x2d.p, x2d + 2 * c.base, 2 * n_total * sizeof(double), hipMemcpyHostToDevice, c.stream));
  MVGX_HIP(hipMemcpyAsync(c.d_X.p, X3d + 3 * c.base, 3 * n_total * sizeof(double), hipMemcpyHostToDevice, c.stream));
  MVGX_HIP(hipMemsetAsync(c.d_res.p, 0, (size_t)c.n_problems * sizeof(ResResult), c.stream));
  return MVGX_OK;
}
// Test hook: this call takes the trace that mvgx_resection_debug_trace asked for (one call only)
int res_trace_setup(ResCall& c) {
  c.host_trace = g_res_trace;
  c.trace_events = c.host_trace ? g_res_trace_events : 0;
  g_res_trace = nullptr;
  c.trace_words = (size_t)c.n_problems * res_trace_words(c.trace_events);
  if (c.host_trace) {
    int rc;
    if ((rc = c.d_trace.ensure(c.trace_words))) return rc;
    MVGX_HIP(hipMemsetAsync(c.d_trace.p, 0, c.trace_words * sizeof(uint32_t), c.stream));
  }
  return MVGX_OK;
}
// The first event, then the prepare pass: one thread per correspondence, from x2d into d_bear
template <class Problem>
int res_prepare(ResCall& c, void (*kernel)(const Problem*, uint32_t, uint64_t, const double*, double*)) {
  const Problem* const p_prob = c.p_prob<Problem>();
  const double* const p_x2d = c.d_x2d.p;
  double* const p_out = c.d_bear.p;
  const uint32_t n_problems = c.n_problems;
  const uint64_t n_total = c.n_total;
  MVGX_HIP(hipEventRecord(c.e0, c.stream));
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, c.stream, p_prob, n_problems, n_total, p_x2d, p_out);
  MVGX_HIP(hipGetLastError());
  return MVGX_OK;
}

// A loop kernel's two launches: the problems of the LDS form, every workgroup with the LDS of the largest of them, then those of the
// global form. The kernels take (order, n_work, n_lds_max, args...).
template <class... Params, class... Args>
int res_launch_one(void (*kernel)(Params...), uint32_t n_work, uint32_t lds_bytes, hipStream_t stream, Args... args) {
  MVGX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL(kernel, dim3(n_work), dim3(64 * kResWaves), lds_bytes, stream, args...);
  MVGX_HIP(hipGetLastError());
  return MVGX_OK;
}
template <class... Params, class... Args>
int res_launch(ResCall& c, void (*kernel_lds)(Params...), void (*kernel_global)(Params...), uint32_t (*lds_bytes_of)(uint32_t), Args... args) {
  const uint32_t n_lds = (uint32_t)c.in_lds.size(), n_global = (uint32_t)c.in_global.size();
  int rc;
  if (n_lds && (rc = res_launch_one(kernel_lds, n_lds, lds_bytes_of(c.n_lds_max), c.stream, c.p_lists(), n_lds, c.n_lds_max, args...))) return rc;
  if (n_global && (rc = res_launch_one(kernel_global, n_global, lds_bytes_of(0), c.stream, c.p_lists() + n_lds, n_global, 0u, args...))) return rc;
  return MVGX_OK;
}

// R, t and the centre C = -R^T t into a problem's 15 doubles of out_pose
inline void res_write_pose(const double* R, const double* t, double* pose) {
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) pose[4 * i + j] = R[3 * i + j];
    pose[4 * i + 3] = t[i];
    pose[12 + i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
  }
}
// After the loop kernels: the second event, the results and the inlier lists back; per problem with more than 2.5 min_sample inliers
// write_model(p, record, result) leaves pose, P (and K). scale: the record's member that unormalizeError divides by.
template <class Problem, class WriteModel>
int res_finish(ResCall& c, uint32_t min_sample, double Problem::*scale, uint8_t* out_ok, double* out_error_max, double* out_min_nfa, uint64_t* out_inlier_start,
               uint32_t* out_inliers, mvgx_resection_stats* stats, std::chrono::steady_clock::time_point t_begin, WriteModel write_model) {
  const uint32_t n_problems = c.n_problems;
  const Problem* const hp = c.h_prob<Problem>();
  MVGX_HIP(hipEventRecord(c.e1, c.stream));
  MVGX_HIP(hipMemcpyAsync(c.h_res.p, c.d_res.p, (size_t)n_problems * sizeof(ResResult), hipMemcpyDeviceToHost, c.stream));
  // the inlier lists come back in place (one list per problem at its start), then are packed
  std::vector<uint32_t> inl(c.n_total);
  MVGX_HIP(hipMemcpyAsync(inl.data(), c.d_inl.p, c.n_total * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  if (c.host_trace) MVGX_HIP(hipMemcpyAsync(c.host_trace, c.d_trace.p, c.trace_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  MVGX_HIP(hipStreamSynchronize(c.stream));

  uint64_t at = 0, iterations = 0, n_models = 0;
  for (uint32_t p = 0; p < n_problems; ++p) {
    out_inlier_start[p] = at;
    const ResResult& r = c.h_res.p[p];
    if (hp[p].n <= min_sample) continue;   // ACRANSAC's early return of (0, 0): nothing else is written
    iterations += r.n_iterations; n_models += r.n_models;
    out_min_nfa[p] = r.min_nfa;
    out_error_max[p] = r.n_inliers ? std::sqrt(r.error_max) / (hp[p].*scale) : r.error_max;   // unormalizeError
    if (r.n_inliers) memcpy(out_inliers + at, inl.data() + hp[p].start, (size_t)r.n_inliers * sizeof(uint32_t));
    at += r.n_inliers;
    if ((double)r.n_inliers > 2.5 * min_sample) {
      write_model(p, hp[p], r);
      out_ok[p] = 1;
    }
  }
  out_inlier_start[n_problems] = at;
  if (stats) {
    float kernel_ms = 0.f;
    (void)hipEventElapsedTime(&kernel_ms, c.e0, c.e1);
    stats->n_problems = n_problems; stats->n_iterations = iterations; stats->n_models = n_models; stats->kernel_ms = kernel_ms;
    stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return MVGX_OK;
}

// What the two calibrated entries differ in: bounded, and with it the second table, the LDS bound and the kernel
int res_localize_calibrated(const char* entry, bool bounded, int device, uint32_t n_problems, const uint64_t* start, const double* x2d, const double* X3d,
                            const int32_t* intr_model, const double* intrinsics, const mvgx_resection_options* opt, uint8_t* out_ok, double* out_pose, double* out_P,
                            double* out_error_max, double* out_min_nfa, uint64_t* out_inlier_start, uint32_t* out_inliers, mvgx_resection_stats* stats) {
  const auto t_begin = std::chrono::steady_clock::now();
  ResCall c;
  c.entry = entry;
  int rc;
  bool work = false;
  if ((rc = res_check_arguments(c, bounded, n_problems, start, intr_model, intrinsics, opt, out_ok, out_pose, out_P, out_error_max, out_min_nfa, out_inlier_start))) return rc;
  if ((rc = res_classify(c, 3, start, x2d, X3d, out_inliers, opt->global_above, bounded ? kResBLdsMaxN : kResLdsMaxN, out_ok, out_error_max, out_min_nfa, out_inlier_start,
                         stats, &work)))
    return rc;
  if (!work) return MVGX_OK;
  if ((rc = mvgx::select_device(device < 0 ? -1 : device))) return rc;
  const double error_max = opt->error_max;
  if ((rc = res_stage<ResProblem>(c, start, bounded ? (size_t)n_problems * sizeof(ResBound) / 4 : 0,
                                  bounded ? &ResBLayout::scratch_bytes : &ResP3PForm::Layout::scratch_bytes,
                                  [&](uint32_t p, uint32_t n, ResProblem& g) { res_fill_calibrated(c, bounded, intr_model, intrinsics, error_max, p, n, g); })))
    return rc;
  if ((rc = res_upload(c, x2d, X3d))) return rc;
  if (!bounded && (rc = res_trace_setup(c))) return rc;   // (the bounded loop leaves no trace)
  if ((rc = res_prepare<ResProblem>(c, resection_bearing_kernel))) return rc;
  if (bounded)
    rc = res_launch(c, resection_acransac_bounded_kernel<false>, resection_acransac_bounded_kernel<true>, &ResBLayout::lds_bytes, c.p_prob<ResProblem>(),
                    c.p_bound<ResBound>(), c.d_x2d.p, c.d_X.p, c.d_bear.p, c.p_l10(), c.p_mt(), opt->max_iteration, opt->solver, opt->waves_ahead, c.d_scratch.p, c.d_res.p,
                    c.d_inl.p);
  else
    rc = res_launch(c, resection_acransac_kernel<ResP3PForm, false>, resection_acransac_kernel<ResP3PForm, true>, &ResP3PForm::Layout::lds_bytes, c.p_prob<ResProblem>(),
                    c.d_x2d.p, c.d_X.p, c.d_bear.p, c.p_l10(), c.p_mt(), opt->max_iteration, opt->solver, opt->waves_ahead, c.d_scratch.p, c.d_res.p, c.d_inl.p, c.p_trace(),
                    c.trace_events);
  if (rc) return rc;
  return res_finish<ResProblem>(c, 3, &ResProblem::n1, out_ok, out_error_max, out_min_nfa, out_inlier_start, out_inliers, stats, t_begin,
                                [&](uint32_t p, const ResProblem&, const ResResult& r) {
                                  double K[9], R[9], t[3];
                                  res_krt_from_p(r.P, K, R, t);
                                  res_write_pose(R, t, out_pose + 15 * (size_t)p);
                                  memcpy(out_P + 12 * (size_t)p, r.P, 12 * sizeof(double));
                                });
}

}  // namespace

extern "C" {

void mvgx_resection_default_options(mvgx_resection_options* o) {
  if (!o) return;
  // Image_Localizer_Match_Data's defaults (SfM_Localizer.hpp:28-37) and resection::SolverType::DEFAULT
  o->solver = MVGX_RESECTION_P3P_DING; o->max_iteration = 4096; o->error_max = std::numeric_limits<double>::infinity();
  o->waves_ahead = 0; o->global_above = 0;
}

int mvgx_resection_localize(int device, uint32_t n_problems, const uint64_t* start, const double* x2d, const double* X3d, const int32_t* intr_model,
                            const double* intrinsics, const mvgx_resection_options* opt, uint8_t* out_ok, double* out_pose, double* out_P,
                            double* out_error_max, double* out_min_nfa, uint64_t* out_inlier_start, uint32_t* out_inliers, mvgx_resection_stats* stats) {
  return res_localize_calibrated(__func__, /*bounded=*/false, device, n_problems, start, x2d, X3d, intr_model, intrinsics, opt, out_ok, out_pose, out_P, out_error_max,
                                 out_min_nfa, out_inlier_start, out_inliers, stats);
}

// The bounded form: opt->error_max is the bound in pixels (Image_Localizer_Match_Data::error_max on entry), finite and > 0. ACRANSAC then
// reads the NFA off a 20-bin histogram of the residuals below the bound, starts as a max-consensus loop with the rejection sampler and
// gives up after 2 (max_iteration / 10) + 2 iterations if no model has more than 2.5 x 3 residuals inside the bound. The inlier lists
// come back in ascending index order.
int mvgx_resection_localize_bounded(int device, uint32_t n_problems, const uint64_t* start, const double* x2d, const double* X3d, const int32_t* intr_model,
                                    const double* intrinsics, const mvgx_resection_options* opt, uint8_t* out_ok, double* out_pose, double* out_P,
                                    double* out_error_max, double* out_min_nfa, uint64_t* out_inlier_start, uint32_t* out_inliers, mvgx_resection_stats* stats) {
  return res_localize_calibrated(__func__, /*bounded=*/true, device, n_problems, start, x2d, X3d, intr_model, intrinsics, opt, out_ok, out_pose, out_P, out_error_max,
                                 out_min_nfa, out_inlier_start, out_inliers, stats);
}


// Test hook (not declared in include/mvgx.h): the NEXT mvgx_resection_localize call of this process leaves in `out`, per problem,
// 1 + 10 * events words: the number of iterations that found a better model, then per such iteration (the first `events` of them)
// iteration | k | the first 8 indices of its sorted list (0xffffffff beyond k). The order of a sample's own three points at the head of
// that list is rounding noise ("Resection"); with it the tests' restatement follows the device's sample sequence.
int mvgx_resection_debug_trace(uint32_t* out, uint32_t events) {
  g_res_trace = out;
  g_res_trace_events = out ? events : 0;
  return MVGX_OK;
}

// Test hook (not declared in include/mvgx.h): the minimal solvers alone, one lane per sample. bearings, X: n_samples x 3 x 3 doubles (three
// vectors per sample); Rt_out: n_samples x 4 x 12 ([R | t] row-major, zeros beyond n_out[i]); n_out: n_samples
int mvgx_resection_debug_p3p(int solver, const double* bearings, const double* X, uint32_t n_samples, double* Rt_out, int* n_out) {
  MVGX_REQUIRE(bearings && X && Rt_out && n_out, MVGX_ERR_ARG, "%s: NULL argument", __func__);
  MVGX_REQUIRE(solver == kResSolverDing || solver == kResSolverNordberg, MVGX_ERR_UNSUPPORTED, "%s: solver %d has no device path", __func__, solver);
  if (!n_samples) return MVGX_OK;
  int rc = mvgx::select_device(-1);
  if (rc) return rc;
  mvgx::DevBuf<double> db, dX, dR;
  mvgx::DevBuf<int> dn;
  if ((rc = db.ensure(9 * (size_t)n_samples)) || (rc = dX.ensure(9 * (size_t)n_samples)) || (rc = dR.ensure(48 * (size_t)n_samples)) || (rc = dn.ensure(n_samples))) return rc;
  MVGX_HIP(hipMemcpy(db.p, bearings, 9 * (size_t)n_samples * sizeof(double), hipMemcpyHostToDevice));
  MVGX_HIP(hipMemcpy(dX.p, X, 9 * (size_t)n_samples * sizeof(double), hipMemcpyHostToDevice));
  MVGX_HIP(hipMemset(dR.p, 0, 48 * (size_t)n_samples * sizeof(double)));
  MVGX_HIP(hipMemset(dn.p, 0, (size_t)n_samples * sizeof(int)));
  {
    const double *pb = db.p, *pX = dX.p;
    double* const pR = dR.p;
    int* const pn = dn.p;
    hipLaunchKernelGGL(resection_p3p_debug_kernel, dim3((n_samples + 63) / 64), dim3(64), 0, nullptr, solver, pb, pX, n_samples, pR, pn);
  }
  MVGX_HIP(hipGetLastError());
  MVGX_HIP(hipStreamSynchronize(nullptr));
  MVGX_HIP(hipMemcpy(Rt_out, dR.p, 48 * (size_t)n_samples * sizeof(double), hipMemcpyDeviceToHost));
  MVGX_HIP(hipMemcpy(n_out, dn.p, (size_t)n_samples * sizeof(int), hipMemcpyDeviceToHost));
  return MVGX_OK;
}

}  // extern "C"
