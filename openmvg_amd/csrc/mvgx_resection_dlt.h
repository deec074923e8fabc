// mvgx_resection_dlt.h - robust resection of a view WITHOUT intrinsics on the device: AC-RANSAC over the six-point DLT solver, a batch
// of independent problems per call (mvgx_resection_localize_uncalibrated). Included after mvgx_resection_loop.h and mvgx_resection.h,
// under the former's `#pragma clang fp contract(off)`. The loop is resection_acransac_kernel of mvgx_resection_loop.h, the host stages
// are the res_* functions of mvgx_resection.h; what is here is what the six-point form gives them: its problem record, its prepare
// pass, its solver, its residual (ResDltForm) and the unnormalisation of the winning model.
// What is restated here (paths under src/openMVG of the reference):
//   sfm/pipelines/localization/SfM_Localizer.cpp:134-161, :321-331                 the DLT_6POINTS branch of SfM_Localizer::Localize
//   robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:203-288         ACKernelAdaptorResection, UnnormalizerResection
//   multiview/conditioning.cpp:54-77                                               NormalizePoints(points, ..., width, height)
//   multiview/solver_resection_kernel.cpp:29-136                                   SixPointResectionSolver::Solve
//   multiview/solver_resection_metrics.hpp:28-39                                   SquaredPixelReprojectionError
//   multiview/projection.cpp:40-132, :192-194                                      KRt_From_P, Depth
// The solver is run by a wave as a whole: the null vector of the 12 x 12 design matrix by a one-sided (Hestenes) Jacobi iteration on
// its columns, six column pairs per step, eight lanes per pair ("Resection without intrinsics").
#pragma once

namespace {

constexpr int kDltSample = 6;                 // MINIMUM_SAMPLES; MAX_MODELS = 1
constexpr uint32_t kDltLdsMaxN = 1024;        // largest n whose sort slices and tables live in LDS (DESIGN.md derives it)
constexpr int kDltSweepCap = 30;              // sweeps after which a sample that has not converged yields no model (the fixture's samples need 6 to 10)
constexpr double kDltOrthTol = 1.7763568394002505e-15;   // 8 eps: columns with |a_p . a_q| <= tol |a_p| |a_q| count as orthogonal
constexpr double kDltRatioGate = 1e-5;        // solver_resection_kernel.cpp:110
// a wave's work area in doubles: [A; V] 24 x 12 | six pixels, six points | P | the squared column norms | ratio, sweeps
constexpr int kDltM = 0, kDltPix = 288, kDltPts = 300, kDltP = 318, kDltNorms = 330, kDltInfo = 342, kDltWork = 344;

struct DltProblem {       // per problem, prepared on the host (glibc's log10: the reference's value)
  uint64_t start;         // first correspondence, counted from the first problem's
  uint64_t scratch;       // global form: byte offset of the problem's scratch
  uint32_t n, pad_;
  double d_norm, off_x, off_y;   // N1: the scale and the two offsets (conditioning.cpp:54-62)
  double loge0;                  // log10(MAX_MODELS (n - 6))
};

// ---- prepare pass: the normalised pixel of every correspondence, once per problem (N1 (x, y, 1), the third coordinate exactly 1) ----
__global__ __launch_bounds__(256) void resection_dlt_normalize_kernel(const DltProblem* __restrict__ problems, uint32_t n_problems, uint64_t n_total,
                                                                      const double* __restrict__ x2d, double* __restrict__ xn) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_total) return;
  const DltProblem& P = res_problem_of(problems, n_problems, i);
  xn[2 * i] = add_rn(mul_rn(P.d_norm, x2d[2 * i]), P.off_x);
  xn[2 * i + 1] = add_rn(mul_rn(P.d_norm, x2d[2 * i + 1]), P.off_y);
}

// ---- the solver, by one wave ----
// KRt_From_P (projection.cpp:40-132; res_krt_from_p of mvgx_resection.h is the host's) and Depth(R, t, X) > 0 of the six points
__device__ __forceinline__ void dlt_mul3(const double* A, const double* B, double* C) {
  double T[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) T[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
  for (int e = 0; e < 9; ++e) C[e] = T[e];
}
__device__ __forceinline__ void dlt_rotate(double* K, double* Q, const double* Qr) {
  double Qt[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Qt[3 * i + j] = Qr[3 * j + i];
  dlt_mul3(K, Qr, K);
  dlt_mul3(Qt, Q, Q);
}
__device__ __forceinline__ bool dlt_in_front(const double* __restrict__ P, const double* __restrict__ pts) {
  double K[9], Q[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K[3 * i + j] = P[4 * i + j];
  if (K[7] != 0) {
    double c = -K[8], s = K[7];
    const double l = hypot(c, s);
    c /= l; s /= l;
    const double Qx[9] = {1, 0, 0, 0, c, -s, 0, s, c};
    dlt_rotate(K, Q, Qx);
  }
  if (K[6] != 0) {
    double c = K[8], s = K[6];
    const double l = hypot(c, s);
    c /= l; s /= l;
    const double Qy[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
    dlt_rotate(K, Q, Qy);
  }
  if (K[3] != 0) {
    double c = -K[4], s = K[3];
    const double l = hypot(c, s);
    c /= l; s /= l;
    const double Qz[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
    dlt_rotate(K, Q, Qz);
  }
  double* const R = Q;
  if (K[8] < 0)
    for (int e = 0; e < 9; ++e) { K[e] = -K[e]; R[e] = -R[e]; }
  if (K[4] < 0) {
    const double S[9] = {1, 0, 0, 0, -1, 0, 0, 0, 1};
    dlt_mul3(K, S, K);
    dlt_mul3(S, R, R);
  }
  if (K[0] < 0) {
    const double S[9] = {-1, 0, 0, 0, 1, 0, 0, 0, 1};
    dlt_mul3(K, S, K);
    dlt_mul3(S, R, R);
  }
  // t = K^-1 p4 by elimination with partial pivoting (Eigen::PartialPivLU); Depth reads t(2) alone. The three rows are named, so that
  // no array is indexed by the pivot (which would put it into scratch memory).
  double a0[4] = {K[0], K[1], K[2], P[3]}, a1[4] = {K[3], K[4], K[5], P[7]}, a2[4] = {K[6], K[7], K[8], P[11]};
  const auto swap_rows = [](double* x, double* y) {
    for (int e = 0; e < 4; ++e) { const double v = x[e]; x[e] = y[e]; y[e] = v; }
  };
  {
    const bool one = fabs(a1[0]) > fabs(a0[0]);
    const bool two = fabs(a2[0]) > (one ? fabs(a1[0]) : fabs(a0[0]));
    if (two) swap_rows(a0, a2); else if (one) swap_rows(a0, a1);
    const double f1 = a1[0] / a0[0], f2 = a2[0] / a0[0];
    for (int e = 0; e < 4; ++e) { a1[e] -= f1 * a0[e]; a2[e] -= f2 * a0[e]; }
    if (fabs(a2[1]) > fabs(a1[1])) swap_rows(a1, a2);
    const double f = a2[1] / a1[1];
    for (int e = 1; e < 4; ++e) a2[e] -= f * a1[e];
  }
  double t2 = a2[3] / a2[2];
  const double det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) + R[2] * (R[3] * R[7] - R[4] * R[6]);
  double r20 = R[6], r21 = R[7], r22 = R[8];
  if (det < 0) { r20 = -r20; r21 = -r21; r22 = -r22; t2 = -t2; }
  int front = 0;
  for (int i = 0; i < kDltSample; ++i) front += (r20 * pts[3 * i] + r21 * pts[3 * i + 1] + r22 * pts[3 * i + 2]) + t2 > 0 ? 1 : 0;
  return front == kDltSample;
}

// SixPointResectionSolver::Solve(pt2D, pt3d, &Ps, bcheck = true) by the 64 lanes of one wave. work: the wave's area, its six normalised
// pixels at kDltPix and six points at kDltPts (visible to the wave). Returns the number of models (0 or 1, the same in every lane) and
// leaves P at kDltP, the ratio of the second smallest to the largest singular value and the sweeps used at kDltInfo.
//   [A; V], 24 x 12 row-major: A's twelve normalised rows over V = I. A step of a sweep takes the six disjoint column pairs of one round
//   of a tournament of twelve; pair g belongs to lanes 8 g .. 8 g + 7, lane j of them owns rows j, j + 8 and j + 16 of both columns: the
//   three sums over A's rows are reduced across the eight lanes (every lane gets the same bits), the rotation is applied to the owned
//   rows. A^T A is never formed. A sweep without a rotation ends the iteration; after kDltSweepCap sweeps the sample yields no model.
__device__ __forceinline__ int dlt_solve(double* __restrict__ work, int lane) {
  double* const M = work + kDltM;
  const double* const pix = work + kDltPix;
  const double* const pts = work + kDltPts;
  if (lane < 12) {
    const int i = lane >> 1;
    const double X = pts[3 * i] - pts[0], Y = pts[3 * i + 1] - pts[1], Z = pts[3 * i + 2] - pts[2];   // translated by -X0
    const double x = pix[2 * i + (lane & 1)];
    const double h[4] = {X, Y, Z, 1.0};
    double row[12];
    for (int e = 0; e < 4; ++e) {
      row[e] = (lane & 1) ? 0.0 : h[e];
      row[4 + e] = (lane & 1) ? h[e] : 0.0;
      row[8 + e] = -x * h[e];
    }
    double n2 = 0.0;
    for (int e = 0; e < 12; ++e) n2 += row[e] * row[e];
    const double nrm = sqrt(n2);
    for (int e = 0; e < 12; ++e) M[12 * lane + e] = n2 > 0.0 ? row[e] / nrm : row[e];
  } else if (lane < 24) {
    for (int e = 0; e < 12; ++e) M[12 * lane + e] = (e == lane - 12) ? 1.0 : 0.0;
  }
  wave_sync();

  const int g = lane >> 3, j = lane & 7;
  int sweeps = 0;
  bool converged = false;
  for (int sweep = 0; sweep < kDltSweepCap; ++sweep) {
    bool rotated = false;
    for (int k = 0; k < 11; ++k) {
      // round k of the tournament: 11 meets k; (k + g) mod 11 meets (k - g) mod 11
      int p = 11, q = k;
      if (g > 0) { p = (k + g) % 11; q = (k + 11 - g) % 11; }
      if (p > q) { const int s = p; p = q; q = s; }
      double a0p = 0, a0q = 0, a1p = 0, a1q = 0, a2p = 0, a2q = 0;
      double al = 0.0, be = 0.0, ga = 0.0;
      if (g < 6) {
        a0p = M[12 * j + p]; a0q = M[12 * j + q];
        a1p = M[12 * (j + 8) + p]; a1q = M[12 * (j + 8) + q];
        a2p = M[12 * (j + 16) + p]; a2q = M[12 * (j + 16) + q];
        al = a0p * a0p; be = a0q * a0q; ga = a0p * a0q;
        if (j < 4) { al += a1p * a1p; be += a1q * a1q; ga += a1p * a1q; }   // rows 8 .. 11 are A's, rows 12 .. 23 are V's
      }
      for (int d = 1; d < 8; d <<= 1) {
        al += __shfl_xor(al, d); be += __shfl_xor(be, d); ga += __shfl_xor(ga, d);
      }
      if (g < 6 && fabs(ga) > kDltOrthTol * sqrt(al * be)) {
        const double zeta = (be - al) / (2.0 * ga);
        const double t = (zeta < 0 ? -1.0 : 1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        M[12 * j + p] = c * a0p - s * a0q; M[12 * j + q] = s * a0p + c * a0q;
        M[12 * (j + 8) + p] = c * a1p - s * a1q; M[12 * (j + 8) + q] = s * a1p + c * a1q;
        M[12 * (j + 16) + p] = c * a2p - s * a2q; M[12 * (j + 16) + q] = s * a2p + c * a2q;
        rotated = true;
      }
      wave_sync();
    }
    ++sweeps;
    if (__ballot(rotated) == 0) { converged = true; break; }
  }

  // the singular values are the norms of A's columns: the largest, the smallest (its column of V is the null vector) and the second smallest
  if (lane < 12) {
    double n2 = 0.0;
    for (int r = 0; r < 12; ++r) n2 += M[12 * r + lane] * M[12 * r + lane];
    work[kDltNorms + lane] = n2;
  }
  wave_sync();
  double n_max = work[kDltNorms], n_min = n_max, n_second = INFINITY;
  int c_min = 0;
  for (int c = 1; c < 12; ++c) {
    const double v = work[kDltNorms + c];
    if (v > n_max) n_max = v;
    if (v < n_min) { n_second = n_min; n_min = v; c_min = c; }
    else if (v < n_second) n_second = v;
  }
  const double ratio = sqrt(n_second) / sqrt(n_max);
  int count = 0;
  if (converged && ratio > kDltRatioGate) count = 1;   // (a NaN fails the gate)
  if (lane == 0) {
    double P[12];
    for (int e = 0; e < 12; ++e) P[e] = M[12 * (12 + e) + c_min];   // Map<Mat>(p, 4, 3).transpose(): row-major 3 x 4
    if (count) {
      const double t0 = -pts[0], t1 = -pts[1], t2 = -pts[2];
      for (int r = 0; r < 3; ++r) P[4 * r + 3] = ((P[4 * r] * t0 + P[4 * r + 1] * t1) + P[4 * r + 2] * t2) + P[4 * r + 3];   // P [I | -X0; 0 1]
      const double w = P[11];
      for (int e = 0; e < 12; ++e) P[e] /= w;
      if (!dlt_in_front(P, pts)) count = 0;
    }
    for (int e = 0; e < 12; ++e) work[kDltP + e] = count ? P[e] : 0.0;
    work[kDltInfo] = ratio;
    work[kDltInfo + 1] = (double)sweeps;
  }
  wave_sync();
  return __shfl(count, 0);
}

// Test hook: one wave per sample. xn: n x 6 x 2 normalised pixels, X: n x 6 x 3; P_out n x 12, info_out n x 2 (ratio | sweeps)
__global__ __launch_bounds__(64) void resection_dlt6_debug_kernel(const double* __restrict__ xn, const double* __restrict__ X, uint32_t n_samples,
                                                                  double* __restrict__ P_out, double* __restrict__ info_out, int* __restrict__ n_out) {
  __shared__ double work[kDltWork];
  const uint32_t i = blockIdx.x;
  const int lane = threadIdx.x;
  if (i >= n_samples) return;
  if (lane < 12) work[kDltPix + lane] = xn[12 * (size_t)i + lane];
  if (lane < 18) work[kDltPts + lane] = X[18 * (size_t)i + lane];
  wave_sync();
  const int count = dlt_solve(work, lane);
  if (lane < 12) P_out[12 * (size_t)i + lane] = work[kDltP + lane];
  if (lane < 2) info_out[2 * (size_t)i + lane] = work[kDltInfo + lane];
  if (lane == 0) n_out[i] = count;
}

// ---- what the six-point solver gives the exhaustive loop of mvgx_resection_loop.h ----
struct ResDltForm {
  using Problem = DltProblem;
  using Layout = ResLayout<kDltSample, kResVerdict, kDltWork, 0, true>;
  static constexpr int kSample = kDltSample, kMaxModels = 1, kModelAt = kDltP;
  const double2* px;   // the normalised pixels of the prepare pass
  const double* pX;
  __device__ __forceinline__ ResDltForm(const DltProblem& P, const double* __restrict__, const double* __restrict__ X3d, const double* __restrict__ xn, int)
      : px(reinterpret_cast<const double2*>(xn) + P.start), pX(X3d + 3 * P.start) {}
  __device__ __forceinline__ void load_sample(const uint32_t* sample, double* work, double*, int lane) const {
    if (lane < kDltSample) {
      const uint32_t s = sample[lane];
      const double2 obs = px[s];
      work[kDltPix + 2 * lane] = obs.x; work[kDltPix + 2 * lane + 1] = obs.y;
      work[kDltPts + 3 * lane] = pX[3 * s]; work[kDltPts + 3 * lane + 1] = pX[3 * s + 1]; work[kDltPts + 3 * lane + 2] = pX[3 * s + 2];
    }
  }
  __device__ __forceinline__ int solve(double* work, const double*, uint32_t*, int lane) const { return dlt_solve(work, lane); }
  // | x - hnormalized(P (X, 1)) |^2 in normalised pixels
  __device__ __forceinline__ double residual(const ResRt& M, uint32_t i) const {
    const double X = pX[3 * i], Y = pX[3 * i + 1], Z = pX[3 * i + 2];
    const double u = add_rn(add_rn(add_rn(mul_rn(M.m0, X), mul_rn(M.m1, Y)), mul_rn(M.m2, Z)), M.m3);
    const double v = add_rn(add_rn(add_rn(mul_rn(M.m4, X), mul_rn(M.m5, Y)), mul_rn(M.m6, Z)), M.m7);
    const double w = add_rn(add_rn(add_rn(mul_rn(M.m8, X), mul_rn(M.m9, Y)), mul_rn(M.m10, Z)), M.m11);
    const double2 obs = px[i];
    const double rx = add_rn(obs.x, -(u / w)), ry = add_rn(obs.y, -(v / w));
    return add_rn(mul_rn(rx, rx), mul_rn(ry, ry));
  }
};
static_assert(4 * ResDltForm::Layout::words(kDltLdsMaxN) <= 160 * 1024, "the LDS form must fit a workgroup's 160 KiB");

}  // namespace

extern "C" {

// SfM_Localizer::Localize for a view WITHOUT intrinsics (resection::SolverType::DLT_6POINTS, error_max = infinity); include/mvgx.h
int mvgx_resection_localize_uncalibrated(int device, uint32_t n_problems, const uint64_t* start, const double* x2d, const double* X3d, const uint32_t* image_wh,
                                         const mvgx_resection_options* opt, uint8_t* out_ok, double* out_pose, double* out_P, double* out_K, double* out_error_max,
                                         double* out_min_nfa, uint64_t* out_inlier_start, uint32_t* out_inliers, mvgx_resection_stats* stats) {
  const auto t_begin = std::chrono::steady_clock::now();
  const char* const fn = __func__;
  ResCall c;
  c.entry = fn;
  int rc;
  bool work = false;
  MVGX_REQUIRE(opt && start && out_ok && out_pose && out_P && out_K && out_error_max && out_min_nfa && out_inlier_start, MVGX_ERR_ARG, "%s: NULL argument", fn);
  MVGX_REQUIRE(n_problems == 0 || image_wh, MVGX_ERR_ARG, "%s: NULL image sizes", fn);
  MVGX_REQUIRE(opt->solver == MVGX_RESECTION_DLT_6POINTS, MVGX_ERR_ARG,
               "%s: solver %d: this entry runs DLT_6POINTS = 0 alone (the calibrated solvers are mvgx_resection_localize's)", fn, opt->solver);
  MVGX_REQUIRE(!std::isfinite(opt->error_max), MVGX_ERR_UNSUPPORTED,
               "%s: a finite error_max selects the quantified NFA with the max-consensus early exit, which the six-point loop has no device path for", fn);
  MVGX_REQUIRE(std::isinf(opt->error_max) && opt->error_max > 0, MVGX_ERR_ARG, "%s: error_max must be +infinity", fn);
  if ((rc = res_check_batch(c, n_problems, start, opt, [&](uint32_t p) -> int {
         const uint64_t w = image_wh[2 * p], h = image_wh[2 * p + 1];
         MVGX_REQUIRE(w > 0 && h > 0 && w * h <= 0x7fffffffull, MVGX_ERR_ARG, "%s: problem %u: image size %llu x %llu (both must be > 0, their product an int)", fn, p,
                      (unsigned long long)w, (unsigned long long)h);
         return MVGX_OK;
       })))
    return rc;
  if ((rc = res_classify(c, kDltSample, start, x2d, X3d, out_inliers, opt->global_above, kDltLdsMaxN, out_ok, out_error_max, out_min_nfa, out_inlier_start, stats, &work)))
    return rc;
  if (!work) return MVGX_OK;
  if ((rc = mvgx::select_device(device < 0 ? -1 : device))) return rc;
  if ((rc = res_stage<DltProblem>(c, start, 0, &ResDltForm::Layout::scratch_bytes, [&](uint32_t p, uint32_t n, DltProblem& g) {
         const int width = (int)image_wh[2 * p], height = (int)image_wh[2 * p + 1];
         g.pad_ = 0;
         // PreconditionerFromPoints(width, height, &T) (conditioning.cpp:54-62): the x offset goes through a float product (-.5f * width)
         g.d_norm = 1.0 / std::sqrt(static_cast<double>(width * height));
         g.off_x = -.5f * width * g.d_norm;
         g.off_y = -.5 * height * g.d_norm;
         g.loge0 = n > (uint32_t)kDltSample ? std::log10((double)(n - kDltSample)) : 0.0;   // MAX_MODELS = 1, MINIMUM_SAMPLES = 6
       })))
    return rc;
  if ((rc = res_upload(c, x2d, X3d))) return rc;
  if ((rc = res_trace_setup(c))) return rc;
  if ((rc = res_prepare<DltProblem>(c, resection_dlt_normalize_kernel))) return rc;
  if ((rc = res_launch(c, resection_acransac_kernel<ResDltForm, false>, resection_acransac_kernel<ResDltForm, true>, &ResDltForm::Layout::lds_bytes, c.p_prob<DltProblem>(),
                       c.d_x2d.p, c.d_X.p, c.d_bear.p, c.p_l10(), c.p_mt(), opt->max_iteration, opt->solver, opt->waves_ahead, c.d_scratch.p, c.d_res.p, c.d_inl.p, c.p_trace(),
                       c.trace_events)))
    return rc;
  return res_finish<DltProblem>(c, kDltSample, &DltProblem::d_norm, out_ok, out_error_max, out_min_nfa, out_inlier_start, out_inliers, stats, t_begin,
                                [&](uint32_t p, const DltProblem& g, const ResResult& r) {
                                  // UnnormalizerResection: N1^-1 P, the inverse as Eigen's PartialPivLU of the dynamic matrix forms it (back substitution of I)
                                  const double d = g.d_norm;
                                  const double i00 = 1.0 / d, i02 = (0.0 - g.off_x * 1.0) / d, i12 = (0.0 - g.off_y * 1.0) / d;
                                  double* const Pu = out_P + 12 * (size_t)p;
                                  for (int e = 0; e < 4; ++e) {
                                    Pu[e] = i00 * r.P[e] + i02 * r.P[8 + e];
                                    Pu[4 + e] = i00 * r.P[4 + e] + i12 * r.P[8 + e];
                                    Pu[8 + e] = r.P[8 + e];
                                  }
                                  double R[9], t[3];
                                  res_krt_from_p(Pu, out_K + 9 * (size_t)p, R, t);
                                  res_write_pose(R, t, out_pose + 15 * (size_t)p);
                                });
}

// Test hook (not declared in include/mvgx.h): the six-point solver alone, one wave per sample. x_norm: n_samples x 6 x 2 NORMALISED
// pixels, X: n_samples x 6 x 3; P_out: n_samples x 12 (the normalised-space P, zeros without a model), info_out: n_samples x 2 (the ratio
// of the second smallest to the largest singular value | sweeps used), n_out: n_samples (0 or 1)
int mvgx_resection_debug_dlt6(const double* x_norm, const double* X, uint32_t n_samples, double* P_out, double* info_out, int* n_out) {
  MVGX_REQUIRE(x_norm && X && P_out && info_out && n_out, MVGX_ERR_ARG, "%s: NULL argument", __func__);
  if (!n_samples) return MVGX_OK;
  int rc = mvgx::select_device(-1);
  if (rc) return rc;
  mvgx::DevBuf<double> dx, dX, dP, di;
  mvgx::DevBuf<int> dn;
  if ((rc = dx.ensure(12 * (size_t)n_samples)) || (rc = dX.ensure(18 * (size_t)n_samples)) || (rc = dP.ensure(12 * (size_t)n_samples)) ||
      (rc = di.ensure(2 * (size_t)n_samples)) || (rc = dn.ensure(n_samples)))
    return rc;
  MVGX_HIP(hipMemcpy(dx.p, x_norm, 12 * (size_t)n_samples * sizeof(double), hipMemcpyHostToDevice));
  MVGX_HIP(hipMemcpy(dX.p, X, 18 * (size_t)n_samples * sizeof(double), hipMemcpyHostToDevice));
  {
    const double *px = dx.p, *pX = dX.p;
    double *const pP = dP.p, *const pi = di.p;
    int* const pn = dn.p;
    hipLaunchKernelGGL(resection_dlt6_debug_kernel, dim3(n_samples), dim3(64), 0, nullptr, px, pX, n_samples, pP, pi, pn);
  }
  MVGX_HIP(hipGetLastError());
  MVGX_HIP(hipStreamSynchronize(nullptr));
  MVGX_HIP(hipMemcpy(P_out, dP.p, 12 * (size_t)n_samples * sizeof(double), hipMemcpyDeviceToHost));
  MVGX_HIP(hipMemcpy(info_out, di.p, 2 * (size_t)n_samples * sizeof(double), hipMemcpyDeviceToHost));
  MVGX_HIP(hipMemcpy(n_out, dn.p, (size_t)n_samples * sizeof(int), hipMemcpyDeviceToHost));
  return MVGX_OK;
}

}  // extern "C"
