// mvgx_resection_dlt.h - robust resection of a view WITHOUT intrinsics on the device: AC-RANSAC over the six-point DLT solver, a batch
// of independent problems per call (mvgx_resection_localize_uncalibrated). Included after mvgx_resection.h, under that header's
// `#pragma clang fp contract(off)`: it uses its sort, table layout, verdict and trace records, result struct, KRt_From_P on the host and
// the generator, logcombi and un-contracted mul_rn / add_rn of mvgx_geofilter.hip.
// What is restated (paths under src/openMVG of the reference):
//   sfm/pipelines/localization/SfM_Localizer.cpp:134-161, :321-331                 the DLT_6POINTS branch of SfM_Localizer::Localize
//   robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:203-288         ACKernelAdaptorResection, UnnormalizerResection
//   robust_estimation/robust_estimator_ACRansac.hpp:257-304, :326-489              the exhaustive NFA, the a-contrario loop
//   robust_estimation/rand_sampling.hpp:71-100                                     UniformSample on the pool (six swaps at its head)
//   multiview/conditioning.cpp:54-77                                               NormalizePoints(points, ..., width, height)
//   multiview/solver_resection_kernel.cpp:29-136                                   SixPointResectionSolver::Solve
//   multiview/solver_resection_metrics.hpp:28-39                                   SquaredPixelReprojectionError
//   multiview/projection.cpp:40-132, :192-194                                      KRt_From_P, Depth
// Mapping: the loop's of mvgx_resection.h - one workgroup per problem, one wave per iteration evaluated ahead, verdicts read in iteration
// order. What is new is the solver, which a wave runs as a whole: the null vector of the 12 x 12 design matrix by a one-sided (Hestenes)
// Jacobi iteration on its columns, six column pairs per step, eight lanes per pair ("Resection without intrinsics").
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
  uint32_t lo = 0, hi = n_problems - 1;   // the last problem that starts at or before i and is not empty there
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (problems[mid].start <= i) lo = mid; else hi = mid - 1;
  }
  const DltProblem& P = problems[lo];
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

// ---- the loop ----
// words of LDS a workgroup needs: generator | its copy | verdicts | work areas | samples, swaps, counts | best model | (LDS form) pool,
// inliers, logc_n, logc_k, slices
__host__ __device__ constexpr uint32_t dlt_fixed_words() { return 2 * kMtN + 2 * kResWaves * kResVerdict + 2 * kResWaves * kDltWork + 16 * kResWaves + 24; }
inline uint32_t dlt_lds_bytes(uint32_t n_lds_max) { return 4 * (dlt_fixed_words() + (n_lds_max ? res_table_words(n_lds_max) + kResWaves * res_slice_words(res_pow2(n_lds_max)) : 0)); }
static_assert(4 * (dlt_fixed_words() + res_table_words(kDltLdsMaxN) + kResWaves * res_slice_words(kDltLdsMaxN)) <= 160 * 1024, "the LDS form must fit a workgroup's 160 KiB");

template <bool kGlobal>
__global__ __launch_bounds__(64 * kResWaves) void resection_dlt_acransac_kernel(const DltProblem* __restrict__ problems, const uint32_t* __restrict__ order, uint32_t n_work,
                                                                                const double* __restrict__ xn, const double* __restrict__ X3d,
                                                                                const float* __restrict__ l10, const uint32_t* __restrict__ mt_init, uint32_t max_iteration,
                                                                                uint32_t waves_ahead, uint32_t n_lds_max, unsigned char* __restrict__ scratch,
                                                                                ResResult* __restrict__ results, uint32_t* __restrict__ inliers_out, uint32_t* __restrict__ trace, uint32_t trace_events) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_u32[];
  if (blockIdx.x >= n_work) return;
  const uint32_t pi = order[blockIdx.x];
  const DltProblem& P = problems[pi];
  const uint32_t n = P.n, p2 = res_pow2(n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_threads = 64 * kResWaves;

  uint32_t* const mt = lds_u32;
  uint32_t* const mt_saved = mt + kMtN;
  double* const verdicts = reinterpret_cast<double*>(mt_saved + kMtN);
  double* const works = verdicts + kResWaves * kResVerdict;            // kDltWork doubles per wave
  uint32_t* const samples = reinterpret_cast<uint32_t*>(works + kResWaves * kDltWork);   // 6 per wave | swap partners, 6 per wave | models per wave
  uint32_t* const swaps = samples + kDltSample * kResWaves;
  uint32_t* const n_mod = swaps + kDltSample * kResWaves;
  double* const best_model = reinterpret_cast<double*>(samples + 16 * kResWaves);   // the winning P (thread 0 writes and reads it)
  uint32_t* const tables = kGlobal ? reinterpret_cast<uint32_t*>(scratch + P.scratch) : lds_u32 + dlt_fixed_words();
  const uint32_t n1 = n + 1;
  uint32_t* const pool = tables;
  uint32_t* const inliers = pool + n1;
  float* const logc_n = reinterpret_cast<float*>(inliers + n1);
  float* const logc_k = logc_n + n1;
  uint32_t* const slices = tables + res_table_words(kGlobal ? n : n_lds_max);
  const uint32_t slice_words = res_slice_words(kGlobal ? p2 : res_pow2(n_lds_max));   // LDS form: every wave's slice is sized for the launch's largest problem
  uint64_t* const my_keys = reinterpret_cast<uint64_t*>(slices + (size_t)wave * slice_words);
  uint32_t* const my_idx = reinterpret_cast<uint32_t*>(my_keys + p2);

  const double2* const px = reinterpret_cast<const double2*>(xn) + P.start;
  const double* const pX = X3d + 3 * P.start;
  const double loge0 = P.loge0;
  const double logalpha0 = 0.49714987269413385;   // log10(M_PI)

  // tables and generator
  for (uint32_t k = tid; k <= n; k += n_threads) {
    pool[k] = k;
    logc_k[k] = logcombi(kDltSample, k, l10);
  }
  if (tid == 0) {   // logc_n[k] = logcombi(k, n): the running float sum, then the mirror (as in the P3P loop)
    float r = 0.f;
    logc_n[0] = 0.f;
    for (uint32_t i = 1; i <= n / 2; ++i) { r += l10[n - i + 1] - l10[i]; logc_n[i] = r; }
  }
  __syncthreads();
  for (uint32_t k = n / 2 + 1 + tid; k <= n; k += n_threads) logc_n[k] = k >= n ? 0.f : logc_n[n - k];
  for (int i = tid; i < kMtN; i += n_threads) mt[i] = mt_init[i];
  int mt_idx = kMtN, mt_idx_saved = kMtN;   // (tracked by wave 0 alone)
  __syncthreads();

  const uint32_t Wa = waves_ahead ? waves_ahead : (uint32_t)kResWaves;
  double minNFA = INFINITY, errorMax = INFINITY;
  if (tid == 0)
    for (int e = 0; e < 12; ++e) best_model[e] = 0.0;
  uint32_t n_inl = 0, pool_n = n;
  int nIterReserve = (int)(max_iteration / 10);
  uint32_t nIter = max_iteration - (uint32_t)nIterReserve;
  uint32_t iter = 0, n_models_total = 0;

  while (iter < nIter && iter < max_iteration) {
    const uint32_t nb = min(Wa, min(nIter - iter, max_iteration - iter));
    // ---- the samples of the block, drawn in iteration order from the one generator (wave 0) ----
    if (wave == 0) {
      for (int i = lane; i < kMtN; i += 64) mt_saved[i] = mt[i];   // (a twist cannot be taken back: the state before the block is kept)
      wave_sync();
      mt_idx_saved = mt_idx;
      for (uint32_t j = 0; j < nb; ++j) {
        for (uint32_t i = 0; i < (uint32_t)kDltSample; ++i) {
          const uint32_t r = uniform_u32(mt, mt_idx, lane, i, pool_n - 1);
          if (lane == 0) {   // (lane 0 alone reads and writes the pool here)
            const uint32_t a = pool[i], b = pool[r];
            pool[i] = b; pool[r] = a;
            swaps[kDltSample * j + i] = r;
          }
        }
        if (lane == 0)
          for (int i = 0; i < kDltSample; ++i) samples[kDltSample * j + i] = pool[i];
      }
    }
    __syncthreads();

    // ---- one wave, one iteration ----
    if ((uint32_t)wave < nb) {
      double* const work = works + kDltWork * wave;
      double* const my_verdict = verdicts + kResVerdict * wave;
      if (lane < kDltSample) {
        const uint32_t s = samples[kDltSample * wave + lane];
        const double2 obs = px[s];
        work[kDltPix + 2 * lane] = obs.x; work[kDltPix + 2 * lane + 1] = obs.y;
        work[kDltPts + 3 * lane] = pX[3 * s]; work[kDltPts + 3 * lane + 1] = pX[3 * s + 1]; work[kDltPts + 3 * lane + 2] = pX[3 * s + 2];
      }
      wave_sync();
      const int nm = dlt_solve(work, lane);
      const double* const M = work + kDltP;
      double run_min = minNFA, win_err = 0.0;
      bool winner = false;
      uint32_t win_k = 0, evaluated = 0;
      const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5], m6 = M[6], m7 = M[7], m8 = M[8], m9 = M[9], m10 = M[10], m11 = M[11];
      // a model with a non-finite entry is skipped (the reference would sort NaNs: undefined)
      const double probe = m0 + m1 + m2 + m3 + m4 + m5 + m6 + m7 + m8 + m9 + m10 + m11;
      if (nm > 0 && fabs(probe) < INFINITY) {
        for (uint32_t i = lane; i < p2; i += 64) {
          double e = INFINITY;
          if (i < n) {
            // | x - hnormalized(P (X, 1)) |^2 in normalised pixels
            const double X = pX[3 * i], Y = pX[3 * i + 1], Z = pX[3 * i + 2];
            const double u = add_rn(add_rn(add_rn(mul_rn(m0, X), mul_rn(m1, Y)), mul_rn(m2, Z)), m3);
            const double v = add_rn(add_rn(add_rn(mul_rn(m4, X), mul_rn(m5, Y)), mul_rn(m6, Z)), m7);
            const double w = add_rn(add_rn(add_rn(mul_rn(m8, X), mul_rn(m9, Y)), mul_rn(m10, Z)), m11);
            const double2 obs = px[i];
            const double rx = add_rn(obs.x, -(u / w)), ry = add_rn(obs.y, -(v / w));
            e = add_rn(mul_rn(rx, rx), mul_rn(ry, ry));
            if (!(e < INFINITY)) e = INFINITY;   // NaN too
          }
          my_keys[i] = (uint64_t)__double_as_longlong(e);
          my_idx[i] = i;
        }
        wave_sync();
        res_sort(my_keys, my_idx, p2, lane);
        ++evaluated;
        // NFA(k) for every k in [7, n]: the smallest, the lowest k among equals
        double best = INFINITY;
        uint32_t best_k = kDltSample;
        for (uint32_t k = kDltSample + 1 + lane; k <= n; k += 64) {
          const double r = __longlong_as_double((long long)my_keys[k - 1]);
          const double logalpha = add_rn(logalpha0, log10(add_rn(r, kResFltEps)));
          const double nfa = add_rn(add_rn(add_rn(loge0, mul_rn(logalpha, (double)(k - kDltSample))), (double)logc_n[k]), (double)logc_k[k]);
          if (nfa < best) { best = nfa; best_k = k; }
        }
        for (int d = 32; d > 0; d >>= 1) {
          const double o = __shfl_xor(best, d);
          const uint32_t ok = (uint32_t)__shfl_xor((int)best_k, d);
          if (o < best || (o == best && ok < best_k)) { best = o; best_k = ok; }
        }
        if (best < run_min) {
          run_min = best; winner = true; win_k = best_k;
          win_err = __longlong_as_double((long long)my_keys[best_k - 1]);
        }
      }
      wave_sync();
      if (lane == 0) {
        my_verdict[0] = winner ? 1.0 : 0.0;
        my_verdict[1] = run_min; my_verdict[2] = (double)win_k; my_verdict[3] = win_err;
        for (int e = 0; e < 12; ++e) my_verdict[4 + e] = M[e];
        my_verdict[16] = (double)evaluated;
      }
    }
    __syncthreads();

    // ---- the verdicts in iteration order: the first event is applied, what follows it is void ----
    uint32_t done = nb;
    bool event = false;
    for (uint32_t j = 0; j < nb && !event; ++j) {
      const double* const v = verdicts + kResVerdict * j;
      n_models_total += (uint32_t)v[16];
      const bool better = v[0] != 0.0;   // (evaluated under the block's minNFA, which no earlier verdict of the block has changed)
      if (better) {
        minNFA = v[1]; errorMax = v[3]; n_inl = (uint32_t)v[2];
        if (tid == 0)
          for (int e = 0; e < 12; ++e) best_model[e] = v[4 + e];
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint64_t*>(slices + (size_t)j * slice_words) + p2);
        for (uint32_t i = tid; i < n_inl; i += n_threads) inliers[i] = src[i];
        if (trace && tid == 0) {   // test hook: iteration | k | the head of the sorted list, one record per iteration that found a better model
          uint32_t* const T = trace + (size_t)pi * res_trace_words(trace_events);
          const uint32_t at = T[0];
          if (at < trace_events) {
            uint32_t* const rec = T + 1 + (size_t)kResTraceRecord * at;
            rec[0] = iter + j; rec[1] = n_inl;
            for (uint32_t i = 0; i < (uint32_t)kResTraceRecord - 2; ++i) rec[2 + i] = i < n_inl ? src[i] : 0xffffffffu;
          }
          T[0] = at + 1;
        }
      }
      const bool branch = (better && minNFA < 0) || ((iter + j + 1) == nIter && nIterReserve > 0);
      bool take_pool = false;
      if (branch) {
        if (n_inl == 0) { ++nIter; --nIterReserve; }
        else {
          take_pool = true;
          if (nIterReserve) { nIter = iter + j + 1 + (uint32_t)nIterReserve; nIterReserve = 0; }
        }
      }
      if (better || branch) {
        event = true;
        done = j + 1;
        __syncthreads();   // the inlier list is complete; wave 0 may touch the pool
        if (done < nb && wave == 0) {
          // the generator and the pool as they stood after iteration j: undo the block's swaps, restore the state, draw j + 1 again
          if (lane == 0)
            for (int s = kDltSample * (int)nb - 1; s >= 0; --s) {
              const uint32_t i = (uint32_t)s % kDltSample, r = swaps[s];
              const uint32_t a = pool[i], b = pool[r];
              pool[i] = b; pool[r] = a;
            }
          for (int i = lane; i < kMtN; i += 64) mt[i] = mt_saved[i];
          wave_sync();
          mt_idx = mt_idx_saved;
          for (uint32_t jj = 0; jj < done; ++jj)
            for (uint32_t i = 0; i < (uint32_t)kDltSample; ++i) {
              const uint32_t r = uniform_u32(mt, mt_idx, lane, i, pool_n - 1);
              if (lane == 0) { const uint32_t a = pool[i], b = pool[r]; pool[i] = b; pool[r] = a; }
            }
        }
        __syncthreads();
        if (take_pool) {   // vec_index = vec_inliers: in sorted order
          for (uint32_t i = tid; i < n_inl; i += n_threads) pool[i] = inliers[i];
          pool_n = n_inl;
        }
      }
    }
    iter += done;
    __syncthreads();
  }

  if (minNFA >= 0) n_inl = 0;   // no meaningful model
  for (uint32_t i = tid; i < n_inl; i += n_threads) inliers_out[P.start + i] = inliers[i];
  if (tid == 0) {
    ResResult& R = results[pi];
    for (int e = 0; e < 12; ++e) R.P[e] = best_model[e];
    R.error_max = errorMax; R.min_nfa = minNFA; R.n_inliers = n_inl; R.n_iterations = iter; R.n_models = n_models_total; R.pad_ = 0;
  }
}

// ---- host ----
template <bool kGlobal>
int dlt_launch(uint32_t n_work, uint32_t lds_bytes, hipStream_t stream, const DltProblem* problems, const uint32_t* order, const double* xn, const double* X3d,
               const float* l10, const uint32_t* mt_init, uint32_t max_iteration, uint32_t waves_ahead, uint32_t n_lds_max, unsigned char* scratch, ResResult* results,
               uint32_t* inliers_out, uint32_t* trace, uint32_t trace_events) {
  MVGX_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&resection_dlt_acransac_kernel<kGlobal>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
  hipLaunchKernelGGL((resection_dlt_acransac_kernel<kGlobal>), dim3(n_work), dim3(64 * kResWaves), lds_bytes, stream, problems, order, n_work, xn, X3d, l10, mt_init,
                     max_iteration, waves_ahead, n_lds_max, scratch, results, inliers_out, trace, trace_events);
  MVGX_HIP(hipGetLastError());
  return MVGX_OK;
}

// The staging buffer of the uncalibrated entry (the layout of res_stage): problem table | launch lists | log10 table | generator state
int dlt_stage(ResCall& c, const uint64_t* start, const uint32_t* image_wh) {
  const uint32_t n_problems = c.n_problems;
  int rc;
  c.n_lists = c.in_lds.size() + c.in_global.size();
  c.prob_words = (size_t)n_problems * sizeof(DltProblem) / 4;
  c.bound_words = 0;
  c.l10_n = (size_t)c.n_max + 2;
  c.stage_words = c.prob_words + c.n_lists + c.l10_n + kMtN;
  if ((rc = c.stage.ensure((c.stage_words + 1) / 2))) return rc;
  DltProblem* const hp = reinterpret_cast<DltProblem*>(c.stage.p);
  c.h_lists = reinterpret_cast<uint32_t*>(c.stage.p) + c.prob_words;
  float* const h_l10 = reinterpret_cast<float*>(c.h_lists + c.n_lists);
  uint32_t* const h_mt = reinterpret_cast<uint32_t*>(h_l10 + c.l10_n);
  for (uint32_t p = 0; p < n_problems; ++p) {
    DltProblem& g = hp[p];
    const uint32_t n = (uint32_t)(start[p + 1] - start[p]);
    const int width = (int)image_wh[2 * p], height = (int)image_wh[2 * p + 1];
    g.start = start[p] - c.base; g.n = n; g.pad_ = 0; g.scratch = 0;
    // PreconditionerFromPoints(width, height, &T) (conditioning.cpp:54-62): the x offset goes through a float product (-.5f * width)
    g.d_norm = 1.0 / std::sqrt(static_cast<double>(width * height));
    g.off_x = -.5f * width * g.d_norm;
    g.off_y = -.5 * height * g.d_norm;
    g.loge0 = n > (uint32_t)kDltSample ? std::log10((double)(n - kDltSample)) : 0.0;   // MAX_MODELS = 1, MINIMUM_SAMPLES = 6
  }
  c.scratch_bytes = 0;
  for (uint32_t p : c.in_global) { hp[p].scratch = c.scratch_bytes; c.scratch_bytes += res_scratch_bytes(hp[p].n); }
  if (!c.in_lds.empty()) memcpy(c.h_lists, c.in_lds.data(), c.in_lds.size() * 4);
  if (!c.in_global.empty()) memcpy(c.h_lists + c.in_lds.size(), c.in_global.data(), c.in_global.size() * 4);
  for (size_t i = 0; i < c.l10_n; ++i) h_l10[i] = (float)::log10((double)static_cast<float>(i));
  h_mt[0] = 5489u;   // std::mt19937::default_seed
  for (int i = 1; i < kMtN; ++i) h_mt[i] = 1812433253u * (h_mt[i - 1] ^ (h_mt[i - 1] >> 30)) + (uint32_t)i;
  return MVGX_OK;
}

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
  MVGX_REQUIRE(opt && start && out_ok && out_pose && out_P && out_K && out_error_max && out_min_nfa && out_inlier_start, MVGX_ERR_ARG, "%s: NULL argument", fn);
  MVGX_REQUIRE(n_problems == 0 || image_wh, MVGX_ERR_ARG, "%s: NULL image sizes", fn);
  MVGX_REQUIRE(opt->solver == MVGX_RESECTION_DLT_6POINTS, MVGX_ERR_ARG,
               "%s: solver %d: this entry runs DLT_6POINTS = 0 alone (the calibrated solvers are mvgx_resection_localize's)", fn, opt->solver);
  MVGX_REQUIRE(!std::isfinite(opt->error_max), MVGX_ERR_UNSUPPORTED,
               "%s: a finite error_max selects the quantified NFA with the max-consensus early exit, which the six-point loop has no device path for", fn);
  MVGX_REQUIRE(std::isinf(opt->error_max) && opt->error_max > 0, MVGX_ERR_ARG, "%s: error_max must be +infinity", fn);
  MVGX_REQUIRE(opt->waves_ahead <= (uint32_t)kResWaves, MVGX_ERR_ARG, "%s: waves_ahead %u exceeds the build's %d", fn, opt->waves_ahead, kResWaves);
  c.n_problems = n_problems;
  for (uint32_t p = 0; p < n_problems; ++p) {
    MVGX_REQUIRE(start[p + 1] >= start[p], MVGX_ERR_ARG, "%s: start decreases at problem %u", fn, p);
    const uint64_t n = start[p + 1] - start[p];
    MVGX_REQUIRE(n <= kResMaxN, MVGX_ERR_ARG, "%s: problem %u has %llu correspondences, the supported maximum is %u", fn, p, (unsigned long long)n, kResMaxN);
    const uint64_t w = image_wh[2 * p], h = image_wh[2 * p + 1];
    MVGX_REQUIRE(w > 0 && h > 0 && w * h <= 0x7fffffffull, MVGX_ERR_ARG, "%s: problem %u: image size %llu x %llu (both must be > 0, their product an int)", fn, p,
                 (unsigned long long)w, (unsigned long long)h);
    c.n_max = std::max(c.n_max, (uint32_t)n);
  }
  if (stats) memset(stats, 0, sizeof(*stats));
  for (uint32_t p = 0; p < n_problems; ++p) { out_ok[p] = 0; out_error_max[p] = 0.0; out_min_nfa[p] = 0.0; }
  for (uint32_t p = 0; p <= n_problems; ++p) out_inlier_start[p] = 0;
  if (!n_problems) return MVGX_OK;
  c.base = start[0];
  c.n_total = start[n_problems] - c.base;
  MVGX_REQUIRE(c.n_total == 0 || (x2d && X3d && out_inliers), MVGX_ERR_ARG, "%s: NULL correspondence arrays", fn);
  // the storage form per problem: the LDS form up to kDltLdsMaxN, global scratch above it
  const uint32_t lds_bound = opt->global_above ? std::min(opt->global_above, kDltLdsMaxN) : kDltLdsMaxN;
  for (uint32_t p = 0; p < n_problems; ++p) {
    const uint64_t n = start[p + 1] - start[p];
    if (n > (uint64_t)kDltSample) (n <= lds_bound ? c.in_lds : c.in_global).push_back(p);   // ACRANSAC's early return below that
  }
  const auto by_n = [&](uint32_t a, uint32_t b) { const uint64_t na = start[a + 1] - start[a], nb = start[b + 1] - start[b]; return na != nb ? na > nb : a < b; };
  std::sort(c.in_lds.begin(), c.in_lds.end(), by_n);
  std::sort(c.in_global.begin(), c.in_global.end(), by_n);
  if (c.in_lds.empty() && c.in_global.empty()) return MVGX_OK;
  if ((rc = mvgx::select_device(device < 0 ? -1 : device))) return rc;
  if ((rc = dlt_stage(c, start, image_wh))) return rc;
  if ((rc = res_upload(c, x2d, X3d))) return rc;
  uint32_t* const host_trace = g_res_trace;   // (one call only)
  const uint32_t trace_events = host_trace ? g_res_trace_events : 0;
  g_res_trace = nullptr;
  const size_t trace_words = (size_t)n_problems * res_trace_words(trace_events);
  if (host_trace) {
    if ((rc = c.d_trace.ensure(trace_words))) return rc;
    MVGX_HIP(hipMemsetAsync(c.d_trace.p, 0, trace_words * sizeof(uint32_t), c.stream));
  }
  uint32_t* const p_trace = host_trace ? c.d_trace.p : nullptr;
  const DltProblem* const hp = reinterpret_cast<const DltProblem*>(c.stage.p);
  const DltProblem* const p_prob = reinterpret_cast<const DltProblem*>(c.d_stage.p);
  double* const p_xn = c.d_bear.p;   // (2 of its 3 doubles per correspondence)
  {
    const double* const p_x2d = c.d_x2d.p;
    const uint64_t n_total = c.n_total;
    MVGX_HIP(hipEventRecord(c.e0, c.stream));
    hipLaunchKernelGGL(resection_dlt_normalize_kernel, dim3((unsigned)((n_total + 255) / 256)), dim3(256), 0, c.stream, p_prob, n_problems, n_total, p_x2d, p_xn);
    MVGX_HIP(hipGetLastError());
  }
  if (!c.in_lds.empty()) {
    const uint32_t n_lds_max = hp[c.in_lds[0]].n;   // (every workgroup of the launch gets the LDS of its largest problem)
    if ((rc = dlt_launch<false>((uint32_t)c.in_lds.size(), dlt_lds_bytes(n_lds_max), c.stream, p_prob, c.p_lists(), p_xn, c.d_X.p, c.p_l10(), c.p_mt(), opt->max_iteration,
                                opt->waves_ahead, n_lds_max, c.d_scratch.p, c.d_res.p, c.d_inl.p, p_trace, trace_events)))
      return rc;
  }
  if (!c.in_global.empty()) {
    if ((rc = dlt_launch<true>((uint32_t)c.in_global.size(), dlt_lds_bytes(0), c.stream, p_prob, c.p_lists() + c.in_lds.size(), p_xn, c.d_X.p, c.p_l10(), c.p_mt(),
                               opt->max_iteration, opt->waves_ahead, 0, c.d_scratch.p, c.d_res.p, c.d_inl.p, p_trace, trace_events)))
      return rc;
  }
  MVGX_HIP(hipEventRecord(c.e1, c.stream));
  MVGX_HIP(hipMemcpyAsync(c.h_res.p, c.d_res.p, (size_t)n_problems * sizeof(ResResult), hipMemcpyDeviceToHost, c.stream));
  std::vector<uint32_t> inl(c.n_total);   // the inlier lists come back in place (one list per problem at its start), then are packed
  MVGX_HIP(hipMemcpyAsync(inl.data(), c.d_inl.p, c.n_total * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  if (host_trace) MVGX_HIP(hipMemcpyAsync(host_trace, c.d_trace.p, trace_words * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
  MVGX_HIP(hipStreamSynchronize(c.stream));

  uint64_t at = 0, iterations = 0, n_models = 0;
  for (uint32_t p = 0; p < n_problems; ++p) {
    out_inlier_start[p] = at;
    const ResResult& r = c.h_res.p[p];
    if (hp[p].n <= (uint32_t)kDltSample) continue;   // ACRANSAC's early return of (0, 0): nothing else is written
    iterations += r.n_iterations; n_models += r.n_models;
    out_min_nfa[p] = r.min_nfa;
    const double d = hp[p].d_norm;
    out_error_max[p] = r.n_inliers ? std::sqrt(r.error_max) / d : r.error_max;   // unormalizeError: sqrt(val) / N1(0, 0)
    if (r.n_inliers) memcpy(out_inliers + at, inl.data() + hp[p].start, (size_t)r.n_inliers * sizeof(uint32_t));
    at += r.n_inliers;
    if ((double)r.n_inliers > 2.5 * kDltSample) {
      // UnnormalizerResection: N1^-1 P, the inverse as Eigen's PartialPivLU of the dynamic matrix forms it (back substitution of I)
      const double i00 = 1.0 / d, i02 = (0.0 - hp[p].off_x * 1.0) / d, i12 = (0.0 - hp[p].off_y * 1.0) / d;
      double* const Pu = out_P + 12 * (size_t)p;
      for (int e = 0; e < 4; ++e) {
        Pu[e] = i00 * r.P[e] + i02 * r.P[8 + e];
        Pu[4 + e] = i00 * r.P[4 + e] + i12 * r.P[8 + e];
        Pu[8 + e] = r.P[8 + e];
      }
      double R[9], t[3];
      res_krt_from_p(Pu, out_K + 9 * (size_t)p, R, t);
      double* const pose = out_pose + 15 * (size_t)p;
      for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) pose[4 * i + j] = R[3 * i + j];
        pose[4 * i + 3] = t[i];
        pose[12 + i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);   // C = -R^T t
      }
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
