// mvgx_resection_loop.h - the a-contrario loop of the device's robust resections, written once. Included by mvgx_geofilter.hip before
// mvgx_resection.h (the P3P solvers, the exhaustive and the bounded form, the host side) and mvgx_resection_dlt.h (the six-point solver
// and its form); it uses that unit's std::mt19937, bounded draw, logcombi and un-contracted mul_rn / add_rn.
// What is restated (paths under src/openMVG of the reference):
//   robust_estimation/robust_estimator_ACRansac.hpp:257-304      the exhaustive NFA of one model
//   robust_estimation/robust_estimator_ACRansac.hpp:326-489      the a-contrario loop: its iteration reserve, the adopted pool
//   robust_estimation/rand_sampling.hpp:71-100                   UniformSample on the pool (kSample Fisher-Yates swaps at its head)
// Mapping ("Resection"): one workgroup runs one problem from start to end; each of its kResWaves waves evaluates one
// iteration of a block of consecutive iterations ahead, under the pool and minNFA the block started with; the verdicts are read in
// iteration order, the first event is applied and what was drawn after it is drawn again. No workgroup waits for another.
// What is here: the LDS layout (ResLayout) and the tables (ResTables), the generator and the block's draw and rewind (ResGen,
// res_draw_block, res_rewind_block), the iteration budget (ResBudget), the sort and the NFA scan (res_sort, res_best_nfa), the pieces
// of a verdict's application (res_keep_model, res_trace_record, res_adopt_pool, res_write_result) and the exhaustive loop itself
// (resection_acransac_kernel) over a form struct: ResP3PForm of mvgx_resection.h, ResDltForm of mvgx_resection_dlt.h. The bounded
// loop (resection_acransac_bounded_kernel of mvgx_resection.h) is built from the same pieces around its own verdict handling.
#pragma once
#include "ba_math.h"

// The reference's build has no fused multiply-add. The solvers are ill-conditioned on some samples (a sample of the fixture moves by
// 7e-11 under contraction, 20 times the distance between reference and restatement there), and the order of near-equal residuals
// follows the last bits: everything in the resection headers is compiled as separate products and sums. (Division and square root of
// doubles round correctly on the device; cbrt, acos, cos and log10 are OCML's, within an ulp or two of glibc's.)
// (A file-scope pragma holds to the end of the translation unit: the three resection headers are the last things mvgx_geofilter.hip
// includes. In the emulation's single unit the files included after them are compiled for a host without fused multiply-add, where it
// changes nothing.)
#pragma clang fp contract(off)

namespace {

constexpr int kResWaves = 8;                  // W: waves (= iterations evaluated ahead) per workgroup
constexpr uint32_t kResMaxN = 65536;          // largest supported n
constexpr int kResVerdict = 18;               // doubles per wave (exhaustive forms): better | nfa | k | error | P[12] | models evaluated | unused
constexpr double kResFltEps = 1.1920928955078125e-07;       // std::numeric_limits<float>::epsilon()
constexpr int kResTraceRecord = 10;           // words of a trace record (test hook): iteration | k | the first 8 sorted indices
__host__ __device__ constexpr uint32_t res_trace_words(uint32_t events) { return 1 + kResTraceRecord * events; }   // per problem: count | records
// Test hook (mvgx_resection_debug_trace): where the next call leaves, per problem, the iterations that found a better model
uint32_t* g_res_trace = nullptr;
uint32_t g_res_trace_events = 0;

struct ResResult {
  double P[12];           // best model, row-major 3 x 4; valid if n_inliers > 0
  double error_max, min_nfa;   // normalised squared residual at the chosen k; minNFA
  uint32_t n_inliers, n_iterations, n_models, pad_;
};

// ---- storage ----
__host__ __device__ constexpr uint32_t res_table_words(uint32_t n) { return 4 * (n + 1); }    // pool, inliers, logc_n, logc_k (n + 1 each)
__host__ __device__ constexpr uint32_t res_slice_words(uint32_t p2) { return 3 * p2; }         // keys (64 bit) | indices
__host__ __device__ constexpr uint32_t res_pow2(uint32_t n) { uint32_t p = 64; while (p < n) p <<= 1; return p; }   // the sort's length: n padded with +inf

// The words of LDS a workgroup needs, and where each part lies: generator | its copy | verdicts | per-wave work (the models) | samples,
// swap partners, model counts | the form's extra words | best model | (LDS form) pool, inliers, logc_n, logc_k and, with kSlices, the
// waves' sort slices. The sizes the host asks for and the pointers a kernel carves both come from the offsets below.
template <int kSample, int kVerdict_, int kWork_, int kExtra, bool kSlices>
struct ResLayout {
  static constexpr int kVerdict = kVerdict_, kWork = kWork_;      // doubles per wave
  static constexpr bool kHasSlices = kSlices;
  static constexpr uint32_t kDraw = (2 * kSample + 1 + 7) / 8 * 8;   // words per wave: sample | swap partners | model count, padded
  static constexpr uint32_t kAtSaved = kMtN, kAtVerdicts = 2 * kMtN, kAtWorks = kAtVerdicts + 2 * kResWaves * kVerdict,
                            kAtSamples = kAtWorks + 2 * kResWaves * kWork, kAtSwaps = kAtSamples + kResWaves * kSample,
                            kAtCounts = kAtSwaps + kResWaves * kSample, kAtExtra = kAtSamples + kResWaves * kDraw, kAtBest = kAtExtra + kExtra,
                            kFixed = kAtBest + 24;
  static_assert(kExtra % 2 == 0, "the best model is read as doubles");
  __host__ __device__ static constexpr uint32_t words(uint32_t n_lds_max) {   // 0: the global form (tables and slices in the problem's scratch)
    return kFixed + (n_lds_max ? res_table_words(n_lds_max) + (kSlices ? kResWaves * res_slice_words(res_pow2(n_lds_max)) : 0) : 0);
  }
  static uint32_t lds_bytes(uint32_t n_lds_max) { return 4 * words(n_lds_max); }
  static size_t scratch_bytes(uint32_t n) { return ((size_t)4 * (words(n) - kFixed) + 255) / 256 * 256; }

  uint32_t *mt, *mt_saved, *samples, *swaps, *n_mod, *extra, *tables;
  double *verdicts, *works, *best_model;   // best_model: the winning 3 x 4 matrix (thread 0 writes and reads it)
  __device__ __forceinline__ explicit ResLayout(uint32_t* lds)
      : mt(lds), mt_saved(lds + kAtSaved), samples(lds + kAtSamples), swaps(lds + kAtSwaps), n_mod(lds + kAtCounts), extra(lds + kAtExtra), tables(lds + kFixed),
        verdicts(reinterpret_cast<double*>(lds + kAtVerdicts)), works(reinterpret_cast<double*>(lds + kAtWorks)), best_model(reinterpret_cast<double*>(lds + kAtBest)) {}
};

struct ResTables {
  uint32_t *pool, *inliers;
  float *logc_n, *logc_k;
  uint32_t* slices;        // one per wave, slice_words each: p2 keys, then p2 indices
  uint32_t slice_words;
};
// base: the LDS behind the fixed part, or the problem's scratch; n_sized: what the storage was sized for (LDS form: the launch's largest
// problem, so that every wave's slice starts at the same place in every workgroup); has_slices: the layout's kHasSlices - a form
// without a sort has no slices to point at
__device__ __forceinline__ ResTables res_tables(uint32_t* base, uint32_t n, uint32_t n_sized, bool has_slices) {
  ResTables T;
  T.pool = base;
  T.inliers = T.pool + (n + 1);
  T.logc_n = reinterpret_cast<float*>(T.inliers + (n + 1));
  T.logc_k = T.logc_n + (n + 1);
  T.slices = has_slices ? base + res_table_words(n_sized) : nullptr;
  T.slice_words = has_slices ? res_slice_words(res_pow2(n_sized)) : 0;
  return T;
}

// The one generator of a problem and its state from before the block (a twist cannot be taken back); the positions are tracked by wave 0 alone
struct ResGen {
  uint32_t *mt, *saved;
  int idx, idx_saved;
  __device__ __forceinline__ void save(int lane) {
    for (int i = lane; i < kMtN; i += 64) saved[i] = mt[i];
    wave_sync();
    idx_saved = idx;
  }
  __device__ __forceinline__ void restore(int lane) {
    for (int i = lane; i < kMtN; i += 64) mt[i] = saved[i];
    wave_sync();
    idx = idx_saved;
  }
};

// pool = 0 .. n, logc_k[k] = logcombi(kSample, k), logc_n[k] = logcombi(k, n), the generator's initial state; by the workgroup, two barriers
template <int kSample>
__device__ __forceinline__ void res_tables_init(const ResTables& T, ResGen& gen, const uint32_t* __restrict__ mt_init, const float* __restrict__ l10, uint32_t n, int tid) {
  const int n_threads = 64 * kResWaves;
  for (uint32_t k = tid; k <= n; k += n_threads) {
    T.pool[k] = k;
    T.logc_k[k] = logcombi(kSample, k, l10);
  }
  // logc_n[k] = logcombi(k, n) is the running float sum of min(k, n - k) terms that do not depend on k: one pass of n / 2 dependent
  // additions by one thread (the sum's order is the reference's; n calls of logcombi would be n^2 / 4 additions), then the mirror
  if (tid == 0) {
    float r = 0.f;
    T.logc_n[0] = 0.f;
    for (uint32_t i = 1; i <= n / 2; ++i) { r += l10[n - i + 1] - l10[i]; T.logc_n[i] = r; }
  }
  __syncthreads();
  for (uint32_t k = n / 2 + 1 + tid; k <= n; k += n_threads) T.logc_n[k] = k >= n ? 0.f : T.logc_n[n - k];
  for (int i = tid; i < kMtN; i += n_threads) gen.mt[i] = mt_init[i];
  gen.idx = gen.idx_saved = kMtN;
  __syncthreads();
}

// ---- the block's samples, by wave 0 ----
// UniformSample on the pool: kSample swaps at its head; record: where the swap partners go (nullptr: an iteration that is drawn again)
template <int kSample>
__device__ __forceinline__ void res_draw_swaps(ResGen& gen, uint32_t* pool, uint32_t pool_n, uint32_t* record, int lane) {
  for (uint32_t i = 0; i < (uint32_t)kSample; ++i) {
    const uint32_t r = uniform_u32(gen.mt, gen.idx, lane, i, pool_n - 1);
    if (lane == 0) {   // (lane 0 alone reads and writes the pool here)
      const uint32_t a = pool[i], b = pool[r];
      pool[i] = b; pool[r] = a;
      if (record) record[i] = r;
    }
  }
}
// the samples of nb iterations, drawn in iteration order from the one generator
template <int kSample>
__device__ __forceinline__ void res_draw_block(ResGen& gen, uint32_t* pool, uint32_t pool_n, uint32_t* swaps, uint32_t* samples, uint32_t nb, int lane) {
  gen.save(lane);
  for (uint32_t j = 0; j < nb; ++j) {
    res_draw_swaps<kSample>(gen, pool, pool_n, swaps + kSample * j, lane);
    if (lane == 0)
      for (int i = 0; i < kSample; ++i) samples[kSample * j + i] = pool[i];
  }
}
// the generator and the pool as they stood after iteration done - 1 of the block: undo the block's swaps, restore the state, draw `done` again
template <int kSample>
__device__ __forceinline__ void res_rewind_block(ResGen& gen, uint32_t* pool, uint32_t pool_n, const uint32_t* swaps, uint32_t nb, uint32_t done, int lane) {
  if (lane == 0)
    for (int s = kSample * (int)nb - 1; s >= 0; --s) {
      const uint32_t i = (uint32_t)s % kSample, r = swaps[s];
      const uint32_t a = pool[i], b = pool[r];
      pool[i] = b; pool[r] = a;
    }
  gen.restore(lane);
  for (uint32_t jj = 0; jj < done; ++jj) res_draw_swaps<kSample>(gen, pool, pool_n, nullptr, lane);
}

// ---- the iteration budget and its reserve (robust_estimator_ACRansac.hpp:375-380, :454-474) ----
struct ResBudget {
  uint32_t max_iteration, nIter, iter;
  int nIterReserve;
  __device__ __forceinline__ explicit ResBudget(uint32_t max_iteration_)
      : max_iteration(max_iteration_), nIter(max_iteration_ - max_iteration_ / 10), iter(0), nIterReserve((int)(max_iteration_ / 10)) {}
  __device__ __forceinline__ bool running() const { return iter < nIter && iter < max_iteration; }
  __device__ __forceinline__ uint32_t block(uint32_t waves_ahead) const { return min(waves_ahead, min(nIter - iter, max_iteration - iter)); }
  // after iteration iter + j: a meaningful better model, or the last iteration before the reserve. Returns whether either happened;
  // take_pool: the inlier list becomes the pool that is sampled from
  __device__ __forceinline__ bool reserve_event(bool meaningful, uint32_t j, uint32_t n_inl, bool& take_pool) {
    const bool branch = meaningful || ((iter + j + 1) == nIter && nIterReserve > 0);
    if (branch) {
      if (n_inl == 0) { ++nIter; --nIterReserve; }
      else {
        take_pool = true;
        if (nIterReserve) { nIter = iter + j + 1 + (uint32_t)nIterReserve; nIterReserve = 0; }
      }
    }
    return branch;
  }
};

// ---- a model, its sorted residuals, its NFA ----
struct ResRt { double m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11; };   // a 3 x 4 model, row-major
__device__ __forceinline__ ResRt res_rt_load(const double* __restrict__ M) { return {M[0], M[1], M[2], M[3], M[4], M[5], M[6], M[7], M[8], M[9], M[10], M[11]}; }
// a model with a non-finite entry is skipped (the reference would sort NaNs: undefined)
__device__ __forceinline__ bool res_rt_finite(const ResRt& M) {
  const double probe = M.m0 + M.m1 + M.m2 + M.m3 + M.m4 + M.m5 + M.m6 + M.m7 + M.m8 + M.m9 + M.m10 + M.m11;
  return fabs(probe) < INFINITY;
}

// (residual bits, index) ascending: residuals are non-negative or +inf, so the bit patterns order as the values do
__device__ __forceinline__ bool res_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}
// bitonic sort of p2 (a power of two >= 64) records by one wave; every stage ends with the wave's writes visible to its lanes. In the
// global form the slice is global memory: wave_sync's wavefront-scope fence covers every address space (the compiler waits for the
// stores), and a CU's vector memory path serves one wave's accesses to an address in order, so the next stage's loads see them.
__device__ __forceinline__ void res_sort(uint64_t* keys, uint32_t* idx, uint32_t p2, int lane) {
  for (uint32_t k = 2; k <= p2; k <<= 1) {
    for (uint32_t j = k >> 1; j > 0; j >>= 1) {
      for (uint32_t t = lane; t < p2 / 2; t += 64) {
        const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const uint64_t ki = keys[i], kl = keys[l];
        const uint32_t ii = idx[i], il = idx[l];
        const bool up = (i & k) == 0;
        if (res_less(kl, il, ki, ii) == up) { keys[i] = kl; keys[l] = ki; idx[i] = il; idx[l] = ii; }
      }
      wave_sync();
    }
  }
}
// NFA(k) of the sorted residuals for every k in [kSample + 1, n]: the smallest, the lowest k among equals, in every lane
template <int kSample>
__device__ __forceinline__ void res_best_nfa(const uint64_t* keys, const float* logc_n, const float* logc_k, double loge0, uint32_t n, int lane, double& best, uint32_t& best_k) {
  const double logalpha0 = 0.49714987269413385;   // log10(M_PI)
  best = INFINITY;
  best_k = kSample;
  for (uint32_t k = kSample + 1 + lane; k <= n; k += 64) {
    const double r = __longlong_as_double((long long)keys[k - 1]);
    const double logalpha = add_rn(logalpha0, log10(add_rn(r, kResFltEps)));
    const double nfa = add_rn(add_rn(add_rn(loge0, mul_rn(logalpha, (double)(k - kSample))), (double)logc_n[k]), (double)logc_k[k]);
    if (nfa < best) { best = nfa; best_k = k; }
  }
  for (int d = 32; d > 0; d >>= 1) {
    const double o = __shfl_xor(best, d);
    const uint32_t ok = (uint32_t)__shfl_xor((int)best_k, d);
    if (o < best || (o == best && ok < best_k)) { best = o; best_k = ok; }
  }
}

// ---- what a verdict's application and the end of a problem are made of ----
__device__ __forceinline__ void res_keep_model(double* best_model, const double* M, int tid) {
  if (tid == 0)
    for (int e = 0; e < 12; ++e) best_model[e] = M[e];
}
// test hook (one thread): iteration | k | the head of the sorted list, one record per iteration that found a better model
__device__ __forceinline__ void res_trace_record(uint32_t* trace, uint32_t trace_events, uint32_t pi, uint32_t iteration, uint32_t n_inl, const uint32_t* sorted) {
  uint32_t* const T = trace + (size_t)pi * res_trace_words(trace_events);
  const uint32_t at = T[0];
  if (at < trace_events) {
    uint32_t* const rec = T + 1 + (size_t)kResTraceRecord * at;
    rec[0] = iteration; rec[1] = n_inl;
    for (uint32_t i = 0; i < (uint32_t)kResTraceRecord - 2; ++i) rec[2 + i] = i < n_inl ? sorted[i] : 0xffffffffu;
  }
  T[0] = at + 1;
}
// vec_index = vec_inliers, in the list's order
__device__ __forceinline__ void res_adopt_pool(uint32_t* pool, const uint32_t* inliers, uint32_t n_inl, uint32_t& pool_n, int tid) {
  for (uint32_t i = tid; i < n_inl; i += 64 * kResWaves) pool[i] = inliers[i];
  pool_n = n_inl;
}
__device__ __forceinline__ void res_write_result(ResResult& R, uint32_t* inliers_out, const uint32_t* inliers, const double* best_model, double minNFA, double errorMax,
                                                 uint32_t n_inl, uint32_t iter, uint32_t n_models, int tid) {
  if (minNFA >= 0) n_inl = 0;   // no meaningful model
  for (uint32_t i = tid; i < n_inl; i += 64 * kResWaves) inliers_out[i] = inliers[i];
  if (tid == 0) {
    for (int e = 0; e < 12; ++e) R.P[e] = best_model[e];
    R.error_max = errorMax; R.min_nfa = minNFA; R.n_inliers = n_inl; R.n_iterations = iter; R.n_models = n_models; R.pad_ = 0;
  }
}

// the problem of correspondence i (prepare passes): the last one that starts at or before i and is not empty there
template <class Problem>
__device__ __forceinline__ const Problem& res_problem_of(const Problem* __restrict__ problems, uint32_t n_problems, uint64_t i) {
  uint32_t lo = 0, hi = n_problems - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) / 2;
    if (problems[mid].start <= i) lo = mid; else hi = mid - 1;
  }
  return problems[lo];
}

// ---- the exhaustive loop ----
// A Form supplies: Problem (the per-problem record: start, scratch, n, loge0 and what the form reads), Layout (a ResLayout), kSample,
// kMaxModels (per sample), kModelAt (where a wave's work area holds its models, 12 doubles each), a constructor from (problem, x2d, X3d,
// prepared, solver), load_sample (by the wave's first kSample lanes), solve (returns the number of models, the same in every lane) and
// residual(M, i). prepared: what the form's prepare pass wrote per correspondence.
template <class Form, bool kGlobal>
__global__ __launch_bounds__(64 * kResWaves) void resection_acransac_kernel(const uint32_t* __restrict__ order, uint32_t n_work, uint32_t n_lds_max,
                                                                            const typename Form::Problem* __restrict__ problems, const double* __restrict__ x2d,
                                                                            const double* __restrict__ X3d, const double* __restrict__ prepared, const float* __restrict__ l10,
                                                                            const uint32_t* __restrict__ mt_init, uint32_t max_iteration, int solver, uint32_t waves_ahead,
                                                                            unsigned char* __restrict__ scratch, ResResult* __restrict__ results, uint32_t* __restrict__ inliers_out,
                                                                            uint32_t* __restrict__ trace, uint32_t trace_events) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds_u32[];
  if (blockIdx.x >= n_work) return;
  using L = typename Form::Layout;
  constexpr int kSample = Form::kSample;
  const uint32_t pi = order[blockIdx.x];
  const typename Form::Problem& P = problems[pi];
  const uint32_t n = P.n, p2 = res_pow2(n);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n_threads = 64 * kResWaves;

  const L lds(lds_u32);
  // LDS form: every wave's slice is sized for the launch's largest problem
  const ResTables T = res_tables(kGlobal ? reinterpret_cast<uint32_t*>(scratch + P.scratch) : lds.tables, n, kGlobal ? n : n_lds_max, L::kHasSlices);
  uint64_t* const my_keys = reinterpret_cast<uint64_t*>(T.slices + (size_t)wave * T.slice_words);
  uint32_t* const my_idx = reinterpret_cast<uint32_t*>(my_keys + p2);
  const Form F(P, x2d, X3d, prepared, solver);
  const double loge0 = P.loge0;

  ResGen gen{lds.mt, lds.mt_saved, kMtN, kMtN};
  res_tables_init<kSample>(T, gen, mt_init, l10, n, tid);

  const uint32_t Wa = waves_ahead ? waves_ahead : (uint32_t)kResWaves;
  double minNFA = INFINITY, errorMax = INFINITY;
  if (tid == 0)
    for (int e = 0; e < 12; ++e) lds.best_model[e] = 0.0;
  uint32_t n_inl = 0, pool_n = n, n_models_total = 0;
  ResBudget it(max_iteration);

  while (it.running()) {
    const uint32_t nb = it.block(Wa);
    if (wave == 0) res_draw_block<kSample>(gen, T.pool, pool_n, lds.swaps, lds.samples, nb, lane);
    __syncthreads();

    // ---- one wave, one iteration ----
    if ((uint32_t)wave < nb) {
      double* const work = lds.works + L::kWork * wave;
      double* const my_verdict = lds.verdicts + L::kVerdict * wave;
      F.load_sample(lds.samples + kSample * wave, work, my_verdict, lane);
      wave_sync();
      const int nm = F.solve(work, my_verdict, lds.n_mod + wave, lane);
      const double* const models = work + Form::kModelAt;
      double run_min = minNFA, win_err = 0.0;
      int winner = -1, sorted = -1;
      uint32_t win_k = 0, evaluated = 0;
      // One pass per model. A form with several models per sample has pass nm too: the winner's order once more, if a later model was
      // sorted over it. A form with one model says so to the compiler: the loop is then an `if` (as a loop of unknown length it cost the
      // six-point kernel 0.3 - 0.6 % through the schedule of dlt_solve's round: DESIGN.md)
      const int n_pass = Form::kMaxModels > 1 ? nm + 1 : (nm > 0 ? 1 : 0);
      for (int m = 0; m < n_pass; ++m) {
        const int mm = m < nm ? m : winner;
        if (m == nm && (winner < 0 || winner == sorted)) break;
        const ResRt M = res_rt_load(models + 12 * mm);
        if (!res_rt_finite(M)) continue;
        for (uint32_t i = lane; i < p2; i += 64) {
          double e = INFINITY;
          if (i < n) {
            e = F.residual(M, i);
            if (!(e < INFINITY)) e = INFINITY;   // NaN too
          }
          my_keys[i] = (uint64_t)__double_as_longlong(e);
          my_idx[i] = i;
        }
        wave_sync();
        res_sort(my_keys, my_idx, p2, lane);
        sorted = mm;
        if (m == nm) break;
        ++evaluated;
        double best;
        uint32_t best_k;
        res_best_nfa<kSample>(my_keys, T.logc_n, T.logc_k, loge0, n, lane, best, best_k);
        if (best < run_min) {
          run_min = best; winner = mm; win_k = best_k;
          win_err = __longlong_as_double((long long)my_keys[best_k - 1]);
        }
      }
      wave_sync();   // every lane has read the sample's vectors and the keys before the verdict overwrites the slot
      if (lane == 0) {
        my_verdict[0] = winner >= 0 ? 1.0 : 0.0;
        my_verdict[1] = run_min; my_verdict[2] = (double)win_k; my_verdict[3] = win_err;
        const double* const M = models + (Form::kMaxModels > 1 && winner > 0 ? 12 * winner : 0);
        for (int e = 0; e < 12; ++e) my_verdict[4 + e] = M[e];
        my_verdict[16] = (double)evaluated;
      }
    }
    __syncthreads();

    // ---- the verdicts in iteration order: the first event is applied, what follows it is void ----
    uint32_t done = nb;
    bool event = false;
    for (uint32_t j = 0; j < nb && !event; ++j) {
      const double* const v = lds.verdicts + L::kVerdict * j;
      n_models_total += (uint32_t)v[16];
      const bool better = v[0] != 0.0;   // (evaluated under the block's minNFA, which no earlier verdict of the block has changed)
      if (better) {
        minNFA = v[1]; errorMax = v[3]; n_inl = (uint32_t)v[2];
        res_keep_model(lds.best_model, v + 4, tid);
        const uint32_t* const src = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint64_t*>(T.slices + (size_t)j * T.slice_words) + p2);
        for (uint32_t i = tid; i < n_inl; i += n_threads) T.inliers[i] = src[i];
        if (trace && tid == 0) res_trace_record(trace, trace_events, pi, it.iter + j, n_inl, src);
      }
      bool take_pool = false;
      const bool branch = it.reserve_event(better && minNFA < 0, j, n_inl, take_pool);
      if (better || branch) {
        event = true;
        done = j + 1;
        __syncthreads();   // the inlier list is complete; wave 0 may touch the pool
        if (done < nb && wave == 0) res_rewind_block<kSample>(gen, T.pool, pool_n, lds.swaps, nb, done, lane);
        __syncthreads();
        if (take_pool) res_adopt_pool(T.pool, T.inliers, n_inl, pool_n, tid);   // (in sorted order)
      }
    }
    it.iter += done;
    __syncthreads();
  }
  res_write_result(results[pi], inliers_out + P.start, T.inliers, lds.best_model, minNFA, errorMax, n_inl, it.iter, n_models_total, tid);
}

}  // namespace
