// Stand-alone check of the geometric filter's host path (TEST INFRASTRUCTURE ONLY): openmvg_amd/csrc/mvgx_geofilter.hip under the HIP
// emulation, driven through the C ABI from a main() of its own and built with AddressSanitizer + UndefinedBehaviorSanitizer, so that a
// stage of a call that reads past an input, frees a buffer twice, forgets one or leaves one to a kernel still enqueued is a report
// (tests/test_geofilter_call_cpu.py builds and runs it). The inputs are made here and have no geometry: what counts is which code runs.
//   * all ten mvgx_geofilter_* entries, 16 iterations, four pairs per call: 0 correspondences | exactly a minimal sample (not estimated:
//     identity model) | one more | 24; the orthographic entries once with per-pair bounds and once with NULL
//   * per model: the indexed entry returns the bytes of the gathered one (mask, results, n_iterations, n_models)
//   * the same calls with MVGX_GEO_GLOBAL_ABOVE=8 (tables in global scratch) return the bytes of the LDS form
//   * n_pairs == 0, and a call whose pairs are all below a minimal sample, return MVGX_OK
//   * one gathered and one indexed entry with the emulation's allocation-failure injection (HIPEMU_FAIL_MALLOC_AFTER) at allocation
//     0, 1, 2, ... until a call succeeds: every failing call returns MVGX_ERR_HIP, and the call after the injection is switched off
//     returns the uninjected bytes
// Exit status 0 and the final "ok" line = every step behaved.
#include "hipemu.cpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <vector>

namespace geocall {

int g_failed = 0;
#define EXPECT(cond, ...)                                                                                \
  do {                                                                                                   \
    if (!(cond)) { fprintf(stderr, "geofilter_call: " __VA_ARGS__); fputc('\n', stderr); ++g_failed; }   \
  } while (0)

enum Model { F, H, E, EA8, EU3, EO, kModels };
const char* const kName[kModels] = {"f", "h", "e", "e_angular(8)", "e_angular(upright)", "eo"};
const uint32_t kMinSample[kModels] = {7, 4, 5, 8, 3, 3};

struct Lcg {
  uint32_t s;
  double unit() { s = s * 1664525u + 1013904223u; return (s >> 8) * (1.0 / 16777216.0); }   // [0, 1)
  uint32_t below(uint32_t n) { return (uint32_t)(unit() * n) % n; }
};

// The correspondences of one call in both forms: gathered per match, and - image 2 p / 2 p + 1 of pair p - per feature in shuffled order
// with three unused features per image, plus the index pairs
struct Scene {
  std::vector<uint64_t> start;
  std::vector<double> xI, xJ, bI, bJ, K_pair, bound;
  std::vector<uint32_t> wh_pair;
  std::vector<double> feat_xy, feat_bearing, K_image;
  std::vector<uint64_t> feat_start;
  std::vector<uint32_t> wh_image, pairs, ij;
  uint64_t n_pairs() const { return start.size() - 1; }
  uint32_t n_images() const { return (uint32_t)feat_start.size() - 1; }
};

Scene make_scene(const std::vector<uint32_t>& sizes, bool camera_plane, uint32_t seed) {
  Scene sc;
  Lcg rng{seed};
  static const double K[9] = {900, 0, 500, 0, 900, 400, 0, 0, 1};
  sc.start.push_back(0);
  sc.feat_start.push_back(0);
  for (size_t p = 0; p < sizes.size(); ++p) {
    const uint32_t n = sizes[p];
    sc.start.push_back(sc.start.back() + n);
    sc.bound.push_back(0.05);
    for (int im = 0; im < 2; ++im) {
      for (uint32_t v : {1000u, 800u}) { sc.wh_image.push_back(v); sc.wh_pair.push_back(v); }
      sc.K_pair.insert(sc.K_pair.end(), K, K + 9);
      sc.K_image.insert(sc.K_image.end(), K, K + 9);
      std::vector<uint32_t> slot(n + 3);   // match m of the pair is feature slot[m] of the image
      std::iota(slot.begin(), slot.end(), 0u);
      for (uint32_t k = n + 2; k > 0; --k) std::swap(slot[k], slot[rng.below(k + 1)]);
      const size_t f0 = sc.feat_start.back();
      sc.feat_start.push_back(f0 + n + 3);
      sc.feat_xy.resize(2 * (f0 + n + 3), 7.0);
      sc.feat_bearing.resize(3 * (f0 + n + 3), 0.5);
      std::vector<double>& x = im ? sc.xJ : sc.xI;
      std::vector<double>& b = im ? sc.bJ : sc.bI;
      for (uint32_t m = 0; m < n; ++m) {
        const double px = camera_plane ? rng.unit() - 0.5 : 1000.0 * rng.unit(), py = camera_plane ? rng.unit() - 0.5 : 800.0 * rng.unit();
        double v[3] = {rng.unit() - 0.5, rng.unit() - 0.5, 1.0};
        const double norm = std::sqrt(v[0] * v[0] + v[1] * v[1] + 1.0);
        x.push_back(px); x.push_back(py);
        sc.feat_xy[2 * (f0 + slot[m])] = px; sc.feat_xy[2 * (f0 + slot[m]) + 1] = py;
        for (int k = 0; k < 3; ++k) { b.push_back(v[k] / norm); sc.feat_bearing[3 * (f0 + slot[m]) + k] = v[k] / norm; }
      }
      if (im == 0) { sc.ij.resize(2 * sc.start.back()); sc.pairs.push_back(2 * (uint32_t)p); sc.pairs.push_back(2 * (uint32_t)p + 1); }
      for (uint32_t m = 0; m < n; ++m) sc.ij[2 * (sc.start[p] + m) + im] = slot[m];
    }
  }
  return sc;
}

struct Out {
  int rc = 0;
  std::vector<uint8_t> mask;
  std::vector<mvgx_geofilter_result> results;
  uint64_t n_iterations = 0, n_models = 0;
  bool same(const Out& o) const {
    return rc == o.rc && mask == o.mask && n_iterations == o.n_iterations && n_models == o.n_models && results.size() == o.results.size() &&
           (results.empty() || !memcmp(results.data(), o.results.data(), results.size() * sizeof(mvgx_geofilter_result)));
  }
};

// NULL for an empty array: what a caller with nothing to hand over passes
template <typename T> const T* ptr(const std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

Out run(Model model, bool indexed, const Scene& sc, bool per_pair_bound = true) {
  Out o;
  const uint64_t np = sc.n_pairs();
  o.mask.assign(sc.start.back(), 0xcc);
  o.results.resize(np);
  if (np) memset(o.results.data(), 0, np * sizeof(mvgx_geofilter_result));
  uint8_t* mask = o.mask.empty() ? nullptr : o.mask.data();
  mvgx_geofilter_result* res = np ? o.results.data() : nullptr;
  mvgx_geofilter_stats st;
  memset(&st, 0, sizeof(st));
  const mvgx_geofilter_options opt{model == EO ? 0.05 : 4.0, 16};
  const uint64_t* start = sc.start.data();
  const double *xI = ptr(sc.xI), *xJ = ptr(sc.xJ), *bI = ptr(sc.bI), *bJ = ptr(sc.bJ), *fxy = ptr(sc.feat_xy), *fb = ptr(sc.feat_bearing);
  const double* bound = per_pair_bound ? ptr(sc.bound) : nullptr;
  const uint64_t* fs = sc.feat_start.data();
  const uint32_t *whp = ptr(sc.wh_pair), *whi = ptr(sc.wh_image), *pr = ptr(sc.pairs), *ij = ptr(sc.ij);
  const uint32_t ni = sc.n_images();
  switch (model) {
    case F: o.rc = indexed ? mvgx_geofilter_f_acransac_indexed(0, fxy, fs, whi, ni, pr, start, ij, np, &opt, mask, res, &st)
                           : mvgx_geofilter_f_acransac(0, xI, xJ, start, whp, np, &opt, mask, res, &st); break;
    case H: o.rc = indexed ? mvgx_geofilter_h_acransac_indexed(0, fxy, fs, whi, ni, pr, start, ij, np, &opt, mask, res, &st)
                           : mvgx_geofilter_h_acransac(0, xI, xJ, start, whp, np, &opt, mask, res, &st); break;
    case E: o.rc = indexed ? mvgx_geofilter_e_acransac_indexed(0, fxy, fb, fs, whi, ptr(sc.K_image), ni, pr, start, ij, np, &opt, mask, res, &st)
                           : mvgx_geofilter_e_acransac(0, xI, xJ, bI, bJ, start, whp, ptr(sc.K_pair), np, &opt, mask, res, &st); break;
    case EA8: case EU3:
      o.rc = indexed ? mvgx_geofilter_e_angular_acransac_indexed(0, fb, fs, ni, pr, start, ij, np, model == EU3, &opt, mask, res, &st)
                     : mvgx_geofilter_e_angular_acransac(0, bI, bJ, start, np, model == EU3, &opt, mask, res, &st); break;
    default: o.rc = indexed ? mvgx_geofilter_eo_acransac_indexed(0, fxy, fs, whi, ni, pr, start, ij, bound, np, &opt, mask, res, &st)
                            : mvgx_geofilter_eo_acransac(0, xI, xJ, start, whp, bound, np, &opt, mask, res, &st); break;
  }
  o.n_iterations = st.n_iterations; o.n_models = st.n_models;
  return o;
}

// after >= 0: allocation number `after` (from 0) of what follows fails, and every later one; -1: none
void inject(int after) {
  unsetenv("HIPEMU_FAIL_MALLOC_AFTER");
  void* p = nullptr;   // (the emulation restarts its count at an allocation made while the variable is unset)
  if (hipMalloc(&p, 16) == hipSuccess) (void)hipFree(p);
  if (after >= 0) setenv("HIPEMU_FAIL_MALLOC_AFTER", std::to_string(after).c_str(), 1);
}

Scene scene_of(Model m) { return make_scene({0, kMinSample[m], kMinSample[m] + 1, 24}, m == EO, 1000u + (uint32_t)m); }

// pairs 0 and 1 of scene_of (no correspondence, exactly a minimal sample) are not estimated: rejected, the identity model
void expect_not_estimated(const char* what, Model m, const Out& o) {
  static const double kIdentity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  for (int p = 0; p < 2; ++p)
    EXPECT(!o.results[p].ok && o.results[p].n_inliers == 0 && !memcmp(o.results[p].F, kIdentity, sizeof(kIdentity)),
           "%s %s: pair %d (at most a minimal sample) did not come back rejected with the identity model", kName[m], what, p);
  for (uint32_t i = 0; i < kMinSample[m]; ++i) EXPECT(o.mask[i] == 0, "%s %s: inlier flag %u of a pair that is not estimated is set", kName[m], what, i);
}

// every entry, both sources; returns the gathered outputs per model
std::vector<Out> all_entries(const char* what) {
  std::vector<Out> outs;
  for (int mi = 0; mi < kModels; ++mi) {
    const Model m = (Model)mi;
    const Scene sc = scene_of(m);
    const Out g = run(m, false, sc), x = run(m, true, sc);
    EXPECT(g.rc == 0, "%s %s: gathered entry returned %d (%s)", kName[m], what, g.rc, mvgx_last_error());
    EXPECT(x.rc == 0, "%s %s: indexed entry returned %d (%s)", kName[m], what, x.rc, mvgx_last_error());
    EXPECT(g.same(x), "%s %s: the indexed entry does not return the bytes of the gathered one", kName[m], what);
    EXPECT(g.n_iterations > 0 && g.n_models >= g.n_iterations, "%s %s: %llu iterations, %llu models", kName[m], what,
           (unsigned long long)g.n_iterations, (unsigned long long)g.n_models);
    if (g.rc == 0) expect_not_estimated(what, m, g);
    if (m == EO) {   // one bound for all (opt->precision, the same value): the same bytes again
      const Out g1 = run(m, false, sc, false), x1 = run(m, true, sc, false);
      EXPECT(g1.rc == 0 && x1.rc == 0, "eo %s: NULL pair_precision returned %d / %d (%s)", what, g1.rc, x1.rc, mvgx_last_error());
      EXPECT(g1.same(g) && x1.same(g), "eo %s: NULL pair_precision with the same bound in the options changes the bytes", what);
    }
    outs.push_back(g);
  }
  return outs;
}

void degenerate_calls() {
  const Scene none = make_scene({}, false, 5), tiny = make_scene({0, 1, 2}, false, 6);
  for (int indexed = 0; indexed <= 1; ++indexed) {
    const Out a = run(F, indexed, none);
    EXPECT(a.rc == 0, "n_pairs == 0 (indexed %d): returned %d (%s)", indexed, a.rc, mvgx_last_error());
    for (Model m : {F, EU3}) {
      const Out b = run(m, indexed, tiny);
      EXPECT(b.rc == 0 && b.n_iterations == 0, "%s, every pair below a minimal sample (indexed %d): returned %d (%s)", kName[m], indexed, b.rc, mvgx_last_error());
      for (size_t p = 0; b.rc == 0 && p < b.results.size(); ++p) EXPECT(!b.results[p].ok && b.results[p].F[0] == 1.0, "%s: tiny pair %zu accepted", kName[m], p);
    }
  }
}

void failing_allocations(Model m, bool indexed, const Out& want) {
  const Scene sc = scene_of(m);
  int k = 0;
  for (; k < 200; ++k) {
    inject(k);
    const Out o = run(m, indexed, sc);
    inject(-1);
    if (o.rc == 0) {
      EXPECT(o.same(want), "%s (indexed %d): the call that got past failing allocation %d returns other bytes", kName[m], indexed, k);
      break;
    }
    EXPECT(o.rc == MVGX_ERR_HIP, "%s (indexed %d): allocation %d failing: returned %d, not MVGX_ERR_HIP (%s)", kName[m], indexed, k, o.rc, mvgx_last_error());
  }
  EXPECT(k >= 10 && k < 200, "%s (indexed %d): %d failing allocations before a call succeeded (a call makes more than ten)", kName[m], indexed, k);
  const Out after = run(m, indexed, sc);
  EXPECT(after.same(want), "%s (indexed %d): the call after the injection returns other bytes (rc %d)", kName[m], indexed, after.rc);
}

}  // namespace geocall

int main() {
  using namespace geocall;
  inject(-1);
  unsetenv("MVGX_GEO_GLOBAL_ABOVE");
  const std::vector<Out> lds = all_entries("(tables in LDS)");
  setenv("MVGX_GEO_GLOBAL_ABOVE", "8", 1);
  const std::vector<Out> global = all_entries("(MVGX_GEO_GLOBAL_ABOVE=8)");
  unsetenv("MVGX_GEO_GLOBAL_ABOVE");
  for (int m = 0; m < kModels; ++m) EXPECT(lds[m].same(global[m]), "%s: MVGX_GEO_GLOBAL_ABOVE=8 changes the bytes", kName[m]);
  degenerate_calls();
  failing_allocations(F, false, lds[F]);
  failing_allocations(E, true, lds[E]);
  if (g_failed) { fprintf(stderr, "geofilter_call: %d check(s) failed\n", g_failed); return 1; }
  printf("geofilter_call: ok\n");
  return 0;
}
