// Stand-alone lifetime check of the matcher contexts (TEST INFRASTRUCTURE ONLY): the product's host + device code under the HIP
// emulation, driven through the C ABI from a main() of its own and built with AddressSanitizer, so that a buffer a context forgets to
// free is a LeakSanitizer report at exit (ASAN_OPTIONS=detect_leaks=1) and a buffer freed twice or used after its context an
// AddressSanitizer one. tests/test_context_lifetime_cpu.py builds it twice, once per emulation source:
//   -DLIFETIME_MATCH : hipemu_match.cpp  -> mvgx_match_*  (default form, filter_shape 17, variant 1: the three work lists and d_cd)
//   (otherwise)      : hipemu.cpp        -> mvgx_hamming_*, mvgx_l2f_*, mvgx_l2u8_*, mvgx_cascade_*
// Every context: create, regions of 0 / 5 / 70 descriptors, all ordered pairs in batches small enough for two or more, regions of
// 0 / 130 / 70 descriptors (the buffers regrow), the pairs again, destroy. Then the same with the emulation's allocation-failure
// injection (HIPEMU_FAIL_MALLOC_AFTER) at the first allocation of the sequence, at one inside set_regions and at one inside run: the call
// must report an error and the context must still destroy cleanly. Exit status 0 = every step behaved.
#ifdef LIFETIME_MATCH
#include "hipemu_match.cpp"
#else
#include "hipemu.cpp"
#endif

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <set>
#include <string>
#include <vector>

namespace lifetime {

int g_failed = 0;
#define EXPECT(cond, ...)                                                     \
  do {                                                                        \
    if (!(cond)) { fprintf(stderr, "context_lifetime: " __VA_ARGS__); fputc('\n', stderr); ++g_failed; } \
  } while (0)

// images of n[k] rows of `row_bytes` bytes (float rows: small integers as floats, any bit pattern would do for a lifetime check)
struct Regions {
  std::vector<std::vector<uint8_t>> rows;
  std::vector<const uint8_t*> ptr;
  std::vector<uint32_t> n;
  Regions(std::vector<uint32_t> counts, uint32_t row_bytes, bool as_float) : n(counts) {
    uint32_t s = 12345u;
    for (uint32_t c : n) {
      rows.emplace_back((size_t)c * row_bytes);
      for (size_t i = 0; i < rows.back().size(); ++i) { s = s * 1664525u + 1013904223u; rows.back()[i] = (uint8_t)(s >> 24); }
      if (as_float) {
        float* f = reinterpret_cast<float*>(rows.back().data());
        for (size_t i = 0; i < rows.back().size() / 4; ++i) { s = s * 1664525u + 1013904223u; f[i] = (float)(s >> 24); }
      }
      ptr.push_back(c ? rows.back().data() : nullptr);
    }
  }
};

const uint32_t kPairs[12] = {0, 1, 0, 2, 1, 0, 1, 2, 2, 0, 2, 1};   // all ordered pairs of three images
constexpr uint64_t kNPairs = 6;

// one context kind behind the same four calls
struct Kind {
  const char* name;
  uint32_t row_bytes;
  bool as_float;
  std::function<int(void**)> create;
  std::function<int(void*, const Regions&)> set_regions;
  std::function<int(void*)> run;
  std::function<int(void*)> destroy;
};

// after >= 0: allocation number `after` (from 0) of what follows fails, and every later one; -1: none
void inject(int after) {
  unsetenv("HIPEMU_FAIL_MALLOC_AFTER");
  void* p = nullptr;   // (the emulation restarts its count at an allocation made while the variable is unset)
  if (hipMalloc(&p, 16) == hipSuccess) (void)hipFree(p);
  if (after >= 0) setenv("HIPEMU_FAIL_MALLOC_AFTER", std::to_string(after).c_str(), 1);
}

// fail_stage: -1 none; 0 from create on (the first allocation of the sequence); 1 inside the first set_regions; 2 inside the first run
void sequence(const Kind& k, int fail_stage, int fail_after) {
  const Regions a({0, 5, 70}, k.row_bytes, k.as_float), b({0, 130, 70}, k.row_bytes, k.as_float);
  void* c = nullptr;
  bool failed = false;
  auto step = [&](int stage, const char* what, const std::function<int()>& call) {
    if (failed) return;
    if (stage == fail_stage) inject(fail_after);
    const int rc = call();
    if (fail_stage < 0) EXPECT(rc == 0, "%s: %s returned %d (%s)", k.name, what, rc, mvgx_last_error());
    else if (rc != 0) failed = true;
    // an injected failure at stage 1 or 2 must surface in that very call
    if (fail_stage >= 1 && stage == fail_stage) EXPECT(rc != 0, "%s: %s succeeded with its allocation %d failing", k.name, what, fail_after);
    if (failed) inject(-1);
  };
  step(0, "create", [&] { return k.create(&c); });
  step(1, "set_regions", [&] { return k.set_regions(c, a); });
  step(2, "run", [&] { return k.run(c); });
  step(3, "set_regions (regrow)", [&] { return k.set_regions(c, b); });
  step(4, "run (regrown)", [&] { return k.run(c); });
  inject(-1);
  if (fail_stage >= 0) EXPECT(failed, "%s: no call reported the injected allocation failure (stage %d, allocation %d)", k.name, fail_stage, fail_after);
  if (c) EXPECT(k.destroy(c) == 0, "%s: destroy failed", k.name);
}

void all_sequences(const Kind& k) {
  sequence(k, -1, 0);
  sequence(k, 0, 0);
  sequence(k, 1, 2);
  sequence(k, 2, 2);
}

#ifdef LIFETIME_MATCH
struct SinkLog { std::set<const uint32_t*> buffers; uint64_t matches = 0; };
int sink(void* user, uint64_t, uint32_t nb, const uint32_t* offsets, const uint32_t* ij) {
  auto* log = static_cast<SinkLog*>(user);
  if (offsets[nb]) { log->buffers.insert(ij); log->matches += offsets[nb]; }
  return 0;
}

Kind match_kind(const char* name, const char* option, int64_t value) {
  Kind k{name, 128, false, nullptr, nullptr, nullptr, nullptr};
  k.create = [=](void** out) {
    mvgx_match_ctx* c = nullptr;
    int rc = mvgx_match_create(0, &c);
    if (!rc && option) rc = mvgx_match_set_option(c, option, value);
    if (!rc) rc = mvgx_match_set_option(c, "batch_pairs", 4);
    if (rc && c) { mvgx_match_destroy(c); c = nullptr; }
    *out = c;
    return rc;
  };
  k.set_regions = [](void* c, const Regions& r) { return mvgx_match_set_regions(static_cast<mvgx_match_ctx*>(c), r.ptr.data(), r.n.data(), 3, 128); };
  k.run = [](void* c) { return mvgx_match_run(static_cast<mvgx_match_ctx*>(c), kPairs, kNPairs, 1.0f, nullptr); };
  k.destroy = [](void* c) { return mvgx_match_destroy(static_cast<mvgx_match_ctx*>(c)); };
  return k;
}

// mvgx_match_run_stream with "stream_hold": one pair per batch, so the slot of the odd batches delivers (1, 2) and (2, 1) from its two sets
// of host buffers - both must go with the context
void stream_hold() {
  for (int pinned = 0; pinned <= 1; ++pinned) {
    const Regions a({0, 5, 70}, 128, false);
    mvgx_match_ctx* c = nullptr;
    SinkLog log;
    int rc = mvgx_match_create(0, &c);
    if (!rc) rc = mvgx_match_set_option(c, "batch_pairs", 1);
    if (!rc) rc = mvgx_match_set_option(c, "stream_hold", 1);
    if (!rc) rc = mvgx_match_set_option(c, "pinned_stream", pinned);
    if (!rc) rc = mvgx_match_set_regions(c, a.ptr.data(), a.n.data(), 3, 128);
    if (!rc) rc = mvgx_match_run_stream(c, kPairs, kNPairs, 1.0f, sink, &log, nullptr);
    EXPECT(rc == 0, "stream_hold (pinned %d): returned %d (%s)", pinned, rc, mvgx_last_error());
    EXPECT(log.buffers.size() >= 2 && log.matches > 0, "stream_hold (pinned %d): %zu host buffers delivered %llu matches - both sets were to be used",
           pinned, log.buffers.size(), (unsigned long long)log.matches);
    if (c) EXPECT(mvgx_match_destroy(c) == 0, "stream_hold: destroy failed");
  }
}
#else
template <typename Ctx>
Kind bf_kind(const char* name, uint32_t row_bytes, bool as_float, int (*create)(int, Ctx**), int (*set_option)(Ctx*, const char*, int64_t),
             std::function<int(Ctx*, const Regions&)> set_regions, int (*run)(Ctx*, const uint32_t*, uint64_t, float, mvgx_match_stats*), int (*destroy)(Ctx*)) {
  Kind k{name, row_bytes, as_float, nullptr, nullptr, nullptr, nullptr};
  k.create = [=](void** out) {
    Ctx* c = nullptr;
    int rc = create(0, &c);
    if (!rc) rc = set_option(c, "batch_pairs", 4);
    if (rc && c) { destroy(c); c = nullptr; }
    *out = c;
    return rc;
  };
  k.set_regions = [=](void* c, const Regions& r) { return set_regions(static_cast<Ctx*>(c), r); };
  k.run = [=](void* c) { return run(static_cast<Ctx*>(c), kPairs, kNPairs, 1.0f, nullptr); };
  k.destroy = [=](void* c) { return destroy(static_cast<Ctx*>(c)); };
  return k;
}
#endif

}  // namespace lifetime

int main() {
  using namespace lifetime;
  inject(-1);
#ifdef LIFETIME_MATCH
  all_sequences(match_kind("match (default)", nullptr, 0));
  all_sequences(match_kind("match (filter_shape 17)", "filter_shape", 17));
  all_sequences(match_kind("match (variant 1)", "variant", 1));
  stream_hold();
#else
  all_sequences(bf_kind<mvgx_hamming_ctx>("hamming", 64, false, mvgx_hamming_create, mvgx_hamming_set_option,
      [](mvgx_hamming_ctx* c, const Regions& r) { return mvgx_hamming_set_regions(c, r.ptr.data(), r.n.data(), 3, 64); }, mvgx_hamming_run, mvgx_hamming_destroy));
  all_sequences(bf_kind<mvgx_l2f_ctx>("l2f", 256, true, mvgx_l2f_create, mvgx_l2f_set_option,
      [](mvgx_l2f_ctx* c, const Regions& r) { return mvgx_l2f_set_regions(c, reinterpret_cast<const float* const*>(r.ptr.data()), r.n.data(), 3, 64); },
      mvgx_l2f_run, mvgx_l2f_destroy));
  all_sequences(bf_kind<mvgx_l2u8_ctx>("l2u8", 144, false, mvgx_l2u8_create, mvgx_l2u8_set_option,
      [](mvgx_l2u8_ctx* c, const Regions& r) { return mvgx_l2u8_set_regions(c, r.ptr.data(), r.n.data(), 3, 144); }, mvgx_l2u8_run, mvgx_l2u8_destroy));
  static const float zero_mean[128] = {};
  all_sequences(bf_kind<mvgx_cascade_ctx>("cascade", 128, false, mvgx_cascade_create, mvgx_cascade_set_option,
      [](mvgx_cascade_ctx* c, const Regions& r) { return mvgx_cascade_hash_regions(c, r.ptr.data(), r.n.data(), 3, 128, zero_mean, 2, 3, 7, nullptr, nullptr); },
      mvgx_cascade_run, mvgx_cascade_destroy));
#endif
  if (g_failed) { fprintf(stderr, "context_lifetime: %d check(s) failed\n", g_failed); return 1; }
  printf("context_lifetime: ok\n");
  return 0;
}
