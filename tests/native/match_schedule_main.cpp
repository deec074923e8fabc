// Stand-alone check of the two host decisions around the matching filter's launches (openmvg_amd/csrc/mvgx_match_batch.h, plain C++):
// mvgx_records::batch_schedule, the cut of a run into batches with ramps at its two ends, and mvgx_records::order_records, the order
// of the records inside an XCD's slice. Built with -fsanitize=address,undefined and run by tests/test_match_schedule_cpu.py.
//
//   match_schedule_main <cases file>           the checks; the file is that of match_records_main (image rows, then pair lists)
//   match_schedule_main n_pairs B nd ramp_min  prints the schedule, one "p0 nb" per line
//
// Schedule, for n_pairs in {0, 1, 4B-1, 4B, 4B+1, 499500} x B in {3, 64, 8192, 31218} x nd in {1, 2, 8} x ramp_min in {0, 8, 1024}:
//   - p0 starts at 0 and every batch starts where the one before ended; the sizes add up to n_pairs; 1 <= nb <= B
//   - inactive (ramp_min = 0, B / 8 < ramp_min or n_pairs < 4 B): steps of exactly B, the last one shorter
//   - active: B/8, B/4, B/2 each rep times, ceil(mid / B) middle batches whose sizes differ by at most 1, B/2, B/4, B/8 each rep times;
//     1 <= rep <= nd, rep = nd wherever that leaves the middle B pairs; no batch below ramp_min
//   - 499500 pairs at B = 31218 on one device: 21 batches
// Order, over the batches of the file's lists, over random lists of images large enough for many chunks, and over the first 0 .. 17
// records of such lists:
//   - every slice of the output (the slices of xcd_remap) is the stable sort by key of the same slice of the input, so the output is a
//     permutation of the input's 144-byte records, no record leaves its slice and the keys do not decrease inside a slice
//   - a slice whose records share one database image is the input's
#define MVGX_MATCH_BATCH_RECORDS_ONLY
#include "mvgx_match_batch.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace mvgx_records;

#define REQUIRE(cond, ...)                                                   \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "match_schedule: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

// ------------------------------------------------------------------------------------------------
// the schedule
// ------------------------------------------------------------------------------------------------
static unsigned long long g_schedules = 0, g_active = 0, g_fewer_reps = 0;

static void check_schedule(uint64_t n, uint64_t B, uint32_t nd, uint64_t ramp_min) {
  const std::vector<BatchSpan> s = batch_schedule(n, B, nd, ramp_min);
  uint64_t at = 0;
  for (size_t k = 0; k < s.size(); ++k) {
    REQUIRE(s[k].p0 == at && s[k].nb >= 1 && s[k].nb <= B, "n %llu B %llu nd %u floor %llu: batch %zu = (%llu, %u) at %llu", (unsigned long long)n,
            (unsigned long long)B, nd, (unsigned long long)ramp_min, k, (unsigned long long)s[k].p0, s[k].nb, (unsigned long long)at);
    at += s[k].nb;
  }
  REQUIRE(at == n, "n %llu B %llu nd %u floor %llu: %llu pairs covered", (unsigned long long)n, (unsigned long long)B, nd,
          (unsigned long long)ramp_min, (unsigned long long)at);
  const bool active = ramp_min > 0 && B / 8 >= ramp_min && n >= 4 * B;   // the rule, restated
  REQUIRE(active == batch_ramp_active(n, B, ramp_min), "active");
  ++g_schedules;
  if (!active) {
    REQUIRE(s.size() == (n + B - 1) / B, "inactive: %zu batches", s.size());
    for (size_t k = 0; k < s.size(); ++k)
      REQUIRE(s[k].p0 == k * B && s[k].nb == std::min<uint64_t>(B, n - k * B), "inactive: batch %zu = (%llu, %u)", k, (unsigned long long)s[k].p0, s[k].nb);
    return;
  }
  ++g_active;
  const uint64_t steps[3] = {B / 8, B / 4, B / 2}, ramp = B / 8 + B / 4 + B / 2;
  size_t rep = 0;
  while (rep < s.size() && s[rep].nb == steps[0]) ++rep;   // (B / 8 < B / 4, and no middle batch is below B / 2)
  REQUIRE(rep >= 1 && rep <= nd && s.size() >= 6 * rep, "rep %zu of %u, %zu batches", rep, nd, s.size());
  REQUIRE(n >= B + 2 * rep * ramp, "rep %zu leaves the middle less than B", rep);
  if (rep < nd) { REQUIRE(n < B + 2 * (rep + 1) * ramp, "rep %zu of %u although one more fits", rep, nd); ++g_fewer_reps; }
  for (int st = 0; st < 3; ++st)
    for (size_t r = 0; r < rep; ++r) {
      REQUIRE(s[st * rep + r].nb == steps[st], "head step %d", st);
      REQUIRE(s[s.size() - 1 - (st * rep + r)].nb == steps[st], "tail step %d", st);
    }
  const uint64_t mid = n - 2 * rep * ramp;
  const size_t n_mid = s.size() - 6 * rep;
  REQUIRE(n_mid == (mid + B - 1) / B, "%zu middle batches for %llu pairs", n_mid, (unsigned long long)mid);
  uint32_t lo = UINT32_MAX, hi = 0;
  for (size_t k = 3 * rep; k < 3 * rep + n_mid; ++k) { lo = std::min(lo, s[k].nb); hi = std::max(hi, s[k].nb); }
  REQUIRE(hi - lo <= 1 && lo >= B / 2, "middle batches of %u .. %u", lo, hi);
  for (const BatchSpan& b : s) REQUIRE(b.nb >= ramp_min, "a batch of %u below the floor %llu", b.nb, (unsigned long long)ramp_min);
}

static void check_schedules() {
  const uint64_t Bs[] = {3, 64, 8192, 31218}, floors[] = {0, 8, 1024};
  const uint32_t nds[] = {1, 2, 8};
  for (uint64_t B : Bs)
    for (uint32_t nd : nds)
      for (uint64_t ramp_min : floors) {
        const uint64_t ns[] = {0, 1, 4 * B - 1, 4 * B, 4 * B + 1, 499500};
        for (uint64_t n : ns) check_schedule(n, B, nd, ramp_min);
        for (uint64_t n = 0; n < 40 * B; n += 1 + B / 3) check_schedule(n, B, nd, ramp_min);   // ... and every repetition count on the way to nd
      }
  REQUIRE(batch_schedule(499500, 31218, 1, 1024).size() == 21, "the benchmark's run has %zu batches", batch_schedule(499500, 31218, 1, 1024).size());
  REQUIRE(batch_schedule(4 * 8192, 8192, 1, 1024)[0].nb == 1024 && batch_schedule(4 * 8192 - 1, 8192, 1, 1024)[0].nb == 8192, "threshold at 4 B");
  REQUIRE(batch_schedule(40000, 4096, 1, 1024)[0].nb == 4096, "B / 8 below the floor");
  REQUIRE(g_active > 100 && g_fewer_reps > 10, "%llu active schedules, %llu with fewer repetitions than devices", g_active, g_fewer_reps);
}

// ------------------------------------------------------------------------------------------------
// the record order
// ------------------------------------------------------------------------------------------------
struct Images {
  std::vector<uint32_t> n, tile_off, ntiles, qtile_off;
  explicit Images(const std::vector<uint32_t>& rows) : n(rows) {
    tile_off.assign(n.size() + 1, 0); qtile_off.assign(n.size() + 1, 0); ntiles.assign(n.size(), 0);
    for (size_t k = 0; k < n.size(); ++k) {
      ntiles[k] = (n[k] + 31) / 32 + 1;
      tile_off[k + 1] = tile_off[k] + ntiles[k] + 1;        // a different first tile for every image
      qtile_off[k + 1] = qtile_off[k] + (n[k] + 31) / 32;
    }
  }
  ImageTables tables() const { return ImageTables{n.data(), tile_off.data(), ntiles.data(), qtile_off.data()}; }
};

constexpr size_t kWords = (size_t)4 * kRecQuads;
using Record = std::array<uint32_t, kWords>;
static unsigned long long g_lists = 0, g_sorted_slices = 0, g_kept_slices = 0, g_moved = 0, g_max_keys = 0;

static void check_order(const Images& im, uint32_t chunk_tiles, const uint32_t* ij, const uint32_t* rec, uint32_t n_rec) {
  static_assert(sizeof(Record) == 144, "a record is 144 bytes");
  std::vector<uint32_t> dst(kWords * n_rec), count;   // exactly n_rec records: one word more written is a heap overflow report
  order_records(im.qtile_off.data(), chunk_tiles, ij, rec, n_rec, dst.data(), count);
  auto key = [&](const Record& r) { return im.qtile_off[ij[2 * r[4] + 1]] / chunk_tiles; };
  uint32_t covered = 0;
  for (uint32_t xcd = 0; xcd < 8; ++xcd) {
    uint32_t first, n;
    xcd_slice(n_rec, xcd, first, n);
    REQUIRE(first == covered && n == n_rec / 8 + (xcd < n_rec % 8 ? 1 : 0), "slice %u of %u records: %u + %u", xcd, n_rec, first, n);
    covered += n;
    std::vector<Record> in(n), out(n);
    if (n) { std::memcpy(in.data(), rec + kWords * first, n * sizeof(Record)); std::memcpy(out.data(), dst.data() + kWords * first, n * sizeof(Record)); }
    bool one_image = true;
    for (const Record& r : in) one_image = one_image && r[0] == in[0][0];
    if (one_image) {
      REQUIRE(in == out, "slice %u of %u records: one database image, yet changed", xcd, n_rec);
      g_kept_slices += n > 0;
      continue;
    }
    std::vector<Record> want = in;
    std::stable_sort(want.begin(), want.end(), [&](const Record& a, const Record& b) { return key(a) < key(b); });
    REQUIRE(want == out, "slice %u of %u records is not the stable sort of the input's by key", xcd, n_rec);
    for (uint32_t k = 0; k + 1 < n; ++k) REQUIRE(key(out[k]) <= key(out[k + 1]), "slice %u: keys decrease at %u", xcd, k);
    ++g_sorted_slices;
    for (uint32_t k = 0; k < n; ++k) g_moved += in[k] != out[k];
    g_max_keys = std::max<unsigned long long>(g_max_keys, key(out[n - 1]) - key(out[0]) + 1);
  }
  REQUIRE(covered == n_rec, "slices cover %u of %u records", covered, n_rec);
  std::vector<Record> a(n_rec), b(n_rec);   // (implied by the above; stated on its own: the multisets of records are equal)
  if (n_rec) { std::memcpy(a.data(), rec, n_rec * sizeof(Record)); std::memcpy(b.data(), dst.data(), n_rec * sizeof(Record)); }
  std::sort(a.begin(), a.end()); std::sort(b.begin(), b.end());
  REQUIRE(a == b, "%u records: not a permutation", n_rec);
  ++g_lists;
}

static void check_order_batches(const Images& im, uint32_t chunk_tiles, const std::vector<uint32_t>& ij, uint32_t batch_pairs, bool prefixes) {
  const uint32_t n_pairs = (uint32_t)(ij.size() / 2);
  for (uint32_t k0 = 0; k0 < n_pairs; k0 += batch_pairs) {
    const uint32_t nb = std::min(batch_pairs, n_pairs - k0);
    size_t cap = 0;
    for (uint32_t k = 0; k < nb; ++k)
      if (pair_has_work(im.n.data(), ij[2 * (k0 + k)], ij[2 * (k0 + k) + 1])) cap += ((im.n[ij[2 * (k0 + k) + 1]] + kBlockRows - 1) / kBlockRows + 31) / 32;
    std::vector<uint32_t> rec(cap * kWords);
    const uint32_t n_rec = build_block_records(im.tables(), ij.data() + 2 * k0, nb, rec.data());
    REQUIRE(n_rec <= cap, "%u records, bound %zu", n_rec, cap);
    check_order(im, chunk_tiles, ij.data() + 2 * k0, rec.data(), n_rec);
    if (prefixes)
      for (uint32_t m = 0; m <= 17 && m <= n_rec; ++m) {
        const std::vector<uint32_t> head(rec.begin(), rec.begin() + kWords * m);   // its own allocation of exactly m records
        check_order(im, chunk_tiles, ij.data() + 2 * k0, head.data(), m);
      }
  }
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*: [0, n)
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

static void print_schedule(char** argv) {
  const std::vector<BatchSpan> s = batch_schedule(std::strtoull(argv[1], nullptr, 10), std::strtoull(argv[2], nullptr, 10),
                                                  (uint32_t)std::strtoul(argv[3], nullptr, 10), std::strtoull(argv[4], nullptr, 10));
  for (const BatchSpan& b : s) std::printf("%llu %u\n", (unsigned long long)b.p0, b.nb);
}

int main(int argc, char** argv) {
  if (argc == 5) { print_schedule(argv); return 0; }
  REQUIRE(argc == 2, "usage: match_schedule_main <cases file> | n_pairs B nd ramp_min");
  check_schedules();

  std::FILE* f = std::fopen(argv[1], "r");
  REQUIRE(f, "cannot open %s", argv[1]);
  unsigned v = 0, n_images = 0;
  REQUIRE(std::fscanf(f, "%u", &n_images) == 1 && n_images > 0, "no image count");
  std::vector<uint32_t> rows(n_images);
  for (auto& r : rows) { REQUIRE(std::fscanf(f, "%u", &v) == 1, "short image list"); r = v; }
  const Images im(rows);
  unsigned file_cases = 0, batch_pairs = 0, n_pairs = 0;
  while (std::fscanf(f, "%u %u", &batch_pairs, &n_pairs) == 2) {
    REQUIRE(batch_pairs > 0, "batch_pairs 0");
    std::vector<uint32_t> ij(2 * (size_t)n_pairs);
    for (auto& x : ij) { REQUIRE(std::fscanf(f, "%u", &v) == 1 && v < n_images, "bad pair list"); x = v; }
    check_order_batches(im, 4, ij, batch_pairs, batch_pairs >= n_pairs);   // (the file's images have at most 8 dense tiles)
    check_order_batches(im, kOrderChunkTiles, ij, batch_pairs, false);
    ++file_cases;
  }
  std::fclose(f);
  REQUIRE(file_cases > 0, "no cases in %s", argv[1]);

  // random sets: images of up to 6000 rows (188 dense tiles: a chunk holds a few of them, a set many chunks) among tiny and empty ones;
  // exhaustive lists (runs of one database image, several per slice), mirrored and shuffled ones, whole and in batches
  for (int set = 0; set < 60; ++set) {
    const uint32_t n = 4 + rnd(28);
    std::vector<uint32_t> r(n);
    for (auto& x : r) x = rnd(5) == 0 ? rnd(34) : 200 + rnd(5801);
    const Images ri(r);
    std::vector<uint32_t> ij;
    for (uint32_t i = 0; i < n; ++i)
      for (uint32_t j = i + 1; j < n; ++j) { ij.push_back(i); ij.push_back(j); }
    if (set % 2) {
      const size_t m = ij.size();
      for (size_t k = 0; k < m; k += 2) { ij.push_back(ij[k + 1]); ij.push_back(ij[k]); }
    }
    if (set % 5 == 4)
      for (size_t k = ij.size() / 2; k > 1; --k) {
        const size_t o = rnd((uint32_t)k);
        std::swap(ij[2 * (k - 1)], ij[2 * o]); std::swap(ij[2 * (k - 1) + 1], ij[2 * o + 1]);
      }
    const uint32_t np = (uint32_t)(ij.size() / 2);
    check_order_batches(ri, kOrderChunkTiles, ij, np, set < 10);
    check_order_batches(ri, kOrderChunkTiles, ij, 1 + rnd(np), false);
    check_order_batches(ri, 1 + rnd(500), ij, np, false);
  }
  REQUIRE(g_sorted_slices > 500 && g_kept_slices > 50 && g_moved > 10000 && g_max_keys >= 8,
          "the lists do not exercise the order: %llu slices sorted, %llu kept, %llu records moved, %llu keys in one slice", g_sorted_slices,
          g_kept_slices, g_moved, g_max_keys);
  std::printf("match_schedule: ok (%llu schedules, %llu with ramps; %u file cases, %llu record lists, %llu slices sorted, %llu kept, %llu records moved)\n",
              g_schedules, g_active, file_cases, g_lists, g_sorted_slices, g_kept_slices, g_moved);
  return 0;
}
