// Stand-alone check of the block-granular record builder (openmvg_amd/csrc/mvgx_match_batch.h, mvgx_records::build_block_records): the
// builder is plain C++, so this program needs neither HIP nor its emulation. Built with -fsanitize=address,undefined and run by
// tests/test_match_block_records_cpu.py.
//
//   match_records_main <cases file>
//
// The file holds whitespace-separated numbers: n_images, the rows of each image, then cases until the end: batch_pairs, n_pairs, and
// 2 * n_pairs image indices. Every case is cut into batches of batch_pairs as the matcher cuts them. After the file's cases the program
// runs random image sets and pair lists of its own. For every batch it decodes the records exactly as the kernels do and requires:
//   - every (pair, block) with work is covered exactly once, and nothing else is
//   - a unit holds at most two segments and at most 8 blocks; segment A's blocks exist in its image; a second segment only after a first
//   - all units of a record have the record's database image; absent segments point at that image's own dense tiles
//   - the output never exceeds one record per 32 blocks (rounded up) of every pair with work - the size of the buffer it is given
//   - when no image has fewer than 8 blocks: units = sum over the runs of one database image of ceil(blocks / 8), records = ceil(units / 4)
#define MVGX_MATCH_BATCH_RECORDS_ONLY
#include "mvgx_match_batch.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

using namespace mvgx_records;

#define REQUIRE(cond, ...)                                                   \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "match_records: %s:%d: %s: ", __FILE__, __LINE__, #cond); \
      std::fprintf(stderr, __VA_ARGS__);                                     \
      std::fprintf(stderr, "\n");                                            \
      std::exit(1);                                                          \
    }                                                                        \
  } while (0)

struct Images {
  std::vector<uint32_t> n, tile_off, ntiles, qtile_off;
  explicit Images(const std::vector<uint32_t>& rows) : n(rows) {
    tile_off.assign(n.size() + 1, 0); qtile_off.assign(n.size() + 1, 0); ntiles.assign(n.size(), 0);
    for (size_t k = 0; k < n.size(); ++k) {
      ntiles[k] = (n[k] + 31) / 32 + 1;                     // the parity tiles are copied, not interpreted: any distinct layout does
      tile_off[k + 1] = tile_off[k] + ntiles[k] + 1;        // ... with a different first tile for every image
      qtile_off[k + 1] = qtile_off[k] + (n[k] + 31) / 32;
    }
  }
  ImageTables tables() const { return ImageTables{n.data(), tile_off.data(), ntiles.data(), qtile_off.data()}; }
  uint32_t blocks(uint32_t img) const { return (n[img] + kBlockRows - 1) / kBlockRows; }
};

static unsigned long long g_units = 0, g_records = 0, g_batches = 0, g_two_segment_units = 0;

static void check_batch(const Images& im, const uint32_t* ij, uint32_t nb) {
  size_t cap = 0;
  bool all_large = true;
  for (uint32_t k = 0; k < nb; ++k) {
    if (!pair_has_work(im.n.data(), ij[2 * k], ij[2 * k + 1])) continue;
    cap += (im.blocks(ij[2 * k + 1]) + 31) / 32;
    all_large = all_large && im.blocks(ij[2 * k + 1]) >= (uint32_t)kUnitBlocks;
  }
  std::vector<uint32_t> out(cap * 4 * kRecQuads);   // exactly the bound: one word more written is a heap overflow report
  const uint32_t n_rec = build_block_records(im.tables(), ij, nb, out.data());
  REQUIRE(n_rec <= cap, "%u records, bound %zu", n_rec, cap);

  std::map<std::pair<uint32_t, uint32_t>, int> seen;   // (pair, block) -> times covered
  uint32_t units = 0;
  for (uint32_t r = 0; r < n_rec; ++r) {
    const uint32_t* rec = out.data() + (size_t)4 * kRecQuads * r;
    uint32_t rec_I = UINT32_MAX;
    bool open = true;   // units of a record are filled from wave 0 on
    for (int w = 0; w < kRecWaves; ++w) {
      const uint32_t* a = rec + 4 * (1 + 2 * w);
      const uint32_t* b = a + 4;
      const uint32_t split = b[2];
      if (a[3] == 0) {   // an empty wave
        REQUIRE(b[3] == 0 && split == 0 && w > 0, "record %u wave %d: a second segment without a first, or an empty first wave", r, w);
        open = false;
      } else {
        REQUIRE(open, "record %u wave %d: a unit after an empty wave", r, w);
        REQUIRE(split >= 1 && split <= (uint32_t)kUnitBlocks, "record %u wave %d: split %u", r, w, split);
        ++units;
        if (b[3]) ++g_two_segment_units;
      }
      const uint32_t* segs[2] = {a, b};
      for (int s = 0; s < 2; ++s) {
        const uint32_t* g = segs[s];
        if (g[3] == 0) {   // absent: aimed at the database image's own dense tiles (rec_I is known by the first wave's segment A)
          REQUIRE(rec_I != UINT32_MAX && g[1] == im.qtile_off[rec_I], "record %u wave %d segment %d: dead pointer %u", r, w, s, g[1]);
          continue;
        }
        REQUIRE(g[0] < nb, "record %u wave %d: pair %u of %u", r, w, g[0], nb);
        const uint32_t I = ij[2 * g[0]], J = ij[2 * g[0] + 1];
        REQUIRE(pair_has_work(im.n.data(), I, J), "record %u wave %d: pair %u has no work", r, w, g[0]);
        if (rec_I == UINT32_MAX) rec_I = I;
        REQUIRE(I == rec_I && rec[0] == im.tile_off[I] && rec[1] == im.ntiles[I], "record %u wave %d: database image %u in a record of %u", r, w, I, rec_I);
        REQUIRE(g[1] == im.qtile_off[J] && g[3] == im.n[J], "record %u wave %d: query image tables", r, w);
        if (s == 0) REQUIRE(g[2] + split <= im.blocks(J), "record %u wave %d: segment A blocks %u + %u of %u", r, w, g[2], split, im.blocks(J));
      }
      // the kernels' decoding: block n of the unit is block a.z + n of A below the split, block n - split of B from it on; rows below nJ count
      uint32_t unit_blocks = 0;
      for (uint32_t n = 0; n < (uint32_t)kUnitBlocks; ++n) {
        const bool inA = n < split;
        const uint32_t* g = inA ? a : b;
        const uint32_t blk = inA ? a[2] + n : n - split;
        if (blk * kBlockRows < g[3]) { ++seen[{g[0], blk}]; ++unit_blocks; }
      }
      REQUIRE(unit_blocks <= (uint32_t)kUnitBlocks && (a[3] == 0) == (unit_blocks == 0), "record %u wave %d: %u blocks", r, w, unit_blocks);
    }
  }
  size_t want = 0;
  unsigned long long run_units = 0, run_blocks = 0, want_units = 0, want_records = 0;
  uint32_t run_I = UINT32_MAX;
  auto close_run = [&] {
    run_units = (run_blocks + kUnitBlocks - 1) / kUnitBlocks;
    want_units += run_units; want_records += (run_units + kRecWaves - 1) / kRecWaves;
    run_blocks = 0;
  };
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t I = ij[2 * k], J = ij[2 * k + 1];
    if (!pair_has_work(im.n.data(), I, J)) continue;
    if (I != run_I) { close_run(); run_I = I; }
    run_blocks += im.blocks(J);
    for (uint32_t blk = 0; blk < im.blocks(J); ++blk) {
      auto it = seen.find({k, blk});
      REQUIRE(it != seen.end() && it->second == 1, "pair %u block %u covered %d times", k, blk, it == seen.end() ? 0 : it->second);
      ++want;
    }
  }
  close_run();
  REQUIRE(seen.size() == want, "%zu (pair, block) covered, %zu have work", seen.size(), want);
  if (all_large) REQUIRE(units == want_units && n_rec == want_records, "%u units (want %llu), %u records (want %llu)", units, want_units, n_rec, want_records);
  g_units += units; g_records += n_rec; ++g_batches;
}

static void check_case(const Images& im, const std::vector<uint32_t>& ij, uint32_t batch_pairs) {
  const uint32_t n_pairs = (uint32_t)(ij.size() / 2);
  for (uint32_t k0 = 0; k0 < n_pairs; k0 += batch_pairs) check_batch(im, ij.data() + 2 * k0, std::min(batch_pairs, n_pairs - k0));
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {   // xorshift64*: [0, n)
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (uint32_t)(((g_rng * 0x2545F4914F6CDD1Dull) >> 33) % n);
}

int main(int argc, char** argv) {
  REQUIRE(argc == 2, "usage: match_records_main <cases file>");
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
    check_case(im, ij, batch_pairs);
    ++file_cases;
  }
  std::fclose(f);
  REQUIRE(file_cases > 0, "no cases in %s", argv[1]);

  // random sets: ragged images of 0 .. 40 blocks (a third of the sets: none below 8 blocks, so that the unit count is the derived one),
  // exhaustive, mirrored and shuffled lists, batches from 1 pair to the whole list
  for (int set = 0; set < 300; ++set) {
    const uint32_t n = 2 + rnd(14);
    const bool large = set % 3 == 0;
    std::vector<uint32_t> r(n);
    for (auto& x : r) x = large ? 113 + rnd(528) : (rnd(4) == 0 ? rnd(34) : rnd(641));
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
    check_case(ri, ij, np);
    check_case(ri, ij, 1 + rnd(np));
    check_case(ri, ij, 1 + rnd(9));
  }
  REQUIRE(g_two_segment_units > 1000, "only %llu units of two segments: the random sets do not exercise the packing", g_two_segment_units);
  std::printf("match_records: ok (%u file cases, %llu batches, %llu records, %llu units, %llu of two segments)\n", file_cases, g_batches, g_records,
              g_units, g_two_segment_units);
  return 0;
}
