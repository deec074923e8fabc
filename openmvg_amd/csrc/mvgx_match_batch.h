// What every matcher's batch loop shares (mvgx_match.hip, mvgx_bruteforce.hip): the no-match sentinel of best[], the two kernels that
// turn best[] + per-pair counts into ordered match lists, the pairs-per-batch rule and the argument checks of a run. In front of them,
// in plain C++: the work records of mvgx_match.hip's default filter, their order inside an XCD's slice and the batch schedule of its runs.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

// ------------------------------------------------------------------------------------------------
// The block-granular records of l2_filter16_kernel and the two kernels that walk the same units (MatchParams::work8).
// Plain C++ without a HIP header: with MVGX_MATCH_BATCH_RECORDS_ONLY defined this part is the whole file (tests/native/
// match_records_main.cpp runs it alone).
//
// The granule of the query side is the BLOCK of 16 query rows: block k of image J is dense tile k >> 1, half k & 1, rows 16 k .. 16 k + 15.
// A wave's unit is kUnitBlocks consecutive blocks of the block stream of the batch's pairs that share the database image I: up to two
// SEGMENTS, the tail of one pair's blocks (A) and the head of the next pair's (B, always from its block 0). Four units make a record. A
// unit is closed when it holds kUnitBlocks blocks, when I changes, at the end of the batch and when a third image would enter it (only
// images of fewer than kUnitBlocks blocks do that). A record is kRecQuads quads of four words:
//   quad 0              (tileI0, ntI, 0, 0)                                           shared by the workgroup
//   quad 1 + 2 w        (pair A, first dense tile of JA, first block in JA, nJA)       wave w, blocks n < split
//   quad 2 + 2 w        (pair B, first dense tile of JB, split = blocks of A, nJB)     wave w, block n >= split is block n - split of JB
// nJ = 0 marks an absent segment: its blocks take part in everything and store nothing, and its tile offset is I's own (mapped memory; a
// dead block reads at most four tiles from there, the slack after the last image covers them). A is filled first, so a unit without A is
// an empty wave. Everything a wave needs to start is in its record: no table walks.
// ------------------------------------------------------------------------------------------------
namespace mvgx_records {

constexpr int kRecWaves = 4;                    // units per record (= waves per workgroup)
constexpr int kUnitBlocks = 8;                  // blocks of 16 query rows per unit
constexpr int kBlockRows = 16;
constexpr int kRecQuads = 1 + 2 * kRecWaves;    // quads (4 x uint32) per record

struct ImageTables {            // per image, as prep_regions lays them out
  const uint32_t* n;            // descriptors
  const uint32_t* tile_off;     // first parity tile (database role)
  const uint32_t* ntiles;       // occupied parity tiles
  const uint32_t* qtile_off;    // first dense tile (query role)
};

// a pair with nJ > 0 and nI >= 2 has work, any other pair none:
// matcher_brute_force.hpp:108-113: NN(=2) > rows -> no result; Matcher_Regions.cpp:65-69,85-90: empty regions skipped
inline bool pair_has_work(const uint32_t* n, uint32_t I, uint32_t J) { return n[I] >= 2 && n[J] != 0; }

// Records of the batch of nb pairs ij[2 k], ij[2 k + 1], walked in order; `out` holds 4 * kRecQuads words per record. Returns the records
// written: at most the sum over the pairs with work of ceil(blocks of J / (kRecWaves * kUnitBlocks)) - a pair that opens a record fills
// its units to kUnitBlocks while its blocks last, a pair that enters an open record opens fewer.
inline uint32_t build_block_records(const ImageTables& im, const uint32_t* ij, uint32_t nb, uint32_t* out) {
  uint32_t n_rec = 0, rec_used = kRecWaves, unit_I = 0;   // records written; units taken in the open one (kRecWaves: none is open), its image
  uint32_t* unit = nullptr;                               // the open unit's two quads; nullptr: none is open
  uint32_t unit_blocks = 0, unit_segs = 0;
  for (uint32_t k = 0; k < nb; ++k) {
    const uint32_t I = ij[2 * k], J = ij[2 * k + 1];
    if (!pair_has_work(im.n, I, J)) continue;
    const uint32_t nblk = (im.n[J] + kBlockRows - 1) / kBlockRows;
    for (uint32_t blk = 0; blk < nblk;) {
      if (!unit || unit_I != I || unit_blocks == kUnitBlocks || unit_segs == 2) {
        if (rec_used == kRecWaves || unit_I != I) {
          uint32_t* r = out + (size_t)4 * kRecQuads * n_rec++;
          r[0] = im.tile_off[I]; r[1] = im.ntiles[I]; r[2] = 0; r[3] = 0;
          for (int q = 1; q < kRecQuads; ++q) { r[4 * q] = 0; r[4 * q + 1] = im.qtile_off[I]; r[4 * q + 2] = 0; r[4 * q + 3] = 0; }
          rec_used = 0;
        }
        unit = out + (size_t)4 * kRecQuads * (n_rec - 1) + 4 * (1 + 2 * rec_used++);
        unit_I = I; unit_blocks = 0; unit_segs = 0;
      }
      const uint32_t take = (nblk - blk < kUnitBlocks - unit_blocks) ? nblk - blk : kUnitBlocks - unit_blocks;
      uint32_t* seg = unit + 4 * unit_segs;   // B is entered only by a pair's first block: blk = 0 there
      seg[0] = k; seg[1] = im.qtile_off[J]; seg[3] = im.n[J];
      if (unit_segs == 0) { seg[2] = blk; unit[4 + 2] = take; }
      ++unit_segs; unit_blocks += take; blk += take;
    }
  }
  return n_rec;
}

// ------------------------------------------------------------------------------------------------
// The batches of a run. A run pipelines issue(b) | finish(b-1) | deliver(b-2); the host work and the upload of its
// first batch and the verify, scan, compaction and copy-out of its last one have no filter kernel to hide behind, and both grow with
// the size of that batch. So a run that is long enough starts and ends on small batches:
//   head    B/8, B/4, B/2, each `rep` times (one per device: every device has a pipeline of its own to fill)
//   middle  ceil(mid / B) batches whose sizes differ by at most 1 - no stub batch
//   tail    B/2, B/4, B/8, each `rep` times
// The ramp is active iff ramp_min > 0, B / 8 >= ramp_min and n_pairs >= 4 B; otherwise the steps are exactly B, the last one shorter.
// rep = nd where the run has room for it: the two ramps of one device take 2 (B/8 + B/4 + B/2) <= 1.75 B pairs, and at least B pairs
// are left to the middle, which keeps every middle batch at B / 2 or above. (n_pairs >= 4 B leaves room for one repetition; a run on eight
// devices needs 15 B pairs for all eight and gets fewer below that.)
// Every nb <= B, every pair is in exactly one batch, p0 increases, and no batch of an active schedule is below ramp_min.
// ------------------------------------------------------------------------------------------------
struct BatchSpan { uint64_t p0; uint32_t nb; };

inline bool batch_ramp_active(uint64_t n_pairs, uint64_t B, uint64_t ramp_min) {
  return ramp_min > 0 && B / 8 >= ramp_min && n_pairs >= 4 * B;
}

inline std::vector<BatchSpan> batch_schedule(uint64_t n_pairs, uint64_t B, uint32_t nd, uint64_t ramp_min) {
  std::vector<BatchSpan> out;
  if (B == 0) B = 1;
  uint64_t p0 = 0;
  auto put = [&](uint64_t nb) { out.push_back(BatchSpan{p0, (uint32_t)nb}); p0 += nb; };
  if (!batch_ramp_active(n_pairs, B, ramp_min)) {
    while (p0 < n_pairs) put(B < n_pairs - p0 ? B : n_pairs - p0);
    return out;
  }
  const uint64_t steps[3] = {B / 8, B / 4, B / 2};
  const uint64_t ramp = steps[0] + steps[1] + steps[2];
  uint64_t rep = (n_pairs - B) / (2 * ramp);   // >= 1: n_pairs - B >= 3 B > 2 ramp
  if (rep > nd) rep = nd ? nd : 1;
  const uint64_t mid = n_pairs - 2 * rep * ramp, n_mid = (mid + B - 1) / B;   // mid >= B
  for (int s = 0; s < 3; ++s)
    for (uint64_t r = 0; r < rep; ++r) put(steps[s]);
  for (uint64_t k = 0; k < n_mid; ++k) put(mid / n_mid + (k < mid % n_mid ? 1 : 0));
  for (int s = 2; s >= 0; --s)
    for (uint64_t r = 0; r < rep; ++r) put(steps[s]);
  return out;
}

// ------------------------------------------------------------------------------------------------
// Record order inside an XCD's slice. The kernels give XCD x the x-th of eight contiguous slices of the record list
// (xcd_remap: q = n >> 3 records each, one more in the first n & 7). The list is I-major, so a slice walks its database images one
// after the other and a query image comes back only with the next database image, thousands of records later. Ordered by the CHUNK of
// the query image instead - chunks cut the images at every kOrderChunkTiles dense query tiles - the workgroups resident together on an
// XCD read the same query tiles for all the database images of the slice. A stable counting sort per slice: records are independent, so
// any permutation gives the same lists; a slice of one database image is left as it is (its records already ascend in J when the pairs do).
// The key of a record is the chunk of ij[2 * pair A + 1] of wave 0 (a record always has that segment).
// ------------------------------------------------------------------------------------------------
constexpr uint32_t kOrderChunkTiles = 256;   // 1 MiB of dense query tiles (32 rows x 128 B each)

inline void xcd_slice(uint32_t n_rec, uint32_t xcd, uint32_t& first, uint32_t& count) {   // the records xcd_remap gives XCD `xcd`
  const uint32_t q = n_rec >> 3, r = n_rec & 7u;
  first = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  count = q + (xcd < r ? 1 : 0);
}

inline uint32_t record_order_key(const uint32_t* qtile_off, uint32_t chunk_tiles, const uint32_t* ij, const uint32_t* rec) {
  return qtile_off[ij[2 * rec[4] + 1]] / chunk_tiles;
}

// `src` -> `dst` (n_rec records each, not overlapping); chunk_tiles > 0: kOrderChunkTiles outside tests; `count` is scratch that the
// function sizes itself
inline void order_records(const uint32_t* qtile_off, uint32_t chunk_tiles, const uint32_t* ij, const uint32_t* src, uint32_t n_rec, uint32_t* dst,
                          std::vector<uint32_t>& count) {
  constexpr size_t kWords = (size_t)4 * kRecQuads;
  for (uint32_t xcd = 0; xcd < 8; ++xcd) {
    uint32_t first, n;
    xcd_slice(n_rec, xcd, first, n);
    if (!n) continue;
    const uint32_t* s = src + kWords * first;
    uint32_t* d = dst + kWords * first;
    bool one_image = true;
    uint32_t key_max = 0;
    for (uint32_t k = 0; k < n; ++k) {
      one_image = one_image && s[kWords * k] == s[0];   // quad 0 word 0: the database image's first tile, distinct per image
      const uint32_t key = record_order_key(qtile_off, chunk_tiles, ij, s + kWords * k);
      key_max = key > key_max ? key : key_max;
    }
    if (one_image) { std::memcpy(d, s, kWords * n * sizeof(uint32_t)); continue; }
    count.assign((size_t)key_max + 2, 0);
    for (uint32_t k = 0; k < n; ++k) ++count[record_order_key(qtile_off, chunk_tiles, ij, s + kWords * k) + 1];
    for (uint32_t c = 0; c <= key_max; ++c) count[c + 1] += count[c];
    for (uint32_t k = 0; k < n; ++k)
      std::memcpy(d + kWords * count[record_order_key(qtile_off, chunk_tiles, ij, s + kWords * k)]++, s + kWords * k, kWords * sizeof(uint32_t));
  }
}

}  // namespace mvgx_records

#ifndef MVGX_MATCH_BATCH_RECORDS_ONLY
#include <hip/hip_runtime.h>

#include <algorithm>

#include "mvgx_common.h"

namespace {

constexpr uint32_t kNoMatch = 0xFFFFFFFFu;

// ------------------------------------------------------------------------------------------------
// compaction: exclusive scan of per-pair counts, then ordered (ascending j) gather of the accepted queries
// (regions_matcher.hpp:198-205 emits the matches of a pair in that order)
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void scan_counts_kernel(const uint32_t* __restrict__ count, uint32_t n,
                                                           uint32_t* __restrict__ offsets /* n+1 */) {
  __shared__ uint32_t s_part[1024];
  const uint32_t per = (n + 1023) / 1024;
  const uint32_t lo = min(n, threadIdx.x * per), hi = min(n, lo + per);
  uint32_t sum = 0;
  for (uint32_t i = lo; i < hi; ++i) sum += count[i];
  s_part[threadIdx.x] = sum;
  __syncthreads();
  // Hillis-Steele inclusive scan over 1024 partials
  for (uint32_t d = 1; d < 1024; d <<= 1) {
    const uint32_t v = (threadIdx.x >= d) ? s_part[threadIdx.x - d] : 0;
    __syncthreads();
    s_part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = s_part[threadIdx.x] - sum;
  for (uint32_t i = lo; i < hi; ++i) { offsets[i] = run; run += count[i]; }
  if (threadIdx.x == 1023) offsets[n] = s_part[1023];
}

__global__ __launch_bounds__(256) void compact_matches_kernel(const uint32_t* __restrict__ best,
                                                              const uint32_t* __restrict__ offsets,
                                                              const uint2* __restrict__ pairs,
                                                              const uint32_t* __restrict__ img_n,
                                                              const uint64_t* __restrict__ img_row_off,
                                                              const uint32_t* __restrict__ rowpos,
                                                              uint32_t n_pairs, uint32_t qstride,
                                                              uint2* __restrict__ out_ij) {
  const uint32_t pidx = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per image pair
  if (pidx >= n_pairs) return;
  const int lane = threadIdx.x & 63;
  const uint32_t off = offsets[pidx];
  if (offsets[pidx + 1] == off) return;
  const uint32_t J = pairs[pidx].y;
  const uint32_t nJ = img_n[J];
  // original query row -> slot (best[] is slot-indexed); no table: the dense query slots of l2_filter16_kernel, slot = row
  const uint32_t* pos = rowpos ? rowpos + img_row_off[J] : nullptr;
  uint32_t run = off;
  for (uint32_t q0 = 0; q0 < nJ; q0 += 64) {
    const uint32_t q = q0 + lane;
    const uint32_t v = (q < nJ) ? best[(size_t)pidx * qstride + (pos ? pos[q] : q)] : kNoMatch;
    const bool ok = v != kNoMatch;
    const unsigned long long m = __ballot(ok);
    if (ok) {
      const uint32_t pre = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      out_ij[run + pre] = make_uint2(v, q);
    }
    run += (uint32_t)__popcll(m);
  }
}

// pairs per batch: the option, capped so that the scratch per pair and query slot (mvgx_match.hip: 12 B in each of two slots, near
// 6 GB; mvgx_bruteforce.hip: 4 B, near 2 GB) stays bounded when the images carry tens of thousands of descriptors
inline uint64_t batch_size(int64_t batch_pairs, uint32_t qstride) {
  return std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)batch_pairs, std::max<uint64_t>(16, (1ull << 29) / std::max<uint32_t>(qstride, 1))));
}

inline int check_pairs_in_range(const uint32_t* pairs_IJ, uint64_t n_pairs, uint32_t n_images, const char* who) {
  for (uint64_t k = 0; k < n_pairs; ++k)
    MVGX_REQUIRE(pairs_IJ[2 * k] < n_images && pairs_IJ[2 * k + 1] < n_images, MVGX_ERR_ARG,
                 "%s: pair %llu references image out of range", who, (unsigned long long)k);
  return MVGX_OK;
}

// `who` names the quantity in the caller's terms (the squared-metric matchers are given ratio^2)
inline int check_ratio(float ratio, const char* who) {
  MVGX_REQUIRE(ratio <= 1.0f && ratio >= 0.0f, MVGX_ERR_UNSUPPORTED,
               "%s = %g: the device path reproduces the reference only for 0 <= %s <= 1 "
               "(ties are libstdc++ partial_sort order beyond that)", who, (double)ratio, who);
  return MVGX_OK;
}

}  // namespace
#endif  // MVGX_MATCH_BATCH_RECORDS_ONLY
