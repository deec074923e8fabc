// What every matcher's batch loop shares (mvgx_match.hip, mvgx_bruteforce.hip): the no-match sentinel of best[], the two kernels that
// turn best[] + per-pair counts into ordered match lists, the pairs-per-batch rule and the argument checks of a run.
#pragma once
#include <cstddef>
#include <cstdint>

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
