// What every matcher's batch loop shares (mvgx_match.hip, mvgx_bruteforce.hip): the no-match sentinel of best[], the two kernels that
// turn best[] + per-pair counts into ordered match lists, the pairs-per-batch rule and the argument checks of a run.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

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
