// mvgx_tracks.h — feature tracks from pairwise matches on the device: kernels and host entry of mvgx_tracks_build.
// Included at the end of mvgx_bruteforce.hip (it uses scan_counts_kernel of mvgx_match_batch.h for the second level of its scans).
//
// What the reference does on the host (paths under src/openMVG of the reference):
//   tracks/tracks.hpp:70-121     TracksBuilder::Build: a std::set of every (image, feature) node, node index = rank in that order,
//                                one UnionFind::Union per match, pairs ascending, each list in order
//   tracks/union_find.hpp:75-103 Union by rank; on equal rank the FIRST argument's root stays root and its rank grows
//   tracks/tracks.hpp:124-165    Filter(min_length): drops every component in which an image occurs twice or with fewer images
//   tracks/tracks.hpp:178-196    ExportToSTL: ascending track id (the node index of the final root), ascending image inside a track
//
// Exact: everything; all outputs are integers. The id of a track is the root the reference's forest ends with. That root depends on
// the unions inside its own component alone, so each SURVIVING component (at most n_images nodes) replays its own matches in global
// match order on a private union-by-rank forest; colliding components are rejected before and never replayed.
//
// Passes (all lane-per-item unless said otherwise):
//   extent   n_features == NULL only: per image the largest kept feature index + 1 (one wave per pair, one 64-bit atomicMax per wave)
//   mark     kept matches: pair by binary search of match_start, indices validated into `first_bad`, used[feat_off[image] + feature] = 1
//   number   exclusive scan of `used`: node index = rank in (image, feature) order; node -> (image, feature); matches -> node pairs
//   label    connected components: hook the larger root under the smaller (64-bit atomicMin), then a shortcut pass; repeated until a
//            sweep changes nothing (the flag is read once per sweep by the host). label = the smallest node of the component
//   collide  one workgroup per image over its (contiguous) nodes: the labels go through an ordered open-addressing hash set
//            (atomicMax on 64-bit slots: a slot only ever grows, an evicted smaller key moves on; a key that meets itself flags its
//            component). Images of up to MVGX_TRACKS_LDS_CAP used features keep the table in LDS (2 x that many 8-byte slots: 32 KiB
//            at the default 2048); larger images take the same kernel on a table in global memory (2 x the next power of two slots)
//   select   nodes per component without a collision; survivors = no collision and >= min_length nodes (= images); survivor list by flag + scan
//   gather   matches per survivor: count, scan, fill through atomic cursors (arrival order - undone by the rank sort below)
//   replay   one wave per survivor: rank sort of its match list by match index, then lane 0 replays the unions; root -> track id
//   export   flag per root + scan = ascending-id order; lengths + scan = track_start; members through atomic cursors, then each node
//            is placed at (number of members with a smaller node index) = ascending image. Nothing the cursors' order touches survives.
// n_sweeps: a hook never gives up before its two roots are one (trk_hook_kernel), so the first sweep unites every component and the
// second finds nothing to change: 2 whenever a match is kept, whatever the scheduling. The loop stays as the check of that argument.
// Cost of the replay: a survivor with k matches pays k^2 / 64 reads per lane for the rank sort and k unions on one lane. k counts the
// matches, not the nodes: lists that repeat a match many times pay for every copy (the reference's matchers emit a match once).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mvgx_buffers.h"

// Used features per image up to which the collision pass keeps its hash set in LDS; a power of two. A build may set another
// value (-DMVGX_TRACKS_LDS_CAP=...) - the tests run at the default.
#ifndef MVGX_TRACKS_LDS_CAP
#define MVGX_TRACKS_LDS_CAP 2048
#endif

namespace {

constexpr uint32_t kTrkLdsCap = MVGX_TRACKS_LDS_CAP;
constexpr uint32_t kTrkLdsSlots = 2 * kTrkLdsCap;
static_assert((kTrkLdsCap & (kTrkLdsCap - 1)) == 0 && kTrkLdsSlots * 8 <= 65536, "MVGX_TRACKS_LDS_CAP: a power of two, at most 4096");
constexpr uint32_t kTrkNone = 0xFFFFFFFFu;
constexpr uint32_t kTrkChunk = 4096;   // elements one workgroup of 256 scans: 16 per lane

typedef unsigned long long trk_u64;

// ---- exclusive scan of n uint32 into n + 1: chunk sums, scan_counts_kernel over them, chunk scans (chunk_off == NULL: n fits one chunk) ----
__global__ __launch_bounds__(256) void trk_chunk_sum_kernel(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ sums) {
  __shared__ uint32_t s_sum[256];
  const uint64_t base = (uint64_t)blockIdx.x * kTrkChunk;
  uint32_t sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint64_t idx = base + (uint64_t)k * 256 + threadIdx.x;
    if (idx < n) sum += in[idx];
  }
  s_sum[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 128; d > 0; d >>= 1) {
    if (threadIdx.x < d) s_sum[threadIdx.x] += s_sum[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) sums[blockIdx.x] = s_sum[0];
}
__global__ __launch_bounds__(256) void trk_chunk_scan_kernel(const uint32_t* __restrict__ in, uint32_t n, const uint32_t* __restrict__ chunk_off,
                                                             uint32_t* __restrict__ out /* n + 1 */) {
  __shared__ uint32_t s_part[256];
  const uint64_t first = (uint64_t)blockIdx.x * kTrkChunk + (uint64_t)threadIdx.x * 16;
  uint32_t v[16], sum = 0;
#pragma unroll
  for (int k = 0; k < 16; ++k) { v[k] = first + k < n ? in[first + k] : 0u; sum += v[k]; }
  s_part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 256; d <<= 1) {   // Hillis-Steele, inclusive
    const uint32_t add = threadIdx.x >= d ? s_part[threadIdx.x - d] : 0u;
    __syncthreads();
    s_part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = (chunk_off ? chunk_off[blockIdx.x] : 0u) + s_part[threadIdx.x] - sum;
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    if (first + k < n) out[first + k] = run;
    run += v[k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 255) out[n] = chunk_off ? chunk_off[gridDim.x] : s_part[255];   // (one chunk: its own total)
}

// ---- extent: n_features == NULL. One wave per pair: the largest kept index + 1 on either side ----
__global__ __launch_bounds__(256) void trk_extent_kernel(const uint32_t* __restrict__ pairs, const uint64_t* __restrict__ match_start, uint32_t n_pairs,
                                                         const uint32_t* __restrict__ ij, const uint8_t* __restrict__ mask, trk_u64* __restrict__ extent) {
  const uint32_t p = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (p >= n_pairs) return;   // (wave-uniform)
  const uint64_t lo = match_start[p], hi = match_start[p + 1];
  trk_u64 ei = 0, ej = 0;
  for (uint64_t m = lo + lane; m < hi; m += 64) {
    if (mask && !mask[m]) continue;
    ei = max(ei, (trk_u64)ij[2 * m] + 1);
    ej = max(ej, (trk_u64)ij[2 * m + 1] + 1);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {   // (an extent is at most 2^32: two 32-bit exchanges per value)
    const trk_u64 oi = ((trk_u64)(uint32_t)__shfl_xor((int)(ei >> 32), off) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)ei, off);
    const trk_u64 oj = ((trk_u64)(uint32_t)__shfl_xor((int)(ej >> 32), off) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)ej, off);
    ei = max(ei, oi); ej = max(ej, oj);
  }
  if (lane == 0) {
    if (ei) atomicMax(&extent[pairs[2 * p]], ei);
    if (ej) atomicMax(&extent[pairs[2 * p + 1]], ej);
  }
}

// last index e in [0, n) with start[e] <= v (start[0] <= v is given): the owner of v among ranges, empty ranges skipped
template <typename T>
__device__ __forceinline__ uint32_t trk_owner(const T* __restrict__ start, uint32_t n, uint64_t v) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((uint64_t)start[mid] <= v) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- mark ----
// key_a / key_b: the dense keys feat_off[image] + feature of a kept, valid match; kTrkNone otherwise. counters[0] += kept matches.
__global__ __launch_bounds__(256) void trk_mark_kernel(const uint32_t* __restrict__ pairs, const uint64_t* __restrict__ match_start, uint32_t n_pairs,
                                                       const uint32_t* __restrict__ ij, const uint8_t* __restrict__ mask, uint32_t n_matches,
                                                       const uint32_t* __restrict__ feat_off, uint32_t* __restrict__ used, uint32_t* __restrict__ key_a,
                                                       uint32_t* __restrict__ key_b, unsigned* __restrict__ counters, trk_u64* __restrict__ first_bad) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  const bool kept = m < n_matches && (!mask || mask[m]);
  bool good = false;
  if (kept) {
    const uint32_t p = trk_owner(match_start, n_pairs, m);
    const uint32_t I = pairs[2 * p], J = pairs[2 * p + 1], i = ij[2 * (size_t)m], j = ij[2 * (size_t)m + 1];
    const uint32_t oI = feat_off[I], oJ = feat_off[J];
    good = i < feat_off[I + 1] - oI && j < feat_off[J + 1] - oJ;
    if (good) {
      used[oI + i] = 1u; used[oJ + j] = 1u;
      key_a[m] = oI + i; key_b[m] = oJ + j;
    } else {
      atomicMin(first_bad, (trk_u64)m);
    }
  }
  if (m < n_matches && !good) { key_a[m] = kTrkNone; key_b[m] = kTrkNone; }
  const trk_u64 votes = __ballot(good);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&counters[0], (unsigned)__popcll(votes));
}

// ---- number ----
// node -> (image, feature), one lane per dense key
__global__ __launch_bounds__(256) void trk_nodes_kernel(const uint32_t* __restrict__ used, const uint32_t* __restrict__ node_of_key, uint32_t n_keys,
                                                        const uint32_t* __restrict__ feat_off, uint32_t n_images, uint32_t* __restrict__ node_image,
                                                        uint32_t* __restrict__ node_feature) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_keys || !used[k]) return;
  const uint32_t I = trk_owner(feat_off, n_images, k), n = node_of_key[k];
  node_image[n] = I;
  node_feature[n] = k - feat_off[I];
}
// the node range of every image: nodes are numbered in (image, feature) order, so an image's nodes are contiguous
__global__ __launch_bounds__(256) void trk_image_range_kernel(const uint32_t* __restrict__ node_of_key, const uint32_t* __restrict__ feat_off,
                                                              uint32_t n_images, uint32_t* __restrict__ image_node_start /* n_images + 1 */) {
  const uint32_t I = blockIdx.x * blockDim.x + threadIdx.x;
  if (I <= n_images) image_node_start[I] = node_of_key[feat_off[I]];
}
// keys -> nodes, in place
__global__ __launch_bounds__(256) void trk_resolve_kernel(uint32_t* __restrict__ key_a, uint32_t* __restrict__ key_b, uint32_t n_matches,
                                                          const uint32_t* __restrict__ node_of_key) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_matches || key_a[m] == kTrkNone) return;
  key_a[m] = node_of_key[key_a[m]];
  key_b[m] = node_of_key[key_b[m]];
}
__global__ __launch_bounds__(256) void trk_iota_kernel(trk_u64* __restrict__ parent, uint32_t* __restrict__ forest, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) { parent[i] = i; forest[i] = i; }
}

// ---- label ----
__device__ __forceinline__ trk_u64 trk_root(const trk_u64* parent, trk_u64 x) {   // parent[x] <= x always: no cycle
  for (;;) {
    const trk_u64 p = parent[x];
    if (p == x) return x;
    x = p;
  }
}
// One lane per match. A hook that finds its target hooked meanwhile (old != hi) goes on with the pair (old, lo): no edge is lost to a
// concurrent hook, the values only fall, so the loop ends.
__global__ __launch_bounds__(256) void trk_hook_kernel(const uint32_t* __restrict__ node_a, const uint32_t* __restrict__ node_b, uint32_t n_matches,
                                                       trk_u64* parent, uint32_t* __restrict__ changed) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_matches || node_a[m] == kTrkNone) return;
  trk_u64 a = node_a[m], b = node_b[m];
  for (;;) {
    a = trk_root(parent, a); b = trk_root(parent, b);
    if (a == b) return;
    const trk_u64 hi = a > b ? a : b, lo = a > b ? b : a;
    const trk_u64 old = atomicMin(&parent[hi], lo);
    *changed = 1u;
    if (old == hi) return;
    a = old; b = lo;
  }
}
__global__ __launch_bounds__(256) void trk_shortcut_kernel(trk_u64* parent, uint32_t* __restrict__ label, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const trk_u64 r = trk_root(parent, i);
  parent[i] = r;
  label[i] = (uint32_t)r;
}

// ---- collide ----
// One workgroup per listed image. Ordered open addressing: a slot holds the largest key + 1 that probed it, an evicted smaller key
// goes on to the next slot. Two instances of a key walk the same probe sequence past slots that only grow, so the later one meets
// the earlier one (in its slot, or on the way to the same slot): a key equal to the slot's content is a label met twice.
// The table is at most half full (slots >= 2 x the image's nodes), so every walk ends.
template <bool kLds>
__global__ __launch_bounds__(256) void trk_collide_kernel(const uint32_t* __restrict__ image_list, const uint32_t* __restrict__ image_node_start,
                                                          const uint32_t* __restrict__ label, trk_u64* global_tables, const trk_u64* __restrict__ table_off,
                                                          const uint32_t* __restrict__ table_slots, uint32_t* __restrict__ collision) {
  __shared__ trk_u64 s_table[kLds ? kTrkLdsSlots : 1];
  const uint32_t I = image_list[blockIdx.x];
  const uint32_t n0 = image_node_start[I], n1 = image_node_start[I + 1];
  trk_u64* table = s_table;
  uint32_t mask = kTrkLdsSlots - 1;
  if constexpr (kLds) {
    if (n1 - n0 > kTrkLdsCap) return;   // (the host never lists such an image here)
    for (uint32_t s = threadIdx.x; s < kTrkLdsSlots; s += 256) s_table[s] = 0;
    __syncthreads();
  } else {
    table = global_tables + table_off[blockIdx.x];   // zeroed by the host's memset
    mask = table_slots[blockIdx.x] - 1;
    if ((trk_u64)(n1 - n0) * 2 > (trk_u64)mask + 1) return;
  }
  for (uint32_t n = n0 + threadIdx.x; n < n1; n += 256) {
    trk_u64 key = (trk_u64)label[n] + 1;
    uint32_t h = (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 32) & mask;
    for (;;) {
      const trk_u64 old = atomicMax(&table[h], key);
      if (old == 0) break;
      if (old == key) { collision[(uint32_t)(key - 1)] = 1u; break; }
      if (old < key) key = old;   // evicted: it moves on
      h = (h + 1) & mask;
    }
  }
}

// ---- select ----
// (a component with a collision is dropped whatever its size: not counted - the wrongly merged giant one would put a million
// additions on one address, measured at 20 ms)
__global__ __launch_bounds__(256) void trk_count_nodes_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ collision, uint32_t n,
                                                              unsigned* __restrict__ comp_nodes) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && !collision[label[i]]) atomicAdd(&comp_nodes[label[i]], 1u);
}
// counters: [1] components, [2] with a collision, [3] short without one, [4] survivors, [5] their nodes
__global__ __launch_bounds__(256) void trk_select_kernel(const uint32_t* __restrict__ label, const unsigned* __restrict__ comp_nodes,
                                                         const uint32_t* __restrict__ collision, uint32_t n, uint32_t min_length,
                                                         uint32_t* __restrict__ survives, unsigned* __restrict__ counters) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool root = i < n && label[i] == i;
  const bool bad = root && collision[i] != 0;
  const bool brief = root && !bad && comp_nodes[i] < min_length;
  const bool keep = root && !bad && !brief;
  if (i < n) survives[i] = keep ? 1u : 0u;
  unsigned nodes = keep ? comp_nodes[i] : 0u;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) nodes += (unsigned)__shfl_xor((int)nodes, off);
  const trk_u64 v_root = __ballot(root), v_bad = __ballot(bad), v_brief = __ballot(brief), v_keep = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && v_root) {
    atomicAdd(&counters[1], (unsigned)__popcll(v_root));
    if (v_bad) atomicAdd(&counters[2], (unsigned)__popcll(v_bad));
    if (v_brief) atomicAdd(&counters[3], (unsigned)__popcll(v_brief));
    if (v_keep) { atomicAdd(&counters[4], (unsigned)__popcll(v_keep)); atomicAdd(&counters[5], nodes); }
  }
}
// list[index[i]] = i for every flagged i (index = the exclusive scan of flag)
__global__ __launch_bounds__(256) void trk_compact_kernel(const uint32_t* __restrict__ flag, const uint32_t* __restrict__ index, uint32_t n,
                                                          uint32_t* __restrict__ list) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && flag[i]) list[index[i]] = i;
}

// ---- gather the matches of the survivors ----
__global__ __launch_bounds__(256) void trk_count_matches_kernel(const uint32_t* __restrict__ node_a, uint32_t n_matches, const uint32_t* __restrict__ label,
                                                                const uint32_t* __restrict__ survives, unsigned* __restrict__ comp_matches) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_matches || node_a[m] == kTrkNone) return;
  const uint32_t c = label[node_a[m]];
  if (survives[c]) atomicAdd(&comp_matches[c], 1u);
}
__global__ __launch_bounds__(256) void trk_fill_matches_kernel(const uint32_t* __restrict__ node_a, uint32_t n_matches, const uint32_t* __restrict__ label,
                                                               const uint32_t* __restrict__ survives, const uint32_t* __restrict__ match_off,
                                                               unsigned* __restrict__ cursor, uint32_t* __restrict__ list) {
  const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n_matches || node_a[m] == kTrkNone) return;
  const uint32_t c = label[node_a[m]];
  if (survives[c]) list[match_off[c] + atomicAdd(&cursor[c], 1u)] = m;
}

// ---- replay ----
// One wave per survivor. The list arrives in cursor order; every lane ranks its entries (distinct match indices: rank = the number of
// smaller ones) into `sorted`, then lane 0 runs UnionFind::Union over them on the component's own nodes of `forest` / `rank` (no path
// compression: it changes neither a rank nor a root). root_of[label] = the final root, is_root / label_of_root mark it.
__global__ __launch_bounds__(64) void trk_replay_kernel(const uint32_t* __restrict__ survivors, const uint32_t* __restrict__ match_off,
                                                        const uint32_t* list, uint32_t* sorted, const uint32_t* __restrict__ node_a,
                                                        const uint32_t* __restrict__ node_b, uint32_t* forest, uint32_t* rank,
                                                        uint32_t* __restrict__ root_of, uint32_t* __restrict__ is_root, uint32_t* __restrict__ label_of_root) {
  const uint32_t c = survivors[blockIdx.x];
  const uint32_t o0 = match_off[c], k = match_off[c + 1] - o0;
  for (uint32_t e = threadIdx.x; e < k; e += 64) {
    const uint32_t v = list[o0 + e];
    uint32_t r = 0;
    for (uint32_t q = 0; q < k; ++q) r += list[o0 + q] < v ? 1u : 0u;
    sorted[o0 + r] = v;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (uint32_t e = 0; e < k; ++e) {
    const uint32_t m = sorted[o0 + e];
    uint32_t i = node_a[m], j = node_b[m];
    while (forest[i] != i) i = forest[i];
    while (forest[j] != j) j = forest[j];
    if (i == j) continue;
    const uint32_t ri = rank[i], rj = rank[j];
    if (ri < rj) forest[i] = j;
    else { forest[j] = i; if (ri == rj) rank[i] = ri + 1; }
  }
  uint32_t r = c;
  while (forest[r] != r) r = forest[r];
  root_of[c] = r;
  is_root[r] = 1u;
  label_of_root[r] = c;
}

// ---- export ----
__global__ __launch_bounds__(256) void trk_track_kernel(const uint32_t* __restrict__ is_root, const uint32_t* __restrict__ track_of_root,
                                                        const uint32_t* __restrict__ label_of_root, const unsigned* __restrict__ comp_nodes, uint32_t n,
                                                        uint32_t* __restrict__ track_id, uint32_t* __restrict__ track_len) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n || !is_root[r]) return;
  const uint32_t t = track_of_root[r];
  track_id[t] = r;
  track_len[t] = comp_nodes[label_of_root[r]];
}
__global__ __launch_bounds__(256) void trk_members_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ survives,
                                                          const uint32_t* __restrict__ root_of, const uint32_t* __restrict__ track_of_root,
                                                          const uint32_t* __restrict__ track_start, uint32_t n, unsigned* __restrict__ cursor,
                                                          uint32_t* __restrict__ members) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !survives[label[i]]) return;
  const uint32_t t = track_of_root[root_of[label[i]]];
  members[track_start[t] + atomicAdd(&cursor[t], 1u)] = i;
}
// a node's place in its track = the number of members with a smaller node index: ascending (image, feature), and a surviving track
// holds an image once
__global__ __launch_bounds__(256) void trk_place_kernel(const uint32_t* __restrict__ label, const uint32_t* __restrict__ survives,
                                                        const uint32_t* __restrict__ root_of, const uint32_t* __restrict__ track_of_root,
                                                        const uint32_t* __restrict__ track_start, const uint32_t* __restrict__ members, uint32_t n,
                                                        const uint32_t* __restrict__ node_image, const uint32_t* __restrict__ node_feature,
                                                        uint32_t* __restrict__ obs_image, uint32_t* __restrict__ obs_feature) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || !survives[label[i]]) return;
  const uint32_t t = track_of_root[root_of[label[i]]];
  const uint32_t s0 = track_start[t], s1 = track_start[t + 1];
  uint32_t pos = 0;
  for (uint32_t s = s0; s < s1; ++s) pos += members[s] < i ? 1u : 0u;
  obs_image[s0 + pos] = node_image[i];
  obs_feature[s0 + pos] = node_feature[i];
}

// ---- host ----
enum { kTrkPassExtent = 0, kTrkPassMark, kTrkPassNumber, kTrkPassLabel, kTrkPassCollide, kTrkPassSelect, kTrkPassGather, kTrkPassReplay, kTrkPassExport, kTrkPasses };
double g_trk_pass_ms[kTrkPasses];   // the passes of the last call (mvgx_debug_tracks_pass_ms; a measuring aid, not thread-safe)

// HIP events around the launches of a pass; the elapsed times are read after the call's last synchronisation
struct TrkTimer {
  hipStream_t stream;
  bool enabled;   // false (the caller asked for no stats): no event is created, recorded or read
  struct Span { int pass; hipEvent_t a, b; };
  std::vector<Span> spans;
  ~TrkTimer() { for (Span& s : spans) { (void)hipEventDestroy(s.a); (void)hipEventDestroy(s.b); } }
  int begin(int pass) {
    if (!enabled) return MVGX_OK;
    Span s{pass, nullptr, nullptr};
    MVGX_HIP(hipEventCreate(&s.a));
    if (hipEventCreate(&s.b) != hipSuccess) { (void)hipEventDestroy(s.a); ::mvgx::set_error("mvgx_tracks_build: hipEventCreate failed"); return MVGX_ERR_HIP; }
    spans.push_back(s);
    MVGX_HIP(hipEventRecord(s.a, stream));
    return MVGX_OK;
  }
  int end() { if (enabled) MVGX_HIP(hipEventRecord(spans.back().b, stream)); return MVGX_OK; }
  double collect(double* per_pass) {   // after a synchronisation of the stream
    double sum = 0.0;
    for (int k = 0; k < kTrkPasses; ++k) per_pass[k] = 0.0;
    for (Span& s : spans) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, s.a, s.b) == hipSuccess) { per_pass[s.pass] += ms; sum += ms; }
    }
    return sum;
  }
};

inline dim3 trk_grid(uint64_t n, uint32_t per_block = 256) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

struct TrkScan {   // scratch of the two-level scan
  mvgx::DevBuf<uint32_t> sums, chunk_off;
  int run(const uint32_t* in, uint32_t n, uint32_t* out, hipStream_t stream) {
    if (!n) { MVGX_HIP(hipMemsetAsync(out, 0, sizeof(uint32_t), stream)); return MVGX_OK; }
    const uint32_t chunks = (uint32_t)(((uint64_t)n + kTrkChunk - 1) / kTrkChunk);
    if (chunks == 1) {   // one launch: the chunk's scan is the scan
      hipLaunchKernelGGL(trk_chunk_scan_kernel, dim3(1), dim3(256), 0, stream, in, n, (const uint32_t*)nullptr, out);
      MVGX_HIP(hipGetLastError());
      return MVGX_OK;
    }
    int rc;
    if ((rc = sums.ensure(chunks)) || (rc = chunk_off.ensure((size_t)chunks + 1))) return rc;
    uint32_t* const p_sums = sums.p;   // (raw pointers: the test-suite's emulation captures launch arguments by value)
    uint32_t* const p_off = chunk_off.p;
    hipLaunchKernelGGL(trk_chunk_sum_kernel, dim3(chunks), dim3(256), 0, stream, in, n, p_sums);
    hipLaunchKernelGGL(scan_counts_kernel, dim3(1), dim3(1024), 0, stream, (const uint32_t*)p_sums, chunks, p_off);
    hipLaunchKernelGGL(trk_chunk_scan_kernel, dim3(chunks), dim3(256), 0, stream, in, n, (const uint32_t*)p_off, out);
    MVGX_HIP(hipGetLastError());
    return MVGX_OK;
  }
};

template <typename T>
int trk_upload(mvgx::DevBuf<T>& dst, const T* src, size_t n, hipStream_t stream) {
  const int rc = dst.ensure(std::max<size_t>(n, 1));
  if (rc) return rc;
  if (n) MVGX_HIP(hipMemcpyAsync(dst.p, src, n * sizeof(T), hipMemcpyHostToDevice, stream));
  return MVGX_OK;
}
template <typename T>
int trk_zeroed(mvgx::DevBuf<T>& dst, size_t n, hipStream_t stream) {
  const int rc = dst.ensure(std::max<size_t>(n, 1));
  if (rc) return rc;
  MVGX_HIP(hipMemsetAsync(dst.p, 0, std::max<size_t>(n, 1) * sizeof(T), stream));
  return MVGX_OK;
}

int trk_check_arguments(uint32_t n_images, const uint32_t* n_features, const uint32_t* pairs, const uint64_t* match_start, const uint32_t* ij, uint64_t n_pairs,
                        const mvgx_tracks_options* opt, uint32_t* n_tracks, uint32_t** track_id, uint64_t** track_start, uint32_t** obs_image,
                        uint32_t** obs_feature) {
  MVGX_REQUIRE(opt && n_tracks && track_id && track_start && obs_image && obs_feature, MVGX_ERR_ARG, "mvgx_tracks_build: NULL options or output");
  MVGX_REQUIRE(opt->min_length >= 2, MVGX_ERR_ARG, "mvgx_tracks_build: min_length %u (a track has at least two images)", opt->min_length);
  MVGX_REQUIRE(!n_pairs || (pairs && match_start), MVGX_ERR_ARG, "mvgx_tracks_build: NULL pairs or match_start");
  MVGX_REQUIRE(n_pairs < 0xFFFFFFFFull, MVGX_ERR_UNSUPPORTED, "mvgx_tracks_build: more than 2^32 - 2 pairs");
  for (uint64_t p = 0; p < n_pairs; ++p) {
    const uint32_t I = pairs[2 * p], J = pairs[2 * p + 1];
    MVGX_REQUIRE(I < J, MVGX_ERR_ARG, "mvgx_tracks_build: pair %llu is (%u, %u): I < J is required", (unsigned long long)p, I, J);
    MVGX_REQUIRE(J < n_images, MVGX_ERR_ARG, "mvgx_tracks_build: pair %llu names image %u of %u", (unsigned long long)p, J, n_images);
    MVGX_REQUIRE(!p || pairs[2 * p - 2] < I || (pairs[2 * p - 2] == I && pairs[2 * p - 1] < J), MVGX_ERR_ARG,
                 "mvgx_tracks_build: pair %llu is not above the pair before it (the order of a std::map<Pair, IndMatches> is required)", (unsigned long long)p);
    MVGX_REQUIRE(match_start[p] <= match_start[p + 1], MVGX_ERR_ARG, "mvgx_tracks_build: match_start decreases at pair %llu", (unsigned long long)p);
  }
  if (n_pairs) {
    const uint64_t n_matches = match_start[n_pairs] - match_start[0];
    MVGX_REQUIRE(!n_matches || ij, MVGX_ERR_ARG, "mvgx_tracks_build: NULL ij");
    MVGX_REQUIRE(n_matches < 0xFFFFFFFFull, MVGX_ERR_UNSUPPORTED, "mvgx_tracks_build: more than 2^32 - 2 matches");
  }
  if (n_features) {
    uint64_t sum = 0;
    for (uint32_t I = 0; I < n_images; ++I) sum += n_features[I];
    MVGX_REQUIRE(sum < 0xFFFFFFFFull, MVGX_ERR_UNSUPPORTED, "mvgx_tracks_build: %llu features do not fit 32 bits", (unsigned long long)sum);
  }
  return MVGX_OK;
}

// the four arrays of an empty result (track_start = {0}); every pointer can go to mvgx_host_free
int trk_allocate_outputs(uint32_t n_t, uint32_t n_obs, uint32_t** track_id, uint64_t** track_start, uint32_t** obs_image, uint32_t** obs_feature) {
  uint32_t* id = static_cast<uint32_t*>(malloc(std::max<size_t>(n_t, 1) * sizeof(uint32_t)));
  uint64_t* start = static_cast<uint64_t*>(calloc((size_t)n_t + 1, sizeof(uint64_t)));
  uint32_t* oi = static_cast<uint32_t*>(malloc(std::max<size_t>(n_obs, 1) * sizeof(uint32_t)));
  uint32_t* of = static_cast<uint32_t*>(malloc(std::max<size_t>(n_obs, 1) * sizeof(uint32_t)));
  if (!id || !start || !oi || !of) {
    free(id); free(start); free(oi); free(of);
    ::mvgx::set_error("mvgx_tracks_build: out of host memory");
    return MVGX_ERR_HIP;
  }
  *track_id = id; *track_start = start; *obs_image = oi; *obs_feature = of;
  return MVGX_OK;
}

}  // namespace

extern "C" {

void mvgx_tracks_default_options(mvgx_tracks_options* o) {
  if (o) o->min_length = 2;   // TracksBuilder::Filter's default
}

// Measuring aid (not declared in include/mvgx.h): device time of each pass of the calling process's last mvgx_tracks_build, milliseconds,
// in the order extent, mark, number, label, collide, select, gather, replay, export
int mvgx_debug_tracks_pass_ms(double* out, int n) {
  MVGX_REQUIRE(out && n >= kTrkPasses, MVGX_ERR_ARG, "mvgx_debug_tracks_pass_ms: room for %d values", (int)kTrkPasses);
  for (int k = 0; k < kTrkPasses; ++k) out[k] = g_trk_pass_ms[k];
  return MVGX_OK;
}

int mvgx_tracks_build(int device, uint32_t n_images, const uint32_t* n_features, const uint32_t* pairs, const uint64_t* match_start, const uint32_t* ij,
                      const uint8_t* match_mask, uint64_t n_pairs, const mvgx_tracks_options* opt, uint32_t* n_tracks, uint32_t** track_id,
                      uint64_t** track_start, uint32_t** obs_image, uint32_t** obs_feature, mvgx_tracks_stats* stats) {
  using clock = std::chrono::steady_clock;
  const auto t_begin = clock::now();
  int rc;
  if ((rc = trk_check_arguments(n_images, n_features, pairs, match_start, ij, n_pairs, opt, n_tracks, track_id, track_start, obs_image, obs_feature))) return rc;
  mvgx_tracks_stats st;
  memset(&st, 0, sizeof(st));
  const auto finish = [&](uint32_t n_t) {
    *n_tracks = n_t;
    st.n_tracks = n_t;
    st.total_ms = std::chrono::duration<double, std::milli>(clock::now() - t_begin).count();
    if (stats) *stats = st;
    return MVGX_OK;
  };
  const uint64_t m_base = n_pairs ? match_start[0] : 0;
  const uint32_t n_matches = n_pairs ? (uint32_t)(match_start[n_pairs] - m_base) : 0;
  if (!n_matches) {   // no pairs, or every list empty
    if ((rc = trk_allocate_outputs(0, 0, track_id, track_start, obs_image, obs_feature))) return rc;
    return finish(0);
  }
  // matches are addressed from match_start[0]: ij and the mask are taken from there
  const uint32_t* const ij0 = ij + 2 * m_base;
  const uint8_t* const mask0 = match_mask ? match_mask + m_base : nullptr;
  const uint32_t np = (uint32_t)n_pairs;
  std::vector<uint64_t> start0(n_pairs + 1);
  for (uint64_t p = 0; p <= n_pairs; ++p) start0[p] = match_start[p] - m_base;

  if ((rc = mvgx::select_device(device < 0 ? -1 : device))) return rc;
  mvgx::DevBuf<uint32_t> d_pairs, d_ij, d_feat_off, d_used, d_node_of_key, d_a, d_b, d_node_image, d_node_feature, d_image_start, d_label, d_flag;
  mvgx::DevBuf<uint32_t> d_collision, d_survives, d_index, d_survivors, d_match_off, d_list, d_sorted, d_forest, d_rank, d_root_of, d_is_root;
  mvgx::DevBuf<uint32_t> d_label_of_root, d_track_of_root, d_track_id, d_track_len, d_track_start, d_members, d_obs_image, d_obs_feature, d_image_list, d_table_slots;
  mvgx::DevBuf<unsigned> d_counters, d_comp_nodes, d_comp_matches, d_cursor;
  mvgx::DevBuf<uint64_t> d_start;
  mvgx::DevBuf<trk_u64> d_extent, d_first_bad, d_parent, d_tables, d_table_off;
  mvgx::DevBuf<uint8_t> d_mask;
  TrkScan scan;
  hipStream_t stream = nullptr;
  if ((rc = mvgx::acquire_stream(&stream))) return rc;
  int stream_device = 0;
  MVGX_HIP(hipGetDevice(&stream_device));
  mvgx::StreamGuard sg{stream_device, stream};   // (after the buffers: drained first, they are freed after)
  TrkTimer timer{stream, stats != nullptr, {}};

  if ((rc = trk_upload(d_pairs, pairs, 2 * (size_t)n_pairs, stream)) || (rc = trk_upload(d_start, start0.data(), start0.size(), stream)) ||
      (rc = trk_upload(d_ij, ij0, 2 * (size_t)n_matches, stream)) || (rc = trk_upload(d_mask, mask0, mask0 ? n_matches : 0, stream)))
    return rc;
  // (launch arguments are plain pointers and counts: the test-suite's emulation captures them by value)
  const uint32_t* const p_pairs = d_pairs.p;
  const uint64_t* const p_start = d_start.p;
  const uint32_t* const p_ij = d_ij.p;
  const uint8_t* const p_mask = mask0 ? d_mask.p : nullptr;

  // ---- the dense key space: feat_off[image] + feature ----
  std::vector<uint32_t> feat_off((size_t)n_images + 1, 0u);
  if (n_features) {
    for (uint32_t I = 0; I < n_images; ++I) feat_off[I + 1] = feat_off[I] + n_features[I];
  } else {
    if ((rc = trk_zeroed(d_extent, n_images, stream)) || (rc = timer.begin(kTrkPassExtent))) return rc;
    trk_u64* const p_extent = d_extent.p;
    hipLaunchKernelGGL(trk_extent_kernel, trk_grid(np, 4), dim3(256), 0, stream, p_pairs, p_start, np, p_ij, p_mask, p_extent);
    MVGX_HIP(hipGetLastError());
    if ((rc = timer.end())) return rc;
    std::vector<trk_u64> extent(n_images);
    MVGX_HIP(hipMemcpyAsync(extent.data(), d_extent.p, (size_t)n_images * sizeof(trk_u64), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipStreamSynchronize(stream));
    uint64_t sum = 0;
    for (uint32_t I = 0; I < n_images; ++I) {
      sum += extent[I];
      MVGX_REQUIRE(sum < 0xFFFFFFFFull, MVGX_ERR_UNSUPPORTED, "mvgx_tracks_build: the feature indices used span %llu and more keys: they do not fit 32 bits",
                   (unsigned long long)sum);
      feat_off[I + 1] = (uint32_t)sum;
    }
  }
  const uint32_t n_keys = feat_off[n_images];

  // ---- mark, number ----
  if ((rc = trk_upload(d_feat_off, feat_off.data(), feat_off.size(), stream)) || (rc = trk_zeroed(d_used, n_keys, stream)) ||
      (rc = d_node_of_key.ensure((size_t)n_keys + 1)) || (rc = d_a.ensure(n_matches)) || (rc = d_b.ensure(n_matches)) || (rc = trk_zeroed(d_counters, 8, stream)) ||
      (rc = d_first_bad.ensure(1)) || (rc = d_image_start.ensure((size_t)n_images + 1)))
    return rc;
  MVGX_HIP(hipMemsetAsync(d_first_bad.p, 0xFF, sizeof(trk_u64), stream));
  const uint32_t* const p_feat_off = d_feat_off.p;
  uint32_t* const p_used = d_used.p;
  uint32_t* const p_node_of_key = d_node_of_key.p;
  uint32_t* const p_a = d_a.p;
  uint32_t* const p_b = d_b.p;
  unsigned* const p_counters = d_counters.p;
  trk_u64* const p_first_bad = d_first_bad.p;
  uint32_t* const p_image_start = d_image_start.p;
  if ((rc = timer.begin(kTrkPassMark))) return rc;
  hipLaunchKernelGGL(trk_mark_kernel, trk_grid(n_matches), dim3(256), 0, stream, p_pairs, p_start, np, p_ij, p_mask, n_matches, p_feat_off, p_used, p_a, p_b,
                     p_counters, p_first_bad);
  MVGX_HIP(hipGetLastError());
  if ((rc = timer.end()) || (rc = timer.begin(kTrkPassNumber)) || (rc = scan.run(p_used, n_keys, p_node_of_key, stream))) return rc;
  hipLaunchKernelGGL(trk_image_range_kernel, trk_grid((uint64_t)n_images + 1), dim3(256), 0, stream, (const uint32_t*)p_node_of_key, p_feat_off, n_images,
                     p_image_start);
  MVGX_HIP(hipGetLastError());
  if ((rc = timer.end())) return rc;
  std::vector<uint32_t> image_start((size_t)n_images + 1);
  trk_u64 first_bad = 0;
  unsigned counters[8];
  MVGX_HIP(hipMemcpyAsync(image_start.data(), d_image_start.p, image_start.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
  MVGX_HIP(hipMemcpyAsync(&first_bad, d_first_bad.p, sizeof(trk_u64), hipMemcpyDeviceToHost, stream));
  MVGX_HIP(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
  MVGX_HIP(hipStreamSynchronize(stream));
  if (first_bad != ~0ull) {
    const uint64_t m = first_bad;
    const uint64_t p = (uint64_t)(std::upper_bound(start0.begin(), start0.end(), m) - start0.begin()) - 1;
    MVGX_REQUIRE(false, MVGX_ERR_ARG, "mvgx_tracks_build: match %llu (%u, %u) of pair (%u, %u) names a feature beyond n_features", (unsigned long long)(m + m_base),
                 ij0[2 * m], ij0[2 * m + 1], pairs[2 * p], pairs[2 * p + 1]);
  }
  const uint32_t n_nodes = image_start[n_images];
  st.n_matches_used = counters[0];
  st.n_nodes = n_nodes;
  if (!n_nodes) {   // the mask keeps nothing
    if ((rc = trk_allocate_outputs(0, 0, track_id, track_start, obs_image, obs_feature))) return rc;
    st.kernel_ms = timer.collect(g_trk_pass_ms);
    return finish(0);
  }

  if ((rc = d_node_image.ensure(n_nodes)) || (rc = d_node_feature.ensure(n_nodes)) || (rc = d_parent.ensure(n_nodes)) || (rc = d_forest.ensure(n_nodes)) ||
      (rc = d_label.ensure(n_nodes)) || (rc = d_flag.ensure(1)))
    return rc;
  uint32_t* const p_node_image = d_node_image.p;
  uint32_t* const p_node_feature = d_node_feature.p;
  trk_u64* const p_parent = d_parent.p;
  uint32_t* const p_forest = d_forest.p;
  uint32_t* const p_label = d_label.p;
  uint32_t* const p_flag = d_flag.p;
  if ((rc = timer.begin(kTrkPassNumber))) return rc;
  hipLaunchKernelGGL(trk_nodes_kernel, trk_grid(n_keys), dim3(256), 0, stream, (const uint32_t*)p_used, (const uint32_t*)p_node_of_key, n_keys, p_feat_off, n_images,
                     p_node_image, p_node_feature);
  hipLaunchKernelGGL(trk_resolve_kernel, trk_grid(n_matches), dim3(256), 0, stream, p_a, p_b, n_matches, (const uint32_t*)p_node_of_key);
  hipLaunchKernelGGL(trk_iota_kernel, trk_grid(n_nodes), dim3(256), 0, stream, p_parent, p_forest, n_nodes);
  MVGX_HIP(hipGetLastError());
  if ((rc = timer.end())) return rc;

  // ---- label: until a sweep changes nothing ----
  for (;;) {
    uint32_t changed = 0;
    if ((rc = timer.begin(kTrkPassLabel))) return rc;
    MVGX_HIP(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), stream));
    hipLaunchKernelGGL(trk_hook_kernel, trk_grid(n_matches), dim3(256), 0, stream, (const uint32_t*)p_a, (const uint32_t*)p_b, n_matches, p_parent, p_flag);
    hipLaunchKernelGGL(trk_shortcut_kernel, trk_grid(n_nodes), dim3(256), 0, stream, p_parent, p_label, n_nodes);
    MVGX_HIP(hipGetLastError());
    if ((rc = timer.end())) return rc;
    MVGX_HIP(hipMemcpyAsync(&changed, d_flag.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipStreamSynchronize(stream));
    ++st.n_sweeps;
    if (!changed) break;
  }

  // ---- collide: the images by class ----
  std::vector<uint32_t> lds_images, big_images, big_slots;
  std::vector<trk_u64> big_off;
  trk_u64 table_words = 0;
  for (uint32_t I = 0; I < n_images; ++I) {
    const uint32_t cnt = image_start[I + 1] - image_start[I];
    if (cnt < 2) continue;   // one node cannot collide
    if (cnt <= kTrkLdsCap) { lds_images.push_back(I); continue; }
    MVGX_REQUIRE(cnt < (1u << 30), MVGX_ERR_UNSUPPORTED, "mvgx_tracks_build: image %u has %u matched features (2^30 and more have no table)", I, cnt);
    uint32_t slots = 2 * kTrkLdsSlots;
    while ((uint64_t)slots < 2ull * cnt) slots *= 2;
    big_images.push_back(I); big_slots.push_back(slots); big_off.push_back(table_words);
    table_words += slots;
  }
  std::vector<uint32_t> image_lists(lds_images);
  image_lists.insert(image_lists.end(), big_images.begin(), big_images.end());
  if ((rc = trk_upload(d_image_list, image_lists.data(), image_lists.size(), stream)) || (rc = trk_upload(d_table_slots, big_slots.data(), big_slots.size(), stream)) ||
      (rc = trk_upload(d_table_off, big_off.data(), big_off.size(), stream)) || (rc = trk_zeroed(d_tables, (size_t)table_words, stream)) ||
      (rc = trk_zeroed(d_collision, n_nodes, stream)) || (rc = trk_zeroed(d_comp_nodes, n_nodes, stream)) || (rc = d_survives.ensure(n_nodes)) ||
      (rc = d_index.ensure((size_t)n_nodes + 1)) || (rc = d_survivors.ensure(n_nodes)) || (rc = trk_zeroed(d_comp_matches, n_nodes, stream)) ||
      (rc = d_match_off.ensure((size_t)n_nodes + 1)) || (rc = trk_zeroed(d_cursor, n_nodes, stream)) || (rc = d_list.ensure(n_matches)) ||
      (rc = d_sorted.ensure(n_matches)))
    return rc;
  const uint32_t n_lds = (uint32_t)lds_images.size(), n_big = (uint32_t)big_images.size();
  const uint32_t* const p_image_list = d_image_list.p;
  const uint32_t* const p_table_slots = d_table_slots.p;
  const trk_u64* const p_table_off = d_table_off.p;
  trk_u64* const p_tables = d_tables.p;
  uint32_t* const p_collision = d_collision.p;
  unsigned* const p_comp_nodes = d_comp_nodes.p;
  uint32_t* const p_survives = d_survives.p;
  uint32_t* const p_index = d_index.p;
  uint32_t* const p_survivors = d_survivors.p;
  unsigned* const p_comp_matches = d_comp_matches.p;
  uint32_t* const p_match_off = d_match_off.p;
  unsigned* const p_cursor = d_cursor.p;
  uint32_t* const p_list = d_list.p;
  uint32_t* const p_sorted = d_sorted.p;
  if ((rc = timer.begin(kTrkPassCollide))) return rc;
  if (n_lds)
    hipLaunchKernelGGL(trk_collide_kernel<true>, dim3(n_lds), dim3(256), 0, stream, p_image_list, (const uint32_t*)p_image_start, (const uint32_t*)p_label, p_tables,
                       p_table_off, p_table_slots, p_collision);
  if (n_big)
    hipLaunchKernelGGL(trk_collide_kernel<false>, dim3(n_big), dim3(256), 0, stream, p_image_list + n_lds, (const uint32_t*)p_image_start, (const uint32_t*)p_label,
                       p_tables, p_table_off, p_table_slots, p_collision);
  MVGX_HIP(hipGetLastError());
  if ((rc = timer.end()) || (rc = timer.begin(kTrkPassSelect))) return rc;
  hipLaunchKernelGGL(trk_count_nodes_kernel, trk_grid(n_nodes), dim3(256), 0, stream, (const uint32_t*)p_label, (const uint32_t*)p_collision, n_nodes, p_comp_nodes);
  hipLaunchKernelGGL(trk_select_kernel, trk_grid(n_nodes), dim3(256), 0, stream, (const uint32_t*)p_label, (const unsigned*)p_comp_nodes,
                     (const uint32_t*)p_collision, n_nodes, opt->min_length, p_survives, p_counters);
  MVGX_HIP(hipGetLastError());
  if ((rc = scan.run(p_survives, n_nodes, p_index, stream))) return rc;
  hipLaunchKernelGGL(trk_compact_kernel, trk_grid(n_nodes), dim3(256), 0, stream, (const uint32_t*)p_survives, (const uint32_t*)p_index, n_nodes, p_survivors);
  MVGX_HIP(hipGetLastError());
  if ((rc = timer.end()) || (rc = timer.begin(kTrkPassGather))) return rc;
  hipLaunchKernelGGL(trk_count_matches_kernel, trk_grid(n_matches), dim3(256), 0, stream, (const uint32_t*)p_a, n_matches, (const uint32_t*)p_label,
                     (const uint32_t*)p_survives, p_comp_matches);
  MVGX_HIP(hipGetLastError());
  if ((rc = scan.run(p_comp_matches, n_nodes, p_match_off, stream))) return rc;
  hipLaunchKernelGGL(trk_fill_matches_kernel, trk_grid(n_matches), dim3(256), 0, stream, (const uint32_t*)p_a, n_matches, (const uint32_t*)p_label,
                     (const uint32_t*)p_survives, (const uint32_t*)p_match_off, p_cursor, p_list);
  MVGX_HIP(hipGetLastError());
  if ((rc = timer.end())) return rc;
  MVGX_HIP(hipMemcpyAsync(counters, d_counters.p, sizeof(counters), hipMemcpyDeviceToHost, stream));
  MVGX_HIP(hipStreamSynchronize(stream));
  st.n_components = counters[1]; st.n_collision = counters[2]; st.n_short = counters[3];
  const uint32_t n_t = counters[4], n_obs = counters[5];
  st.n_obs = n_obs;
  if ((rc = trk_allocate_outputs(n_t, n_obs, track_id, track_start, obs_image, obs_feature))) return rc;
  if (!n_t) {
    st.kernel_ms = timer.collect(g_trk_pass_ms);
    return finish(0);
  }
  const auto release_outputs = [&]() { free(*track_id); free(*track_start); free(*obs_image); free(*obs_feature); *track_id = *obs_image = *obs_feature = nullptr; *track_start = nullptr; };
  const auto device_tail = [&]() -> int {
    int rc2;
    if ((rc2 = trk_zeroed(d_rank, n_nodes, stream)) || (rc2 = d_root_of.ensure(n_nodes)) || (rc2 = trk_zeroed(d_is_root, n_nodes, stream)) ||
        (rc2 = d_label_of_root.ensure(n_nodes)) || (rc2 = d_track_of_root.ensure((size_t)n_nodes + 1)) || (rc2 = d_track_id.ensure(n_t)) ||
        (rc2 = d_track_len.ensure(n_t)) || (rc2 = d_track_start.ensure((size_t)n_t + 1)) || (rc2 = d_members.ensure(n_obs)) || (rc2 = d_obs_image.ensure(n_obs)) ||
        (rc2 = d_obs_feature.ensure(n_obs)))
      return rc2;
    uint32_t* const p_rank = d_rank.p;
    uint32_t* const p_root_of = d_root_of.p;
    uint32_t* const p_is_root = d_is_root.p;
    uint32_t* const p_label_of_root = d_label_of_root.p;
    uint32_t* const p_track_of_root = d_track_of_root.p;
    uint32_t* const p_track_id = d_track_id.p;
    uint32_t* const p_track_len = d_track_len.p;
    uint32_t* const p_track_start = d_track_start.p;
    uint32_t* const p_members = d_members.p;
    uint32_t* const p_obs_image = d_obs_image.p;
    uint32_t* const p_obs_feature = d_obs_feature.p;
    // ---- replay ----
    if ((rc2 = timer.begin(kTrkPassReplay))) return rc2;
    hipLaunchKernelGGL(trk_replay_kernel, dim3(n_t), dim3(64), 0, stream, (const uint32_t*)p_survivors, (const uint32_t*)p_match_off, (const uint32_t*)p_list, p_sorted,
                       (const uint32_t*)p_a, (const uint32_t*)p_b, p_forest, p_rank, p_root_of, p_is_root, p_label_of_root);
    MVGX_HIP(hipGetLastError());
    // ---- export ----
    if ((rc2 = timer.end()) || (rc2 = timer.begin(kTrkPassExport)) || (rc2 = scan.run(p_is_root, n_nodes, p_track_of_root, stream))) return rc2;
    hipLaunchKernelGGL(trk_track_kernel, trk_grid(n_nodes), dim3(256), 0, stream, (const uint32_t*)p_is_root, (const uint32_t*)p_track_of_root,
                       (const uint32_t*)p_label_of_root, (const unsigned*)p_comp_nodes, n_nodes, p_track_id, p_track_len);
    MVGX_HIP(hipGetLastError());
    if ((rc2 = scan.run(p_track_len, n_t, p_track_start, stream))) return rc2;
    MVGX_HIP(hipMemsetAsync(d_cursor.p, 0, (size_t)n_nodes * sizeof(unsigned), stream));   // (its first life, the match cursors, is over)
    hipLaunchKernelGGL(trk_members_kernel, trk_grid(n_nodes), dim3(256), 0, stream, (const uint32_t*)p_label, (const uint32_t*)p_survives, (const uint32_t*)p_root_of,
                       (const uint32_t*)p_track_of_root, (const uint32_t*)p_track_start, n_nodes, p_cursor, p_members);
    hipLaunchKernelGGL(trk_place_kernel, trk_grid(n_nodes), dim3(256), 0, stream, (const uint32_t*)p_label, (const uint32_t*)p_survives, (const uint32_t*)p_root_of,
                       (const uint32_t*)p_track_of_root, (const uint32_t*)p_track_start, (const uint32_t*)p_members, n_nodes, (const uint32_t*)p_node_image,
                       (const uint32_t*)p_node_feature, p_obs_image, p_obs_feature);
    MVGX_HIP(hipGetLastError());
    if ((rc2 = timer.end())) return rc2;
    std::vector<uint32_t> start32((size_t)n_t + 1);
    MVGX_HIP(hipMemcpyAsync(*track_id, d_track_id.p, (size_t)n_t * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipMemcpyAsync(start32.data(), d_track_start.p, start32.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipMemcpyAsync(*obs_image, d_obs_image.p, (size_t)n_obs * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipMemcpyAsync(*obs_feature, d_obs_feature.p, (size_t)n_obs * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    MVGX_HIP(hipStreamSynchronize(stream));
    for (uint32_t t = 0; t <= n_t; ++t) (*track_start)[t] = start32[t];
    MVGX_REQUIRE(start32[n_t] == n_obs, MVGX_ERR_HIP, "mvgx_tracks_build: the tracks hold %u observations, the survivors %u nodes", start32[n_t], n_obs);
    return MVGX_OK;
  };
  if ((rc = device_tail())) { release_outputs(); return rc; }
  st.kernel_ms = timer.collect(g_trk_pass_ms);
  return finish(n_t);
}

}  // extern "C"
