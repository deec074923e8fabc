/*
 * mvgx.h — C ABI of libmvgx_hip.so: MI355X (gfx950) accelerators behind two openMVG interfaces.
 *
 *   matching : exhaustive brute-force L2 2-NN + Lowe ratio on 128-D uint8 descriptors
 *              (drop-in for openMVG::matching_image_collection::Matcher_Regions(ratio, BRUTE_FORCE_L2))
 *   ba       : Levenberg-Marquardt bundle adjustment (Jacobians -> Schur -> reduced solve -> back-substitution)
 *              (drop-in for openMVG::sfm::Bundle_Adjustment_Ceres::Adjust)
 *
 * Plain C: pointers + sizes only, no C++/torch types. Every entry point returns an int status
 * (MVGX_OK == 0) and never throws. `mvgx_last_error()` returns a thread-local message.
 *
 * Reference interfaces each entry point replaces are cited as  <path under /root/reference/src>:<line>.
 */
#ifndef MVGX_H_
#define MVGX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVGX_OK 0
#define MVGX_ERR_ARG 1      /* bad argument (null pointer, dim != 128, index out of range ...)   */
#define MVGX_ERR_HIP 2      /* a HIP runtime call failed; see mvgx_last_error()                  */
#define MVGX_ERR_NODEV 3    /* no gfx950 device visible                                          */
#define MVGX_ERR_STATE 4    /* call order violated (e.g. run before set_regions)                 */
#define MVGX_ERR_UNSUPPORTED 5 /* semantics the device path does not reproduce (ratio > 1, camera model) */
#define MVGX_ERR_NUMERIC 6  /* BA: linear solve failed / non-finite cost                         */
#define MVGX_ERR_STRUCTURE 7 /* mvgx_ba_update: the problem's structure is not the context's (the context is untouched) */

const char* mvgx_last_error(void);
int mvgx_device_count(int* count);
/* abi version, bumped on any signature or struct-layout change (2: mvgx_ba_problem control points / priors;
 * 3: mvgx_ba_get_solver_info; 4: multi-device contexts, mvgx_match_run_stream; 5: geometric filter; 6: indexed filter entry,
 * cascade hashing on the device; 7: homography model of the geometric filter; 8: iteration / clock counters in
 * mvgx_geofilter_stats, essential-matrix model of the geometric filter; 9: mvgx_host_parallel_for; 10: guided matching;
 * 11: mvgx_cascade_hash_regions_typed; 12: mvgx_guided_match for float and binary regions). Pure additions keep the number:
 * mvgx_triangulate_tracks came without a bump - a caller detects it by the symbol's presence (dlsym). */
int mvgx_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * MATCHING
 * replaces: matching_image_collection/Matcher_Regions.cpp:32-107 (Matcher_Regions::Match),
 *           matching/regions_matcher.hpp:162-207 (RegionsMatcherT::MatchDistanceRatio),
 *           matching/matcher_brute_force.hpp:100-200 (ArrayMatcherBruteForce::SearchNeighbours),
 *           matching/metric.hpp:55-93 (L2<uint8_t>), matching/matching_filters.hpp:39-60 (NNdistanceRatio)
 * ---------------------------------------------------------------------------------------------- */

typedef struct mvgx_match_ctx mvgx_match_ctx;

/* Called serially on the calling thread, once per image pair that has >= 1 putative match
 * (Matcher_Regions.cpp:95-103 inserts only non-empty vectors). `ij` holds n (i_in_I, j_in_J) uint32
 * pairs in ascending j, exactly the IndMatch(i_, j_) order of regions_matcher.hpp:198-204. */
typedef void (*mvgx_match_sink)(void* user, uint32_t I, uint32_t J, const uint32_t* ij, uint32_t n);

typedef struct mvgx_match_stats {
  uint64_t n_pairs;            /* image pairs processed on the device                              */
  uint64_t n_desc_pairs;       /* sum over processed pairs of nI * nJ distance evaluations          */
  uint64_t n_matches;          /* putative matches emitted                                          */
  uint64_t n_kernel_launches;  /* launches of the dominant kernel (l2_top2_ratio)                   */
  double   kernel_ms;          /* HIP-event time summed over those launches (profile mode only)     */
  double   total_ms;           /* HIP-event time of the whole device pass (match + compaction)      */
  uint32_t kernel_vgprs;       /* informational                                                     */
  uint32_t variant;            /* kernel variant actually used                                      */
} mvgx_match_stats;

/* device >= 0: that device. device == -1 ("no preference", what the openMVG adapter passes): the devices named by the
 * environment variable MVGX_DEVICES - "all" or a comma-separated list of ordinals; two or more make a multi-device
 * context (below) - or, when it is unset, the current HIP device. device <= -2: the current HIP device, environment ignored. */
int mvgx_match_create(int device, mvgx_match_ctx** out);
/* One context over several devices of this process (Matcher_Regions.cpp:49-54 fans the pairs of an image I out over host
 * threads; here the pair list is cut into batches that the devices take in turn, one host thread per device, no
 * collective): descriptors are replicated by set_regions, every run call shares its batches out dynamically, results are
 * identical to a single-device run. An ordinal may repeat (several contexts on one device). */
int mvgx_match_create_multi(const int* devices, int n_devices, mvgx_match_ctx** out);
int mvgx_match_destroy(mvgx_match_ctx* ctx);

/* knobs: "variant" (kernel variant id), "profile" (1: HIP events around every match-kernel launch; 2: also a statistics
 * pass that counts the candidates the filter hands to the verify stage, reported in kernel_vgprs),
 * "batch_pairs" (pairs per device batch), "keep_host_results" (0: skip D2H of the match lists),
 * "overlap" (default 1: two batch slots, batch b filters while batch b-1 is verified/compacted/copied; 0: one at a time),
 * "double_buffer_results" (default 0, see mvgx_match_run),
 * "pinned_results" (default 1: the host match lists live in pinned memory - fastest when a context is run many times;
 * 0: plain memory, for one-shot use where pinning a gigabyte costs more than the staged copies; set before the first run),
 * "stream_hold" (mvgx_match_run_stream, default 0; 1: the buffers handed to the sink stay valid until TWO further sink
 * calls have returned or the run has returned - a second set of host buffers per batch slot - so that a caller can
 * convert batch k on its own threads while batches k + 1 and k + 2 arrive),
 * "pinned_stream" (default 1: the batch buffers of mvgx_match_run_stream are pinned; 0: plain memory, for one-shot use).
 * "stream_reserve" (uint32 words per buffer): page-locks the stream's host buffers ahead of the run - callable from another thread
 *   while mvgx_match_set_regions uploads (pinning ~100 MB takes tens of milliseconds the first batches would otherwise wait for).
 * "batch_pairs" (default 32 768): image pairs per device batch - the cap B of a batch.
 * "batch_ramp" (default 1024; 0: off): the floor, in pairs, of the ramps at the two ends of a run. A run of at least 4 B pairs whose
 *   B / 8 is not below the floor starts on batches of B/8, B/4, B/2 pairs and ends on B/2, B/4, B/8 (each once per device), with
 *   equal batches of at most B between them: the work around the first and the last batch of a run, which no kernel hides, shrinks
 *   with them. Any other run is cut into steps of exactly B. The lists do not depend on it; mvgx_match_batch_schedule tells the cut.
 * "record_order" (default 1; 0: off): the default filter's work records are ordered by query image inside each XCD's share of a
 *   batch, so that the workgroups resident together read the same query tiles. The lists do not depend on it.
 *   "record_chunk_tiles" (default 256 = 1 MiB): the granule of that order in dense query tiles of 32 rows; for tests on small images.
 * Kernel selection (cross-checks and A/B runs; every combination returns the same lists): "variant" 0 = one thread per query, 1 / 2 / 3 =
 *   the exact top-2 kernel with the database window staged through registers / LDS-DMA builtin / LDS-DMA asm, 4 (default) = filter +
 *   verify. Under 4 only: "stage" 1 / 2 / 3 (default 3) = the same three staging modes, "filter_shape" 16 (default; 16x16x64 MFMA), 17
 *   (the same at three workgroups per CU) or 32 (32x32x32), "debug_filter" 0 (default), 8 or 16 = epilogue form of the 32x32x32 filter
 *   (anything else: MVGX_ERR_ARG; the environment variable MVGX_MATCH_FILTER sets it at create, other values are ignored there).
 *   The 16x16x64 kernels exist for stage 3 with debug_filter 0 only: shape 16 / 17 with stage 1 or 2, or with debug_filter 8 / 16, runs
 *   the 32x32x32 filter; stage 1 or 2 ignores debug_filter. Variants 0..3 ignore all three.
 * "verify_alone" (default 0; 1: a batch's filter kernel also waits for the verify kernel of the batch before). */
int mvgx_match_set_option(mvgx_match_ctx* ctx, const char* key, int64_t value);

/* Load the descriptor arrays of n_images images into HBM (replaces Regions_Provider::get +
 * RegionsMatcherT ctor/Build, sfm_regions_provider.hpp:76-85, regions_matcher.hpp:119-132).
 * desc_rows[k] -> n_desc[k] x dim row-major uint8 (Scalar_Regions::DescriptorRawData, scalar_regions.hpp:93);
 * may be NULL when n_desc[k] == 0. dim must be 128. The arrays are copied; the caller keeps ownership. */
int mvgx_match_set_regions(mvgx_match_ctx* ctx, const uint8_t* const* desc_rows, const uint32_t* n_desc,
                           uint32_t n_images, uint32_t dim);

/* Same, descriptors already resident on the device: one concatenated (sum n_desc) x 128 row-major uint8
 * buffer (device pointer), image k starting at row sum_{m<k} n_desc[m]. The buffer is NOT copied: it stays the
 * caller's and must remain valid and unchanged until the regions are replaced or the context is destroyed (the runs
 * read query rows from it). */
int mvgx_match_set_regions_device(mvgx_match_ctx* ctx, const void* d_desc_concat, const uint32_t* n_desc,
                                  uint32_t n_images, uint32_t dim);

/* Match `n_pairs` image pairs. pairs_IJ = 2*n_pairs uint32 (I = database image, J = query image, as
 * Matcher_Regions.cpp:57-93). ratio_sq = Square(dist_ratio) computed in float by the caller
 * (regions_matcher.hpp:196, numeric.h:56). ratio_sq > 1 -> MVGX_ERR_UNSUPPORTED (tie order would be
 * libstdc++-specific, stl/indexed_sort.hpp:48-63). Pairs whose I has < 2 descriptors or whose J is
 * empty produce no matches (matcher_brute_force.hpp:108-113, Matcher_Regions.cpp:65-69,85-90).
 * Results stay valid until the next run/destroy; with the option "double_buffer_results" = 1 until the run AFTER the next
 * one: the context then alternates between two result buffers, so a caller may consume run k on another thread while
 * run k + 1 executes (the adapter fills the match container that way). */
int mvgx_match_run(mvgx_match_ctx* ctx, const uint32_t* pairs_IJ, uint64_t n_pairs, float ratio_sq,
                   mvgx_match_stats* stats /* may be NULL */);

/* Streaming form of mvgx_match_run for runs whose match lists should not be held in host memory at once (10k images:
 * 5e7 pairs, ~1e10 matches): the lists are handed over batch by batch ("batch_pairs" image pairs each) and host memory
 * stays O(batch) - two pinned buffers per device. `sink` is entered on the CALLING thread only, one batch at a time:
 * pairs [first_pair, first_pair + n_pairs) of the input list, offsets[n_pairs + 1] relative to the batch (in matches),
 * ij = 2 uint32 per match, ascending j within a pair; the pointers are valid during the call only. Batches arrive in
 * ascending order on a single device and in any order on a multi-device context. A non-zero return stops the run (the
 * sink is not entered again; the call still returns MVGX_OK). mvgx_match_results is not affected by this call. */
typedef int (*mvgx_match_batch_sink)(void* user, uint64_t first_pair, uint32_t n_pairs, const uint32_t* offsets,
                                     const uint32_t* ij);
int mvgx_match_run_stream(mvgx_match_ctx* ctx, const uint32_t* pairs_IJ, uint64_t n_pairs, float ratio_sq,
                          mvgx_match_batch_sink sink, void* user, mvgx_match_stats* stats /* may be NULL */);

/* The batches a run over n_pairs pairs is cut into with the context's present options ("batch_pairs", "batch_ramp") and regions:
 * *n_batches receives their number, and the first min(capacity, *n_batches) entries of first_pair[] / batch_pairs[] the batches in
 * ascending order (both may be NULL with capacity 0). What a sink of mvgx_match_run_stream sees, e.g. to size its own buffers. */
int mvgx_match_batch_schedule(mvgx_match_ctx* ctx, uint64_t n_pairs, uint64_t* first_pair, uint32_t* batch_pairs, uint64_t capacity,
                              uint64_t* n_batches);

/* Host view of the last run: offsets[n_pairs+1] into ij (in units of matches); ij = 2 uint32 per match. */
int mvgx_match_results(mvgx_match_ctx* ctx, const uint64_t** offsets, const uint32_t** ij);

/* One-shot convenience with the exact shape of Matcher_Regions::Match: upload, run, and feed `sink`
 * pair by pair in ascending (I, J) order of the input list. */
int mvgx_match_pairs_u8_l2(const uint8_t* const* desc_rows, const uint32_t* n_desc, uint32_t n_images,
                           uint32_t dim, const uint32_t* pairs_IJ, uint64_t n_pairs, float ratio_sq,
                           int device, mvgx_match_sink sink, void* user);

/* ------------------------------------------------------------------------------------------------
 * MATCHING OF BINARY DESCRIPTORS (BRUTE_FORCE_HAMMING)
 * replaces, behind the same factory as the L2 path (matching/regions_matcher.cpp:184-191):
 *   RegionsMatcherT<ArrayMatcherBruteForce<unsigned char, Hamming<unsigned char>>>(regions, false) on binary regions
 *   (features::Binary_Regions<SIOPointFeature, 64> = AKAZE_Binary_Regions, features/regions_factory.hpp:26):
 *   matching/metric_hamming.hpp:36-107 (popcount of the XOR, unsigned int), matching/matcher_brute_force.hpp:95-200,
 *   MatchDistanceRatio with the ratio as given (regions_matcher.hpp:162-207), inside the I/J loops of
 *   Matcher_Regions::Match (Matcher_Regions.cpp:57-105). Same call shapes as mvgx_match_*; the ratio is dist_ratio itself
 *   (the metric is not squared), accepted range 0 <= dist_ratio <= 1. desc_bytes: 1..64 (AKAZE MLDB: 64).
 * ---------------------------------------------------------------------------------------------- */
typedef struct mvgx_hamming_ctx mvgx_hamming_ctx;
int mvgx_hamming_create(int device, mvgx_hamming_ctx** out);
int mvgx_hamming_destroy(mvgx_hamming_ctx* ctx);
int mvgx_hamming_set_option(mvgx_hamming_ctx* ctx, const char* key /* "batch_pairs" */, int64_t value);
/* desc_rows[k] -> n_desc[k] x desc_bytes row-major bytes (Binary_Regions::DescriptorRawData, binary_regions.hpp) */
int mvgx_hamming_set_regions(mvgx_hamming_ctx* ctx, const uint8_t* const* desc_rows, const uint32_t* n_desc,
                             uint32_t n_images, uint32_t desc_bytes);
int mvgx_hamming_run(mvgx_hamming_ctx* ctx, const uint32_t* pairs_IJ, uint64_t n_pairs, float dist_ratio,
                     mvgx_match_stats* stats /* may be NULL */);
int mvgx_hamming_results(mvgx_hamming_ctx* ctx, const uint64_t** offsets, const uint32_t** ij);

/* ------------------------------------------------------------------------------------------------
 * MATCHING OF FLOAT DESCRIPTORS (BRUTE_FORCE_L2 on Scalar_Regions<SIOPointFeature, float, 64> = AKAZE_Float_Regions)
 * replaces matching/regions_matcher.cpp:119-124: RegionsMatcherT<ArrayMatcherBruteForce<float, L2<float>>>(regions, true);
 * L2<float> (matching/metric.hpp:98-135) is evaluated with the reference's own operation order in IEEE binary32 without
 * contraction, so distances - and therefore the match lists - are bit-identical, not merely close.
 * Same call shapes as mvgx_match_*; ratio_sq = Square(dist_ratio) in float, accepted range 0 <= ratio_sq <= 1; dim must be 64.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mvgx_l2f_ctx mvgx_l2f_ctx;
int mvgx_l2f_create(int device, mvgx_l2f_ctx** out);
int mvgx_l2f_destroy(mvgx_l2f_ctx* ctx);
int mvgx_l2f_set_option(mvgx_l2f_ctx* ctx, const char* key /* "batch_pairs" */, int64_t value);
/* desc_rows[k] -> n_desc[k] x dim row-major floats (Scalar_Regions::DescriptorRawData, scalar_regions.hpp:93) */
int mvgx_l2f_set_regions(mvgx_l2f_ctx* ctx, const float* const* desc_rows, const uint32_t* n_desc, uint32_t n_images,
                         uint32_t dim);
int mvgx_l2f_run(mvgx_l2f_ctx* ctx, const uint32_t* pairs_IJ, uint64_t n_pairs, float ratio_sq,
                 mvgx_match_stats* stats /* may be NULL */);
int mvgx_l2f_results(mvgx_l2f_ctx* ctx, const uint64_t** offsets, const uint32_t** ij);

/* ------------------------------------------------------------------------------------------------
 * MATCHING OF uint8 DESCRIPTORS OF OTHER LENGTHS (BRUTE_FORCE_L2 on Scalar_Regions<SIOPointFeature, unsigned char, N>,
 * N = 144: AKAZE_Liop_Regions, features/regions_factory.hpp:24)
 * replaces matching/regions_matcher.cpp:75-81 for those region types; L2<uint8_t> (matching/metric.hpp:55-93) in exact integer
 * arithmetic (v_dot4_u32_u8), so the lists are bit-identical. Same call shapes as mvgx_match_* (ratio_sq = Square(dist_ratio));
 * dim must be 64, 128 or 144 - SIFT's 128 is better served by mvgx_match_* (the MFMA path) and accepted here as a cross-check.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mvgx_l2u8_ctx mvgx_l2u8_ctx;
int mvgx_l2u8_create(int device, mvgx_l2u8_ctx** out);
int mvgx_l2u8_destroy(mvgx_l2u8_ctx* ctx);
int mvgx_l2u8_set_option(mvgx_l2u8_ctx* ctx, const char* key /* "batch_pairs" */, int64_t value);
int mvgx_l2u8_set_regions(mvgx_l2u8_ctx* ctx, const uint8_t* const* desc_rows, const uint32_t* n_desc, uint32_t n_images,
                          uint32_t dim);
int mvgx_l2u8_run(mvgx_l2u8_ctx* ctx, const uint32_t* pairs_IJ, uint64_t n_pairs, float ratio_sq,
                  mvgx_match_stats* stats /* may be NULL */);
int mvgx_l2u8_results(mvgx_l2u8_ctx* ctx, const uint64_t** offsets, const uint32_t** ij);

/* ------------------------------------------------------------------------------------------------
 * CASCADE HASHING (CASCADE_HASHING_L2, the default nearest-neighbour method of main_ComputeMatches for scalar regions)
 * replaces the MATCHING stage of matching_image_collection/Cascade_Hashing_Matcher_Regions.cpp:134-215:
 *   matching/cascade_hasher.hpp:241-367 CascadeHasher::Match_HashedDescriptions (candidates from the query's bucket in every
 *   bucket group, de-duplicated in order of appearance, the ten nearest in Hamming distance of the hash codes, exact
 *   L2<uint8> on those, the two smallest (distance, id) pairs) and the NNdistanceRatio test with Square(dist_ratio).
 * The HASHING stage (cascade_hasher.hpp:154-239: zero-mean descriptor, primary / secondary random projections - single-
 * precision Eigen products) stays host code of the caller; its per-descriptor outputs are inputs here, so the device part
 * is integer work and the lists are bit-identical for any ratio. The openMVG adapter runs the reference's own
 * CascadeHasher for the hashing stage and applies the reference's two de-duplication steps (:218-226) to the lists.
 *   desc_rows[k]  n_desc[k] x 128 uint8      hash_codes[k]  n_desc[k] x 16 bytes (stl::dynamic_bitset blocks)
 *   bucket_ids[k] n_desc[k] x n_groups uint16 (HashedDescription::bucket_ids), values < 2^bits_per_bucket
 * Results: per pair the list BEFORE de-duplication, (descriptor of I, descriptor of J) in ascending J.
 * ---------------------------------------------------------------------------------------------- */
typedef struct mvgx_cascade_ctx mvgx_cascade_ctx;
int mvgx_cascade_create(int device, mvgx_cascade_ctx** out);
int mvgx_cascade_destroy(mvgx_cascade_ctx* ctx);
int mvgx_cascade_set_option(mvgx_cascade_ctx* ctx, const char* key /* "batch_pairs" */, int64_t value);
int mvgx_cascade_set_regions(mvgx_cascade_ctx* ctx, const uint8_t* const* desc_rows, const uint8_t* const* hash_codes,
                             const uint16_t* const* bucket_ids, const uint32_t* n_desc, uint32_t n_images, uint32_t dim,
                             uint32_t hash_bytes, uint32_t n_groups, uint32_t bits_per_bucket);
/* ... for the other scalar region types Cascade_Hashing_Matcher_Regions.cpp:233-262 accepts (ABI 9): scalar_type 0 = uint8 rows of
 * 128 (SIFT_Regions) or 144 bytes (AKAZE_Liop_Regions), 1 = float rows of length 64 (AKAZE_Float_Regions: the ten candidates are
 * ranked by L2<float> in the reference's summation order, the ratio test runs on the float distances). hash_bytes = (dim + 7) / 8:
 * CascadeHasher::Init(dimension) makes one code bit per dimension. The hashing stage of these types stays with the caller. */
int mvgx_cascade_set_regions_typed(mvgx_cascade_ctx* ctx, int scalar_type, const void* const* desc_rows, const uint8_t* const* hash_codes,
                                   const uint16_t* const* bucket_ids, const uint32_t* n_desc, uint32_t n_images, uint32_t dim,
                                   uint32_t hash_bytes, uint32_t n_groups, uint32_t bits_per_bucket);
/* The HASHING stage on the device (cascade_hasher.hpp:120-163 Init, :179-239 CreateHashedDescriptions) in place of
 * mvgx_cascade_set_regions: the projections are generated like CascadeHasher::Init(dim, n_groups, bits_per_bucket, random_seed)
 * (std::mt19937 + std::normal_distribution<>, the reference's default seed is 5489), every descriptor is centred on zero_mean
 * (dim floats: the caller's CascadeHasher::GetZeroMeanDescriptor result) and projected with the operation order of Eigen 3.4's
 * single-precision column-major matrix x vector kernel (column blocks of 16, products and sums rounded separately - no FMA, as
 * in a reference build without -mfma), so codes and bucket ids equal the reference's bit for bit (tests/test_cascade.py against
 * the compiled reference). hash_codes_out[k] (n_desc[k] x 16 bytes) / bucket_ids_out[k] (n_desc[k] x n_groups uint16) receive
 * the per-descriptor outputs when non-NULL. */
int mvgx_cascade_hash_regions(mvgx_cascade_ctx* ctx, const uint8_t* const* desc_rows, const uint32_t* n_desc, uint32_t n_images, uint32_t dim,
                              const float* zero_mean, uint32_t n_groups, uint32_t bits_per_bucket, uint32_t random_seed,
                              uint8_t* const* hash_codes_out /* may be NULL */, uint16_t* const* bucket_ids_out /* may be NULL */);
/* The same for every shape the device covers (ABI 11): scalar_type 0 = uint8 rows of 128 or 144 bytes, 1 = float rows of length 64 (the shapes
 * of mvgx_cascade_set_regions_typed); dim code bits per descriptor ((dim + 7) / 8 bytes in hash_codes_out). Eigen's kernel walks 144 columns
 * in nine blocks of 16 and 64 columns as one block (block_cols = cols below 128): the same order here, the same bits (tests/test_cascade_typed.py
 * against the compiled reference's CascadeHasher). */
int mvgx_cascade_hash_regions_typed(mvgx_cascade_ctx* ctx, int scalar_type, const void* const* desc_rows, const uint32_t* n_desc, uint32_t n_images, uint32_t dim,
                                    const float* zero_mean, uint32_t n_groups, uint32_t bits_per_bucket, uint32_t random_seed,
                                    uint8_t* const* hash_codes_out /* may be NULL */, uint16_t* const* bucket_ids_out /* may be NULL */);
int mvgx_cascade_run(mvgx_cascade_ctx* ctx, const uint32_t* pairs_IJ, uint64_t n_pairs, float ratio_sq,
                     mvgx_match_stats* stats /* may be NULL */);
int mvgx_cascade_results(mvgx_cascade_ctx* ctx, const uint64_t** offsets, const uint32_t** ij);

/* ------------------------------------------------------------------------------------------------
 * BUNDLE ADJUSTMENT
 * replaces: sfm/sfm_data_BA_ceres.cpp:165-608 (Bundle_Adjustment_Ceres::Adjust) and, underneath it,
 *           vendored Ceres 1.13: program_evaluator.h:138-285, residual_block.cc:68-196, corrector.cc:41-155,
 *           schur_eliminator_impl.h:176-410, schur_complement_solver.cc:120-224,
 *           levenberg_marquardt_strategy.cc:65-160, trust_region_minimizer.cc:66-786
 * ---------------------------------------------------------------------------------------------- */

typedef struct mvgx_ba_ctx mvgx_ba_ctx;

/* camera models, numeric values of cameras::EINTRINSIC (cameras/Camera_Common.hpp:39-50) */
#define MVGX_CAM_PINHOLE 1          /* PINHOLE_CAMERA          params {f, ppx, ppy}              */
#define MVGX_CAM_PINHOLE_RADIAL1 2  /* PINHOLE_CAMERA_RADIAL1  params {f, ppx, ppy, k1}          */
#define MVGX_CAM_PINHOLE_RADIAL3 3  /* PINHOLE_CAMERA_RADIAL3  params {f, ppx, ppy, k1, k2, k3}  */
#define MVGX_CAM_PINHOLE_BROWN 4    /* PINHOLE_CAMERA_BROWN    params {f, ppx, ppy, k1, k2, k3, t1, t2} */
#define MVGX_CAM_PINHOLE_FISHEYE 5  /* PINHOLE_CAMERA_FISHEYE  params {f, ppx, ppy, k1, k2, k3, k4} */
#define MVGX_CAM_SPHERICAL 7        /* CAMERA_SPHERICAL: no parameter block (getParams() is empty, sfm_data_BA_ceres.cpp:366-383);
                                       the intrinsics row carries the image size {w, h} the functor needs           */
#define MVGX_BA_MAX_INTR_PARAMS 8

typedef struct mvgx_ba_problem {
  uint32_t n_poses, n_intrinsics, n_points;
  uint64_t n_obs;
  /* parameter blocks, layouts of sfm_data_BA_ceres.cpp:260-351 */
  const double* poses;        /* n_poses x 6: angle-axis(3), translation(3) with t = -R*C          */
  const double* intrinsics;   /* n_intrinsics x MVGX_BA_MAX_INTR_PARAMS (unused tail ignored)      */
  const int32_t* intr_model;  /* n_intrinsics: MVGX_CAM_*                                          */
  const double* points;       /* n_points x 3                                                      */
  /* observations (one residual block each, sfm_data_BA_ceres.cpp:354-396) */
  const uint32_t* obs_pose;   /* n_obs */
  const uint32_t* obs_intr;   /* n_obs */
  const uint32_t* obs_point;  /* n_obs */
  const double* obs_xy;       /* n_obs x 2 */
  /* constant-parameter masks (bit k set = component k of the block held constant;
   * all bits of the block set = SetParameterBlockConstant). NULL = everything free. */
  const uint8_t* pose_const_mask;   /* n_poses, bits 0..5   (Extrinsic_Parameter_Type, sfm_data_BA.hpp:28-34) */
  const uint8_t* intr_const_mask;   /* n_intrinsics, bits 0..7 (subsetParameterization, Camera_Intrinsics.hpp) */
  uint8_t points_constant;          /* Structure_Parameter_Type::NONE (sfm_data_BA.hpp:38-42)      */
  double huber_a;                   /* HuberLoss(a): sfm_data_BA_ceres.cpp:249 uses Square(4.0)=16; <=0: no loss */
  /* ---- optional (NULL / 0 = absent): ground control points and pose-centre priors ---- */
  const double* obs_weight;         /* n_obs: residual weight of WeightedCostFunction (camera_functor.hpp:35-90);
                                       0 = the unweighted functor (IntrinsicsToCostFunction's weight == 0.0 case)          */
  const uint8_t* obs_is_control;    /* n_obs: 1 = residual block of a control point: added WITHOUT loss function
                                       (sfm_data_BA_ceres.cpp:421-435) and not part of the RMSE (not a Landmark)          */
  const uint8_t* point_const_mask;  /* n_points: 1 = SetParameterBlockConstant on this point (control points, :447)       */
  uint32_t n_pose_priors;           /* PoseCenterConstraintCostFunction residuals (sfm_data_BA_ceres.cpp:44-80,454-473)   */
  const uint32_t* prior_pose;       /* n_pose_priors: pose block index                                                    */
  const double* prior_center;       /* n_pose_priors x 3: ViewPriors::pose_center_                                        */
  const double* prior_weight;       /* n_pose_priors x 3: ViewPriors::center_weight_                                      */
  double prior_huber_a;             /* HuberLoss(a) of the priors: Square(pose_center_robust_fitting_error); may be 0     */
} mvgx_ba_problem;

typedef struct mvgx_ba_options {
  int32_t max_num_iterations;   /* 50  (sfm_data_BA_ceres.cpp:120,478)           */
  double function_tolerance;    /* 1e-6 (ceres solver.h:91)                       */
  double gradient_tolerance;    /* 1e-10 (sfm_data_BA_ceres.cpp:117)              */
  double parameter_tolerance;   /* 1e-8  (sfm_data_BA_ceres.cpp:118)              */
  double initial_radius;        /* 1e4  (solver.h:84)                             */
  double max_radius;            /* 1e16                                           */
  double min_radius;            /* 1e-32                                          */
  double min_relative_decrease; /* 1e-3                                           */
  double min_lm_diagonal;       /* 1e-6                                           */
  double max_lm_diagonal;       /* 1e32                                           */
  int32_t max_consecutive_invalid_steps; /* 5                                     */
  int32_t jacobi_scaling;       /* 1                                              */
  int32_t verbose;              /* 0                                              */
} mvgx_ba_options;

typedef struct mvgx_ba_summary {
  int32_t num_iterations;         /* LM iterations executed (successful + unsuccessful)            */
  int32_t num_successful_steps;
  int32_t termination;            /* 0 convergence, 1 no-convergence (max iters), 2 failure         */
  double initial_cost, final_cost;      /* 1/2 sum rho(|r|^2), as ceres Solver::Summary             */
  double initial_rmse, final_rmse;      /* sqrt(sum |x - proj|^2 / (2 n_obs)), sfm_data_BA_test.cpp:310-330 */
  double total_ms;                /* device wall time of the solve (HIP events)                     */
  double iter_ms_mean;            /* mean time of one LM iteration                                  */
  double jacobian_ms, schur_ms, solve_ms, backsub_ms, cost_ms; /* per-phase device time summed over the context's life
                                   * when MVGX_BA_PHASE_TIMING=1 was set at create (HIP events), else 0            */
} mvgx_ba_summary;

void mvgx_ba_default_options(mvgx_ba_options* opt);
/* device >= 0: that device; -1 ("no preference", what the openMVG adapter passes): MVGX_DEVICES ("all" or a list of
 * ordinals) names the device(s) - two or more make a multi-device context when the problem has at least
 * MVGX_BA_MULTI_MIN_OBS observations (default 200 000; smaller problems use the first one) - or, unset, the current
 * device; <= -2: the current device, environment ignored. */
int mvgx_ba_create(int device, const mvgx_ba_problem* problem, mvgx_ba_ctx** out);
/* One context over several devices of THIS process (sfm_data_BA_ceres.cpp:165-608 is one call of one process): the
 * problem is cut as described under "multi-GPU" below (points + their observations partitioned by sum L_p^2, camera blocks
 * replicated, priors on the first shard), one single-device context and one host thread per shard, the per-iteration sums
 * go over RCCL (distinct devices, librccl present) or over peer-mapped device memory (MVGX_BA_TRANSPORT=rccl|peer forces
 * either; an ordinal may repeat with the peer transport). Every entry point below accepts such a context; results
 * (parameters, residuals, track angles) come back in the caller's numbering. */
int mvgx_ba_create_multi(const int* devices, int n_devices, const mvgx_ba_problem* problem, mvgx_ba_ctx** out);
int mvgx_ba_destroy(mvgx_ba_ctx* ctx);
/* Re-binds an existing context to a problem of the SAME structure and new values - what an SfM engine's consecutive Adjust() calls
 * on one scene are when nothing was added or removed in between (global_SfM.cpp's three refinement passes with growing parameter
 * sets; a caller's own re-runs; sequential_SfM.cpp:1190-1232 whenever the rejection step removed nothing): the host structure
 * build, the device allocations and the symbolic phase of the reduced solve of mvgx_ba_create are kept, only values are uploaded.
 *   structure (must be equal, compared through a 128-bit fingerprint taken at create): the counts, obs_pose / obs_intr / obs_point,
 *     intr_model, points_constant, point_const_mask, obs_is_control, presence of obs_weight, prior_pose;
 *   values (taken from `problem`): poses, intrinsics, points, obs_xy, obs_weight, prior_center / prior_weight, pose_const_mask,
 *     intr_const_mask, huber_a, prior_huber_a.
 * Returns MVGX_OK (the next mvgx_ba_solve starts from the new values with a fresh trust-region state; results are bit-identical
 * to a context created from `problem`), or MVGX_ERR_STRUCTURE when the structure differs: the context is untouched and still
 * solves its old problem; the caller destroys it and creates a new one. Works on single- and multi-device contexts. (ABI 9) */
int mvgx_ba_update(mvgx_ba_ctx* ctx, const mvgx_ba_problem* problem);
/* mvgx_ba_update with some observations switched off: `problem` still has the context's structure, obs_enabled[k] == 0 (k in the
 * order of the problem's observation arrays) removes observation k from the program - no residual, no Jacobian rows, no cost, not
 * in the RMSE, not in the track's angle - a point left without observations stops being a parameter (it keeps its value, takes no
 * step, does not count in the parameter norm) and a pose / intrinsic block left without observations leaves the program, as when the
 * reference builds its problem from a scene those observations and tracks were erased from (the rejection step of
 * sequential_SfM.cpp:1190-1232: RemoveOutliers_* erase, then Adjust() again). Equal to a context created from the reduced scene up to
 * the order of the sums (the point groups are the original ones): same iterations and decisions on the test scenes, final RMSE to
 * 1e-12. mvgx_ba_residuals / mvgx_ba_track_angles keep the indexing of `problem`. obs_enabled NULL = mvgx_ba_update; a later
 * mvgx_ba_update switches everything back on. MVGX_ERR_UNSUPPORTED on a multi-device context. (ABI 9) */
int mvgx_ba_update_subset(mvgx_ba_ctx* ctx, const mvgx_ba_problem* problem, const uint8_t* obs_enabled);
/* The library's persistent host workers (the ones the structure build of mvgx_ba_create runs on; started on first use, parked
 * between jobs), lent to the host side of a caller - the replacement TU flattens SfM_Data with them instead of starting threads
 * of its own per Adjust() call. fn(user, item, worker) runs once for every item in [0, n_items), items handed out one at a time in
 * ascending order, worker < max(1, min(max_workers or 32, hardware threads)) identifies the executing thread (0 = the caller);
 * returns when every item is done. Not re-entrant from inside fn. (ABI 9) */
typedef void (*mvgx_host_item_fn)(void* user, uint64_t item, unsigned worker);
int mvgx_host_parallel_for(uint64_t n_items, unsigned max_workers, mvgx_host_item_fn fn, void* user);
/* ---- multi-GPU (one process per GPU) --------------------------------------------------------------
 * Every rank creates its context from ITS shard of the problem: all poses and intrinsics (replicated, same
 * order on every rank) and a disjoint subset of the points together with ALL observations of those points
 * (a point's rows must be local to be eliminated, ceres schur_eliminator_impl.h:114-151). Per LM iteration
 * the solver sums across ranks: cost, camera column norms + gradient, the partial reduced camera system
 * (S, rhs), the model-cost change and the point parts of |step|^2 / |x|^2; max: gradient max-norm and the
 * failure flag. Every rank then factors the same S (no second exchange) and back-substitutes its points.
 * Either bind RCCL (mvgx_ba_comm_init: ncclAllReduce on the solver's stream, unique id from
 * mvgx_comm_unique_id on rank 0, distributed by the caller) or supply a callback transport. */
#define MVGX_REDUCE_SUM 0
#define MVGX_REDUCE_MAX 1
typedef int (*mvgx_allreduce_f64)(void* user, void* device_buffer, uint64_t count, int op, void* hip_stream);
int mvgx_ba_set_allreduce(mvgx_ba_ctx* ctx, mvgx_allreduce_f64 fn, void* user);
int mvgx_comm_unique_id(void* out128 /* 128 bytes: ncclUniqueId */);
int mvgx_ba_comm_init(mvgx_ba_ctx* ctx, int world, int rank, const void* unique_id128);
int mvgx_ba_solve(mvgx_ba_ctx* ctx, const mvgx_ba_options* opt, mvgx_ba_summary* summary);
/* one LM iteration (Jacobian + Schur + reduced solve + back-substitution + candidate cost + accept/reject) */
int mvgx_ba_lm_iteration(mvgx_ba_ctx* ctx, const mvgx_ba_options* opt, mvgx_ba_summary* summary);
/* copy the current parameter blocks back (same layouts as mvgx_ba_problem) */
int mvgx_ba_read_params(mvgx_ba_ctx* ctx, double* poses, double* intrinsics, double* points);
/* residual-only evaluation at the current parameters: cost (1/2 sum rho) and RMSE (no loss) */
int mvgx_ba_evaluate(mvgx_ba_ctx* ctx, double* cost, double* rmse);
/* |x - project(pose(X))| in pixels for every observation at the current parameters (unweighted, no loss), in the order
 * of the problem's observation arrays: the quantity RemoveOutliers_PixelResidualError (sfm/sfm_data_filters.cpp:40-73)
 * compares with its threshold in the "do { BA } while (badTrackRejector)" loops (sequential_SfM.cpp:206-210,1226-1232). */
int mvgx_ba_residuals(mvgx_ba_ctx* ctx, double* residual_norm /* n_obs */);
/* per point (track): the largest angle in degrees between the world rays of two of its observations at the current
 * poses / intrinsics (undistorted pixel -> bearing -> R^T, cameras/Camera_Intrinsics.hpp:263-280), 0 for tracks with fewer
 * than two observations: the quantity RemoveOutliers_AngleError (sfm/sfm_data_filters.cpp:77-121) compares with
 * dMinAcceptedAngle - the second half of badTrackRejector (sequential_SfM.cpp:1226-1232). */
int mvgx_ba_track_angles(mvgx_ba_ctx* ctx, double* max_angle_deg /* n_points */);

/* How the reduced camera system of this context is solved (decided at the first iteration, on the union of the ranks'
 * block patterns): the reference picks SPARSE_SCHUR above 100 poses (sfm/pipelines/sequential/sequential_SfM.cpp:1193-1205,
 * ceres schur_complement_solver.cc:241-347); here a block-sparse tile Cholesky in a nested-dissection order is used
 * whenever it needs fewer rounds of dependent launches than the dense sweep and no more tiles, the dense blocked Cholesky otherwise.
 * MVGX_BA_SOLVER=dense|sparse (environment, read at create) forces either. */
typedef struct mvgx_ba_solver_info {
  int32_t sparse;          /* 1: block-sparse tile Cholesky, 0: dense                                              */
  int32_t n_columns;       /* N = 6 n_poses + 8 n_intrinsics                                                       */
  int32_t n_padded;        /* sparse: columns after padding every part of the dissection to a multiple of 64      */
  int32_t n_parts;         /* sparse: parts of the nested dissection (incl. the dense border)                      */
  int32_t n_border_blocks; /* sparse: camera blocks ordered last as dense border (e.g. shared intrinsics)          */
  int32_t n_levels;        /* sparse: levels of the tile elimination tree = rounds of dependent launches           */
  int64_t n_factor_tiles;  /* 64 x 64 tiles of the factor's lower triangle (dense: nt (nt + 1) / 2)                */
  int64_t n_dense_tiles;   /* nt (nt + 1) / 2 with nt = ceil(N / 64)                                               */
  double flops;            /* floating-point operations of one factorisation + solve on the stored tiles           */
  /* Schur assembly: points whose pose x pose products are formed group-wise on the f64 matrix cores (groups of up to 42
   * points that share a set of at most 10 poses); the other points go through the flat product list                   */
  int32_t n_point_groups;
  int32_t n_grouped_points;
} mvgx_ba_solver_info;
int mvgx_ba_get_solver_info(mvgx_ba_ctx* ctx, mvgx_ba_solver_info* out);   /* MVGX_ERR_STATE before the first iteration */
/* The caller's choice of linear solver (ABI 9) - Bundle_Adjustment_Ceres::BA_Ceres_options::linear_solver_type_
 * (sfm/sfm_data_BA_ceres.cpp:132-146 default, :483 handed to ceres; sequential_SfM.cpp:1193-1205 and the other engines pick
 * DENSE_SCHUR or SPARSE_SCHUR by the pose count): both are direct solves of the Schur complement, what differs is the storage and
 * factorisation of the reduced camera system. AUTO is the library's rule above; DENSE the dense blocked Cholesky; SPARSE the block-
 * sparse tile Cholesky (MVGX_ERR_UNSUPPORTED when its task lists cannot be built); SPARSE_PREFERRED falls back to DENSE in that case
 * (what the replacement TU passes for SPARSE_SCHUR). Before the first iteration the symbolic phase is simply run again; afterwards
 * MVGX_OK when the solver in place is the one asked for, else MVGX_ERR_STATE. The environment's MVGX_BA_SOLVER (dense | sparse |
 * auto) outranks this call. ceres' iterative types (ITERATIVE_SCHUR, CGNR) have no counterpart: see INTEGRATION.md. */
enum { MVGX_BA_LINEAR_SOLVER_AUTO = 0, MVGX_BA_LINEAR_SOLVER_DENSE = 1, MVGX_BA_LINEAR_SOLVER_SPARSE = 2, MVGX_BA_LINEAR_SOLVER_SPARSE_PREFERRED = 3 };
int mvgx_ba_set_linear_solver(mvgx_ba_ctx* ctx, int kind);

/* ---- geometric filter of putative matches: a-contrario fundamental-matrix estimation --------------------------
 * Replaces, per image pair of a putative-match container, GeometricFilter_FMatrix_AC::Robust_estimation
 * (matching_image_collection/F_ACRobust.hpp:65-122): ACKernelAdaptor<SevenPointSolver, EpipolarDistanceError, UnnormalizerT>
 * (robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:104-202) + ACRANSAC
 * (robust_estimation/robust_estimator_ACRansac.hpp:339-489), as called for every pair by
 * ImageCollectionGeometricFilter::Robust_model_estimation (matching_image_collection/GeometricFilter.hpp:66-131).
 * Pair p owns the correspondences [match_start[p], match_start[p + 1]) of xI / xJ: (undistorted) pixel positions of the matched
 * features in image I / J, what MatchesPairToMat (Geometric_Filter_utils.hpp:56-64) builds, in the order of the pair's IndMatches;
 * image_wh[4 p ..] = {w_I, h_I, w_J, h_J} (View::ui_width / ui_height). Outputs: inlier_mask[m] = 1 for the geometric inliers of a
 * pair whose estimation succeeded (the reference's geometric_inliers are the putative matches with mask 1, in their order),
 * results[p]. One wave of the device runs one pair; pairs with at most 7 correspondences are rejected without estimation like the
 * reference does. Not reproduced (MVGX_ERR_UNSUPPORTED): an unbounded precision (the exhaustive NFA form), pairs with more than
 * 2^20 correspondences (up to 12 000 a wave's tables are in LDS, above that in global scratch). Parity: same sample sequence, tables and NFA arithmetic; the minimal solver's null space is computed by
 * elimination instead of Eigen's eigen-solver, so models agree to rounding, not bit for bit (parity policy). */
typedef struct mvgx_geofilter_options {
  double precision;          /* GeometricFilter_FMatrix_AC::m_dPrecision, pixels (main_GeometricFilter: 4.0)  */
  uint32_t max_iterations;   /* m_stIteration (main_GeometricFilter: 2048; constructor default 1024)          */
} mvgx_geofilter_options;
typedef struct mvgx_geofilter_result {
  double F[9];               /* m_F, row-major, in pixel coordinates (identity if no model was found)          */
  double precision_robust;   /* ACRansacOut.first -> m_dPrecision_robust (pixels)                              */
  double nfa;                /* ACRansacOut.second                                                             */
  uint32_t n_inliers;        /* |vec_inliers|                                                                  */
  uint32_t ok;               /* Robust_estimation's return value: n_inliers > 2.5 x 7                          */
} mvgx_geofilter_result;
typedef struct mvgx_geofilter_stats {
  uint64_t n_pairs, n_pairs_estimated, n_pairs_ok, n_inliers;
  double kernel_ms;          /* device time of the estimation kernels (HIP events)                             */
  double host_prepare_ms;    /* normalisation + per-pair constants on host threads                             */
  double total_ms;           /* the whole call incl. transfers                                                 */
  /* measurement (ABI version 8): what the estimation waves did, summed over the estimated pairs                  */
  uint64_t n_iterations;     /* a-contrario iterations run (sample + fit + evaluation of its models)           */
  uint64_t n_models;         /* models evaluated (F: 1 - 3 per iteration, H: 1)                                */
  uint64_t wave_clocks;      /* shader clocks (s_memtime) from the first to the last instruction of every wave */
} mvgx_geofilter_stats;
int mvgx_geofilter_f_acransac(int device, const double* xI, const double* xJ, const uint64_t* match_start, const uint32_t* image_wh,
                              uint64_t n_pairs, const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                              mvgx_geofilter_stats* stats /* may be NULL */);
/* The same estimation on a PairWiseMatches-shaped input: instead of gathered coordinates (MatchesPairToMat,
 * Geometric_Filter_utils.hpp:56-64, per pair) the caller hands over the feature positions of every image once - feat_xy, image k
 * owning rows [feat_start[k], feat_start[k + 1]) - and per pair its two images (pairs[2 p], pairs[2 p + 1]) and the index pairs
 * (i, j) of its putative matches (ij rows [match_start[p], match_start[p + 1])): exactly what Matcher_Regions::Match produces.
 * image_wh is per IMAGE here: {w, h}. The gather runs on the device; results, mask and statistics as above. Image or feature
 * indices out of range -> MVGX_ERR_ARG. */
int mvgx_geofilter_f_acransac_indexed(int device, const double* feat_xy, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                      const uint32_t* pairs, const uint64_t* match_start, const uint32_t* ij, uint64_t n_pairs,
                                      const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                                      mvgx_geofilter_stats* stats /* may be NULL */);

/* The homography model of the same filter: GeometricFilter_HMatrix_AC::Robust_estimation (matching_image_collection/H_ACRobust.hpp:49-113) -
 * ACKernelAdaptor<homography::kernel::FourPointSolver, AsymmetricError, UnnormalizerI> with the point-to-point error model
 * (multiview/solver_homography_kernel.cpp:37-93, solver_homography_kernel.hpp:60-64) + the same ACRANSAC. Same arguments, result
 * layout and limits as the two entries above; result.F holds m_H (x_J ~ H x_I, pixels), ok is n_inliers > 2.5 x 4, pairs with at most
 * 4 correspondences are rejected without estimation. Parity: as for F - the null vector of the 8 x 9 DLT system comes from
 * complete-pivoting elimination instead of Eigen's JacobiSVD (the same line to rounding; a rank-deficient sample has a family of
 * null vectors and the two methods pick different members). */
int mvgx_geofilter_h_acransac(int device, const double* xI, const double* xJ, const uint64_t* match_start, const uint32_t* image_wh,
                              uint64_t n_pairs, const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                              mvgx_geofilter_stats* stats /* may be NULL */);
int mvgx_geofilter_h_acransac_indexed(int device, const double* feat_xy, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                      const uint32_t* pairs, const uint64_t* match_start, const uint32_t* ij, uint64_t n_pairs,
                                      const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                                      mvgx_geofilter_stats* stats /* may be NULL */);
/* The essential-matrix model, GeometricFilter_EMatrix_AC (matching_image_collection/E_ACRobust.hpp:39-150; main_GeometricFilter -g e,
 * the model of the calibrated pipelines): ACKernelAdaptorEssential<FivePointSolver, EpipolarDistanceError> + ACRANSAC with samples of
 * five, up to ten models per sample (multiview/solver_essential_five_point.cpp:170-230 on the device: null space, constraint expansion,
 * Gauss-Jordan elimination, Hessenberg + shifted QR iteration of the 10 x 10 action matrix, one wave per image pair), residuals =
 * EpipolarDistanceError of F = K_J^-T E K_I^-1 on the PIXEL positions, precision in pixels (no normalisation), acceptance above
 * 2.5 x 5 inliers. Additional inputs: the cameras' bearing vectors of the positions (what Pinhole_Intrinsic::operator()(x) returns,
 * Camera_Pinhole.hpp:136-139: normalised Kinv (x, y, 1); 3 doubles per match, or per feature in the indexed form - computed by the
 * caller with the camera's own code) and the calibration matrices (row-major 3 x 3: 18 doubles per pair {K_I, K_J}, or 9 per image).
 * results[p].F receives m_E, results[p].precision_robust = ACRansacOut.first as the reference stores it (for this adaptor the SQUARED
 * pixel distance: ACKernelAdaptorEssential::unormalizeError returns its argument). Same parity policy as the F / H models. */
int mvgx_geofilter_e_acransac(int device, const double* xI, const double* xJ, const double* bearingI, const double* bearingJ,
                              const uint64_t* match_start, const uint32_t* image_wh, const double* K, uint64_t n_pairs,
                              const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                              mvgx_geofilter_stats* stats /* may be NULL */);
int mvgx_geofilter_e_acransac_indexed(int device, const double* feat_xy, const double* feat_bearing, const uint64_t* feat_start,
                                      const uint32_t* image_wh, const double* image_K, uint32_t n_images, const uint32_t* pairs,
                                      const uint64_t* match_start, const uint32_t* ij, uint64_t n_pairs, const mvgx_geofilter_options* opt,
                                      uint8_t* inlier_mask, mvgx_geofilter_result* results, mvgx_geofilter_stats* stats /* may be NULL */);

/* The essential matrix with the ANGULAR residual, GeometricFilter_ESphericalMatrix_AC_Angular<isUpright> (matching_image_collection/
 * E_ACRobust_Angular.hpp:33-191; main_GeometricFilter -g a and -g u, the models of spherical / upright rigs - ABI 9):
 * ACKernelAdaptor_AngularRadianError<Solver, AngularError> (robust_estimator_ACRansacKernelAdaptator.hpp:465-541) + ACRANSAC on the
 * cameras' bearing vectors alone - no pixel positions, image sizes or normalisation; log alpha0 = log10(1 / 2), multError = 1 / 4,
 * residual = the squared angle asin(x2 . normalized(E x1))^2 (multiview/solver_essential_eight_point.cpp:50-61). upright = 0:
 * EightPointRelativePoseSolver (:17-47, samples of eight, one model: the null vector of the 8 x 9 epipolar system), acceptance above
 * 2.5 x 8 inliers; upright = 1: ThreePointUprightRelativePoseSolver (multiview/solver_essential_three_point.cpp:84-113, samples of
 * three). opt->precision is the functor's precision_upper_bound in DEGREES (main_GeometricFilter passes 4.0): like the reference the
 * bound D2R(precision) is compared with the SQUARED angles as it is. results[p].F receives m_E scaled to unit Frobenius norm (the
 * reference's eigenvector; the sign is free), results[p].precision_robust = ACRansacOut.first (radians), inlier_mask / n_inliers / ok
 * describe the a-contrario result; the functor's second stage - RelativePoseFromEssential on those inliers (cheirality), E_ACRobust_
 * Angular.hpp:126-143 - is not part of this entry: mvgx_relative_pose_from_essential below runs it on the device for a batch of
 * pairs (the replacement TU keeps calling the reference's own function). Bearing vectors: 3 doubles per match, or per feature in the indexed form. */
int mvgx_geofilter_e_angular_acransac(int device, const double* bearingI, const double* bearingJ, const uint64_t* match_start, uint64_t n_pairs,
                                      int upright, const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                                      mvgx_geofilter_stats* stats /* may be NULL */);
int mvgx_geofilter_e_angular_acransac_indexed(int device, const double* feat_bearing, const uint64_t* feat_start, uint32_t n_images,
                                              const uint32_t* pairs, const uint64_t* match_start, const uint32_t* ij, uint64_t n_pairs, int upright,
                                              const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                                              mvgx_geofilter_stats* stats /* may be NULL */);
/* The ORTHOGRAPHIC essential matrix, GeometricFilter_EOMatrix_RA (matching_image_collection/Eo_Robust.hpp:35-165; main_GeometricFilter
 * -g o - ABI 9): ACKernelAdaptorEssentialOrtho<ThreePointKernel, OrthographicSymmetricEpipolarDistanceError>
 * (robust_estimator_ACRansacKernelAdaptator.hpp:384-456) + ACRANSAC with samples of three and the two closed-form models of
 * ThreePointsRelativePose per sample (multiview/solver_essential_three_point.cpp:31-79: + - x / sqrt only, evaluated in the
 * reference's order without contraction - the models are the reference's bit for bit), residual |E22 + x0 E02 + x1 E12 + y0 E20 +
 * y1 E21| (multiview/solver_essential_kernel.hpp:69-78), log alpha0 of the second image's size (point to line, scale 0.5), acceptance
 * above 2.5 x 3 inliers. xI / xJ (feat_xy in the indexed form) are the HNORMALIZED bearing vectors (b.x / b.z, b.y / b.z of what the
 * pinhole camera's operator() returns). pair_precision[p] = the bound the functor hands to ACRANSAC for pair p (Eo_Robust.hpp:96-100: the
 * mean of the two cameras' imagePlane_toCameraPlaneError(precision^2)); NULL: opt->precision for every pair. results[p].F = m_E,
 * precision_robust = ACRansacOut.first. */
int mvgx_geofilter_eo_acransac(int device, const double* xI, const double* xJ, const uint64_t* match_start, const uint32_t* image_wh,
                               const double* pair_precision, uint64_t n_pairs, const mvgx_geofilter_options* opt, uint8_t* inlier_mask,
                               mvgx_geofilter_result* results, mvgx_geofilter_stats* stats /* may be NULL */);
int mvgx_geofilter_eo_acransac_indexed(int device, const double* feat_xy, const uint64_t* feat_start, const uint32_t* image_wh, uint32_t n_images,
                                       const uint32_t* pairs, const uint64_t* match_start, const uint32_t* ij, const double* pair_precision,
                                       uint64_t n_pairs, const mvgx_geofilter_options* opt, uint8_t* inlier_mask, mvgx_geofilter_result* results,
                                       mvgx_geofilter_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------------
 * Guided matching (ABI 10): the second stage of the a-contrario geometric filters - SURVEY.md 8(f) N2's files
 *   /root/reference/src/openMVG/robust_estimation/guided_matching.hpp:178-227  GuidedMatching(model, camL, lRegions, camR, rRegions, ...)
 *   /root/reference/src/openMVG/matching_image_collection/F_ACRobust.hpp:109-152, E_ACRobust.hpp:153-215, H_ACRobust.hpp:136-180
 * For every pair (I, J) and every feature i of I: over the features j of J whose geometric error under the pair's model is below
 * error_th[pair] (kind FUNDAMENTAL: EpipolarDistanceError of F - the essential functor passes F = K2^-T E K1^-1; kind HOMOGRAPHY:
 * AsymmetricError of H), the smallest and second smallest SquaredDescriptorDistance (L2<uint8_t>, exact); (i, j_best) is a match iff a
 * second one exists and best < dist_ratio_sq * second (double arithmetic, guided_matching.hpp:68-112). Matches of a pair in ascending
 * i (what IndMatch::getDeduplicated leaves). feat_xy: the positions the reference would compare - camL->get_ud_pixel(position) or the
 * position itself - as doubles, image k owning rows [feat_start[k], feat_start[k + 1]); desc: desc_bytes (64, 128 or 144) per feature,
 * same rows. A pair whose error_th is not a positive finite number gives no match (the functors' m_dPrecision_robust != infinity
 * test). match_start: n_pairs + 1 offsets (out); *matches_ij: 2 uint32 per match (i, j), allocated by the library - release it with
 * mvgx_host_free. */
#define MVGX_GUIDED_FUNDAMENTAL 0
#define MVGX_GUIDED_HOMOGRAPHY 1
typedef struct mvgx_guided_stats {
  uint64_t n_pairs, n_matches;
  uint64_t n_geometric_tests;     /* (i, j) evaluated                                                              */
  uint64_t n_geometric_passed;    /* ... with an error below the bound: descriptor distances that counted          */
  uint64_t n_descriptor_stages;   /* wave-iterations in which the descriptor stage ran (some lane had passed)      */
  double kernel_ms;               /* device time of the norm + matching kernels (HIP events)                       */
  double total_ms;                /* the whole call incl. transfers                                                 */
} mvgx_guided_stats;
int mvgx_guided_match_u8(int device, const double* feat_xy, const uint8_t* desc, uint32_t desc_bytes, const uint64_t* feat_start, uint32_t n_images,
                         const uint32_t* pairs, const double* models /* 9 per pair, row-major */, const double* error_th /* per pair */,
                         uint64_t n_pairs, int kind, double dist_ratio_sq, uint64_t* match_start, uint32_t** matches_ij,
                         mvgx_guided_stats* stats /* may be NULL */);
/* The same for every region type the reference's functors can meet (ABI 12; Regions::SquaredDescriptorDistance is virtual,
 * guided_matching.hpp:213): desc_type MVGX_DESC_U8 = mvgx_guided_match_u8; MVGX_DESC_F32 = float rows of 64 or 128 values (desc_bytes
 * 256 / 512: AKAZE_Float_Regions, scalar_regions.hpp:107-116 + L2<float>, metric.hpp:95-131 - the reference's float sums in its order, no
 * fused multiply-add, widened to double: equal lists, not a tolerance); MVGX_DESC_BINARY = rows of 32 or 64 bytes under the SQUARED
 * Hamming distance (AKAZE_Binary_Regions, binary_regions.hpp:109-120). Everything else as above. */
#define MVGX_DESC_U8 0
#define MVGX_DESC_F32 1
#define MVGX_DESC_BINARY 2
int mvgx_guided_match(int device, const double* feat_xy, const void* desc, int desc_type, uint32_t desc_bytes, const uint64_t* feat_start,
                      uint32_t n_images, const uint32_t* pairs, const double* models, const double* error_th, uint64_t n_pairs, int kind,
                      double dist_ratio_sq, uint64_t* match_start, uint32_t** matches_ij, mvgx_guided_stats* stats /* may be NULL */);
void mvgx_host_free(void* p);   /* releases an array the library allocated for the caller (mvgx_guided_match{,_u8}) */

/* ------------------------------------------------------------------------------------------------------------------------
 * Triangulation of the tracks of a scene (no ABI bump: detect it by the symbol): the step between "tracks + poses" and the points
 * bundle adjustment starts from -
 *   sfm/sfm_data_triangulation.cpp:166-222  SfM_Data_Structure_Computation_Blind::triangulate
 *   sfm/sfm_data_triangulation.cpp:319-434  SfM_Data_Structure_Computation_Robust::robust_triangulation
 * as the global, stellar and sequential-v2 engines, structure_estimator.cpp:317 and main_ComputeStructureFromKnownPoses.cpp:287 call them.
 * Track t owns the observations [track_start[t], track_start[t + 1]) in the order of the reference's Observations map (ascending view
 * id); poses / intrinsics / intr_model have the layout of mvgx_ba_problem, all six MVGX_CAM_* models are accepted; obs_defined[o] == 0
 * marks an observation whose view has no pose or no intrinsic (IsPoseAndIntrinsicDefined, its obs_pose / obs_intr are not read).
 * MVGX_TRI_BLIND: track_triangulation (:45-101; more than two views TriangulateNViewAlgebraic, two views the inverse-depth-weighted
 * midpoint), kept iff it succeeds and every observation passes CheiralityTest. MVGX_TRI_ROBUST: 2 n iterations of UniformSample(
 * min_sample_index, n) on a fresh std::mt19937 per track, the sample triangulated (two-view samples by `method`, ETriangulationMethod
 * of multiview/triangulation_method.hpp:15-22) and checked, every observation scored, the smallest error with at least
 * min_required_inliers inliers wins (the earliest among equals); n == min_required_inliers == min_sample_index: one hypothesis from all
 * observations. min_sample_index other than 2 or 3: MVGX_ERR_UNSUPPORTED; indices out of range, a track_start that decreases:
 * MVGX_ERR_ARG. Parity: decisions and sample sequence as the reference's, points to rounding ("Triangulation"). */
#define MVGX_TRI_BLIND 0
#define MVGX_TRI_ROBUST 1
typedef struct mvgx_triangulate_options {
  int32_t mode;                     /* MVGX_TRI_*                                              */
  int32_t method;                   /* ETriangulationMethod 0..3, two-view samples (robust)    */
  double  max_reprojection_error;   /* pixels; 4.0                                             */
  uint32_t min_required_inliers;    /* 3                                                       */
  uint32_t min_sample_index;        /* 2 or 3                                                  */
} mvgx_triangulate_options;
typedef struct mvgx_triangulate_stats {
  uint64_t n_tracks, n_kept, n_inlier_obs, n_hypotheses;
  double kernel_ms, total_ms;
} mvgx_triangulate_stats;
void mvgx_triangulate_default_options(mvgx_triangulate_options*);
int mvgx_triangulate_tracks(int device,
    const double* poses /* n_poses x 6, layout of mvgx_ba_problem */, uint32_t n_poses,
    const double* intrinsics /* n_intrinsics x MVGX_BA_MAX_INTR_PARAMS */, const int32_t* intr_model, uint32_t n_intrinsics,
    const uint64_t* track_start /* n_tracks + 1 */, uint32_t n_tracks,
    const uint32_t* obs_pose, const uint32_t* obs_intr, const double* obs_xy,
    const uint8_t* obs_defined /* NULL = all; 0 = view without pose or intrinsic */,
    const mvgx_triangulate_options* opt,
    double* X /* n_tracks x 3; rejected tracks: zeros */, uint8_t* track_ok /* n_tracks */,
    uint8_t* obs_inlier /* n_obs: blind = every observation of a kept track, robust = the inlier set */,
    mvgx_triangulate_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------------
 * Robust camera resection (no ABI bump: detect it by the symbol): the step that starts every round of the sequential pipeline -
 *   sfm/pipelines/localization/SfM_Localizer.cpp:109-343   SfM_Localizer::Localize with error_max = infinity
 *   robust_estimation/robust_estimator_ACRansac.hpp:257-304, :326-489   the exhaustive NFA and the a-contrario loop
 *   multiview/solver_resection_p3p_ding.cpp, solver_resection_p3p_nordberg.cpp   the minimal solvers
 * A batch of independent problems, each run from start to end on the device. Problem p owns the correspondences [start[p], start[p + 1])
 * of x2d (2 doubles each: pixels with the distortion ALREADY removed, as sequential_SfM.cpp:925-928 passes them) and X3d (3 doubles);
 * intr_model[p] is a MVGX_CAM_* value and intrinsics + 8 p its row, laid out as in mvgx_ba_problem (spherical: {w, h}). The residual is
 * the reprojection without distortion (the spherical camera: its own projection) scaled by imagePlane_toCameraPlaneError(1).
 * Outputs per problem: out_ok = more than 2.5 * 3 inliers; then out_pose + 15 p = R | t (row-major 3 x 4) of KRt_From_P(P) followed by
 * the centre C = -R^T t, and out_P + 12 p = the winning [R | t] of the solver (row-major). out_error_max: the a-contrario threshold in
 * pixels (infinity if no model was found), out_min_nfa: the NFA reached. out_inliers: the inlier lists one after the other, the list
 * of p at [out_inlier_start[p], out_inlier_start[p + 1]), indices within the problem in the reference's order (ascending residual);
 * room for start[n_problems] - start[0] entries. A problem of three or fewer correspondences: not ok, zeros, nothing else written.
 * MVGX_ERR_UNSUPPORTED: a solver other than the two P3P ones below, a finite error_max (the quantified NFA with the max-consensus early
 * exit: mvgx_resection_localize_bounded below), an unknown camera model. MVGX_ERR_ARG: NULL arrays, a start that decreases, more than 65 536 correspondences in one problem.
 * Parity: decisions, sample sequence and inlier order as the reference's, numbers to rounding ("Resection"); a model with a
 * non-finite entry is skipped. */
#define MVGX_RESECTION_P3P_NORDBERG 3   /* resection::SolverType::P3P_NORDBERG_ECCV18 */
#define MVGX_RESECTION_P3P_DING 4       /* resection::SolverType::P3P_DING_CVPR23 (DEFAULT) */
typedef struct mvgx_resection_options {
  int32_t solver;           /* resection::SolverType 0..5; 3 and 4 have a device path                                   */
  uint32_t max_iteration;   /* 4096                                                                                      */
  double error_max;         /* infinity                                                                                  */
  uint32_t waves_ahead;     /* test hook: iterations evaluated ahead, 0 = as built, else 1 .. the build's (8)            */
  uint32_t global_above;    /* test hook: problems above this many correspondences use global scratch, 0 = as built      */
} mvgx_resection_options;
typedef struct mvgx_resection_stats {
  uint64_t n_problems, n_iterations, n_models;   /* a-contrario iterations run, models evaluated (all problems) */
  double kernel_ms, total_ms;
} mvgx_resection_stats;
void mvgx_resection_default_options(mvgx_resection_options*);
int mvgx_resection_localize(int device, uint32_t n_problems, const uint64_t* start /* n_problems + 1 */, const double* x2d, const double* X3d,
                            const int32_t* intr_model /* n_problems */, const double* intrinsics /* n_problems x MVGX_BA_MAX_INTR_PARAMS */,
                            const mvgx_resection_options* opt, uint8_t* out_ok, double* out_pose /* n_problems x 15 */,
                            double* out_P /* n_problems x 12 */, double* out_error_max, double* out_min_nfa,
                            uint64_t* out_inlier_start /* n_problems + 1 */, uint32_t* out_inliers,
                            mvgx_resection_stats* stats /* may be NULL */);
/* The bounded form (no ABI bump: detect it by the symbol): SfM_Localizer::Localize with a finite error_max, as main_SfM_Localization -r
 * and SfM_Localizer_Single_3DTrackObservation_Database::Localize call it. Arguments, options struct and outputs are those of
 * mvgx_resection_localize; opt->error_max is the bound in pixels (Image_Localizer_Match_Data::error_max on entry) and must be finite and
 * > 0 (MVGX_ERR_ARG otherwise: infinity is mvgx_resection_localize's form). ACRANSAC then (robust_estimator_ACRansac.hpp:205-256, :351-358,
 * :375, :386-389, :402-413, :446-452) reads the NFA off a 20-bin histogram of the residuals below the bound - no sort -, starts as a
 * max-consensus loop with the rejection sampler (rand_sampling.hpp:36-58), turns a-contrario at the first model with more than 2.5 * 3
 * residuals inside the bound and gives up after 2 (max_iteration / 10) + 2 iterations if there is none. out_error_max: the threshold
 * ACRANSAC found, as Localize writes it back (one of 19 steps of the bound). out_inliers: ASCENDING INDEX order in this form.
 * Besides the skipped non-finite model: an adopted sampling pool of fewer than three entries ends the problem with its current result
 * (the reference's sampler returns false there, unchecked, and a stale sample is evaluated again). */
int mvgx_resection_localize_bounded(int device, uint32_t n_problems, const uint64_t* start /* n_problems + 1 */, const double* x2d, const double* X3d,
                                    const int32_t* intr_model /* n_problems */, const double* intrinsics /* n_problems x MVGX_BA_MAX_INTR_PARAMS */,
                                    const mvgx_resection_options* opt, uint8_t* out_ok, double* out_pose /* n_problems x 15 */,
                                    double* out_P /* n_problems x 12 */, double* out_error_max, double* out_min_nfa,
                                    uint64_t* out_inlier_start /* n_problems + 1 */, uint32_t* out_inliers,
                                    mvgx_resection_stats* stats /* may be NULL */);

/* Resection of a view WITHOUT intrinsics (no ABI bump: detect it by the symbol): what SfM_Localizer::Localize runs when the sequential
 * engine passes resection::SolverType::DLT_6POINTS for a view that has no intrinsic group yet (sequential_SfM.cpp:937,
 * sequential_SfM2.cpp:400), with error_max = infinity -
 *   sfm/pipelines/localization/SfM_Localizer.cpp:134-161, :321-331   the DLT_6POINTS branch
 *   robust_estimation/robust_estimator_ACRansacKernelAdaptator.hpp:203-288   ACKernelAdaptorResection<SixPointResectionSolver, ...>
 *   multiview/solver_resection_kernel.cpp:29-136, multiview/conditioning.cpp:54-77   the solver, the normalisation by the image size
 * Batch layout, options struct, stats and inlier lists are those of mvgx_resection_localize. What differs: x2d holds the pixels AS
 * MEASURED (there is no intrinsic to undistort with), image_wh + 2 p is the view's (ui_width, ui_height), and K is an output.
 * Outputs per problem: out_ok = more than 2.5 * 6 inliers (15 are not enough, 16 are); then out_P + 12 p = the UNNORMALISED projection
 * matrix N1^-1 P (row-major 3 x 4, scaled as the solver leaves it: what resection_data.projection_matrix gets), out_pose + 15 p = R | t
 * of KRt_From_P(out_P) followed by C = -R^T t, out_K + 9 p = the K of the same decomposition (K / K(2,2), row-major; the engine seeds
 * the new intrinsic group with focal = (K(0,0) + K(1,1)) / 2 and the principal point K(0,2), K(1,2): sequential_SfM.cpp:986-987).
 * out_error_max: sqrt(errorMax) / N1(0,0) in pixels. A problem of six or fewer correspondences: not ok, zeros, nothing else written.
 * MVGX_ERR_ARG: opt->solver != MVGX_RESECTION_DLT_6POINTS (the calibrated solvers are mvgx_resection_localize's), a zero width or height
 * (or a product beyond int), NULL arrays, a start that decreases, more than 65 536 correspondences in one problem. MVGX_ERR_UNSUPPORTED: a
 * finite opt->error_max (the quantified form of the six-point loop has no device path).
 * Parity: decisions, sample sequence and inlier order as the reference's, numbers to rounding ("Resection without
 * intrinsics"). Deliberate differences: a model with a non-finite entry is skipped; a sample whose singular value iteration has not
 * converged after 30 sweeps yields no model (none does: the fixture's samples need at most 10). */
#define MVGX_RESECTION_DLT_6POINTS 0   /* resection::SolverType::DLT_6POINTS */
int mvgx_resection_localize_uncalibrated(int device, uint32_t n_problems, const uint64_t* start /* n_problems + 1 */, const double* x2d, const double* X3d,
                                         const uint32_t* image_wh /* n_problems x 2 */, const mvgx_resection_options* opt, uint8_t* out_ok,
                                         double* out_pose /* n_problems x 15 */, double* out_P /* n_problems x 12 */, double* out_K /* n_problems x 9 */,
                                         double* out_error_max, double* out_min_nfa, uint64_t* out_inlier_start /* n_problems + 1 */, uint32_t* out_inliers,
                                         mvgx_resection_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------------
 * Relative pose of image pairs (no ABI bump: detect it by the symbol): from an essential matrix to (R, t) by cheirality, and the whole
 * of sfm::robustRelativePose -
 *   multiview/essential.cpp:79-113                         MotionFromEssential: the four candidate motions of E
 *   multiview/motion_from_essential.cpp:20-95              RelativePoseFromEssential: the cheirality vote and the ratio test
 *   sfm/pipelines/sfm_robust_model_estimation.cpp:29-120   robustRelativePose, as Relative_Pose_Engine::Process (sfm/pipelines/
 *                                                          relative_pose_engine.cpp:87-223; 256 iterations, Square(2.5)), the sequential
 *                                                          engine's initial pair (sequential_SfM.cpp:396-398, :531; 4096, Square(4.0)) and
 *                                                          SfmSceneInitializerMaxPair.cpp:97-98 call it
 * A batch of independent pairs, one wave each. Pair p owns the correspondences [start[p], start[p + 1]) of the two bearing arrays (3
 * doubles each: what the camera's operator() returns).
 * Reproduced: the candidates R in {U W V^T, U W^T V^T}, t = +-u3 after the two determinant fixes; Triangulate2View(method) of every
 * listed correspondence under each candidate with the first camera at the origin; the winner = the FIRST maximum of the four counts,
 * rejected unless its count is above 0 and second / best < positive_depth_ratio in double arithmetic; the selected positions in the
 * order of the list and their points. Not reproduced: Eigen's JacobiSVD - the singular vectors come from a one-sided Jacobi iteration,
 * so R, t and the points agree to rounding, and the ORDER of the four candidates follows this build's sign choices: a sign matrix that
 * flips U and V together can turn W into W^T, which swaps candidates 0 <-> 1 and 2 <-> 3. Nothing reported for an accepted pair depends
 * on that order (a tie for the first place rejects the pair: its ratio is 1); compare `cheirality` as a sorted tuple. t is u3 itself
 * (Pose3 stores the centre and returns -(R C)); n_selected == the largest entry of cheirality, always.
 * That exchange is the only one: the signs of u2 v1^T - u1 v2^T and of u3 change together or not at all (the tests assert it).
 * The decomposition does not depend on the scale of E (any finite double, subnormals included: the iteration runs on E times a power of
 * two); the E reported is the one given. An E that is zero or has an entry that is not finite gives no pose: every count 0, ok 0.
 * A pair that is not ok: pose zeros, n_selected 0, nothing written to the lists (the reference leaves stale values, its callers drop
 * the pair). */
#define MVGX_RELPOSE_PINHOLE 0
#define MVGX_RELPOSE_ANGULAR 1
typedef struct mvgx_relative_pose_options {
  int32_t  kind;                   /* robust entry: MVGX_RELPOSE_PINHOLE (five-point, pixel epipolar error) or
                                      MVGX_RELPOSE_ANGULAR (eight-point on bearing vectors; a camera that is not a pinhole) */
  int32_t  method;                 /* ETriangulationMethod 0..3; default 3 (INVERSE_DEPTH_WEIGHTED_MIDPOINT) */
  double   positive_depth_ratio;   /* 0.7 */
  double   residual_tolerance;     /* robust entry: RelativePose_Info::initial_residual_tolerance AS THE REFERENCE TAKES IT:
                                      squared pixels (pinhole), degrees (angular). Must be finite and > 0 */
  uint32_t max_iterations;         /* robust entry: 256 (global engine), 4096 (sequential) */
} mvgx_relative_pose_options;
typedef struct mvgx_relative_pose_result {
  double   pose[15];               /* R | t row-major 3 x 4, then the centre C = -R^T t  (layout of mvgx_resection_localize) */
  double   E[9];                   /* the essential matrix used (robust entry: the a-contrario model)            */
  double   found_precision;        /* robust entry: ACRansacOut.first as robustRelativePose stores it (angular: R2D) */
  uint32_t cheirality[4];          /* points in front under each candidate, in this build's candidate order      */
  uint32_t n_acransac_inliers;     /* robust entry                                                                */
  uint32_t n_selected;             /* |vec_selected_points| of the winner                                         */
  uint32_t ok;
} mvgx_relative_pose_result;
typedef struct mvgx_relative_pose_stats {
  uint64_t n_pairs, n_pairs_ok, n_selected;
  double kernel_ms;                /* device time of the cheirality kernel (HIP events)                           */
  double acransac_kernel_ms;       /* robust entry: device time of the a-contrario stage before it                */
  double total_ms;                 /* the whole call incl. transfers                                              */
} mvgx_relative_pose_stats;
void mvgx_relative_pose_default_options(mvgx_relative_pose_options*);   /* PINHOLE, 3, 0.7, Square(2.5), 256 */
/* The cheirality stage alone: RelativePoseFromEssential on E + 9 p. use_index rows [use_start[p], use_start[p + 1]) are the positions
 * within the pair to vote with (bearing_vector_index_to_use: any order, a subset, repeats allowed); use_index == NULL (use_start is then
 * not read): all correspondences of the pair in their order - the call Relative_Pose_Engine makes with the winning pose's E to build
 * its tiny scene (relative_pose_engine.cpp:168-187). Outputs: results[p]; out_selected_start (n_pairs + 1 offsets), out_selected /
 * out_X (room for every list entry: 1 / 3 values each) = vec_selected_points / vec_points of the accepted pairs, one after the other.
 * MVGX_ERR_ARG (outputs untouched): NULL arrays, a decreasing start, an index outside its pair, positive_depth_ratio outside (0, 1], a
 * method outside 0..3. kind, residual_tolerance and max_iterations are not read. */
int mvgx_relative_pose_from_essential(int device, uint32_t n_pairs, const uint64_t* start /* n_pairs + 1 */, const double* bearingI,
                                      const double* bearingJ, const double* E /* n_pairs x 9, row-major */,
                                      const uint64_t* use_start /* n_pairs + 1, or NULL */, const uint32_t* use_index /* or NULL */,
                                      const mvgx_relative_pose_options* opt, mvgx_relative_pose_result* results,
                                      uint64_t* out_selected_start /* n_pairs + 1 */, uint32_t* out_selected, double* out_X,
                                      mvgx_relative_pose_stats* stats /* may be NULL */);
/* robustRelativePose from start to end on the device: the E a-contrario stage of the geometric filter (PINHOLE: the five-point form of
 * mvgx_geofilter_e_acransac with its inputs - pixels, bearings, image_wh, K per pair; ANGULAR: the eight-point form of
 * mvgx_geofilter_e_angular_acransac - xI, xJ, image_wh, K are not read), then the stage above on the a-contrario inliers; bearings,
 * mask and model stay on the device between the two, one download at the end. opt->residual_tolerance goes to the loop AS GIVEN
 * (robustRelativePose hands initial_residual_tolerance to ACRANSAC unchanged: squared pixels; angular: D2R of it) - the filter entries
 * take the square root of that for the pinhole model. The pair goes on to the cheirality stage unless n_acransac_inliers < 2.5 x
 * MINIMUM_SAMPLES (:70-74, :101-105): 13 of 5, 20 of 8 - the filter functor's rule is `>` and refuses 20. inlier_mask: the a-contrario
 * inliers of every pair that passed that rule (whatever the cheirality stage then decides), zeros otherwise. out_selected_start /
 * out_selected / out_X: as above, each may be NULL to skip it; positions in ASCENDING index (the reference's list is in ACRANSAC's
 * order, no caller reads that order). MVGX_ERR_UNSUPPORTED: an infinite residual_tolerance (the exhaustive-NFA form has no E path on the
 * device, and no caller of the reference passes it), more than 2^20 correspondences in a pair. MVGX_ERR_ARG as above and as the filter
 * entries'. */
int mvgx_relative_pose_robust(int device, const double* xI, const double* xJ, const double* bearingI, const double* bearingJ,
                              const uint64_t* match_start /* n_pairs + 1 */, const uint32_t* image_wh, const double* K, uint64_t n_pairs,
                              const mvgx_relative_pose_options* opt, uint8_t* inlier_mask, mvgx_relative_pose_result* results,
                              uint64_t* out_selected_start /* n_pairs + 1, or NULL */, uint32_t* out_selected /* or NULL */,
                              double* out_X /* or NULL */, mvgx_relative_pose_stats* stats /* may be NULL */);

/* ------------------------------------------------------------------------------------------------------------------------
 * Feature tracks from pairwise matches (no ABI bump: detect it by the symbol): the step between Matcher_Regions::Match + the
 * geometric filter and triangulation / resection / relative pose -
 *   tracks/tracks.hpp:62-197        tracks::TracksBuilder: Build (:70-121), Filter (:124-165), ExportToSTL (:178-196)
 *   tracks/union_find.hpp:75-103    UnionFind::Union: by rank; on equal rank the first argument's root stays root
 * as every engine calls it (sequential_SfM.cpp:273-285, sequential_SfM2.cpp:208-212: Filter() = 2; the global and stellar engines,
 * structure from known poses, translation averaging and LiGT: Filter(3)).
 * Input: the PairWiseMatches container in the layout mvgx_match_results and the `_indexed` filter entries use - `pairs` (I, J) in the
 * order of a std::map<Pair, IndMatches> (strictly ascending, I < J), pair p owns the matches [match_start[p], match_start[p + 1]) of
 * `ij` ((i, j) per match, in list order). match_mask: one byte per match, 0 drops it (a geometric filter's inlier_mask goes in as it
 * is); NULL keeps all. n_features: features per image, or NULL - then taken from the largest index a kept match uses.
 * Reproduced exactly (all outputs are integers): a node is a distinct (image, feature) of a kept match, its index its rank in ascending
 * (image, feature) order; one Union(node(I, i), node(J, j)) per kept match in container order; a track's id is the node index of its
 * final root (NOT the smallest node of the component); Filter drops whole every component in which an image occurs twice and every one
 * with fewer than min_length images; surviving tracks come out in ascending id, (image, feature) in ascending image inside a track.
 * Output, allocated by the library, each released with mvgx_host_free: track_id (n_tracks, ascending), track_start (n_tracks + 1
 * offsets: the CSR layout mvgx_triangulate_tracks takes), obs_image / obs_feature (track_start[n_tracks] each). No pairs, empty lists
 * or a mask that keeps nothing: MVGX_OK, zero tracks, track_start = {0}.
 * MVGX_ERR_ARG (nothing allocated): pairs not strictly ascending, I >= J, an image index >= n_images, a kept match with a feature
 * index >= n_features[image], a match_start that decreases, min_length < 2, NULL arrays. MVGX_ERR_UNSUPPORTED: the sum of n_features
 * (or of the spans derived) does not fit 32 bits; 2^32 - 1 or more matches. Bit-identical from run to run.
 * Memory: 8 bytes of device memory per key of the dense key space, which is the sum of n_features - or, with n_features == NULL, the sum
 * over the images of (largest used index + 1): a few large sparse indices per image are legal there but cost gigabytes (an image whose
 * largest used index is 10^9 takes 8 GB); pass n_features, or renumber the features, when the indices are sparse. About 60 bytes per node
 * and 24 per match beside that. Matches repeated inside a list are legal (a Union of one set with itself) but each copy is replayed:
 * a surviving track with k matches costs k^2 / 64 reads per lane. */
typedef struct mvgx_tracks_options {
  uint32_t min_length;             /* TracksBuilder::Filter(nLengthSupTo); default 2, the global engines pass 3 */
} mvgx_tracks_options;
typedef struct mvgx_tracks_stats {
  uint64_t n_matches_used;         /* matches the mask keeps                                                     */
  uint64_t n_nodes;                /* distinct (image, feature) among them                                       */
  uint64_t n_components;
  uint64_t n_collision;            /* components in which an image occurs twice                                  */
  uint64_t n_short;                /* components without a collision, below min_length                           */
  uint64_t n_tracks, n_obs;
  uint64_t n_sweeps;               /* iterations of the component labelling: 2 whenever a match is kept (one unites, one confirms) */
  double kernel_ms;                /* device time of all passes (HIP events; the host's waits between are not in it) */
  double total_ms;                 /* the whole call incl. transfers                                             */
} mvgx_tracks_stats;
void mvgx_tracks_default_options(mvgx_tracks_options*);   /* 2 */
int mvgx_tracks_build(int device, uint32_t n_images, const uint32_t* n_features /* n_images, or NULL */, const uint32_t* pairs /* n_pairs x 2 */,
                      const uint64_t* match_start /* n_pairs + 1 */, const uint32_t* ij, const uint8_t* match_mask /* or NULL */, uint64_t n_pairs,
                      const mvgx_tracks_options* opt, uint32_t* n_tracks, uint32_t** track_id, uint64_t** track_start, uint32_t** obs_image,
                      uint32_t** obs_feature, mvgx_tracks_stats* stats /* may be NULL */);

#ifdef __cplusplus
}
#endif
#endif /* MVGX_H_ */
