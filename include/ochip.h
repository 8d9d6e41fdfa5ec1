/* ochip.h — C ABI of libochip.so, the MI355X (gfx950) device side of the opencalibration hot path.
 *
 * The reference (jkflying/opencalibration) has no plugin/FFI layer; its seam is the stage triple
 * init/get_runners/finalize (src/pipeline/link_stage.hpp:25-30, relax_stage.hpp:24-35) over
 * value-semantic free functions.  Each entry point below replaces the inner loop of one of those
 * functions and is what a reference-side binding would call (INTEGRATION.md shows the C++ stub).
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * OCHIP_E* code and never throws; ochip_last_error() gives the text.  Pointers are HOST pointers
 * unless the name says `_dev`.  A context owns one HIP device, its streams and device arenas; calls
 * on one context must be serialised by the caller (the host stages call from one thread per context,
 * SURVEY.md §8b), different contexts are independent.
 */
#ifndef OCHIP_H
#define OCHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C"
{
#endif

#define OCHIP_OK 0
#define OCHIP_EINVAL (-1)  /* bad argument */
#define OCHIP_ENOMEM (-2)  /* device or host allocation failed */
#define OCHIP_EHIP (-3)    /* HIP runtime error, see ochip_last_error */
#define OCHIP_ENODEV (-4)  /* no usable gfx950 device */
#define OCHIP_ESTATE (-5)  /* call order violated (e.g. match before upload) */

#define OCHIP_DESC_WORDS64 8 /* std::bitset<486> = 8 x u64, bits 486..511 zero (feature_2d.hpp:9-21) */
#define OCHIP_DESC_BITS 486
#define OCHIP_NO_SECOND 0xFFFFu /* second_count sentinel: fewer than two reference descriptors */

    typedef struct ochip_ctx ochip_ctx;

    typedef struct ochip_pair
    {
        uint32_t image_1; /* query image (source node, link_stage.cpp:57) */
        uint32_t image_2; /* reference image (match_node_id, link_stage.cpp:67) */
    } ochip_pair;

    /* per query descriptor of image_1, in subset order */
    typedef struct ochip_match
    {
        uint32_t best_k;       /* position in image_2's uploaded subset of the nearest descriptor; lowest k on ties */
        uint16_t best_count;   /* Hamming distance (popcount of xor over 486 bits) */
        uint16_t second_count; /* distance of the 2nd nearest (== best_count on a tie); OCHIP_NO_SECOND if n2 < 2 */
    } ochip_match;

    /* kernel ids for ochip_profile_get */
    enum
    {
        OCHIP_K_MATCH = 0,
        OCHIP_K_RANSAC = 1,
        OCHIP_K_RELAX_EVAL = 2,
        OCHIP_K_RELAX_SOLVE = 3,
        OCHIP_K_AKAZE = 4,
        OCHIP_K_DENSE = 5,
        OCHIP_K_COUNT = 8
    };

    /* ---- context ------------------------------------------------------------------------------ */
    int ochip_ctx_create(int device, ochip_ctx **out);
    void ochip_ctx_destroy(ochip_ctx *ctx);
    /* The index-th sibling of ctx: another context on the same device with its own streams, scratch buffers and
     * pools, created on first use and destroyed with ctx.  Lets independent batches (e.g. the link stage's runners,
     * src/pipeline/link_stage.cpp:41-117) be in flight at once: one host thread per context.  Kernel times of
     * siblings are included in ochip_profile_get(ctx, ...). */
    int ochip_ctx_sibling(ochip_ctx *ctx, uint32_t index, ochip_ctx **out);
    /* One object that a caller keeps with ctx for the context's life (the host library's extraction slots): made with
     * make() on the first call - calls from several threads get the same object - and handed to destroy() by
     * ochip_ctx_destroy before anything of the context is freed. */
    /* How many chunks of ochip_akaze_* on ctx have passed their first host read-back (the candidate counts: the scale space
     * and the detector are then behind the sequence).  May be read from another thread while a chunk runs. */
    uint64_t ochip_akaze_progress(const ochip_ctx *ctx);
    void *ochip_ctx_attachment(ochip_ctx *ctx, void *(*make)(void), void (*destroy)(void *));
    /* Re-creates the context's compute stream with the highest (high != 0) or lowest stream priority of the device: a
     * latency-bound solve that shares the GPU with throughput kernels of other contexts is scheduled ahead of them.  The
     * context must be idle. */
    int ochip_ctx_set_priority(ochip_ctx *ctx, int high);
    const char *ochip_last_error(const ochip_ctx *ctx); /* ctx may be NULL: error of the last failed create */
    int ochip_device_info(const ochip_ctx *ctx, char *name, size_t name_len, int *compute_units, size_t *hbm_bytes);
    int ochip_synchronize(ochip_ctx *ctx);

    /* ---- descriptor store (replaces the packed_2 build, src/match/match_features.cpp:62-66) ----- */
    /* Size the arena once: n_images slots, total_descriptors descriptors over all images. */
    int ochip_descriptors_reserve(ochip_ctx *ctx, uint32_t n_images, uint64_t total_descriptors);
    /* Copy one image's 40-px-subset descriptors (subset order, n x 8 u64) into HBM.  The caller keeps
     * ownership of `desc`.  An image may be uploaded once. */
    int ochip_upload_descriptors(ochip_ctx *ctx, uint32_t image_id, const uint64_t *desc, uint32_t n);
    int ochip_descriptor_count(const ochip_ctx *ctx, uint32_t image_id, uint32_t *n);

    /* ---- brute-force Hamming 2-NN (replaces the double loop src/match/match_features.cpp:71-93) - */
    /* For pair p, out[out_offset[p] + i] describes query i of image_1 (i < n(image_1)).
     * out_offset has n_pairs entries; the caller sizes `out` as sum of n(image_1).  The Lowe ratio
     * test (:94), the index remap through indices_2 (:86) and the std::sort (:100-101) stay on the
     * host so libstdc++'s tie order is preserved. */
    int ochip_match_batch(ochip_ctx *ctx, const ochip_pair *pairs, uint32_t n_pairs, const uint64_t *out_offset,
                          ochip_match *out);
    /* The tail of match_features_subset (match_features.cpp:94-101) on the device, on the records ochip_match_launch left
     * in HBM (same pairs, offsets and total): Lowe's ratio test (best < 0.8 * second on count / 486 as doubles) and the
     * std::sort by descending distance - libstdc++'s permutation among equal distances, csrc/std_sort.hip.  The sorted
     * matches stay in HBM for ochip_ransac_homography_batch_sorted; counts_out[p] = matches of pair p; fallback_out[p] != 0:
     * the pair's sort needs libstdc++'s heap sort (not restated on the device) - the caller then takes the host route
     * (ochip_match_fetch, host ratio test and sort, ochip_ransac_homography_batch) for the batch. */
    int ochip_match_sort(ochip_ctx *ctx, const ochip_pair *pairs, uint32_t n_pairs, const uint64_t *out_offset, uint64_t out_total,
                         uint32_t *counts_out, uint8_t *fallback_out);
    /* Asynchronous flavour: results stay in HBM until ochip_match_fetch (lets the caller overlap). */
    int ochip_match_launch(ochip_ctx *ctx, const ochip_pair *pairs, uint32_t n_pairs, const uint64_t *out_offset,
                           uint64_t out_total);
    int ochip_match_fetch(ochip_ctx *ctx, ochip_match *out, uint64_t out_total);

    /* ---- extract: AKAZE keypoints + 486-bit M-LDB descriptors for a batch of equally sized BGR images
     *      (replaces cvtColor + resize(INTER_AREA, max side 1600) + cv::AKAZE::detectAndCompute of
     *      src/extract/extract_features.cpp:25-36; AKAZE restated from its publication) ---- */
    /* images_bgr: n_images x height x width x 3 bytes.  Per image up to max_kp keypoints are written, in
     * cv::AKAZE's detection order (evolution level, then row, then column of the extremum - the order the
     * unstable std::sort of extract_features.cpp:55-56 starts from, which decides the result when responses tie):
     * kp6[(i*max_kp + k)*6] = {x, y, diameter, angle (radians), response, evolution level}
     * in pixels of the working (downscaled) image, desc[(i*max_kp + k)*8] = descriptor words (bit j = word j>>6,
     * bit j&63, the packing of extract_features.cpp:47-51); counts[i] = keypoints of image i;
     * work_wh = working width, height. */
    int ochip_akaze_batch(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                          uint32_t max_kp, float *kp6, uint64_t *desc, uint32_t *counts, int *work_wh);

    /* Same with the images already resident in HBM (device pointer): the PCIe upload is outside the call. */
    int ochip_akaze_batch_dev(ochip_ctx *ctx, const uint8_t *images_bgr_dev, uint32_t n_images, int width, int height,
                              uint32_t max_kp, float *kp6, uint64_t *desc, uint32_t *counts, int *work_wh);

    /* Test seam: the working image alone - what ochip_akaze_batch computes in front of AKAZE (BGR -> grey with cvtColor's
     * fixed-point weights, cv::resize(INTER_AREA) to a long side of 1600, (float)u8 * (1 / 255f)) through the same function
     * as the product, and nothing after it.  images_bgr: host, or device when on_device (any alignment); out: n_images x
     * work_wh[1] x work_wh[0] floats (host); any image size, also ones AKAZE has no levels for.  *route names the kernels
     * that ran: OCHIP_WI_RESIZE_* | OCHIP_WI_GREY_* << 8. */
#define OCHIP_WI_RESIZE_NONE 0        /* no side above 1600: to_float_kernel */
#define OCHIP_WI_RESIZE_FUSED4 1      /* resize_area_lds_kernel<true, 4>: BGR -> LDS -> area, at most 4 horizontal taps */
#define OCHIP_WI_RESIZE_FUSED8 2      /* resize_area_lds_kernel<true, 8> */
#define OCHIP_WI_RESIZE_STAGED_GREY 3 /* resize_area_lds_kernel<false, 8> over the grey image */
#define OCHIP_WI_RESIZE_PER_TAP 4     /* resize_area_kernel over the grey image */
#define OCHIP_WI_GREY_FUSED 0         /* inside the resize */
#define OCHIP_WI_GREY_GRAY4 1         /* gray4_kernel */
#define OCHIP_WI_GREY_GRAY4_TAIL 2    /* gray4_kernel and gray_kernel on the last pixels, fewer than 4 */
#define OCHIP_WI_GREY_BYTEWISE 3      /* gray_kernel on everything (a source that is not 4-byte aligned) */
    int ochip_debug_working_image(ochip_ctx *ctx, const uint8_t *images_bgr, int on_device, uint32_t n_images, int width,
                                  int height, float *out, int *work_wh, int *route);

    /* ---- extract_features' tail (src/extract/extract_features.cpp:38-87) on the device ---- */
    /* The reference rescales the keypoints, std::sorts them by response (unstable: libstdc++'s order among equal
     * responses, restated move for move on the device, csrc/std_sort.hip), runs a greedy 8 px suppression in that order
     * and emits [sparse..., dense...].  All arrays are the caller's (host; page-locked ones copy at link speed):
     *   records    [n][max_kp + 1][88]  the image's output list [sparse..., dense...] as feature_2d records (location =
     *                                   pt / scale as doubles, strength, 4 bytes padding, 8 descriptor words):
     *                                   counts[i] + 1 records (the strongest feature heads both lists: the reference
     *                                   visits its seed again, :60-66)
     *   response   [n][max_kp]          responses in detection order
     *   slot       [n][max_kp]          slot[s] = where the keypoint of detection index s lies in `records` (the seed:
     *                                   its sparse slot, 0)
     *   num_sparse [n]                  length of the sparse list
     *   conflict   [n]                  non-zero: this image's responses drive introsort to its depth limit, where
     *                                   libstdc++ switches to a heap sort the device does not restate; `records` then
     *                                   holds the features in no particular order and the host orders and suppresses
     *                                   them itself (host/extract_features.cpp: extract_tail_prepared), using `response`
     *                                   and `slot`.  Never seen on detector output; organ-pipe responses do it. */
    /* Optionally also spatially_subsample_feature_indices(features, subset_spacing, num_sparse)
     * (src/match/match_features.cpp:8-52: the sparse features' indices std::sorted by strength, then accepted greedily when
     * no accepted feature lies within the spacing) - what LinkStage computes per image before matching (link_stage.cpp:63-65
     * with 40 px):
     *   subset          [n][OCHIP_SUBSET_CAP]  accepted indices into the feature list, in the function's output order
     *   num_subset      [n]                    their number (> OCHIP_SUBSET_CAP: row truncated, the host computes it)
     *   subset_conflict [n]                    non-zero: this sort hit the depth limit, the host computes the subset
     * Leave subset NULL (or subset_spacing 0) to skip it. */
#define OCHIP_SUBSET_CAP 16384
    typedef struct ochip_feature_lists
    {
        uint8_t *records;
        float *response;
        uint32_t *slot;
        uint32_t *num_sparse;
        uint8_t *conflict;
        uint32_t *subset;
        uint32_t *num_subset;
        uint8_t *subset_conflict;
        double subset_spacing;
    } ochip_feature_lists;
    /* ochip_akaze_batch / _dev with the tail prepared: counts as there, `lists` instead of kp6 / desc.
     * scale = working / original size (the reference's `scale`, :26), nms_radius in working pixels (8, :58). */
    int ochip_akaze_features(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height, uint32_t max_kp,
                             double nms_radius, uint32_t *counts, const ochip_feature_lists *lists, int *work_wh);
    int ochip_akaze_features_dev(ochip_ctx *ctx, const uint8_t *images_bgr_dev, uint32_t n_images, int width, int height,
                                 uint32_t max_kp, double nms_radius, uint32_t *counts, const ochip_feature_lists *lists, int *work_wh);
    /* the same preparation for keypoints the caller already has (kp6 / desc / counts as ochip_akaze_batch returns them) */
    int ochip_feature_lists_from_keypoints(ochip_ctx *ctx, const float *kp6, const uint64_t *desc, const uint32_t *counts, uint32_t n_images,
                            uint32_t max_kp, int work_w, int work_h, double scale, double nms_radius,
                            const ochip_feature_lists *out);

    /* ---- synthetic views: benchmark / test DATA generated directly in HBM (no algorithm of the path) ---- */
    /* A jittered ground lattice of Gaussian blobs on the plane z = a x + b y rendered through pinhole cameras;
     * all views of one seed show the same ground.  cams: n x {pos3, quat4 (x y z w)}; model3 = {f, ppx, ppy};
     * plane2 = {a, b}; lattice3 = {x0, y0, spacing}.  Images are BGR (grey replicated), n x height x width x 3. */
    int ochip_synth_views_alloc(ochip_ctx *ctx, uint32_t n_images, int width, int height, uint8_t **images_dev);
    void ochip_synth_views_free(ochip_ctx *ctx, uint8_t *images_dev);
    int ochip_synth_views_read(ochip_ctx *ctx, const uint8_t *images_dev, uint32_t index, int width, int height,
                               uint8_t *host_out); /* copy view `index` back to the host (for the CPU checker) */
    int ochip_synth_render_views(ochip_ctx *ctx, uint8_t *images_dev, uint32_t first_image, uint32_t n_images, int width,
                                 int height, const double *cams, const double *model3, const double *plane2,
                                 const double *lattice3, uint32_t seed);

    /* ---- keypoints -> unit rays (replaces image_to_3d of src/distort/distort_keypoints.cpp:68-103,
     *      hoisted from once per match to once per keypoint) ------------------------------------------ */
    /* xy: n x 2 pixel locations in the same subset order as the descriptors of image_id (n must equal
     * the uploaded descriptor count).  model8 = {focal_length_pixels, pp_x, pp_y, k1, k2, k3, p1, p2}
     * (DifferentiableCameraModel, include/opencalibration/types/camera_model.hpp:22-60). */
    int ochip_upload_keypoints(ochip_ctx *ctx, uint32_t image_id, const double *xy, uint32_t n, const double *model8);

    /* One-call flavour of reserve + upload_descriptors + upload_keypoints for a whole batch: image i owns
     * counts[i] consecutive rows of desc_all (x 8 u64) and xy_all (x 2 f64); models8 is n_images x 8. */
    int ochip_upload_batch(ochip_ctx *ctx, uint32_t n_images, const uint32_t *counts, const uint64_t *desc_all,
                           const double *xy_all, const double *models8);

    /* Page-locked host memory for the large transfers (match results, RANSAC inputs): PCIe copies from
     * pageable memory run at a fraction of the link rate. */
    int ochip_host_alloc(ochip_ctx *ctx, size_t bytes, void **out);
    void ochip_host_free(ochip_ctx *ctx, void *p);

    /* ---- homography RANSAC, one job per directed pair (replaces ransac<homography_model>,
     *      src/model_inliers/ransac.cpp:53-257 + homography_model.cpp:19-136) -------------------------- */
    typedef struct ochip_ransac_match
    {
        uint32_t k1, k2;   /* positions of the matched keypoints in the uploaded subsets of image_1 / image_2 */
        uint16_t count;    /* Hamming distance; correspondence.quality = count * (1.0/486) */
        uint16_t reserved; /* 0 */
    } ochip_ransac_match;

    typedef struct ochip_ransac_job
    {
        uint32_t image_1, image_2;
        uint32_t n;            /* number of matches = correspondences, in match_features_subset's output order */
        uint32_t rng_state;    /* std::default_random_engine(42) state after std::shuffle(eval_order) */
        uint64_t match_offset; /* into matches[], sorted_idx[] and inliers[] */
        uint64_t eval_offset;  /* into eval_order[]: iota(n) after std::shuffle (ransac.cpp:158) */
    } ochip_ransac_job;

    typedef struct ochip_ransac_result
    {
        double H[9];           /* row-major homography (model.homography), NaN if nothing was fitted */
        double score;          /* return value of ransac(): evaluate(best) / n */
        uint32_t iterations;   /* loop trips executed */
        uint32_t n_inliers;
        uint32_t improvements; /* times a hypothesis beat the best score */
        uint32_t reserved;
    } ochip_ransac_result;

    /* sorted_idx: per job, iota(n) std::sort-ed by quality ascending (the PROSAC order, ransac.cpp:83-90);
     * both it and eval_order come from the host's libstdc++ so tie order is the reference's.
     * inliers: total_matches bytes, 1 = inlier, indexed like matches[]. */
    int ochip_ransac_homography_batch(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs,
                                      const ochip_ransac_match *matches, const uint32_t *sorted_idx,
                                      uint64_t total_matches, const uint32_t *eval_order, uint64_t eval_total,
                                      double inlier_threshold, ochip_ransac_result *results, uint8_t *inliers);

    /* ---- the fundamental- and essential-matrix models under the same RANSAC loop (replaces
     *      ransac<fundamental_matrix_model> / ransac<essential_matrix_model>, src/model_inliers/ransac.cpp:260-261 over
     *      fundamental_matrix_model.cpp:12-217 (8-point fit, rank-2 constraint, Sampson error, DEGENSAC) and
     *      essential_matrix_model.cpp:12-123 (5-point linear fit, equal singular values); tests-only in the reference).
     *      model: 0 = fundamental (threshold 0.01), 1 = essential.  corr6: per correspondence {measurement1,
     *      measurement2} (any scale: both are divided by their z); sorted_idx / eval_order as for the homography batch
     *      (sorted_idx is read only by jobs with has_quality != 0).  results[j].H = the matrix, .score = evaluate / n. */
    typedef struct ochip_epipolar_job
    {
        uint32_t n;           /* correspondences */
        uint32_t rng_state;   /* std::default_random_engine(42) state after std::shuffle(eval_order) */
        uint32_t has_quality; /* any correspondence.quality != 0: PROSAC sampling over sorted_idx */
        uint32_t reserved;
        uint64_t corr_offset; /* into corr6 (x 6), sorted_idx and inliers */
        uint64_t eval_offset; /* into eval_order */
    } ochip_epipolar_job;
    int ochip_ransac_epipolar_batch(ochip_ctx *ctx, int model, const ochip_epipolar_job *jobs, uint32_t n_jobs,
                                    const double *corr6, const uint32_t *sorted_idx, uint64_t total,
                                    const uint32_t *eval_order, uint64_t eval_total, double inlier_threshold,
                                    ochip_ransac_result *results, uint8_t *inliers);

    /* ---- re-fit of accepted edges after the camera models changed (replaces the per-edge loop of
     *      RelaxGroup::finalize, src/relax/relax_group.cpp:137-177: distort_keypoints with the current models, then
     *      `rounds` (= 3 there) times fitInliers + evaluate starting from the previous inliers).  jobs / matches as for
     *      ochip_ransac_homography_batch (rng_state and eval_offset unused); the keypoints and the CURRENT models must
     *      have been uploaded (ochip_upload_keypoints / ochip_upload_batch).  inliers: in = the previous inlier flags,
     *      out = the flags of the last evaluate; results[j].H = the last fit, .n_inliers, .score = evaluate / n. */
    /* homography_model::decompose (homography_model.cpp:138-185) of a job's result: the four poses of
     * cv::decomposeHomographyMat(H, I) as {orientation x y z w, position x y z, score = cheirality votes of the inliers} in
     * std::stable_sort's order (absent solutions: NaN, score -1), can_decompose = decompose()'s return value, n_inliers =
     * number of inlier flags set. */
    typedef struct ochip_decomposition
    {
        double pose[4][8];
        uint32_t can_decompose, n_inliers;
    } ochip_decomposition;
    /* The same on the matches ochip_match_sort left in HBM (decomp_out: NULL or one ochip_decomposition per job): jobs[j] is pair j of that call with n = counts_out[j]; the
     * correspondences (their order is the sort's), the PROSAC order (ransac.cpp:83-90, the same device std::sort) are built
     * on the device.  matches_out[match_offset + i] = correspondence i of the job (for the host's feature_match list);
     * fallback_out[j] != 0: the PROSAC order of job j needs the host (then nothing of this call is to be used). */
    int ochip_ransac_homography_batch_sorted(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, uint64_t total_matches,
                                             const uint32_t *eval_order, uint64_t eval_total, double inlier_threshold,
                                             ochip_ransac_result *results, uint8_t *inliers, ochip_ransac_match *matches_out,
                                             uint8_t *fallback_out, ochip_decomposition *decomp_out);
    /* The two lists an accepted edge keeps (camera_relations.matches / .inlier_matches, link_stage.cpp:99-107), gathered on
     * the device right after ochip_ransac_homography_batch_sorted (same context, same batch):
     *   feature_match_out  [total_matches] x {u64 feature_index_1, u64 feature_index_2, f64 distance}  (types/feature_match.hpp:
     *                      feature_match, 24 bytes), job j's matches at its match_offset, in the sort's order
     *   inlier_match_out   [total_inliers] x {f64 pixel_1[2], pixel_2[2], u64 feature_index_1, feature_index_2, match_index}
     *                      (feature_match_denormalized, 56 bytes): job j's inliers in match order at inlier_offset[j] (the
     *                      caller sums ochip_decomposition.n_inliers)
     * feature_index[k]: index in its image's feature list of the k-th keypoint of the upload (ochip_upload_batch order) -
     * the 40 px subset's indices. */
    int ochip_edge_lists(ochip_ctx *ctx, uint32_t n_jobs, uint64_t total_matches, const uint32_t *feature_index, uint64_t n_keypoints,
                         const uint64_t *inlier_offset, uint64_t total_inliers, void *feature_match_out, void *inlier_match_out);
    int ochip_refit_homography_batch(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs,
                                     const ochip_ransac_match *matches, uint64_t total_matches, uint32_t rounds,
                                     double inlier_threshold, ochip_ransac_result *results, uint8_t *inliers);

    /* Test seam: homography_model::fit (homography_model.cpp:19-50) of n minimal samples through the two device routes that
     * have no entry of their own.  xy16: per sample four correspondences x {x, y, x', y'}, already divided by z.  route 0: one
     * wavefront per sample through the wave-cooperative 9 x 9 factorisation (what the RANSAC loop's normal path runs); route 1:
     * the fast-forward's lane-private fit, 32 samples per wavefront in its LDS layout.  H9 / Hinv9: n x 9 row-major;
     * degenerate[s] = checkSampleDegeneracy of sample s (the fit runs either way). */
    int ochip_debug_homography_fit4(ochip_ctx *ctx, int route, const double *xy16, uint32_t n, double *H9, double *Hinv9,
                                    uint8_t *degenerate);

    /* Test seam: decompose_vote_kernel, launched as ochip_ransac_homography_batch_sorted launches it, on homographies the
     * caller gives instead of the RANSAC kernel's results.  jobs / matches / inliers as for ochip_ransac_homography_batch
     * (rng_state and eval_offset unused); H9: n_jobs x 9 row-major; the rays are the device's image_to_3d of the uploaded
     * keypoints and models (ochip_upload_keypoints / ochip_upload_batch).  decomp_out: one ochip_decomposition per job.
     * Refuses NULL arguments, jobs whose images, offsets or keypoint indices exceed the upload.  Leaves the RANSAC scratch
     * (what ochip_edge_lists reads) alone. */
    int ochip_debug_decompose_votes(ochip_ctx *ctx, const ochip_ransac_job *jobs, uint32_t n_jobs, const ochip_ransac_match *matches,
                                    uint64_t total_matches, const double *H9, const uint8_t *inliers, ochip_decomposition *decomp_out);

    /* ---- relax: ground-plane bundle adjustment (replaces ceres::Solver::Solve on the problem
     *      RelaxProblem::setupGroundPlaneProblem builds, src/relax/relax_problem.cpp:61-81,1390-1420) ---- */
    typedef struct ochip_relax_problem ochip_relax_problem;

    typedef struct ochip_relax_desc
    {
        uint32_t n_cams;
        const double *cam_pos;       /* n_cams x 3, constants (GPS positions are never optimised) */
        const double *cam_q;         /* n_cams x 4 initial orientation, Eigen coefficient order x y z w */
        const uint8_t *cam_optimize; /* n_cams: 1 = in _nodes_to_optimize, 0 = constant context camera */
        double plane_xy[6];          /* the three plane corners' x,y (initializeGroundPlane, :1189-1242) */
        double plane_z[3];           /* initial corner heights (the structure parameters) */
        uint8_t z_optimize[3];
        uint32_t n_blocks;           /* 2-ray PlaneIntersectionAngleCost blocks (relax_cost_function.hpp:658-684) */
        const uint32_t *blk_cam_a;   /* n_blocks: source camera */
        const uint32_t *blk_cam_b;   /* n_blocks: dest camera */
        const double *blk_rays;      /* n_blocks x 6: camera-frame unit rays of the source and dest keypoint */
        uint32_t n_prior;            /* PointsDownwardsPrior blocks (relax_cost_function.hpp:21-49) */
        const uint32_t *prior_cam;
        double huber_a;              /* HuberLoss scale of the 2-ray blocks (1 degree in radians, :68) */
        double prior_weight;         /* 1e-3 (:1297) */
    } ochip_relax_desc;

    typedef struct ochip_relax_options /* the ceres::Solver::Options fields the reference sets or relies on */
    {
        int max_num_iterations;             /* 100 (:32) */
        double initial_trust_region_radius; /* 1 (:36) */
        double function_tolerance;          /* 1e-6 */
        double gradient_tolerance;          /* 1e-10 */
        double parameter_tolerance;         /* 1e-8 */
    } ochip_relax_options;

    enum
    {
        OCHIP_RELAX_NO_PARAMETERS = 0,
        OCHIP_RELAX_CONVERGENCE_GRADIENT = 1,
        OCHIP_RELAX_CONVERGENCE_PARAMETER = 2,
        OCHIP_RELAX_CONVERGENCE_FUNCTION = 3,
        OCHIP_RELAX_CONVERGENCE_RADIUS = 4,
        OCHIP_RELAX_NO_CONVERGENCE = 5,
        OCHIP_RELAX_FAILURE = 6
    };

    typedef struct ochip_relax_summary
    {
        int termination;
        int iterations; /* summary.iterations.size(): iteration 0 + every trust-region step attempted */
        int successful_steps, unsuccessful_steps;
        int num_parameters; /* tangent dimension of the reduced program */
        int num_residual_blocks;
        double initial_cost, final_cost;
    } ochip_relax_summary;

    /* ---- set-up of the ground-plane relax: gridFilterMatchesPerImage + the residual-block list -------------------
     * Replaces, for the edges of one RelaxProblem::setupGroundPlaneProblem, src/relax/relax_problem.cpp:234-309 (score every
     * inlier match, keep the best one per cell of each image's grid: GridFilter::addMeasurement,
     * include/opencalibration/relax/grid_filter.hpp:33-51) and :388-560 with fixed intrinsics (a kept match whose rays'
     * closest approach lies over the plane's border triangle becomes a residual block), one wavefront per edge. */
    typedef struct ochip_plane_edge
    {
        uint32_t cam_a, cam_b;     /* rows of cam_pos / cam_q: the source and the destination image's pose */
        uint32_t model_a, model_b; /* rows of models10 */
        uint32_t n_inliers;
        uint32_t flags;            /* bit 0: relationType == HOMOGRAPHY (H scores the match, :279-287) */
        uint64_t inlier_offset;    /* first record of the edge in `inliers` */
        double H[9];               /* camera_relations::ransac_relation, row-major */
    } ochip_plane_edge;
    typedef struct ochip_plane_inlier
    {
        double px1[2], px2[2];   /* feature_match_denormalized::pixel_1 / pixel_2 */
        double descriptor_score; /* 1 - matches[match_index].distance (1 if the index is out of range), :273-275 */
    } ochip_plane_inlier;
    typedef struct ochip_plane_setup ochip_plane_setup;
    /* Scores and filters.  cam_pos [n_cams][3], cam_q [n_cams][4] (x, y, z, w); models10 [n_models][10] = f, ppx, ppy,
     * k1, k2, k3, p1, p2, pixels_cols, pixels_rows; triangle_xy6 = the border triangle's corners in the searcher's order
     * (after its orientation fix-up, src/surface/intersect.cpp:56-163); grid_fraction = 0.15 (:66).
     * keep_out[i] (n_inliers bytes): bit 0 = match i is on the source image's whitelist, bit 1 = on the destination's.
     * inexact_out[e] != 0 (n_edges bytes): two matches of edge e share the best score of a cell (the reference's unstable
     * std::sort decides, grid_filter.hpp:33-51) or a match lies outside the cell table - the caller computes that edge's
     * flags itself and passes them to ochip_plane_setup_override.  The handle holds device blocks of `ctx`. */
    int ochip_plane_setup_create(ochip_ctx *ctx, const ochip_plane_edge *edges, uint32_t n_edges, const ochip_plane_inlier *inliers,
                                 uint64_t n_inliers, const double *cam_pos, const double *cam_q, uint32_t n_cams,
                                 const double *models10, uint32_t n_models, const double *triangle_xy6, double grid_fraction,
                                 uint8_t *keep_out, uint8_t *inexact_out, ochip_plane_setup **out);
    int ochip_plane_setup_override(ochip_plane_setup *s, uint64_t first_inlier, uint64_t n, const uint8_t *keep);
    /* The residual blocks in edge order, matches in index order: cameras (rows of cam_pos) and the two camera-frame unit
     * rays (6 doubles) of each - the arrays ochip_relax_desc takes.  All three arrays NULL: only *n_blocks is returned; it
     * is set even when capacity is too small (OCHIP_ENOMEM). */
    int ochip_plane_setup_blocks(ochip_plane_setup *s, uint32_t *blk_cam_a, uint32_t *blk_cam_b, double *blk_rays, uint64_t capacity,
                                 uint64_t *n_blocks);
    void ochip_plane_setup_destroy(ochip_plane_setup *s);

    /* ---- the NaN bootstrap of runGroundPlane as one resident launch (csrc/relax_chain.hip) -------------------------
     * Replaces the loop of src/relax/relax.cpp:52-80: every camera of a batch that arrives without an orientation takes
     * the orientation of the pose in front of it and is relaxed - setupGroundPlaneProblem, relaxObservedModelOnly, solve -
     * before the next one.  The group's cameras, edges (in edges_to_optimize's order) and inlier matches are uploaded
     * once; ochip_plane_chain_run walks the steps on the device without a host round trip in between.
     * A step: `cam` takes the current orientation of `prev_cam` (prev_cam < 0: prev_q), the plane is the triangle tri_xy
     * (corners in the mesh searcher's order, initializeGroundPlane :1189-1242) at height z0, the edges [0, n_filter) take
     * part (gridFilterMatchesPerImage stops at the first edge without usable poses, :251-252).  mode 0: `cam` alone is
     * optimised, every other camera is constant (relax.cpp:61-68: the caller puts the first edge that touches a camera
     * without an orientation in the graph at n_filter); mode 1: every camera with cam_optimize set (relax.cpp:70-75);
     * mode 2: the group's own solve behind the loop (relax.cpp:81-84): as mode 1, but nobody takes an orientation (cam, prev_*
     * unused). */
    typedef struct ochip_plane_chain_step
    {
        uint32_t cam, mode, n_filter;
        int32_t prev_cam;
        double prev_q[4];
        double tri_xy[6];
        double z0;
    } ochip_plane_chain_step;
    typedef struct ochip_plane_chain_result
    {
        uint32_t steps_done; /* the steps before this one are finished and in cam_q_out */
        int32_t status;      /* 0: every step done; 1: step `steps_done` needs the host's grid filter (a tie for a cell's best
                                score, a match outside the cell table); 2: given up (a wait on the device ran into its limit).
                                The caller continues from that step with its own loop. */
        int32_t solves, iterations_total, last_iterations, last_residual_blocks; /* as ochip_relax_summary counts them */
        double last_initial_cost, last_final_cost;
        int32_t grid_syncs, workgroups;
        double plane_z[3];   /* the last step's corner heights, in tri_xy's order */
    } ochip_plane_chain_result;
    typedef struct ochip_plane_chain ochip_plane_chain;
    /* cam_pos [n_cams][3], cam_q [n_cams][4] (NaN: not oriented yet), cam_optimize [n_cams] (mode 1), models10 as for
     * ochip_plane_setup_create; huber_a, prior_weight as in ochip_relax_desc.  Fails with OCHIP_EINVAL for what the chain
     * does not take (more than 340 optimised cameras, a grid finer than 1 / 15, an edge from a camera to itself). */
    int ochip_plane_chain_create(ochip_ctx *ctx, const ochip_plane_edge *edges, uint32_t n_edges, const ochip_plane_inlier *inliers,
                                 uint64_t n_inliers, const double *cam_pos, const double *cam_q, const uint8_t *cam_optimize,
                                 uint32_t n_cams, const double *models10, uint32_t n_models, double grid_fraction, double huber_a,
                                 double prior_weight, const ochip_plane_chain_step *steps, uint32_t n_steps, ochip_plane_chain **out);
    /* stepped != 0: one phase per launch (the test route; same code, same numbers).  cam_q_out [n_cams][4]: the state after
     * the last finished step, normalised as RelaxProblem::solve leaves it (:1410-1413). */
    int ochip_plane_chain_run(ochip_plane_chain *chain, int stepped, double *cam_q_out, ochip_plane_chain_result *result);
    /* The test seam of the chain: runs it as ochip_plane_chain_run does (the same numbers, from an instantiation of the
     * kernel the product never launches) and records what its serial part computed as events of 8-byte words: a header
     * (kind, words including the header, index, step) and the payload of the kind - 1: a step's set-up (counts, the state,
     * blk_cnt, inexact, cam_prior, cam_blocks, the block lists, the keep flags), 2: a finished evaluation (the state, cam_t,
     * cost, fail bits, J'r, the clamped diagonal, J'J's lower triangle), 3: a linear solve and its candidate (radius, scale,
     * damping, scaled gradient, the step, the model's cost change; above 12 unknowns also the factor with its augmented
     * row and the inverses of its diagonal tiles), 4: a finished solve (termination, iterations, costs).  The layouts are
     * the ones opencalibration_amd/capi.py parses.  Events [first_event, first_event + max_events) are written into
     * events[capacity] as long as they fit; every event is counted: *n_events, and *n_words of the buffer are filled.
     * capacity 0 (events may be NULL) only counts.  rays_out: NULL or [n_inliers][6], the camera-frame rays of every
     * inlier match.  OCHIP_EINVAL, and nothing launched, for a NULL chain, cam_q_out, result, n_events or n_words. */
    int ochip_plane_chain_trace(ochip_plane_chain *chain, int stepped, uint64_t first_event, uint64_t max_events, double *events,
                                uint64_t capacity, uint64_t *n_events, uint64_t *n_words, double *rays_out, double *cam_q_out,
                                ochip_plane_chain_result *result);
    void ochip_plane_chain_destroy(ochip_plane_chain *chain);

    /* A problem (this one and the ochip_relaxg_ / ochip_relaxp_ ones below) holds device blocks and a page-locked host
       block of its context: destroy it before the context. */
    int ochip_relax_problem_create(ochip_ctx *ctx, const ochip_relax_desc *desc, ochip_relax_problem **out);
    void ochip_relax_problem_destroy(ochip_relax_problem *p);
    /* relaxObservedModelOnly (:931-984): freeze every camera, leave the plane heights variable (or undo) */
    int ochip_relax_set_cameras_constant(ochip_relax_problem *p, int constant);
    /* Levenberg-Marquardt trust-region solve; the state stays in HBM */
    int ochip_relax_solve(ochip_relax_problem *p, const ochip_relax_options *opt, ochip_relax_summary *summary);
    /* Sharded evaluation of one relax problem over `world` ranks (one process per GPU, every rank creates the same
     * problem): rank r evaluates the residual blocks of camera pairs [r * chunk, (r + 1) * chunk),
     * chunk = ceil(n_pairs / world); after every evaluation `exchange` must all-gather the record arrays in place
     * (rank r's slice of an array starts at ptr + r * bytes_per_rank; acc_bytes_per_rank is 0 for a cost-only
     * evaluation) - an RCCL all-gather over xGMI in production (torch.distributed backend "nccl"), any transport
     * in tests - and return 0 once the gathered data is visible to later work on the context's stream.  The library
     * synchronises its stream before the call.  `exchange` is called whenever it is given, also with world == 1.  Every rank then runs the same deterministic assembly and linear solve on the same
     * records, so the result is bit-identical to the unsharded solve.  This is the one exchange step of the path
     * (single-group global relax, src/pipeline/pipeline.cpp:653-655; Ceres itself is single-process). */
    typedef int (*ochip_relax_exchange_fn)(void *user, void *acc_dev, uint64_t acc_bytes_per_rank, void *cost_dev,
                                           uint64_t cost_bytes_per_rank, void *fail_dev, uint64_t fail_bytes_per_rank);
    int ochip_relax_set_shard(ochip_relax_problem *p, uint32_t rank, uint32_t world, ochip_relax_exchange_fn exchange,
                              void *user);
    /* The native transport for that exchange: RCCL all-gathers, in place, on the context's compute stream (no host
     * wait: the solver's next kernels are on the same stream).  librccl is resolved at run time; the calls fail with
     * OCHIP_EHIP where it is absent.  Rank 0 draws the id (ncclGetUniqueId) and hands it to the other ranks by any means;
     * every rank then creates its communicator on the context its relax problem lives on and passes
     * ochip_rccl_relax_exchange / the communicator as `exchange` / `user` of ochip_relax_set_shard.
     * Stands where SURVEY.md section 8b sketches ochip_allreduce_normal_eq over ncclAllReduce: the per-pair records are
     * 4 MB per evaluation at C3 against 72 MB for the dense normal equations. */
#define OCHIP_RCCL_ID_BYTES 128
    typedef struct ochip_rccl_comm ochip_rccl_comm;
    int ochip_rccl_unique_id(ochip_ctx *ctx, uint8_t *id /* OCHIP_RCCL_ID_BYTES */);
    int ochip_rccl_comm_create(ochip_ctx *ctx, const uint8_t *id, uint32_t rank, uint32_t world, ochip_rccl_comm **out);
    void ochip_rccl_comm_destroy(ochip_rccl_comm *comm);
    int ochip_rccl_comm_stats(const ochip_rccl_comm *comm, uint64_t *exchanges, uint64_t *bytes_gathered);
    int ochip_rccl_relax_exchange(void *user, void *acc_dev, uint64_t acc_bytes_per_rank, void *cost_dev,
                                  uint64_t cost_bytes_per_rank, void *fail_dev, uint64_t fail_bytes_per_rank);
    /* cam_q: n_cams x 4; ochip_relax_solve leaves the optimised cameras' quaternions normalised exactly as
     * RelaxProblem::solve does after every Solve (:1410-1413); plane_z: 3 */
    int ochip_relax_get_state(ochip_relax_problem *p, double *cam_q, double *plane_z);
    /* One evaluation for tests, in the library's unknown order (n unknowns): the cost of the reduced program and, when not
     * NULL, the dense J'J (n x n; entries outside the stored tiles of the block envelope read as zero) and J'r (n).
     * route 0: the current state (delta must be NULL); route 1: the candidate x [+] delta the way an accepted LM step
     * evaluates it, with a Jacobi scale of 1 (the state buffers exchanged, with its Jacobian and the damping's diagonal into
     * the system's second set; J'J or J'r required);
     * route 2: the candidate as state 1 of the plain evaluation.  delta (n, or NULL = zero) is applied by the solver's
     * own candidate kernel; the current state is left as it is.  order_out (n_cams + 3): first unknown of every camera,
     * then of the three plane heights, or -1.  layout_out (4): n, the first unknown of the dense tail, the number of
     * regions of the band and the number of separator cameras.  cost NULL (and JtJ, Jtr NULL): n_out, order_out and
     * layout_out only, nothing evaluated.  Returns 1 for a non-finite block. */
    int ochip_relax_evaluate(ochip_relax_problem *p, int route, const double *delta, double *cost, int *n_out, double *JtJ,
                             double *Jtr, int32_t *order_out, int32_t *layout_out);

    /* ---- relax, general form: ground mesh, multi-ray tracks, shared intrinsics (replaces ceres::Solver::Solve on the
     *      problems RelaxProblem::setupGroundMeshProblem / setupGroundPlaneProblem build, src/relax/relax_problem.cpp:61-120:
     *      residual blocks of 2..5 rays on a triangle of the surface mesh (relax_cost_function.hpp:601-790), mesh priors
     *      (:51-69, :119-155; relax_problem.cpp:1303-1366), downward prior (:21-49), distortion monotonicity (:157-185)).
     *      Unknowns: 3 per optimised camera (quaternion tangent), 1 per optimised mesh vertex (height), and the shared
     *      inverse lens model: focal (bounded, :496-497), principal point, radial k1..k_n (SubsetManifold, :22-23). ---- */
    typedef struct ochip_relaxg_problem ochip_relaxg_problem;

    typedef struct ochip_relaxg_desc
    {
        uint32_t n_cams;
        const double *cam_pos;       /* n_cams x 3 */
        const double *cam_q;         /* n_cams x 4, x y z w */
        const uint8_t *cam_optimize; /* n_cams */
        uint32_t n_verts;            /* mesh vertices; their heights are the structure parameters */
        const double *vert_xy;       /* n_verts x 2 */
        const double *vert_z;        /* n_verts */
        const uint8_t *vert_optimize;
        uint32_t n_blocks;           /* ray blocks, in the order the reference adds them (tracks, then 2-ray blocks) */
        const uint8_t *blk_n;        /* rays of block b: 2 (Huber loss huber_a) or 3..5 (no loss) */
        const uint8_t *blk_intr;     /* 1 = the FocalRadial functor on the shared model (:501-566), NULL = none */
        const uint32_t *blk_ray_off; /* n_blocks + 1 */
        const uint32_t *blk_tri;     /* n_blocks x 3 vertex indices (the triangle under the rays) */
        const uint32_t *ray_cam;     /* per ray */
        const double *ray_dir;       /* per ray x 3: camera-frame unit ray (used by blocks with blk_intr = 0) */
        const double *ray_px;        /* per ray x 2: pixel (used by blocks with blk_intr = 1); may be NULL */
        uint32_t n_down;             /* PointsDownwardsPrior */
        const uint32_t *down_cam;
        double down_weight;          /* 1e-3 */
        uint32_t n_diff;             /* DifferenceCost between the heights of the two ends of a mesh edge */
        const uint32_t *diff_v;      /* n_diff x 2 */
        double diff_weight;          /* 1e-4 */
        double anchor_weight;        /* DifferenceCost of every vertex against its initial height (1e-5); 0 = none */
        uint32_t n_smooth;           /* AdjacentTriangleNormalCost per inner mesh edge: vertices A B C D */
        const uint32_t *smooth_v;    /* n_smooth x 4 */
        double smooth_weight;        /* 1e-4 */
        double huber_a;              /* 1 degree in radians */
        /* shared inverse lens model (InverseDifferentiableCameraModel) of the blk_intr blocks */
        double model[8];             /* f, ppx, ppy, k1, k2, k3, p1, p2 */
        uint8_t opt_focal, opt_principal, n_radial_free; /* n_radial_free: 0..3 leading radial coefficients are variable */
        double focal_lo, focal_hi;   /* 100, 20000 */
        uint32_t mono_observations;  /* DistortionMonotonicityCost: weight sqrt(n / 10); 0 = none */
        double mono_r_max;
        /* sharded evaluation over `shard_world` ranks (0 or 1 = not sharded): every rank creates the same problem and
         * evaluates its run of the ray blocks; ochip_relaxg_set_exchange names the transport */
        uint32_t shard_rank, shard_world;
        /* relation blocks of setupDecompositionProblem (src/relax/relax_problem.cpp:40-59,311-350):
         * MultiDecomposedRotationCost (relax_cost_function.hpp:188-307) between cameras rel_cam[2i], rel_cam[2i + 1] over
         * the four homography decompositions rel_pose[32 i ..] = 4 x {q xyzw, t xyz, score}, HuberLoss(rel_huber_a) */
        uint32_t n_rel;
        const uint32_t *rel_cam;
        const double *rel_pose;
        double rel_huber_a; /* 10 degrees in radians */
    } ochip_relaxg_desc;

    int ochip_relaxg_problem_create(ochip_ctx *ctx, const ochip_relaxg_desc *desc, ochip_relaxg_problem **out);
    void ochip_relaxg_problem_destroy(ochip_relaxg_problem *p);
    /* The exchange step of a problem created with shard_world > 1 (the reference's single global group is
     * {ORIENTATION, GROUND_MESH}, src/pipeline/pipeline.cpp:645-664): after every evaluation `exchange` all-gathers the
     * ranks' runs of the record array in place - same contract as ochip_relax_set_shard; ochip_rccl_relax_exchange with a
     * communicator created on the problem's context is the native transport.  The padded layout keeps every rank's run the
     * same size; the assembly and the cost sum then run on identical arrays in an order that does not depend on the
     * sharding, so the solve is bit-identical to the unsharded one on every rank.  A ray block's record is 0.4 - 2.6 KB
     * (the packed J'J of its 9 - 24 columns), so an evaluation exchanges a few hundred MB at C3 size: the sharding buys
     * nothing against an evaluation of ~1 ms on one GPU; it exists for memory (a survey whose records do not fit one
     * device) and for the contract of BASELINE config C4. */
    int ochip_relaxg_set_exchange(ochip_relaxg_problem *p, ochip_relax_exchange_fn exchange, void *user);
    /* relaxObservedModelOnly (:931-984): 1 = everything but the mesh heights held constant, 0 = undo */
    int ochip_relaxg_set_structure_only(ochip_relaxg_problem *p, int on);
    int ochip_relaxg_solve(ochip_relaxg_problem *p, const ochip_relax_options *opt, ochip_relax_summary *summary);
    /* cam_q: n_cams x 4 (optimised cameras normalised as RelaxProblem::solve leaves them), vert_z: n_verts, model: 8;
     * any may be NULL */
    int ochip_relaxg_get_state(ochip_relaxg_problem *p, double *cam_q, double *vert_z, double *model);
    /* One evaluation at the current state for tests: total cost, and (when not NULL) the dense J'J (n x n) and J'r (n) of
     * the reduced system in the library's unknown order; order_out (n_cams + n_verts + 3 entries) receives the first
     * unknown of every camera / vertex / f / pp / k or -1. */
    int ochip_relaxg_evaluate(ochip_relaxg_problem *p, double *cost, int *n_out, double *JtJ, double *Jtr, int32_t *order_out);

    /* ---- relax with 3-D points: reprojection bundle adjustment, the points eliminated by a per-point 3 x 3 Schur
     *      complement (replaces ceres::Solver::Solve with SPARSE_SCHUR on the problem RelaxProblem::setup3dPointProblem
     *      builds, src/relax/relax_problem.cpp:122-145,986-1187: PixelErrorCost_Orientation[Focal[Radial[Tangential]]],
     *      relax_cost_function.hpp:309-500, HuberLoss(10 px), focal bounds, SubsetManifold of the radial block,
     *      DistortionMonotonicityCost :157-185).  Every point is seen by exactly two cameras - the reference makes one
     *      point per whitelisted inlier of an edge - and the points of one edge form a group: points
     *      [grp_first[g], grp_first[g + 1]) are seen by cameras grp_cam[2g] (pixels obs_px[2p]) and grp_cam[2g + 1]
     *      (obs_px[2p + 1]).  Unknowns of the reduced system: 3 per optimised camera (quaternion tangent) and the shared
     *      lens model's free parameters; the points are back-substituted. ---- */
    typedef struct ochip_relaxp_problem ochip_relaxp_problem;
    typedef struct ochip_relaxp_desc
    {
        uint32_t n_cams;
        const double *cam_pos;       /* n_cams x 3 */
        const double *cam_q;         /* n_cams x 4, x y z w */
        const uint8_t *cam_optimize; /* n_cams */
        uint32_t n_points;
        const double *point_xyz;     /* n_points x 3: the triangulated starting points */
        uint32_t n_groups;
        const uint32_t *grp_first;   /* n_groups + 1 */
        const uint32_t *grp_cam;     /* n_groups x 2 */
        const double *obs_px;        /* (2 n_points) x 2 pixels */
        int functor;                 /* 0 Orientation, 1 OrientationFocal, 2 ...Radial, 3 ...RadialTangential */
        double model[8];             /* f, ppx, ppy, k1, k2, k3, p1, p2 of the shared forward lens model */
        uint8_t opt_focal, opt_principal, n_radial_free; /* functor >= 1: f / pp variable; functor >= 2: 0..3 leading radial
                                                            coefficients variable (3 = a free Euclidean block) */
        double focal_lo, focal_hi;   /* bounds of a variable focal length (100, 20000) */
        double huber_a;              /* 10 px */
        uint32_t mono_observations;  /* DistortionMonotonicityCost (functor >= 2): weight sqrt(n / 10); 0 = none */
        double mono_r_max;
    } ochip_relaxp_desc;
    int ochip_relaxp_problem_create(ochip_ctx *ctx, const ochip_relaxp_desc *desc, ochip_relaxp_problem **out);
    void ochip_relaxp_problem_destroy(ochip_relaxp_problem *p);
    /* relaxObservedModelOnly (:931-984): 1 = cameras and lens model held constant, only the points move; 0 = undo */
    int ochip_relaxp_set_structure_only(ochip_relaxp_problem *p, int on);
    int ochip_relaxp_solve(ochip_relaxp_problem *p, const ochip_relax_options *opt, ochip_relax_summary *summary);
    /* cam_q: n_cams x 4 (optimised cameras normalised), point_xyz: n_points x 3, model: 8; any may be NULL */
    int ochip_relaxp_get_state(ochip_relaxp_problem *p, double *cam_q, double *point_xyz, double *model);
    /* Test seams.  ochip_relaxp_evaluate: one evaluation with Jacobians at the current state (the engine's own kernels):
     * the total cost, n (unknowns of the reduced system), U (n x n, both triangles) and g_c (n) in the library's unknown
     * order, per point V (6: xx xy xz yy yz zz) and g_p (3), gmax_p = the largest |g| over the point columns; order_out
     * (n_cams + 8) = the first unknown of every camera, then of f, ppx, ppy, k1, k2, k3, p1, p2, or -1.  Outputs may be
     * NULL; with all of cost .. gmax_p NULL nothing is evaluated (n and the order only).  Returns 1 when an observation is
     * not finite.
     * ochip_relaxp_step: one LM step on the Jacobian of the last ochip_relaxp_evaluate, as lm_solve takes it: the damped,
     * scaled reduced system with the points' Schur term, its factorisation and back-solve, the candidate state.  scale_in
     * (n, NULL: the solver's 1 / (1 + sqrt(diag U))) scales the reduced unknowns; the points' scaling is the engine's own,
     * fixed by the first step after create / solve / set_structure_only.  y_in (n, may be NULL) replaces the solved y
     * before the candidate is formed.  alpha2 != 0: the candidate is formed a second time, as the line search contracts a
     * step (the stored point step times alpha2, then the slope kernel); the outputs are then the second candidate's.
     * Output (any may be NULL): W_out ((n + 1) x n, lower triangle) the reduced system as built, row n its right-hand
     * side; y_out (n) the solved y; the candidate cam_q2 (n_cams x 4), model2 (8), X2 (n_points x 3); pt_scale (3 per
     * point), pt_Vinv (6) and pt_d (3, the unscaled full step of the point); scal_out[4] = model cost change, |x -
     * candidate|^2, |candidate|^2, g_p . d_p; fail_out the factorisation's failure flag.  The current state is untouched. */
    int ochip_relaxp_evaluate(ochip_relaxp_problem *p, double *cost, int *n_out, double *U, double *g_c, double *V, double *g_p,
                              double *gmax_p, int32_t *order_out);
    int ochip_relaxp_step(ochip_relaxp_problem *p, double radius, const double *scale_in, const double *y_in, double alpha2,
                          double *W_out, double *y_out, double *cam_q2, double *model2, double *X2, double *pt_scale, double *pt_Vinv,
                          double *pt_d, double *scal_out, int32_t *fail_out);

    /* ---- profiling: HIP-event time of every launch of a kernel since the last reset ------------- */
    int ochip_profile_reset(ochip_ctx *ctx);
    int ochip_profile_get(ochip_ctx *ctx, int kernel_id, uint64_t *launches, double *total_ms);
    /* descriptor distances of the match launches since the last ochip_profile_reset (siblings included): computed (a pair
     * matched in both directions from one pass counts its n1 x n2 distances once) and delivered (twice) */
    int ochip_match_work(ochip_ctx *ctx, uint64_t *computed, uint64_t *delivered);
    /* fp64 flops the relax solves issued on the matrix cores (the panel and trailing-update GEMMs of their Cholesky
     * factorisations, inside the block envelope) since the last ochip_profile_reset; their time is OCHIP_K_RELAX_SOLVE's */
    int ochip_relax_work(ochip_ctx *ctx, double *mfma_flops);
    /* roofline bookkeeping since the last ochip_profile_reset (siblings included): counters3[0] = sum over the homography
     * RANSAC jobs of loop trips x correspondences (an upper bound of the (hypothesis, correspondence) errors evaluated -
     * the SPRT exit of src/model_inliers/ransac.cpp:197-200 leaves a hypothesis early; time: OCHIP_K_RANSAC),
     * [1] / [2] = 2-ray residual blocks the ground-plane engine evaluated with / without Jacobians (OCHIP_K_RELAX_EVAL) */
    int ochip_work_counters(ochip_ctx *ctx, uint64_t *counters3);
    /* the largest reduced system a relax on this context (or a sibling) has held: its unknowns, the bytes of J'J and its
     * factor as stored (64 x 64 tiles of the block envelope, lower triangle) and what the same two matrices take dense -
     * the reference hands this system to ceres::SPARSE_NORMAL_CHOLESKY (src/relax/relax_problem.cpp:30-37) */
    int ochip_relax_memory(ochip_ctx *ctx, uint64_t *unknowns, uint64_t *stored_bytes, uint64_t *dense_bytes);

    /* ---- diagnostics ----------------------------------------------------------------------------- */
    /* libstdc++'s std::sort on the device (csrc/std_sort.hip), for the tests: segment s = [offsets[s], offsets[s + 1]) of
     * (keys, payload), sorted as std::sort with comp(a, b) = key(a) > key(b) leaves them - the permutation among equal keys
     * included.  fallback_out[s] != 0: the segment hit introsort's depth limit (libstdc++ heap-sorts there) and is NOT
     * sorted; callers sort such a segment on the host. */
    int ochip_debug_std_sort(ochip_ctx *ctx, const uint32_t *keys, const uint32_t *payload, const uint32_t *offsets, uint32_t n_segs,
                             uint32_t *keys_out, uint32_t *payload_out, uint8_t *fallback_out);
    /* out[i] = x[i] op y[i] computed on the device with the hot-path kernels' compile flags:
     * op 0: x/y, 1: sqrt(x), 2: log(x), 3: x*y+x (unfused), 4: x+y.  Host pointers. */
    int ochip_debug_fp64(ochip_ctx *ctx, int op, const double *x, const double *y, size_t n, double *out);
    /* The linear algebra of one relax LM step on a given system, for the tests: the plan of lm_system_resize and the
     * launches of lm_solve (relax_lm.hip: lm_linear_step).  Input: A (n x n row-major, lower triangle read; a non-zero
     * outside the envelope is OCHIP_EINVAL), g, scale, diagonal (n each), the trust-region radius and the envelope as
     * lm_envelope holds it: env_end per 64-column block (ceil(n / 64) entries), tail_begin and n_region_begin first blocks
     * of the band's regions (may be 0).  route 0: chol_tiles_kernel, 1: the launch chain chol_diag / panel / update.
     * back 0: the back-solve lm_solve picks, 1: back_solve_kernel (one workgroup), 2: back_solve_regions_kernel with x in
     * LDS, 3: the same with x in HBM.  Output: x (n) solves (S A S + D) x = S g, y (n) = L^-1 S g (the factored
     * augmented row), L_out (n x n, may be NULL) the factor with unstored entries 0, W_out ((n + 1) x n, may be NULL) the
     * system as built, lower triangle, row n = S g; scal1_out the model cost change (may be NULL); info_out[8]: [0] the
     * factorisation's failure flag, [1] the claim order (0 column order, 1 tail first, 2 regions), [2] the device's
     * slots for the factorisation's workgroups, [3] stored tiles, [4] claims, [5] regions, [6] the back-solve run (1 - 3),
     * [7] 0.  Host pointers.  n = 0: nothing to factor, OCHIP_OK. */
    int ochip_debug_lm_step(ochip_ctx *ctx, int n, const double *A, const double *g, const double *scale, const double *diagonal,
                            double radius, const int32_t *env_end, int32_t tail_begin, const int32_t *region_begin, int32_t n_region_begin,
                            int32_t route, int32_t back, double *x_out, double *y_out, double *L_out, double *W_out, double *scal1_out,
                            int32_t *info_out);

    /* ---- dense guided matching: the descriptor search of densifyMesh (src/dense/dense_stereo.cpp:245-283) ------------
     * The index holds, for every image, its dense features sorted by the cell of a uniform grid over the image (cell edge
     * cell_size > the search radius): feat_off (n_images + 1) offsets into desc8 (8 u64 per feature) / loc2 (x, y), per
     * image a table of ncx * ncy + 1 cell starts (relative to the image's first feature) at cell_off[i] in cell_start,
     * grid2 = {ncx, ncy} and origin2 = the grid's corner per image; a feature at (x, y) lies in cell
     * (floor((x - ox) / cell_size), floor((y - oy) / cell_size)).  A query names a feature of the index (its descriptor is
     * the probe), the image to search and the predicted pixel; the result is the nearest and second nearest Hamming
     * distance among that image's features with squared pixel distance < radius^2, the nearest one's position in the
     * image's sorted order, and how many features the disc held.  0xFFFF = no such neighbour. */
    typedef struct ochip_dense_index ochip_dense_index;
    typedef struct ochip_dense_query
    {
        uint32_t src_feature; /* position in the index (all images concatenated) */
        uint32_t cand_image;
        double px, py;
    } ochip_dense_query;
    typedef struct ochip_dense_result
    {
        uint32_t best_feature; /* position within cand_image's features */
        uint16_t best_count, second_count;
        uint32_t nearby;
    } ochip_dense_result;
    int ochip_dense_index_create(ochip_ctx *ctx, uint32_t n_images, const uint64_t *feat_off, const uint64_t *desc8,
                                 const double *loc2, const uint64_t *cell_off, const uint32_t *cell_start, const int32_t *grid2,
                                 const double *origin2, double cell_size, ochip_dense_index **out);
    void ochip_dense_index_destroy(ochip_dense_index *ix);
    int ochip_dense_match(ochip_dense_index *ix, const ochip_dense_query *queries, uint64_t n_queries, double radius,
                          ochip_dense_result *out);
    /* densifyMesh after the mesh intersections, whole survey, on the device (replaces the rest of the per-feature loop of
     * src/dense/dense_stereo.cpp:174-297 - the k nearest cameras of the hit point, its projection into each, the disc
     * search, the accept rule - and the union of the matched measurements; ochip_dense_match stays for callers that
     * build their queries themselves).
     * cams17 [n_images][17]: position (3), orientation.inverse() (4, xyzw), model10 (f ppx ppy k1 k2 k3 p1 p2 cols rows);
     * id_of_pos [total]: the reference's measurement id (image offset + dense feature number) of every index position - a
     * permutation of [0, total), anything else is OCHIP_EINVAL;
     * hits3 [total][3] by index position: where the feature's ray meets the mesh, x = NaN: nowhere (:196-207).
     * max_candidates = MAX_CANDIDATE_IMAGES (10), descriptor_bits = 486, ratio = 0.85, max_abs = 0.35 (:51-56).
     * root_out [total] by measurement id: the smallest member of the measurement's track, 0xFFFFFFFF = unmatched;
     * counts2: queries issued, matches accepted; slot_dst_out (may be NULL) [total][11]: per feature and candidate in
     * nearest-camera order the accepted match's measurement id or 0xFFFFFFFF (tests: the reference's match order). */
    int ochip_dense_link(ochip_dense_index *ix, const double *cams17, const uint32_t *id_of_pos, const double *hits3, double radius,
                         uint32_t max_candidates, uint32_t descriptor_bits, double ratio, double max_abs, uint32_t *root_out,
                         uint64_t *counts2, uint32_t *slot_dst_out);

    /* The tracks' 3-D points (dense_stereo.cpp:299-340 with triangulateTrack, :112-172) after ochip_dense_link on the same
     * index: track t = the measurement ids track_member[track_start[t] .. track_start[t + 1]) in ascending order; its first two
     * rays meet in a point, members reprojecting within max_reprojection_error px are inliers, fewer than two give no point,
     * fewer than all give the point of the first two inliers (a member >= the index's measurement count: OCHIP_EINVAL).
     * cam_q4 [n_images][4]: the images' orientations (x y z w).
     * points3_out [n_tracks][3], valid_out [n_tracks] (0: the track has no point). */
    int ochip_dense_triangulate(ochip_dense_index *ix, const double *cam_q4, uint32_t n_tracks, const uint32_t *track_start,
                                const uint32_t *track_member, double max_reprojection_error, double *points3_out, uint8_t *valid_out);

    /* ---- orthomosaic preview and DSM raster (src/ortho/ortho.cpp:478-653, 793-856) -----------------------------------
     * The mesh table: n_surfaces surfaces in the reference's order (the first that holds a pixel wins), surface s owning
     * triangles [tri_off[s], tri_off[s + 1]) of tri9 (three corners xyz each, in ascending mesh node order).  The library
     * bins every surface's triangles into a uniform grid; a pixel takes the first triangle of its cell, in table order,
     * that contains it (the walker's predicates: a point on an edge is inside).
     * raster4 = {min_x, max_y, gsd, mean_camera_z}: pixel (row, col) is the vertical ray through
     * (col * gsd + min_x, max_y - row * gsd) from height mean_camera_z. */
    typedef struct ochip_ortho_mesh ochip_ortho_mesh;
    int ochip_ortho_mesh_create(ochip_ctx *ctx, uint32_t n_surfaces, const uint64_t *tri_off, const double *tri9,
                                ochip_ortho_mesh **out);
    void ochip_ortho_mesh_destroy(ochip_ortho_mesh *m);
    /* DSM rows [row0, row0 + rows) of a raster `cols` wide: out[(row - row0) * cols + col] = (float)z, NaN where no surface
     * holds the pixel.  out_on_device != 0: out is a device pointer of this context's GPU, else a host pointer.  The kernels
     * run on the context's stream, which does not wait for other streams: the caller finishes its own work on `out` first.
     * The call returns once the band is written.
     * Debug outputs (host, may be NULL): tri_out the triangle (table index) that gave z, 0xFFFFFFFF where none did;
     * z64_out z in fp64. */
    int ochip_ortho_dsm(ochip_ortho_mesh *m, const double *raster4, int32_t cols, int64_t row0, int64_t rows, float *out,
                        int out_on_device, uint32_t *tri_out, double *z64_out);
    /* The preview raster, rows x cols: per pixel z as above; where it exists, the first of the 5 nearest cameras in XY
     * (squared distance, then camera order) with R_inv * (p - position) in front of it whose projection, scaled by
     * thumb_scale and truncated, lies strictly inside its thumbnail (0 < px < cols, 0 < py < rows) gives
     * (r, g, b, 255) and cam_id; none does: checkerboard grey (64 or 128 by (row + col) parity), alpha 0, id 0xFFFFFFFF;
     * no surface: (0, 0, 0, 0) and 0xFFFFFFFF.
     * cams24 [n_cams][24]: position 3, R_inv 9 (row-major), f, ppx, ppy, k1, k2, k3, p1, p2, thumb_scale, thumbnail rows,
     * thumbnail cols, 0.  Thumbnail i: rows x cols x 3 bytes at thumbs + thumb_off[i] (thumb_bytes in all).
     * rgba_out [rows][cols][4], id_out [rows][cols]; z_out (fp64) and tri_out may be NULL.  Host pointers. */
    int ochip_ortho_thumbnail(ochip_ortho_mesh *m, const double *raster4, int32_t cols, int32_t rows, uint32_t n_cams,
                              const double *cams24, const uint32_t *cam_id, const uint64_t *thumb_off, const uint8_t *thumbs,
                              uint64_t thumb_bytes, uint8_t *rgba_out, uint32_t *id_out, double *z_out, uint32_t *tri_out);

    /* ---- layered full-resolution orthomosaic (src/ortho/ortho.cpp:1206-1663; opencalibration_amd/csrc/ortho_layers.hpp) ----
     * One colour correspondence (include/opencalibration/ortho/color_balance.hpp:25-49) and where it was taken: raster
     * row / col of the sample pixel and the two layers.  96 bytes, no padding. */
    typedef struct ochip_color_corr
    {
        float lab_a[3], lab_b[3];
        uint64_t camera_id_a, camera_id_b;
        uint32_t model_id_a, model_id_b;
        float normalized_radius_a, normalized_radius_b, view_angle_a, view_angle_b;
        float normalized_x_a, normalized_y_a, normalized_x_b, normalized_y_b;
        int32_t row, col;
        uint32_t layer_a, layer_b;
    } ochip_color_corr;
    /* Rows [row0, row0 + rows) of the layered raster `cols` wide (raster4 as ochip_ortho_dsm); row0 a multiple of the tile
     * size, so that the band is whole output tiles (the last tile row may be partial).  config4 = {num_layers (1..8),
     * tile_size, correspondence_kernel_radius, correspondence_subsample}.  Per pixel: the mesh height as (float)z; the 5
     * nearest cameras in XY (squared distance, then camera order); for each in turn, skipped when R_inv (p - position)
     * has z <= 0 or the projection lies outside [0, cols) x [0, rows), the next layer takes the patch sample and its
     * bookkeeping (ortho_layers.hpp), until num_layers.  Invalid layers: BGRA (0, 0, 0, 0), id 0, weight 0.  Then the
     * colour correspondences of the finished band, output tiles row-major, local raster order, (a, b) lexicographically.
     * cams [n_cams][28]: position 3, R_inv 9 (row-major), f, ppx, ppy, k1, k2, k3, p1, p2, pixels_cols, pixels_rows,
     * orientation^-1 (0, 0, 1), 3 unused; node_ids, model_ids per camera; images [n_cams] device pointers to
     * pixels_rows x pixels_cols x 3 BGR bytes each (the caller checks their size).
     * bgra_out [L][rows][cols][4], id_out [L][rows][cols], weight_out [L][rows][cols] (may be NULL): device pointers of
     * this context's GPU when out_on_device, else host; the context's stream does not wait for other streams.  The
     * correspondences (host): the first min(*n_corr, corr_capacity) into corr_out (may be NULL with capacity 0), their
     * number in *n_corr.  knn_out (host, may be NULL): [rows][cols][5] camera indices, 0xFFFFFFFF padded. */
    int ochip_ortho_layers(ochip_ortho_mesh *m, const double *raster4, int32_t cols, int64_t row0, int64_t rows,
                           const int32_t *config4, uint32_t n_cams, const double *cams, const uint64_t *node_ids,
                           const uint32_t *model_ids, const uint64_t *images, int out_on_device, uint8_t *bgra_out,
                           uint64_t *id_out, float *weight_out, ochip_color_corr *corr_out, uint64_t corr_capacity,
                           uint64_t *n_corr, uint32_t *knn_out);

    /* The cameras each band of a raster can read: the raster rows x cols (raster4 as ochip_ortho_dsm) cut into bands of
     * band_rows rows from row 0 (the last may be shorter), n_bands = ceil(rows / band_rows).  used_out (host)
     * [n_bands][n_cams]: 1 exactly when the camera is among the 5 nearest in XY (squared distance, then camera order;
     * ochip_ortho_layers' kNN) of at least one pixel of the band, else 0.  Pixels count whatever their height, so the set
     * needs no mesh and holds every camera ochip_ortho_layers reads for the band.  At most 65535 16-row tile rows in all. */
    int ochip_ortho_band_cameras(ochip_ctx *ctx, const double *raster4, int32_t cols, int64_t rows, int64_t band_rows,
                                 uint32_t n_cams, const double *cams, uint8_t *used_out);
    /* Image slots for a render that streams its source images: n_slots blocks of slot_bytes (rounded up to 256) in one
     * block of the context's pool, and n_marks events.  ochip_image_slots_upload enqueues a host-to-device copy into a
     * slot on the context's copy stream and returns at once when `host` is page-locked (pageable memory: correct, not
     * overlapped); the caller keeps `host` alive until a mark behind the copy has passed.  ochip_image_slots_mark records
     * mark i behind everything enqueued on the copy stream so far; ochip_image_slots_wait makes the context's compute
     * stream (on_host != 0: the calling thread) wait for it; ochip_image_slots_elapsed waits for to_mark and gives the
     * milliseconds between two recorded marks.  ochip_image_slots_address: the slot's device address, 0 when out of range.
     * Nothing here orders an upload against a kernel that still reads the slot: the caller does (och_ortho_stream_*).
     * Destroy waits for both streams and hands the block back. */
    typedef struct ochip_image_slots ochip_image_slots;
    int ochip_image_slots_create(ochip_ctx *ctx, uint32_t n_slots, uint64_t slot_bytes, uint32_t n_marks, ochip_image_slots **out);
    void ochip_image_slots_destroy(ochip_image_slots *s);
    uint64_t ochip_image_slots_address(const ochip_image_slots *s, uint32_t slot);
    int ochip_image_slots_upload(ochip_image_slots *s, uint32_t slot, const void *host, uint64_t bytes);
    int ochip_image_slots_mark(ochip_image_slots *s, uint32_t mark);
    int ochip_image_slots_wait(ochip_image_slots *s, uint32_t mark, int on_host);
    int ochip_image_slots_elapsed(ochip_image_slots *s, uint32_t from_mark, uint32_t to_mark, float *ms);

    /* ---- blended full-resolution orthomosaic (src/ortho/ortho.cpp:1665-1990, src/ortho/blending.cpp;
     * opencalibration_amd/csrc/ortho_blend.hpp) ----
     * One node id the layers may name, the table sorted by id, ids unique: cam, its row in cams (0xFFFFFFFF: none, the
     * sample keeps black and weight 0), and its colour balance (has_color 0: no entry, no correction).  64 bytes. */
    typedef struct ochip_blend_id
    {
        uint64_t id;
        uint32_t cam, has_color;
        double lab_offset[3], brdf, slope[2];
    } ochip_blend_id;
    /* Rows [row0, row0 + rows) of the blended orthomosaic `cols` wide, whole tile rows from a tile row (the raster's last
     * may be partial); raster3 = {min_x, max_y, gsd}; config4 = {num_layers (1..8), tile_size (1..4096), pyramid_levels,
     * blend_transition_radius (>= 1)}.  Inputs as ochip_ortho_layers writes them: bgra [L][rows][cols][4] (valid: alpha
     * > 0), id [L][rows][cols], and the DSM band dsm [rows][cols]; cams [n_cams][28] as ochip_ortho_layers'.  vig0: the
     * vignetting coefficients of model id 0 (NULL: no entry), which every sample uses.  rgba_out [rows][cols][4].
     * bgra, id, dsm and rgba_out are device pointers of this context's GPU when on_device, else host.  Debug outputs
     * (host, each may be NULL): weight_out [L][rows][cols] the recomputed weight before the falloff, dist_out
     * [rows][cols] the boundary distance (+inf: no boundary in the tile), lab_out [L][rows][cols][3] the corrected Lab. */
    int ochip_ortho_blend(ochip_ctx *ctx, const double *raster3, int32_t cols, int64_t row0, int64_t rows,
                          const int32_t *config4, uint32_t n_cams, const double *cams, uint32_t n_ids,
                          const ochip_blend_id *ids, const double *vig0, int on_device, const uint8_t *bgra,
                          const uint64_t *id, const float *dsm, uint8_t *rgba_out, float *weight_out, float *dist_out,
                          float *lab_out);
    /* laplacianBlend (src/ortho/blending.cpp) alone on one rows x cols tile (each at most 4096) on the device, the steps
     * of ochip_ortho_blend: lab [L][rows][cols][3] float Lab, weight [L][rows][cols], host; bgra_out [rows][cols][4]
     * host, alpha 255. */
    int ochip_laplacian_blend(ochip_ctx *ctx, int32_t num_layers, int32_t rows, int32_t cols, int32_t pyramid_levels,
                              const float *lab, const float *weight, uint8_t *bgra_out);

    /* ---- colour balance between the layered render and the blend (solveColorBalance, src/ortho/color_balance.cpp;
     * opencalibration_amd/csrc/color_balance.hpp) ----
     * The problem: per camera id lab_offset[3], brdf, slope[2], per model id three vignetting coefficients, all starting
     * at 0; per correspondence three residuals under HuberLoss(5) (RadiometricMatchCost and its shared-model variant are
     * one formula), priors of weight 0.1 sqrt(max(1, appearances)) on every unknown; max_num_iterations 20, function /
     * gradient / parameter tolerance 1e-4 / 1e-6 / 1e-4, initial trust-region radius 1e4, Ceres' defaults otherwise.
     * corr (host, n_corr > 0): the records ochip_ortho_layers writes; cam_ids, model_ids (host): sorted, unique, holding
     * every id the correspondences name.  A correspondence whose camera_id_a == camera_id_b is refused with OCHIP_EINVAL:
     * the reference's ceres::Problem aborts on a residual block that names one parameter block twice.
     * cam6_out [n_cams][6], vig3_out [n_models][3] in the tables' order, BEFORE the gauge removal (the host library's,
     * och_color_balance_solve).  summary as ochip_relax_solve's: success = termination != OCHIP_RELAX_FAILURE; a
     * non-finite observation fails at iteration 0 (iterations 0, the parameters stay 0).  Two solves of one input are
     * bit-identical. */
    int ochip_color_balance_solve(ochip_ctx *ctx, const ochip_color_corr *corr, uint64_t n_corr, const uint64_t *cam_ids,
                                  uint32_t n_cams, const uint32_t *model_ids, uint32_t n_models, double *cam6_out,
                                  double *vig3_out, ochip_relax_summary *summary);
    /* One evaluation at the given parameters for tests: total cost, and (when not NULL) the dense J'J (n x n) and J'r (n)
     * in the library's unknown order, n = 6 n_cams + 3 n_models into *n_out; cam_col [n_cams], model_col [n_models]
     * receive the first unknown of every camera / model.  Returns 0, 1 when a residual is not finite, or a negative code. */
    int ochip_color_balance_evaluate(ochip_ctx *ctx, const ochip_color_corr *corr, uint64_t n_corr, const uint64_t *cam_ids,
                                     uint32_t n_cams, const uint32_t *model_ids, uint32_t n_models, const double *cam6,
                                     const double *vig3, double *cost, int32_t *n_out, double *JtJ, double *Jtr,
                                     int32_t *cam_col, int32_t *model_col);

    /* ---- the load stage's image thumbnails (opencalibration_amd/csrc/thumbnail.hip; src/extract/extract_image.cpp:42-52:
     *      BGR -> 8-bit Lab, INTER_AREA by 50 / sqrt(pixels), Lab -> BGR, stored R G B) ---- */
    /* rows = rint(height * scale), cols = rint(width * scale), ties to even.  OCHIP_EINVAL for a side outside 1..65535, an
     * image of fewer than 2500 pixels (scale > 1) and a thumbnail side of 0.  Needs no device. */
    int ochip_thumbnail_size(int width, int height, int32_t *rows, int32_t *cols);
    /* images_bgr: n_images x height x width x 3 bytes, a device pointer when images_on_device; rgb_out (host): n_images x
     * rows x cols x 3, R G B interleaved - the layout och_graph_set_thumbnail takes.  The first call on a context fills
     * the context's table of all 2^24 BGR codes' Lab (64 MB of HBM, kept until the context goes). */
    int ochip_image_thumbnails(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                               int images_on_device, uint8_t *rgb_out);
    /* For tests and probes: out[i] = that table's entry (L | a << 8 | b << 16) of code B | G << 8 | R << 16 = codes[i]
     * (host arrays; n may be 0); fill_ms (may be NULL): what the one launch that filled the table took. */
    int ochip_debug_lab_table(ochip_ctx *ctx, const uint32_t *codes, size_t n, uint32_t *out, float *fill_ms);

    /* ---- averaged overview levels of the orthomosaic and the DSM (opencalibration_amd/csrc/ortho_overview.hip, the rule in
     *      csrc/ortho_overview.hpp; the reference's BuildOverviews("AVERAGE", 2, 4, 8, ...), src/ortho/ortho.cpp:944-961,
     *      1642-1657, 2028-2044) ----
     * Level 0 is the raster, width x height pixels of 4 bytes; the levels are k = 1, 2, ... for every factor 2^k <
     * min(width, height), level k of ceil(height / 2^k) rows and ceil(width / 2^k) columns.  Pixel (r, c) of level k comes
     * from its cell, the pixels (2r .. 2r + 1, 2c .. 2c + 1) of level k - 1 that exist (4, 2 or 1).
     * OCHIP_OVERVIEW_RGBA8 (alpha is byte 3; BGRA alike): n = cell pixels with alpha > 0, m = all of them; n = 0 gives
     * (0, 0, 0, 0), else every colour is (sum over the n valid + n / 2) / n and alpha (sum over all m + m / 2) / m in
     * integers.  OCHIP_OVERVIEW_FLOAT32 (NaN: no data; inputs finite or NaN): the double sum of the cell's non-NaN pixels
     * in the order top-left, top-right, bottom-left, bottom-right over their count, rounded once to float; NaN when none.
     * ochip_ortho_overviews_levels: the number of levels (0 for min(width, height) <= 2; OCHIP_EINVAL for a side below 1)
     * and, when rows_cols is not NULL, {rows, cols} of levels 1, 2, ...  Needs no device.
     * The builder is fed level 0 band by band and writes into the caller's level buffers (levels[k - 1]: level k, whole;
     * device pointers of this context's GPU when on_device, else host - then the fed bands are host memory too, and a feed
     * uploads its band, downloads the rows it completed and waits).  feed: rows [row0, row0 + rows) of level 0, bands in
     * ascending order and contiguous from row 0, of any row count; with device bands it enqueues on the context's stream
     * and does not wait.  complete_rows: the rows of level `level` (1 ..) the feeds so far have computed, monotone (0 for a
     * level that does not exist).  finish: after the last row; waits for the stream, the levels are then the caller's to
     * read.  Refused with OCHIP_EINVAL and a message that names the rows: a gap, an overlap, rows beyond the raster, a feed
     * after finish, finish before the last row.  The only state between feeds is one pending level-0 row (a band that ends
     * on an odd row) in a block of the context's pool; destroy waits for the stream and hands it back. */
#define OCHIP_OVERVIEW_RGBA8 0
#define OCHIP_OVERVIEW_FLOAT32 1
    typedef struct ochip_ortho_overviews ochip_ortho_overviews;
    int ochip_ortho_overviews_levels(int64_t width, int64_t height, int64_t *rows_cols);
    int ochip_ortho_overviews_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, void *const *levels, int on_device,
                                     ochip_ortho_overviews **out);
    int ochip_ortho_overviews_feed(ochip_ortho_overviews *o, int64_t row0, int64_t rows, const void *band);
    int64_t ochip_ortho_overviews_complete_rows(const ochip_ortho_overviews *o, int level);
    int ochip_ortho_overviews_finish(ochip_ortho_overviews *o);
    void ochip_ortho_overviews_destroy(ochip_ortho_overviews *o);

    /* ---- points per triangle of a surface mesh (opencalibration_amd/csrc/mesh_points.hip, the rule in
     *      csrc/mesh_locate.hpp; the reference's countPointsPerTriangle, src/surface/refine_mesh.cpp:713-825, the expensive
     *      part of the DENSE_MESH_RELAX state) ----
     * The object holds a cloud, xyz [n][3] fp64 (n < 2^32; n = 0 is valid), uploaded once by create; the mesh changes from
     * count to count and arrives as a flat locate table (host arrays, built by the host library from a mesh and an edge
     * order): per located triangle the x, y of its vertices [T][6], its neighbours [T][3] as triangle indices or
     * OCHIP_LOCATE_NONE, its plane [T][6] (origin, unit normal), its centroid, and the centroids' bucket grid of nx x nx
     * cells (start: n_start = nx * nx + 1 offsets into items, n_items = T triangle indices).
     * count: every point is located - nearest centroid, then a walk of at most max_steps triangles - and per triangle come
     * back the number of its points, the index of its first point (OCHIP_LOCATE_NONE without one), and sum and sum of
     * squares of the points' signed plane distances added in ascending point index, bit for bit what a sequential host
     * loop gives.  A point whose steps ran out is in none of these: its index comes back in `exhausted` (ascending;
     * exhausted_cap entries, n is always enough) and the caller resolves it by scanning the mesh.  Nothing is carried from
     * one count to the next except the answer of `where`: the last count's per-point result (triangle index,
     * OCHIP_LOCATE_NONE outside the mesh, OCHIP_LOCATE_EXHAUSTED | the triangle the walk stood on).
     * The table is checked before anything is launched: OCHIP_EINVAL and a message for a neighbour or an item >= T, a
     * start that is not monotone from 0 to T, a grid side outside 1 .. 1024, a NULL array.  OCHIP_EINVAL too for a handle
     * that create did not return or destroy has taken (then the message is ochip_last_error(NULL)'s).  The calls wait for
     * the context's stream; destroy hands the device blocks back to the context's pool. */
#define OCHIP_LOCATE_NONE 0xFFFFFFFFu
#define OCHIP_LOCATE_EXHAUSTED 0x80000000u
    typedef struct ochip_locate_table
    {
        uint32_t n_triangles; /* T */
        const double *vertex_xy;
        const uint32_t *neighbours;
        const double *plane;
        const double *centroid_x, *centroid_y;
        double x0, y0, cell;
        int32_t nx;
        const uint32_t *start;
        size_t n_start;
        const uint32_t *items;
        size_t n_items;
    } ochip_locate_table;
    typedef struct ochip_mesh_points ochip_mesh_points;
    int ochip_mesh_points_create(ochip_ctx *ctx, const double *xyz, uint64_t n, ochip_mesh_points **out);
    uint64_t ochip_mesh_points_size(const ochip_mesh_points *m); /* n; 0 for a handle that is not live */
    int ochip_mesh_points_count(ochip_mesh_points *m, const ochip_locate_table *table, int max_steps, uint32_t *count /* [T] */,
                                uint32_t *first /* [T] */, double *sum /* [T] */, double *sum_sq /* [T] */, uint32_t *exhausted,
                                uint64_t exhausted_cap, uint64_t *n_exhausted);
    int ochip_mesh_points_where(ochip_mesh_points *m, uint32_t *where /* [n] */);
    void ochip_mesh_points_destroy(ochip_mesh_points *m);

    /* ---- per-tile progress thumbnails of the layer and blend passes (opencalibration_amd/csrc/ortho_tile_thumbs.hip, the
     *      arithmetic in csrc/ortho_tile_thumbs.hpp; the reference's TileProgressCallback, src/ortho/ortho.cpp:1553-1614 and
     *      1962-2011) ----
     * A band of rows x cols pixels - whole tile rows from a tile row - is cut into tiles of tile_size T (1..4096), counted
     * row-major; tile (tx, ty) is tw = min(T, cols - tx T) by th = min(T, rows - ty T).  Its thumbnail takes every scale-th
     * pixel, scale = max(1, (max(tw, th) + 127) / 128), thumb_w = (tw + scale - 1) / scale, thumb_h likewise: thumbnail
     * pixel (y, x) reads tile pixel (min(y scale, th - 1), min(x scale, tw - 1)).  ochip_ortho_tile_thumb_dims: dims3 =
     * {scale, thumb_w, thumb_h} of a tw x th tile (each 1..4096); needs no device.
     * pass OCHIP_TILE_PASS_LAYERS: pixels = bgra [L][rows][cols][4] and weight [L][rows][cols] as ochip_ortho_layers writes
     * them (num_layers L in 1..8).  Over the layers in ascending order, from best = -1 and colour 0: a sample with alpha > 0
     * and weight > best (a float compare: a NaN never wins, an equal weight keeps the lower layer) sets best and the colour.
     * The pixel is (B, G, R, 255) when best >= 0, else the background (0, 0, 0, 51).
     * pass OCHIP_TILE_PASS_BLEND: pixels = rgba [rows][cols][4] as ochip_ortho_blend writes it (weight is not read, num_layers
     * still 1..8): alpha > 0 gives (rgba[2], rgba[1], rgba[0], 255), else (0, 0, 0, 0).
     * thumbs_out (host): per tile, in tile order, a slot of min(T, 128)^2 BGRA pixels; the thumbnail lies densely at the
     * slot's start, thumb_h rows of thumb_w, the rest of the slot is zero.
     * ochip_ortho_tile_thumbs is synchronous; pixels and weight are device pointers of this context's GPU when on_device,
     * else host.  ctx == NULL: the CPU route over host inputs (the message then in ochip_last_error(NULL)'s place).
     * The asynchronous form: enqueue launches the one kernel and the copy into a page-locked block of the context's pool on
     * the context's stream, records an event and returns (host inputs are uploaded and free on return); wait sleeps until
     * that job's event alone has passed and gives the block (bytes: tiles x slot bytes), valid until release, which hands
     * the blocks back to the pools (and waits first when nobody has).
     * Refused with OCHIP_EINVAL and a message, before anything is read: a pass that is neither, T or L out of range, cols <= 0,
     * rows <= 0, a NULL or unaligned array, pass 1 without weights, more than 2^31 - 1 tiles. */
#define OCHIP_TILE_PASS_LAYERS 1
#define OCHIP_TILE_PASS_BLEND 2
    typedef struct ochip_tile_thumbs_job ochip_tile_thumbs_job;
    int ochip_ortho_tile_thumb_dims(int32_t tw, int32_t th, int32_t *dims3);
    int ochip_ortho_tile_thumbs(ochip_ctx *ctx, int pass, int32_t cols, int64_t rows, int32_t tile_size, int32_t num_layers,
                                int on_device, const uint8_t *pixels, const float *weight, uint8_t *thumbs_out);
    int ochip_ortho_tile_thumbs_enqueue(ochip_ctx *ctx, int pass, int32_t cols, int64_t rows, int32_t tile_size, int32_t num_layers,
                                        int on_device, const uint8_t *pixels, const float *weight, ochip_tile_thumbs_job **out);
    int ochip_ortho_tile_thumbs_wait(ochip_tile_thumbs_job *job, const uint8_t **thumbs, uint64_t *bytes);
    void ochip_ortho_tile_thumbs_release(ochip_tile_thumbs_job *job);

    /* ---- the point cloud file (opencalibration_amd/csrc/xyz_export.hip, the rules in csrc/xyz_export.hpp; the reference's
     *      filterOutliers and toXYZ, src/io/saveXYZ.cpp) ----
     * The object holds one flat cloud, xyz [n][3] fp64 (n < 2^32; n = 0 is valid): create uploads it from host memory,
     * create_from_points copies the clouds of live ochip_mesh_points objects of the same context, in the given order, on
     * the device (the objects are only read and stay as they are).
     * bounds: bounds6 = {x first, x second, y first, y second, z first, z second}, filterOutliers' box - per axis the
     * number of points in every integer cell static_cast<int64_t>(v), exact for any span of cells, then the reference's walk
     * over the sorted (cell, count) rows.  A coordinate that is not finite or not below 2^63 in magnitude has no cell:
     * OCHIP_EINVAL.
     * text_size, then text: the bytes toXYZ writes, a line "x,y,z\n" per point inside the box in point order, every number
     * as `ostream << double` prints it ("%g").  bounds6 == NULL: no filter (the box {0, 0} x 3 means the same, as in the
     * reference).  text_size gives the file's size and its number of lines and keeps the lines on the device; text writes the
     * bytes of the last text_size into out (cap >= bytes; no terminator) and may be called again.  text before any
     * text_size is OCHIP_ESTATE.
     * OCHIP_EINVAL and a message, before anything is launched, for a NULL array, cap < bytes and a handle that create did
     * not return or destroy has taken (then the message is ochip_last_error(NULL)'s).  The calls wait for the context's
     * stream; destroy hands the device blocks back to the context's pool.
     * ochip_debug_format_g6: the device's number formatter alone - per value 16 bytes of text (zero-padded) and the length,
     * 0 where the integer formatter declines (|v| outside [1e-5, 2^63) and not 0) and the library formats on the host. */
    typedef struct ochip_xyz_export ochip_xyz_export;
    int ochip_xyz_export_create(ochip_ctx *ctx, const double *xyz, uint64_t n, ochip_xyz_export **out);
    int ochip_xyz_export_create_from_points(ochip_ctx *ctx, const ochip_mesh_points *const *clouds, uint64_t n_clouds,
                                            ochip_xyz_export **out);
    uint64_t ochip_xyz_export_size(const ochip_xyz_export *e); /* n; 0 for a handle that is not live */
    int ochip_xyz_export_bounds(ochip_xyz_export *e, int64_t *bounds6);
    int ochip_xyz_export_text_size(ochip_xyz_export *e, const int64_t *bounds6 /* or NULL */, uint64_t *bytes, uint64_t *kept);
    int ochip_xyz_export_text(ochip_xyz_export *e, char *out, uint64_t cap);
    void ochip_xyz_export_destroy(ochip_xyz_export *e);
    int ochip_debug_format_g6(ochip_ctx *ctx, const double *values, uint64_t n, char *text16 /* [n][16] */, uint8_t *len /* [n] */);

    /* ---- the textured OBJ's JPEG texture (opencalibration_amd/csrc/jpeg_encode.hip, the rules in csrc/jpeg_encode.hpp; the
     *      reference's cv::imwrite(jpg_path, texture), src/ortho/ortho.cpp:2096-2123) ----
     * Baseline JPEG, YCbCr 4:2:0, the Annex K tables scaled by quality (1..100; cv::imwrite's default is 95), no restart
     * intervals: the bytes libjpeg-turbo writes for these settings.  An encoder belongs to one raster of width x height
     * (each 1..65500) on one context.  feed takes rows [row0, row0 + rows) as pixels of pixel_stride 3 or 4 bytes, channels
     * 0, 1, 2 = R, G, B: a device pointer on the context's device (on_device) or host memory, which goes through a
     * page-locked block of the context's pool.  Bands ascend and are contiguous from row 0 and have any row count; the
     * rows behind the last complete 16-row MCU row, 15 at most, stay on the device and precede the next feed.  A feed
     * enqueues on the context's stream and returns; it waits - for the oldest pass alone - only when four passes (of up to
     * 32 768 MCUs each) have not been read, and a host band waits for the feed before.  A device band stays the caller's to
     * keep alive until the next collect or finish.  pending: the bytes collect would deliver now.  collect: *n bytes of the file into buf - the header first,
     * after a feed the complete bytes so far, after finish the rest with EOI - and buf == NULL only reports *n; cap < *n
     * is refused and the bytes stay.  finish: after the raster's last row.
     * OCHIP_EINVAL and a message, before anything is launched, for a side or quality out of range, a NULL band, a stride
     * that is neither, a gap, an overlap, rows beyond the raster, cap too small and a handle that create did not return or
     * destroy has taken (then the message is ochip_last_error(NULL)'s); OCHIP_ESTATE for a feed after finish and a finish
     * before the last row or a second one. */
    typedef struct ochip_jpeg ochip_jpeg;
    int ochip_jpeg_create(ochip_ctx *ctx, int64_t width, int64_t height, int quality, ochip_jpeg **out);
    int ochip_jpeg_feed(ochip_jpeg *e, int64_t row0, int64_t rows, const void *pixels, int pixel_stride, int on_device);
    int64_t ochip_jpeg_pending(ochip_jpeg *e);
    int ochip_jpeg_collect(ochip_jpeg *e, uint8_t *buf /* or NULL */, uint64_t cap, uint64_t *n);
    int ochip_jpeg_finish(ochip_jpeg *e);
    void ochip_jpeg_destroy(ochip_jpeg *e);

    /* ---- baseline JPEG decoding of the load stage (opencalibration_amd/csrc/jpeg_decode.hip, the rules in
     *      csrc/jpeg_decode.hpp; the reference's cv::imread(path), src/extract/extract_image.cpp:18-21; DESIGN.md section
     *      4.18) ----
     * The pixels libjpeg-turbo's default decode gives (islow inverse DCT, triangle chroma upsampling, B G R order) with the
     * EXIF orientation applied, for a batch of files per call.  The host reads the headers only; the entropy-coded bytes go
     * to the device once and every step from them to the pixels is a kernel on the context's stream.  Taken: SOF0 / SOF1
     * with Huffman coding, 8 bits, one component or Y Cb Cr with luma 1x1, 2x1 or 2x2, one interleaved scan, any DHT, 8-bit
     * DQT, DRI / RSTn.  status per file: OCHIP_JPEG_OK, OCHIP_JPEG_UNSUPPORTED (progressive, arithmetic, 12 bits, four
     * components, other samplings, several scans, 16-bit DQT, RGB files) or OCHIP_JPEG_CORRUPT (truncated, not decodable:
     * no picture is written where libjpeg would warn and deliver a partly grey one).
     * create: subsequence_bits is the length of the pieces the scan is decoded in, a multiple of 32 from 32 on; 0: the
     * default.  decode: files[i] / sizes[i] are host memory; out is a device pointer of out_cap bytes on the context's
     * device; image i goes to out + offsets[i] as [height][width][3] uint8 (offsets == NULL: back to back), width and height
     * as info[i] reports them: with apply_orientation the oriented ones, and info[i].offset says where it went.  A file
     * whose status is not OK writes nothing and leaves its neighbours alone; one whose headers are refused takes no room,
     * one whose scan turns out corrupt keeps the room its headers asked for.  At most 65 535 files a call.  A header that
     * promises more blocks than its scan has bits for two each is corrupt; bytes of a scan behind its last block are not
     * read.  rounds (or NULL): [0] the launches of the synchronisation kernel, [1] the most rounds a
     * workgroup ran inside one.  The call returns when the pixels are there.
     * OCHIP_EINVAL and a message, before anything is launched, for a NULL or dead handle (then the message is
     * ochip_last_error(NULL)'s), subsequence_bits out of range, NULL arguments and an output that is too small. */
#define OCHIP_JPEG_OK 0
#define OCHIP_JPEG_UNSUPPORTED 1
#define OCHIP_JPEG_CORRUPT 2
    typedef struct ochip_jpeg_file_info
    {
        int32_t width, height;   /* as decoded: oriented when the orientation was applied */
        int32_t components;      /* 1 or 3 */
        int32_t h_samp, v_samp;  /* luma sampling factors */
        int32_t restart_interval;
        int32_t orientation;     /* EXIF tag 0x0112, 1 .. 8; 1 when absent */
        int32_t status;
        uint64_t offset;         /* decode: the image's first byte in out; ~0: its headers were refused, it took no room */
    } ochip_jpeg_file_info;
    typedef struct ochip_jpeg_decoder ochip_jpeg_decoder;
    int ochip_jpeg_decoder_create(ochip_ctx *ctx, int subsequence_bits, ochip_jpeg_decoder **out);
    int ochip_jpeg_decoder_decode(ochip_jpeg_decoder *d, int64_t n, const uint8_t *const *files, const uint64_t *sizes,
                                  int apply_orientation, void *out, uint64_t out_cap, const uint64_t *offsets /* or NULL */,
                                  ochip_jpeg_file_info *info /* [n] */, int32_t *rounds /* [2] or NULL */);
    void ochip_jpeg_decoder_destroy(ochip_jpeg_decoder *d);

    /* ---- the tiles of the tiled DEFLATE GeoTIFFs (opencalibration_amd/csrc/geotiff.hip, the rules in
     *      csrc/deflate_rules.hpp; the reference's createGeoTIFF / createDSMGeoTIFF, src/ortho/ortho.cpp:655-708 and
     *      :745-791) ----
     * A writer belongs to one raster of width x height pixels of 4 bytes: kind 0 R G B A bytes, kind 1 one float32.  It
     * turns the raster, fed band by band on the context's stream, into the zlib streams of its 512 x 512 tiles: horizontal
     * predictor, one deflate block per 16 384 bytes, or the stored form when that is not larger; no stream exceeds
     * 1 048 667 bytes.  The TIFF structure around the streams is the caller's (host.GeoTiffWriter).
     * feed: bands ascend from row 0 without gaps, of any row count; rows behind the last complete tile row are kept on the
     *   device (at most 511), a tile row is encoded once complete, the last at the raster's end.  on_device: pixels is a
     *   device pointer whose producer has run, or is enqueued on the context's stream; the call does not wait for what it
     *   enqueues.  Otherwise a host pointer that may be reused on return.
     * payloads: n predicted payloads of 1 048 576 bytes (host memory) straight into the encoder, n at most the raster's
     *   tiles across; their streams are collected like a tile row's.
     * collect: the streams of the tiles complete so far, in tile order, back to back in buf, counts[k] the bytes of the
     *   k-th (0: an all-zero RGBA tile of a sparse writer, nothing is kept for it).  buf and counts NULL: only *bytes and
     *   *tiles, what a collect would need now.  Waits for the encoded tile rows alone.
     * finish: every row has been fed.  OCHIP_EINVAL and a message, before anything is launched, for a kind or side out of
     * range, a NULL band, a gap, an overlap, rows beyond the raster, too little room, and a handle that create did not
     * return or destroy has taken; OCHIP_ESTATE for a feed after finish and a finish before the last row. */
#define OCHIP_GEOTIFF_RGBA8 0
#define OCHIP_GEOTIFF_FLOAT32 1
#define OCHIP_GEOTIFF_MAX_SIDE 1048576
    typedef struct ochip_geotiff ochip_geotiff;
    int ochip_geotiff_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, int sparse, ochip_geotiff **out);
    int ochip_geotiff_feed(ochip_geotiff *e, int64_t row0, int64_t rows, const void *pixels, int on_device);
    int ochip_geotiff_payloads(ochip_geotiff *e, const uint8_t *payloads, int64_t n);
    int ochip_geotiff_collect(ochip_geotiff *e, uint8_t *buf /* or NULL */, uint64_t cap, uint64_t *bytes,
                              uint64_t *counts /* or NULL */, uint64_t max_tiles, uint64_t *tiles);
    int ochip_geotiff_finish(ochip_geotiff *e);
    void ochip_geotiff_destroy(ochip_geotiff *e);

    /* The layers and cameras rasters between the layer pass and the blend (the reference's createMultiBandGeoTIFF,
     * src/ortho/ortho.cpp:969-1008): a writer as above whose pixel holds num_layers layers, 1 or 2.
     * kind 2: B G R A bytes per layer, a pixel of 4 num_layers bytes, the predictor over bytes; kind 3: the low and the
     * high 32-bit word of each layer's 64-bit node id, a pixel of 8 num_layers bytes, the predictor over 32-bit words.
     * feed takes a band as ortho_layers leaves it, layer-major: [num_layers][rows][width] of 4 bytes, respectively of one
     * little-endian uint64; the tiles are pixel-interleaved, [row][col][layer][sample].  A tile's payload has
     * 262 144 x the pixel's bytes, which is also what payloads takes, and no stream exceeds that plus 5 bytes per
     * 65 535 and 6.  sparse leaves out an all-zero tile of either kind.  Everything else is the writer above; the
     * refusals name ochip_geotiff_create_layered. */
#define OCHIP_GEOTIFF_LAYERS8 2
#define OCHIP_GEOTIFF_CAMERAS32 3
#define OCHIP_GEOTIFF_MAX_LAYERS 2
    int ochip_geotiff_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int sparse,
                                     ochip_geotiff **out);

    /* ---- PNG files of thumbnails and previews (opencalibration_amd/csrc/png.hip, the rules in csrc/png_rules.hpp; the
     *      reference's cv::imencode(".png") of a node's thumbnail, src/io/serialize_MeasurementGraph.cpp:260-267,
     *      src/ortho/thumbnail_encode.hpp, and thumb.png) ----
     * A batch of n images (at most 65 535) of mixed sizes to n PNG files per call: 8 bits per sample, 1, 3 or 4 channels
     * (colour types 0, 2, 6), sides of 1 .. 65 535, non-interlaced, one IDAT.  pixels: [height][width][channels] bytes
     * without padding; swap_rb exchanges channels 0 and 2 (B G R (A) arrays) before anything else.  on_device: every
     * pixels is a device pointer on the context's device whose producer has finished; otherwise host memory.  Every row
     * takes the filter with the smallest sum of min(v, 256 - v), every 16 384 payload bytes one deflate block, and an image
     * whose stream would not shrink is stored: file i has at most 2 + F + 5 ceil(F / 65535) + 4 + 57 bytes, F = height (1 +
     * width channels).  out (host, out_cap bytes): the files back to back, file i at offsets[i] .. offsets[i + 1]; with
     * base64 their RFC 4648 text instead (padded, no line breaks).  The call returns when out is written.
     * OCHIP_EINVAL and a message, before anything is launched: a handle that create did not return or destroy has taken
     * (the message is ochip_last_error(NULL)'s), NULL arrays, n out of range, a size or channel count out of range or a
     * payload from 2^31 bytes on (one refused image refuses the call), out_cap below the sum of the files' bounds. */
    typedef struct ochip_png_image
    {
        const void *pixels;
        int32_t width, height, channels, swap_rb;
    } ochip_png_image;
    typedef struct ochip_png_encoder ochip_png_encoder;
    int ochip_png_encoder_create(ochip_ctx *ctx, ochip_png_encoder **out);
    int ochip_png_encoder_encode(ochip_png_encoder *e, int64_t n, const ochip_png_image *images, int on_device, int base64,
                                 uint8_t *out, uint64_t out_cap, uint64_t *offsets /* [n + 1] */);
    void ochip_png_encoder_destroy(ochip_png_encoder *e);

    /* ---- reading tiled DEFLATE GeoTIFFs: inflate, un-predict, raster (opencalibration_amd/csrc/geotiff_read.hip, the
     *      rules in csrc/inflate_rules.hpp; the reference reads orthomosaic.tif and dsm.tif through GDAL,
     *      src/ortho/ortho.cpp:2052-2123 and :1735-1756) ----
     * A reader belongs to a sample layout (samples 1, 3 or 4 of 8 bits, or is_float with one float32), a raster size, a
     * tile size (sides multiples of 16, a payload of at most 4 MiB) and a predictor (1 or 2).  The TIFF structure around
     * the streams is the caller's (host.GeoTiffReader).  scratch_budget: the device bytes (streams plus payloads) one
     * launch may take, 0 for the default of 1.5 GiB; a call's streams go through as many launches as that needs, a launch
     * at least one stream.  All work runs on the context's stream.
     * inflate: n zlib streams (at most 65 535), stream i at streams[offsets[i] .. offsets[i + 1]), each of expect[i] bytes
     * (at most 2^30), into out (host): payload i begins at the sum of the expects before it, each rounded up to 16
     * (out_cap: at least where the last payload ends).
     * status[i]: OCHIP_INFLATE_OK only for a stream that gave exactly expect[i] bytes, ended with a BFINAL block, whose
     * Adler-32 matched and that has nothing behind it; bytes[i]: what it produced.  A stream that is not OK touches
     * nothing outside its own payload.
     * read: the streams of the tiles of the tile rows that cover raster rows [row0, row0 + rows), in tile order (n is
     * their number; an empty stream is a sparse tile: zeros), un-predicted and placed into raster - rows x width pixels,
     * host memory or, with on_device, device memory of the context's device.  *bad_tile: -1, or the first tile (an index
     * into the call's streams) whose stream was not OK; the raster's contents are then unspecified.  The call returns
     * when raster is written.
     * OCHIP_EINVAL and a message, before anything is launched: a handle that create did not return or destroy has taken
     * (the message is ochip_last_error(NULL)'s), NULL arrays, n out of range or not the window's tile count, offsets
     * that descend, an expect beyond 2^30, out_cap too small, a window outside the raster. */
#define OCHIP_INFLATE_OK 0
#define OCHIP_INFLATE_CORRUPT 1
#define OCHIP_INFLATE_MAX_STREAMS 65535
    typedef struct ochip_geotiff_reader ochip_geotiff_reader;
    int ochip_geotiff_reader_create(ochip_ctx *ctx, int samples, int is_float, int64_t width, int64_t height, int tile_w,
                                    int tile_h, int predictor, uint64_t scratch_budget, ochip_geotiff_reader **out);
    /* The reader of a layers (kind OCHIP_GEOTIFF_LAYERS8) or cameras (OCHIP_GEOTIFF_CAMERAS32) raster of num_layers layers,
     * 1 or 2: the tiles are pixel-interleaved, 4 num_layers bytes or 2 num_layers 32-bit words a
     * pixel, Predictor 2 at that stride over bytes respectively words; read places layer-major, as ortho_blend takes its
     * layers: [num_layers][rows][width] of 4 bytes B G R A, respectively of one little-endian uint64, in host or device
     * memory.  A tile without a stream is a sparse one and reads as zeros.  Everything else is the reader above. */
    int ochip_geotiff_reader_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int tile_w,
                                            int tile_h, int predictor, uint64_t scratch_budget, ochip_geotiff_reader **out);
    int ochip_geotiff_reader_inflate(ochip_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets /* [n + 1] */,
                                     const uint64_t *expect /* [n] */, uint8_t *out, uint64_t out_cap, int32_t *status /* [n] */,
                                     uint64_t *bytes /* [n] */);
    int ochip_geotiff_reader_read(ochip_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets /* [n + 1] */,
                                  int64_t row0, int64_t rows, void *raster, int on_device, int64_t *bad_tile);
    int64_t ochip_geotiff_reader_launches(ochip_geotiff_reader *r); /* the inflate launches so far, -1 for a dead handle */
    void ochip_geotiff_reader_destroy(ochip_geotiff_reader *r);

#ifdef __cplusplus
}
#endif
#endif /* OCHIP_H */
