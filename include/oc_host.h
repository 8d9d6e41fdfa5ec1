/* oc_host.h — C driver API of liboc_host.so, the C++17 host side of the MI355X hot path.
 *
 * liboc_host.so holds the host code that sits above libochip.so (include/ochip.h): the reference's
 * stage classes and value types re-stated for flat-array device calls (opencalibration_amd/csrc/host).
 * A C++ application links the classes directly; this flat API exists so the same code can be driven
 * from Python (tests/, bench.py) without a C++ test harness.
 */
#ifndef OC_HOST_H
#define OC_HOST_H

#include <stddef.h>
#include <stdint.h>

#include "ochip.h"

#ifdef __cplusplus
extern "C"
{
#endif

    /* spatially_subsample_feature_indices (src/match/match_features.cpp:8-52); out sized >= n */
    size_t och_subsample(const double *loc, const float *strength, size_t n, double spacing, size_t count,
                         uint64_t *out);

    /* ratio test + remap + std::sort of match_features_subset (src/match/match_features.cpp:94-101)
     * over the device kernel's raw output for one pair; outputs sized >= n1 */
    size_t och_matches_from_device(const ochip_match *raw, const uint64_t *idx1, size_t n1, const uint64_t *idx2,
                                   size_t n2, uint64_t *out_i1, uint64_t *out_i2, double *out_dist);

    /* ---- MeasurementGraph + LinkStage driver (opencalibration_amd/csrc/host/link_stage.hpp) ---- */
    typedef struct och_graph och_graph;
    och_graph *och_graph_create(void);
    void och_graph_destroy(och_graph *g);
    const char *och_last_error(const och_graph *g);
    /* m10 = {f, ppx, ppy, k1, k2, k3, p1, p2, pixels_cols, pixels_rows}; returns the model handle */
    uint32_t och_graph_add_model(och_graph *g, const double *m10);
    /* one image = what extract_features hands to the link stage; returns the node id */
    uint64_t och_graph_add_image(och_graph *g, const double *loc, const float *strength, const uint64_t *desc, size_t n,
                                 size_t num_sparse, uint32_t model, const double *position3);
    /* graph.addEdge(relations, source, dest) from flat arrays (a deserialised graph, a test): inl_px4 n x {pixel_1, pixel_2},
     * inl_idx3 n x {feature_index_1, feature_index_2, match_index}; matches: match_idx2 (may be NULL), match_dist (may be
     * NULL); poses32: 4 x {q xyzw, t xyz, score} or NULL.  Returns the edge id (0 + och_last_error on an unknown node). */
    uint64_t och_graph_add_edge(och_graph *g, uint64_t source_id, uint64_t dest_id, const double *H9, int is_homography,
                                size_t n_inliers, const double *inl_px4, const uint64_t *inl_idx3, size_t n_matches,
                                const uint64_t *match_idx2, const double *match_dist, const double *poses32);
    void och_graph_get_orientations(const och_graph *g, double *ori /* n_nodes x 4, node order */);
    /* work of the last link stage's match step: {directed pairs, descriptor distances needed = sum n1 * n2, subset features} */
    void och_link_match_work(const och_graph *g, double *out3);
    size_t och_graph_num_nodes(const och_graph *g);
    size_t och_graph_num_edges(const och_graph *g);
    void och_graph_node_ids(const och_graph *g, uint64_t *out);
    /* LinkStage::init + the batch runner + finalize; timers = 8 doubles {link_init, subsample, upload,
     * match_device, match_host, ransac_device, decompose_host, link_finalize} seconds */
    int och_link_stage_run(och_graph *g, ochip_ctx *ctx, const uint64_t *node_ids, size_t n, int keep_debug,
                           double *timers);
    size_t och_link_debug_count(const och_graph *g);
    void och_link_debug_pair(const och_graph *g, size_t p, uint64_t *ids2, uint64_t *n_matches, double *score,
                             uint32_t *iters3);
    void och_link_debug_matches(const och_graph *g, size_t p, uint64_t *i1, uint64_t *i2, double *dist, uint8_t *inl);
    void och_graph_edge_info(const och_graph *g, size_t e, uint64_t *ids2, uint64_t *counts2, double *H, double *poses);
    void och_graph_edge_inliers(const och_graph *g, size_t e, uint64_t *f1, uint64_t *f2, uint64_t *match_index,
                                double *px4);
    void och_graph_edge_match_distances(const och_graph *g, size_t e, double *out); /* relations.matches[i].distance */
    /* relations.matches of edge e: feature index pairs (n_matches x 2) and distances; relationType == HOMOGRAPHY */
    void och_graph_edge_matches(const och_graph *g, size_t e, uint64_t *idx2, double *dist, int *is_homography);
    void och_graph_set_orientations(och_graph *g, const double *ori /* n_nodes x 4, node order */);

    /* ---- extract (opencalibration_amd/csrc/host/extract_features.hpp): extract_features(cv::Mat) of
     *      src/extract/extract_features.cpp:11-88 for a batch of equally sized BGR images ------------------ */
    /* Per image up to max_out features at stride max_out: loc (x, y in full-resolution pixels), strength, desc
     * (8 u64); counts[i] features of image i, the first num_sparse[i] of which passed the 8 px NMS.
     * images_on_device != 0: images_bgr is a device pointer (images already resident in HBM). */
    int och_extract_features_batch(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                                   uint32_t max_keypoints, uint32_t max_out, double *loc, float *strength,
                                   uint64_t *desc, uint32_t *counts, uint32_t *num_sparse, int images_on_device);
    const char *och_extract_last_error(void);
    /* Host pieces of the link step, callable without a device (tests): homography_model::decompose on the inlier rays
     * (n x {measurement1, measurement2}; poses 4 x {q xyzw, t xyz, score}; returns can_decompose) and image_to_3d. */
    int och_homography_decompose(const double *H9, const double *m1m2, size_t n, double *poses);
    void och_image_to_3d(const double *px, size_t n, const double *model10, double *rays);
    /* ransac<fundamental_matrix_model> (model 0) / ransac<essential_matrix_model> (model 1) on the device
     * (ochip_ransac_epipolar_batch) for one set of correspondences: rays6 n x {measurement1, measurement2}, quality n or
     * NULL (PROSAC), threshold = the model's inlier_threshold (0.01).  M9: the matrix (row-major), inliers: n flags,
     * counts3: {iterations, improvements, inliers}.  Returns ransac()'s score, NAN on a device error. */
    double och_ransac_epipolar(ochip_ctx *ctx, int model, const double *rays6, const double *quality, size_t n, double threshold,
                               double *M9, uint8_t *inliers, uint32_t *counts3);
    /* The host tail of extract_features alone (extract_features.cpp:38-87), no device involved: kp6 rows
     * {x, y, size, angle, response, level} in cv::AKAZE's order -> loc / strength / desc as above; returns the count. */
    size_t och_extract_tail(const float *kp6, const uint64_t *desc, uint32_t n, double scale, double *loc, float *strength,
                            uint64_t *desc_out, uint64_t *num_sparse);
    /* The same tail for ONE image on the lists the device prepared (ochip_akaze_features / ochip_feature_lists_from_keypoints,
     * include/ochip.h: records, response, slot, num_sparse of that image): the host's part is the std::sort order, the copy
     * and the re-seating inside groups of equal responses; conflict != 0 runs the suppression here as well. */
    size_t och_extract_tail_prepared(const uint8_t *records, const float *response, const uint32_t *slot, uint32_t num_sparse_in,
                                     int conflict, uint32_t n, double scale, double *loc, float *strength, uint64_t *desc_out,
                                     uint64_t *num_sparse);
    /* Cumulative CPU seconds of that tail's phases, recorded while OCHIP_VERBOSE=extract is set: ordering, NMS, feature
     * records, total, and the number of images whose responses tied (they take std::sort's route). */
    void och_extract_tail_profile(double *out5);
    /* The strength order of that tail alone: the permutation of 0..n-1 that std::sort by descending response produces
     * (extract_features.cpp:55-56; ties keep whatever order libstdc++'s introsort leaves them in).  use_std != 0 calls
     * std::sort itself, 0 the library's own implementation of the same sequence of moves (host/sort_like_std.hpp). */
    void och_sort_by_response(const float *response, uint32_t n, uint32_t *order_out, int use_std);
    /* The load stage's job for a batch of equally sized images (src/pipeline/load_stage.cpp:43-110: extract_features,
     * then one graph node per image): extract on the device in chunks (host tail of chunk k overlapped with the device
     * work of chunk k + 1), then addNode in image order.  positions: n x 3; node_ids_out: n (may be NULL);
     * totals2 (may be NULL) receives {features, sparse features} summed over the images.  Returns 0, or -1 with the
     * message in och_last_error(g). */
    int och_graph_load_images(och_graph *g, ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width,
                              int height, uint32_t max_keypoints, int images_on_device, uint32_t model,
                              const double *positions, uint64_t *node_ids_out, double *totals2);

    /* Load and link overlapped, the way the reference's pipeline overlaps the stages of consecutive image batches
     * (src/pipeline/pipeline.cpp:522-570): nodes are created first (positions, optional orientations n x 4, model),
     * extraction streams chunk by chunk, and every range of links whose images all have their features is linked on
     * its own device context while later chunks are still being extracted.  The graph is the one och_graph_load_images
     * followed by och_link_stage_run produces.  link_timers8 as och_link_stage_run; stage_seconds2 = {seconds until
     * the last features were final, seconds until the graph was linked}.  Any output pointer may be NULL. */
    int och_graph_load_link_images(och_graph *g, ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width,
                                   int height, uint32_t max_keypoints, int images_on_device, uint32_t model,
                                   const double *positions, const double *orientations, uint64_t *node_ids_out,
                                   double *totals2, double *link_timers8, double *stage_seconds2);

    /* ---- INITIAL_PROCESSING with the reference's software pipelining (Pipeline::Impl::initial_processing,
     *      src/pipeline/pipeline.cpp:522-570; opencalibration_amd/csrc/host/initial_processing.cpp): one step loads (extracts)
     *      the batch it is given, links the batch of the step before against everything loaded before it, and relaxes the
     *      batch of two steps before as ONE group with two rings of context cameras ({ORIENTATION, GROUND_PLANE},
     *      disable_parallelism, :545-546) - the three stages' runners side by side (:548-556), finalized in the reference's
     *      order (:558-560).  Images arrive WITHOUT orientations (types/image.hpp:31); the relax stage initialises them
     *      (src/relax/relax.cpp:44-87).  n_images == 0 drains the pipeline: call until och_initial_processing_pending() is 0.
     *      sequential != 0: the three stages one after the other on the calling thread (the test route: the same graph).
     *      stats16 (may be NULL): seconds of the step, its init, its runners, its finalize; seconds of the load, link and
     *      relax runners; features and sparse features extracted; images linked and relaxed in this step; the relax
     *      stage's solves, LM iterations, host set-up seconds, device seconds; images handed to the next step's relax. */
    typedef struct och_initial_processing och_initial_processing;
    och_initial_processing *och_initial_processing_create(och_graph *g, ochip_ctx *ctx);
    void och_initial_processing_destroy(och_initial_processing *ip);
    int och_initial_processing_pending(const och_initial_processing *ip);
    int och_initial_processing_step(och_initial_processing *ip, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                                    uint32_t max_keypoints, int images_on_device, uint32_t model, const double *positions,
                                    int sequential, uint64_t *node_ids_out, double *stats16);

    /* ---- ONE survey's load + link stages over `world` ranks, one process per GPU (opencalibration_amd/csrc/host/shard_link.cpp).
     *      The reference parallelises one survey over its workers: one load closure per image
     *      (src/pipeline/load_stage.cpp:36-50), one link closure per directed pair (src/pipeline/link_stage.cpp:75-112),
     *      run by the worker loop of src/pipeline/pipeline.cpp:42-49.  Rank r extracts a contiguous block of the images and
     *      links the directed pairs owned by that block; pairs are independent units, no collective runs inside a stage.
     *      Two exchanges between the calls are the caller's (an all-gather over RCCL, or any transport):
     *        och_shard_load_link_local  extract the block, link the pairs whose two images are both in it (streamed)
     *        och_shard_subsets_export   -> all-gather -> och_shard_subsets_import (once per other rank's buffer)
     *        och_shard_link_remote      the rank's pairs that touch another block
     *        och_shard_edges_export     -> all-gather -> och_shard_edges_import (once per other rank's buffer)
     *        och_shard_finalize         LinkStage::finalize: the same edge list, ids included, on every rank
     *      Buffers handed to the import calls must be 8-byte aligned.  The graph must hold the camera model and no nodes
     *      of this survey yet; afterwards every rank's graph has all nodes and all edges, and the feature lists of the
     *      rank's own block. ------------------------------------------------------------------------------------------- */
    typedef struct och_shard och_shard;
    void och_shard_block(uint32_t n_images, uint32_t rank, uint32_t world, uint32_t *first, uint32_t *count);
    och_shard *och_shard_begin(och_graph *g, ochip_ctx *ctx, uint32_t n_images, uint32_t model, const double *positions,
                               const double *orientations, uint32_t rank, uint32_t world, uint64_t *node_ids_out);
    void och_shard_destroy(och_shard *s);
    /* counts4: images of the block, pairs linked inside the block, pairs that touch another block, images of other
     * blocks those pairs need descriptors of */
    void och_shard_counts(const och_shard *s, uint64_t *counts4);
    /* images_bgr: the BLOCK's images (host or device pointer) */
    int och_shard_load_link_local(och_shard *s, const uint8_t *images_bgr, int width, int height, uint32_t max_keypoints,
                                  int images_on_device);
    /* *buf stays valid until the next export on this shard */
    int och_shard_subsets_export(och_shard *s, const void **buf, uint64_t *bytes);
    int och_shard_subsets_import(och_shard *s, const void *buf, uint64_t bytes);
    int och_shard_link_remote(och_shard *s);
    int och_shard_edges_export(och_shard *s, const void **buf, uint64_t *bytes);
    int och_shard_edges_import(och_shard *s, const void *buf, uint64_t bytes);
    /* totals2: {features, sparse features} of the block; link_timers8 as och_link_stage_run; seconds9: extract, block
     * linked, subsets export, subsets import, remote links, edges export, edges import, finalize, whole stage */
    int och_shard_finalize(och_shard *s, double *totals2, double *link_timers8, double *seconds9);

    /* ---- relax (opencalibration_amd/csrc/host/relax.hpp): relax(graph, nodes, cam_models, edges,
     *      {ORIENTATION, GROUND_PLANE}, {}) of src/relax/relax.cpp:122-134 ------------------------------ */
    /* Stand-alone problem from flat arrays.  graph: n_nodes x {pos3, ori4 xyzw (may be NaN)} + one shared
     * camera model; poses: node indices + orientations (in/out, NaN = uninitialised); edges: src/dst node
     * index, H (9), is_homography, inlier offsets, per inlier {px1 xy, px2 xy} + match_index, optional
     * per-edge match distances; opt_edges: whitelist order.  plane_out: 3 corners x (x,y,z).
     * summary_out (8): solves, iterations_total, last_iterations, last_initial_cost, last_final_cost,
     * last_residual_blocks, host setup seconds, device seconds.  Returns 0 or -1. */
    int och_relax_ground_plane(ochip_ctx *ctx, size_t n_nodes, const double *node_pos, const double *node_ori,
                               const double *model10, size_t n_poses, const uint64_t *pose_node, double *pose_ori,
                               size_t n_edges, const uint64_t *edge_src, const uint64_t *edge_dst,
                               const double *edge_H, const uint8_t *edge_is_homography, const uint64_t *inl_off,
                               const double *inl_px, const uint64_t *inl_match_index, const uint64_t *dist_off,
                               const double *dist, size_t n_opt_edges, const uint64_t *opt_edges, double *plane_out,
                               double *summary_out);
    const char *och_relax_last_error(void);
    /* Test hook.  on = 1: every ground-plane relax set-up from now on repeats gridFilterMatchesPerImage and the block
     * assembly (relax_problem.cpp:234-309, :388-560) with the host code and fails unless the blocks the device built
     * (ochip_plane_setup_*, include/ochip.h) equal them bit for bit; 0: off (default); < 0: unchanged.  Returns the
     * number of set-ups compared so far. */
    int och_debug_relax_setup_check(int on);
    /* Every node of a linked graph as one group, every edge whitelisted (the single-group global relax,
     * src/pipeline/pipeline.cpp:653-655).  ori_inout: n_nodes x 4 in node order. */
    int och_graph_relax_ground_plane(och_graph *g, ochip_ctx *ctx, double *ori_inout, double *plane_out,
                                     double *summary_out);
    /* The same relax with the residual-block evaluation sharded over `world` ranks (one process per GPU, each holding
     * the same graph); `exchange` all-gathers the per-pair records, see ochip_relax_set_shard in ochip.h.  Results
     * are bit-identical to the unsharded call on every rank. */
    int och_graph_relax_ground_plane_sharded(och_graph *g, ochip_ctx *ctx, double *ori_inout, double *plane_out,
                                             double *summary_out, uint32_t rank, uint32_t world,
                                             ochip_relax_exchange_fn exchange, void *user);

    /* ---- relax, every flavour the device runs (opencalibration_amd/csrc/host/relax_mesh.hpp):
     *      relax(graph, nodes, cam_models, edges, config, previousSurfaces) of src/relax/relax.cpp:118-134 with
     *      config.options = bits of include/opencalibration/types/relax_options.hpp:9-33 in enum order (ORIENTATION = 1,
     *      POSITION = 2, GROUND_PLANE = 4, GROUND_MESH = 8, ..., MINIMAL_MESH = 4096). ------------------------------ */
    typedef struct och_surface och_surface; /* surface_model: mesh (vertices, edges with their opposite vertices) + cloud */
    och_surface *och_surface_create(void);
    void och_surface_destroy(och_surface *s);
    void och_surface_counts(const och_surface *s, size_t *n_vertices, size_t *n_edges, size_t *n_cloud);
    /* vertices n x 3; edges n x 5 {source, dest, border, opposite 0, opposite 1} (UINT64_MAX = none); cloud n x 3 */
    void och_surface_get(const och_surface *s, double *vertices, uint64_t *edges5, double *cloud);
    void och_surface_set(och_surface *s, size_t n_vertices, const double *vertices, size_t n_edges, const uint64_t *edges5,
                         size_t n_cloud, const double *cloud);
    /* new heights for the mesh vertices (n_vertices doubles); topology and the order of the mesh's containers stay */
    void och_surface_set_heights(och_surface *s, const double *z);
    /* rebuildMesh / buildMinimalMesh (src/surface/expand_mesh.cpp) from camera positions and an optional previous surface */
    void och_rebuild_mesh(const double *cam_xyz, size_t n, const och_surface *previous, int minimal, och_surface *out);
    /* Stand-alone problem from flat arrays, as och_relax_ground_plane plus what the mesh flavour reads: per node its
     * feature locations (feat_off n_nodes + 1, feat_xy), per inlier the two feature indices (inl_feat n x 2).
     * previous / surface_out may be NULL.  summary_out (12): solves, iterations_total, last_iterations,
     * last_initial_cost, last_final_cost, last_residual_blocks, host setup seconds, device seconds, track blocks,
     * 2-ray blocks, mesh vertices, unknowns of the last solve.  model10_inout (may be NULL): the caller's cam_models entry of
     * the shared camera model, read before and written after the relax (the intrinsics flavours change it). */
    int och_relax(ochip_ctx *ctx, size_t n_nodes, const double *node_pos, const double *node_ori, const double *model10,
                  const uint64_t *feat_off, const double *feat_xy, size_t n_poses, const uint64_t *pose_node,
                  double *pose_ori, size_t n_edges, const uint64_t *edge_src, const uint64_t *edge_dst, const double *edge_H,
                  const uint8_t *edge_is_homography, const uint64_t *inl_off, const double *inl_px,
                  const uint64_t *inl_feat, const uint64_t *inl_match_index, const uint64_t *dist_off, const double *dist,
                  size_t n_opt_edges, const uint64_t *opt_edges, uint32_t options, double grid_fraction,
                  const och_surface *previous, och_surface *surface_out, double *summary_out, double *model10_inout);
    /* och_relax with what the two flavours the reference only reaches from its tests need: edge_poses32 (may be NULL) =
     * per edge the four homography decompositions 4 x {q xyzw, t xyz, score} of camera_relations::relative_poses - the
     * relative-orientation flavour (no GROUND_*, no POINTS_3D option: runRelativeOrientation, src/relax/relax.cpp:14-42)
     * reads them; points_mode >= 0 with POINTS_3D runs TestRelaxProblem (test/test_relax.cpp:470-483) instead of the driver:
     * setup3dPointProblem, then nothing (0), solve (1) or relaxObservedModelOnly (2); points_before / points_after
     * (points_cap x 3, may be NULL) receive the tracks' 3-D points after the set-up and at the end, *n_points_out their
     * number.  points_mode < 0: exactly och_relax (POINTS_3D then runs runPoints, relax.cpp:103-115). */
    int och_relax_ex(ochip_ctx *ctx, size_t n_nodes, const double *node_pos, const double *node_ori, const double *model10,
                     const uint64_t *feat_off, const double *feat_xy, size_t n_poses, const uint64_t *pose_node,
                     double *pose_ori, size_t n_edges, const uint64_t *edge_src, const uint64_t *edge_dst, const double *edge_H,
                     const uint8_t *edge_is_homography, const uint64_t *inl_off, const double *inl_px,
                     const uint64_t *inl_feat, const uint64_t *inl_match_index, const uint64_t *dist_off, const double *dist,
                     size_t n_opt_edges, const uint64_t *opt_edges, uint32_t options, double grid_fraction,
                     const och_surface *previous, och_surface *surface_out, double *summary_out, double *model10_inout,
                     const double *edge_poses32, int points_mode, double *points_before, double *points_after,
                     size_t points_cap, size_t *n_points_out);
    /* Every node of a linked graph as one group, every edge whitelisted, any flavour.  ori_inout: n_nodes x 4. */
    int och_graph_relax(och_graph *g, ochip_ctx *ctx, double *ori_inout, uint32_t options, double grid_fraction,
                        const och_surface *previous, och_surface *surface_out, double *summary_out);

    /* The same with the evaluation of the residual blocks sharded over `world` ranks (one process per GPU, each holding the
     * same graph edges): the single global group of the reference's FINAL_GLOBAL_RELAX ({ORIENTATION, GROUND_MESH},
     * src/pipeline/pipeline.cpp:645-664) and the plane flavour alike; `exchange` as for
     * och_graph_relax_ground_plane_sharded.  Bit-identical to the unsharded call on every rank. */
    int och_graph_relax_sharded(och_graph *g, ochip_ctx *ctx, double *ori_inout, uint32_t options, double grid_fraction,
                                const och_surface *previous, och_surface *surface_out, double *summary_out, uint32_t rank,
                                uint32_t world, ochip_relax_exchange_fn exchange, void *user);

    /* RelaxStage (src/pipeline/relax_stage.cpp): init (partition into floor(n / 50) groups - 150 with free intrinsics -
     * by spectral clustering of the link graph, or one group with two rings of context cameras when disable_parallelism),
     * the groups' runners (concurrently, on sibling device contexts), finalize (write-back + merged surface).
     * node_ids may be NULL with relax_all != 0.  max_groups > 0: trim_groups(max_groups) before running.
     * group_of_node (n_nodes, may be NULL) receives for every node the group it is a primary node of (0 = largest) or -1.
     * summary_out as och_relax (sums over the groups), summary_out[12] = number of groups run. */
    int och_relax_stage_run(och_graph *g, ochip_ctx *ctx, const uint64_t *node_ids, size_t n_ids, int relax_all,
                            int disable_parallelism, uint32_t options, double grid_fraction, size_t max_groups,
                            const och_surface *previous, och_surface *surface_out, int64_t *group_of_node,
                            double *summary_out);
    /* The same stage in steps, for the groups of one survey over `world` ranks (one process per GPU, the same graph on every
     * rank): groups are independent during their solves (src/pipeline/relax_stage.cpp:95-111), rank r runs groups
     * r, r + world, ... of the largest-first list and nothing is exchanged inside a solve.  begin = init (+ trim_groups);
     * run_groups = this rank's runners; export -> all-gather -> import (once per other rank's buffer) moves the groups'
     * results (orientations, camera models, surfaces); end = finalize (write-back and mergeSurfaceModels - the
     * point-count-weighted vertex mean of src/surface/refine_mesh.cpp:931-1010 - over ALL groups in group order, so the
     * result is the single-process one) and destroys the handle.  och_relax_stage_run is begin + run_groups(0, 1) + end. */
    typedef struct och_relax_stage och_relax_stage;
    och_relax_stage *och_relax_stage_begin(och_graph *g, const uint64_t *node_ids, size_t n_ids, int relax_all,
                                           int disable_parallelism, uint32_t options, double grid_fraction, size_t max_groups,
                                           const och_surface *previous, int64_t *group_of_node);
    size_t och_relax_stage_num_groups(const och_relax_stage *st);
    int och_relax_stage_run_groups(och_relax_stage *st, ochip_ctx *ctx, uint32_t rank, uint32_t world);
    int och_relax_stage_export(och_relax_stage *st, uint32_t rank, uint32_t world, const void **buf, uint64_t *bytes);
    int och_relax_stage_import(och_relax_stage *st, const void *buf, uint64_t bytes);
    int och_relax_stage_end(och_relax_stage *st, och_surface *surface_out, double *summary_out);
    /* the partition alone (no device): group_of_node as above, position_in_group (may be NULL) the node's place in its
     * group's list; returns the number of groups */
    size_t och_relax_partition(const och_graph *g, size_t num_groups, int64_t *group_of_node, int64_t *position_in_group);
    /* convertModel (src/distort/invert_distortion.cpp:105-191): the inverse lens model fitted to a forward one (to_inverse),
     * or the forward model fitted to an inverse one; m10 as och_graph_add_model */
    void och_convert_model(const double *m10, int to_inverse, double *out10);
    /* mergeSurfaceModels of n surfaces (src/surface/refine_mesh.cpp:916-1016) */
    void och_merge_surfaces(const och_surface *const *surfaces, size_t n, och_surface *out);

    /* ---- after a relax changed a camera model: the write-back half of RelaxGroup::finalize
     *      (src/relax/relax_group.cpp:125-177).  och_graph_set_model replaces the intrinsics of model `model` (m10 as for
     *      och_graph_add_model; every image sharing the model sees the change, as with the reference's
     *      shared_ptr<CameraModel>); och_graph_refit_edges then re-fits EVERY edge of the graph on its previous inliers:
     *      correspondences from the current models, three rounds of fitInliers + evaluate on the device
     *      (ochip_refit_homography_batch), decomposition and inlier assembly on the host. */
    int och_graph_set_model(och_graph *g, uint32_t model, const double *m10);
    int och_graph_refit_edges(och_graph *g, ochip_ctx *ctx);

    /* ---- the reference's on-disk formats (opencalibration_amd/csrc/host/graph_io.hpp): the MeasurementGraph as
     *      graph.json (serialize / deserialize, src/io/serialize_MeasurementGraph.cpp:204-591,
     *      src/io/deserialize_MeasurementGraph.cpp:30-272), a surface mesh as ASCII PLY (src/io/serialize_MeshGraph.cpp,
     *      src/io/deserialize_MeshGraph.cpp) and the checkpoint directory (saveCheckpoint / loadCheckpoint /
     *      validateCheckpoint, src/io/checkpoint.cpp:155-337).  Loading REPLACES the handle's graph and model table;
     *      0 = ok, -1 + och_last_error(g) otherwise. ------------------------------------------------------------------ */
    char *och_graph_to_json(const och_graph *g, size_t *len); /* malloc'd, NUL-terminated: och_free */
    void och_free(void *p);
    int och_graph_from_json(och_graph *g, const char *text, size_t len);
    int och_graph_save_json(och_graph *g, const char *path);
    int och_graph_load_json(och_graph *g, const char *path);
    /* per node in the graph's order (any pointer may be NULL): id, index into the model table, features, sparse features */
    void och_graph_node_table(const och_graph *g, uint64_t *ids, uint32_t *model_index, uint64_t *n_features, uint64_t *n_sparse);
    /* one node's payload by its place in the graph's order (any pointer may be NULL): feature locations n x 2, strengths,
     * descriptors n x 8 words, position 3, orientation 4 (x y z w); its image path */
    int och_graph_node_payload(const och_graph *g, size_t index, double *loc, float *strength, uint64_t *desc,
                               double *position3, double *orientation4);
    const char *och_graph_node_path(const och_graph *g, size_t index);
    int och_graph_set_node_path(och_graph *g, size_t index, const char *path);
    /* a node's "metadata" object as text: set takes any well-formed JSON value (NaN allowed) and keeps it in the
     * writer's layout, -1 + och_last_error(g) otherwise; "" until one is set or a graph.json brought one */
    const char *och_graph_node_metadata(const och_graph *g, size_t index);
    int och_graph_set_node_metadata(och_graph *g, size_t index, const char *json, size_t len);
    size_t och_graph_num_models(const och_graph *g);
    int och_graph_get_model(const och_graph *g, uint32_t index, double *m11); /* och_graph_add_model's ten, then the id */
    int och_surface_save_ply(const och_surface *s, const char *path);
    int och_surface_load_ply(och_surface *s, const char *path);
    size_t och_surface_num_clouds(const och_surface *s);
    void och_surface_cloud_sizes(const och_surface *s, uint64_t *sizes);
    void och_surface_set_clouds(och_surface *s, size_t n_clouds, const uint64_t *sizes, const double *xyz);
    typedef struct och_checkpoint och_checkpoint;
    int och_checkpoint_validate(const char *dir); /* 1 = metadata.json and graph.json exist */
    /* state: a PipelineState name (types/pipeline_state.hpp:25-55); info4: state_run_count, origin latitude, longitude, 0 */
    int och_checkpoint_save(const char *dir, och_graph *g, const och_surface *const *surfaces, size_t n_surfaces,
                            const char *state, const double *info4);
    och_checkpoint *och_checkpoint_load(const char *dir, och_graph *g); /* NULL + och_last_error(g) on failure */
    void och_checkpoint_destroy(och_checkpoint *cp);
    size_t och_checkpoint_num_surfaces(const och_checkpoint *cp);
    const char *och_checkpoint_state(const och_checkpoint *cp);
    void och_checkpoint_info(const och_checkpoint *cp, double *info4);
    int och_checkpoint_get_surface(const och_checkpoint *cp, size_t index, och_surface *out);

    /* ---- a survey from its files alone: image metadata, the local frame, the GeoJSON camera graph.
     *      Host code only: nothing here touches a device. ---------------------------------------------------------------
     * och_jpeg_metadata: image_metadata of a JPEG file's bytes (opencalibration_amd/csrc/host/image_metadata.hpp; the
     * reference's extract_metadata over its EXIF / XMP reader).  numbers14: width, height, focal_length_px, principal x y,
     * latitude, longitude, altitude, relative_altitude, roll, pitch, yaw, accuracy_xy, accuracy_z (NaN = absent).
     * strings: make, model, serial_no, lens_make, lens_model, datum, timestamp, datestamp, each NUL-terminated, one after
     * the other in the caller's `cap` bytes; *needed (may be NULL) is their total length.  Returns OCH_METADATA_OK /
     * _ABSENT (no Exif, no XMP: the defaults) / _CORRUPT (the defaults), or -1 for a NULL argument or a `cap` below
     * *needed (nothing but *needed written).  Never reads outside data[0 .. size). */
#define OCH_METADATA_OK 0
#define OCH_METADATA_ABSENT 1
#define OCH_METADATA_CORRUPT 2
    int och_jpeg_metadata(const uint8_t *data, uint64_t size, double *numbers14, char *strings, uint64_t cap, uint64_t *needed);
    /* GeoCoord (opencalibration_amd/csrc/host/geo_coord.hpp): Transverse Mercator on WGS84 about the origin, k0 = 1, no
     * false origin, Krueger's series to n^6 in fp64.  The projection's centre is strtod("%g") of the origin - the
     * reference writes its WKT with six significant digits - while the origin reported stays unrounded.  create: NULL for
     * a non-finite origin.  origin4: origin latitude, longitude, then the centre's.  to_local: n x (latitude, longitude,
     * altitude) -> n x (easting, northing, altitude); to_wgs84: n x (x, y, z) -> n x (longitude, latitude, altitude); a
     * point that cannot be transformed (non-finite, 90 degrees or more from the central meridian) becomes three NaNs.
     * wkt: the text into buf[0 .. cap) when it fits (NUL-terminated); returns its length without the NUL. */
    typedef struct och_geo och_geo;
    och_geo *och_geo_create(double latitude, double longitude);
    void och_geo_destroy(och_geo *geo);
    void och_geo_origin(const och_geo *geo, double *origin4);
    void och_geo_to_local(const och_geo *geo, size_t n, const double *lat_lon_alt, double *xyz);
    void och_geo_to_wgs84(const och_geo *geo, size_t n, const double *xyz, double *lon_lat_alt);
    size_t och_geo_wkt(const och_geo *geo, char *buf, size_t cap);
    /* toVisualizedGeoJson (src/io/serialize_MeasurementGraph.cpp:62-209): Points of the nodes then LineStrings of the
     * edges, positions through geo (NULL: the local coordinates as they are).  node_ids / edge_ids NULL: all of them,
     * sorted by id, else the given ones in the given order.  malloc'd, NUL-terminated (och_free); NULL +
     * och_last_error(g) for an id the graph does not have. */
    char *och_graph_geojson(och_graph *g, const och_geo *geo, const uint64_t *node_ids, size_t n_nodes, const uint64_t *edge_ids,
                            size_t n_edges, size_t *len);

    /* ---- dense guided matching (opencalibration_amd/csrc/host/dense_stereo.hpp): densifyMesh(graph, surfaces) of
     *      src/dense/dense_stereo.cpp:66-403 with the surface's mesh as surfaces[0]; the triangulated points are appended
     *      to the surface as one more cloud.  stats10 (may be NULL): images, dense features, queries sent to the device,
     *      accepted matches, tracks, points, then seconds {index build, rays + predictions, device, tracks}.  match_pairs
     *      (may be NULL, match_cap pairs): accepted matches as measurement ids (image offset + dense feature number). */
    int och_densify_mesh(och_graph *g, ochip_ctx *ctx, och_surface *surface, double *stats10, uint64_t *match_pairs,
                         size_t match_cap);
    uint32_t och_hilbert_xy2d(int order, int x, int y); /* types/hilbert.hpp:9-28 */

    /* ---- mesh refinement (opencalibration_amd/csrc/host/refine_mesh.hpp; src/surface/refine_mesh.cpp:15-909) ----------
     * refineByPointDensity / refineAtPoint on the surface's mesh with its clouds; countPointsPerTriangle as rows of
     * (three vertices, {count, distance variance}) in the order the triangles first receive a point; the triangle under
     * points (TriangleLocator).  och_mesh_refinement_run: the MESH_REFINEMENT state of the pipeline
     * (src/pipeline/pipeline.cpp:666-819) - minimal mesh, RelaxStage {ORIENTATION, GROUND_MESH} at grid fraction
     * 0.1 / 2^level on the device, count, refine or advance the level - repeated until the state is left or max_steps
     * runs were made; log8 rows {level, grid fraction, gsd, triangles above threshold, max points per triangle,
     * triangles created, mesh vertices, repeat flag}.  Returns the steps made, -1 + och_last_error(g) on a device error. */
    size_t och_refine_by_point_density(och_surface *s, size_t max_points_per_triangle, double min_distance_variance,
                                       int max_iterations, double min_triangle_size);
    size_t och_refine_at_point(och_surface *s, double x, double y, int levels);
    size_t och_count_points_per_triangle(const och_surface *s, uint64_t *tri3, double *stats2, size_t cap);
    void och_surface_locate(const och_surface *s, const double *xy, size_t n, uint64_t *tri3);
    int och_mesh_refinement_run(och_graph *g, ochip_ctx *ctx, och_surface *surface, int max_steps, double *log8);

    /* ---- points per triangle over the flat locate table, and the DENSE_MESH_RELAX state (opencalibration_amd/csrc/host/
     *      mesh_points.hpp, csrc/mesh_locate.hpp; src/pipeline/pipeline.cpp:844-924) ----------
     * The two entries above stay as they are; these give the same rows bit for bit by another route: the mesh flattened
     * into a locate table, every point located by nearest centroid and a walk of at most max_steps triangles (100 where
     * no argument says otherwise; a point whose steps run out is found by the exhaustive scan on the host), the sums in
     * point order.  ctx == NULL: that route in host loops (locate under OpenMP); else on the device (ochip_mesh_points_*
     * of ochip.h), the cloud uploaded once per call or per counter.  och_surface_count_points returns SIZE_MAX and
     * och_surface_locate_on -1 on a device error, with the text in och_points_last_error() (per thread).
     * och_point_counter: a cloud (xyz [n][3]) kept for counts against changing meshes - what refineByPointDensity and the
     * state use between their iterations; count: the rows for the surface's mesh (its own clouds are not read),
     * exhausted (may be NULL): how many points ran out of steps.  create returns NULL on a device error.
     * och_surface_locate_table: the flat table of the surface's mesh as arrays - sizes2 = {T, entries of start};
     * vertex_xy [T][6], neighbours [T][3] (0xFFFFFFFF: none), plane [T][6], cx, cy [T], grid4 = {x0, y0, cell, nx},
     * start [sizes2[1]], items [T].
     * och_dense_mesh_relax_run: the DENSE_MESH_RELAX state - gsd and reduced gsd at grid fraction 0.05, one
     * refineByPointDensity(mesh, cloud, 20, (2 gsd)^2, 1, reduced gsd), repeat while triangles were created, at most 21
     * runs - repeated until the state is left or max_steps runs were made; surface: in = the densified surface, out = the
     * refined one (a surface without mesh and cloud stands for an empty surface list).  log6 rows {run, gsd, reduced gsd,
     * triangles above threshold, triangles created, mesh vertices}.  Returns the steps made, -1 + och_last_error(g) on a
     * device error.  With a context the cloud crosses to the device once per call. */
    typedef struct och_point_counter och_point_counter;
    const char *och_points_last_error(void);
    size_t och_surface_count_points(const och_surface *s, ochip_ctx *ctx, uint64_t *tri3, double *stats2, size_t cap);
    int och_surface_locate_on(const och_surface *s, ochip_ctx *ctx, const double *xy, size_t n, int max_steps, uint64_t *tri3);
    och_point_counter *och_point_counter_create(ochip_ctx *ctx, const double *xyz, size_t n, int max_steps);
    void och_point_counter_destroy(och_point_counter *c);
    size_t och_point_counter_count(och_point_counter *c, const och_surface *s, uint64_t *tri3, double *stats2, size_t cap,
                                   uint64_t *exhausted);
    void och_surface_locate_table_sizes(const och_surface *s, uint64_t *sizes2);
    void och_surface_locate_table(const och_surface *s, double *vertex_xy, uint32_t *neighbours, double *plane, double *cx, double *cy,
                                  double *grid4, uint32_t *start, uint32_t *items);
    int och_dense_mesh_relax_run(och_graph *g, ochip_ctx *ctx, och_surface *surface, int max_steps, double *log6);

    /* ---- the filtered point cloud file and the textured OBJ (opencalibration_amd/csrc/host/xyz_export.hpp, .cpp;
     *      csrc/xyz_export.hpp; the runner's deliverables after COMPLETE, app/pipeline_runner.cpp:351-395; DESIGN.md
     *      section 4.16) ----------
     * The cloud is all clouds of all surfaces in surface, cloud, point order.  och_cloud_outlier_bounds: filterOutliers
     * (src/io/saveXYZ.cpp:50-105), bounds6 = {x first, x second, y first, y second, z first, z second}; a coordinate that
     * is not finite or not below 2^63 in magnitude is refused.  och_cloud_to_xyz: the bytes of toXYZ (:6-48) for that box
     * (bounds6 == NULL: no filter), malloc'd and NUL-terminated (och_free), *len its length, *kept (may be NULL) its lines;
     * och_cloud_save_xyz: the same into a file.  ctx == NULL: host loops under OpenMP; else the device route
     * (ochip_xyz_export_* of ochip.h) - the same bytes; the route never changes by size.  och_xyz_*: the same for a
     * flat array xyz [n][3].  0 = ok; -1 or NULL + och_export_last_error() (per thread) otherwise.
     * och_format_g6: per value 16 bytes of text (zero-padded) and the length of `ostream << double` - the integer
     * formatter of csrc/xyz_export.hpp, which gives length 0 for |v| outside [1e-5, 2^63) and not 0; with_fallback != 0:
     * those through snprintf("%g"), as the exports do.
     * och_textured_obj: the OBJ and MTL text of generateTexturedOBJ (src/ortho/ortho.cpp:2125-2255) over an orthomosaic
     * of width x height pixels whose top-left corner is (min_x, max_y) at gsd_x, gsd_y metres per pixel: per surface with
     * edges its vertices `v x y z` and `vt u v` in ascending node id, then the faces the PLY writer lists, in its order,
     * as `f a/a b/b c/c` with 1-based indices past the surfaces before.  Both texts malloc'd (och_free). */
    const char *och_export_last_error(void);
    int och_cloud_outlier_bounds(const och_surface *const *surfaces, size_t n_surfaces, ochip_ctx *ctx, int64_t *bounds6);
    char *och_cloud_to_xyz(const och_surface *const *surfaces, size_t n_surfaces, ochip_ctx *ctx, const int64_t *bounds6,
                           size_t *len, uint64_t *kept);
    int och_cloud_save_xyz(const och_surface *const *surfaces, size_t n_surfaces, ochip_ctx *ctx, const int64_t *bounds6,
                           const char *path);
    int och_xyz_outlier_bounds(const double *xyz, size_t n, ochip_ctx *ctx, int64_t *bounds6);
    char *och_xyz_to_text(const double *xyz, size_t n, ochip_ctx *ctx, const int64_t *bounds6, size_t *len, uint64_t *kept);
    void och_format_g6(const double *values, size_t n, int with_fallback, char *text16, uint8_t *len);
    int och_textured_obj(const och_surface *const *surfaces, size_t n_surfaces, int64_t width, int64_t height, double min_x,
                         double max_y, double gsd_x, double gsd_y, const char *mtl_name, const char *jpg_name, char **obj_out,
                         size_t *obj_len, char **mtl_out, size_t *mtl_len);

    /* ---- orthomosaic preview and DSM raster (opencalibration_amd/csrc/host/ortho.hpp; src/ortho/ortho.cpp:228-964) -------
     * The reference's context: calculateBoundsAndMeanZ (bounds5 = min_x, max_x, min_y, max_y, mean_surface_z; a surface's
     * clouds count only when it has no mesh), calculateGSD over the given nodes in the given order (thumbnail != 0: the
     * preview's, at thumbnail scale), prepareOrthoMosaicContext (ctx8 = bounds5, gsd, mean_camera_z,
     * average_camera_elevation; returns the involved nodes: those with a finite orientation), the two output clamps
     * (input pixels = the involved nodes' model pixels_cols x pixels_rows) and rayTraceHeight. */
    /* rows, cols <= 65535 (0 x 0 clears the thumbnail); -1 + och_last_error(g) otherwise */
    int och_graph_set_thumbnail(och_graph *g, size_t node_index, size_t rows, size_t cols, const uint8_t *rgb /* rows x cols x 3 */);
    void och_ortho_bounds(const och_surface *const *surfaces, size_t n, double *bounds5);
    double och_ortho_gsd(const och_graph *g, const uint64_t *node_ids, size_t n_ids, double mean_surface_z, int thumbnail);
    size_t och_ortho_context(const och_graph *g, const och_surface *const *surfaces, size_t n, int thumbnail, double *ctx8);
    void och_ortho_clamp_resolution(uint64_t total_input_pixels, double *gsd, int32_t *width, int32_t *height);
    void och_ortho_clamp_megapixels(double max_output_megapixels, double *gsd, int32_t *width, int32_t *height);
    double och_ray_trace_height(const och_surface *const *surfaces, size_t n, double x, double y, double mean_camera_z);
    /* generateOrthomosaic (ortho.cpp:478-653): plan8 = {width, height, gsd, min_x, max_x, min_y, max_y, mean_camera_z} is
     * always written; rgba == NULL: size query only.  rgba [height][width][4], ids [height][width] (node id & 0xFFFFFFFF,
     * 0xFFFFFFFF for background and for pixels no surface holds, which get (0, 0, 0, 0)).  Every involved node needs a
     * thumbnail (och_graph_set_thumbnail).  ctx == NULL: the CPU route, whose heights come from z_in when it is given
     * (height x width fp64); z_out (may be NULL) returns the fp64 heights used.  -1 + och_last_error(g) on failure. */
    int och_orthomosaic_thumbnail(och_graph *g, ochip_ctx *ctx, const och_surface *const *surfaces, size_t n, const double *z_in,
                                  double *plan8, uint8_t *rgba, uint32_t *ids, double *z_out);
    /* generateDSMGeoTIFF's raster (ortho.cpp:866-964): the full-resolution plan (plan8 as above) with
     * max_output_megapixels (<= 0: no cap), then bands of it.  och_ortho_mesh_upload builds the surfaces' triangle table on
     * the device (release with ochip_ortho_mesh_destroy).  och_dsm_render: rows [row0, row0 + rows) into out
     * [rows][width] as float, NaN where no surface holds the pixel; dev != NULL: on the device (ctx = dev's context; out a
     * device pointer when out_on_device), dev == NULL: the CPU route (host out).  Debug outputs (host, may be NULL):
     * tri_out the triangle (index into the table: surfaces in order, each one's triangles by ascending node triple),
     * z64_out the fp64 heights, capped_walks the CPU route's walks that ran out of steps.  -1 + och_ortho_last_error(). */
    int och_dsm_plan(const och_graph *g, const och_surface *const *surfaces, size_t n, double max_output_megapixels, double *plan8);
    int och_ortho_mesh_upload(ochip_ctx *ctx, const och_surface *const *surfaces, size_t n, ochip_ortho_mesh **out);
    int och_dsm_render(ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces, size_t n, const double *plan8,
                       int64_t row0, int64_t rows, float *out, int out_on_device, uint32_t *tri_out, double *z64_out,
                       uint64_t *capped_walks);
    const char *och_ortho_last_error(void);
    /* ---- layered full-resolution orthomosaic (opencalibration_amd/csrc/host/ortho_layers.cpp; src/ortho/ortho.cpp:
     * 1206-1663) -----------------------------------------------------------------------------------------------------------
     * och_ortho_layers_cameras: the involved nodes (finite orientation, node order) as ochip_ortho_layers' camera records
     * (cams [n][28], node_ids, model_ids, image_hw [n][2] = the model's pixels_rows, pixels_cols; each may be NULL);
     * returns n.  Camera i of the render is involved node i.
     * och_ortho_layers_render: rows [row0, row0 + rows) of plan8 (och_dsm_plan's full-resolution plan), whole tile rows
     * from a tile row (the raster's last may be partial); config4 = {num_layers 1..8, tile_size,
     * correspondence_kernel_radius, correspondence_subsample}.  images [n]: one BGR image per involved camera,
     * image_hw[i] rows x cols x 3 bytes, refused unless that is the model's size; host pointers for the CPU route, device
     * pointers for the device route.  ctx and dev (och_ortho_mesh_upload) == NULL: the CPU route (brute-force kNN, one
     * thread per row, host outputs), whose heights are dsm_in ([rows][width] float) when given; else the device
     * (out_on_device: bgra / ids / weight are device pointers).  Outputs as ochip_ortho_layers; corr_out == NULL (capacity
     * 0): *n_corr is the count only.  -1 + och_ortho_layers_last_error() on failure.
     * och_lab_convert (L1, the conversion both routes use): mode 0 BGR -> 8-bit Lab, 1 8-bit Lab -> BGR (3 bytes each),
     * 2 BGR -> float Lab (3 floats).  och_ortho_patch_sample: PatchSampler::sampleWithJacobian at world point xyz for one
     * camera record over img; returns 1 with bgr_out, 0 when the camera does not see the point; pixel2 and J4 (row-major
     * d pixel / d (x, y)) are always written.  och_ortho_sample_fields: normalized radius, x, y, the blend weight and
     * acos(cos_view) as the render computes them. */
    size_t och_ortho_layers_cameras(const och_graph *g, const och_surface *const *surfaces, size_t n, double *cams,
                                    uint64_t *node_ids, uint32_t *model_ids, int64_t *image_hw);
    int och_ortho_layers_render(const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces,
                                size_t n, const double *plan8, const int32_t *config4, int64_t row0, int64_t rows,
                                const uint64_t *images, const int64_t *image_hw, const float *dsm_in, int out_on_device,
                                uint8_t *bgra, uint64_t *ids, float *weight, ochip_color_corr *corr_out, uint64_t corr_capacity,
                                uint64_t *n_corr, uint32_t *knn_out);
    const char *och_ortho_layers_last_error(void);
    void och_lab_convert(int mode, const uint8_t *in, size_t n, void *out);
    int och_ortho_patch_sample(const double *cam28, const uint8_t *img, double gsd, const double *xyz, uint8_t *bgr_out,
                               double *pixel2, double *J4);
    void och_ortho_sample_fields(double pixel_x, double pixel_y, int32_t width, int32_t height, float camera_distance,
                                 double cos_view, float *out5);
    /* ---- the layered render with streamed source images (opencalibration_amd/csrc/host/ortho_stream.cpp,
     * ortho_residency.hpp; the reference's findTileCameras, LRU image cache and prefetch thread, src/ortho/ortho.cpp:
     * 1010-1066, 1501-1539) ------------------------------------------------------------------------------------------------
     * och_ortho_band_cameras: the raster rows x cols (raster4 = {min_x, max_y, gsd, mean_camera_z}) cut into bands of
     * band_rows rows (a multiple of the tile size; the last may be shorter); used [n_bands][n_cams] = 1 exactly when
     * camera i (cams [n_cams][28], och_ortho_layers_cameras') is among the 5 nearest in XY (squared distance, then camera
     * order) of at least one pixel of band b, whatever the pixel's height: a superset of what the band's render reads,
     * independent of the DSM.  ctx == NULL: the CPU route (brute force), else ochip_ortho_band_cameras.
     * och_ortho_layers_render_subset: och_ortho_layers_render over the cameras subset [n_subset] alone (ascending, unique
     * indices into och_ortho_layers_cameras' order, refused otherwise); images and image_hw have n_subset entries.  A
     * subset that holds the band's set of och_ortho_band_cameras gives the full table's BGRA, ids, weights and
     * correspondences bit for bit; knn_out names full-table indices.
     * och_ortho_residency_plan: ortho_residency.hpp's rule over the sets used [n_bands][n_cams] and `capacity` slots.
     * resident [capacity]: the camera each slot holds before the first band (-1: free), replaced by the state after the
     * last; load_off [n_bands + 1]; loads3 (may be NULL) [sum of the sets' sizes at most][3] = camera, slot, phase
     * (0 ahead, 1 late), band k's at [load_off[k], load_off[k + 1]).  -1 when a band reads more than `capacity` images.
     * och_ortho_stream_*: the render of plan8 in bands of band_tile_rows tile rows from capacity_images slots of the
     * largest image's size, one block of ctx's pool (ctx and mesh NULL: the CPU route, slots in host memory).  create
     * computes the bands' sets and the plan; g, mesh and surfaces outlive the object.  band_cameras / loads: a band's
     * cameras (ascending) and loads3 as above, returning their number (arguments may be NULL).  upload copies involved
     * camera `camera`'s image (pixels_rows x pixels_cols x 3) into its planned slot on the context's copy stream: it
     * returns at once and overlaps the band that renders when host_bgr is page-locked and must then stay valid until the
     * band's render has returned; pageable memory is merely correct.  render: band `band` as och_ortho_layers_render
     * writes it, after the compute stream has waited for the band's uploads; returns once the band is written.
     * The order the plan assumes is enforced: bands render ascending; an ahead upload of band k is accepted once
     * render(k - 2) has returned, a late one once render(k - 1) has; render(k) is refused while a planned load of k is
     * missing; an upload that is not planned, or made twice, is refused.  rewind (after the last band): a further sweep,
     * planned from the images the slots hold.  upload_end_ms: when band's last upload finished on the device, in ms since
     * the sweep began.  -1 + och_ortho_stream_last_error() on failure.
     * upload_jpegs (the reference's cv::imread in FullResolutionImageCache::getImage,
     * src/ortho/image_cache.cpp:37): n planned loads of `band` from baseline JPEG files, files[i] / sizes[i] (host memory)
     * being involved camera cameras[i]'s, decoded by one och_jpeg_decoder the stream owns - made at the first call, on the
     * stream's route, destroyed with it - straight into the planned slots: out is the slot block, offsets[i] the slot's
     * distance from its start, the EXIF orientation applied.  Before a byte is parsed every camera passes upload's checks
     * (a planned load of the band, not uploaded yet, the ahead / late rule), none appears twice and no file is NULL; then
     * the headers of all files are read, and the call is refused when one is unsupported or corrupt or decodes to
     * another size than the camera's pixels_cols x pixels_rows.  A refusal up to here launches nothing and marks nothing;
     * info (or NULL) [n] is filled from the headers on.  Behind the headers the files count one by one, in decoder batches
     * of at most 2^28 pixels: a file whose scan turns out corrupt leaves its load pending - upload may still bring that
     * camera's pixels - while the call's others count as uploaded; the call then returns -1, the message names the
     * camera and info[i].status the file.  n == 0 does nothing.  The call returns when the pixels are in their slots (the
     * decoder runs on the context's compute stream and waits for it), so the band's mark, recorded behind the band's last
     * load whichever way it came, still covers exactly the copies. */
    int och_ortho_band_cameras(ochip_ctx *ctx, const double *raster4, int32_t cols, int64_t rows, int64_t band_rows, size_t n_cams,
                               const double *cams, uint8_t *used);
    int och_ortho_layers_render_subset(const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *dev, const och_surface *const *surfaces,
                                       size_t n, const double *plan8, const int32_t *config4, int64_t row0, int64_t rows,
                                       const uint32_t *subset, size_t n_subset, const uint64_t *images, const int64_t *image_hw,
                                       const float *dsm_in, int out_on_device, uint8_t *bgra, uint64_t *ids, float *weight,
                                       ochip_color_corr *corr_out, uint64_t corr_capacity, uint64_t *n_corr, uint32_t *knn_out);
    int och_ortho_residency_plan(const uint8_t *used, size_t n_bands, size_t n_cams, size_t capacity, int32_t *resident,
                                 size_t *load_off, int32_t *loads3);
    typedef struct och_ortho_stream och_ortho_stream;
    int och_ortho_stream_create(const och_graph *g, ochip_ctx *ctx, ochip_ortho_mesh *mesh, const och_surface *const *surfaces,
                                size_t n, const double *plan8, const int32_t *config4, int64_t band_tile_rows,
                                size_t capacity_images, och_ortho_stream **out);
    void och_ortho_stream_destroy(och_ortho_stream *s);
    size_t och_ortho_stream_num_bands(const och_ortho_stream *s);
    size_t och_ortho_stream_band_cameras(const och_ortho_stream *s, size_t band, uint32_t *cameras);
    size_t och_ortho_stream_loads(const och_ortho_stream *s, size_t band, int32_t *loads3);
    int och_ortho_stream_upload(och_ortho_stream *s, size_t band, uint32_t camera, const uint8_t *host_bgr);
    int och_ortho_stream_upload_jpegs(och_ortho_stream *s, size_t band, size_t n, const uint32_t *cameras,
                                      const uint8_t *const *files, const uint64_t *sizes,
                                      ochip_jpeg_file_info *info /* [n] or NULL */);
    int och_ortho_stream_render(och_ortho_stream *s, size_t band, const float *dsm_in, int out_on_device, uint8_t *bgra,
                                uint64_t *ids, float *weight, ochip_color_corr *corr_out, uint64_t corr_capacity, uint64_t *n_corr,
                                uint32_t *knn_out);
    int och_ortho_stream_rewind(och_ortho_stream *s);
    int och_ortho_stream_upload_end_ms(och_ortho_stream *s, size_t band, double *ms);
    const char *och_ortho_stream_last_error(void);
    /* ---- blended full-resolution orthomosaic (opencalibration_amd/csrc/host/ortho_blend.cpp; src/ortho/ortho.cpp:
     * 1665-1990, src/ortho/blending.cpp) ------------------------------------------------------------------------------------
     * och_ortho_blend_render: rows [row0, row0 + rows) of plan8 (och_dsm_plan's plan) blended from the layers of
     * och_ortho_layers_render (bgra, ids: [L][rows][width]) and the DSM band dsm [rows][width]; config4 = {num_layers
     * 1..8, tile_size 1..4096, pyramid_levels, blend_transition_radius >= 1}.  The colour balance: per node id color_ids[i]
     * color6[i] = lab_offset 3, brdf, slope 2; per model id vig3[i] = 3 vignetting coefficients, of which only model id
     * 0's are used.  ctx == NULL: the CPU route (one thread per tile, host memory); else
     * ochip_ortho_blend on ctx's device (on_device: bgra / ids / dsm / rgba are device pointers).  rgba [rows][width][4];
     * debug outputs as ochip_ortho_blend's, host, each may be NULL.  -1 + och_ortho_blend_last_error() on failure.
     * och_laplacian_blend: laplacianBlend on the CPU route (ochip_laplacian_blend's arguments); -1 on a bad argument.
     * och_blend_chamfer: the sequential two-pass chamfer of a rows x cols mask (non-zero: boundary) in 1e-4 units.
     * och_blend_pyr: pyrDown (up 0; w x h -> W x H = ((w + 1) / 2, (h + 1) / 2)) or pyrUp (up 1; to W x H) of 1 or 3
     * interleaved float channels.  och_blend_math: mode 0 exp_restated (n floats), 1 the falloff (n pairs steepness, d),
     * 2 float Lab -> BGR8 (n triples). */
    int och_ortho_blend_render(const och_graph *g, ochip_ctx *ctx, const och_surface *const *surfaces, size_t n,
                               const double *plan8, const int32_t *config4, int64_t row0, int64_t rows, size_t n_color,
                               const uint64_t *color_ids, const double *color6, size_t n_models, const uint32_t *model_ids,
                               const double *vig3, int on_device, const uint8_t *bgra, const uint64_t *ids, const float *dsm,
                               uint8_t *rgba, float *weight_out, float *dist_out, float *lab_out);
    const char *och_ortho_blend_last_error(void);
    int och_laplacian_blend(int32_t num_layers, int32_t rows, int32_t cols, int32_t pyramid_levels, const float *lab,
                            const float *weight, uint8_t *bgra_out);
    void och_blend_chamfer(int32_t rows, int32_t cols, const uint8_t *boundary, int32_t *dist);
    void och_blend_pyr(int up, int32_t channels, int32_t w, int32_t h, int32_t W, int32_t H, const float *src, float *out);
    void och_blend_math(int mode, size_t n, const float *in, void *out);

    /* ---- colour balance between the layered render and the blend (opencalibration_amd/csrc/host/color_balance.cpp;
     * solveColorBalance, src/ortho/color_balance.cpp, and its caller Pipeline::Impl::color_balance,
     * src/pipeline/pipeline.cpp:987-1018) ------------------------------------------------------------------------------
     * och_color_balance_solve: collects the camera and model ids of corr (och_ortho_layers_render's records), solves the
     * radiometric parameters - ctx != NULL: ochip_color_balance_solve on its device; NULL: the CPU route, same arithmetic
     * and trust-region rules with a dense Cholesky, at most 4096 unknowns (6 per camera + 3 per model) - and removes the
     * gauge: over the solved cameras that have a position (the explicit list position_ids / position_xy [n][2] first,
     * else graph node id -> payload.position x, y; g may be NULL; an id without either is skipped), at least 3 of them,
     * the least-squares plane a x + b y + c per Lab channel is subtracted from their offsets; the minimum-norm solution
     * when the positions are collinear (singular values at or below max(n, 3) * 2^-52 * the largest count as zero).
     * Outputs in ascending id order, the blend's layout: cam_ids_out, color6_out [n][6] = lab_offset 3, brdf, slope 2;
     * model_ids_out, vig3_out [n][3]; *n_cams / *n_models always receive the counts (a capacity too small: -1).
     * summary4 = {success, final_cost, num_iterations (summary.iterations.size()), termination (OCHIP_RELAX_*)}.
     * n_corr == 0: success 0, empty tables, nothing launched.  A correspondence with camera_id_a == camera_id_b is
     * refused (-1): the reference's Ceres aborts on a duplicate parameter block.  -1 + och_color_balance_last_error().
     * och_color_balance_evaluate (tests): cost, dense J'J (n x n) and J'r (n), n = 6 n_cams + 3 n_models, at the given
     * parameters (ids sorted and unique), cam_col / model_col the first unknown of every camera / model; ctx as above.
     * Returns 0, 1 when a residual is not finite, -1 on an error.
     * och_color_balance_evaluate_plan (tests): the same evaluation as the DEVICE forms it, run on the host - the plan of
     * opencalibration_amd/csrc/color_balance_plan.hpp (chunks, the order of the unknowns, the owners' record lists) and
     * the kernels' own arithmetic in the kernels' order, so the device's result equals it bit for bit; cam_col / model_col
     * in the plan's order; layout4 (may be NULL) = {tail_begin, regions, separator cameras, chunks}.
     * och_color_balance_remove_gauge: the gauge step alone on n positions xy [n][2] and offsets3 [n][3] (in place; n < 3:
     * untouched); returns the rank used. */
    int och_color_balance_solve(const och_graph *g, ochip_ctx *ctx, const ochip_color_corr *corr, size_t n_corr,
                                size_t n_positions, const uint64_t *position_ids, const double *position_xy,
                                size_t cam_capacity, uint64_t *cam_ids_out, double *color6_out, size_t *n_cams,
                                size_t model_capacity, uint32_t *model_ids_out, double *vig3_out, size_t *n_models,
                                double *summary4);
    int och_color_balance_evaluate(ochip_ctx *ctx, const ochip_color_corr *corr, size_t n_corr, size_t n_cams,
                                   const uint64_t *cam_ids, const double *color6, size_t n_models, const uint32_t *model_ids,
                                   const double *vig3, double *cost, double *JtJ, double *Jtr, int32_t *cam_col,
                                   int32_t *model_col);
    int och_color_balance_evaluate_plan(const ochip_color_corr *corr, size_t n_corr, size_t n_cams, const uint64_t *cam_ids,
                                        const double *color6, size_t n_models, const uint32_t *model_ids, const double *vig3,
                                        double *cost, double *JtJ, double *Jtr, int32_t *cam_col, int32_t *model_col,
                                        int32_t *layout4);
    int och_color_balance_remove_gauge(size_t n, const double *xy, double *offsets3);
    const char *och_color_balance_last_error(void);

    /* ---- the load stage's image thumbnails (opencalibration_amd/csrc/host/thumbnail.cpp, csrc/thumbnail.hpp;
     * src/extract/extract_image.cpp:42-52) -----------------------------------------------------------------------------------
     * och_thumbnail_size: the thumbnail of a width x height image has rint(height * s) rows and rint(width * s) columns, s =
     * 50 / sqrt(width * height); refused below 2500 pixels and when a side comes out 0.  och_image_thumbnails: a batch of
     * equally sized BGR images (a device pointer when images_on_device, which needs ctx) -> rgb_out (host) [n][rows][cols][3],
     * R G B; ctx == NULL: the CPU route, bit for bit what the device computes.  och_graph_make_thumbnails: the same, stored
     * on the nodes node_ids[i] (ids as och_graph_load_images returns them) for och_orthomosaic_thumbnail.  -1 +
     * och_thumbnail_last_error() (och_last_error(g) for the graph call) on failure. */
    int och_thumbnail_size(int width, int height, int32_t *rows, int32_t *cols);
    int och_image_thumbnails(ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width, int height,
                             int images_on_device, uint8_t *rgb_out);
    int och_graph_make_thumbnails(och_graph *g, ochip_ctx *ctx, const uint8_t *images_bgr, uint32_t n_images, int width,
                                  int height, int images_on_device, const uint64_t *node_ids);
    const char *och_thumbnail_last_error(void);

    /* ---- averaged overview levels of the orthomosaic and the DSM (opencalibration_amd/csrc/host/ortho_overview.cpp,
     * csrc/ortho_overview.hpp; the reference's three BuildOverviews("AVERAGE", ...) calls, src/ortho/ortho.cpp:944-961,
     * 1642-1657, 2028-2044) --------------------------------------------------------------------------------------------------
     * The levels, the two cell rules and the builder of include/ochip.h (ochip_ortho_overviews_*, kind OCHIP_OVERVIEW_RGBA8 /
     * OCHIP_OVERVIEW_FLOAT32): ctx != NULL builds on its device; ctx == NULL is the CPU route, the same rule in straight
     * loops with the same builder semantics - host bands, host levels, bit for bit what the device computes.  A binding
     * that writes the rasters band by band creates its overview levels empty, feeds every finished band and writes the
     * rows complete_rows newly reports.  The refusals return OCHIP_EINVAL (a failed device call its
     * code) with the message in och_ortho_overviews_last_error. */
    typedef struct och_ortho_overviews och_ortho_overviews;
    int och_ortho_overviews_levels(int64_t width, int64_t height, int64_t *rows_cols);
    int och_ortho_overviews_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, void *const *levels, int on_device,
                                   och_ortho_overviews **out);
    int och_ortho_overviews_feed(och_ortho_overviews *o, int64_t row0, int64_t rows, const void *band);
    int64_t och_ortho_overviews_complete_rows(const och_ortho_overviews *o, int level);
    int och_ortho_overviews_finish(och_ortho_overviews *o);
    void och_ortho_overviews_destroy(och_ortho_overviews *o);
    const char *och_ortho_overviews_last_error(void);

    /* ---- per-tile progress of the layer and blend passes (opencalibration_amd/csrc/host/ortho_tile_thumbs.cpp,
     * csrc/ortho_tile_thumbs.hpp; the reference's TileProgressCallback, include/opencalibration/pipeline/progress.hpp:15-34,
     * src/ortho/ortho.cpp:1553-1614, 1962-2011) -------------------------------------------------------
     * One record per finished tile, the reference's TileUpdate with the thumbnail as pixels: the tile's rectangle in the
     * raster, the raster's size, tile_index the 1-based row-major index over the whole raster (the reference's is its
     * completion count; here bands run in raster order), total_tiles = ceil(width / T) * ceil(height / T), the thumbnail's
     * size and scale (include/ochip.h), pass 1 (layers) or 2 (blend), and the raster's min_x, max_y and gsd.  72 bytes, no
     * padding.
     * The object belongs to one raster (plan8 as och_dsm_plan writes it: width, height, gsd, min_x, max_x, min_y, max_y,
     * mean_camera_z), one tile size (1..4096) and layer count (1..8).  ctx != NULL: feed enqueues the thumbnail kernel and an
     * asynchronous copy into a page-locked block of the context's pool behind whatever the context's stream holds - the
     * band's render - and returns: the device never waits for the host.  pixels / weight as ochip_ortho_tile_thumbs' (device
     * pointers when on_device).  ctx == NULL: the CPU route, host inputs, computed in feed.  row0 must lie on a tile row,
     * rows be whole tile rows or end the raster, and the bands of one pass arrive in raster order without gaps (after the
     * raster's last row a pass may start again at row 0, and seek names the tile row a pass's next band starts at, for a
     * caller that reports a part of the raster); anything else is refused with the rows named.  pending: the bands
     * fed and not yet collected.  collect waits for the oldest fed band alone and returns its tiles in tile order: *n
     * records into updates and n slots of min(T, 128)^2 BGRA pixels into thumbs (host; the thumbnail densely at a slot's
     * start, the rest zero).  With updates == NULL it only reports that band's tile count in *n; a capacity below it is
     * refused and the band stays.  The refusals return OCHIP_EINVAL (a failed device call its code) with the message in
     * och_tile_progress_last_error.  destroy waits for what is still in flight and hands the blocks back. */
    typedef struct och_tile_update
    {
        int32_t pixel_x, pixel_y, pixel_w, pixel_h, total_output_width, total_output_height, tile_index, total_tiles, thumb_w,
            thumb_h, scale, pass;
        double bounds_min_x, bounds_max_y, meters_per_pixel;
    } och_tile_update;
    typedef struct och_tile_progress och_tile_progress;
    int och_tile_progress_create(ochip_ctx *ctx, const double *plan8, int32_t tile_size, int32_t num_layers, och_tile_progress **out);
    int och_tile_progress_feed(och_tile_progress *p, int pass, int64_t row0, int64_t rows, int on_device, const uint8_t *pixels,
                               const float *weight);
    int och_tile_progress_seek(och_tile_progress *p, int pass, int64_t row0);
    int och_tile_progress_pending(const och_tile_progress *p);
    int och_tile_progress_collect(och_tile_progress *p, och_tile_update *updates, uint8_t *thumbs, uint64_t capacity, uint64_t *n);
    void och_tile_progress_destroy(och_tile_progress *p);
    const char *och_tile_progress_last_error(void);

    /* ---- the textured OBJ's JPEG texture (opencalibration_amd/csrc/host/jpeg_encode.cpp, csrc/jpeg_encode.hpp; the
     * reference's cv::imwrite(jpg_path, texture) in generateTexturedOBJ, src/ortho/ortho.cpp:2096-2123; DESIGN.md section
     * 4.17) ---------------------------------------------------------------------------------------------------------------
     * The encoder of include/ochip.h (ochip_jpeg_*) over both routes.  ctx != NULL: the device route, as described there.
     * ctx == NULL: the same rules in host loops - the coefficients under OpenMP over the MCUs, the entropy coder serially -
     * over host bands, computed in feed; this route never changes by size.  Both give the same bytes.  The refusals
     * return OCHIP_EINVAL or OCHIP_ESTATE as there (a failed device call its code) with the message in
     * och_jpeg_last_error; a handle that create did not return or destroy has taken is refused, not followed. */
    typedef struct och_jpeg och_jpeg;
    int och_jpeg_create(ochip_ctx *ctx, int64_t width, int64_t height, int quality, och_jpeg **out);
    int och_jpeg_feed(och_jpeg *e, int64_t row0, int64_t rows, const void *pixels, int pixel_stride, int on_device);
    int64_t och_jpeg_pending(och_jpeg *e);
    int och_jpeg_collect(och_jpeg *e, uint8_t *buf /* or NULL */, uint64_t cap, uint64_t *n);
    int och_jpeg_finish(och_jpeg *e);
    void och_jpeg_destroy(och_jpeg *e);
    const char *och_jpeg_last_error(void);

    /* ---- baseline JPEG decoding of the load stage (opencalibration_amd/csrc/host/jpeg_decode.cpp, csrc/jpeg_decode.hpp;
     *      the reference's cv::imread(path), src/extract/extract_image.cpp:18-21) ----
     * och_jpeg_info: the headers of one file - size (oriented when apply_orientation), components, sampling, restart
     * interval, orientation, status (OCHIP_JPEG_*) - without a context; -1 only for NULL arguments.
     * The decoder of include/ochip.h (ochip_jpeg_decoder_*) over both routes.  ctx != NULL: the device route, out is a device
     * pointer.  ctx == NULL: the same pixels computed here in loops, OpenMP over the images, out is host memory.  -1 + a
     * message in och_jpeg_decode_last_error; a handle that create did not return or destroy has taken is refused, not
     * followed. */
    int och_jpeg_info(const uint8_t *data, uint64_t size, int apply_orientation, ochip_jpeg_file_info *out);
    typedef struct och_jpeg_decoder och_jpeg_decoder;
    int och_jpeg_decoder_create(ochip_ctx *ctx, int subsequence_bits, och_jpeg_decoder **out);
    int och_jpeg_decoder_decode(och_jpeg_decoder *d, int64_t n, const uint8_t *const *files, const uint64_t *sizes,
                                int apply_orientation, void *out, uint64_t out_cap, const uint64_t *offsets /* or NULL */,
                                ochip_jpeg_file_info *info /* [n] */, int32_t *rounds /* [2] or NULL */);
    void och_jpeg_decoder_destroy(och_jpeg_decoder *d);
    const char *och_jpeg_decode_last_error(void);

    /* ---- the tiles of the tiled DEFLATE GeoTIFFs (opencalibration_amd/csrc/host/geotiff.cpp, csrc/deflate_rules.hpp;
     *      DESIGN.md section 4.19) ----
     * The writer of include/ochip.h (ochip_geotiff_*) over both routes.  ctx != NULL: the device route, as described there.
     * ctx == NULL: the CPU route, host bands, the same rules in loops (a tile row's tiles under OpenMP) and the same bytes.
     * The message of a refusal is in och_geotiff_last_error; a handle that create did not return or destroy has taken is
     * refused, not followed.
     * och_deflate_code_lengths: the length limiter of the rules alone - lens[s] of at most `limit` bits for n <= 286
     * counts. */
#define OCH_GEOTIFF_RGBA8 OCHIP_GEOTIFF_RGBA8
#define OCH_GEOTIFF_FLOAT32 OCHIP_GEOTIFF_FLOAT32
#define OCH_GEOTIFF_MAX_SIDE OCHIP_GEOTIFF_MAX_SIDE
    typedef struct och_geotiff och_geotiff;
    int och_geotiff_create(ochip_ctx *ctx, int kind, int64_t width, int64_t height, int sparse, och_geotiff **out);
    /* ochip_geotiff_create_layered over both routes: the layers (kind 2) and cameras (kind 3) rasters of num_layers layers,
     * layer-major bands in, pixel-interleaved tiles out */
#define OCH_GEOTIFF_LAYERS8 OCHIP_GEOTIFF_LAYERS8
#define OCH_GEOTIFF_CAMERAS32 OCHIP_GEOTIFF_CAMERAS32
#define OCH_GEOTIFF_MAX_LAYERS OCHIP_GEOTIFF_MAX_LAYERS
    int och_geotiff_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int sparse,
                                   och_geotiff **out);
    int och_geotiff_feed(och_geotiff *e, int64_t row0, int64_t rows, const void *pixels, int on_device);
    int och_geotiff_payloads(och_geotiff *e, const uint8_t *payloads, int64_t n);
    int och_geotiff_collect(och_geotiff *e, uint8_t *buf /* or NULL */, uint64_t cap, uint64_t *bytes,
                            uint64_t *counts /* or NULL */, uint64_t max_tiles, uint64_t *tiles);
    int och_geotiff_finish(och_geotiff *e);
    void och_geotiff_destroy(och_geotiff *e);
    const char *och_geotiff_last_error(void);
    int och_deflate_code_lengths(const uint32_t *counts, int n, int limit, uint8_t *lens);

    /* ---- the PNG codec (opencalibration_amd/csrc/host/png.cpp, csrc/png_rules.hpp, csrc/host/png_decode.hpp; DESIGN.md
     *      section 4.20) ----
     * The encoder of include/ochip.h (ochip_png_encoder_*) over both routes.  ctx != NULL: the device route, as described
     * there.  ctx == NULL: the same rules in loops (OpenMP over the rows and segments of all images) and the same bytes; it
     * never changes route by size.  och_png_bound: the most bytes a file (or its base64) of that shape has, 0 for a shape
     * that is refused.  och_png_filter: the filtered payload alone, height (1 + width channels) bytes.  The message of a
     * refusal is in och_png_last_error.
     * The decoder is host code only.  och_png_info reads the signature and IHDR; och_png_decode gives the picture in the
     * file's channels (1, 2, 3 or 4), *pixels allocated here and released with och_png_free.  status: OCHIP_PNG_OK,
     * OCHIP_PNG_UNSUPPORTED (palette, 16 bits, fewer than 8 bits, Adam7: the caller falls back) or OCHIP_PNG_CORRUPT
     * (anything that does not parse or check: a chunk CRC, the zlib stream, its Adler-32, bytes behind it, a stream that
     * gives fewer or more bytes than IHDR says, a filter type above 4); *pixels is NULL unless the status is OK.  Both
     * return OCHIP_OK whatever the status, OCHIP_EINVAL only for a NULL output argument.
     * och_graph_encode_thumbnails: every node that has thumbnail pixels gets its thumbnail text, the base64 of a colour
     * type 2 file of the three bytes as stored, all nodes in one batch; returns their number, -1 + och_last_error(g).
     * och_graph_decode_thumbnails: every node with thumbnail text gets thumbnail pixels of three channels (gray replicated,
     * alpha dropped); statuses (or NULL): per node index -1 (no text) or the status, a refused node is left as it was;
     * returns the number decoded.  och_graph_get_thumbnail: the decoded thumbnail's size (0 x 0: none) and, with rgb, its
     * rows x cols x 3 bytes. */
#define OCHIP_PNG_OK 0
#define OCHIP_PNG_UNSUPPORTED 1
#define OCHIP_PNG_CORRUPT 2
    typedef struct och_png_file_info
    {
        uint32_t width, height;
        int32_t bit_depth, color_type, interlace, channels, status;
    } och_png_file_info;
    typedef struct och_png_encoder och_png_encoder;
    int och_png_encoder_create(ochip_ctx *ctx, och_png_encoder **out);
    int och_png_encoder_encode(och_png_encoder *e, int64_t n, const ochip_png_image *images, int on_device, int base64, uint8_t *out,
                               uint64_t out_cap, uint64_t *offsets /* [n + 1] */);
    void och_png_encoder_destroy(och_png_encoder *e);
    const char *och_png_last_error(void);
    uint64_t och_png_bound(int64_t width, int64_t height, int64_t channels, int base64);
    int och_png_filter(const ochip_png_image *image, uint8_t *payload, uint64_t cap);
    int och_png_info(const uint8_t *data, uint64_t size, och_png_file_info *out);
    int och_png_decode(const uint8_t *data, uint64_t size, och_png_file_info *info, uint8_t **pixels);
    void och_png_free(uint8_t *pixels);
    int och_graph_get_thumbnail(och_graph *g, size_t node_index, size_t *rows, size_t *cols, uint8_t *rgb /* or NULL */);
    int och_graph_encode_thumbnails(och_graph *g, ochip_ctx *ctx);
    int och_graph_decode_thumbnails(och_graph *g, int32_t *statuses /* [nodes] or NULL */);

    /* ---- reading tiled DEFLATE GeoTIFFs (opencalibration_amd/csrc/host/geotiff_read.cpp, csrc/inflate_rules.hpp;
     *      DESIGN.md section 4.21) ----
     * The reader of include/ochip.h (ochip_geotiff_reader_*) over both routes, with the same arguments.  ctx != NULL: the
     * device route, as described there.  ctx == NULL: the host route, the same rules in loops, one tile or stream a thread
     * under OpenMP, host rasters only; it never changes route by size.  The message of a refusal is in
     * och_geotiff_read_last_error; a handle that create did not return or destroy has taken is refused, not followed. */
    typedef struct och_geotiff_reader och_geotiff_reader;
    int och_geotiff_reader_create(ochip_ctx *ctx, int samples, int is_float, int64_t width, int64_t height, int tile_w, int tile_h,
                                  int predictor, uint64_t scratch_budget, och_geotiff_reader **out);
    int och_geotiff_reader_create_layered(ochip_ctx *ctx, int kind, int num_layers, int64_t width, int64_t height, int tile_w,
                                          int tile_h, int predictor, uint64_t scratch_budget, och_geotiff_reader **out);
    int och_geotiff_reader_inflate(och_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets /* [n + 1] */,
                                   const uint64_t *expect /* [n] */, uint8_t *out, uint64_t out_cap, int32_t *status /* [n] */,
                                   uint64_t *bytes /* [n] */);
    int och_geotiff_reader_read(och_geotiff_reader *r, int64_t n, const uint8_t *streams, const uint64_t *offsets /* [n + 1] */,
                                int64_t row0, int64_t rows, void *raster, int on_device, int64_t *bad_tile);
    int64_t och_geotiff_reader_launches(och_geotiff_reader *r);
    void och_geotiff_reader_destroy(och_geotiff_reader *r);
    const char *och_geotiff_read_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
