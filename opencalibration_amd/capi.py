"""ctypes binding of libochip.so (include/ochip.h).  No fallbacks: if the library is missing or no
gfx950 device is present the calls raise."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libochip.so")

K_MATCH, K_RANSAC, K_RELAX_EVAL, K_RELAX_SOLVE, K_AKAZE = 0, 1, 2, 3, 4
NO_SECOND = 0xFFFF

PAIR_DTYPE = np.dtype([("image_1", np.uint32), ("image_2", np.uint32)])
MATCH_DTYPE = np.dtype([("best_k", np.uint32), ("best_count", np.uint16), ("second_count", np.uint16)])
RANSAC_JOB_DTYPE = np.dtype([("image_1", np.uint32), ("image_2", np.uint32), ("n", np.uint32), ("rng_state", np.uint32),
                             ("match_offset", np.uint64), ("eval_offset", np.uint64)])
RANSAC_MATCH_DTYPE = np.dtype([("k1", np.uint32), ("k2", np.uint32), ("count", np.uint16), ("reserved", np.uint16)])
RANSAC_RESULT_DTYPE = np.dtype([("H", np.float64, (9,)), ("score", np.float64), ("iterations", np.uint32), ("n_inliers", np.uint32),
                                ("improvements", np.uint32), ("reserved", np.uint32)])
DECOMPOSITION_DTYPE = np.dtype([("pose", np.float64, (4, 8)), ("can_decompose", np.uint32), ("n_inliers", np.uint32)])

# every symbol include/ochip.h declares; tests check that the built library exports all of them
EXPORTS = [
    "ochip_ctx_create", "ochip_ctx_destroy", "ochip_ctx_sibling", "ochip_ctx_attachment", "ochip_akaze_progress", "ochip_ctx_set_priority", "ochip_last_error", "ochip_device_info", "ochip_synchronize",
    "ochip_descriptors_reserve", "ochip_upload_descriptors", "ochip_descriptor_count",
    "ochip_match_batch", "ochip_match_launch", "ochip_match_fetch",
    "ochip_upload_keypoints", "ochip_ransac_homography_batch", "ochip_refit_homography_batch", "ochip_ransac_epipolar_batch",
    "ochip_upload_batch", "ochip_host_alloc", "ochip_host_free", "ochip_akaze_batch", "ochip_akaze_batch_dev", "ochip_debug_working_image", "ochip_akaze_features", "ochip_akaze_features_dev", "ochip_feature_lists_from_keypoints",
    "ochip_synth_views_alloc", "ochip_synth_views_free", "ochip_synth_render_views", "ochip_synth_views_read",
    "ochip_relax_problem_create", "ochip_relax_problem_destroy", "ochip_relax_set_cameras_constant",
    "ochip_relax_solve", "ochip_relax_get_state", "ochip_relax_set_shard", "ochip_relax_evaluate",
    "ochip_plane_setup_create", "ochip_plane_setup_override", "ochip_plane_setup_blocks", "ochip_plane_setup_destroy",
    "ochip_plane_chain_create", "ochip_plane_chain_run", "ochip_plane_chain_trace", "ochip_plane_chain_destroy",
    "ochip_relaxg_problem_create", "ochip_relaxg_problem_destroy", "ochip_relaxg_set_structure_only", "ochip_relaxg_solve",
    "ochip_relaxg_get_state", "ochip_relaxg_evaluate", "ochip_relaxg_set_exchange",
    "ochip_relaxp_problem_create", "ochip_relaxp_problem_destroy", "ochip_relaxp_set_structure_only", "ochip_relaxp_solve",
    "ochip_relaxp_get_state", "ochip_relaxp_evaluate", "ochip_relaxp_step",
    "ochip_profile_reset", "ochip_profile_get", "ochip_match_work", "ochip_relax_work", "ochip_relax_memory", "ochip_work_counters",
    "ochip_debug_fp64", "ochip_debug_std_sort", "ochip_debug_lm_step", "ochip_debug_homography_fit4", "ochip_debug_decompose_votes", "ochip_match_sort", "ochip_ransac_homography_batch_sorted", "ochip_edge_lists",
    "ochip_dense_index_create", "ochip_dense_index_destroy", "ochip_dense_match", "ochip_dense_link", "ochip_dense_triangulate",
    "ochip_rccl_unique_id", "ochip_rccl_comm_create", "ochip_rccl_comm_destroy", "ochip_rccl_comm_stats",
    "ochip_rccl_relax_exchange",
    "ochip_ortho_mesh_create", "ochip_ortho_mesh_destroy", "ochip_ortho_dsm", "ochip_ortho_thumbnail", "ochip_ortho_layers",
    "ochip_ortho_blend", "ochip_laplacian_blend",
    "ochip_ortho_band_cameras", "ochip_image_slots_create", "ochip_image_slots_destroy", "ochip_image_slots_address",
    "ochip_image_slots_upload", "ochip_image_slots_mark", "ochip_image_slots_wait", "ochip_image_slots_elapsed",
    "ochip_color_balance_solve", "ochip_color_balance_evaluate",
    "ochip_thumbnail_size", "ochip_image_thumbnails", "ochip_debug_lab_table",
    "ochip_ortho_overviews_levels", "ochip_ortho_overviews_create", "ochip_ortho_overviews_feed",
    "ochip_ortho_overviews_complete_rows", "ochip_ortho_overviews_finish", "ochip_ortho_overviews_destroy",
    "ochip_mesh_points_create", "ochip_mesh_points_size", "ochip_mesh_points_count", "ochip_mesh_points_where",
    "ochip_mesh_points_destroy",
    "ochip_ortho_tile_thumb_dims", "ochip_ortho_tile_thumbs", "ochip_ortho_tile_thumbs_enqueue", "ochip_ortho_tile_thumbs_wait",
    "ochip_ortho_tile_thumbs_release",
    "ochip_xyz_export_create", "ochip_xyz_export_create_from_points", "ochip_xyz_export_size", "ochip_xyz_export_bounds",
    "ochip_xyz_export_text_size", "ochip_xyz_export_text", "ochip_xyz_export_destroy", "ochip_debug_format_g6",
    "ochip_jpeg_create", "ochip_jpeg_feed", "ochip_jpeg_pending", "ochip_jpeg_collect", "ochip_jpeg_finish", "ochip_jpeg_destroy",
    "ochip_jpeg_decoder_create", "ochip_jpeg_decoder_decode", "ochip_jpeg_decoder_destroy",
    "ochip_geotiff_create", "ochip_geotiff_feed", "ochip_geotiff_payloads", "ochip_geotiff_collect", "ochip_geotiff_finish",
    "ochip_geotiff_destroy", "ochip_geotiff_create_layered",
    "ochip_geotiff_reader_create", "ochip_geotiff_reader_inflate", "ochip_geotiff_reader_read", "ochip_geotiff_reader_launches",
    "ochip_geotiff_reader_destroy", "ochip_geotiff_reader_create_layered",
    "ochip_png_encoder_create", "ochip_png_encoder_encode", "ochip_png_encoder_destroy",
]

_lib = None


class PngImage(C.Structure):
    """include/ochip.h: ochip_png_image"""
    _fields_ = [("pixels", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("channels", C.c_int32),
                ("swap_rb", C.c_int32)]


class RelaxDesc(C.Structure):
    """include/ochip.h: ochip_relax_desc"""
    _fields_ = [("n_cams", C.c_uint32), ("cam_pos", C.c_void_p), ("cam_q", C.c_void_p), ("cam_optimize", C.c_void_p),
                ("plane_xy", C.c_double * 6), ("plane_z", C.c_double * 3), ("z_optimize", C.c_uint8 * 3),
                ("n_blocks", C.c_uint32), ("blk_cam_a", C.c_void_p), ("blk_cam_b", C.c_void_p), ("blk_rays", C.c_void_p),
                ("n_prior", C.c_uint32), ("prior_cam", C.c_void_p), ("huber_a", C.c_double), ("prior_weight", C.c_double)]


class RelaxOptions(C.Structure):
    """include/ochip.h: ochip_relax_options"""
    _fields_ = [("max_num_iterations", C.c_int), ("initial_trust_region_radius", C.c_double),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double)]


class RelaxSummary(C.Structure):
    """include/ochip.h: ochip_relax_summary"""
    _fields_ = [("termination", C.c_int), ("iterations", C.c_int), ("successful_steps", C.c_int),
                ("unsuccessful_steps", C.c_int), ("num_parameters", C.c_int), ("num_residual_blocks", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double)]


def relax_desc(scene):
    """(RelaxDesc, arrays it points into) of a dict holding the ochip_relax_desc fields by name: cam_pos, cam_q,
    cam_optimize, plane_xy (6), plane_z (3), z_optimize (3), blk_cam_a, blk_cam_b, blk_rays (n_blocks x 6), prior_cam,
    huber_a, prior_weight"""
    d = RelaxDesc()
    keep = []

    def arr(name, dtype):
        a = np.ascontiguousarray(scene[name], dtype).reshape(-1)
        a = a if a.size else np.zeros(1, dtype)
        keep.append(a)
        return a.ctypes.data

    d.n_cams = len(scene["cam_pos"])
    d.cam_pos, d.cam_q, d.cam_optimize = arr("cam_pos", np.float64), arr("cam_q", np.float64), arr("cam_optimize", np.uint8)
    for i in range(6):
        d.plane_xy[i] = float(np.reshape(scene["plane_xy"], -1)[i])
    for i in range(3):
        d.plane_z[i] = float(scene["plane_z"][i])
        d.z_optimize[i] = int(scene["z_optimize"][i])
    d.n_blocks = len(scene["blk_cam_a"])
    d.blk_cam_a, d.blk_cam_b = arr("blk_cam_a", np.uint32), arr("blk_cam_b", np.uint32)
    d.blk_rays = arr("blk_rays", np.float64)
    d.n_prior, d.prior_cam = len(scene["prior_cam"]), arr("prior_cam", np.uint32)
    d.huber_a, d.prior_weight = scene["huber_a"], scene["prior_weight"]
    return d, keep


class RelaxgDesc(C.Structure):
    """include/ochip.h: ochip_relaxg_desc"""
    _fields_ = [("n_cams", C.c_uint32), ("cam_pos", C.c_void_p), ("cam_q", C.c_void_p), ("cam_optimize", C.c_void_p),
                ("n_verts", C.c_uint32), ("vert_xy", C.c_void_p), ("vert_z", C.c_void_p), ("vert_optimize", C.c_void_p),
                ("n_blocks", C.c_uint32), ("blk_n", C.c_void_p), ("blk_intr", C.c_void_p), ("blk_ray_off", C.c_void_p),
                ("blk_tri", C.c_void_p), ("ray_cam", C.c_void_p), ("ray_dir", C.c_void_p), ("ray_px", C.c_void_p),
                ("n_down", C.c_uint32), ("down_cam", C.c_void_p), ("down_weight", C.c_double),
                ("n_diff", C.c_uint32), ("diff_v", C.c_void_p), ("diff_weight", C.c_double), ("anchor_weight", C.c_double),
                ("n_smooth", C.c_uint32), ("smooth_v", C.c_void_p), ("smooth_weight", C.c_double), ("huber_a", C.c_double),
                ("model", C.c_double * 8), ("opt_focal", C.c_uint8), ("opt_principal", C.c_uint8), ("n_radial_free", C.c_uint8),
                ("focal_lo", C.c_double), ("focal_hi", C.c_double), ("mono_observations", C.c_uint32), ("mono_r_max", C.c_double),
                ("shard_rank", C.c_uint32), ("shard_world", C.c_uint32),
                ("n_rel", C.c_uint32), ("rel_cam", C.c_void_p), ("rel_pose", C.c_void_p), ("rel_huber_a", C.c_double)]


def relaxg_desc(scene):
    """(RelaxgDesc, arrays it points into) of a scene dict holding the ochip_relaxg_desc fields by name: cam_pos, cam_q,
    cam_optimize, vert_xy, vert_z, vert_optimize, blk_n, blk_ray_off, blk_tri, ray_cam, ray_dir, down_cam, down_weight,
    diff_v, diff_weight, anchor_weight, huber_a, model; optional blk_intr, ray_px, smooth_v, smooth_weight, opt_focal,
    opt_principal, n_radial_free, focal_lo, focal_hi, mono_observations, mono_r_max, rel_cam, rel_pose, rel_huber_a (absent:
    none / zero)."""
    d = RelaxgDesc()
    keep = []

    def arr(name, dtype):
        if scene.get(name) is None:
            return None
        a = np.ascontiguousarray(scene[name], dtype)
        keep.append(a)
        return a.ctypes.data

    d.n_cams = len(scene["cam_pos"])
    d.cam_pos, d.cam_q, d.cam_optimize = arr("cam_pos", np.float64), arr("cam_q", np.float64), arr("cam_optimize", np.uint8)
    d.n_verts = len(scene["vert_z"])
    d.vert_xy, d.vert_z, d.vert_optimize = arr("vert_xy", np.float64), arr("vert_z", np.float64), arr("vert_optimize", np.uint8)
    d.n_blocks = len(scene["blk_n"])
    d.blk_n, d.blk_ray_off, d.blk_tri = arr("blk_n", np.uint8), arr("blk_ray_off", np.uint32), arr("blk_tri", np.uint32)
    d.blk_intr, d.ray_px = arr("blk_intr", np.uint8), arr("ray_px", np.float64)
    d.ray_cam, d.ray_dir = arr("ray_cam", np.uint32), arr("ray_dir", np.float64)
    d.n_down, d.down_cam, d.down_weight = len(scene["down_cam"]), arr("down_cam", np.uint32), scene["down_weight"]
    d.n_diff, d.diff_v, d.diff_weight = np.size(scene["diff_v"]) // 2, arr("diff_v", np.uint32), scene["diff_weight"]
    d.anchor_weight, d.huber_a = scene["anchor_weight"], scene["huber_a"]
    if scene.get("smooth_v") is not None:
        d.n_smooth, d.smooth_v, d.smooth_weight = np.size(scene["smooth_v"]) // 4, arr("smooth_v", np.uint32), scene["smooth_weight"]
    for i, v in enumerate(scene["model"]):
        d.model[i] = v
    d.opt_focal, d.opt_principal = int(scene.get("opt_focal", 0)), int(scene.get("opt_principal", 0))
    d.n_radial_free = int(scene.get("n_radial_free", 0))
    d.focal_lo, d.focal_hi = scene.get("focal_lo", 100.0), scene.get("focal_hi", 20000.0)
    d.mono_observations, d.mono_r_max = int(scene.get("mono_observations", 0)), scene.get("mono_r_max", 0.0)
    if scene.get("rel_cam") is not None:
        d.n_rel, d.rel_cam, d.rel_pose = np.size(scene["rel_cam"]) // 2, arr("rel_cam", np.uint32), arr("rel_pose", np.float64)
        d.rel_huber_a = scene["rel_huber_a"]
    return d, keep


class RelaxpDesc(C.Structure):
    """include/ochip.h: ochip_relaxp_desc"""
    _fields_ = [("n_cams", C.c_uint32), ("cam_pos", C.c_void_p), ("cam_q", C.c_void_p), ("cam_optimize", C.c_void_p),
                ("n_points", C.c_uint32), ("point_xyz", C.c_void_p), ("n_groups", C.c_uint32), ("grp_first", C.c_void_p),
                ("grp_cam", C.c_void_p), ("obs_px", C.c_void_p), ("functor", C.c_int), ("model", C.c_double * 8),
                ("opt_focal", C.c_uint8), ("opt_principal", C.c_uint8), ("n_radial_free", C.c_uint8),
                ("focal_lo", C.c_double), ("focal_hi", C.c_double), ("huber_a", C.c_double),
                ("mono_observations", C.c_uint32), ("mono_r_max", C.c_double)]


def relaxp_desc(scene):
    """(RelaxpDesc, arrays it points into) of a scene dict holding the ochip_relaxp_desc fields by name: cam_pos, cam_q,
    cam_optimize, point_xyz, grp_first (n_groups + 1), grp_cam, obs_px, functor, model, huber_a; optional opt_focal,
    opt_principal, n_radial_free, focal_lo, focal_hi, mono_observations, mono_r_max (absent: zero / 100, 20000)."""
    d = RelaxpDesc()
    keep = []

    def arr(name, dtype):
        a = np.ascontiguousarray(scene[name], dtype).reshape(-1)
        a = a if a.size else np.zeros(1, dtype)
        keep.append(a)
        return a.ctypes.data

    d.n_cams = len(scene["cam_pos"])
    d.cam_pos, d.cam_q, d.cam_optimize = arr("cam_pos", np.float64), arr("cam_q", np.float64), arr("cam_optimize", np.uint8)
    d.n_points, d.point_xyz = np.size(scene["point_xyz"]) // 3, arr("point_xyz", np.float64)
    d.n_groups = np.size(scene["grp_cam"]) // 2
    d.grp_first, d.grp_cam, d.obs_px = arr("grp_first", np.uint32), arr("grp_cam", np.uint32), arr("obs_px", np.float64)
    assert np.size(scene["grp_first"]) == d.n_groups + 1 and np.size(scene["obs_px"]) == 4 * d.n_points
    d.functor, d.huber_a = int(scene["functor"]), float(scene["huber_a"])
    for i, v in enumerate(scene["model"]):
        d.model[i] = v
    d.opt_focal, d.opt_principal = int(scene.get("opt_focal", 0)), int(scene.get("opt_principal", 0))
    d.n_radial_free = int(scene.get("n_radial_free", 0))
    d.focal_lo, d.focal_hi = scene.get("focal_lo", 100.0), scene.get("focal_hi", 20000.0)
    d.mono_observations, d.mono_r_max = int(scene.get("mono_observations", 0)), scene.get("mono_r_max", 0.0)
    return d, keep


class LocateTable(C.Structure):
    """ochip_locate_table (include/ochip.h)."""
    _fields_ = [("n_triangles", C.c_uint32), ("vertex_xy", C.c_void_p), ("neighbours", C.c_void_p), ("plane", C.c_void_p),
                ("centroid_x", C.c_void_p), ("centroid_y", C.c_void_p), ("x0", C.c_double), ("y0", C.c_double), ("cell", C.c_double),
                ("nx", C.c_int32), ("start", C.c_void_p), ("n_start", C.c_size_t), ("items", C.c_void_p), ("n_items", C.c_size_t)]


class OchipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise OchipError(f"{LIB_PATH} is missing: run `python -m opencalibration_amd.build` "
                             "(there is no CPU fallback for the hot path)")
        L = C.CDLL(LIB_PATH)
        vp, u32, u64, i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
        L.ochip_ctx_create.argtypes = [i32, C.POINTER(vp)]
        L.ochip_ctx_destroy.argtypes = [vp]
        L.ochip_ctx_destroy.restype = None
        L.ochip_last_error.argtypes = [vp]
        L.ochip_last_error.restype = C.c_char_p
        L.ochip_device_info.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(i32), C.POINTER(C.c_size_t)]
        L.ochip_synchronize.argtypes = [vp]
        L.ochip_rccl_unique_id.argtypes = [vp, vp]
        L.ochip_rccl_comm_create.argtypes = [vp, vp, u32, u32, C.POINTER(vp)]
        L.ochip_rccl_comm_destroy.argtypes = [vp]
        L.ochip_rccl_comm_destroy.restype = None
        L.ochip_rccl_comm_stats.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.ochip_descriptors_reserve.argtypes = [vp, u32, u64]
        L.ochip_upload_descriptors.argtypes = [vp, u32, vp, u32]
        L.ochip_descriptor_count.argtypes = [vp, u32, C.POINTER(u32)]
        L.ochip_match_batch.argtypes = [vp, vp, u32, vp, vp]
        L.ochip_match_launch.argtypes = [vp, vp, u32, vp, u64]
        L.ochip_match_fetch.argtypes = [vp, vp, u64]
        L.ochip_profile_reset.argtypes = [vp]
        L.ochip_profile_get.argtypes = [vp, i32, C.POINTER(u64), C.POINTER(C.c_double)]
        L.ochip_match_work.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
        L.ochip_relax_work.argtypes = [vp, C.POINTER(C.c_double)]
        L.ochip_relax_memory.argtypes = [vp, C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        L.ochip_debug_fp64.argtypes = [vp, i32, vp, vp, C.c_size_t, vp]
        L.ochip_debug_std_sort.argtypes = [vp, vp, vp, vp, u32, vp, vp, vp]
        L.ochip_debug_lm_step.argtypes = [vp, i32, vp, vp, vp, vp, C.c_double, vp, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp]
        L.ochip_debug_homography_fit4.argtypes = [vp, i32, vp, u32, vp, vp, vp]
        L.ochip_debug_decompose_votes.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp]
        L.ochip_upload_batch.argtypes = [vp, u32, vp, vp, vp, vp]
        L.ochip_refit_homography_batch.argtypes = [vp, vp, u32, vp, u64, u32, C.c_double, vp, vp]
        L.ochip_akaze_batch.argtypes = [vp, vp, u32, i32, i32, u32, vp, vp, vp, vp]
        L.ochip_feature_lists_from_keypoints.argtypes = [vp, vp, vp, vp, u32, u32, i32, i32, C.c_double, C.c_double, vp]
        L.ochip_akaze_batch_dev.argtypes = [vp, vp, u32, i32, i32, u32, vp, vp, vp, vp]
        L.ochip_debug_working_image.argtypes = [vp, vp, i32, u32, i32, i32, vp, vp, vp]
        L.ochip_synth_views_alloc.argtypes = [vp, u32, i32, i32, C.POINTER(vp)]
        L.ochip_synth_views_free.argtypes = [vp, vp]
        L.ochip_synth_views_free.restype = None
        L.ochip_synth_render_views.argtypes = [vp, vp, u32, u32, i32, i32, vp, vp, vp, vp, u32]
        L.ochip_synth_views_read.argtypes = [vp, vp, u32, i32, i32, vp]
        L.ochip_ortho_mesh_destroy.argtypes = [vp]
        L.ochip_ortho_mesh_destroy.restype = None
        L.ochip_laplacian_blend.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp]
        L.ochip_color_balance_solve.argtypes = [vp, vp, C.c_uint64, vp, u32, vp, u32, vp, vp, vp]
        L.ochip_color_balance_evaluate.argtypes = [vp, vp, C.c_uint64, vp, u32, vp, u32, vp, vp, vp, vp, vp, vp, vp, vp]
        L.ochip_thumbnail_size.argtypes = [i32, i32, vp, vp]
        L.ochip_image_thumbnails.argtypes = [vp, vp, u32, i32, i32, i32, vp]
        L.ochip_debug_lab_table.argtypes = [vp, vp, C.c_size_t, vp, vp]
        L.ochip_ortho_overviews_levels.argtypes = [C.c_int64, C.c_int64, vp]
        L.ochip_ortho_overviews_create.argtypes = [vp, i32, C.c_int64, C.c_int64, vp, i32, C.POINTER(vp)]
        L.ochip_ortho_overviews_feed.argtypes = [vp, C.c_int64, C.c_int64, vp]
        L.ochip_ortho_overviews_complete_rows.argtypes = [vp, i32]
        L.ochip_ortho_overviews_complete_rows.restype = C.c_int64
        L.ochip_ortho_overviews_finish.argtypes = [vp]
        L.ochip_ortho_overviews_destroy.argtypes = [vp]
        L.ochip_ortho_overviews_destroy.restype = None
        L.ochip_mesh_points_create.argtypes = [vp, vp, u64, C.POINTER(vp)]
        L.ochip_mesh_points_size.argtypes = [vp]
        L.ochip_mesh_points_size.restype = u64
        L.ochip_mesh_points_count.argtypes = [vp, C.POINTER(LocateTable), i32, vp, vp, vp, vp, vp, u64, C.POINTER(u64)]
        L.ochip_mesh_points_where.argtypes = [vp, vp]
        L.ochip_mesh_points_destroy.argtypes = [vp]
        L.ochip_mesh_points_destroy.restype = None
        L.ochip_ortho_tile_thumb_dims.argtypes = [i32, i32, vp]
        L.ochip_ortho_tile_thumbs.argtypes = [vp, i32, i32, C.c_int64, i32, i32, i32, vp, vp, vp]
        L.ochip_ortho_tile_thumbs_enqueue.argtypes = [vp, i32, i32, C.c_int64, i32, i32, i32, vp, vp, C.POINTER(vp)]
        L.ochip_ortho_tile_thumbs_wait.argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        L.ochip_ortho_tile_thumbs_release.argtypes = [vp]
        L.ochip_ortho_tile_thumbs_release.restype = None
        L.ochip_xyz_export_create.argtypes = [vp, vp, u64, C.POINTER(vp)]
        L.ochip_xyz_export_create_from_points.argtypes = [vp, vp, u64, C.POINTER(vp)]
        L.ochip_xyz_export_size.argtypes = [vp]
        L.ochip_xyz_export_size.restype = u64
        L.ochip_xyz_export_bounds.argtypes = [vp, vp]
        L.ochip_xyz_export_text_size.argtypes = [vp, vp, C.POINTER(u64), C.POINTER(u64)]
        L.ochip_xyz_export_text.argtypes = [vp, vp, u64]
        L.ochip_xyz_export_destroy.argtypes = [vp]
        L.ochip_xyz_export_destroy.restype = None
        L.ochip_debug_format_g6.argtypes = [vp, vp, u64, vp, vp]
        L.ochip_jpeg_create.argtypes = [vp, C.c_int64, C.c_int64, i32, C.POINTER(vp)]
        L.ochip_jpeg_feed.argtypes = [vp, C.c_int64, C.c_int64, vp, i32, i32]
        L.ochip_jpeg_pending.argtypes = [vp]
        L.ochip_jpeg_pending.restype = C.c_int64
        L.ochip_jpeg_collect.argtypes = [vp, vp, u64, C.POINTER(u64)]
        L.ochip_jpeg_finish.argtypes = [vp]
        L.ochip_jpeg_destroy.argtypes = [vp]
        L.ochip_jpeg_destroy.restype = None
        L.ochip_jpeg_decoder_create.argtypes = [vp, i32, C.POINTER(vp)]
        L.ochip_jpeg_decoder_decode.argtypes = [vp, C.c_int64, vp, vp, i32, vp, u64, vp, vp, vp]
        L.ochip_jpeg_decoder_destroy.argtypes = [vp]
        L.ochip_jpeg_decoder_destroy.restype = None
        L.ochip_geotiff_create.argtypes = [vp, i32, C.c_int64, C.c_int64, i32, C.POINTER(vp)]
        L.ochip_geotiff_create_layered.argtypes = [vp, i32, i32, C.c_int64, C.c_int64, i32, C.POINTER(vp)]
        L.ochip_geotiff_feed.argtypes = [vp, C.c_int64, C.c_int64, vp, i32]
        L.ochip_geotiff_payloads.argtypes = [vp, vp, C.c_int64]
        L.ochip_geotiff_collect.argtypes = [vp, vp, u64, C.POINTER(u64), vp, u64, C.POINTER(u64)]
        L.ochip_geotiff_finish.argtypes = [vp]
        L.ochip_geotiff_destroy.argtypes = [vp]
        L.ochip_geotiff_destroy.restype = None
        L.ochip_geotiff_reader_create.argtypes = [vp, i32, i32, C.c_int64, C.c_int64, i32, i32, i32, u64, C.POINTER(vp)]
        L.ochip_geotiff_reader_create_layered.argtypes = [vp, i32, i32, C.c_int64, C.c_int64, i32, i32, i32, u64, C.POINTER(vp)]
        L.ochip_geotiff_reader_inflate.argtypes = [vp, C.c_int64, vp, vp, vp, vp, u64, vp, vp]
        L.ochip_geotiff_reader_read.argtypes = [vp, C.c_int64, vp, vp, C.c_int64, C.c_int64, vp, i32, C.POINTER(C.c_int64)]
        L.ochip_geotiff_reader_launches.argtypes = [vp]
        L.ochip_geotiff_reader_launches.restype = C.c_int64
        L.ochip_geotiff_reader_destroy.argtypes = [vp]
        L.ochip_geotiff_reader_destroy.restype = None
        L.ochip_png_encoder_create.argtypes = [vp, C.POINTER(vp)]
        L.ochip_png_encoder_encode.argtypes = [vp, C.c_int64, vp, i32, i32, vp, u64, vp]
        L.ochip_png_encoder_destroy.argtypes = [vp]
        L.ochip_png_encoder_destroy.restype = None
        _lib = L
    return _lib


class RcclComm:
    """ochip_rccl_comm: all-gathers on the owning context's stream (include/ochip.h)."""

    def __init__(self, ctx, unique_id, rank, world):
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        self.h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(unique_id)
        ctx._check(ctx.L.ochip_rccl_comm_create(ctx.h, buf, self.rank, self.world, C.byref(self.h)), "ochip_rccl_comm_create")

    @property
    def exchange(self):
        """(function pointer, user pointer) for ochip_relax_set_shard."""
        return C.cast(self.ctx.L.ochip_rccl_relax_exchange, C.c_void_p).value, self.h

    def stats(self):
        n, b = C.c_uint64(), C.c_uint64()
        self.ctx._check(self.ctx.L.ochip_rccl_comm_stats(self.h, C.byref(n), C.byref(b)), "ochip_rccl_comm_stats")
        return {"exchanges": n.value, "bytes_gathered": b.value}

    def close(self):
        if self.h:
            self.ctx.L.ochip_rccl_comm_destroy(self.h)
            self.h = C.c_void_p()


class MeshPoints:
    """ochip_mesh_points: a cloud on the device, counted against flat locate tables (host.Surface.locate_table())."""

    def __init__(self, ctx, xyz):
        self.ctx, self.L = ctx, ctx.L
        xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        self.n = len(xyz)
        self.h = C.c_void_p()
        ctx._check(self.L.ochip_mesh_points_create(ctx.h, xyz.ctypes.data if self.n else None, self.n, C.byref(self.h)),
                   "ochip_mesh_points_create")
        self.raw = self.h.value # kept after close(): what a caller that held on to the handle would pass

    def count(self, table, max_steps=100, handle=None):
        """Per triangle count, first point, sum, sum of squares; the exhausted points; the per-point result."""
        T = len(table["vertex_xy"])
        keep = {k: np.ascontiguousarray(table[k]) for k in ("vertex_xy", "neighbours", "plane", "cx", "cy", "start", "items")}
        ptr = lambda a: a.ctypes.data if a.size else None
        t = LocateTable(T, ptr(keep["vertex_xy"]), ptr(keep["neighbours"]), ptr(keep["plane"]), ptr(keep["cx"]), ptr(keep["cy"]),
                        table["x0"], table["y0"], table["cell"], table["nx"], ptr(keep["start"]), len(keep["start"]), ptr(keep["items"]),
                        len(keep["items"]))
        count, first = np.zeros(max(T, 1), np.uint32), np.zeros(max(T, 1), np.uint32)
        s, ss, ex, nex = np.zeros(max(T, 1)), np.zeros(max(T, 1)), np.zeros(max(self.n, 1), np.uint32), C.c_uint64(0)
        h = self.h if handle is None else C.c_void_p(handle)
        rc = self.L.ochip_mesh_points_count(h, C.byref(t), max_steps, count.ctypes.data, first.ctypes.data, s.ctypes.data, ss.ctypes.data,
                                            ex.ctypes.data, len(ex), C.byref(nex))
        if rc != 0:
            text = self.L.ochip_last_error(self.ctx.h).decode() + " | " + self.L.ochip_last_error(None).decode()
            raise OchipError(f"ochip_mesh_points_count = {rc}: {text}")
        where = np.zeros(max(self.n, 1), np.uint32)
        self.ctx._check(self.L.ochip_mesh_points_where(h, where.ctypes.data), "ochip_mesh_points_where")
        return dict(count=count[:T], first=first[:T], sum=s[:T], sum_sq=ss[:T], exhausted=ex[:nex.value], where=where[:self.n])

    def close(self):
        if self.h:
            self.L.ochip_mesh_points_destroy(self.h)
            self.h = C.c_void_p()


def bounds6(bounds):
    """A box ((lo, hi),) * 3 as the int64 array of ochip_xyz_export_text_size; None stays None (no filter)."""
    if bounds is None:
        return None
    b = np.ascontiguousarray(bounds, np.int64).reshape(-1)
    if b.size != 6:
        raise ValueError("bounds: three (first, second) pairs")
    return b


class XyzExport:
    """ochip_xyz_export: a flat cloud on the device, written out as the reference's point cloud file (DESIGN.md section
    4.16).  bounds(): filterOutliers' box as ((lo, hi),) * 3; text(bounds): toXYZ's bytes for a box (None: no filter)."""

    def __init__(self, ctx, xyz, _points=None):
        self.ctx, self.L = ctx, ctx.L
        self.h = C.c_void_p()
        if _points is None:
            xyz = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
            ctx._check(self.L.ochip_xyz_export_create(ctx.h, xyz.ctypes.data if len(xyz) else None, len(xyz), C.byref(self.h)),
                       "ochip_xyz_export_create")
        else:
            arr = (C.c_void_p * max(len(_points), 1))(*_points)
            ctx._check(self.L.ochip_xyz_export_create_from_points(ctx.h, arr, len(_points), C.byref(self.h)),
                       "ochip_xyz_export_create_from_points")
        self.raw = self.h.value  # kept after close(): what a caller that held on to the handle would pass
        self.n = self.L.ochip_xyz_export_size(self.h)
        self.kept = 0

    @classmethod
    def from_points(cls, ctx, points):
        """The clouds of live MeshPoints objects (or raw handles) in the given order, copied on the device."""
        return cls(ctx, None, _points=[p.h.value if isinstance(p, MeshPoints) else p for p in points])

    def _call(self, rc, what):
        if rc != 0:
            text = self.L.ochip_last_error(self.ctx.h).decode() + " | " + self.L.ochip_last_error(None).decode()
            raise OchipError(f"{what} = {rc}: {text}")

    def bounds(self, handle=None):
        b = np.zeros(6, np.int64)
        h = self.h if handle is None else C.c_void_p(handle)
        self._call(self.L.ochip_xyz_export_bounds(h, b.ctypes.data), "ochip_xyz_export_bounds")
        return tuple((int(b[2 * a]), int(b[2 * a + 1])) for a in range(3))

    def text_size(self, bounds=None, handle=None):
        b = bounds6(bounds)
        nbytes, kept = C.c_uint64(0), C.c_uint64(0)
        h = self.h if handle is None else C.c_void_p(handle)
        self._call(self.L.ochip_xyz_export_text_size(h, b.ctypes.data if b is not None else None, C.byref(nbytes), C.byref(kept)),
                   "ochip_xyz_export_text_size")
        self.kept = kept.value
        return nbytes.value, kept.value

    def text(self, bounds=None, cap=None):
        """The file's bytes; cap: the room offered to ochip_xyz_export_text (default: exactly what text_size said)."""
        nbytes, _ = self.text_size(bounds)
        cap = nbytes if cap is None else cap
        out = np.zeros(max(cap, 1), np.uint8)
        self._call(self.L.ochip_xyz_export_text(self.h, out.ctypes.data, cap), "ochip_xyz_export_text")
        return out[:nbytes].tobytes()

    def close(self):
        if self.h:
            self.L.ochip_xyz_export_destroy(self.h)
            self.h = C.c_void_p()


PLANE_EDGE_DTYPE = np.dtype([("cam_a", np.uint32), ("cam_b", np.uint32), ("model_a", np.uint32), ("model_b", np.uint32),
                             ("n_inliers", np.uint32), ("flags", np.uint32), ("inlier_offset", np.uint64), ("H", np.float64, (9,))])
PLANE_INLIER_DTYPE = np.dtype([("px1", np.float64, (2,)), ("px2", np.float64, (2,)), ("descriptor_score", np.float64)])
PLANE_CHAIN_STEP_DTYPE = np.dtype([("cam", np.uint32), ("mode", np.uint32), ("n_filter", np.uint32), ("prev_cam", np.int32),
                                   ("prev_q", np.float64, (4,)), ("tri_xy", np.float64, (6,)), ("z0", np.float64)])
PLANE_CHAIN_RESULT_DTYPE = np.dtype([("steps_done", np.uint32), ("status", np.int32), ("solves", np.int32),
                                     ("iterations_total", np.int32), ("last_iterations", np.int32),
                                     ("last_residual_blocks", np.int32), ("last_initial_cost", np.float64),
                                     ("last_final_cost", np.float64), ("grid_syncs", np.int32), ("workgroups", np.int32),
                                     ("plane_z", np.float64, (3,))])
TR_SETUP, TR_EVAL, TR_SOLVE, TR_FINISH = 1, 2, 3, 4


def parse_chain_trace(words):
    """The events of ochip_plane_chain_trace's buffer (its filled words) as dicts: kind, index, step and the payload of the
    kind by name (csrc/relax_chain.hip: trace_setup, trace_eval, trace_solve, trace_finish).  Counts are ints, A and L are
    dense lower triangles (L with the augmented row: (n + 1) x n), blk_idx a list of one array per edge."""
    w = np.asarray(words, np.float64)
    out, at = [], 0

    def take(p, k, dtype=np.float64):
        v = p[take.at:take.at + k]
        take.at += k
        return v.copy() if dtype is np.float64 else v.astype(dtype)

    while at < len(w):
        kind, size, index, step = (int(v) for v in w[at:at + 4])
        assert size >= 4 and at + size <= len(w), (at, size, len(w))
        p = w[at + 4:at + size]
        at += size
        ev = dict(kind=kind, index=index, step=step)
        take.at = 0
        if kind == TR_SETUP:
            names = ("complete", "mode", "cam", "n_filter", "n_blocks", "n_prior", "n_live", "n_cams", "n_edges", "n_keep", "n_idx",
                     "cur")
            ev.update({k: int(v) for k, v in zip(names, take(p, 12))})
            ev["plane_xy"], ev["z"] = take(p, 6), take(p, 3)
            nc, ne = ev["n_cams"], ev["n_edges"]
            ev["q"] = take(p, 4 * nc).reshape(nc, 4)
            ev["blk_cnt"], ev["inexact"] = take(p, ne, np.int64), take(p, ne, np.uint8)
            ev["cam_prior"], ev["cam_blocks"] = take(p, nc, np.uint8), take(p, nc, np.uint8)
            off = take(p, ne + 1, np.int64)
            idx = take(p, ev["n_idx"], np.int64)
            ev["blk_idx"] = [idx[off[e]:off[e] + ev["blk_cnt"][e]] for e in range(ne)] if ev["n_idx"] else [idx[:0]] * ne
            ev["keep"] = take(p, ev["n_keep"], np.uint8)
        elif kind == TR_EVAL:
            names = ("which", "first", "state", "set", "n", "n_active", "nz", "n_cams")
            ev.update({k: int(v) for k, v in zip(names, take(p, 8))})
            ev["cost"] = float(take(p, 1)[0])
            ev["fail_bits"], ev["iter"], ev["has_diag"] = (int(v) for v in take(p, 3))
            ev["z"] = take(p, 3)
            nc, n = ev["n_cams"], ev["n"]
            ev["q"], ev["cam_t"] = take(p, 4 * nc).reshape(nc, 4), take(p, nc, np.int64)
            ev["g"], ev["diagonal"] = take(p, n), take(p, n)
            ev["A"] = np.zeros((n, n))
            ev["A"][np.tril_indices(n)] = take(p, n * (n + 1) // 2)
        elif kind == TR_SOLVE:
            names = ("which", "iter", "tiles", "n", "n_active", "nz", "n_cams", "cur")
            ev.update({k: int(v) for k, v in zip(names, take(p, 8))})
            for k, v in zip(("radius", "mcc"), take(p, 2)):
                ev[k] = float(v)
            ev["chol_fail"] = int(take(p, 1)[0])
            for k, v in zip(("step_norm2", "cand_norm2", "x_norm", "x_cost"), take(p, 4)):
                ev[k] = float(v)
            ev["nbc"] = int(take(p, 1)[0])
            ev["z"] = take(p, 3)
            nc, n = ev["n_cams"], ev["n"]
            ev["q"] = take(p, 4 * nc).reshape(nc, 4)
            ev["scale"], ev["lm_diag"], ev["gs"], ev["x"] = take(p, n), take(p, n), take(p, n), take(p, n)
            if ev["tiles"]:
                L = np.zeros((n + 1, n))
                L[:n][np.tril_indices(n)] = take(p, n * (n + 1) // 2)
                L[n] = take(p, n)
                ev["L"], ev["linv"] = L, take(p, ev["nbc"] * 4096).reshape(ev["nbc"], 64, 64)
        elif kind == TR_FINISH:
            v = take(p, 8)
            ev.update(which=int(v[0]), termination=int(v[1]), iterations=int(v[2]), initial_cost=float(v[3]), final_cost=float(v[4]),
                      successful=int(v[5]), unsuccessful=int(v[6]), radius=float(v[7]))
        else:
            raise OchipError(f"ochip_plane_chain_trace: event {index} of unknown kind {kind}")
        assert take.at == len(p), (kind, take.at, len(p))
        out.append(ev)
    return out


class PlaneChain:
    """An ochip_plane_chain (the NaN bootstrap of runGroundPlane as one resident launch).  edges, inliers, steps: arrays of
    PLANE_EDGE_DTYPE, PLANE_INLIER_DTYPE, PLANE_CHAIN_STEP_DTYPE; models10 [n_models][10]."""

    def __init__(self, ctx, edges, inliers, cam_pos, cam_q, cam_optimize, models10, grid_fraction, huber_a, prior_weight, steps):
        self.ctx, self.L = ctx, ctx.L
        L = self.L
        vp, u32, u64, dbl = C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
        L.ochip_plane_chain_create.argtypes = [vp, vp, u32, vp, u64, vp, vp, vp, u32, vp, u32, dbl, dbl, dbl, vp, u32, C.POINTER(vp)]
        L.ochip_plane_chain_run.argtypes = [vp, C.c_int, vp, vp]
        L.ochip_plane_chain_trace.argtypes = [vp, C.c_int, u64, u64, vp, u64, C.POINTER(u64), C.POINTER(u64), vp, vp, vp]
        L.ochip_plane_chain_destroy.argtypes = [vp]
        L.ochip_plane_chain_destroy.restype = None
        edges = np.ascontiguousarray(edges, PLANE_EDGE_DTYPE)
        inliers = np.ascontiguousarray(inliers, PLANE_INLIER_DTYPE)
        steps = np.ascontiguousarray(steps, PLANE_CHAIN_STEP_DTYPE)
        cam_pos = np.ascontiguousarray(cam_pos, np.float64).reshape(-1, 3)
        cam_q = np.ascontiguousarray(cam_q, np.float64).reshape(-1, 4)
        cam_optimize = np.ascontiguousarray(cam_optimize, np.uint8)
        models10 = np.ascontiguousarray(models10, np.float64).reshape(-1, 10)
        assert len(cam_q) == len(cam_pos) == len(cam_optimize)
        self.n_cams, self.n_inliers = len(cam_pos), len(inliers)
        self.h = vp()
        ctx._check(L.ochip_plane_chain_create(ctx.h, edges.ctypes.data if len(edges) else None, len(edges),
                                              inliers.ctypes.data if len(inliers) else None, len(inliers), cam_pos.ctypes.data,
                                              cam_q.ctypes.data, cam_optimize.ctypes.data, len(cam_pos), models10.ctypes.data,
                                              len(models10), grid_fraction, huber_a, prior_weight,
                                              steps.ctypes.data if len(steps) else None, len(steps), C.byref(self.h)),
                   "ochip_plane_chain_create")

    def run(self, stepped=False):
        """ochip_plane_chain_run: (cam_q [n_cams][4], the result struct as a numpy record)"""
        q, res = np.zeros((self.n_cams, 4)), np.zeros(1, PLANE_CHAIN_RESULT_DTYPE)
        self.ctx._check(self.L.ochip_plane_chain_run(self.h, int(stepped), q.ctypes.data, res.ctypes.data), "ochip_plane_chain_run")
        return q, res[0]

    def trace(self, stepped=False, first_event=0, max_events=2 ** 62, capacity=1 << 22):
        """ochip_plane_chain_trace: dict(cam_q, result, n_events, n_words, events = parse_chain_trace of the filled words,
        rays [n_inliers][6])."""
        q, res = np.zeros((self.n_cams, 4)), np.zeros(1, PLANE_CHAIN_RESULT_DTYPE)
        words, rays = np.zeros(max(int(capacity), 1)), np.zeros((max(self.n_inliers, 1), 6))
        n_events, n_words = C.c_uint64(0), C.c_uint64(0)
        self.ctx._check(self.L.ochip_plane_chain_trace(self.h, int(stepped), int(first_event), int(max_events),
                                                       words.ctypes.data if capacity else None, int(capacity), C.byref(n_events),
                                                       C.byref(n_words), rays.ctypes.data, q.ctypes.data, res.ctypes.data),
                        "ochip_plane_chain_trace")
        return dict(cam_q=q, result=res[0], n_events=int(n_events.value), n_words=int(n_words.value),
                    events=parse_chain_trace(words[:n_words.value]), rays=rays[:self.n_inliers])

    def close(self):
        if getattr(self, "h", None):
            self.L.ochip_plane_chain_destroy(self.h)
            self.h = None


class Context:
    """Owns one ochip_ctx (one GPU)."""

    def plane_setup(self, edges, inliers, cam_pos, cam_q, models10, triangle_xy6, grid_fraction):
        """ochip_plane_setup_create + ochip_plane_setup_blocks + destroy: dict(keep [n_inliers], inexact [n_edges], blk_cam_a,
        blk_cam_b, blk_rays [n_blocks][6]); the blocks are None when an edge is inexact."""
        L = self.L
        vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
        L.ochip_plane_setup_create.argtypes = [vp, vp, u32, vp, u64, vp, vp, u32, vp, u32, vp, C.c_double, vp, vp, C.POINTER(vp)]
        L.ochip_plane_setup_blocks.argtypes = [vp, vp, vp, vp, u64, C.POINTER(u64)]
        L.ochip_plane_setup_destroy.argtypes = [vp]
        L.ochip_plane_setup_destroy.restype = None
        edges = np.ascontiguousarray(edges, PLANE_EDGE_DTYPE)
        inliers = np.ascontiguousarray(inliers, PLANE_INLIER_DTYPE)
        cam_pos = np.ascontiguousarray(cam_pos, np.float64).reshape(-1, 3)
        cam_q = np.ascontiguousarray(cam_q, np.float64).reshape(-1, 4)
        models10 = np.ascontiguousarray(models10, np.float64).reshape(-1, 10)
        tri = np.ascontiguousarray(triangle_xy6, np.float64).reshape(6)
        keep, inexact = np.zeros(max(len(inliers), 1), np.uint8), np.zeros(max(len(edges), 1), np.uint8)
        h = vp()
        self._check(L.ochip_plane_setup_create(self.h, edges.ctypes.data, len(edges), inliers.ctypes.data, len(inliers),
                                               cam_pos.ctypes.data, cam_q.ctypes.data, len(cam_pos), models10.ctypes.data, len(models10),
                                               tri.ctypes.data, grid_fraction, keep.ctypes.data, inexact.ctypes.data, C.byref(h)),
                    "ochip_plane_setup_create")
        out = dict(keep=keep[:len(inliers)], inexact=inexact[:len(edges)], blk_cam_a=None, blk_cam_b=None, blk_rays=None)
        try:
            if not inexact.any():
                n = u64(0)
                self._check(L.ochip_plane_setup_blocks(h, None, None, None, 0, C.byref(n)), "ochip_plane_setup_blocks")
                a, b, r = np.zeros(max(n.value, 1), np.uint32), np.zeros(max(n.value, 1), np.uint32), np.zeros((max(n.value, 1), 6))
                self._check(L.ochip_plane_setup_blocks(h, a.ctypes.data, b.ctypes.data, r.ctypes.data, n.value, C.byref(n)),
                            "ochip_plane_setup_blocks")
                out.update(blk_cam_a=a[:n.value], blk_cam_b=b[:n.value], blk_rays=r[:n.value])
        finally:
            L.ochip_plane_setup_destroy(h)
        return out

    def __init__(self, device=0):
        self.L = load()
        h = C.c_void_p()
        rc = self.L.ochip_ctx_create(device, C.byref(h))
        if rc != 0:
            raise OchipError(f"ochip_ctx_create({device}) = {rc}: {self.L.ochip_last_error(None).decode()}")
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self.L.ochip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise OchipError(f"{what} = {rc}: {self.L.ochip_last_error(self.h).decode()}")

    def lab_table(self, codes):
        """The thumbnail pass's table of all BGR codes (filled on first use) at `codes` (B | G << 8 | R << 16): the 8-bit Lab as
        L | a << 8 | b << 16, and the milliseconds its one fill launch took."""
        codes = np.ascontiguousarray(codes, np.uint32).reshape(-1)
        out, ms = np.zeros(len(codes), np.uint32), C.c_float(0)
        self._check(self.L.ochip_debug_lab_table(self.h, codes.ctypes.data, len(codes), out.ctypes.data, C.byref(ms)),
                    "ochip_debug_lab_table")
        return out, float(ms.value)

    def format_g6(self, values):
        """The device's number formatter alone (ochip_debug_format_g6): (text [n] of S16, lengths [n]; 0 = declined)."""
        v = np.ascontiguousarray(values, np.float64).reshape(-1)
        text, ln = np.zeros((max(len(v), 1), 16), np.uint8), np.zeros(max(len(v), 1), np.uint8)
        self._check(self.L.ochip_debug_format_g6(self.h, v.ctypes.data if len(v) else None, len(v), text.ctypes.data, ln.ctypes.data),
                    "ochip_debug_format_g6")
        return text[:len(v)].view("S16").reshape(-1), ln[:len(v)]

    def sibling(self, index):
        """The index-th sibling context (same device, own streams and scratch; owned by this context): independent work
        submitted through it overlaps with this context's."""
        h = C.c_void_p()
        self._check(self.L.ochip_ctx_sibling(self.h, index, C.byref(h)), "ochip_ctx_sibling")
        s = Context.__new__(Context)
        s.L, s.h, s._owner = self.L, h, self
        s.close = lambda: None          # the owner destroys it
        return s

    def rccl_unique_id(self):
        """ncclGetUniqueId as bytes (rank 0 draws it and hands it to the other ranks)."""
        buf = (C.c_uint8 * 128)()
        self._check(self.L.ochip_rccl_unique_id(self.h, buf), "ochip_rccl_unique_id")
        return bytes(buf)

    def rccl_comm(self, unique_id, rank, world):
        """This rank's RCCL communicator on this context (RcclComm): the native transport of the sharded relax."""
        return RcclComm(self, unique_id, rank, world)

    def set_priority(self, high=True):
        self._check(self.L.ochip_ctx_set_priority(self.h, int(high)), "ochip_ctx_set_priority")

    def device_info(self):
        name = C.create_string_buffer(256)
        cu, mem = C.c_int(), C.c_size_t()
        self._check(self.L.ochip_device_info(self.h, name, 256, C.byref(cu), C.byref(mem)), "ochip_device_info")
        return dict(name=name.value.decode(), compute_units=cu.value, hbm_bytes=mem.value)

    def synchronize(self):
        self._check(self.L.ochip_synchronize(self.h), "ochip_synchronize")

    def descriptors_reserve(self, n_images, total):
        self._check(self.L.ochip_descriptors_reserve(self.h, n_images, total), "ochip_descriptors_reserve")

    def upload_descriptors(self, image_id, desc):
        desc = np.ascontiguousarray(desc, np.uint64).reshape(-1, 8)
        self._check(self.L.ochip_upload_descriptors(self.h, image_id, desc.ctypes.data, len(desc)),
                    "ochip_upload_descriptors")

    def match_batch(self, pairs, out_offset, out_total=None):
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        out_offset = np.ascontiguousarray(out_offset, np.uint64)
        if out_total is None:
            raise ValueError("out_total required")
        out = np.zeros(max(out_total, 1), MATCH_DTYPE)
        self._check(self.L.ochip_match_launch(self.h, pairs.ctypes.data, len(pairs), out_offset.ctypes.data, out_total),
                    "ochip_match_launch")
        self._check(self.L.ochip_match_fetch(self.h, out.ctypes.data, out_total), "ochip_match_fetch")
        return out[:out_total]

    def match_launch(self, pairs, out_offset, out_total):
        pairs = np.ascontiguousarray(pairs, PAIR_DTYPE)
        out_offset = np.ascontiguousarray(out_offset, np.uint64)
        self._check(self.L.ochip_match_launch(self.h, pairs.ctypes.data, len(pairs), out_offset.ctypes.data, out_total),
                    "ochip_match_launch")

    def akaze_batch(self, images_bgr, max_kp=20000):
        """images_bgr: (n, h, w, 3) uint8.  Returns (list of (kp6, desc) per image, (work_w, work_h))."""
        imgs = np.ascontiguousarray(images_bgr, np.uint8)
        n, h, w, _ = imgs.shape
        kp = np.zeros((n, max_kp, 6), np.float32)
        desc = np.zeros((n, max_kp, 8), np.uint64)
        counts = np.zeros(n, np.uint32)
        wh = np.zeros(2, np.int32)
        self._check(self.L.ochip_akaze_batch(self.h, imgs.ctypes.data, n, w, h, max_kp, kp.ctypes.data, desc.ctypes.data,
                                             counts.ctypes.data, wh.ctypes.data), "ochip_akaze_batch")
        return [(kp[i, :counts[i]].copy(), desc[i, :counts[i]].copy()) for i in range(n)], (int(wh[0]), int(wh[1]))

    def working_image(self, images_bgr, device_ptr=None, shape=None):
        """ochip_debug_working_image: the grey, INTER_AREA-downscaled float image in front of AKAZE and the route taken.
        images_bgr: (n, h, w, 3) uint8 on the host - or None with device_ptr (an address in device memory, any alignment) and
        shape = (n, h, w).  Returns (n x H x W float32, (W, H), resize route, grey route): include/ochip.h, OCHIP_WI_*."""
        if device_ptr is None:
            imgs = np.ascontiguousarray(images_bgr, np.uint8)
            n, h, w, _ = imgs.shape
            src, on_device = imgs.ctypes.data, 0
        else:
            (n, h, w), src, on_device = shape, int(device_ptr), 1
        wh, route = np.zeros(2, np.int32), C.c_int(0)
        self._check(self.L.ochip_debug_working_image(self.h, src, on_device, 0, w, h, None, wh.ctypes.data, None),
                    "ochip_debug_working_image")
        out = np.zeros((n, int(wh[1]), int(wh[0])), np.float32)
        self._check(self.L.ochip_debug_working_image(self.h, src, on_device, n, w, h, out.ctypes.data, wh.ctypes.data,
                                                     C.byref(route)), "ochip_debug_working_image")
        return out, (int(wh[0]), int(wh[1])), route.value & 255, route.value >> 8

    def std_sort(self, keys, payload, offsets):
        """ochip_debug_std_sort: (keys, payload, fallback flags) with every segment [offsets[s], offsets[s + 1]) ordered as
        std::sort by descending key leaves it."""
        keys = np.ascontiguousarray(keys, np.uint32)
        payload = np.ascontiguousarray(payload, np.uint32)
        offsets = np.ascontiguousarray(offsets, np.uint32)
        n_segs = len(offsets) - 1
        ko, po = np.zeros(max(len(keys), 1), np.uint32), np.zeros(max(len(keys), 1), np.uint32)
        fb = np.zeros(max(n_segs, 1), np.uint8)
        kin = keys if len(keys) else np.zeros(1, np.uint32)
        pin = payload if len(keys) else np.zeros(1, np.uint32)
        self._check(self.L.ochip_debug_std_sort(self.h, kin.ctypes.data, pin.ctypes.data, offsets.ctypes.data, n_segs, ko.ctypes.data,
                                                po.ctypes.data, fb.ctypes.data), "ochip_debug_std_sort")
        return ko[:len(keys)], po[:len(keys)], fb[:n_segs].astype(bool)

    def feature_lists(self, kp6, desc, work_wh, scale, nms_radius=8.0, subset_spacing=0.0):
        """ochip_feature_lists_from_keypoints for ONE image's keypoints (detection order): dict of records ((n + 1) x 88
        bytes: the output list), response, slot (n each), num_sparse, conflict; with subset_spacing > 0 also subset (indices
        into the feature list) and subset_conflict."""
        kp6 = np.ascontiguousarray(kp6, np.float32).reshape(-1, 6)
        desc = np.ascontiguousarray(desc, np.uint64).reshape(-1, 8)
        n = len(kp6)
        m = max(n, 1)
        rec, resp = np.zeros((m + 1, 88), np.uint8), np.zeros(m, np.float32)
        slot, ns, conflict = np.zeros(m, np.uint32), np.zeros(4, np.uint32), np.zeros(16, np.uint8)
        subset, nsub, sconf = np.zeros(16384, np.uint32), np.zeros(4, np.uint32), np.zeros(16, np.uint8)
        counts = np.array([n], np.uint32)

        class Lists(C.Structure):
            _fields_ = [("records", C.c_void_p), ("response", C.c_void_p), ("slot", C.c_void_p), ("num_sparse", C.c_void_p),
                        ("conflict", C.c_void_p), ("subset", C.c_void_p), ("num_subset", C.c_void_p), ("subset_conflict", C.c_void_p),
                        ("subset_spacing", C.c_double)]

        lists = Lists(rec.ctypes.data, resp.ctypes.data, slot.ctypes.data, ns.ctypes.data, conflict.ctypes.data, subset.ctypes.data,
                      nsub.ctypes.data, sconf.ctypes.data, float(subset_spacing))
        kin = kp6 if n else np.zeros((1, 6), np.float32)
        din = desc if n else np.zeros((1, 8), np.uint64)
        self._check(self.L.ochip_feature_lists_from_keypoints(self.h, kin.ctypes.data, din.ctypes.data, counts.ctypes.data, 1, m,
                                                              int(work_wh[0]), int(work_wh[1]), float(scale), float(nms_radius),
                                                              C.byref(lists)), "ochip_feature_lists_from_keypoints")
        out = dict(records=rec[:n + 1 if n else 0], response=resp[:n], slot=slot[:n], num_sparse=int(ns[0]), conflict=bool(conflict[0]))
        if subset_spacing > 0:
            out.update(subset=subset[:int(nsub[0])].copy(), subset_conflict=bool(sconf[0]))
        return out

    def synth_views(self, position, orientation, width, height, f, pp, plane, spacing, origin, seed=7, chunk=64):
        """Render one synthetic view per camera directly into HBM (benchmark / test data).  Returns an opaque
        device pointer (int) to n x height x width x 3 bytes; free with synth_views_free."""
        n = len(position)
        ptr = C.c_void_p()
        self._check(self.L.ochip_synth_views_alloc(self.h, n, width, height, C.byref(ptr)), "ochip_synth_views_alloc")
        cams = np.ascontiguousarray(np.concatenate([position, orientation], axis=1), np.float64)
        model3 = np.array([f, pp[0], pp[1]], np.float64)
        plane2 = np.array(plane, np.float64)
        lat3 = np.array([origin[0], origin[1], spacing], np.float64)
        for i in range(0, n, chunk):
            m = min(chunk, n - i)
            c = np.ascontiguousarray(cams[i:i + m])
            self._check(self.L.ochip_synth_render_views(self.h, ptr, i, m, width, height, c.ctypes.data, model3.ctypes.data,
                                                        plane2.ctypes.data, lat3.ctypes.data, seed), "ochip_synth_render_views")
        return ptr.value

    def synth_views_read(self, ptr, index, width, height):
        out = np.zeros((height, width, 3), np.uint8)
        self._check(self.L.ochip_synth_views_read(self.h, C.c_void_p(ptr), index, width, height, out.ctypes.data),
                    "ochip_synth_views_read")
        return out

    def synth_views_read_into(self, ptr, index, width, height, out):
        """The same into a caller's (height, width, 3) uint8 array (e.g. a slice of host_array())."""
        self._check(self.L.ochip_synth_views_read(self.h, C.c_void_p(ptr), index, width, height, out.ctypes.data),
                    "ochip_synth_views_read")

    def host_array(self, shape, dtype=np.uint8):
        """A numpy array over page-locked host memory (ochip_host_alloc): PCIe copies from it run at link rate.  Returns
        (array, release); call release() when done (the array must not be used afterwards)."""
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        p = C.c_void_p()
        self.L.ochip_host_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        self.L.ochip_host_free.argtypes = [C.c_void_p, C.c_void_p]
        self.L.ochip_host_free.restype = None
        self._check(self.L.ochip_host_alloc(self.h, nbytes, C.byref(p)), "ochip_host_alloc")
        buf = (C.c_uint8 * nbytes).from_address(p.value)
        arr = np.frombuffer(buf, dtype=dtype).reshape(shape)
        return arr, (lambda: self.L.ochip_host_free(self.h, p))

    def synth_views_free(self, ptr):
        self.L.ochip_synth_views_free(self.h, C.c_void_p(ptr))

    def debug_fp64(self, op, x, y=None):
        x = np.ascontiguousarray(x, np.float64)
        y = np.ascontiguousarray(x if y is None else y, np.float64)
        out = np.zeros_like(x)
        self._check(self.L.ochip_debug_fp64(self.h, op, x.ctypes.data, y.ctypes.data, x.size, out.ctypes.data),
                    "ochip_debug_fp64")
        return out

    def debug_lm_step(self, A, g, scale, diagonal, radius, env_end, tail_begin, region_begin=(), route=0, back=0, want_L=True,
                      want_W=True):
        """ochip_debug_lm_step: one LM step's build, factorisation and back-solve on the dense system A (lower triangle
        read).  route 0: tiles, 1: launch chain; back 0: lm_solve's choice, 1: single workgroup, 2: regions (x in LDS),
        3: regions (x in HBM).  Returns dict x, y, L (n x n or None), W ((n + 1) x n or None), scal1, fail, order (0 column
        order, 1 tail first, 2 regions), slots, tiles, claims, regions, back."""
        A = np.ascontiguousarray(A, np.float64)
        n = int(A.shape[0]) if A.ndim == 2 else 0
        vec = lambda v: np.ascontiguousarray(v, np.float64).reshape(-1) if n else np.zeros(1)
        g, scale, diagonal = vec(g), vec(scale), vec(diagonal)
        env = np.ascontiguousarray(env_end, np.int32).reshape(-1)
        assert len(env) == (n + 63) // 64, (len(env), n)
        env = env if len(env) else np.zeros(1, np.int32)
        rb = np.ascontiguousarray(region_begin, np.int32).reshape(-1)
        n_rb = len(rb)
        rb = rb if n_rb else np.zeros(1, np.int32)
        m = max(n, 1)
        x, y = np.zeros(m), np.zeros(m)
        L = np.zeros((n, n)) if want_L and n else None
        W = np.zeros((n + 1, n)) if want_W and n else None
        s1 = C.c_double()
        info = np.zeros(8, np.int32)
        Ain = A if n else np.zeros(1)
        self._check(self.L.ochip_debug_lm_step(self.h, n, Ain.ctypes.data, g.ctypes.data, scale.ctypes.data, diagonal.ctypes.data,
                                               float(radius), env.ctypes.data, int(tail_begin), rb.ctypes.data, n_rb, int(route),
                                               int(back), x.ctypes.data, y.ctypes.data, None if L is None else L.ctypes.data,
                                               None if W is None else W.ctypes.data, C.byref(s1), info.ctypes.data),
                    "ochip_debug_lm_step")
        return dict(x=x[:n], y=y[:n], L=L, W=W, scal1=s1.value, fail=int(info[0]), order=int(info[1]), slots=int(info[2]),
                    tiles=int(info[3]), claims=int(info[4]), regions=int(info[5]), back=int(info[6]))

    def upload_batch(self, counts, desc, xy, models8):
        """ochip_upload_batch: image i owns counts[i] consecutive rows of desc (x 8 u64) and xy (x 2 f64); models8 n x 8."""
        counts = np.ascontiguousarray(counts, np.uint32)
        total = int(counts.sum())
        desc = np.ascontiguousarray(desc, np.uint64).reshape(-1, 8)
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        models8 = np.ascontiguousarray(models8, np.float64).reshape(-1, 8)
        assert len(desc) == total and len(xy) == total and len(models8) == len(counts)
        self._check(self.L.ochip_upload_batch(self.h, len(counts), counts.ctypes.data, desc.ctypes.data if total else None,
                                              xy.ctypes.data if total else None, models8.ctypes.data), "ochip_upload_batch")

    def refit_homography(self, jobs, matches, flags, rounds, threshold):
        """ochip_refit_homography_batch on uploaded keypoints: `rounds` times fitInliers + evaluate per job, starting from
        flags.  jobs: RANSAC_JOB_DTYPE, matches: RANSAC_MATCH_DTYPE, flags: one byte per match.  Returns (results
        [RANSAC_RESULT_DTYPE], the flags of the last evaluate)."""
        jobs = np.ascontiguousarray(jobs, RANSAC_JOB_DTYPE)
        matches = np.ascontiguousarray(matches, RANSAC_MATCH_DTYPE)
        out = np.ascontiguousarray(flags, np.uint8).copy()
        assert len(out) == len(matches)
        res = np.zeros(len(jobs), RANSAC_RESULT_DTYPE)
        total = len(matches)
        self._check(self.L.ochip_refit_homography_batch(self.h, jobs.ctypes.data, len(jobs), matches.ctypes.data if total else None,
                                                        total, int(rounds), float(threshold), res.ctypes.data,
                                                        out.ctypes.data if total else None), "ochip_refit_homography_batch")
        return res, out

    def debug_homography_fit4(self, xy16, route):
        """ochip_debug_homography_fit4: homography_model::fit of the minimal samples xy16 (n x 16: four correspondences x
        (x, y, x', y'), divided by z).  route 0: the wave-cooperative 9 x 9 factorisation, 1: the fast-forward's lane fit.
        Returns (H [n, 3, 3], Hinv [n, 3, 3], degenerate [n] bool)."""
        xy16 = np.ascontiguousarray(xy16, np.float64).reshape(-1, 16)
        n = len(xy16)
        H, Hi, deg = np.zeros((max(n, 1), 9)), np.zeros((max(n, 1), 9)), np.zeros(max(n, 1), np.uint8)
        self._check(self.L.ochip_debug_homography_fit4(self.h, int(route), xy16.ctypes.data if n else None, n, H.ctypes.data,
                                                       Hi.ctypes.data, deg.ctypes.data), "ochip_debug_homography_fit4")
        return H[:n].reshape(-1, 3, 3), Hi[:n].reshape(-1, 3, 3), deg[:n].astype(bool)

    def debug_decompose_votes(self, jobs, matches, H, flags):
        """ochip_debug_decompose_votes: decompose_vote_kernel on given homographies H (one 3 x 3 per job) over the rays of the
        uploaded keypoints.  jobs: RANSAC_JOB_DTYPE, matches: RANSAC_MATCH_DTYPE, flags: one byte per match.  Returns one
        DECOMPOSITION_DTYPE row per job."""
        jobs = np.ascontiguousarray(jobs, RANSAC_JOB_DTYPE)
        matches = np.ascontiguousarray(matches, RANSAC_MATCH_DTYPE)
        flags = np.ascontiguousarray(flags, np.uint8)
        H = np.ascontiguousarray(H, np.float64).reshape(-1, 9)
        n, total = len(jobs), len(matches)
        assert len(H) == n and len(flags) == total
        out = np.zeros(max(n, 1), DECOMPOSITION_DTYPE)
        self._check(self.L.ochip_debug_decompose_votes(self.h, jobs.ctypes.data if n else None, n, matches.ctypes.data if total else None,
                                                       total, H.ctypes.data if n else None, flags.ctypes.data if total else None,
                                                       out.ctypes.data), "ochip_debug_decompose_votes")
        return out[:n]

    def relaxg_evaluate(self, scene, structure_only=False):
        """One evaluation of a general-engine relax problem (ochip_relaxg_problem_create, ochip_relaxg_evaluate, destroy):
        (cost, dense J'J, J'r, first unknown per camera / vertex / f / pp / k).  scene: dict of the ochip_relaxg_desc fields
        (relaxg_desc).  An evaluation that reports non-finite blocks raises OchipError."""
        d, keep = relaxg_desc(scene)
        p = C.c_void_p()
        self.L.ochip_relaxg_problem_create.argtypes = [C.c_void_p, C.POINTER(RelaxgDesc), C.POINTER(C.c_void_p)]
        self.L.ochip_relaxg_problem_destroy.argtypes = [C.c_void_p]
        self.L.ochip_relaxg_problem_destroy.restype = None
        self.L.ochip_relaxg_evaluate.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.c_void_p, C.c_void_p,
                                                 C.c_void_p]
        self._check(self.L.ochip_relaxg_problem_create(self.h, C.byref(d), C.byref(p)), "ochip_relaxg_problem_create")
        try:
            if structure_only:
                self.L.ochip_relaxg_set_structure_only.argtypes = [C.c_void_p, C.c_int]
                self._check(self.L.ochip_relaxg_set_structure_only(p, 1), "ochip_relaxg_set_structure_only")
            cost, n = C.c_double(), C.c_int()
            order = np.zeros(d.n_cams + d.n_verts + 3, np.int32)
            rc = self.L.ochip_relaxg_evaluate(p, C.byref(cost), C.byref(n), None, None, order.ctypes.data)
            if rc < 0:
                self._check(rc, "ochip_relaxg_evaluate")
            JtJ, Jtr = np.zeros((n.value, n.value)), np.zeros(n.value)
            rc = self.L.ochip_relaxg_evaluate(p, C.byref(cost), C.byref(n), JtJ.ctypes.data, Jtr.ctypes.data, None)
            if rc != 0:
                raise OchipError(f"ochip_relaxg_evaluate = {rc}: {self.L.ochip_last_error(self.h).decode()}")
        finally:
            self.L.ochip_relaxg_problem_destroy(p)
        return cost.value, JtJ, Jtr, order

    def relax_evaluate(self, scene, route=0, delta=None, cameras_constant=False, iterations=0):
        """One evaluation of a plane-engine relax problem (ochip_relax_problem_create, ochip_relax_evaluate, destroy).
        scene: dict of the ochip_relax_desc fields (relax_desc).  iterations > 0: ochip_relax_solve with that many
        iterations first.  route / delta: as ochip_relax_evaluate (delta in the library's unknown order).
        cameras_constant: the evaluation between ochip_relax_set_cameras_constant(1) and (0); the evaluation after the
        undo is returned as well, under "undone".  dict: cost, JtJ, Jtr, order (n_cams + 3), layout (n, tail_begin,
        regions, separator cameras), cam_q and plane_z (the current state), summary (of the solve, or None).  An
        evaluation that reports non-finite blocks raises OchipError."""
        d, keep = relax_desc(scene)
        p = C.c_void_p()
        L = self.L
        L.ochip_relax_problem_create.argtypes = [C.c_void_p, C.POINTER(RelaxDesc), C.POINTER(C.c_void_p)]
        L.ochip_relax_problem_destroy.argtypes = [C.c_void_p]
        L.ochip_relax_problem_destroy.restype = None
        L.ochip_relax_set_cameras_constant.argtypes = [C.c_void_p, C.c_int]
        L.ochip_relax_solve.argtypes = [C.c_void_p, C.POINTER(RelaxOptions), C.POINTER(RelaxSummary)]
        L.ochip_relax_get_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.ochip_relax_evaluate.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int),
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

        def one(route, delta):
            cost, n = C.c_double(), C.c_int()
            order, layout = np.zeros(d.n_cams + 3, np.int32), np.zeros(4, np.int32)
            self._check(L.ochip_relax_evaluate(p, 0, None, None, C.byref(n), None, None, order.ctypes.data, layout.ctypes.data),
                        "ochip_relax_evaluate")  # (the layout alone)
            n = n.value
            JtJ, Jtr = np.zeros((max(n, 1), max(n, 1))), np.zeros(max(n, 1))
            dl = None if delta is None else np.ascontiguousarray(delta, np.float64)
            assert dl is None or dl.shape == (n,), (None if dl is None else dl.shape, n)
            rc = L.ochip_relax_evaluate(p, int(route), None if dl is None else dl.ctypes.data, C.byref(cost), None,
                                        JtJ.ctypes.data, Jtr.ctypes.data, None, None)
            if rc != 0:
                raise OchipError(f"ochip_relax_evaluate = {rc}: {L.ochip_last_error(self.h).decode()}")
            q, z = np.zeros((d.n_cams, 4)), np.zeros(3)
            self._check(L.ochip_relax_get_state(p, q.ctypes.data, z.ctypes.data), "ochip_relax_get_state")
            return dict(cost=cost.value, JtJ=JtJ[:n, :n], Jtr=Jtr[:n], order=order, layout=layout, cam_q=q, plane_z=z)

        self._check(L.ochip_relax_problem_create(self.h, C.byref(d), C.byref(p)), "ochip_relax_problem_create")
        try:
            summary = None
            if iterations > 0:
                opt = RelaxOptions(max_num_iterations=int(iterations), initial_trust_region_radius=1.0, function_tolerance=1e-6,
                                   gradient_tolerance=1e-10, parameter_tolerance=1e-8)
                s = RelaxSummary()
                self._check(L.ochip_relax_solve(p, C.byref(opt), C.byref(s)), "ochip_relax_solve")
                summary = {k: getattr(s, k) for k, _ in RelaxSummary._fields_}
            if cameras_constant:
                self._check(L.ochip_relax_set_cameras_constant(p, 1), "ochip_relax_set_cameras_constant")
            out = one(route, delta)
            out["summary"] = summary
            if cameras_constant:
                self._check(L.ochip_relax_set_cameras_constant(p, 0), "ochip_relax_set_cameras_constant")
                out["undone"] = one(0, None)
        finally:
            L.ochip_relax_problem_destroy(p)
        return out

    def _relaxp_open(self, scene, structure_only):
        L = self.L
        vp = C.c_void_p
        L.ochip_relaxp_problem_create.argtypes = [vp, C.POINTER(RelaxpDesc), C.POINTER(vp)]
        L.ochip_relaxp_problem_destroy.argtypes = [vp]
        L.ochip_relaxp_problem_destroy.restype = None
        L.ochip_relaxp_set_structure_only.argtypes = [vp, C.c_int]
        L.ochip_relaxp_solve.argtypes = [vp, C.POINTER(RelaxOptions), C.POINTER(RelaxSummary)]
        L.ochip_relaxp_get_state.argtypes = [vp, vp, vp, vp]
        L.ochip_relaxp_evaluate.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int), vp, vp, vp, vp, C.POINTER(C.c_double), vp]
        L.ochip_relaxp_step.argtypes = [vp, C.c_double, vp, vp, C.c_double, vp, vp, vp, vp, vp, vp, vp, vp, vp, C.POINTER(C.c_int32)]
        d, keep = relaxp_desc(scene)
        p = vp()
        self._check(L.ochip_relaxp_problem_create(self.h, C.byref(d), C.byref(p)), "ochip_relaxp_problem_create")
        if structure_only:
            rc = L.ochip_relaxp_set_structure_only(p, 1)
            if rc:
                L.ochip_relaxp_problem_destroy(p)
                self._check(rc, "ochip_relaxp_set_structure_only")
        return d, keep, p

    def _relaxp_eval(self, d, p):
        L = self.L
        cost, n, gmax = C.c_double(), C.c_int(), C.c_double()
        order = np.zeros(d.n_cams + 8, np.int32)
        self._check(L.ochip_relaxp_evaluate(p, None, C.byref(n), None, None, None, None, None, order.ctypes.data),
                    "ochip_relaxp_evaluate")  # (n and the order alone)
        n, m = n.value, d.n_points
        U, g_c, V, g_p = np.zeros((max(n, 1), max(n, 1))), np.zeros(max(n, 1)), np.zeros((max(m, 1), 6)), np.zeros((max(m, 1), 3))
        rc = L.ochip_relaxp_evaluate(p, C.byref(cost), None, U.ctypes.data, g_c.ctypes.data, V.ctypes.data, g_p.ctypes.data,
                                     C.byref(gmax), None)
        if rc != 0:
            raise OchipError(f"ochip_relaxp_evaluate = {rc}: {L.ochip_last_error(self.h).decode()}")
        q, X, model = np.zeros((d.n_cams, 4)), np.zeros((max(m, 1), 3)), np.zeros(8)
        self._check(L.ochip_relaxp_get_state(p, q.ctypes.data, X.ctypes.data, model.ctypes.data), "ochip_relaxp_get_state")
        return dict(cost=cost.value, n=n, U=U[:n, :n], g_c=g_c[:n], V=V[:m], g_p=g_p[:m], gmax_p=gmax.value, order=order,
                    cam_q=q, point_xyz=X[:m], model=model)

    def relaxp_evaluate(self, scene, structure_only=False, iterations=0, radius=1e4):
        """One evaluation of a points-engine relax problem (ochip_relaxp_problem_create, ochip_relaxp_evaluate, destroy).
        scene: dict of the ochip_relaxp_desc fields (relaxp_desc).  iterations > 0: ochip_relaxp_solve with that many
        iterations (initial trust-region radius `radius`) first.  dict: cost, n, U (n x n), g_c, V (n_points x 6), g_p
        (n_points x 3), gmax_p, order (n_cams + 8), cam_q, point_xyz and model (the current state), summary (of the solve, or
        None).  An evaluation that reports a non-finite observation raises OchipError."""
        d, keep, p = self._relaxp_open(scene, structure_only)
        try:
            summary = None
            if iterations > 0:
                opt = RelaxOptions(max_num_iterations=int(iterations), initial_trust_region_radius=float(radius),
                                   function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8)
                s = RelaxSummary()
                self._check(self.L.ochip_relaxp_solve(p, C.byref(opt), C.byref(s)), "ochip_relaxp_solve")
                summary = {k: getattr(s, k) for k, _ in RelaxSummary._fields_}
            out = self._relaxp_eval(d, p)
            out["summary"] = summary
        finally:
            self.L.ochip_relaxp_problem_destroy(p)
        return out

    def relaxp_step(self, scene, steps, structure_only=False):
        """ochip_relaxp_evaluate, then one ochip_relaxp_step per entry of `steps` on the same problem (the first fixes the
        points' Jacobi scaling, the later ones keep it).  A step is a dict: radius, and optionally scale (n; absent: the
        solver's own), y_in (n) and alpha2 - or a callable (evaluation, results so far) that returns one.
        Returns (evaluation as relaxp_evaluate, [dict per step: W ((n + 1) x n, lower triangle, row n the right-hand
        side), y, cam_q2, model2, X2, pt_scale, pt_Vinv, pt_d, model_cost_change, step_sq, cand_sq, slope_p, fail])."""
        d, keep, p = self._relaxp_open(scene, structure_only)
        try:
            ev = self._relaxp_eval(d, p)
            n, m = ev["n"], d.n_points
            outs = []
            for st in steps:
                st = st(ev, outs) if callable(st) else st
                sc = None if st.get("scale") is None else np.ascontiguousarray(st["scale"], np.float64)
                yi = None if st.get("y_in") is None else np.ascontiguousarray(st["y_in"], np.float64)
                assert (sc is None or sc.shape == (n,)) and (yi is None or yi.shape == (n,))
                W, y = np.zeros((n + 1, max(n, 1))), np.zeros(max(n, 1))
                q2, m2, X2 = np.zeros((d.n_cams, 4)), np.zeros(8), np.zeros((max(m, 1), 3))
                ps, pv, pd = np.zeros((max(m, 1), 3)), np.zeros((max(m, 1), 6)), np.zeros((max(m, 1), 3))
                scal, fail = np.zeros(4), C.c_int32()
                self._check(self.L.ochip_relaxp_step(p, float(st["radius"]), None if sc is None else sc.ctypes.data,
                                                     None if yi is None else yi.ctypes.data, float(st.get("alpha2", 0.0)),
                                                     W.ctypes.data, y.ctypes.data, q2.ctypes.data, m2.ctypes.data, X2.ctypes.data,
                                                     ps.ctypes.data, pv.ctypes.data, pd.ctypes.data, scal.ctypes.data, C.byref(fail)),
                            "ochip_relaxp_step")
                outs.append(dict(W=W[:, :n], y=y[:n], cam_q2=q2, model2=m2, X2=X2[:m], pt_scale=ps[:m], pt_Vinv=pv[:m], pt_d=pd[:m],
                                 model_cost_change=scal[0], step_sq=scal[1], cand_sq=scal[2], slope_p=scal[3], fail=fail.value))
        finally:
            self.L.ochip_relaxp_problem_destroy(p)
        return ev, outs

    def profile_reset(self):
        self._check(self.L.ochip_profile_reset(self.h), "ochip_profile_reset")

    def relax_work(self):
        f = C.c_double()
        self._check(self.L.ochip_relax_work(self.h, C.byref(f)), "ochip_relax_work")
        return f.value

    def work_counters(self):
        """{ransac loop trips x correspondences, relax residual blocks with / without Jacobians} since the last profile reset."""
        out = (C.c_uint64 * 3)()
        self.L.ochip_work_counters.argtypes = [C.c_void_p, C.c_void_p]
        self._check(self.L.ochip_work_counters(self.h, out), "ochip_work_counters")
        return {"ransac_hyp_corr": int(out[0]), "relax_blocks_jac": int(out[1]), "relax_blocks_cost": int(out[2])}

    def relax_memory(self):
        """(unknowns, bytes stored, bytes dense) of the largest reduced system a relax on this context has held."""
        n, b, d = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(self.L.ochip_relax_memory(self.h, C.byref(n), C.byref(b), C.byref(d)), "ochip_relax_memory")
        return n.value, b.value, d.value

    def match_work(self):
        """(computed, delivered) descriptor distances of the match launches since the last profile_reset."""
        c, d = C.c_uint64(), C.c_uint64()
        self._check(self.L.ochip_match_work(self.h, C.byref(c), C.byref(d)), "ochip_match_work")
        return c.value, d.value

    def profile_get(self, kid):
        n, ms = C.c_uint64(), C.c_double()
        self._check(self.L.ochip_profile_get(self.h, kid, C.byref(n), C.byref(ms)), "ochip_profile_get")
        return n.value, ms.value
