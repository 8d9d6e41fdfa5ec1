"""ctypes binding of liboc_host.so (include/oc_host.h): the C++ host side of the hot path."""
import ctypes as C
import os

import numpy as np

from . import capi

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "liboc_host.so")

_lib = None
_u64p = np.ctypeslib.ndpointer(np.uint64, flags="C_CONTIGUOUS")
_f64p = np.ctypeslib.ndpointer(np.float64, flags="C_CONTIGUOUS")
_f32p = np.ctypeslib.ndpointer(np.float32, flags="C_CONTIGUOUS")


# ochip_relax_exchange_fn (include/ochip.h): all-gather the per-pair record arrays of a sharded relax in place
RELAX_EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)


def effective_cpus():
    """Host cores this process may really use: the affinity mask capped by the cgroup CPU quota (the GPU
    boxes expose 256 hardware threads but run the job under a 16-CPU cfs quota; 256 OpenMP threads inside
    such a quota only thrash)."""
    n = len(os.sched_getaffinity(0))
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        try:
            q = int(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            p = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                n = min(n, max(1, q // p))
        except (OSError, ValueError):
            pass
    return n


def host_threads():
    """OpenMP team size for the host phases.  They are short bursts between device phases (tens of ms of every
    100 ms cfs period), so a team larger than the quota finishes them sooner without exhausting the period's
    budget - provided idle members sleep (OMP_WAIT_POLICY=passive, set in load()) and threads waiting for the device
    block (OCHIP_BLOCKING_SYNC, default on).  Measured on the 16-CPU-quota MI355X boxes, C3 ms per step:
    24 threads 624, 32 600, 48 586, 64 563, 96 568, 128 582 (with spinning waits 32 threads took 668 and 64 were
    throttled)."""
    return max(1, min(len(os.sched_getaffinity(0)), 4 * effective_cpus()))


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise capi.OchipError(f"{LIB_PATH} is missing: run `python -m opencalibration_amd.build`")
        os.environ.setdefault("OMP_NUM_THREADS", str(host_threads()))  # read by libgomp when the library loads
        os.environ.setdefault("OMP_WAIT_POLICY", "passive")           # idle team members sleep (CPU quota, see bench.py)
        capi.load()  # libochip.so first (liboc_host.so links against it)
        L = C.CDLL(LIB_PATH)
        L.och_subsample.restype = C.c_size_t
        L.och_subsample.argtypes = [_f64p, _f32p, C.c_size_t, C.c_double, C.c_size_t, _u64p]
        L.och_matches_from_device.restype = C.c_size_t
        L.och_matches_from_device.argtypes = [C.c_void_p, _u64p, C.c_size_t, _u64p, C.c_size_t, _u64p, _u64p, _f64p]
        vp, u32, u64, sz = C.c_void_p, C.c_uint32, C.c_uint64, C.c_size_t
        L.och_graph_create.restype = vp
        L.och_graph_destroy.argtypes = [vp]
        L.och_graph_destroy.restype = None
        L.och_last_error.argtypes = [vp]
        L.och_last_error.restype = C.c_char_p
        L.och_graph_add_model.argtypes = [vp, _f64p]
        L.och_graph_add_model.restype = u32
        L.och_graph_add_image.argtypes = [vp, _f64p, _f32p, _u64p, sz, sz, u32, _f64p]
        L.och_graph_add_image.restype = u64
        L.och_graph_add_edge.restype = u64
        L.och_graph_add_edge.argtypes = [vp, u64, u64, vp, C.c_int, sz, _f64p, _u64p, sz, vp, vp, vp]
        L.och_link_match_work.argtypes = [vp, _f64p]
        L.och_link_match_work.restype = None
        L.och_graph_get_orientations.argtypes = [vp, _f64p]
        L.och_graph_get_orientations.restype = None
        L.och_graph_num_nodes.argtypes = [vp]
        L.och_graph_num_nodes.restype = sz
        L.och_graph_num_edges.argtypes = [vp]
        L.och_graph_num_edges.restype = sz
        L.och_graph_node_ids.argtypes = [vp, _u64p]
        L.och_link_stage_run.argtypes = [vp, vp, _u64p, sz, C.c_int, _f64p]
        L.och_link_debug_count.argtypes = [vp]
        L.och_link_debug_count.restype = sz
        L.och_link_debug_pair.argtypes = [vp, sz, _u64p, _u64p, _f64p, np.ctypeslib.ndpointer(np.uint32)]
        L.och_link_debug_matches.argtypes = [vp, sz, _u64p, _u64p, _f64p, np.ctypeslib.ndpointer(np.uint8)]
        L.och_graph_edge_info.argtypes = [vp, sz, _u64p, _u64p, _f64p, _f64p]
        L.och_graph_edge_inliers.argtypes = [vp, sz, _u64p, _u64p, _u64p, _f64p]
        L.och_graph_edge_match_distances.argtypes = [vp, sz, _f64p]
        L.och_graph_edge_matches.argtypes = [vp, sz, vp, vp, C.POINTER(C.c_int)]
        L.och_graph_edge_matches.restype = None
        L.och_graph_set_orientations.argtypes = [vp, _f64p]
        u8p = np.ctypeslib.ndpointer(np.uint8, flags="C_CONTIGUOUS")
        L.och_relax_ground_plane.argtypes = [vp, sz, _f64p, _f64p, _f64p, sz, _u64p, _f64p, sz, _u64p, _u64p, _f64p, u8p,
                                             _u64p, _f64p, _u64p, vp, vp, sz, _u64p, _f64p, _f64p]
        L.och_relax_last_error.restype = C.c_char_p
        L.och_debug_relax_setup_check.argtypes = [C.c_int]
        L.och_graph_relax_ground_plane.argtypes = [vp, vp, _f64p, _f64p, _f64p]
        L.och_graph_relax_ground_plane_sharded.argtypes = [vp, vp, _f64p, _f64p, _f64p, u32, u32, vp, vp]
        L.och_surface_create.restype = vp
        L.och_surface_destroy.argtypes = [vp]
        L.och_surface_destroy.restype = None
        L.och_surface_counts.argtypes = [vp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]
        L.och_surface_counts.restype = None
        L.och_surface_get.argtypes = [vp, vp, vp, vp]
        L.och_surface_get.restype = None
        L.och_surface_set.argtypes = [vp, sz, _f64p, sz, _u64p, sz, _f64p]
        L.och_surface_set.restype = None
        L.och_surface_set_heights.argtypes = [vp, _f64p]
        L.och_surface_set_heights.restype = None
        L.och_rebuild_mesh.argtypes = [_f64p, sz, vp, C.c_int, vp]
        L.och_rebuild_mesh.restype = None
        L.och_relax.argtypes = [vp, sz, _f64p, _f64p, _f64p, _u64p, _f64p, sz, _u64p, _f64p, sz, _u64p, _u64p, vp, u8p, _u64p,
                                _f64p, _u64p, _u64p, vp, vp, sz, _u64p, u32, C.c_double, vp, vp, _f64p, vp]
        L.och_relax_ex.argtypes = L.och_relax.argtypes + [vp, C.c_int, vp, vp, sz, C.POINTER(sz)]
        L.och_graph_relax.argtypes = [vp, vp, _f64p, u32, C.c_double, vp, vp, _f64p]
        L.och_graph_relax_sharded.argtypes = [vp, vp, _f64p, u32, C.c_double, vp, vp, _f64p, u32, u32, vp, vp]
        i64p = np.ctypeslib.ndpointer(np.int64, flags="C_CONTIGUOUS")
        L.och_relax_stage_run.argtypes = [vp, vp, vp, sz, C.c_int, C.c_int, u32, C.c_double, sz, vp, vp, i64p, _f64p]
        L.och_relax_stage_begin.restype = vp
        L.och_relax_stage_begin.argtypes = [vp, vp, sz, C.c_int, C.c_int, u32, C.c_double, sz, vp, i64p]
        L.och_relax_stage_num_groups.argtypes = [vp]
        L.och_relax_stage_num_groups.restype = sz
        L.och_relax_stage_run_groups.argtypes = [vp, vp, u32, u32]
        L.och_relax_stage_export.argtypes = [vp, u32, u32, C.POINTER(vp), C.POINTER(u64)]
        L.och_relax_stage_import.argtypes = [vp, vp, u64]
        L.och_relax_stage_end.argtypes = [vp, vp, _f64p]
        L.och_relax_partition.restype = sz
        L.och_relax_partition.argtypes = [vp, sz, i64p, i64p]
        L.och_merge_surfaces.argtypes = [C.POINTER(vp), sz, vp]
        L.och_merge_surfaces.restype = None
        L.och_homography_decompose.argtypes = [_f64p, _f64p, sz, _f64p]
        L.och_image_to_3d.argtypes = [_f64p, sz, _f64p, _f64p]
        L.och_ransac_epipolar.restype = C.c_double
        L.och_ransac_epipolar.argtypes = [vp, C.c_int, _f64p, vp, sz, C.c_double, _f64p, u8p, np.ctypeslib.ndpointer(np.uint32)]
        L.och_extract_tail_prepared.restype = C.c_size_t
        L.och_extract_tail_prepared.argtypes = [C.c_void_p, _f32p, C.c_void_p, u32, C.c_int, u32, C.c_double, _f64p, _f32p, _u64p, _u64p]
        L.och_extract_tail.restype = C.c_size_t
        L.och_extract_tail.argtypes = [_f32p, _u64p, u32, C.c_double, _f64p, _f32p, _u64p, _u64p]
        L.och_graph_set_model.argtypes = [vp, u32, _f64p]
        L.och_graph_refit_edges.argtypes = [vp, vp]
        L.och_extract_features_batch.argtypes = [vp, vp, u32, C.c_int, C.c_int, u32, u32, vp, vp, vp, vp, vp, C.c_int]
        L.och_extract_last_error.restype = C.c_char_p
        L.och_graph_load_images.argtypes = [vp, vp, vp, u32, C.c_int, C.c_int, u32, C.c_int, u32, _f64p, _u64p, _f64p]
        L.och_graph_load_link_images.argtypes = [vp, vp, vp, u32, C.c_int, C.c_int, u32, C.c_int, u32, _f64p, vp, _u64p,
                                                 _f64p, _f64p, _f64p]
        L.och_initial_processing_create.restype = vp
        L.och_initial_processing_create.argtypes = [vp, vp]
        L.och_initial_processing_destroy.restype = None
        L.och_initial_processing_destroy.argtypes = [vp]
        L.och_initial_processing_pending.argtypes = [vp]
        L.och_initial_processing_step.argtypes = [vp, vp, u32, C.c_int, C.c_int, u32, C.c_int, u32, vp, C.c_int, vp, _f64p]
        L.och_graph_to_json.argtypes = [vp, C.POINTER(sz)]
        L.och_graph_to_json.restype = vp
        L.och_free.argtypes = [vp]
        L.och_free.restype = None
        L.och_graph_from_json.argtypes = [vp, C.c_char_p, sz]
        L.och_graph_save_json.argtypes = [vp, C.c_char_p]
        L.och_graph_load_json.argtypes = [vp, C.c_char_p]
        L.och_graph_node_table.argtypes = [vp, vp, vp, vp, vp]
        L.och_graph_node_table.restype = None
        L.och_graph_node_payload.argtypes = [vp, sz, vp, vp, vp, vp, vp]
        L.och_graph_node_path.argtypes = [vp, sz]
        L.och_graph_node_path.restype = C.c_char_p
        L.och_graph_set_node_path.argtypes = [vp, sz, C.c_char_p]
        L.och_graph_num_models.argtypes = [vp]
        L.och_graph_num_models.restype = sz
        L.och_graph_get_model.argtypes = [vp, u32, _f64p]
        L.och_surface_save_ply.argtypes = [vp, C.c_char_p]
        L.och_surface_load_ply.argtypes = [vp, C.c_char_p]
        L.och_surface_num_clouds.argtypes = [vp]
        L.och_surface_num_clouds.restype = sz
        L.och_surface_cloud_sizes.argtypes = [vp, _u64p]
        L.och_surface_cloud_sizes.restype = None
        L.och_surface_set_clouds.argtypes = [vp, sz, _u64p, _f64p]
        L.och_surface_set_clouds.restype = None
        L.och_checkpoint_validate.argtypes = [C.c_char_p]
        L.och_checkpoint_save.argtypes = [C.c_char_p, vp, C.POINTER(vp), sz, C.c_char_p, _f64p]
        L.och_checkpoint_load.argtypes = [C.c_char_p, vp]
        L.och_checkpoint_load.restype = vp
        L.och_checkpoint_destroy.argtypes = [vp]
        L.och_checkpoint_destroy.restype = None
        L.och_checkpoint_num_surfaces.argtypes = [vp]
        L.och_checkpoint_num_surfaces.restype = sz
        L.och_checkpoint_state.argtypes = [vp]
        L.och_checkpoint_state.restype = C.c_char_p
        L.och_checkpoint_info.argtypes = [vp, _f64p]
        L.och_checkpoint_info.restype = None
        L.och_checkpoint_get_surface.argtypes = [vp, sz, vp]
        L.och_densify_mesh.argtypes = [vp, vp, vp, _f64p, vp, sz]
        L.och_refine_by_point_density.argtypes = [vp, sz, C.c_double, C.c_int, C.c_double]
        L.och_refine_by_point_density.restype = sz
        L.och_refine_at_point.argtypes = [vp, C.c_double, C.c_double, C.c_int]
        L.och_refine_at_point.restype = sz
        L.och_count_points_per_triangle.argtypes = [vp, _u64p, _f64p, sz]
        L.och_count_points_per_triangle.restype = sz
        L.och_surface_locate.argtypes = [vp, _f64p, sz, _u64p]
        L.och_surface_locate.restype = None
        L.och_mesh_refinement_run.argtypes = [vp, vp, vp, C.c_int, _f64p]
        L.och_points_last_error.restype = C.c_char_p
        L.och_surface_count_points.argtypes = [vp, vp, _u64p, _f64p, sz]
        L.och_surface_count_points.restype = sz
        L.och_surface_locate_on.argtypes = [vp, vp, _f64p, sz, C.c_int, _u64p]
        L.och_point_counter_create.argtypes = [vp, _f64p, sz, C.c_int]
        L.och_point_counter_create.restype = vp
        L.och_point_counter_destroy.argtypes = [vp]
        L.och_point_counter_destroy.restype = None
        L.och_point_counter_count.argtypes = [vp, vp, _u64p, _f64p, sz, _u64p]
        L.och_point_counter_count.restype = sz
        L.och_surface_locate_table_sizes.argtypes = [vp, _u64p]
        L.och_surface_locate_table_sizes.restype = None
        L.och_surface_locate_table.argtypes = [vp] + [vp] * 8
        L.och_surface_locate_table.restype = None
        L.och_dense_mesh_relax_run.argtypes = [vp, vp, vp, C.c_int, _f64p]
        L.och_export_last_error.restype = C.c_char_p
        L.och_cloud_outlier_bounds.argtypes = [vp, sz, vp, vp]
        L.och_cloud_to_xyz.argtypes = [vp, sz, vp, vp, C.POINTER(sz), C.POINTER(u64)]
        L.och_cloud_to_xyz.restype = vp
        L.och_cloud_save_xyz.argtypes = [vp, sz, vp, vp, C.c_char_p]
        L.och_xyz_outlier_bounds.argtypes = [vp, sz, vp, vp]
        L.och_xyz_to_text.argtypes = [vp, sz, vp, vp, C.POINTER(sz), C.POINTER(u64)]
        L.och_xyz_to_text.restype = vp
        L.och_format_g6.argtypes = [vp, sz, C.c_int, vp, vp]
        L.och_format_g6.restype = None
        L.och_textured_obj.argtypes = [vp, sz, C.c_int64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_char_p,
                                       C.c_char_p, C.POINTER(vp), C.POINTER(sz), C.POINTER(vp), C.POINTER(sz)]
        L.och_shard_block.argtypes = [u32, u32, u32, C.POINTER(u32), C.POINTER(u32)]
        L.och_shard_block.restype = None
        L.och_shard_begin.restype = vp
        L.och_shard_begin.argtypes = [vp, vp, u32, u32, _f64p, vp, u32, u32, _u64p]
        L.och_shard_destroy.argtypes = [vp]
        L.och_shard_destroy.restype = None
        L.och_shard_counts.argtypes = [vp, _u64p]
        L.och_shard_counts.restype = None
        L.och_shard_load_link_local.argtypes = [vp, vp, C.c_int, C.c_int, u32, C.c_int]
        for name in ("och_shard_subsets_export", "och_shard_edges_export"):
            getattr(L, name).argtypes = [vp, C.POINTER(vp), C.POINTER(u64)]
        for name in ("och_shard_subsets_import", "och_shard_edges_import"):
            getattr(L, name).argtypes = [vp, vp, u64]
        L.och_shard_link_remote.argtypes = [vp]
        L.och_shard_finalize.argtypes = [vp, _f64p, _f64p, _f64p]
        L.och_hilbert_xy2d.argtypes = [C.c_int, C.c_int, C.c_int]
        L.och_hilbert_xy2d.restype = u32
        i32, i64, f64 = C.c_int32, C.c_int64, C.c_double
        L.och_graph_set_thumbnail.argtypes = [vp, sz, sz, sz, vp]
        L.och_ortho_bounds.argtypes = [vp, sz, _f64p]
        L.och_ortho_bounds.restype = None
        L.och_ortho_gsd.argtypes = [vp, _u64p, sz, f64, C.c_int]
        L.och_ortho_gsd.restype = f64
        L.och_ortho_context.argtypes = [vp, vp, sz, C.c_int, _f64p]
        L.och_ortho_context.restype = sz
        for fn in (L.och_ortho_clamp_resolution, L.och_ortho_clamp_megapixels):
            fn.argtypes = [u64 if fn is L.och_ortho_clamp_resolution else f64, C.POINTER(f64), C.POINTER(i32), C.POINTER(i32)]
            fn.restype = None
        L.och_ray_trace_height.argtypes = [vp, sz, f64, f64, f64]
        L.och_ray_trace_height.restype = f64
        L.och_orthomosaic_thumbnail.argtypes = [vp, vp, vp, sz, vp, _f64p, vp, vp, vp]
        L.och_dsm_plan.argtypes = [vp, vp, sz, f64, _f64p]
        L.och_ortho_mesh_upload.argtypes = [vp, vp, sz, C.POINTER(vp)]
        L.och_dsm_render.argtypes = [vp, vp, vp, sz, _f64p, i64, i64, vp, C.c_int, vp, vp, C.POINTER(u64)]
        L.och_ortho_last_error.restype = C.c_char_p
        L.och_ortho_layers_cameras.argtypes = [vp, vp, sz, vp, vp, vp, vp]
        L.och_ortho_layers_cameras.restype = sz
        L.och_ortho_layers_render.argtypes = [vp, vp, vp, vp, sz, _f64p, vp, i64, i64, vp, vp, vp, C.c_int, vp, vp, vp, vp, u64,
                                              C.POINTER(u64), vp]
        L.och_ortho_layers_last_error.restype = C.c_char_p
        L.och_ortho_band_cameras.argtypes = [vp, _f64p, i32, i64, i64, sz, vp, vp]
        L.och_ortho_layers_render_subset.argtypes = [vp, vp, vp, vp, sz, _f64p, vp, i64, i64, vp, sz, vp, vp, vp, C.c_int, vp, vp,
                                                     vp, vp, u64, C.POINTER(u64), vp]
        L.och_ortho_residency_plan.argtypes = [vp, sz, sz, sz, vp, vp, vp]
        L.och_ortho_stream_create.argtypes = [vp, vp, vp, vp, sz, _f64p, vp, i64, sz, C.POINTER(vp)]
        L.och_ortho_stream_destroy.argtypes = [vp]
        L.och_ortho_stream_destroy.restype = None
        L.och_ortho_stream_num_bands.argtypes = [vp]
        L.och_ortho_stream_num_bands.restype = sz
        for fn in (L.och_ortho_stream_band_cameras, L.och_ortho_stream_loads):
            fn.argtypes = [vp, sz, vp]
            fn.restype = sz
        L.och_ortho_stream_upload.argtypes = [vp, sz, u32, vp]
        L.och_ortho_stream_upload_jpegs.argtypes = [vp, sz, sz, vp, vp, vp, vp]
        L.och_ortho_stream_render.argtypes = [vp, sz, vp, C.c_int, vp, vp, vp, vp, u64, C.POINTER(u64), vp]
        L.och_ortho_stream_rewind.argtypes = [vp]
        L.och_ortho_stream_upload_end_ms.argtypes = [vp, sz, C.POINTER(f64)]
        L.och_ortho_stream_last_error.restype = C.c_char_p
        L.och_lab_convert.argtypes = [C.c_int, vp, sz, vp]
        L.och_lab_convert.restype = None
        L.och_ortho_patch_sample.argtypes = [vp, vp, f64, vp, vp, vp, vp]
        L.och_ortho_sample_fields.argtypes = [f64, f64, i32, i32, C.c_float, f64, vp]
        L.och_ortho_sample_fields.restype = None
        L.och_ortho_blend_render.argtypes = [vp, vp, vp, sz, _f64p, vp, i64, i64, sz, vp, vp, sz, vp, vp, C.c_int, vp, vp, vp,
                                             vp, vp, vp, vp]
        L.och_ortho_blend_last_error.restype = C.c_char_p
        L.och_laplacian_blend.argtypes = [i32, i32, i32, i32, vp, vp, vp]
        L.och_blend_chamfer.argtypes = [i32, i32, vp, vp]
        L.och_blend_chamfer.restype = None
        L.och_blend_pyr.argtypes = [C.c_int, i32, i32, i32, i32, i32, vp, vp]
        L.och_blend_pyr.restype = None
        L.och_blend_math.argtypes = [C.c_int, sz, vp, vp]
        L.och_blend_math.restype = None
        L.och_color_balance_solve.argtypes = [vp, vp, vp, sz, sz, vp, vp, sz, vp, vp, C.POINTER(sz), sz, vp, vp, C.POINTER(sz), vp]
        L.och_color_balance_evaluate.argtypes = [vp, vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp]
        L.och_color_balance_evaluate_plan.argtypes = [vp, sz, sz, vp, vp, sz, vp, vp, vp, vp, vp, vp, vp, vp]
        L.och_color_balance_remove_gauge.argtypes = [sz, vp, vp]
        L.och_color_balance_last_error.restype = C.c_char_p
        L.och_thumbnail_size.argtypes = [C.c_int, C.c_int, C.POINTER(i32), C.POINTER(i32)]
        L.och_image_thumbnails.argtypes = [vp, vp, u32, C.c_int, C.c_int, C.c_int, vp]
        L.och_graph_make_thumbnails.argtypes = [vp, vp, vp, u32, C.c_int, C.c_int, C.c_int, _u64p]
        L.och_thumbnail_last_error.restype = C.c_char_p
        L.och_ortho_overviews_levels.argtypes = [i64, i64, vp]
        L.och_ortho_overviews_create.argtypes = [vp, C.c_int, i64, i64, vp, C.c_int, C.POINTER(vp)]
        L.och_ortho_overviews_feed.argtypes = [vp, i64, i64, vp]
        L.och_ortho_overviews_complete_rows.argtypes = [vp, C.c_int]
        L.och_ortho_overviews_complete_rows.restype = i64
        L.och_ortho_overviews_finish.argtypes = [vp]
        L.och_ortho_overviews_destroy.argtypes = [vp]
        L.och_ortho_overviews_destroy.restype = None
        L.och_ortho_overviews_last_error.restype = C.c_char_p
        L.och_jpeg_create.argtypes = [vp, i64, i64, C.c_int, C.POINTER(vp)]
        L.och_jpeg_feed.argtypes = [vp, i64, i64, vp, C.c_int, C.c_int]
        L.och_jpeg_pending.argtypes = [vp]
        L.och_jpeg_pending.restype = i64
        L.och_jpeg_collect.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.och_jpeg_finish.argtypes = [vp]
        L.och_jpeg_destroy.argtypes = [vp]
        L.och_jpeg_destroy.restype = None
        L.och_jpeg_last_error.restype = C.c_char_p
        L.och_jpeg_info.argtypes = [vp, C.c_uint64, C.c_int, vp]
        L.och_jpeg_decoder_create.argtypes = [vp, C.c_int, C.POINTER(vp)]
        L.och_jpeg_decoder_decode.argtypes = [vp, i64, vp, vp, C.c_int, vp, C.c_uint64, vp, vp, vp]
        L.och_jpeg_decoder_destroy.argtypes = [vp]
        L.och_jpeg_decoder_destroy.restype = None
        L.och_jpeg_decode_last_error.restype = C.c_char_p
        L.och_geotiff_create.argtypes = [vp, C.c_int, i64, i64, C.c_int, C.POINTER(vp)]
        L.och_geotiff_create_layered.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.c_int, C.POINTER(vp)]
        L.och_geotiff_feed.argtypes = [vp, i64, i64, vp, C.c_int]
        L.och_geotiff_payloads.argtypes = [vp, vp, i64]
        L.och_geotiff_collect.argtypes = [vp, vp, C.c_uint64, C.POINTER(C.c_uint64), vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.och_geotiff_finish.argtypes = [vp]
        L.och_geotiff_destroy.argtypes = [vp]
        L.och_geotiff_destroy.restype = None
        L.och_geotiff_last_error.restype = C.c_char_p
        L.och_geotiff_reader_create.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(vp)]
        L.och_geotiff_reader_create_layered.argtypes = [vp, C.c_int, C.c_int, i64, i64, C.c_int, C.c_int, C.c_int, C.c_uint64, C.POINTER(vp)]
        L.och_geotiff_reader_inflate.argtypes = [vp, i64, vp, vp, vp, vp, C.c_uint64, vp, vp]
        L.och_geotiff_reader_read.argtypes = [vp, i64, vp, vp, i64, i64, vp, C.c_int, C.POINTER(i64)]
        L.och_geotiff_reader_launches.argtypes = [vp]
        L.och_geotiff_reader_launches.restype = i64
        L.och_geotiff_reader_destroy.argtypes = [vp]
        L.och_geotiff_reader_destroy.restype = None
        L.och_geotiff_read_last_error.restype = C.c_char_p
        L.och_deflate_code_lengths.argtypes = [vp, C.c_int, C.c_int, vp]
        L.och_png_encoder_create.argtypes = [vp, C.POINTER(vp)]
        L.och_png_encoder_encode.argtypes = [vp, i64, vp, C.c_int, C.c_int, vp, C.c_uint64, vp]
        L.och_png_encoder_destroy.argtypes = [vp]
        L.och_png_encoder_destroy.restype = None
        L.och_png_last_error.restype = C.c_char_p
        L.och_png_bound.argtypes = [i64, i64, i64, C.c_int]
        L.och_png_bound.restype = C.c_uint64
        L.och_png_filter.argtypes = [vp, vp, C.c_uint64]
        L.och_png_info.argtypes = [vp, C.c_uint64, vp]
        L.och_png_decode.argtypes = [vp, C.c_uint64, vp, C.POINTER(vp)]
        L.och_png_free.argtypes = [vp]
        L.och_png_free.restype = None
        L.och_graph_encode_thumbnails.argtypes = [vp, vp]
        L.och_graph_get_thumbnail.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz), vp]
        L.och_graph_decode_thumbnails.argtypes = [vp, vp]
        L.och_tile_progress_create.argtypes = [vp, _f64p, C.c_int32, C.c_int32, C.POINTER(vp)]
        L.och_tile_progress_feed.argtypes = [vp, C.c_int, i64, i64, C.c_int, vp, vp]
        L.och_tile_progress_seek.argtypes = [vp, C.c_int, i64]
        L.och_tile_progress_pending.argtypes = [vp]
        L.och_tile_progress_collect.argtypes = [vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.och_tile_progress_destroy.argtypes = [vp]
        L.och_tile_progress_destroy.restype = None
        L.och_tile_progress_last_error.restype = C.c_char_p
        L.och_graph_node_metadata.argtypes = [vp, sz]
        L.och_graph_node_metadata.restype = C.c_char_p
        L.och_graph_set_node_metadata.argtypes = [vp, sz, C.c_char_p, sz]
        L.och_jpeg_metadata.argtypes = [vp, C.c_uint64, _f64p, vp, C.c_uint64, C.POINTER(C.c_uint64)]
        L.och_geo_create.argtypes = [C.c_double, C.c_double]
        L.och_geo_create.restype = vp
        L.och_geo_destroy.argtypes = [vp]
        L.och_geo_destroy.restype = None
        L.och_geo_origin.argtypes = [vp, _f64p]
        L.och_geo_origin.restype = None
        L.och_geo_to_local.argtypes = [vp, sz, _f64p, _f64p]
        L.och_geo_to_local.restype = None
        L.och_geo_to_wgs84.argtypes = [vp, sz, _f64p, _f64p]
        L.och_geo_to_wgs84.restype = None
        L.och_geo_wkt.argtypes = [vp, vp, sz]
        L.och_geo_wkt.restype = sz
        L.och_graph_geojson.argtypes = [vp, vp, vp, sz, vp, sz, C.POINTER(sz)]
        L.och_graph_geojson.restype = vp
        _lib = L
    return _lib


def extract_features_batch(ctx, images_bgr, max_keypoints=20000, device_shape=None):
    """extract_features for a batch of equally sized BGR images on the device.  images_bgr: (n, h, w, 3) uint8
    host array, or - with device_shape=(n, h, w) - an integer device pointer to images already in HBM.  Returns
    a list of (loc [k x 2] f64, strength [k] f32, desc [k x 8] u64, num_sparse) per image."""
    L = load()
    if device_shape is None:
        imgs = np.ascontiguousarray(images_bgr, np.uint8)
        n, h, w, _ = imgs.shape
        src, on_dev = imgs.ctypes.data, 0
    else:
        n, h, w = device_shape
        src, on_dev = int(images_bgr), 1
    max_out = max_keypoints + 1   # the NMS seed re-enters the dense list (extract_features.cpp:63-83)
    loc = np.zeros((n, max_out, 2))
    st = np.zeros((n, max_out), np.float32)
    de = np.zeros((n, max_out, 8), np.uint64)
    counts, ns = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rc = L.och_extract_features_batch(ctx.h, src, n, w, h, max_keypoints, max_out, loc.ctypes.data,
                                      st.ctypes.data, de.ctypes.data, counts.ctypes.data, ns.ctypes.data, on_dev)
    if rc != 0:
        raise capi.OchipError("extract failed: " + L.och_extract_last_error().decode())
    return [(loc[i, :counts[i]].copy(), st[i, :counts[i]].copy(), de[i, :counts[i]].copy(), int(ns[i])) for i in range(n)]


def thumbnail_size(width, height):
    """(rows, cols) of the load stage's thumbnail of a width x height image: both sides scaled by 50 / sqrt(width * height)
    and rounded, ties to even.  Refused below 2 500 pixels and when a side comes out 0."""
    L = load()
    rows, cols = C.c_int32(0), C.c_int32(0)
    if L.och_thumbnail_size(int(width), int(height), C.byref(rows), C.byref(cols)) != 0:
        raise ValueError(L.och_thumbnail_last_error().decode())
    return rows.value, cols.value


def _image_batch(images_bgr, device_shape):
    """(keep-alive, pointer, n, h, w, on_device) of a batch given as extract_features_batch takes it"""
    if device_shape is None:
        imgs = np.ascontiguousarray(images_bgr, np.uint8)
        if imgs.ndim != 4 or imgs.shape[3] != 3:
            raise ValueError("images are (n, h, w, 3) uint8")
        n, h, w, _ = imgs.shape
        return imgs, imgs.ctypes.data, n, h, w, 0
    n, h, w = device_shape
    return None, int(images_bgr), n, h, w, 1


def image_thumbnails(images_bgr, ctx=None, device_shape=None):
    """The load stage's thumbnails of a batch of equally sized BGR images (extract_image.cpp:42-52: Lab, INTER_AREA by
    50 / sqrt(pixels), back, R G B): (n, rows, cols, 3) uint8.  images_bgr: (n, h, w, 3) uint8 host array or, with
    device_shape=(n, h, w) and a context, a device pointer.  ctx=None: the CPU route, bit for bit the device's."""
    L = load()
    keep, src, n, h, w, on_dev = _image_batch(images_bgr, device_shape)
    rows, cols = thumbnail_size(w, h)
    out = np.zeros((n, rows, cols, 3), np.uint8)
    if L.och_image_thumbnails(ctx.h if ctx is not None else None, src, n, w, h, on_dev, out.ctypes.data) != 0:
        raise capi.OchipError("image_thumbnails failed: " + L.och_thumbnail_last_error().decode())
    del keep
    return out


RELAX_SUMMARY_NAMES = ["solves", "iterations_total", "last_iterations", "initial_cost", "final_cost", "residual_blocks",
                       "setup_host_s", "device_s"]


def pack_edges(edges):
    """edges: list of dicts {src, dst, H (3x3) or None, px (k x 4), match_index (k,), dist (m,) or None}.
    Returns the flat arrays the stand-alone relax entry points (och_relax_ground_plane, och_relax) take."""
    n = len(edges)
    src = np.array([e["src"] for e in edges], np.uint64)
    dst = np.array([e["dst"] for e in edges], np.uint64)
    H = np.full((max(n, 1), 9), np.nan)
    ish = np.zeros(max(n, 1), np.uint8)
    for i, e in enumerate(edges):
        if e.get("H") is not None:
            H[i] = np.asarray(e["H"], np.float64).reshape(9)
            ish[i] = 1
    counts = [len(e["px"]) for e in edges]
    inl_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    px = np.ascontiguousarray(np.concatenate([np.asarray(e["px"], np.float64).reshape(-1, 4) for e in edges])
                              if n and sum(counts) else np.zeros((1, 4)))
    mi = np.ascontiguousarray(np.concatenate([np.asarray(e["match_index"], np.uint64) for e in edges])
                              if n and sum(counts) else np.zeros(1, np.uint64))
    dcounts = [0 if e.get("dist") is None else len(e["dist"]) for e in edges]
    dist_off = np.concatenate([[0], np.cumsum(dcounts)]).astype(np.uint64)
    dist = np.ascontiguousarray(np.concatenate([np.asarray(e["dist"], np.float64) for e in edges if e.get("dist") is not None])
                                if sum(dcounts) else np.zeros(1))
    return dict(src=src, dst=dst, H=np.ascontiguousarray(H), is_h=ish, inl_off=inl_off, px=px, match_index=mi,
                dist_off=dist_off, dist=dist)


RELAX_OPTIONS = dict(ORIENTATION=1 << 0, POSITION=1 << 1, GROUND_PLANE=1 << 2, GROUND_MESH=1 << 3, POINTS_3D=1 << 4,
                     FOCAL_LENGTH=1 << 5, PRINCIPAL_POINT=1 << 6, LENS_DISTORTIONS_RADIAL=1 << 7, BROWN2=1 << 8, BROWN24=1 << 9,
                     BROWN246=1 << 10, LENS_DISTORTIONS_TANGENTIAL=1 << 11, MINIMAL_MESH=1 << 12)
RELAX_SUMMARY12 = ["solves", "iterations_total", "last_iterations", "initial_cost", "final_cost", "residual_blocks",
                   "setup_host_s", "device_s", "track_blocks", "two_ray_blocks", "mesh_vertices", "unknowns"]


def relax_options(*names):
    bits = 0
    for n in names:
        bits |= RELAX_OPTIONS[n]
    return bits


class _Handle:
    """A native object of the host library behind `h` (library `L`): closed once, by close(), a with block or the
    collector, whichever comes first, and also when __init__ raised half-way.  _destroy and _last_error name the
    family's functions; _check(rc) turns a refused call into the family's exception with the library's text."""

    _destroy = None       # "och_..._destroy"
    _last_error = None    # "och_..._last_error"; None: the family keeps no text
    _failure = capi.OchipError

    def _error(self):
        return getattr(self.L, self._last_error)().decode()

    def _check(self, rc):
        if rc != 0:
            raise self._failure(self._error())
        return rc

    def _context(self):
        """the context whose pools the object's device blocks came from; None: the CPU route"""
        return getattr(self, "ctx", None)

    def _destroy_native(self):
        getattr(self.L, self._destroy)(self.h)

    def _released(self):
        """after every close: drop what was kept alive for the native object"""

    def close(self):
        if getattr(self, "h", None):
            ctx = self._context()
            # a context closed first has taken the device with it: nothing can be handed back to its pools then
            if ctx is None or getattr(ctx, "h", None):
                self._destroy_native()
        self.h = None
        self._released()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()


class Surface(_Handle):
    """surface_model of the host library: mesh (vertices, edges {source, dest, border, opposite 0, opposite 1}) + cloud."""

    _destroy = "och_surface_destroy"

    def __init__(self):
        self.L = load()
        self.h = self.L.och_surface_create()

    def arrays(self):
        nv, ne, nc = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self.L.och_surface_counts(self.h, C.byref(nv), C.byref(ne), C.byref(nc))
        v, e, c = np.zeros((max(nv.value, 1), 3)), np.zeros((max(ne.value, 1), 5), np.uint64), np.zeros((max(nc.value, 1), 3))
        self.L.och_surface_get(self.h, v.ctypes.data, e.ctypes.data, c.ctypes.data)
        return dict(vertices=v[:nv.value], edges=e[:ne.value], cloud=c[:nc.value])

    def set(self, vertices, edges, cloud=None):
        v = np.ascontiguousarray(vertices, np.float64).reshape(-1, 3)
        e = np.ascontiguousarray(edges, np.uint64).reshape(-1, 5)
        c = np.zeros((0, 3)) if cloud is None else np.ascontiguousarray(cloud, np.float64).reshape(-1, 3)
        pad = lambda a, shape, dt: a if len(a) else np.zeros(shape, dt)
        self.L.och_surface_set(self.h, len(v), pad(v, (1, 3), np.float64), len(e), pad(e, (1, 5), np.uint64), len(c),
                               pad(c, (1, 3), np.float64))
        return self


    def set_heights(self, z):
        """New vertex heights; the mesh's topology and container orders stay (what a relax does to a mesh)."""
        self.L.och_surface_set_heights(self.h, np.ascontiguousarray(z, np.float64))
        return self

    def clouds(self):
        """The surface's point clouds one by one (arrays() concatenates them)."""
        n = self.L.och_surface_num_clouds(self.h)
        sizes = np.zeros(max(n, 1), np.uint64)
        self.L.och_surface_cloud_sizes(self.h, sizes)
        pts, out, k = self.arrays()["cloud"], [], 0
        for i in range(n):
            out.append(pts[k:k + int(sizes[i])].copy())
            k += int(sizes[i])
        return out

    def set_clouds(self, clouds):
        sizes = np.array([len(c) for c in clouds] or [0], np.uint64)
        xyz = np.ascontiguousarray(np.concatenate([np.asarray(c, np.float64).reshape(-1, 3) for c in clouds])
                                   if len(clouds) and sizes.sum() else np.zeros((1, 3)))
        self.L.och_surface_set_clouds(self.h, len(clouds), sizes, xyz)
        return self

    def refine_by_point_density(self, max_points_per_triangle, min_distance_variance=0.0, max_iterations=10, min_triangle_size=0.0):
        """refineByPointDensity (src/surface/refine_mesh.cpp:827-909) with the surface's own clouds; returns triangles created."""
        return self.L.och_refine_by_point_density(self.h, max_points_per_triangle, min_distance_variance, max_iterations,
                                                  min_triangle_size)

    def refine_at_point(self, x, y, levels=1):
        return self.L.och_refine_at_point(self.h, x, y, levels)

    def count_points_per_triangle(self, ctx=None, flat=False):
        """countPointsPerTriangle: (vertices n x 3, counts n, distance variances n) in first-point order.  flat=True: by
        the flat locate table in host loops; ctx: by that table on the device - the same rows."""
        cap = 2 * max(len(self.arrays()["edges"]), 1)
        tri, st = np.zeros((cap, 3), np.uint64), np.zeros((cap, 2))
        if ctx is None and not flat:
            n = self.L.och_count_points_per_triangle(self.h, tri, st, cap)
        else:
            n = self.L.och_surface_count_points(self.h, ctx.h if ctx is not None else None, tri, st, cap)
            if n == C.c_size_t(-1).value:
                raise capi.OchipError("count_points_per_triangle failed: " + self.L.och_points_last_error().decode())
        return tri[:n], st[:n, 0].astype(np.int64), st[:n, 1]

    def locate(self, xy, ctx=None, max_steps=None, flat=False):
        """The triangle under every point (three vertices, 0xFFFFFFFFFFFFFFFF x 3 outside).  flat=True or max_steps: by the
        flat locate table in host loops, a walk of at most max_steps (100) triangles and then the exhaustive scan; ctx: the
        same on the device."""
        xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
        tri = np.zeros((max(len(xy), 1), 3), np.uint64)
        if ctx is None and max_steps is None and not flat:
            self.L.och_surface_locate(self.h, xy if len(xy) else np.zeros((1, 2)), len(xy), tri)
        elif self.L.och_surface_locate_on(self.h, ctx.h if ctx is not None else None, xy if len(xy) else np.zeros((1, 2)), len(xy),
                                          100 if max_steps is None else max_steps, tri) != 0:
            raise capi.OchipError("locate failed: " + self.L.och_points_last_error().decode())
        return tri[:len(xy)]

    def locate_table(self):
        """The mesh's flat locate table (csrc/mesh_locate.hpp) as arrays, in capi.MeshPoints.count's layout."""
        sizes = np.zeros(2, np.uint64)
        self.L.och_surface_locate_table_sizes(self.h, sizes)
        T, ns = int(sizes[0]), int(sizes[1])
        t = dict(vertex_xy=np.zeros((max(T, 1), 6)), neighbours=np.zeros((max(T, 1), 3), np.uint32), plane=np.zeros((max(T, 1), 6)),
                 cx=np.zeros(max(T, 1)), cy=np.zeros(max(T, 1)), start=np.zeros(max(ns, 1), np.uint32), items=np.zeros(max(T, 1), np.uint32))
        grid = np.zeros(4)
        self.L.och_surface_locate_table(self.h, t["vertex_xy"].ctypes.data, t["neighbours"].ctypes.data, t["plane"].ctypes.data,
                                        t["cx"].ctypes.data, t["cy"].ctypes.data, grid.ctypes.data, t["start"].ctypes.data,
                                        t["items"].ctypes.data)
        for k in ("vertex_xy", "neighbours", "plane", "cx", "cy", "items"):
            t[k] = t[k][:T]
        t["start"] = t["start"][:ns]
        t.update(x0=grid[0], y0=grid[1], cell=grid[2], nx=int(grid[3]))
        return t

    def save_ply(self, path):
        """serialize(MeshGraph, ostream) of the reference (ASCII PLY, src/io/serialize_MeshGraph.cpp)."""
        if self.L.och_surface_save_ply(self.h, str(path).encode()) != 0:
            raise IOError("cannot write %s" % path)

    def load_ply(self, path):
        if self.L.och_surface_load_ply(self.h, str(path).encode()) != 0:
            raise IOError("%s is not a surface PLY of the reference's layout" % path)
        return self


class PointCounter(_Handle):
    """A cloud kept for counts against changing meshes (host/mesh_points.hpp): on the device with ctx (uploaded once), in
    host memory without.  count(surface): count_points_per_triangle's rows for the surface's mesh and THIS cloud."""

    _destroy = "och_point_counter_destroy"

    def __init__(self, points, ctx=None, max_steps=100):
        self.L = load()
        xyz = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        self.h = self.L.och_point_counter_create(ctx.h if ctx is not None else None, xyz if len(xyz) else np.zeros((1, 3)), len(xyz),
                                                 max_steps)
        if not self.h:
            raise capi.OchipError("point counter: " + self.L.och_points_last_error().decode())
        self.exhausted = 0

    def count(self, surface):
        if not self.h:
            raise capi.OchipError("the point counter is closed")
        cap = 2 * max(len(surface.arrays()["edges"]), 1)
        tri, st, ex = np.zeros((cap, 3), np.uint64), np.zeros((cap, 2)), np.zeros(1, np.uint64)
        n = self.L.och_point_counter_count(self.h, surface.h, tri, st, cap, ex)
        if n == C.c_size_t(-1).value:
            raise capi.OchipError("point counter: " + self.L.och_points_last_error().decode())
        self.exhausted = int(ex[0])
        return tri[:n], st[:n, 0].astype(np.int64), st[:n, 1]


def validate_checkpoint(path):
    """validateCheckpoint (src/io/checkpoint.cpp:318-337)."""
    return bool(load().och_checkpoint_validate(str(path).encode()))


def save_checkpoint(path, graph, surfaces=(), state="INITIAL_PROCESSING", state_run_count=0, origin=(0.0, 0.0),
                    encode_thumbnails=False, ctx=None):
    """saveCheckpoint (src/io/checkpoint.cpp:155-231): metadata.json, graph.json, surface_<i>.ply, pointcloud_<i>_<j>.xyz.
    encode_thumbnails: the nodes' decoded thumbnails go into graph.json as base64 PNGs first (Graph.encode_thumbnails(ctx))."""
    L = load()
    if encode_thumbnails:
        graph.encode_thumbnails(ctx)
    arr = (C.c_void_p * max(len(surfaces), 1))(*[s.h for s in surfaces])
    info = np.array([state_run_count, origin[0], origin[1], 0.0])
    if L.och_checkpoint_save(str(path).encode(), graph.h, arr, len(surfaces), state.encode(), info) != 0:
        raise IOError(L.och_last_error(graph.h).decode())


def load_checkpoint(path, decode_thumbnails=False):
    """loadCheckpoint (src/io/checkpoint.cpp:233-316).  Returns (Graph, [Surface], info dict).  decode_thumbnails: the
    nodes' base64 PNG thumbnails are decoded for the preview (Graph.decode_thumbnails; a refused one leaves its node bare)."""
    L = load()
    g = Graph()
    cp = L.och_checkpoint_load(str(path).encode(), g.h)
    if not cp:
        raise IOError(L.och_last_error(g.h).decode())
    g._refresh_ids()
    if decode_thumbnails:
        g.decode_thumbnails()
    try:
        surfaces = []
        for i in range(L.och_checkpoint_num_surfaces(cp)):
            s = Surface()
            L.och_checkpoint_get_surface(cp, i, s.h)
            surfaces.append(s)
        info = np.zeros(4)
        L.och_checkpoint_info(cp, info)
        meta = dict(state=L.och_checkpoint_state(cp).decode(), state_run_count=int(info[0]), origin=(info[1], info[2]))
    finally:
        L.och_checkpoint_destroy(cp)
    return g, surfaces, meta


def rebuild_mesh(cam_xyz, previous=None, minimal=False):
    """rebuildMesh / buildMinimalMesh of the host library (no device involved)."""
    cam_xyz = np.ascontiguousarray(cam_xyz, np.float64).reshape(-1, 3)
    s = Surface()
    s.L.och_rebuild_mesh(cam_xyz, len(cam_xyz), previous.h if previous is not None else None, int(minimal), s.h)
    return s


# ---- the filtered point cloud file and the textured OBJ (include/oc_host.h) -----------------------
def _export_error(what):
    return capi.OchipError(f"{what}: " + load().och_export_last_error().decode())


def _cloud_source(surfaces):
    """(entry prefix, first arguments): a list of Surface objects, or a flat array xyz [n][3]."""
    if isinstance(surfaces, np.ndarray):
        xyz = np.ascontiguousarray(surfaces, np.float64).reshape(-1, 3)
        return "och_xyz", (xyz.ctypes.data if len(xyz) else None, len(xyz)), xyz
    arr, n = _surface_array(surfaces)
    return "och_cloud", (arr, n), surfaces


def _take_text(L, p, n):
    try:
        return C.string_at(p, n)
    finally:
        L.och_free(p)


def cloud_outlier_bounds(surfaces, ctx=None):
    """filterOutliers (src/io/saveXYZ.cpp:50-105) over all clouds of the surfaces (or a flat array [n][3]): the box as
    ((first, second),) * 3.  ctx: counted on the device, else in host loops - the same box."""
    L = load()
    prefix, args, keep = _cloud_source(surfaces)
    b = np.zeros(6, np.int64)
    fn = L.och_xyz_outlier_bounds if prefix == "och_xyz" else L.och_cloud_outlier_bounds
    if fn(*args, ctx.h if ctx is not None else None, b.ctypes.data) != 0:
        raise _export_error("cloud_outlier_bounds")
    return tuple((int(b[2 * a]), int(b[2 * a + 1])) for a in range(3))


def cloud_to_xyz(surfaces, bounds="filter", ctx=None, want_kept=False):
    """toXYZ (src/io/saveXYZ.cpp:6-48): the point cloud file's bytes.  bounds: "filter" = cloud_outlier_bounds' box, None =
    every point, or a box ((first, second),) * 3.  ctx: formatted on the device, else in host loops - the same bytes."""
    L = load()
    if isinstance(bounds, str):
        if bounds != "filter":
            raise ValueError('bounds: "filter", None or three (first, second) pairs')
        bounds = cloud_outlier_bounds(surfaces, ctx)
    b = capi.bounds6(bounds)
    prefix, args, keep = _cloud_source(surfaces)
    fn = L.och_xyz_to_text if prefix == "och_xyz" else L.och_cloud_to_xyz
    n, kept = C.c_size_t(0), C.c_uint64(0)
    p = fn(*args, ctx.h if ctx is not None else None, b.ctypes.data if b is not None else None, C.byref(n), C.byref(kept))
    if not p:
        raise _export_error("cloud_to_xyz")
    text = _take_text(L, p, n.value)
    return (text, kept.value) if want_kept else text


def save_pointcloud(path, surfaces, ctx=None):
    """The runner's point cloud file: toXYZ(surfaces, out, filterOutliers(surfaces)).  Returns the box."""
    L = load()
    bounds = cloud_outlier_bounds(surfaces, ctx)
    arr, n = _surface_array(surfaces)
    if L.och_cloud_save_xyz(arr, n, ctx.h if ctx is not None else None, capi.bounds6(bounds).ctypes.data, str(path).encode()) != 0:
        raise _export_error("save_pointcloud")
    return bounds


def format_g6(values, fallback=True):
    """`ostream << double` of every value as bytes.  fallback=False: the integer formatter of csrc/xyz_export.hpp alone, b""
    where it declines (|v| outside [1e-5, 2^63) and not 0)."""
    L = load()
    v = np.ascontiguousarray(values, np.float64).reshape(-1)
    text, ln = np.zeros((max(len(v), 1), 16), np.uint8), np.zeros(max(len(v), 1), np.uint8)
    L.och_format_g6(v.ctypes.data, len(v), int(fallback), text.ctypes.data, ln.ctypes.data)
    return text[:len(v)].view("S16").reshape(-1), ln[:len(v)]


def textured_obj(surfaces, plan_or_geometry, name):
    """The OBJ and MTL text of generateTexturedOBJ (src/ortho/ortho.cpp:2125-2255) for meshes over an orthomosaic: `name`.mtl
    and `name`.jpg are the names the texts refer to.  plan_or_geometry: the plan the mosaic was rendered with (dsm_plan), or
    (width, height, min_x, max_y, gsd_x, gsd_y).  Returns (obj_text, mtl_text) as bytes."""
    L = load()
    if isinstance(plan_or_geometry, dict):
        p = plan_or_geometry
        geometry = (p["width"], p["height"], p["min_x"], p["max_y"], p["gsd"], p["gsd"])
    else:
        geometry = tuple(plan_or_geometry)
    w, h, min_x, max_y, gsd_x, gsd_y = geometry
    arr, n = _surface_array(surfaces)
    obj, mtl, no, nm = C.c_void_p(), C.c_void_p(), C.c_size_t(0), C.c_size_t(0)
    if L.och_textured_obj(arr, n, int(w), int(h), float(min_x), float(max_y), float(gsd_x), float(gsd_y), (name + ".mtl").encode(),
                          (name + ".jpg").encode(), C.byref(obj), C.byref(no), C.byref(mtl), C.byref(nm)) != 0:
        raise _export_error("textured_obj")
    return _take_text(L, obj.value, no.value), _take_text(L, mtl.value, nm.value)


def save_textured_obj(path, surfaces, rgba, plan, jpeg=False, ctx=None, quality=95):
    """The runner's 3-D model: `path`.obj (a trailing .obj is dropped first, as in the reference) and .mtl are written, the
    texture - the orthomosaic's first three channels, H x W x 3 - is returned for the caller's encoder.  path=None: nothing
    is written, (obj_text, mtl_text, texture) is returned, the names built from "model".
    rgba: the mosaic ortho_mosaic rendered with `plan`.
    jpeg=True: `path`.jpg, the name the MTL refers to, is written too (encode_jpeg: ctx None the CPU route, else on ctx's
    device, where rgba may be a CUDA tensor), and the texture returned - alone, or as the third value with path=None - is the
    file's bytes instead of the pixels."""
    return _save_textured_obj(path, surfaces, rgba, plan, plan["width"], plan["height"], jpeg, ctx, quality)


def _save_textured_obj(path, surfaces, rgba, plan, pw, ph, jpeg, ctx, quality):
    """save_textured_obj with the mosaic's size named: plan is the plan or textured_obj's geometry tuple"""
    if jpeg and not isinstance(rgba, np.ndarray) and hasattr(rgba, "is_cuda"):
        shape = tuple(int(v) for v in rgba.shape)
    else:
        rgba = np.asarray(rgba)
        shape = rgba.shape
    if len(shape) != 3 or shape[2] < 3 or shape[:2] != (ph, pw):
        raise ValueError(f"rgba {shape} is not the plan's {ph} x {pw} mosaic")
    base = "model" if path is None else str(path)
    if base.endswith(".obj"):
        base = base[:-4]
    obj, mtl = textured_obj(surfaces, plan, os.path.basename(base))
    if jpeg:
        texture = encode_jpeg(rgba if shape[2] in (3, 4) else rgba[:, :, :3], ctx=ctx, quality=quality)
    else:
        texture = np.ascontiguousarray(rgba[:, :, :3])
    if path is None:
        return obj, mtl, texture
    with open(base + ".obj", "wb") as f:
        f.write(obj)
    with open(base + ".mtl", "wb") as f:
        f.write(mtl)
    if jpeg:
        with open(base + ".jpg", "wb") as f:
            f.write(texture)
    return texture


# ---- orthomosaic preview and DSM raster (include/oc_host.h; src/ortho/ortho.cpp) ---------------------------------------
PLAN_KEYS = ("width", "height", "gsd", "min_x", "max_x", "min_y", "max_y", "mean_camera_z")


def _surface_array(surfaces):
    surfaces = list(surfaces)
    return (C.c_void_p * max(len(surfaces), 1))(*[s.h for s in surfaces]), len(surfaces)


def _plan_dict(plan8):
    d = dict(zip(PLAN_KEYS, plan8.tolist()))
    d["width"], d["height"] = int(d["width"]), int(d["height"])
    return d


def _plan_array(plan):
    return np.array([plan[k] for k in PLAN_KEYS], np.float64)


def ortho_bounds(surfaces):
    """calculateBoundsAndMeanZ (src/ortho/ortho.cpp:283-342)."""
    arr, n = _surface_array(surfaces)
    out = np.zeros(5)
    load().och_ortho_bounds(arr, n, out)
    return dict(zip(("min_x", "max_x", "min_y", "max_y", "mean_surface_z"), out.tolist()))


def ortho_gsd(graph, node_ids, mean_surface_z, thumbnail=True):
    """calculateGSD (src/ortho/ortho.cpp:344-377) over node_ids in the given order."""
    ids = np.ascontiguousarray(node_ids, np.uint64)
    return load().och_ortho_gsd(graph.h, ids if len(ids) else np.zeros(1, np.uint64), len(ids), mean_surface_z, int(thumbnail))


def ortho_context(graph, surfaces, thumbnail=True):
    """prepareOrthoMosaicContext (src/ortho/ortho.cpp:379-414) without the k-d tree: bounds, gsd, camera heights and the
    number of involved nodes."""
    arr, n = _surface_array(surfaces)
    out = np.zeros(8)
    k = load().och_ortho_context(graph.h, arr, n, int(thumbnail), out)
    d = dict(zip(("min_x", "max_x", "min_y", "max_y", "mean_surface_z", "gsd", "mean_camera_z", "average_camera_elevation"),
                 out.tolist()))
    d["involved"] = int(k)
    return d


def ortho_clamp_resolution(total_input_pixels, gsd, width, height):
    """clampOutputResolution (src/ortho/ortho.cpp:228-256) with the input pixel count given: (gsd, width, height)."""
    g, w, h = C.c_double(gsd), C.c_int32(width), C.c_int32(height)
    load().och_ortho_clamp_resolution(int(total_input_pixels), C.byref(g), C.byref(w), C.byref(h))
    return g.value, w.value, h.value


def ortho_clamp_megapixels(max_output_megapixels, gsd, width, height):
    """clampOutputMegapixels (src/ortho/ortho.cpp:258-281): (gsd, width, height)."""
    g, w, h = C.c_double(gsd), C.c_int32(width), C.c_int32(height)
    load().och_ortho_clamp_megapixels(float(max_output_megapixels), C.byref(g), C.byref(w), C.byref(h))
    return g.value, w.value, h.value


def ray_trace_height(x, y, mean_camera_z, surfaces):
    """rayTraceHeight (src/ortho/ortho.cpp:462-472): NaN where no surface holds (x, y)."""
    arr, n = _surface_array(surfaces)
    return load().och_ray_trace_height(arr, n, x, y, mean_camera_z)


def orthomosaic_thumbnail(graph, surfaces, ctx=None, z_in=None, want_z=False):
    """generateOrthomosaic (src/ortho/ortho.cpp:478-653): the preview raster from the nodes' thumbnails
    (Graph.set_thumbnail).  ctx: on that device; None: the CPU route, whose heights are z_in when given.
    Returns the plan's keys plus rgba (height x width x 4 uint8), ids (uint32) and, with want_z, z (fp64)."""
    L = load()
    arr, n = _surface_array(surfaces)
    plan8 = np.zeros(8)
    L.och_orthomosaic_thumbnail(graph.h, ctx.h if ctx is not None else None, arr, n, None, plan8, None, None, None)
    out = _plan_dict(plan8)
    h, w = out["height"], out["width"]
    rgba, ids = np.zeros((h, w, 4), np.uint8), np.zeros((h, w), np.uint32)
    z = np.zeros((h, w)) if want_z else None
    zi = None
    if z_in is not None:
        zi = np.ascontiguousarray(z_in, np.float64)
        if zi.shape != (h, w):
            raise ValueError(f"z_in must be {h} x {w}")
    rc = L.och_orthomosaic_thumbnail(graph.h, ctx.h if ctx is not None else None, arr, n,
                                     None if zi is None else zi.ctypes.data, plan8, rgba.ctypes.data, ids.ctypes.data,
                                     None if z is None else z.ctypes.data)
    if rc != 0:
        raise capi.OchipError("orthomosaic thumbnail failed: " + L.och_last_error(graph.h).decode())
    out.update(rgba=rgba, ids=ids)
    if want_z:
        out["z"] = z
    return out


def dsm_plan(graph, surfaces, max_output_megapixels=0.0):
    """The full-resolution DSM raster of generateDSMGeoTIFF (src/ortho/ortho.cpp:866-897): width, height, gsd, bounds,
    mean_camera_z."""
    arr, n = _surface_array(surfaces)
    plan8 = np.zeros(8)
    load().och_dsm_plan(graph.h, arr, n, float(max_output_megapixels), plan8)
    return _plan_dict(plan8)


class OrthoMesh(_Handle):
    """The surfaces' triangle table on the device (ochip_ortho_mesh), for rendering DSM bands."""

    _last_error = "och_ortho_last_error"

    def __init__(self, ctx, surfaces):
        self.L, self.ctx = load(), ctx
        arr, n = _surface_array(surfaces)
        self.h = C.c_void_p()
        if self.L.och_ortho_mesh_upload(ctx.h, arr, n, C.byref(self.h)) != 0:
            raise capi.OchipError("ortho mesh upload failed: " + self._error())

    def _destroy_native(self):
        capi.load().ochip_ortho_mesh_destroy(self.h)  # the table is the device library's own object


def dsm_render(plan, surfaces=(), mesh=None, row0=0, rows=None, out=None, debug=False):
    """DSM rows [row0, row0 + rows) of `plan` (dsm_plan) as float32, NaN where no surface holds the pixel.  mesh (an
    OrthoMesh): on its device, into `out` when that is a float32 CUDA tensor of rows x width (returned as is), else into a
    new host array; mesh None: the CPU route over `surfaces`.  debug: also the triangle index, the fp64 heights and (CPU
    route) the walks that ran out of steps, as (z, tri, z64, capped)."""
    L = load()
    rows = plan["height"] - row0 if rows is None else rows
    w = plan["width"]
    arr, n = _surface_array(surfaces)
    on_device = out is not None and not isinstance(out, np.ndarray)
    if on_device:
        if mesh is None:
            raise ValueError("a device output needs the device route (mesh)")
        if tuple(out.shape) != (rows, w) or str(out.dtype) != "torch.float32" or not out.is_cuda or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 device tensor of {rows} x {w}")
        if out.device.index != mesh.ctx.device:
            raise ValueError(f"out is on cuda:{out.device.index}, the mesh's context on device {mesh.ctx.device}")
        # the kernel runs on the context's own (non-blocking) stream: whatever torch still has queued on its current
        # stream - the fill that made `out`, a reader of the block the allocator just handed out again - finishes first.
        # The call returns after the band is written, so torch's later work on `out` is ordered after it.
        import torch

        torch.cuda.current_stream(out.device).synchronize()
        ptr = out.data_ptr()
    else:
        out = np.zeros((rows, w), np.float32) if out is None else out
        if out.shape != (rows, w) or out.dtype != np.float32 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous float32 array of {rows} x {w}")
        ptr = out.ctypes.data
    tri = np.zeros((rows, w), np.uint32) if debug else None
    z64 = np.zeros((rows, w)) if debug else None
    capped = C.c_uint64(0)
    rc = L.och_dsm_render(mesh.ctx.h if mesh is not None else None, mesh.h if mesh is not None else None, arr, n,
                          _plan_array(plan), int(row0), int(rows), ptr, int(on_device),
                          None if tri is None else tri.ctypes.data, None if z64 is None else z64.ctypes.data, C.byref(capped))
    if rc != 0:
        raise capi.OchipError(L.och_ortho_last_error().decode())
    return (out, tri, z64, int(capped.value)) if debug else out


# ---- layered full-resolution orthomosaic (include/oc_host.h; src/ortho/ortho.cpp:1206-1663) ----------------------------
# ochip_color_corr (include/ochip.h): a ColorCorrespondence and where it was taken
CORR_DTYPE = np.dtype([("lab_a", np.float32, 3), ("lab_b", np.float32, 3), ("camera_id_a", np.uint64),
                       ("camera_id_b", np.uint64), ("model_id_a", np.uint32), ("model_id_b", np.uint32),
                       ("normalized_radius_a", np.float32), ("normalized_radius_b", np.float32),
                       ("view_angle_a", np.float32), ("view_angle_b", np.float32), ("normalized_x_a", np.float32),
                       ("normalized_y_a", np.float32), ("normalized_x_b", np.float32), ("normalized_y_b", np.float32),
                       ("row", np.int32), ("col", np.int32), ("layer_a", np.uint32), ("layer_b", np.uint32)])
assert CORR_DTYPE.itemsize == 96
# OrthoMosaicConfig's defaults (include/opencalibration/ortho/ortho.hpp)
LAYERS_CONFIG = dict(num_layers=2, tile_size=1024, correspondence_kernel_radius=2, correspondence_subsample=50)


def _layers_config(config):
    cfg = dict(LAYERS_CONFIG, **(config or {}))
    unknown = set(cfg) - set(LAYERS_CONFIG)
    if unknown:
        raise ValueError(f"unknown layered-orthomosaic settings {sorted(unknown)}")
    return cfg, np.array([cfg[k] for k in ("num_layers", "tile_size", "correspondence_kernel_radius",
                                           "correspondence_subsample")], np.int32)


def ortho_layers_cameras(graph, surfaces):
    """The involved nodes' camera records of the layered render: cams (n x 28), node_ids, model_ids, image_hw (n x 2).
    images[i] of ortho_layers belongs to node_ids[i]."""
    L = load()
    arr, n = _surface_array(surfaces)
    k = L.och_ortho_layers_cameras(graph.h, arr, n, None, None, None, None)
    cams, ids = np.zeros((k, 28)), np.zeros(k, np.uint64)
    models, hw = np.zeros(k, np.uint32), np.zeros((k, 2), np.int64)
    L.och_ortho_layers_cameras(graph.h, arr, n, cams.ctypes.data, ids.ctypes.data, models.ctypes.data, hw.ctypes.data)
    return dict(cams=cams, node_ids=ids, model_ids=models, image_hw=hw)


def ortho_image_paths(graph, surfaces):
    """The involved nodes' image paths in ortho_layers_cameras' order (node_payload(...)["path"] of each): what
    ortho_mosaic_streamed takes as files= when the graph's nodes carry their paths, as a checkpoint's graph.json does."""
    index_of = {nid: i for i, nid in enumerate(graph.node_ids)}
    return [graph.L.och_graph_node_path(graph.h, index_of[int(nid)]).decode("utf-8")
            for nid in ortho_layers_cameras(graph, surfaces)["node_ids"]]


def _corr_bound(rows, width, cfg):
    """At most this many records in a band: every sampled pixel (boundary: (r + c) % s == 0 per tile row, else the
    multiples of s) times C(num_layers, 2)."""
    t, s, nl = cfg["tile_size"], cfg["correspondence_subsample"], cfg["num_layers"]
    if s <= 0 or nl < 2:
        return 0
    total = 0
    for r0 in range(0, rows, t):
        th = min(t, rows - r0)
        for c0 in range(0, width, t):
            tw = min(t, width - c0)
            total += th * -(-tw // s) + -(-th // s) * -(-tw // s)
    return total * nl * (nl - 1) // 2


def ortho_layers(plan, graph, surfaces, images, mesh=None, row0=0, tile_rows=None, config=None, out=None, dsm=None,
                 debug_knn=False, subset=None):
    """Rows of tile rows [row0 / tile_size, + tile_rows) of the layered full-resolution orthomosaic (processLayeredTile,
    src/ortho/ortho.cpp:1206-1429) over `plan` (dsm_plan).  images: one BGR uint8 array per involved node
    (ortho_layers_cameras' order), pixels_rows x pixels_cols x 3: numpy arrays for the CPU route, CUDA tensors (or raw
    device pointers, int) for the device route.  mesh (an OrthoMesh): on its device; None: the CPU route, whose heights
    are `dsm` (float32, rows x width) when given.  config overrides OrthoMosaicConfig's defaults (LAYERS_CONFIG).
    out (device route): dict of CUDA tensors bgra (L, rows, width, 4) uint8, camera_id (L, rows, width) int64 (the uint64
    ids' bits) and optionally weight (L, rows, width) float32, written in place.
    subset (ascending indices into ortho_layers_cameras' order): render from these cameras alone, images[j] belonging to
    camera subset[j]; with the band's set of ortho_band_cameras (or more) the result equals the full table's bit for bit.
    Returns dict(bgra, camera_id, weight, correspondences (CORR_DTYPE), row0, rows[, knn])."""
    L = load()
    cfg, config4 = _layers_config(config)
    t = cfg["tile_size"]
    if row0 % t:
        raise ValueError(f"row0 {row0} is not on a tile row (tile_size {t})")
    rows = plan["height"] - row0 if tile_rows is None else min(tile_rows * t, plan["height"] - row0)
    w, nl = plan["width"], cfg["num_layers"]
    arr, n = _surface_array(surfaces)
    on_device = out is not None
    keep, tensor_images = [], False
    ptrs, hw = [], []
    for im in images:
        if isinstance(im, int):
            ptrs.append(im)
            hw.append(None)
            continue
        if isinstance(im, np.ndarray):
            if mesh is not None:
                raise ValueError("the device route reads device images (CUDA tensors or device pointers)")
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3:
                raise ValueError("an image is rows x cols x 3 uint8")
            im = np.ascontiguousarray(im)
            keep.append(im)
            ptrs.append(im.ctypes.data)
        else:
            if mesh is None:
                raise ValueError("the CPU route reads host images (numpy arrays)")
            if str(im.dtype) != "torch.uint8" or im.dim() != 3 or im.shape[2] != 3 or not im.is_cuda or not im.is_contiguous():
                raise ValueError("a device image is a contiguous rows x cols x 3 uint8 CUDA tensor")
            ptrs.append(im.data_ptr())
            tensor_images = True
        hw.append(tuple(im.shape[:2]))
    cams = ortho_layers_cameras(graph, surfaces)
    if subset is None:
        which = range(len(cams["node_ids"]))
        if len(ptrs) != len(cams["node_ids"]):
            raise ValueError(f"{len(ptrs)} images for {len(cams['node_ids'])} involved nodes")
    else:
        subset = np.ascontiguousarray(subset, np.uint32).reshape(-1)
        if len(ptrs) != len(subset):
            raise ValueError(f"{len(ptrs)} images for a subset of {len(subset)} cameras")
        which = subset.tolist()
    # raw pointers carry the model's size: the caller vouches for it (a camera out of range is the library's to refuse)
    sizes = cams["image_hw"]
    hw = np.array([h if h is not None else tuple(sizes[i]) if i < len(sizes) else (0, 0) for i, h in zip(which, hw)],
                  np.int64).reshape(-1, 2)
    ptr_arr = np.array(ptrs, np.uint64)
    if tensor_images and not on_device:
        import torch

        torch.cuda.current_stream(mesh.ctx.device).synchronize()  # the images' uploads finish first
    h_ctx, h_mesh = (mesh.ctx.h, mesh.h) if mesh is not None else (None, None)
    images_p, hw_p = ptr_arr.ctypes.data if len(ptr_arr) else None, hw.ctypes.data if len(hw) else None

    def call(*outputs):
        if subset is None:
            return L.och_ortho_layers_render(graph.h, h_ctx, h_mesh, arr, n, _plan_array(plan), config4.ctypes.data, int(row0),
                                             int(rows), images_p, hw_p, *outputs)
        return L.och_ortho_layers_render_subset(graph.h, h_ctx, h_mesh, arr, n, _plan_array(plan), config4.ctypes.data, int(row0),
                                                int(rows), subset.ctypes.data, len(subset), images_p, hw_p, *outputs)

    return _layers_band(call, L.och_ortho_layers_last_error, cfg, w, row0, rows, mesh, out, dsm, debug_knn)


def _layers_band(call, last_error, cfg, w, row0, rows, mesh, out, dsm, debug_knn):
    """The outputs of one band of the layered render, shared by ortho_layers and OrthoStream.render: call(dsm, on_device,
    bgra, ids, weight, corr, capacity, n_corr, knn) is the entry point with everything before those arguments bound."""
    nl, on_device = cfg["num_layers"], out is not None
    if on_device:
        if mesh is None:
            raise ValueError("device outputs need the device route (mesh)")
        import torch

        shapes = dict(bgra=(nl, rows, w, 4), camera_id=(nl, rows, w), weight=(nl, rows, w))
        dtypes = dict(bgra="torch.uint8", camera_id="torch.int64", weight="torch.float32")
        for k in ("bgra", "camera_id") + (("weight",) if out.get("weight") is not None else ()):
            o = out[k]
            if tuple(o.shape) != shapes[k] or str(o.dtype) != dtypes[k] or not o.is_cuda or not o.is_contiguous() or \
                    o.device.index != mesh.ctx.device:
                raise ValueError(f"out[{k!r}] must be a contiguous {dtypes[k]} tensor of {shapes[k]} on device {mesh.ctx.device}")
        # the kernels run on the context's own stream: torch's queued work (the allocations' fills) finishes first
        torch.cuda.current_stream(out["bgra"].device).synchronize()
        bgra, ids, weight = out["bgra"], out["camera_id"], out.get("weight")
        p_bgra, p_ids, p_w = bgra.data_ptr(), ids.data_ptr(), None if weight is None else weight.data_ptr()
    else:
        bgra, ids, weight = np.zeros((nl, rows, w, 4), np.uint8), np.zeros((nl, rows, w), np.uint64), np.zeros((nl, rows, w), np.float32)
        p_bgra, p_ids, p_w = bgra.ctypes.data, ids.ctypes.data, weight.ctypes.data
    dsm_p = None
    if dsm is not None:
        if mesh is not None:
            raise ValueError("dsm is the CPU route's input")
        dsm = np.ascontiguousarray(dsm, np.float32)
        if dsm.shape != (rows, w):
            raise ValueError(f"dsm must be {rows} x {w}")
        dsm_p = dsm.ctypes.data
    cap = _corr_bound(rows, w, cfg)
    corr = np.zeros(max(cap, 1), CORR_DTYPE)
    knn = np.zeros((rows, w, 5), np.uint32) if debug_knn else None
    n_corr = C.c_uint64(0)
    rc = call(dsm_p, int(on_device), p_bgra, p_ids, p_w, corr.ctypes.data, cap, C.byref(n_corr),
              None if knn is None else knn.ctypes.data)
    if rc != 0:
        raise capi.OchipError(last_error().decode())
    if n_corr.value > cap:
        raise capi.OchipError(f"{n_corr.value} correspondences exceed their bound {cap}")
    res = dict(bgra=bgra, camera_id=ids, weight=weight, correspondences=corr[:n_corr.value], row0=row0, rows=rows)
    if knn is not None:
        res["knn"] = knn
    return res


def ortho_layers_bands(plan, graph, surfaces, images, mesh=None, tile_rows=1, config=None):
    """ortho_layers over the whole raster, tile_rows output tile rows per band, in raster order (generateLayeredGeoTIFF's
    tile loop, src/ortho/ortho.cpp:1513-1600, row-major): yields each band's result."""
    cfg, _ = _layers_config(config)
    for row0 in range(0, plan["height"], tile_rows * cfg["tile_size"]):
        yield ortho_layers(plan, graph, surfaces, images, mesh=mesh, row0=row0, tile_rows=tile_rows, config=config)


# ---- the layered render with streamed source images (csrc/host/ortho_stream.cpp, ortho_residency.hpp) ------------------
def ortho_band_cameras(plan, graph, surfaces, tile_rows=1, config=None, ctx=None):
    """The cameras each band of tile_rows output tile rows can read: a bool array (n_bands, n_cameras) over
    ortho_layers_cameras' order, True where the camera is among the 5 nearest in XY of at least one pixel of the band
    (whatever the pixel's height: no mesh is needed).  ctx (a capi.Context): on its device; None: the CPU route."""
    L = load()
    cfg, _ = _layers_config(config)
    cams = ortho_layers_cameras(graph, surfaces)["cams"]
    band_rows = tile_rows * cfg["tile_size"]
    n_bands = -(-plan["height"] // band_rows)
    used = np.zeros((n_bands, len(cams)), np.uint8)
    raster4 = np.array([plan["min_x"], plan["max_y"], plan["gsd"], plan["mean_camera_z"]])
    rc = L.och_ortho_band_cameras(ctx.h if ctx is not None else None, raster4, plan["width"], plan["height"], band_rows, len(cams),
                                  cams.ctypes.data, used.ctypes.data)
    if rc != 0:
        raise capi.OchipError(L.och_ortho_layers_last_error().decode())
    return used.astype(bool)


LOAD_AHEAD, LOAD_LATE = 0, 1


def ortho_residency_plan(used, capacity, resident=None):
    """The loads of a streamed render (ortho_residency.hpp's rule) for the bands' sets used (n_bands, n_cameras) and
    `capacity` image slots, from the slots' state resident (camera per slot, -1 free; None: all free).  Returns (per band a
    list of (camera, slot, phase) with phase LOAD_AHEAD or LOAD_LATE, the slots' state after the last band)."""
    L = load()
    used = np.ascontiguousarray(np.asarray(used).astype(bool), np.uint8)
    if used.ndim != 2:
        raise ValueError("used is (n_bands, n_cameras)")
    state = np.full(max(int(capacity), 0), -1, np.int32) if resident is None else np.array(resident, np.int32)
    if len(state) != capacity:
        raise ValueError(f"resident names {len(state)} slots, the capacity is {capacity}")
    off = np.zeros(used.shape[0] + 1, np.uint64)
    loads = np.zeros((max(int(used.sum()), 1), 3), np.int32)
    if L.och_ortho_residency_plan(used.ctypes.data, used.shape[0], used.shape[1], int(capacity), state.ctypes.data,
                                  off.ctypes.data, loads.ctypes.data) != 0:
        raise capi.OchipError(L.och_ortho_stream_last_error().decode())
    return [[tuple(int(v) for v in l) for l in loads[int(off[k]):int(off[k + 1])]] for k in range(used.shape[0])], state


class OrthoStream(_Handle):
    """The layered render of `plan` in bands of tile_rows output tile rows, its source images streamed through `capacity`
    device slots (och_ortho_stream_*).  mesh (an OrthoMesh): on its device, the slots one block of its context's pool;
    None: the CPU route with the slots in host memory.  The caller drives it: for band k upload(k, camera, image) every
    load of loads(k) - the ahead ones may go out before render(k - 1), so that they overlap it when the image is
    page-locked - then render(k); bands ascend, rewind() starts a further sweep from the images the slots hold.  A call
    out of the plan's order raises OchipError and launches nothing."""

    _destroy, _last_error = "och_ortho_stream_destroy", "och_ortho_stream_last_error"

    def __init__(self, plan, graph, surfaces, capacity, mesh=None, tile_rows=1, config=None):
        self.L, self.plan, self.mesh, self.graph, self.surfaces = load(), dict(plan), mesh, graph, list(surfaces)
        self.cfg, self.config4 = _layers_config(config)
        self.tile_rows = tile_rows
        self.arr, n = _surface_array(self.surfaces)
        self.h = None
        self._keep = []
        self.jpeg_status = []  # the status names of the last upload_jpegs call's files, also when it raised
        h = C.c_void_p()
        self._check(self.L.och_ortho_stream_create(graph.h, mesh.ctx.h if mesh is not None else None,
                                                   mesh.h if mesh is not None else None, self.arr, n, _plan_array(plan),
                                                   self.config4.ctypes.data, int(tile_rows), int(capacity), C.byref(h)))
        self.h = h
        self.image_hw = ortho_layers_cameras(graph, surfaces)["image_hw"]
        self.num_bands = int(self.L.och_ortho_stream_num_bands(self.h))

    def _context(self):
        return self.mesh.ctx if self.mesh is not None else None

    def _released(self):
        self._keep = []

    def band_cameras(self, band):
        n = self.L.och_ortho_stream_band_cameras(self.h, band, None)
        cams = np.zeros(n, np.uint32)
        self.L.och_ortho_stream_band_cameras(self.h, band, cams.ctypes.data)
        return cams

    def loads(self, band, phase=None):
        """band's planned loads as (camera, slot, phase), in issue order; phase: those of LOAD_AHEAD or LOAD_LATE alone"""
        n = self.L.och_ortho_stream_loads(self.h, band, None)
        l3 = np.zeros((n, 3), np.int32)
        self.L.och_ortho_stream_loads(self.h, band, l3.ctypes.data)
        return [tuple(int(v) for v in l) for l in l3 if phase is None or l[2] == phase]

    def upload(self, band, camera, image):
        """image: involved camera `camera`'s BGR image, a numpy array or a (page-locked) torch CPU tensor; it is kept alive
        until the band's render has returned"""
        shape = tuple(self.image_hw[camera]) + (3,) if 0 <= camera < len(self.image_hw) else None
        if isinstance(image, np.ndarray):
            ok = image.dtype == np.uint8 and image.shape == shape and image.flags.c_contiguous
            ptr = image.ctypes.data
        else:
            ok = str(image.dtype) == "torch.uint8" and tuple(image.shape) == shape and not image.is_cuda and image.is_contiguous()
            ptr = image.data_ptr()
        if shape is not None and not ok:
            raise ValueError(f"camera {camera}'s image is a contiguous uint8 host array of {shape}")
        self._check(self.L.och_ortho_stream_upload(self.h, band, camera, ptr))
        self._keep.append((band, image))

    def upload_jpegs(self, band, cameras, files):
        """`band`'s planned loads `cameras` from baseline JPEG files (bytes objects or paths, one per camera), decoded into
        their slots by the stream's own decoder with the EXIF orientation applied (och_ortho_stream_upload_jpegs; DESIGN.md
        §4.22): what upload(band, camera, decode_jpeg(file)) per camera gives.  Returns the files' status names.  A call
        the plan's order does not allow, or with a file whose headers are refused or whose size is not the camera's,
        raises OchipError and launches nothing; a file whose scan turns out corrupt raises it after the call's other
        loads are in their slots, and upload() may then bring that camera's pixels.  Returns when the pixels are there:
        nothing is kept alive."""
        cams = np.array([int(c) for c in cameras] + [0], np.uint32)
        datas = [None if f is None else _jpeg_bytes(f) for f in files]  # None: a NULL file, which the library refuses
        n = len(datas)
        if n != len(cams) - 1:
            raise ValueError(f"{len(cams) - 1} cameras and {n} files")
        bufs = [None if d is None else np.frombuffer(d, np.uint8) if len(d) else np.zeros(1, np.uint8) for d in datas]
        ptrs = np.array([0 if b is None else b.ctypes.data for b in bufs] + [0], np.uint64)
        sizes = np.array([len(d) if d is not None else 0 for d in datas] + [0], np.uint64)
        rec = np.zeros(n + 1, JPEG_INFO_DTYPE)
        rec["status"][:n] = -1
        rc = self.L.och_ortho_stream_upload_jpegs(self.h, band, n, cams.ctypes.data, ptrs.ctypes.data, sizes.ctypes.data,
                                                  rec.ctypes.data)
        self.jpeg_status = [JPEG_STATUS[s] if 0 <= s < 3 else None for s in rec["status"][:n].tolist()]
        self._check(rc)
        return self.jpeg_status

    def render(self, band, out=None, dsm=None, debug_knn=False):
        """band `band` as ortho_layers returns it (out, dsm, debug_knn as there)"""
        t, h = self.cfg["tile_size"], self.plan["height"]
        row0 = band * self.tile_rows * t
        rows = max(0, min(self.tile_rows * t, h - row0))

        def call(*outputs):
            return self.L.och_ortho_stream_render(self.h, band, *outputs)

        res = _layers_band(call, self.L.och_ortho_stream_last_error, self.cfg, self.plan["width"], row0, rows, self.mesh, out, dsm,
                           debug_knn)
        self._keep = [(b, im) for b, im in self._keep if b > band]
        return res

    def rewind(self):
        self._check(self.L.och_ortho_stream_rewind(self.h))

    def upload_end_ms(self, band):
        """when band's last upload finished on the device, ms since the sweep began (None: the band loaded nothing)"""
        ms = C.c_double(0)
        return float(ms.value) if self.L.och_ortho_stream_upload_end_ms(self.h, band, C.byref(ms)) == 0 else None


def lab_convert(values, mode):
    """L1, the colour conversion of the layered render: mode "bgr2lab8" / "lab82bgr" (N x 3 uint8 -> uint8) or
    "bgr2labf" (N x 3 uint8 -> float32)."""
    v = np.ascontiguousarray(values, np.uint8).reshape(-1, 3)
    m = {"bgr2lab8": 0, "lab82bgr": 1, "bgr2labf": 2}[mode]
    out = np.zeros(v.shape, np.float32 if m == 2 else np.uint8)
    load().och_lab_convert(m, v.ctypes.data, len(v), out.ctypes.data)
    return out


# ---- blended full-resolution orthomosaic (include/oc_host.h; src/ortho/ortho.cpp:1665-1990) ---------------------------
# OrthoMosaicConfig's defaults for the blend (include/opencalibration/ortho/ortho.hpp)
BLEND_CONFIG = dict(pyramid_levels=4, blend_transition_radius=64, tile_size=1024)


def _blend_config(config, num_layers):
    cfg = dict(BLEND_CONFIG, **(config or {}))
    unknown = set(cfg) - set(BLEND_CONFIG) - set(LAYERS_CONFIG)
    if unknown:
        raise ValueError(f"unknown blend settings {sorted(unknown)}")
    return cfg, np.array([num_layers, cfg["tile_size"], cfg["pyramid_levels"], cfg["blend_transition_radius"]], np.int32)


def _color_tables(color_balance):
    """ColorBalanceResult as the C tables: per_image {node id: dict(lab_offset (3), brdf, slope (2))}, per_model
    {model id: (3 vignetting coefficients)}."""
    cb = color_balance or {}
    per_image, per_model = cb.get("per_image", {}), cb.get("per_model", {})
    ids = np.array(sorted(per_image), np.uint64)
    six = np.array([[*per_image[int(i)]["lab_offset"], per_image[int(i)]["brdf"], *per_image[int(i)]["slope"]]
                    for i in ids], np.float64).reshape(-1, 6)
    mids = np.array(sorted(per_model), np.uint32)
    vig = np.array([per_model[int(m)] for m in mids], np.float64).reshape(-1, 3)
    return ids, six, mids, vig


def _device_ptr(t, dtype, shape, what, device):
    if tuple(t.shape) != tuple(shape) or str(t.dtype) != dtype or not t.is_cuda or not t.is_contiguous() or \
            t.device.index != device:
        raise ValueError(f"{what} must be a contiguous {dtype} tensor of {tuple(shape)} on device {device}")
    return t.data_ptr()


def ortho_blend(plan, graph, surfaces, layers, dsm, color_balance=None, ctx=None, config=None, out=None, debug=False):
    """blendLayeredGeoTIFF's pass (src/ortho/ortho.cpp:1665-1990) over one band of `layers` (ortho_layers' result:
    bgra (L, rows, width, 4), camera_id (L, rows, width), row0) with the DSM band `dsm` (rows x width float32).
    color_balance: dict(per_image={node id: dict(lab_offset, brdf, slope)}, per_model={model id: 3 coefficients}); None:
    no correction.  ctx (a capi.Context): on its device, where the layers, dsm and `out` may be CUDA tensors; None: the
    CPU route (numpy).  config overrides BLEND_CONFIG.  Returns rgba (rows, width, 4) uint8 (`out` when given), with
    debug (weight (L, rows, width) before the falloff, dist (rows, width), lab (L, rows, width, 3)) as (rgba, dict)."""
    L = load()
    bgra, ids = layers["bgra"], layers["camera_id"]
    nl, rows, w = int(bgra.shape[0]), int(bgra.shape[1]), int(bgra.shape[2])
    cfg, config4 = _blend_config(config, nl)
    row0 = int(layers.get("row0", 0))
    arr, n = _surface_array(surfaces)
    on_device = not isinstance(bgra, np.ndarray)
    if on_device:
        if ctx is None:
            raise ValueError("device layers need the device route (ctx)")
        import torch

        dev = ctx.device
        p_bgra = _device_ptr(bgra, "torch.uint8", (nl, rows, w, 4), "layers['bgra']", dev)
        p_ids = _device_ptr(ids, "torch.int64", (nl, rows, w), "layers['camera_id']", dev)
        p_dsm = _device_ptr(dsm, "torch.float32", (rows, w), "dsm", dev)
        if out is None:
            out = torch.empty((rows, w, 4), dtype=torch.uint8, device=f"cuda:{dev}")
        p_out = _device_ptr(out, "torch.uint8", (rows, w, 4), "out", dev)
        # the kernels run on the context's own stream: torch's queued work on these tensors finishes first
        torch.cuda.current_stream(out.device).synchronize()
    else:
        bgra = np.ascontiguousarray(bgra, np.uint8)
        ids = np.ascontiguousarray(ids).view(np.uint64) if np.asarray(ids).dtype.itemsize == 8 else None
        if ids is None or bgra.shape != (nl, rows, w, 4) or ids.shape != (nl, rows, w):
            raise ValueError("layers must hold bgra (L, rows, width, 4) and 64-bit camera_id (L, rows, width)")
        dsm = np.ascontiguousarray(dsm, np.float32)
        if dsm.shape != (rows, w):
            raise ValueError(f"dsm must be {rows} x {w}")
        out = np.zeros((rows, w, 4), np.uint8) if out is None else out
        if out.shape != (rows, w, 4) or out.dtype != np.uint8 or not out.flags.c_contiguous:
            raise ValueError(f"out must be a contiguous uint8 array of {rows} x {w} x 4")
        p_bgra, p_ids, p_dsm, p_out = bgra.ctypes.data, ids.ctypes.data, dsm.ctypes.data, out.ctypes.data
    cids, six, mids, vig = _color_tables(color_balance)
    dbg = dict(weight=np.zeros((nl, rows, w), np.float32), dist=np.zeros((rows, w), np.float32),
               lab=np.zeros((nl, rows, w, 3), np.float32)) if debug else None
    rc = L.och_ortho_blend_render(graph.h, ctx.h if ctx is not None else None, arr, n, _plan_array(plan), config4.ctypes.data,
                                  row0, rows, len(cids), cids.ctypes.data if len(cids) else None,
                                  six.ctypes.data if len(cids) else None, len(mids), mids.ctypes.data if len(mids) else None,
                                  vig.ctypes.data if len(mids) else None, int(on_device), p_bgra, p_ids, p_dsm, p_out,
                                  *(None if dbg is None else dbg[k].ctypes.data for k in ("weight", "dist", "lab")))
    if rc != 0:
        raise capi.OchipError(L.och_ortho_blend_last_error().decode())
    return (out, dbg) if debug else out


def laplacian_blend(lab_layers, weights, pyramid_levels=4, ctx=None):
    """laplacianBlend (src/ortho/blending.cpp) of float Lab layers (L, rows, cols, 3) with weights (L, rows, cols): BGRA
    (rows, cols, 4) uint8, alpha 255.  ctx: on its device (ochip_laplacian_blend); None: the CPU route."""
    lab = np.ascontiguousarray(lab_layers, np.float32)
    wt = np.ascontiguousarray(weights, np.float32)
    if lab.ndim != 4 or lab.shape[3] != 3 or wt.shape != lab.shape[:3]:
        raise ValueError("lab_layers (L, rows, cols, 3) and weights (L, rows, cols)")
    nl, rows, cols = wt.shape
    out = np.zeros((rows, cols, 4), np.uint8)
    if nl == 0:
        return np.zeros((0, 0, 4), np.uint8)  # laplacianBlend of no layers: an empty Mat
    if ctx is not None:
        ctx._check(capi.load().ochip_laplacian_blend(ctx.h, nl, rows, cols, int(pyramid_levels), lab.ctypes.data,
                                                     wt.ctypes.data, out.ctypes.data), "ochip_laplacian_blend")
    elif load().och_laplacian_blend(nl, rows, cols, int(pyramid_levels), lab.ctypes.data, wt.ctypes.data, out.ctypes.data):
        raise ValueError("laplacian_blend: 1..8 layers of at most 4096 x 4096")
    return out


def _corr_array(correspondences):
    c = np.ascontiguousarray(correspondences)
    if c.dtype != CORR_DTYPE or c.ndim != 1:
        raise ValueError("correspondences are a 1-D array of CORR_DTYPE")
    return c


def color_balance_solve(correspondences, graph=None, positions=None, ctx=None):
    """solveColorBalance (src/ortho/color_balance.cpp) of ortho_layers' correspondences (CORR_DTYPE; the bands'
    concatenated): the per-image and per-model radiometric parameters the blend applies.  ctx (a capi.Context): the
    solve runs on its device; None: the CPU route (small surveys: at most 4096 unknowns, 6 per camera + 3 per model).
    The gauge plane is removed over the cameras with a position: `positions` ({node id: (x, y)} or rows (id, x, y))
    first, else the graph's nodes.  Returns dict(per_image={id: dict(lab_offset, brdf, slope)}, per_model={id: 3
    coefficients}, success, final_cost, num_iterations, termination), which ortho_blend takes as color_balance=."""
    L = load()
    corr = _corr_array(correspondences)
    if positions is None:
        pos = []
    elif isinstance(positions, dict):
        pos = [(int(k), float(v[0]), float(v[1])) for k, v in positions.items()]
    else:
        pos = [(int(r[0]), float(r[1]), float(r[2])) for r in positions]
    pid = np.array([r[0] for r in pos], np.uint64)
    pxy = np.array([r[1:] for r in pos], np.float64).reshape(-1, 2)
    ncap = len(np.unique(np.concatenate([corr["camera_id_a"], corr["camera_id_b"]])))
    mcap = len(np.unique(np.concatenate([corr["model_id_a"], corr["model_id_b"]])))
    cids, six = np.zeros(max(ncap, 1), np.uint64), np.zeros((max(ncap, 1), 6))
    mids, vig = np.zeros(max(mcap, 1), np.uint32), np.zeros((max(mcap, 1), 3))
    nc, nm, summary = C.c_size_t(0), C.c_size_t(0), np.zeros(4)
    rc = L.och_color_balance_solve(graph.h if graph is not None else None, ctx.h if ctx is not None else None,
                                   corr.ctypes.data if len(corr) else None, len(corr), len(pid),
                                   pid.ctypes.data if len(pid) else None, pxy.ctypes.data if len(pid) else None,
                                   ncap, cids.ctypes.data, six.ctypes.data, C.byref(nc), mcap, mids.ctypes.data,
                                   vig.ctypes.data, C.byref(nm), summary.ctypes.data)
    if rc != 0:
        raise capi.OchipError(L.och_color_balance_last_error().decode())
    per_image = {int(cids[i]): dict(lab_offset=tuple(float(v) for v in six[i, :3]), brdf=float(six[i, 3]),
                                    slope=tuple(float(v) for v in six[i, 4:])) for i in range(nc.value)}
    per_model = {int(mids[i]): tuple(float(v) for v in vig[i]) for i in range(nm.value)}
    return dict(per_image=per_image, per_model=per_model, success=bool(summary[0]), final_cost=float(summary[1]),
                num_iterations=int(summary[2]), termination=int(summary[3]))


def color_balance_evaluate(correspondences, cam_ids, color6, model_ids, vig3, ctx=None, jacobian=True, plan=False):
    """Test seam: cost, J'J, J'r of the colour-balance problem at the given parameters (cam_ids, model_ids sorted and
    unique; color6 (n, 6), vig3 (m, 3)), on ctx's device or by the CPU route; plan=True (no ctx): the device's own
    evaluation run on the host (its plan, its arithmetic, its order: bit-equal to the device's), with layout = dict(
    tail_begin, regions, separators, chunks).  Returns dict(cost, failed, JtJ, Jtr, cam_col, model_col): the first
    unknown of every camera / model in the route's own order."""
    L = load()
    corr = _corr_array(correspondences)
    cam_ids, model_ids = np.ascontiguousarray(cam_ids, np.uint64), np.ascontiguousarray(model_ids, np.uint32)
    color6 = np.ascontiguousarray(color6, np.float64).reshape(len(cam_ids), 6)
    vig3 = np.ascontiguousarray(vig3, np.float64).reshape(len(model_ids), 3)
    n = 6 * len(cam_ids) + 3 * len(model_ids)
    JtJ, Jtr = (np.zeros((n, n)), np.zeros(n)) if jacobian else (None, None)
    cam_col, model_col = np.zeros(len(cam_ids), np.int32), np.zeros(len(model_ids), np.int32)
    cost = np.zeros(1)
    args = (corr.ctypes.data, len(corr), len(cam_ids), cam_ids.ctypes.data, color6.ctypes.data, len(model_ids),
            model_ids.ctypes.data, vig3.ctypes.data, cost.ctypes.data, None if JtJ is None else JtJ.ctypes.data,
            None if Jtr is None else Jtr.ctypes.data, cam_col.ctypes.data, model_col.ctypes.data)
    layout = np.zeros(4, np.int32)
    if plan:
        if ctx is not None:
            raise ValueError("plan=True is the host's run of the device evaluation: no ctx")
        rc = L.och_color_balance_evaluate_plan(*args, layout.ctypes.data)
    else:
        rc = L.och_color_balance_evaluate(ctx.h if ctx is not None else None, *args)
    if rc < 0:
        raise capi.OchipError(L.och_color_balance_last_error().decode())
    res = dict(cost=float(cost[0]), failed=rc == 1, JtJ=JtJ, Jtr=Jtr, cam_col=cam_col, model_col=model_col)
    if plan:
        res["layout"] = dict(zip(("tail_begin", "regions", "separators", "chunks"), map(int, layout)))
    return res


def color_balance_remove_gauge(xy, offsets):
    """The gauge step of color_balance_solve alone: offsets (n, 3) minus their least-squares plane over xy (n, 2);
    returns (offsets, rank)."""
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    off = np.array(offsets, np.float64).reshape(len(xy), 3)
    rank = load().och_color_balance_remove_gauge(len(xy), xy.ctypes.data, off.ctypes.data)
    return off, rank


def ortho_mosaic(plan, graph, surfaces, images, mesh=None, config=None, color_balance=None, tile_rows=1, out=None,
                 overviews=False, progress=None, progress_passes=(1, 2), jpeg=None, jpeg_quality=95, geotiff=None,
                 dsm_geotiff=None, geo=None, progress_png=False, layers_geotiff=None, cameras_geotiff=None):
    """The blended full-resolution orthomosaic of `plan` (dsm_plan), band by band of tile_rows output tile rows: DSM ->
    layers (ortho_layers) -> blend (ortho_blend).  mesh (an OrthoMesh): every step on its device, images as CUDA tensors,
    into `out` (a (height, width, 4) uint8 CUDA tensor, made when None); None: the CPU route, numpy images, into a host
    array.  config: LAYERS_CONFIG's and BLEND_CONFIG's keys.
    color_balance: None (no correction), a dict (ortho_blend's), or "solve": the reference's GENERATE_LAYERS ->
    COLOR_BALANCE -> BLEND_LAYERS - a first pass over the bands renders the layers for their correspondences alone,
    color_balance_solve (on the mesh's device, or the CPU route) turns them into the tables, and the second pass
    RE-RENDERS every band's layers and blends them with the result: a band's layers are never kept beyond its blend, so
    the memory held stays one band's whatever the raster's size, at the price of the layer pass run twice.
    overviews=True: (out, dict(rgba=[level 1, ...], dsm=[level 1, ...])), the averaged overview levels (OrthoOverviews) of
    the mosaic and of the DSM, each band fed right after its blend - with "solve" in the second sweep alone.
    progress: a callable that takes one tile update (TileProgress.collect's dict) per tile and pass of progress_passes (1:
    the layers, 2: the blend), the reference's TileProgressCallback; within a pass the calls come in tile_index order.
    With "solve" the first sweep emits pass 1 and the second pass 2, otherwise the single sweep emits a band's pass-1 tiles
    and then its pass-2 tiles.  Band k's updates are collected after band k + 1 has been enqueued, so the device never
    waits for the callback; the rest are flushed before the function returns.  An exception from the callback propagates
    after the stream and the builders are closed.  None: nothing is allocated or launched for it.  progress_png: every
    update also carries png_base64, the reference's TileUpdate text (TileProgress.collect(png=True)), a band's tiles encoded
    as one batch on the mosaic's route; False: nothing is allocated or launched for it.
    jpeg: a path or a binary file object that receives the mosaic as a JPEG of quality jpeg_quality (JpegEncoder, the
    textured OBJ's texture): each band is fed right after its blend - with "solve" in the second sweep alone - and the bytes
    are written as they complete; the file is closed (a path) or flushed (an object) before the function returns and on an
    exception.  None: nothing is allocated or launched for it.
    geotiff, dsm_geotiff: a path or a seekable binary file object each, the mosaic and the DSM as tiled DEFLATE GeoTIFFs
    (GeoTiffWriter; the reference's orthomosaic.tif and dsm.tif): each band's RGBA and DSM are fed right behind its blend -
    with "solve" in the second sweep alone - the overview levels are built for either (as overviews=True does) and become
    the files' further IFDs, and the files are finished before the function returns and closed on an exception.  geo:
    dict(min_x, max_y, gsd[, epsg]) for the georeferencing tags; its missing keys are the plan's.  Both None: nothing is
    allocated or launched for them.
    layers_geotiff, cameras_geotiff: both or neither; a path or a seekable binary file object each, the two rasters
    generateLayeredGeoTIFF leaves (GeoTiffWriter's kinds GEOTIFF_LAYERS8 and GEOTIFF_CAMERAS32), written
    in the sweep that renders the layers, each band's fed right behind its render.  With "solve" that is the first sweep,
    and the second then blends from the files (read_layer_files' bands) instead of rendering again; the mosaic is the same,
    bit for bit.  For that a file object must also be readable and at position 0 (opened "w+b", an io.BytesIO); one that is
    not is refused with OchipError before anything is rendered.  With both None nothing is allocated, launched or changed."""
    return _mosaic(plan, graph, surfaces, mesh, config, color_balance, tile_rows, out, images=images, overviews=overviews,
                   progress=progress, progress_passes=progress_passes, jpeg=jpeg, jpeg_quality=jpeg_quality,
                   geotiff=geotiff, dsm_geotiff=dsm_geotiff, geo=geo, progress_png=progress_png, layers_geotiff=layers_geotiff,
                   cameras_geotiff=cameras_geotiff)


def ortho_mosaic_streamed(plan, graph, surfaces, fetch, mesh, capacity, config=None, color_balance=None, tile_rows=1, out=None,
                          overviews=False, progress=None, progress_passes=(1, 2), jpeg=None, jpeg_quality=95, geotiff=None,
                          dsm_geotiff=None, geo=None, progress_png=False, files=None, layers_geotiff=None, cameras_geotiff=None):
    """ortho_mosaic on mesh's device without the source images resident: fetch(i) returns involved camera i's BGR image
    (ortho_layers_cameras' order) as a numpy array or a page-locked torch CPU tensor, and at most `capacity` images are on
    the device at a time (OrthoStream).  Band k + 1's ahead uploads are issued before band k renders, so that they run
    beside it when the images are page-locked.  color_balance as ortho_mosaic's; "solve" renders the layers twice, the
    second sweep starting from the images the first one left on the device.  Returns the (height, width, 4) RGBA tensor,
    with overviews=True (tensor, dict(rgba=[...], dsm=[...])) as ortho_mosaic does.  progress, progress_passes, jpeg,
    jpeg_quality, geotiff, dsm_geotiff, geo, progress_png: as ortho_mosaic's.
    files: files[i] is involved camera i's baseline JPEG file (bytes or a path; ortho_image_paths gives a checkpoint's), None
    where it has none.  A band's loads that have a file whose headers jpeg_info calls "ok" are decoded into their slots
    (OrthoStream.upload_jpegs: one call for the band's late loads - all of band 0's - and one for the next band's ahead
    loads), so only the files cross to the device; the others - no file, an unsupported or corrupt one, a scan that turns
    out corrupt - come through fetch(i) as before, or raise OchipError naming the camera, the file and its status when fetch
    is None, which files allows.  files None: nothing changes.
    layers_geotiff, cameras_geotiff: as ortho_mosaic's; with "solve" the second sweep reads the layers back from the two files
    and so uploads and decodes nothing."""
    return _mosaic(plan, graph, surfaces, mesh, config, color_balance, tile_rows, out, fetch=fetch, capacity=capacity, files=files,
                   overviews=overviews, progress=progress, progress_passes=progress_passes, jpeg=jpeg, jpeg_quality=jpeg_quality,
                   geotiff=geotiff, dsm_geotiff=dsm_geotiff, geo=geo, progress_png=progress_png, layers_geotiff=layers_geotiff,
                   cameras_geotiff=cameras_geotiff)


def _mosaic(plan, graph, surfaces, mesh, config, color_balance, tile_rows, out, images=None, fetch=None, capacity=None,
            overviews=False, progress=None, progress_passes=(1, 2), jpeg=None, jpeg_quality=95, geotiff=None, dsm_geotiff=None,
            geo=None, progress_png=False, files=None, layers_geotiff=None, cameras_geotiff=None):
    """The band loop of ortho_mosaic (images) and ortho_mosaic_streamed (fetch and / or files, capacity): the two differ in
    where a band's layers come from, ortho_layers over the resident images or an OrthoStream's render behind the band's
    uploads."""
    cfg = {**LAYERS_CONFIG, **BLEND_CONFIG, **(config or {})}
    lcfg = {k: cfg[k] for k in LAYERS_CONFIG}
    bcfg = {k: cfg[k] for k in BLEND_CONFIG}
    if isinstance(color_balance, str) and color_balance != "solve":
        raise ValueError('color_balance is None, a dict of tables or "solve"')
    if (layers_geotiff is None) != (cameras_geotiff is None):
        raise capi.OchipError("layers_geotiff and cameras_geotiff belong together: both, or neither")
    if color_balance == "solve" and layers_geotiff is not None:  # the second sweep reads what the first wrote: known before it renders
        for name, target in (("layers_geotiff", layers_geotiff), ("cameras_geotiff", cameras_geotiff)):
            if not isinstance(target, (str, bytes, os.PathLike)) and not (
                    hasattr(target, "read") and hasattr(target, "readable") and target.readable() and
                    hasattr(target, "seekable") and target.seekable() and target.tell() == 0):
                raise capi.OchipError(f'{name}: with "solve" the second sweep reads the file back, so a file object must be '
                                      "readable as well as writable and seekable, and at position 0")
    h, w, nl, band_rows = plan["height"], plan["width"], cfg["num_layers"], tile_rows * cfg["tile_size"]
    if mesh is None:
        ctx = None
        out = np.zeros((h, w, 4), np.uint8) if out is None else out
    else:
        import torch

        ctx, dev = mesh.ctx, f"cuda:{mesh.ctx.device}"
        out = torch.empty((h, w, 4), dtype=torch.uint8, device=dev) if out is None else out
    stream = OrthoStream(plan, graph, surfaces, capacity, mesh=mesh, tile_rows=tile_rows, config=lcfg) \
        if fetch is not None or files is not None else None
    builders = [OrthoOverviews(kind, w, h, ctx=ctx, on_device=mesh is not None)
                for kind in (OVERVIEW_RGBA8, OVERVIEW_FLOAT32)] if overviews or geotiff is not None or dsm_geotiff is not None else []
    tiffs = [None, None]  # the orthomosaic's and the DSM's GeoTiffWriter
    pair = [None, None]   # the layers' and the cameras' GeoTiffWriter while a sweep renders, their GeoTiffReaders behind it
    passes = {int(p) for p in progress_passes} if progress is not None else set()
    if passes - {TILE_PASS_LAYERS, TILE_PASS_BLEND}:
        raise ValueError("progress_passes names 1 (the layers) and 2 (the blend)")
    tiles = TileProgress(plan, cfg["tile_size"], nl, ctx=ctx) if passes else None
    texture = None

    def deliver(keep):
        """the fed bands' updates to the callback, oldest first, until `keep` bands are pending"""
        while tiles.pending() > keep:
            for update in tiles.collect(png=bool(progress_png)):
                progress(update)

    def fill(k, loads):
        """band k's loads `loads`: one upload_jpegs call for those with a usable file, fetch and upload for the rest"""
        def pixels(cam, status):
            if fetch is None:
                raise capi.OchipError(f"ortho_mosaic_streamed: involved camera {cam} has "
                                      f"{'no file' if status is None else f'the file {_file_name(files[cam])}, which is {status}'}"
                                      ", and there is no fetch to ask for its pixels")
            stream.upload(k, cam, fetch(cam))

        decode = []
        for cam, _, _ in loads:
            data = _jpeg_bytes(files[cam]) if files is not None and files[cam] is not None else None
            status = jpeg_info(data)["status"] if data is not None else None
            if status == "ok":
                decode.append((cam, data))
            else:
                pixels(cam, status)
        if decode:
            try:
                stream.upload_jpegs(k, [cam for cam, _ in decode], [data for _, data in decode])
            except capi.OchipError:
                bad = [(cam, st) for (cam, _), st in zip(decode, stream.jpeg_status) if st == "corrupt"]
                if not bad or fetch is None:  # a refusal of the whole call, or nobody to ask for a corrupt scan's pixels
                    raise
                for cam, st in bad:  # the scans that turned out corrupt: the call's other loads are in their slots
                    pixels(cam, st)

    def band(k, balance, blend, emit=frozenset(), from_files=False):
        row0 = k * band_rows
        rows = min(band_rows, h - row0)
        if stream is not None and not from_files:  # before the band's DSM and render: its own loads still missing, then the next band's ahead ones
            fill(k, stream.loads(0) if k == 0 else stream.loads(k, LOAD_LATE))
            if k + 1 < stream.num_bands:
                fill(k + 1, stream.loads(k + 1, LOAD_AHEAD))
        if mesh is None:
            dsm, lay = dsm_render(plan, surfaces, row0=row0, rows=rows), None
        else:
            dsm = torch.empty((rows, w), dtype=torch.float32, device=dev)
            dsm_render(plan, surfaces, mesh=mesh, row0=row0, rows=rows, out=dsm)
            lay = None if from_files else dict(bgra=torch.empty((nl, rows, w, 4), dtype=torch.uint8, device=dev),
                                               camera_id=torch.empty((nl, rows, w), dtype=torch.int64, device=dev))
            if TILE_PASS_LAYERS in emit:  # the pick among the layers reads their weights
                lay["weight"] = torch.empty((nl, rows, w), dtype=torch.float32, device=dev)
        if from_files:  # the first sweep left the layers in the two files: nothing is uploaded, decoded or rendered
            layers = dict(_read_layer_band(pair[0], pair[1], nl, row0, rows, mesh is not None), correspondences=None)
        elif stream is not None:
            layers = stream.render(k, out=lay)
        else:
            layers = ortho_layers(plan, graph, surfaces, images, mesh=mesh, row0=row0, tile_rows=tile_rows, config=lcfg, out=lay,
                                  dsm=dsm if mesh is None else None)
        if not from_files and pair[0] is not None:  # behind the render on the context's stream: no wait of its own
            pair[0].feed(row0, layers["bgra"])
            pair[1].feed(row0, layers["camera_id"])
        before = tiles.pending() if emit else 0
        if TILE_PASS_LAYERS in emit:  # behind the render on the context's stream: no wait of its own
            tiles.feed(TILE_PASS_LAYERS, row0, layers["bgra"], layers["weight"])
        if blend:
            ortho_blend(plan, graph, surfaces, layers, dsm, balance, ctx=ctx, config=bcfg, out=out[row0:row0 + rows])
            if TILE_PASS_BLEND in emit:
                tiles.feed(TILE_PASS_BLEND, row0, out[row0:row0 + rows])
            if builders:  # behind the blend on the context's stream: no wait of its own
                builders[0].feed(row0, out[row0:row0 + rows])
                builders[1].feed(row0, dsm)
            if texture is not None:  # behind the blend on the context's stream as well
                texture.feed(row0, out[row0:row0 + rows])
            if tiffs[0] is not None:
                tiffs[0].feed(row0, out[row0:row0 + rows])
            if tiffs[1] is not None:
                tiffs[1].feed(row0, dsm)
        if emit:  # this band is enqueued behind the bands before it: their updates are due
            deliver(tiles.pending() - before)
        return layers["correspondences"]

    try:
        if jpeg is not None:
            texture = _JpegSink(jpeg, w, h, ctx, jpeg_quality, mesh is not None)
        for i, (target, kind) in enumerate(((geotiff, OVERVIEW_RGBA8), (dsm_geotiff, OVERVIEW_FLOAT32))):
            if target is not None:
                tiffs[i] = GeoTiffWriter(target, kind, w, h, geo={**{k: plan[k] for k in ("min_x", "max_y", "gsd")}, **(geo or {})},
                                         ctx=ctx, on_device=mesh is not None)
        if layers_geotiff is not None:
            for i, (target, kind) in enumerate(((layers_geotiff, GEOTIFF_LAYERS8), (cameras_geotiff, GEOTIFF_CAMERAS32))):
                pair[i] = GeoTiffWriter(target, kind, w, h, geo={**{k: plan[k] for k in ("min_x", "max_y", "gsd")}, **(geo or {})},
                                        ctx=ctx, on_device=mesh is not None, num_layers=nl)
        bands = range(-(-h // band_rows))
        from_files = False
        if color_balance == "solve":
            corr = [band(k, None, False, passes & {TILE_PASS_LAYERS}) for k in bands]
            if tiles is not None:
                deliver(0)
            if pair[0] is not None:  # the files are complete: the second sweep reads them
                for t in pair:
                    t.finish()
                rl, rc, _ = _open_layer_files(layers_geotiff, cameras_geotiff, ctx)
                pair[0], pair[1], from_files = rl, rc, True
            color_balance = color_balance_solve(np.concatenate(corr) if corr else np.zeros(0, CORR_DTYPE), graph=graph, ctx=ctx)
            if stream is not None and not from_files:
                stream.rewind()
            passes = passes & {TILE_PASS_BLEND}
        for k in bands:
            band(k, color_balance, True, passes, from_files)
        if tiles is not None:
            deliver(0)
        if pair[0] is not None and not from_files:
            for t in pair:
                t.finish()
        if texture is not None:
            texture.finish()
        if builders:
            levels = dict(rgba=builders[0].finish(), dsm=builders[1].finish())
            if tiffs[0] is not None:
                tiffs[0].finish(levels["rgba"])
            if tiffs[1] is not None:
                tiffs[1].finish(levels["dsm"])
            if overviews:
                return out, levels
    finally:
        if texture is not None:
            texture.close()
        for t in tiffs + pair:
            if t is not None:
                t.close()
        if stream is not None:
            stream.close()
        for b in builders:
            b.close()
        if tiles is not None:
            tiles.close()
    return out


def ortho_layers_files(plan, graph, surfaces, images, layers_geotiff, cameras_geotiff, dsm_geotiff=None, mesh=None, config=None,
                       tile_rows=1, geo=None):
    """generateLayeredGeoTIFF (src/ortho/ortho.cpp:1431-1660): the layer pass alone, band by band, into the layers and the
    cameras raster (GeoTiffWriter's kinds GEOTIFF_LAYERS8 and GEOTIFF_CAMERAS32) and, with dsm_geotiff, the
    DSM's file with its overview levels, as ortho_mosaic writes it.  Each band's layers and ids are fed right behind its
    render, and a feed never waits for the band it enqueues.  images, mesh, config, tile_rows, geo: as ortho_mosaic's.
    Returns the correspondences of all bands, which color_balance_solve takes; ortho_blend_files is the other half."""
    cfg = {**LAYERS_CONFIG, **(config or {})}
    lcfg = {k: cfg[k] for k in LAYERS_CONFIG}
    h, w, nl, band_rows = plan["height"], plan["width"], cfg["num_layers"], tile_rows * cfg["tile_size"]
    ctx = None if mesh is None else mesh.ctx
    tags = {**{k: plan[k] for k in ("min_x", "max_y", "gsd")}, **(geo or {})}
    writers, builder, corr = [], None, []
    try:
        for target, kind in ((layers_geotiff, GEOTIFF_LAYERS8), (cameras_geotiff, GEOTIFF_CAMERAS32)):
            writers.append(GeoTiffWriter(target, kind, w, h, geo=tags, ctx=ctx, on_device=mesh is not None, num_layers=nl))
        if dsm_geotiff is not None:
            builder = OrthoOverviews(OVERVIEW_FLOAT32, w, h, ctx=ctx, on_device=mesh is not None)
            writers.append(GeoTiffWriter(dsm_geotiff, OVERVIEW_FLOAT32, w, h, geo=tags, ctx=ctx, on_device=mesh is not None))
        for row0 in range(0, h, band_rows):
            rows = min(band_rows, h - row0)
            dsm = lay = None
            if mesh is None:
                dsm = dsm_render(plan, surfaces, row0=row0, rows=rows)
            else:  # the band stays on the device: the feeds read it there
                import torch

                dev = f"cuda:{ctx.device}"
                lay = dict(bgra=torch.empty((nl, rows, w, 4), dtype=torch.uint8, device=dev),
                           camera_id=torch.empty((nl, rows, w), dtype=torch.int64, device=dev))
                if dsm_geotiff is not None:
                    dsm = torch.empty((rows, w), dtype=torch.float32, device=dev)
                    dsm_render(plan, surfaces, mesh=mesh, row0=row0, rows=rows, out=dsm)
            layers = ortho_layers(plan, graph, surfaces, images, mesh=mesh, row0=row0, tile_rows=tile_rows, config=lcfg, out=lay,
                                  dsm=dsm if mesh is None else None)
            writers[0].feed(row0, layers["bgra"])
            writers[1].feed(row0, layers["camera_id"])
            if dsm_geotiff is not None:
                builder.feed(row0, dsm)
                writers[2].feed(row0, dsm)
            corr.append(layers["correspondences"])
        writers[0].finish()
        writers[1].finish()
        if dsm_geotiff is not None:
            writers[2].finish(builder.finish())
    finally:
        for t in writers:
            t.close()
        if builder is not None:
            builder.close()
    return np.concatenate(corr) if corr else np.zeros(0, CORR_DTYPE)


def ortho_blend_files(plan, graph, surfaces, layers_geotiff, cameras_geotiff, dsm_geotiff, color_balance=None, ctx=None, config=None,
                      tile_rows=1, out=None, geotiff=None, geo=None):
    """blendLayeredGeoTIFF (src/ortho/ortho.cpp:1665-1990): the blend alone, from the three files ortho_layers_files leaves -
    what GeoTiffReader takes each - read band by band (read_layer_files' bands and the DSM's rows) and blended by
    ortho_blend.  color_balance: None or a dict of tables (color_balance_solve's).  ctx None: the CPU route, else through
    ctx's device, where the bands and the mosaic stay.  geotiff: the mosaic's file with its overview levels, as ortho_mosaic
    writes it.  Files whose size or geo tags are not the plan's raise GeoTiffError("refused").  Returns rgba
    (height, width, 4) uint8 (`out` when given)."""
    cfg = {**LAYERS_CONFIG, **BLEND_CONFIG, **(config or {})}
    bcfg = {k: cfg[k] for k in BLEND_CONFIG}
    h, w, band_rows = plan["height"], plan["width"], tile_rows * cfg["tile_size"]
    on_device = ctx is not None
    rl, rc, nl = _open_layer_files(layers_geotiff, cameras_geotiff, ctx)
    rd = writer = builder = None
    try:
        rd = GeoTiffReader(dsm_geotiff, ctx=ctx)
        for name, r in (("layers", rl), ("cameras", rc), ("DSM", rd)):
            if (r.width, r.height) != (w, h):
                raise GeoTiffError("refused", f"the {name} file is {r.width} x {r.height}, the plan {w} x {h}")
            g = r.geo
            if g is None or (g["min_x"], g["max_y"], g["gsd_x"], g["gsd_y"]) != (plan["min_x"], plan["max_y"], plan["gsd"], plan["gsd"]):
                raise GeoTiffError("refused", f"the geo tags of the {name} file, {g}, are not the plan's")
        if rd.kind != OVERVIEW_FLOAT32:
            raise GeoTiffError("refused", "the DSM file holds no float32 raster")
        if on_device:
            import torch

            out = torch.empty((h, w, 4), dtype=torch.uint8, device=f"cuda:{ctx.device}") if out is None else out
        else:
            out = np.zeros((h, w, 4), np.uint8) if out is None else out
        if geotiff is not None:
            builder = OrthoOverviews(OVERVIEW_RGBA8, w, h, ctx=ctx, on_device=on_device)
            writer = GeoTiffWriter(geotiff, OVERVIEW_RGBA8, w, h, geo={**{k: plan[k] for k in ("min_x", "max_y", "gsd")}, **(geo or {})},
                                   ctx=ctx, on_device=on_device)
        for row0 in range(0, h, band_rows):
            rows = min(band_rows, h - row0)
            layers = _read_layer_band(rl, rc, nl, row0, rows, on_device)
            dsm = rd.read(row0, rows, on_device=on_device)
            ortho_blend(plan, graph, surfaces, layers, dsm, color_balance, ctx=ctx, config=bcfg, out=out[row0:row0 + rows])
            if writer is not None:
                builder.feed(row0, out[row0:row0 + rows])
                writer.feed(row0, out[row0:row0 + rows])
        if writer is not None:
            writer.finish(builder.finish())
    finally:
        for t in (rl, rc, rd, writer, builder):
            if t is not None:
                t.close()
    return out


# ---- per-tile progress of the layer and blend passes (include/oc_host.h) -----------------------------------
TILE_PASS_LAYERS, TILE_PASS_BLEND = 1, 2
# och_tile_update: 72 bytes, no padding
TILE_UPDATE_DTYPE = np.dtype([(k, np.int32) for k in (
    "pixel_x", "pixel_y", "pixel_w", "pixel_h", "total_output_width", "total_output_height", "tile_index", "total_tiles",
    "thumb_w", "thumb_h", "scale", "pass")] + [(k, np.float64) for k in ("bounds_min_x", "bounds_max_y", "meters_per_pixel")])


def tile_thumb_dims(tw, th):
    """(scale, thumb_w, thumb_h) of the progress thumbnail of a tw x th tile (each 1..4096): every scale-th pixel, scale =
    max(1, (max(tw, th) + 127) // 128)."""
    dims = np.zeros(3, np.int32)
    if capi.load().ochip_ortho_tile_thumb_dims(int(tw), int(th), dims.ctypes.data) != 0:
        raise ValueError(f"a tile of {tw} x {th}")
    return tuple(int(v) for v in dims)


def _tile_band(pass_, pixels, weight, device):
    """(num_layers, rows, width, on_device, pixels' pointer, weights' pointer, what to keep alive) of a band fed to the tile
    thumbnails: pass 1 bgra (L, rows, width, 4) uint8 with weight (L, rows, width) float32, pass 2 rgba (rows, width, 4)"""
    on_device = not isinstance(pixels, np.ndarray)
    lead = 1 if pass_ == TILE_PASS_LAYERS else 0
    if len(pixels.shape) != 3 + lead or pixels.shape[-1] != 4:
        raise ValueError("a band is bgra (L, rows, width, 4) for pass 1, rgba (rows, width, 4) otherwise")
    shape = tuple(int(v) for v in pixels.shape)
    nl, rows, w = (shape[0] if lead else 1), shape[lead], shape[lead + 1]
    if weight is not None and (isinstance(weight, np.ndarray) == on_device):
        raise ValueError("pixels and weight are both numpy arrays or both CUDA tensors")
    if on_device:
        if device is None:
            raise ValueError("a device band needs the device route (ctx)")
        p = _device_ptr(pixels, "torch.uint8", shape, "pixels", device)
        pw = None if weight is None else _device_ptr(weight, "torch.float32", shape[:-1], "weight", device)
    else:
        if pixels.dtype != np.uint8:
            raise ValueError("the pixels are uint8")
        pixels = np.ascontiguousarray(pixels)
        if weight is not None:
            weight = np.ascontiguousarray(weight, np.float32)
            if weight.shape != shape[:-1]:
                raise ValueError(f"weight must be {shape[:-1]}")
        p, pw = pixels.ctypes.data, None if weight is None else weight.ctypes.data
    return nl, rows, w, on_device, p, pw, (pixels, weight)


def ortho_tile_thumbs(pixels, pass_, tile_size=None, weight=None, ctx=None):
    """The raw thumbnail slots of one band (ochip_ortho_tile_thumbs): (tiles, min(T, 128)^2, 4) uint8 BGRA in tile order, the
    thumbnail densely at each slot's start and zeros behind it.  pixels / weight: numpy arrays (ctx None: the CPU route,
    else through ctx's device) or CUDA tensors on ctx's device."""
    t = int(BLEND_CONFIG["tile_size"] if tile_size is None else tile_size)
    nl, rows, w, on_device, p, pw, _keep = _tile_band(pass_, pixels, weight, None if ctx is None else ctx.device)
    if on_device:
        import torch

        torch.cuda.current_stream(pixels.device).synchronize()  # the kernel runs on the context's own stream
    side = min(max(t, 1), 128)
    out = np.zeros((max(-(-w // max(t, 1)) * -(-rows // max(t, 1)), 0), side * side, 4), np.uint8)
    L = capi.load()
    if L.ochip_ortho_tile_thumbs(ctx.h if ctx is not None else None, int(pass_), w, rows, t, nl, int(on_device), p, pw,
                                 out.ctypes.data) != 0:
        raise capi.OchipError(L.ochip_last_error(ctx.h if ctx is not None else None).decode())
    return out


class TileProgress(_Handle):
    """The per-tile updates of a raster's layer and blend passes, band by band (och_tile_progress_*).
    plan: the raster (dsm_plan); ctx None: the CPU route, numpy bands; ctx: numpy bands through its device, or CUDA tensors,
    fed on the context's stream without a host wait - the caller has torch's work on a band finished before feed, as
    ortho_blend does.  feed(pass_, row0, pixels, weight): pass 1 takes bgra (L, rows, width, 4) and weight (L, rows,
    width), pass 2 rgba (rows, width, 4); row0 lies on a tile row and a pass's bands arrive in raster order without gaps.
    collect(): waits for the oldest fed band alone and returns its tiles in tile order as dicts of TILE_UPDATE_DTYPE's
    fields plus thumbnail, a (thumb_h, thumb_w, 4) uint8 BGRA array; raw=True: (records, slots) as the library wrote them."""

    _destroy, _last_error = "och_tile_progress_destroy", "och_tile_progress_last_error"

    def __init__(self, plan, tile_size=None, num_layers=None, ctx=None):
        self.L, self.ctx, self.plan = load(), ctx, dict(plan)
        self.tile_size = int(BLEND_CONFIG["tile_size"] if tile_size is None else tile_size)
        self.num_layers = int(LAYERS_CONFIG["num_layers"] if num_layers is None else num_layers)
        self.h = None
        self._keep = []
        self._png = None  # the PngEncoder of collect(png=True), made by the first such call
        h = C.c_void_p()
        self._check(self.L.och_tile_progress_create(ctx.h if ctx is not None else None, _plan_array(plan), self.tile_size,
                                                    self.num_layers, C.byref(h)))
        self.h = h

    def _released(self):
        self._keep = []
        if getattr(self, "_png", None) is not None:
            self._png.close()
            self._png = None

    def feed(self, pass_, row0, pixels, weight=None):
        nl, rows, w, on_device, p, pw, keep = _tile_band(pass_, pixels, weight, None if self.ctx is None else self.ctx.device)
        if w != self.plan["width"] or (pass_ == TILE_PASS_LAYERS and nl != self.num_layers):
            raise ValueError(f"a band of this raster is {self.plan['width']} pixels wide, of {self.num_layers} layers")
        self._check(self.L.och_tile_progress_feed(self.h, int(pass_), int(row0), rows, int(on_device), p, pw))
        self._keep.append(keep if on_device else None)  # the kernel may still read a device band: alive until collected

    def seek(self, pass_, row0):
        """pass_'s next band starts at row0, a tile row: for a caller that reports a part of the raster"""
        self._check(self.L.och_tile_progress_seek(self.h, int(pass_), int(row0)))

    def pending(self):
        return int(self.L.och_tile_progress_pending(self.h))

    def collect(self, raw=False, png=False):
        """png: every update also has png_base64, the thumbnail as the base64 of a PNG file (B G R A in, R G B A in the
        file), the band's tiles encoded as one batch on the object's route"""
        n = C.c_uint64(0)
        self._check(self.L.och_tile_progress_collect(self.h, None, None, 0, C.byref(n)))
        side = min(self.tile_size, 128)
        records = np.zeros(n.value, TILE_UPDATE_DTYPE)
        slots = np.zeros((n.value, side * side, 4), np.uint8)
        self._check(self.L.och_tile_progress_collect(self.h, records.ctypes.data, slots.ctypes.data, n.value, C.byref(n)))
        self._keep.pop(0)
        if raw:
            return records, slots
        updates = []
        for r, slot in zip(records, slots):
            u = {k: (float(r[k]) if r.dtype[k] == np.float64 else int(r[k])) for k in TILE_UPDATE_DTYPE.names}
            u["thumbnail"] = slot[:u["thumb_w"] * u["thumb_h"]].reshape(u["thumb_h"], u["thumb_w"], 4).copy()
            updates.append(u)
        if png and updates:
            if self._png is None:
                self._png = PngEncoder(self.ctx)
            for u, text in zip(updates, self._png.encode([u["thumbnail"] for u in updates], bgr=True, base64=True)):
                u["png_base64"] = text
        return updates


def ortho_tile_updates(plan, pixels, pass_, row0=0, tile_size=None, weight=None, ctx=None):
    """The tile updates of one band of `plan`'s raster from row0 on (TileProgress in one feed): a list of dicts, per tile
    in tile order pixel_x, pixel_y, pixel_w, pixel_h, total_output_width, total_output_height, tile_index (1-based, row-major
    over the whole raster), total_tiles, thumb_w, thumb_h, scale, pass, bounds_min_x, bounds_max_y, meters_per_pixel and
    thumbnail, a (thumb_h, thumb_w, 4) uint8 BGRA array.  pass_ 1: pixels = the layers' bgra (L, rows, width, 4) and weight
    (L, rows, width); the best-weighted valid layer, (0, 0, 0, 51) where none is.  pass_ 2: pixels = the blended rgba (rows,
    width, 4); (0, 0, 0, 0) where alpha is 0.  numpy arrays (ctx None: the CPU route) or CUDA tensors on ctx's device."""
    nl = int(pixels.shape[0]) if pass_ == TILE_PASS_LAYERS and len(pixels.shape) == 4 else 1
    if not isinstance(pixels, np.ndarray):
        import torch

        torch.cuda.current_stream(pixels.device).synchronize()  # the kernel runs on the context's own stream
    with TileProgress(plan, tile_size, nl, ctx=ctx) as t:
        t.seek(pass_, row0)  # a band in the middle of the raster: the pass's order starts where it does
        t.feed(pass_, row0, pixels, weight)
        return t.collect()


# ---- the textured OBJ's JPEG texture (include/oc_host.h) ------------------------------------------------
class JpegEncoder(_Handle):
    """A baseline JPEG (YCbCr 4:2:0, cv::imwrite's settings) of a width x height raster fed band by band (och_jpeg_*; the
    rules: DESIGN.md §4.17).  ctx None: the CPU route, numpy bands.  ctx with on_device: CUDA tensors on ctx's device, fed
    on the context's stream - the caller has torch's work on a band finished before feed, as ortho_blend does.  ctx
    without on_device: numpy bands through the device.  feed(row0, band): band is (rows, width, 3) or (rows, width, 4) uint8,
    channels R, G, B first; bands ascend and are contiguous from row 0, of any row count.  collect(): the file's bytes
    that are complete and not collected yet (the header first).  finish(): the rest, EOI included.  A gap, an overlap, a
    feed after finish and a finish before the last row raise OchipError naming the rows."""

    _destroy, _last_error = "och_jpeg_destroy", "och_jpeg_last_error"

    def __init__(self, width, height, ctx=None, quality=95, on_device=False):
        self.L, self.width, self.height, self.ctx = load(), int(width), int(height), ctx
        self.on_device = bool(on_device)
        if self.on_device and ctx is None:
            raise ValueError("bands on the device need the device route (ctx)")
        self.h = None
        self._keep = []
        h = C.c_void_p()
        self._check(self.L.och_jpeg_create(ctx.h if ctx is not None else None, self.width, self.height, int(quality), C.byref(h)))
        self.h = h

    def _released(self):
        self._keep = []

    def feed(self, row0, band):
        shape = tuple(int(v) for v in band.shape)
        if len(shape) != 3 or shape[1] != self.width or shape[2] not in (3, 4) or str(band.dtype).replace("torch.", "") != "uint8":
            raise ValueError(f"a band of this encoder is (rows, {self.width}, 3 or 4) uint8")
        if self.on_device:
            ptr = _device_ptr(band, "torch.uint8", shape, "band", self.ctx.device)
            self._keep.append(band)  # the kernels may still read it: alive until collect, finish or close
        else:
            band = np.ascontiguousarray(band)
            ptr = band.ctypes.data
        if shape[0] > 0:
            self._check(self.L.och_jpeg_feed(self.h, int(row0), shape[0], ptr, shape[2], int(self.on_device)))

    def pending(self):
        """the bytes collect() would return now"""
        return int(self.L.och_jpeg_pending(self.h))

    def collect(self, cap=None):
        """cap: the room offered (default: exactly what is ready)"""
        return self._collect(cap).tobytes()

    def _collect(self, cap=None):
        """collect() as a uint8 array, for a writer that takes the buffer as it is"""
        n = C.c_uint64(0)
        self._check(self.L.och_jpeg_collect(self.h, None, 0, C.byref(n)))
        self._keep = []  # collect has waited for the kernels
        buf = np.empty(max(int(n.value if cap is None else cap), 1), np.uint8)
        self._check(self.L.och_jpeg_collect(self.h, buf.ctypes.data, int(n.value if cap is None else cap), C.byref(n)))
        return buf[:n.value]

    def finish(self):
        self._check(self.L.och_jpeg_finish(self.h))
        return self.collect()


def encode_jpeg(raster, ctx=None, quality=95):
    """The JPEG file (bytes) of a whole (height, width, 3 or 4) uint8 raster, channels R, G, B first, in one feed: a numpy
    array (ctx None: the CPU route, else through ctx's device) or a CUDA tensor on ctx's device."""
    on_device = not isinstance(raster, np.ndarray)
    if len(raster.shape) != 3:
        raise ValueError("a raster is (height, width, 3 or 4) uint8")
    if on_device:
        if ctx is None:
            raise ValueError("a device raster needs the device route (ctx)")
        import torch

        torch.cuda.current_stream(raster.device).synchronize()  # the kernels run on the context's own stream
    with JpegEncoder(int(raster.shape[1]), int(raster.shape[0]), ctx=ctx, quality=quality, on_device=on_device) as e:
        e.feed(0, raster)
        return e.collect() + e.finish()


# ---- baseline JPEG decoding of the load stage (include/oc_host.h) -----------------------------------------
JPEG_STATUS = ("ok", "unsupported", "corrupt")
JPEG_INFO_DTYPE = np.dtype([("width", "<i4"), ("height", "<i4"), ("components", "<i4"), ("h_samp", "<i4"), ("v_samp", "<i4"),
                            ("restart_interval", "<i4"), ("orientation", "<i4"), ("status", "<i4"), ("offset", "<u8")])
JPEG_LOAD_PIXEL_BUDGET = 1 << 28  # Graph.load_jpegs decodes chunks of at most this many pixels


def _jpeg_bytes(f):
    """a file of the decoder: bytes-like as it is, anything else a path"""
    if isinstance(f, (bytes, bytearray, memoryview)):
        return bytes(f)
    with open(f, "rb") as fh:
        return fh.read()


def _file_name(f):
    """a file of the decoder in a message: its path, or its size when it is bytes"""
    return f"of {len(f)} bytes" if isinstance(f, (bytes, bytearray, memoryview)) else repr(os.fspath(f))


def _jpeg_info_dict(rec):
    d = {k: int(rec[k]) for k in JPEG_INFO_DTYPE.names if k != "offset"}
    d["sampling"] = (d.pop("h_samp"), d.pop("v_samp"))
    d["status"] = JPEG_STATUS[d["status"]]
    return d


def jpeg_info(data, apply_orientation=True):
    """The headers of a JPEG file (bytes or a path): dict(width, height, components, sampling=(h, v) of the luma,
    restart_interval, orientation, status "ok" / "unsupported" / "corrupt").  width and height are the oriented ones when
    apply_orientation.  Reads no entropy-coded bit, needs no context."""
    data = _jpeg_bytes(data)
    rec = np.zeros(1, JPEG_INFO_DTYPE)
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    if load().och_jpeg_info(buf.ctypes.data, len(data), int(bool(apply_orientation)), rec.ctypes.data) != 0:
        raise capi.OchipError(load().och_jpeg_decode_last_error().decode())
    return _jpeg_info_dict(rec[0])


METADATA_STATUS = ["ok", "absent", "corrupt"]
_METADATA_NUMBERS = ["latitude", "longitude", "altitude", "relative_altitude", "roll", "pitch", "yaw", "accuracy_xy", "accuracy_z"]


def jpeg_metadata(data, want_status=False):
    """image_metadata of a JPEG file (bytes or a path), from its EXIF and XMP (och_jpeg_metadata): a dict
    in graph.json's layout and key order - camera_info (dimensions, focal_length_px, principal, make, model, serial_no,
    lens_make, lens_model) and capture_info (latitude ... accuracy_z, datum, timestamp, datestamp).  Absent numbers are NaN,
    absent strings "".  A file with neither Exif nor XMP ("absent") and one whose structure does not hold ("corrupt") give
    the defaults; want_status: (dict, status)."""
    data = _jpeg_bytes(data)
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    numbers, needed, cap = np.zeros(14), C.c_uint64(0), 1024
    L = load()
    while True:
        text = C.create_string_buffer(cap)
        status = L.och_jpeg_metadata(buf.ctypes.data, len(data), numbers, text, cap, C.byref(needed))
        if status >= 0:
            break
        if needed.value <= cap:
            raise capi.OchipError("och_jpeg_metadata: bad arguments")
        cap = int(needed.value)
    s = [t.decode("utf-8", "replace") for t in text.raw[:needed.value].split(b"\0")[:8]]
    v = numbers.tolist()
    camera = dict(dimensions=[int(v[0]), int(v[1])], focal_length_px=v[2], principal=[v[3], v[4]], make=s[0], model=s[1],
                  serial_no=s[2], lens_make=s[3], lens_model=s[4])
    capture = dict(zip(_METADATA_NUMBERS, v[5:]))
    capture.update(datum=s[5], timestamp=s[6], datestamp=s[7])
    out = dict(camera_info=camera, capture_info=capture)
    return (out, METADATA_STATUS[status]) if want_status else out


class GeoCoord(_Handle):
    """The survey's local frame (GeoCoord of the reference; och_geo_*): a Transverse Mercator on WGS84
    about (lat, lon) with k0 = 1 and no false origin, metres east and north of the origin.  The reference writes the origin
    into its WKT with six significant digits, so the projection's centre is `centre` = float("%g" % each) while `origin`
    stays as given; wkt() is that text."""

    _destroy = "och_geo_destroy"

    def __init__(self, lat, lon):
        self.L = load()
        self.h = self.L.och_geo_create(float(lat), float(lon))
        if not self.h:
            raise ValueError(f"GeoCoord: ({lat}, {lon}) is no origin")
        o = np.zeros(4)
        self.L.och_geo_origin(self.h, o)
        self.origin, self.centre = (float(o[0]), float(o[1])), (float(o[2]), float(o[3]))

    def to_local(self, lat, lon, alt=0.0):
        """(lat, lon, alt), scalars or arrays of one length, to (..., 3) easting, northing, altitude; NaN NaN NaN for a
        point that is not finite or 90 degrees or more from the central meridian."""
        lla = np.stack(np.broadcast_arrays(np.asarray(lat, np.float64), np.asarray(lon, np.float64), np.asarray(alt, np.float64)), -1)
        flat = np.ascontiguousarray(lla.reshape(-1, 3))
        out = np.zeros_like(flat)
        if len(flat):
            self.L.och_geo_to_local(self.h, len(flat), flat, out)
        return out.reshape(lla.shape)

    def to_wgs84(self, xyz):
        """(..., 3) local x y z to (..., 3) longitude, latitude, altitude: the order of the reference's toWGS84"""
        xyz = np.asarray(xyz, np.float64)
        flat = np.ascontiguousarray(xyz.reshape(-1, 3))
        out = np.zeros_like(flat)
        if len(flat):
            self.L.och_geo_to_wgs84(self.h, len(flat), flat, out)
        return out.reshape(xyz.shape)

    def wkt(self):
        n = self.L.och_geo_wkt(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        self.L.och_geo_wkt(self.h, buf, n + 1)
        return buf.value.decode()


def _geo_coord(geo):
    """a GeoCoord from what the geo-referenced writers take: one, an (lat, lon) origin, or None"""
    if geo is None or isinstance(geo, GeoCoord):
        return geo
    return GeoCoord(*geo)


def save_geojson(path, graph, geo=None):
    """The camera graph as GeoJSON (Graph.to_geojson) to a file."""
    with open(path, "w", encoding="utf-8") as f:
        f.write(graph.to_geojson(geo))


class JpegBatch:
    """What JpegDecoder.decode returns: status (a name per file), info (jpeg_info's dict per file), shapes ((height, width)
    per file, None where the file was refused), offsets (the image's first byte in pixels, None likewise), pixels (flat
    uint8: a CUDA tensor on the device route, a numpy array on the CPU route) and rounds ((launches of the synchronisation
    kernel, most rounds inside one); (0, 0) on the CPU route).  image(i): the (height, width, 3) B G R view of file i."""

    def __init__(self, info, offsets, pixels, rounds):
        self.info, self.offsets, self.pixels, self.rounds = info, offsets, pixels, rounds
        self.status = [d["status"] for d in info]
        self.shapes = [(d["height"], d["width"]) if d["status"] == "ok" else None for d in info]

    def image(self, i):
        if self.shapes[i] is None:
            raise ValueError(f"file {i} is {self.status[i]}")
        h, w = self.shapes[i]
        return self.pixels[self.offsets[i]:self.offsets[i] + h * w * 3].reshape(h, w, 3)


class JpegDecoder(_Handle):
    """Baseline JPEG files to B G R pixels, a batch per call (och_jpeg_decoder_*; the rules: DESIGN.md §4.18): what
    cv::imread gives - libjpeg-turbo's default decode with the EXIF orientation applied.  ctx: the device route, the pixels
    stay on ctx's device; ctx None: the host loops.  subsequence_bits: the length of the pieces a scan is decoded in on the
    device, a multiple of 32; 0: the default."""

    _destroy, _last_error = "och_jpeg_decoder_destroy", "och_jpeg_decode_last_error"

    def __init__(self, ctx=None, subsequence_bits=0):
        self.L, self.ctx, self.h = load(), ctx, None
        h = C.c_void_p()
        self._check(self.L.och_jpeg_decoder_create(ctx.h if ctx is not None else None, int(subsequence_bits), C.byref(h)))
        self.h = h

    def decode(self, files, out=None, apply_orientation=True):
        """files: bytes objects or paths.  out: where the pixels go - a flat uint8 CUDA tensor on ctx's device (numpy array on
        the CPU route) with room for the images back to back; None: the headers are read once more to size one.  A file
        whose headers are refused takes no room; one whose scan turns out corrupt keeps the room its headers asked for
        and writes nothing.  Either leaves the others alone.  Returns a JpegBatch."""
        datas = [_jpeg_bytes(f) for f in files]
        n = len(datas)
        bufs = [np.frombuffer(d, np.uint8) if len(d) else np.zeros(1, np.uint8) for d in datas]
        ptrs = np.array([b.ctypes.data for b in bufs] + [0], np.uint64)
        sizes = np.array([len(d) for d in datas] + [0], np.uint64)
        rec = np.zeros(n + 1, JPEG_INFO_DTYPE)
        apply = int(bool(apply_orientation))
        if out is None:
            total = 0
            for i in range(n):
                self._check(self.L.och_jpeg_info(int(ptrs[i]), int(sizes[i]), apply, rec[i:].ctypes.data))
                total += int(rec[i]["width"]) * int(rec[i]["height"]) * 3 if rec[i]["status"] == 0 else 0
        if self.ctx is not None:
            import torch

            if out is not None and not hasattr(out, "is_cuda"):
                raise ValueError("out must be a flat uint8 CUDA tensor on the context's device")
            if out is None:
                out = torch.empty(max(total, 1), dtype=torch.uint8, device=f"cuda:{self.ctx.device}")
                torch.cuda.current_stream(out.device).synchronize()
            cap = int(out.numel())
            ptr = _device_ptr(out, "torch.uint8", (cap,), "out", self.ctx.device)
        else:
            if out is None:
                out = np.empty(max(total, 1), np.uint8)
            if not isinstance(out, np.ndarray) or out.dtype != np.uint8 or out.ndim != 1 or not out.flags.c_contiguous:
                raise ValueError("out of the CPU route is a flat contiguous uint8 array")
            cap, ptr = out.size, out.ctypes.data
        rounds = np.zeros(2, np.int32)
        self._check(self.L.och_jpeg_decoder_decode(self.h, n, ptrs.ctypes.data, sizes.ctypes.data, apply, ptr, cap, None, rec.ctypes.data,
                                                   rounds.ctypes.data))
        info = [_jpeg_info_dict(r) for r in rec[:n]]
        offsets = [int(r["offset"]) if d["status"] == "ok" else None for r, d in zip(rec[:n], info)]
        return JpegBatch(info, offsets, out, (int(rounds[0]), int(rounds[1])))


def decode_jpeg(data, ctx=None, apply_orientation=True):
    """The (height, width, 3) B G R uint8 array of one JPEG file (bytes or a path), as cv::imread returns it.  ctx None: the
    host loops; else decoded on ctx's device and fetched.  A refused file raises OchipError with its status."""
    with JpegDecoder(ctx) as d:
        b = d.decode([data], apply_orientation=apply_orientation)
    if b.status[0] != "ok":
        raise capi.OchipError(f"decode_jpeg: the file is {b.status[0]}")
    img = b.image(0)
    return img if isinstance(img, np.ndarray) else img.cpu().numpy()


class _JpegSink:
    """_mosaic's jpeg argument: a path (opened here, closed on close) or a binary file object (flushed on close)"""

    def __init__(self, target, width, height, ctx, quality, on_device):
        self.own = isinstance(target, (str, bytes, os.PathLike))
        self.f = open(target, "wb") if self.own else target
        try:
            self.enc = JpegEncoder(width, height, ctx=ctx, quality=quality, on_device=on_device)
        except Exception:
            if self.own:
                self.f.close()
            raise

    def feed(self, row0, band):
        self.f.write(self.enc._collect())  # what the bands before completed: waits for them alone, not for this band's render
        self.enc.feed(row0, band)

    def finish(self):
        self.f.write(self.enc.finish())

    def close(self):
        self.enc.close()
        if self.own:
            self.f.close()
        else:
            self.f.flush()


# ---- averaged overview levels of the orthomosaic and the DSM (include/oc_host.h) -----------------------
OVERVIEW_RGBA8, OVERVIEW_FLOAT32 = 0, 1


def overview_levels(width, height):
    """[(rows, cols), ...] of the overview levels 1, 2, ... of a width x height raster: one level for every factor
    2^k < min(width, height) - the reference's loop around BuildOverviews - of ceil(height / 2^k) x ceil(width / 2^k)."""
    L = load()
    n = L.och_ortho_overviews_levels(int(width), int(height), None)
    if n < 0:
        raise ValueError(L.och_ortho_overviews_last_error().decode())
    sizes = np.zeros((n, 2), np.int64)
    L.och_ortho_overviews_levels(int(width), int(height), sizes.ctypes.data)
    return [(int(r), int(c)) for r, c in sizes]


def _overview_kind(dtype, shape):
    """(kind, height, width) of a raster or band given by dtype and shape: (rows, width, 4) uint8 or (rows, width) float32"""
    name = str(dtype).replace("torch.", "")
    if name == "uint8" and len(shape) == 3 and shape[2] == 4:
        return OVERVIEW_RGBA8, int(shape[0]), int(shape[1])
    if name == "float32" and len(shape) == 2:
        return OVERVIEW_FLOAT32, int(shape[0]), int(shape[1])
    raise ValueError("an overview raster is (rows, width, 4) uint8 or (rows, width) float32")


class OrthoOverviews(_Handle):
    """The averaged overview levels of a raster fed band by band (och_ortho_overviews_*; the rule: DESIGN.md §4.13).
    kind: OVERVIEW_RGBA8 ((rows, width, 4) uint8 bands, alpha last) or OVERVIEW_FLOAT32 ((rows, width) float32, NaN: no
    data).  ctx None: the CPU route, numpy bands and levels.  ctx with on_device: CUDA tensors, fed on the context's stream
    without a host wait - the caller has torch's work on a band finished before feed, as ortho_blend does - and the levels
    are read after finish().  ctx without on_device: numpy in and out through the device.  levels: the list of level
    arrays, made here when None.  feed(row0, band): bands ascend and are contiguous from row 0, of any row count;
    complete_rows(level) is monotone.  A gap, an overlap, a feed after finish and a finish before the last row raise
    OchipError naming the rows."""

    _destroy, _last_error = "och_ortho_overviews_destroy", "och_ortho_overviews_last_error"

    def __init__(self, kind, width, height, ctx=None, on_device=False, levels=None):
        self.L, self.kind, self.width, self.height, self.ctx = load(), int(kind), int(width), int(height), ctx
        self.on_device = bool(on_device)
        if self.on_device and ctx is None:
            raise ValueError("levels on the device need the device route (ctx)")
        self.h = None
        sizes = overview_levels(width, height)
        tail = (4,) if self.kind == OVERVIEW_RGBA8 else ()
        if self.on_device:
            import torch

            dtype = torch.uint8 if self.kind == OVERVIEW_RGBA8 else torch.float32
            if levels is None:
                levels = [torch.empty(s + tail, dtype=dtype, device=f"cuda:{ctx.device}") for s in sizes]
            ptrs = [_device_ptr(l, str(dtype), s + tail, f"level {k + 1}", ctx.device) for k, (l, s) in enumerate(zip(levels, sizes))]
        else:
            dtype = np.uint8 if self.kind == OVERVIEW_RGBA8 else np.float32
            if levels is None:
                levels = [np.zeros(s + tail, dtype) for s in sizes]
            for k, (l, s) in enumerate(zip(levels, sizes)):
                if not isinstance(l, np.ndarray) or l.shape != s + tail or l.dtype != dtype or not l.flags.c_contiguous:
                    raise ValueError(f"level {k + 1} must be a contiguous {np.dtype(dtype).name} array of {s + tail}")
            ptrs = [l.ctypes.data for l in levels]
        if len(levels) != len(sizes):
            raise ValueError(f"a {width} x {height} raster has {len(sizes)} overview levels")
        self.levels = list(levels)
        arr = (C.c_void_p * max(1, len(ptrs)))(*ptrs)
        h = C.c_void_p()
        self._check(self.L.och_ortho_overviews_create(ctx.h if ctx is not None else None, self.kind, self.width, self.height, arr,
                                                      int(self.on_device), C.byref(h)))
        self.h = h
        self._keep = None

    def _released(self):
        self._keep = None  # one band, not a list: the last fed

    def feed(self, row0, band):
        kind, rows, w = _overview_kind(band.dtype, tuple(band.shape))
        if kind != self.kind or w != self.width:
            raise ValueError(f"a band of this builder is {self.width} pixels wide, kind {self.kind}")
        if self.on_device:
            shape = (rows, w, 4) if kind == OVERVIEW_RGBA8 else (rows, w)
            ptr = _device_ptr(band, str(band.dtype), shape, "band", self.ctx.device)
        else:
            band = np.ascontiguousarray(band)
            ptr = band.ctypes.data
        self._check(self.L.och_ortho_overviews_feed(self.h, int(row0), rows, ptr))
        self._keep = band  # the kernels may still read it: alive until the next feed, finish or close

    def complete_rows(self, level):
        return int(self.L.och_ortho_overviews_complete_rows(self.h, int(level)))

    def finish(self):
        self._check(self.L.och_ortho_overviews_finish(self.h))
        self._keep = None
        return self.levels


def ortho_overviews(raster, ctx=None):
    """The overview levels [level 1, level 2, ...] of a whole raster in one feed: (height, width, 4) uint8 RGBA (or BGRA)
    or (height, width) float32 with NaN as no data; a numpy array (ctx None: the CPU route, else through ctx's device) or
    a CUDA tensor on ctx's device, the levels then CUDA tensors."""
    on_device = not isinstance(raster, np.ndarray)
    kind, h, w = _overview_kind(raster.dtype, tuple(raster.shape))
    if on_device:
        if ctx is None:
            raise ValueError("a device raster needs the device route (ctx)")
        import torch

        torch.cuda.current_stream(raster.device).synchronize()  # the kernels run on the context's own stream
    with OrthoOverviews(kind, w, h, ctx=ctx, on_device=on_device) as b:
        if h > 0:
            b.feed(0, raster)
        return b.finish()


# ---- the orthomosaic and the DSM as tiled DEFLATE GeoTIFFs (include/oc_host.h) ----------------------------
GEOTIFF_TILE, GEOTIFF_PAYLOAD, GEOTIFF_MAX_STREAM = 512, 1 << 20, 1048667
GEOTIFF_BIGTIFF_ABOVE = 2_000_000_000  # uncompressed bytes of the full level: GDAL's BIGTIFF=IF_SAFER as remembered, unpinned
# the rasters between the layer pass and the blend: B G R A per layer, and the two words of a layer's node id
GEOTIFF_LAYERS8, GEOTIFF_CAMERAS32, GEOTIFF_MAX_LAYERS = 2, 3, 2


def geotiff_pixel_bytes(kind, num_layers=1):
    """The bytes of one pixel of a GeoTiffWriter's kind: 4, or 4 (layers) and 8 (cameras) per layer"""
    return 8 * int(num_layers) if kind == GEOTIFF_CAMERAS32 else 4 * int(num_layers) if kind == GEOTIFF_LAYERS8 else 4


def geotiff_stored_bytes(payload):
    """stored_bytes of csrc/deflate_rules.hpp: the size of the stored form of a payload, which no stream exceeds"""
    return 2 + payload + 5 * ((payload + 65534) // 65535) + 4


def deflate_code_lengths(counts, limit):
    """The length limiter of csrc/deflate_rules.hpp alone: code lengths (uint8, 0 for a count of 0) of at most `limit` bits for
    up to 286 symbol counts."""
    counts = np.ascontiguousarray(counts, np.uint32)
    lens = np.zeros(max(len(counts), 1), np.uint8)
    L = load()
    if L.och_deflate_code_lengths(counts.ctypes.data, len(counts), int(limit), lens.ctypes.data) != 0:
        raise capi.OchipError(L.och_geotiff_last_error().decode())
    return lens[:len(counts)]


class _TileEncoder(_Handle):
    """och_geotiff_*: a raster's bands, or predicted payloads, to the zlib streams of its 512 x 512 tiles"""

    _destroy, _last_error = "och_geotiff_destroy", "och_geotiff_last_error"

    def __init__(self, kind, width, height, ctx, sparse, num_layers=None):
        self.L, self.ctx, self.h = load(), ctx, None
        h = C.c_void_p()
        if num_layers is None:
            self._check(self.L.och_geotiff_create(ctx.h if ctx is not None else None, int(kind), int(width), int(height),
                                                  int(bool(sparse)), C.byref(h)))
        else:
            self._check(self.L.och_geotiff_create_layered(ctx.h if ctx is not None else None, int(kind), int(num_layers), int(width),
                                                          int(height), int(bool(sparse)), C.byref(h)))
        self.h = h

    def feed(self, row0, rows, ptr, on_device):
        self._check(self.L.och_geotiff_feed(self.h, int(row0), int(rows), ptr, int(on_device)))

    def payloads(self, arr):
        self._check(self.L.och_geotiff_payloads(self.h, arr.ctypes.data, len(arr)))

    def finish(self):
        self._check(self.L.och_geotiff_finish(self.h))

    def collect(self):
        """(bytes as a uint8 array, counts): the streams of the tiles complete so far, back to back in tile order.  The bytes
        lie in a block this object reuses - a fresh one of a band's size costs more in page faults than the copy into it - so
        they are valid until the next collect."""
        nb, nt = C.c_uint64(0), C.c_uint64(0)
        self._check(self.L.och_geotiff_collect(self.h, None, 0, C.byref(nb), None, 0, C.byref(nt)))
        if getattr(self, "_buf", None) is None or len(self._buf) < nb.value:
            self._buf = np.empty(max(nb.value + nb.value // 4, 1), np.uint8)
        buf, counts = self._buf, np.zeros(max(nt.value, 1), np.uint64)
        self._check(self.L.och_geotiff_collect(self.h, buf.ctypes.data, nb.value, C.byref(nb), counts.ctypes.data, nt.value, C.byref(nt)))
        return buf[:nb.value], counts[:nt.value]


def deflate_tiles(payloads, ctx=None):
    """The zlib streams (a list of bytes) of (n, 1048576) uint8 predicted tile payloads by the rules of csrc/deflate_rules.hpp:
    ctx None the CPU route, else on ctx's device - the same bytes."""
    payloads = np.ascontiguousarray(payloads, np.uint8)
    if payloads.ndim != 2 or payloads.shape[1] != GEOTIFF_PAYLOAD:
        raise ValueError(f"payloads are (n, {GEOTIFF_PAYLOAD}) uint8")
    n, step, out = len(payloads), 4, []
    if n == 0:
        return out
    enc = _TileEncoder(OVERVIEW_RGBA8, GEOTIFF_TILE * min(n, step), 1, ctx, False)
    try:
        for at in range(0, n, step):
            enc.payloads(payloads[at:at + step])
            buf, counts = enc.collect()
            ends = np.cumsum(counts)
            out += [buf[int(e - c):int(e)].tobytes() for c, e in zip(counts, ends)]
    finally:
        enc.close()
    return out


class GeoTiffWriter:
    """A tiled DEFLATE GeoTIFF of a width x height raster fed band by band: the reference's createGeoTIFF (kind
    OVERVIEW_RGBA8: (rows, width, 4) uint8 bands whose four bytes go out as they stand - ortho_blend writes R, G, B, A
    (csrc/ortho_blend.hpp, "Lab -> BGR8 -> RGBA") - with ExtraSamples 2) and createDSMGeoTIFF (OVERVIEW_FLOAT32: (rows, width)
    float32, tag 42113 "nan"): 512 x 512 tiles, Compression 8, Predictor 2, every tile its own zlib stream by the rules of
    csrc/deflate_rules.hpp.  target: a path or a seekable binary file object.  ctx None: the CPU route,
    numpy bands.  ctx with on_device: CUDA tensors on ctx's device, fed on the context's stream - the caller has torch's work
    on a band finished before feed, as ortho_blend does - and a feed never waits for the band it enqueues: it writes the
    tiles the bands before completed.  ctx without on_device: numpy bands through the device.  The routes write the same
    bytes.  geo: dict(min_x, max_y, gsd[, epsg]) for tags 33550, 33922 and 34735; instead of epsg, origin=(lat, lon) or
    coord=GeoCoord writes the local frame's Transverse Mercator as GeoKeys (34735 - 34737).  bigtiff: None chooses BigTIFF above
    2 000 000 000 uncompressed bytes.  sparse: an all-zero RGBA tile gets offset 0 and count 0 and no bytes; DSM tiles are
    always written.  feed(row0, band): bands ascend and are contiguous from row 0, of any row count.  finish(overviews): the
    list of overview level arrays or tensors (OrthoOverviews) become further IFDs with NewSubfileType 1; the file is then
    complete, flushed (an object) or closed (a path).  A gap, an overlap, a wrong kind or width, a feed after finish and a
    finish before the last row raise OchipError naming the rows.

    The reference's createMultiBandGeoTIFF (src/ortho/ortho.cpp:969-1008), the two rasters between
    generateLayeredGeoTIFF and blendLayeredGeoTIFF, are the kinds GEOTIFF_LAYERS8 and GEOTIFF_CAMERAS32 with num_layers 1 or 2
    (the reference's pipeline always has 2).  Their bands come layer-major, as ortho_layers returns them: bgra
    (num_layers, rows, width, 4) uint8, and camera_id (num_layers, rows, width) uint64 - int64 where torch holds it.  The tiles
    are pixel-interleaved: 4 num_layers Byte samples B G R A per layer, respectively 2 num_layers UInt32 samples, the low and
    the high word of each layer's id; Predictor 2 differences a sample with the same sample of the pixel before.  Tags:
    BitsPerSample 8 or 32 per sample, SamplesPerPixel, PlanarConfiguration 1, Photometric 1 (MINISBLACK), ExtraSamples
    (samples - 1 values of 0), SampleFormat 1, the geo tags as above - Photometric and ExtraSamples are GDAL's for a
    multi-band file without colour interpretation as remembered, unpinned.  sparse leaves out the all-zero tiles of both; an
    invalid sample is all zero in both files.  No overview levels: the reference builds none, finish refuses them.  bigtiff: None
    chooses by the kind's own uncompressed size."""

    def __init__(self, target, kind, width, height, geo=None, ctx=None, on_device=False, bigtiff=None, sparse=True, num_layers=None):
        self.enc = self.f = None
        self.kind, self.width, self.height, self.ctx = int(kind), int(width), int(height), ctx
        self.on_device, self.sparse = bool(on_device), bool(sparse)
        self.layered = self.kind in (GEOTIFF_LAYERS8, GEOTIFF_CAMERAS32)
        if not self.layered and self.kind not in (OVERVIEW_RGBA8, OVERVIEW_FLOAT32):
            raise capi.OchipError("a GeoTIFF's kind is OVERVIEW_RGBA8, OVERVIEW_FLOAT32, GEOTIFF_LAYERS8 or GEOTIFF_CAMERAS32")
        if self.layered and num_layers is None:
            raise capi.OchipError("a layers or cameras GeoTIFF needs num_layers")
        if not self.layered and num_layers is not None:
            raise capi.OchipError("num_layers belongs to the kinds GEOTIFF_LAYERS8 and GEOTIFF_CAMERAS32")
        if self.layered and not (isinstance(num_layers, (int, np.integer)) and 1 <= num_layers <= GEOTIFF_MAX_LAYERS):
            raise capi.OchipError(f"num_layers is 1 .. {GEOTIFF_MAX_LAYERS}, not {num_layers!r}")
        self.num_layers = int(num_layers) if self.layered else None
        if self.on_device and ctx is None:
            raise ValueError("bands on the device need the device route (ctx)")
        self.geo = dict(geo) if geo is not None else None
        self.centre = None  # (lat, lon) of the local frame's projection when geo names one instead of an EPSG code
        if self.geo is not None and (self.geo.get("coord") is not None or self.geo.get("origin") is not None):
            if self.geo.get("epsg") is not None:
                raise ValueError("geo names the local frame (origin / coord) or an epsg code, not both")
            self.centre = _geo_coord(self.geo["coord"] if self.geo.get("coord") is not None else self.geo["origin"]).centre
        self.big = self.width * self.height * geotiff_pixel_bytes(self.kind, self.num_layers or 1) > GEOTIFF_BIGTIFF_ABOVE \
            if bigtiff is None else bool(bigtiff)
        self.own = isinstance(target, (str, bytes, os.PathLike))
        if not self.own and not (hasattr(target, "write") and hasattr(target, "seekable") and target.seekable()):
            raise capi.OchipError("a GeoTIFF's target is a path or a seekable binary file object: the first IFD's offset is "
                                  "written last")
        self.enc = _TileEncoder(self.kind, self.width, self.height, ctx, self.sparse, self.num_layers)
        self.f = open(target, "wb") if self.own else target
        self.base = self.f.tell()
        self.f.write(b"II+\0\x08\0\0\0" + bytes(8) if self.big else b"II*\0" + bytes(4))
        self.at = 16 if self.big else 8      # the file's length so far
        self.link = 8 if self.big else 4     # where the next IFD's offset goes
        self.tiles = []                      # (offset, count) of the level being written
        self.finished = False
        self._keep = []

    def close(self):
        if self.enc is not None:
            self.enc.close()
            self.enc = None
        if self.f is not None:
            if self.own:
                self.f.close()
            else:
                self.f.flush()
            self.f = None
        self._keep = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def _write(self, data):
        """at an even offset; returns it"""
        if self.at & 1:
            self.f.write(b"\0")
            self.at += 1
        at = self.at
        self.f.write(data)
        self.at += len(data)
        if not self.big and self.at >= 1 << 32:
            raise capi.OchipError("the file outgrows a classic TIFF's 32-bit offsets: bigtiff=True")
        return at

    def _take(self, enc):
        buf, counts = enc.collect()
        at = 0
        for c in counts:
            c = int(c)
            self.tiles.append((self._write(memoryview(buf[at:at + c])), c) if c else (0, 0))
            at += c

    def feed(self, row0, band):
        if self.enc is None:
            raise capi.OchipError("the writer is closed")
        if self.layered:
            name, shape = str(band.dtype).replace("torch.", ""), tuple(int(v) for v in band.shape)
            want = (self.num_layers, shape[1] if len(shape) > 1 else 0, self.width) + ((4,) if self.kind == GEOTIFF_LAYERS8 else ())
            if shape != want or name not in (("uint8",) if self.kind == GEOTIFF_LAYERS8 else ("uint64", "int64")):
                raise capi.OchipError(f"rows from {int(row0)}: a band of this writer is ({self.num_layers}, rows, {self.width}" +
                                      (", 4) uint8" if self.kind == GEOTIFF_LAYERS8 else ") uint64 or int64") +
                                      f", not {shape} {name}")
            kind, rows, w = self.kind, shape[1], self.width
        else:
            try:
                kind, rows, w = _overview_kind(band.dtype, tuple(band.shape))
            except ValueError:
                kind, rows, w = -1, 0, 0
        if kind != self.kind or w != self.width:
            raise capi.OchipError(f"rows from {int(row0)}: a band of this writer is {self.width} pixels wide, kind {self.kind}")
        self._take(self.enc)  # what the bands before completed: waits for them alone, not for this band
        self._keep = []
        if self.on_device:
            shape = tuple(band.shape) if self.layered else (rows, w, 4) if kind == OVERVIEW_RGBA8 else (rows, w)
            ptr = _device_ptr(band, str(band.dtype), shape, "band", self.ctx.device)
            self._keep.append(band)  # the copy may still read it: alive until the next feed, finish or close
        else:
            band = np.ascontiguousarray(band)
            ptr = band.ctypes.data
        if rows > 0:
            self.enc.feed(row0, rows, ptr, self.on_device)

    def _ifd(self, width, height, overview):
        rgba, big = self.kind == OVERVIEW_RGBA8, self.big
        n = 4 if rgba else 1
        bits = [8] * 4 if rgba else [32]
        if self.layered:  # 4 Byte samples or 2 UInt32 samples a layer
            n = (4 if self.kind == GEOTIFF_LAYERS8 else 2) * self.num_layers
            bits = [8 if self.kind == GEOTIFF_LAYERS8 else 32] * n
        S, L, D, A, L8 = 3, 4, 12, 2, 16
        offsets = np.array([t[0] for t in self.tiles], np.uint64)
        tags = []
        if overview:
            tags.append((254, L, [1]))
        tags += [(256, L, [width]), (257, L, [height]), (258, S, bits), (259, S, [8]), (262, S, [2 if rgba else 1]),
                 (277, S, [n]), (284, S, [1]), (317, S, [2]), (322, S, [GEOTIFF_TILE]), (323, S, [GEOTIFF_TILE]),
                 (324, L8 if big else L, offsets), (325, L, [t[1] for t in self.tiles])]
        if rgba:
            tags.append((338, S, [2]))
        if self.layered:
            tags.append((338, S, [0] * (n - 1)))
        tags.append((339, S, [1] * n if rgba or self.layered else [3]))
        if self.geo is not None and not overview:
            g = self.geo
            keys = [(1025, 0, 1, 1)]
            if g.get("epsg") is not None:
                keys = [(1024, 0, 1, 1), (1025, 0, 1, 1), (3072, 0, 1, int(g["epsg"]))]
            doubles, ascii_ = [], b""
            if self.centre is not None:  # the local frame: a user-defined Transverse Mercator on WGS 84
                names = [b"Custom Transverse Mercator|", b"WGS 84|"]
                doubles = [self.centre[1], self.centre[0], 0.0, 0.0, 1.0]
                ascii_ = b"".join(names) + b"\0"
                keys = [(1024, 0, 1, 1), (1025, 0, 1, 1), (1026, 34737, len(names[0]), 0), (2048, 0, 1, 4326),
                        (2049, 34737, len(names[1]), len(names[0])), (2054, 0, 1, 9102), (3072, 0, 1, 32767), (3074, 0, 1, 32767),
                        (3075, 0, 1, 1), (3076, 0, 1, 9001)] + [(k, 34736, 1, i) for i, k in enumerate((3080, 3081, 3082, 3083, 3092))]
            tags.append((33550, D, [float(g["gsd"]), float(g["gsd"]), 0.0]))
            tags.append((33922, D, [0.0, 0.0, 0.0, float(g["min_x"]), float(g["max_y"]), 0.0]))
            tags.append((34735, S, [1, 1, 0, len(keys)] + [v for k in keys for v in k]))
            if doubles:
                tags.append((34736, D, doubles))
                tags.append((34737, A, ascii_))
        if self.kind == OVERVIEW_FLOAT32:
            tags.append((42113, A, b"nan\0"))
        dtypes = {S: "<u2", L: "<u4", D: "<f8", L8: "<u8"}
        inline, entries = 8 if big else 4, []
        for tag, typ, values in sorted(tags, key=lambda t: t[0]):
            data = bytes(values) if typ == A else np.asarray(values).astype(dtypes[typ]).tobytes()
            count = len(values)
            field = data.ljust(inline, b"\0") if len(data) <= inline else \
                np.array([self._write(data)], "<u8" if big else "<u4").tobytes()
            entries.append(np.array([tag, typ], "<u2").tobytes() + np.array([count], "<u8" if big else "<u4").tobytes() + field)
        head = np.array([len(entries)], "<u8" if big else "<u2").tobytes()
        at = self._write(head + b"".join(entries) + bytes(inline))
        self.f.seek(self.base + self.link)
        self.f.write(np.array([at], "<u8" if big else "<u4").tobytes())
        self.f.seek(self.base + self.at)
        self.link = self.at - inline
        self.tiles = []

    def finish(self, overviews=None):
        if self.enc is None or self.finished:
            raise capi.OchipError("the writer is finished or closed")
        levels = list(overviews) if overviews is not None else []
        if levels and self.layered:
            raise capi.OchipError("the layers and cameras rasters have no overview levels")
        sizes = overview_levels(self.width, self.height) if levels else []
        if len(levels) != len(sizes):
            raise capi.OchipError(f"a {self.width} x {self.height} raster has {len(sizes)} overview levels, {len(levels)} came")
        self.enc.finish()
        self.finished = True
        self._take(self.enc)
        self._keep = []
        self.enc.close()
        self.enc = None
        self._ifd(self.width, self.height, False)
        for k, (level, (rows, cols)) in enumerate(zip(levels, sizes)):
            kind, lr, lc = _overview_kind(level.dtype, tuple(level.shape))
            if kind != self.kind or (lr, lc) != (rows, cols):
                raise capi.OchipError(f"overview level {k + 1} is {cols} x {rows} of kind {self.kind}")
            on_device = not isinstance(level, np.ndarray)
            if on_device and self.ctx is None:
                raise capi.OchipError("an overview level on the device needs the device route (ctx)")
            enc = _TileEncoder(self.kind, cols, rows, self.ctx, self.sparse)
            try:
                if on_device:
                    shape = (rows, cols, 4) if kind == OVERVIEW_RGBA8 else (rows, cols)
                    enc.feed(0, rows, _device_ptr(level, str(level.dtype), shape, f"level {k + 1}", self.ctx.device), True)
                else:
                    level = np.ascontiguousarray(level)
                    enc.feed(0, rows, level.ctypes.data, False)
                enc.finish()
                self._take(enc)
            finally:
                enc.close()
            self._ifd(cols, rows, True)
        self.close()


def save_geotiff(target, raster, geo=None, ctx=None, overviews=True, bigtiff=None, sparse=True):
    """A whole raster - (height, width, 4) uint8 RGBA or (height, width) float32 with NaN as no data; a numpy array (ctx None:
    the CPU route, else through ctx's device) or a CUDA tensor on ctx's device - as a GeoTiffWriter's file, with its averaged
    overview levels (ortho_overviews, on the same route) when overviews."""
    on_device = not isinstance(raster, np.ndarray)
    kind, h, w = _overview_kind(raster.dtype, tuple(raster.shape))
    if on_device:
        if ctx is None:
            raise ValueError("a device raster needs the device route (ctx)")
        import torch

        torch.cuda.current_stream(raster.device).synchronize()  # the kernels run on the context's own stream
    levels = ortho_overviews(raster, ctx=ctx) if overviews else None
    with GeoTiffWriter(target, kind, w, h, geo=geo, ctx=ctx, on_device=on_device, bigtiff=bigtiff, sparse=sparse) as wr:
        wr.feed(0, raster)
        wr.finish(levels)


# ---- reading tiled DEFLATE GeoTIFFs (include/oc_host.h) -------------------------------------------------------
INFLATE_OK, INFLATE_CORRUPT = 0, 1
INFLATE_MAX_STREAMS = 65535
GEOTIFF_MAX_TILE_BYTES = 4 << 20


class GeoTiffError(ValueError):
    """status: "unsupported" (a file this reader does not take: the reason is the text), "corrupt" (a structure that does not
    parse or a tile whose stream does not check) or "refused" (the library refused the call)"""

    def __init__(self, status, text):
        super().__init__(f"{status}: {text}")
        self.status = status


class _TileReader(_Handle):
    """och_geotiff_reader_*: zlib streams to payloads, and a layout's tile streams to a raster"""

    _destroy, _last_error = "och_geotiff_reader_destroy", "och_geotiff_read_last_error"

    @staticmethod
    def _failure(text):
        return GeoTiffError("refused", text)

    def __init__(self, samples, is_float, width, height, tile_w, tile_h, predictor, ctx, budget=0, layered=None):
        """layered: None, or (kind, num_layers) of a layers or cameras raster, for which samples and is_float do not count"""
        self.L, self.ctx, self.h = load(), ctx, None
        h = C.c_void_p()
        if layered is None:
            self._check(self.L.och_geotiff_reader_create(ctx.h if ctx is not None else None, int(samples), int(bool(is_float)), int(width),
                                                         int(height), int(tile_w), int(tile_h), int(predictor), int(budget), C.byref(h)))
        else:
            self._check(self.L.och_geotiff_reader_create_layered(ctx.h if ctx is not None else None, int(layered[0]), int(layered[1]),
                                                                 int(width), int(height), int(tile_w), int(tile_h), int(predictor),
                                                                 int(budget), C.byref(h)))
        self.h = h

    def launches(self):
        return int(self.L.och_geotiff_reader_launches(self.h))

    def inflate(self, packed, offsets, expect):
        """(payloads as one uint8 array, slot offsets, status, bytes) of the packed streams"""
        n = len(expect)
        slots = np.zeros(n + 1, np.uint64)
        np.cumsum((expect + np.uint64(15)) & ~np.uint64(15), out=slots[1:])
        out = np.empty(max(int(slots[-1]), 1), np.uint8)
        status, produced = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64)
        self._check(self.L.och_geotiff_reader_inflate(self.h, n, packed.ctypes.data, offsets.ctypes.data, expect.ctypes.data,
                                                      out.ctypes.data, int(slots[-1]), status.ctypes.data, produced.ctypes.data))
        return out, slots, status[:n], produced[:n]

    def read(self, packed, offsets, row0, rows, ptr, on_device):
        bad = C.c_int64(-1)
        self._check(self.L.och_geotiff_reader_read(self.h, len(offsets) - 1, packed.ctypes.data, offsets.ctypes.data, int(row0), int(rows),
                                                   ptr, int(bool(on_device)), C.byref(bad)))
        return int(bad.value)


def _pack_streams(pieces):
    """(packed uint8 array, offsets uint64 [n + 1]) of a list of bytes-like streams back to back"""
    offsets = np.zeros(len(pieces) + 1, np.uint64)
    if pieces:
        np.cumsum([len(p) for p in pieces], out=offsets[1:])
    packed = np.empty(max(int(offsets[-1]), 1), np.uint8)
    for p, at in zip(pieces, offsets[:-1]):
        if len(p):
            packed[int(at):int(at) + len(p)] = np.frombuffer(p, np.uint8)
    return packed, offsets


def inflate_report(streams, expect, ctx=None, budget=0):
    """inflate_streams without the raise: a list of (status, produced, payload) per stream - INFLATE_OK with the payload's
    bytes, or INFLATE_CORRUPT with None - and `produced`, the bytes the stream gave before it ended or was refused."""
    streams = list(streams)
    n = len(streams)
    expect = np.full(n, expect, np.uint64) if np.ndim(expect) == 0 else np.ascontiguousarray(expect, np.uint64)
    if len(expect) != n:
        raise ValueError(f"{n} streams and {len(expect)} sizes")
    packed, offsets = _pack_streams(streams)
    rd = _TileReader(1, False, 16, 16, 16, 16, 1, ctx, budget)
    try:
        out, slots, status, produced = rd.inflate(packed, offsets, expect)
    finally:
        rd.close()
    return [(int(status[i]), int(produced[i]),
             out[int(slots[i]):int(slots[i]) + int(expect[i])].tobytes() if status[i] == INFLATE_OK else None) for i in range(n)]


def inflate_streams(streams, expect, ctx=None, budget=0):
    """The counterpart of deflate_tiles: the payloads (a list of bytes) of zlib streams (a list of bytes) of known sizes -
    `expect`, one size or a list - by the rules of csrc/inflate_rules.hpp: ctx None the host route, else on ctx's device (one
    wavefront a stream; budget: the device scratch a launch may take, 0 for the default) - the same bytes.  A stream that
    does not give exactly its size, does not end with a final block, fails its Adler-32 or has bytes behind it raises
    GeoTiffError("corrupt") naming the stream's index."""
    report = inflate_report(streams, expect, ctx=ctx, budget=budget)
    for i, (status, produced, _) in enumerate(report):
        if status != INFLATE_OK:
            raise GeoTiffError("corrupt", f"stream {i} of {len(report)}: not a zlib stream of exactly its expected size ({produced} bytes "
                                          f"produced)")
    return [payload for _, _, payload in report]


_TIFF_TYPES = {1: "u1", 2: "S1", 3: "<u2", 4: "<u4", 5: "<u4", 6: "i1", 7: "u1", 8: "<i2", 9: "<i4", 10: "<i4", 11: "<f4", 12: "<f8",
               16: "<u8", 17: "<i8", 18: "<u8"}


class GeoTiffReader:
    """A tiled DEFLATE GeoTIFF read back: the file GeoTiffWriter writes, and what GDAL writes with the same options.  source: a
    path, bytes, or a seekable binary file object.  The structure - header, the IFD chain, the tile arrays - is parsed here;
    the tiles are inflated, un-predicted and placed by och_geotiff_reader_* (DESIGN.md §4.21): ctx None the host route (one
    tile a thread), else on ctx's device (one wavefront a tile; the raster stays there with on_device).  It never changes
    route by size.  Measured on the MI355X (profiles/geotiff_read_probe.json) the device route is the slower
    one: a 16 384 x 16 384 RGBA file of 1 024 tiles takes 0.27 - 0.52 s on the device and 0.18 s on 16 host threads, a
    64-tile file 0.12 - 0.25 s against 0.012 s.  Take it for pixels that must end on the device.
    width, height, samples, kind (OVERVIEW_RGBA8, OVERVIEW_FLOAT32, GEOTIFF_LAYERS8, GEOTIFF_CAMERAS32, or None for 1 or 3
    Byte samples), num_layers (of the kinds GEOTIFF_LAYERS8 and GEOTIFF_CAMERAS32, else None), levels ([(rows, cols), ...]
    of the overview IFDs), geo (dict(min_x, max_y, gsd_x, gsd_y, epsg) from tags 33550 / 33922 / 34735, or None), projection (dict(kind="tmerc", lat0, lon0, k0, false_easting, false_northing) of a
    user-defined Transverse Mercator in the GeoKeys, or None) and nodata
    (tag 42113 as a float, or None).
    Taken: little-endian classic and BigTIFF, tiles with sides that are multiples of 16 and a payload of at most 4 MiB,
    Compression 8 and 32946, Predictor 1 and 2, PlanarConfiguration 1, 8-bit unsigned samples 1, 3 or 4 to a pixel, one
    float32, and the two rasters between the layer pass and the blend: 8 Byte samples are GEOTIFF_LAYERS8
    with two layers of B G R A, 2 or 4 UInt32 samples GEOTIFF_CAMERAS32 with one or two layers' 64-bit ids as a low and a
    high word.  4 Byte samples stay OVERVIEW_RGBA8, which one layer of colours is (read_layer_files reshapes it).  Those two
    kinds are read layer-major, as ortho_blend takes its layers.  Everything else - big-endian files, strips, other compressions (none included), Predictor 3, planar 2, other
    sample formats or depths - raises GeoTiffError("unsupported") with the reason; offsets or counts outside the file, IFD
    loops, tile arrays of the wrong length and any tile whose stream does not check raise GeoTiffError("corrupt"), the last
    naming the level and the tile, and no part of the raster is returned."""

    def __init__(self, source, ctx=None, budget=0):
        self.ctx, self.budget, self._readers, self._f, self._map = ctx, int(budget), {}, None, None
        self.buf = None
        if isinstance(source, (bytes, bytearray, memoryview)):
            self.buf = np.frombuffer(source, np.uint8)
        elif isinstance(source, (str, os.PathLike)):
            import mmap

            self._f = open(source, "rb")
            if os.fstat(self._f.fileno()).st_size == 0:
                self.close()
                raise GeoTiffError("corrupt", "the file is empty")
            self._map = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
            self.buf = np.frombuffer(self._map, np.uint8)
        elif hasattr(source, "read") and hasattr(source, "seekable") and source.seekable():
            source.seek(0)  # the file begins at the object's start, wherever a writer left its position
            self.buf = np.frombuffer(source.read(), np.uint8)
        else:
            raise GeoTiffError("refused", "a GeoTIFF's source is a path, bytes or a seekable binary file object")
        try:
            self._parse()
        except BaseException:
            self.close()
            raise

    # -- the structure
    def _at(self, off, n, what):
        if off < 0 or n < 0 or off + n > len(self.buf):
            raise GeoTiffError("corrupt", f"{what} at {off} + {n} lies outside the file's {len(self.buf)} bytes")
        return self.buf[off:off + n]

    def _num(self, off, dtype, what):
        return int(self._at(off, np.dtype(dtype).itemsize, what).view(dtype)[0])

    def _parse(self):
        head = bytes(self._at(0, 8, "the header"))
        if head[:2] == b"MM":
            raise GeoTiffError("unsupported", "a big-endian file")
        if head[:2] != b"II" or head[2:4] not in (b"*\0", b"+\0"):
            raise GeoTiffError("corrupt", "not a TIFF header")
        self.big = head[2:4] == b"+\0"
        if self.big:
            if bytes(self._at(4, 4, "the BigTIFF header")) != b"\x08\0\0\0":
                raise GeoTiffError("corrupt", "a BigTIFF header's offset size is 8")
            at = self._num(8, "<u8", "the first IFD's offset")
        else:
            at = self._num(4, "<u4", "the first IFD's offset")
        self._ifds, seen = [], set()
        while at:
            if at in seen or len(seen) > 64:
                raise GeoTiffError("corrupt", f"the IFD chain returns to offset {at}" if at in seen else "more than 64 IFDs")
            seen.add(at)
            tags, at = self._read_ifd(at)
            self._ifds.append(self._layout(tags, len(self._ifds)))
        if not self._ifds:
            raise GeoTiffError("corrupt", "no IFD")
        first = self._ifds[0]
        self.width, self.height, self.samples, self.is_float = first["width"], first["height"], first["samples"], first["is_float"]
        self.kind = OVERVIEW_FLOAT32 if self.is_float else OVERVIEW_RGBA8 if self.samples == 4 else None
        self.num_layers = None
        if first["layered"] is not None:
            self.kind, self.num_layers = first["layered"]
        for k, lv in enumerate(self._ifds[1:]):
            if (lv["samples"], lv["is_float"], lv["layered"]) != (self.samples, self.is_float, first["layered"]):
                raise GeoTiffError("unsupported", f"level {k + 1} has another sample layout than the full raster")
        self.levels = [(lv["height"], lv["width"]) for lv in self._ifds[1:]]
        tags = first["tags"]
        self.geo = None
        if 33550 in tags and 33922 in tags and len(tags[33550]) >= 2 and len(tags[33922]) >= 6:
            sx, sy = float(tags[33550][0]), float(tags[33550][1])
            i, j, _, x, y = (float(v) for v in tags[33922][:5])
            epsg, keys = None, tags.get(34735)
            if keys is not None and len(keys) >= 4:
                for q in range(min(int(keys[3]), (len(keys) - 4) // 4)):
                    key, loc, _, value = (int(v) for v in keys[4 + 4 * q:8 + 4 * q])
                    if loc == 0 and (key == 3072 or (key == 2048 and epsg is None)):
                        epsg = value
            self.geo = dict(min_x=x - i * sx, max_y=y + j * sy, gsd_x=sx, gsd_y=sy, epsg=epsg)
        self.projection = self._projection(tags)
        self.nodata = None
        if 42113 in tags:
            try:
                self.nodata = float(bytes(tags[42113]).split(b"\0")[0].decode("ascii").strip())
            except (ValueError, UnicodeDecodeError):
                self.nodata = None

    @staticmethod
    def _projection(tags):
        """dict(kind="tmerc", lat0, lon0, k0, false_easting, false_northing) of a user-defined Transverse Mercator in the
        GeoKeys (3075 = 1; its parameters in tag 34736), else None"""
        keys, doubles = tags.get(34735), tags.get(34736)
        if keys is None or isinstance(keys, bytes) or len(keys) < 4 or doubles is None or isinstance(doubles, bytes):
            return None
        short, real = {}, {}
        for q in range(min(int(keys[3]), (len(keys) - 4) // 4)):
            key, loc, count, value = (int(v) for v in keys[4 + 4 * q:8 + 4 * q])
            if loc == 0:
                short[key] = value
            elif loc == 34736 and count >= 1 and value < len(doubles):
                real[key] = float(doubles[value])
        if short.get(3075) != 1 or 3080 not in real or 3081 not in real:
            return None
        return dict(kind="tmerc", lat0=real[3081], lon0=real[3080], k0=real.get(3092, 1.0), false_easting=real.get(3082, 0.0),
                    false_northing=real.get(3083, 0.0))

    def _read_ifd(self, at):
        big = self.big
        count = self._num(at, "<u8" if big else "<u2", "an IFD's entry count")
        esize, inline, body = (20, 8, at + 8) if big else (12, 4, at + 2)
        if count > 4096:
            raise GeoTiffError("corrupt", f"an IFD of {count} entries")
        raw = self._at(body, count * esize + inline, "an IFD")
        tags = {}
        for k in range(count):
            e = raw[k * esize:(k + 1) * esize]
            tag, typ = int(e[0:2].view("<u2")[0]), int(e[2:4].view("<u2")[0])
            n = int(e[4:12].view("<u8")[0]) if big else int(e[4:8].view("<u4")[0])
            if typ not in _TIFF_TYPES:
                continue
            dt = np.dtype(_TIFF_TYPES[typ])
            size = n * dt.itemsize * (2 if typ in (5, 10) else 1)
            if size > len(self.buf):
                raise GeoTiffError("corrupt", f"tag {tag} claims {size} bytes")
            field = e[esize - inline:]
            data = field[:size] if size <= inline else self._at(int(field.view("<u8" if big else "<u4")[0]), size, f"tag {tag}'s values")
            tags[tag] = bytes(data) if typ == 2 else np.frombuffer(bytes(data), dt)
        nxt = raw[count * esize:]
        return tags, int(nxt.view("<u8" if big else "<u4")[0])

    def _layout(self, tags, index):
        what = f"level {index}"

        def one(tag, default=None):
            if tag not in tags or isinstance(tags[tag], bytes) or len(tags[tag]) == 0:
                if default is None:
                    raise GeoTiffError("corrupt", f"{what}: tag {tag} is missing")
                return default
            return int(tags[tag][0])

        width, height = one(256), one(257)
        if width < 1 or height < 1 or width > 1048576 or height > 1048576:
            raise GeoTiffError("corrupt", f"{what}: a raster of {width} x {height}")
        if 322 not in tags or 323 not in tags or 324 not in tags or 325 not in tags:
            raise GeoTiffError("unsupported" if 273 in tags else "corrupt", f"{what}: strips, not tiles" if 273 in tags
                               else f"{what}: no tile tags")
        comp, planar, pred, samples, fmt = one(259, 1), one(284, 1), one(317, 1), one(277, 1), one(339, 1)
        bits = [int(v) for v in tags[258]] if 258 in tags and not isinstance(tags[258], bytes) else [1]
        if comp not in (8, 32946):
            raise GeoTiffError("unsupported", f"{what}: compression {comp}, not DEFLATE (8 or 32946)")
        if planar != 1:
            raise GeoTiffError("unsupported", f"{what}: PlanarConfiguration {planar}")
        if pred not in (1, 2):
            raise GeoTiffError("unsupported", f"{what}: Predictor {pred}")
        is_float = fmt == 3 and bits == [32] and samples == 1
        # the rasters between the layer pass and the blend: 8 Byte samples are two layers of B G R A, 2 or 4
        # UInt32 samples the ids of one or two layers; 4 Byte samples stay RGBA8, which one layer of colours is
        layered = None
        if fmt == 1 and samples == 8 and bits == [8] * 8:
            layered = (GEOTIFF_LAYERS8, 2)
        elif fmt == 1 and samples in (2, 4) and bits == [32] * samples:
            layered = (GEOTIFF_CAMERAS32, samples // 2)
        if layered is None and not is_float and not (fmt == 1 and samples in (1, 3, 4) and bits == [8] * samples):
            raise GeoTiffError("unsupported", f"{what}: {samples} samples of {bits} bits, SampleFormat {fmt}")
        tw, th = one(322), one(323)
        bpp = geotiff_pixel_bytes(*layered) if layered else 4 if is_float else samples
        if tw < 16 or th < 16 or tw % 16 or th % 16 or tw * th * bpp > GEOTIFF_MAX_TILE_BYTES:
            raise GeoTiffError("unsupported", f"{what}: tiles of {tw} x {th} (sides are multiples of 16, a payload at most 4 MiB)")
        tiles_x, tiles_y = -(-width // tw), -(-height // th)
        for tag in (324, 325):
            if isinstance(tags[tag], bytes) or tags[tag].dtype.kind != "u":
                raise GeoTiffError("corrupt", f"{what}: tag {tag}'s values are not unsigned integers")
        offs, cnts = tags[324].astype(np.uint64), tags[325].astype(np.uint64)
        if len(offs) != tiles_x * tiles_y or len(cnts) != tiles_x * tiles_y:
            raise GeoTiffError("corrupt", f"{what}: {len(offs)} tile offsets and {len(cnts)} counts for {tiles_x} x {tiles_y} tiles")
        live = cnts > 0
        if np.any(offs[live] > len(self.buf)) or np.any(cnts[live] > len(self.buf)) or np.any(offs[live] + cnts[live] > len(self.buf)):
            k = int(np.flatnonzero(live & ((offs > len(self.buf)) | (cnts > len(self.buf)) | (offs + cnts > len(self.buf))))[0])
            raise GeoTiffError("corrupt", f"{what}: tile {k} at {int(offs[k])} + {int(cnts[k])} lies outside the file's {len(self.buf)} bytes")
        return dict(width=width, height=height, samples=samples, is_float=is_float, tile_w=tw, tile_h=th, predictor=pred,
                    tiles_x=tiles_x, tiles_y=tiles_y, offsets=offs, counts=cnts, tags=tags, layered=layered, bpp=bpp)

    # -- the pattern of the other classes
    def close(self):
        for rd in getattr(self, "_readers", {}).values():
            rd.close()
        self._readers = {}
        self.buf = None
        if getattr(self, "_map", None) is not None:
            try:
                self._map.close()
            except BufferError:  # an array over the map is still alive: the map goes with it
                pass
            self._map = None
        if getattr(self, "_f", None) is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        self.close()

    def launches(self, level=0):
        """the inflate launches of the device route for `level` so far"""
        return self._readers[level].launches() if level in self._readers else 0

    def read(self, row0=0, rows=None, level=0, out=None, on_device=False):
        """Rows [row0, row0 + rows) of level `level` (0: the full raster): (rows, width, samples) uint8 or (rows, width)
        float32, a numpy array, or with on_device a CUDA tensor on ctx's device.  The kinds GEOTIFF_LAYERS8 and
        GEOTIFF_CAMERAS32 come layer-major: (num_layers, rows, width, 4) uint8 B G R A, respectively (num_layers, rows, width)
        ids, uint64 in a numpy array and int64 in a CUDA tensor.  Any row window inside the level is taken; the tile rows
        that cover it are decoded: their streams are copied into one block tile by tile, and a read on the device waits for
        torch's stream first.  out: the array or tensor to fill."""
        if self.buf is None:
            raise GeoTiffError("refused", "the reader is closed")
        if not 0 <= int(level) < len(self._ifds):
            raise ValueError(f"level {level} of a file with {len(self._ifds) - 1} overview levels")
        lv = self._ifds[int(level)]
        w, h, th = lv["width"], lv["height"], lv["tile_h"]
        row0 = int(row0)
        rows = h - row0 if rows is None else int(rows)
        if row0 < 0 or rows < 0 or row0 + rows > h:
            raise ValueError(f"rows {row0} .. {row0 + rows} of a level of {h} rows")
        if on_device and self.ctx is None:
            raise ValueError("a raster on the device needs the device route (ctx)")
        shape = (rows, w) if lv["is_float"] else (rows, w, lv["samples"])
        dtype = "float32" if lv["is_float"] else "uint8"
        if lv["layered"] is not None:  # layer-major, as ortho_blend takes its layers; torch holds the ids as int64
            kind, nl = lv["layered"]
            shape = (nl, rows, w, 4) if kind == GEOTIFF_LAYERS8 else (nl, rows, w)
            dtype = "uint8" if kind == GEOTIFF_LAYERS8 else "int64" if on_device else "uint64"
        if on_device:
            import torch

            if out is None:
                out = torch.empty(shape, dtype=getattr(torch, dtype), device=f"cuda:{self.ctx.device}")
            torch.cuda.current_stream(out.device).synchronize()  # the kernels run on the context's own stream
            ptr = _device_ptr(out, "torch." + dtype, shape, "out", self.ctx.device) if rows else None
        else:
            if out is None:
                out = np.empty(shape, dtype)
            if not isinstance(out, np.ndarray) or out.shape != shape or out.dtype != np.dtype(dtype) or not out.flags.c_contiguous or \
                    not out.flags.writeable:
                raise ValueError(f"out must be a writeable C-contiguous {dtype} array of {shape}")
            ptr = out.ctypes.data
        if rows == 0:
            return out
        ty0, ty1 = row0 // th, -(-(row0 + rows) // th)
        lo, hi = ty0 * lv["tiles_x"], ty1 * lv["tiles_x"]
        offs, cnts = lv["offsets"][lo:hi], lv["counts"][lo:hi]
        offsets = np.zeros(hi - lo + 1, np.uint64)
        np.cumsum(cnts, out=offsets[1:])
        packed = np.empty(max(int(offsets[-1]), 1), np.uint8)
        for o, c, at in zip(offs, cnts, offsets[:-1]):
            if c:
                packed[int(at):int(at + c)] = self.buf[int(o):int(o + c)]
        if level not in self._readers:
            self._readers[level] = _TileReader(lv["samples"], lv["is_float"], w, h, lv["tile_w"], th, lv["predictor"], self.ctx, self.budget,
                                               layered=lv["layered"])
        bad = self._readers[level].read(packed, offsets, row0, rows, ptr, on_device)
        if bad >= 0:
            tx, ty = bad % lv["tiles_x"], ty0 + bad // lv["tiles_x"]
            raise GeoTiffError("corrupt", f"level {level}, tile ({tx}, {ty}): its stream is not a zlib stream of exactly "
                                          f"{lv['tile_w'] * th * lv['bpp']} bytes")
        return out


def load_geotiff(source, ctx=None, level=0, on_device=False):
    """(raster, geo) of a tiled DEFLATE GeoTIFF (GeoTiffReader): level `level` as a numpy array (ctx None: the host route, else
    through ctx's device) or, with on_device, a CUDA tensor on ctx's device; geo as GeoTiffReader.geo.  Measured on the
    MI355X the device route is the slower one at 64 and at 1 024 tiles: take it for a raster that must end
    on the device."""
    with GeoTiffReader(source, ctx=ctx) as rd:
        return rd.read(level=level, on_device=on_device), rd.geo


def _open_layer_files(layers, cameras, ctx, budget=0):
    """The two readers of a layers and a cameras file that belong together, checked; the caller closes both"""
    if layers is None or cameras is None:
        raise GeoTiffError("refused", f"the {'cameras' if layers is None else 'layers'} file alone: the layers and the cameras "
                                      "file belong together, and a band is read from both")
    rl = GeoTiffReader(layers, ctx=ctx, budget=budget)
    try:
        rc = GeoTiffReader(cameras, ctx=ctx, budget=budget)
    except BaseException:
        rl.close()
        raise
    try:
        # one layer of colours is four Byte samples, which is RGBA8's layout too
        nl = rl.num_layers if rl.kind == GEOTIFF_LAYERS8 else 1 if rl.kind == OVERVIEW_RGBA8 else None
        if nl is None:
            raise GeoTiffError("refused", "the layers file holds no B G R A layers: 4 Byte samples a layer")
        if rc.kind != GEOTIFF_CAMERAS32:
            raise GeoTiffError("refused", "the cameras file holds no node ids: 2 UInt32 samples a layer")
        if (rl.width, rl.height) != (rc.width, rc.height):
            raise GeoTiffError("refused", f"the layers file is {rl.width} x {rl.height}, the cameras file {rc.width} x {rc.height}")
        if nl != rc.num_layers:
            raise GeoTiffError("refused", f"the layers file has {nl} layers, the cameras file {rc.num_layers}")
        if rl.geo != rc.geo or rl.projection != rc.projection:
            raise GeoTiffError("refused", f"the geo tags of the layers file, {rl.geo}, are not the cameras file's, {rc.geo}")
    except BaseException:
        rl.close()
        rc.close()
        raise
    return rl, rc, nl


def _read_layer_band(rl, rc, nl, row0, rows, on_device):
    bgra = rl.read(row0, rows, on_device=on_device)
    if rl.kind == OVERVIEW_RGBA8:
        bgra = bgra.reshape((1,) + tuple(bgra.shape))
    return dict(bgra=bgra, camera_id=rc.read(row0, rows, on_device=on_device), row0=int(row0), rows=int(bgra.shape[1]))


def read_layer_files(layers, cameras=None, row0=0, rows=None, ctx=None, on_device=False):
    """Rows [row0, row0 + rows) of the two rasters generateLayeredGeoTIFF leaves (GeoTiffWriter's kinds GEOTIFF_LAYERS8 and
    GEOTIFF_CAMERAS32) as ortho_blend takes its `layers`: dict(bgra (L, rows, width, 4) uint8, camera_id
    (L, rows, width) uint64 - int64 in a CUDA tensor -, row0, rows).  layers, cameras: what GeoTiffReader takes.  ctx None: the
    host route; else through ctx's device, where the band stays with on_device.  One file of the pair alone (the other None or
    left out), two files of different size, layer count or geo tags, and a file of another layout in either place, raise
    GeoTiffError("refused")."""
    rl, rc, nl = _open_layer_files(layers, cameras, ctx)
    try:
        return _read_layer_band(rl, rc, nl, row0, rows, on_device)
    finally:
        rl.close()
        rc.close()


def save_textured_obj_from_geotiff(path, surfaces, geotiff, jpeg=True, ctx=None, quality=95):
    """generateTexturedOBJ(surfaces, geotiff_path, obj_path) (src/ortho/ortho.cpp:2052-2123): save_textured_obj with the
    orthomosaic read from its file - `geotiff`: what GeoTiffReader takes - the geometry from the file's geotransform (gsd_x
    and gsd_y as there) and the texture from the first min(samples, 3) samples.  With ctx the pixels go from the reader to
    the JPEG encoder without leaving the device."""
    with GeoTiffReader(geotiff, ctx=ctx) as rd:
        if rd.geo is None:
            raise GeoTiffError("unsupported", "the file has no geotransform (tags 33550 and 33922)")
        if rd.is_float:
            raise GeoTiffError("unsupported", "a float32 raster is not a texture")
        g = rd.geo
        geometry = (rd.width, rd.height, g["min_x"], g["max_y"], g["gsd_x"], g["gsd_y"])
        raster = rd.read(on_device=ctx is not None and bool(jpeg))
    if raster.shape[2] == 1:
        raster = raster.expand(-1, -1, 3).contiguous() if hasattr(raster, "is_cuda") else np.repeat(raster, 3, axis=2)
    return _save_textured_obj(path, surfaces, raster, geometry, geometry[0], geometry[1], jpeg, ctx, quality)


# ---- the PNG codec (include/oc_host.h) ---------------------------------------------------------------------
PNG_OK, PNG_UNSUPPORTED, PNG_CORRUPT = 0, 1, 2
PNG_MAX_BATCH = 65535


class PngFileInfo(C.Structure):
    """include/oc_host.h: och_png_file_info"""
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("bit_depth", C.c_int32), ("color_type", C.c_int32),
                ("interlace", C.c_int32), ("channels", C.c_int32), ("status", C.c_int32)]


class PngError(ValueError):
    """A PNG the decoder does not give a picture for; status is PNG_UNSUPPORTED (the caller falls back) or PNG_CORRUPT"""

    def __init__(self, status, text):
        super().__init__(text)
        self.status = status


def _png_image(raster, bgr, device):
    """(PngImage, what keeps its pixels alive, on_device) of a (h, w), (h, w, 1), (h, w, 3) or (h, w, 4) uint8 array or CUDA
    tensor; refused before any work"""
    on_device = not isinstance(raster, np.ndarray)
    if on_device:
        import torch

        if not isinstance(raster, torch.Tensor) or not raster.is_cuda or raster.dtype != torch.uint8:
            raise ValueError("an image is a uint8 numpy array or a uint8 CUDA tensor")
        if device is None or raster.device.index != device:
            raise ValueError("a CUDA tensor needs the context of its device")
        keep = raster.contiguous()
        ptr = keep.data_ptr()
    else:
        if raster.dtype != np.uint8:
            raise ValueError(f"an image is uint8, not {raster.dtype}")
        keep = np.ascontiguousarray(raster)
        ptr = keep.ctypes.data
    shape = tuple(int(v) for v in keep.shape)
    if len(shape) == 2:
        shape = shape + (1,)
    if len(shape) != 3 or shape[2] not in (1, 3, 4) or not 1 <= shape[0] <= 65535 or not 1 <= shape[1] <= 65535:
        raise ValueError(f"an image is (h, w), (h, w, 1), (h, w, 3) or (h, w, 4) with sides of 1 .. 65535, not {tuple(raster.shape)}")
    return capi.PngImage(ptr, shape[1], shape[0], shape[2], int(bool(bgr))), keep, on_device


class PngEncoder(_Handle):
    """PNG files of batches of images (och_png_encoder_*; the rules: DESIGN.md §4.20).  ctx None: the CPU route; ctx: the
    device route, numpy arrays through the device or CUDA tensors on ctx's device (torch's work on them finished).  Both
    give the same bytes.  encode(images, bgr=False, base64=False): a list of uint8 (h, w), (h, w, 3) or (h, w, 4) images of
    any sizes, at most 65 535 - all numpy or all CUDA - to a list of bytes, or of str with base64; bgr: the arrays are
    B G R (A), the files R G B (A)."""

    _destroy, _last_error = "och_png_encoder_destroy", "och_png_last_error"

    def __init__(self, ctx=None):
        self.L, self.ctx, self.h = load(), ctx, None
        h = C.c_void_p()
        self._check(self.L.och_png_encoder_create(ctx.h if ctx is not None else None, C.byref(h)))
        self.h = h

    def encode(self, images, bgr=False, base64=False, cap=None):
        images = list(images)
        if len(images) > PNG_MAX_BATCH:
            raise ValueError(f"a batch of {len(images)} images, at most {PNG_MAX_BATCH} are taken")
        device = None if self.ctx is None else self.ctx.device
        recs = [_png_image(m, bgr, device) for m in images]
        if not recs:
            return []
        if len({r[2] for r in recs}) != 1:
            raise ValueError("a batch is all numpy arrays or all CUDA tensors")
        on_device = recs[0][2]
        if on_device:
            import torch

            torch.cuda.current_stream(recs[0][1].device).synchronize()  # the kernels run on the context's own stream
        arr = (capi.PngImage * len(recs))(*[r[0] for r in recs])
        need = 0
        for r in recs:
            bound = int(self.L.och_png_bound(r[0].width, r[0].height, r[0].channels, int(bool(base64))))
            if bound == 0:
                raise ValueError(f"an image of {r[0].width} x {r[0].height} x {r[0].channels} has a payload of 2^31 bytes or more")
            need += bound
        out = np.empty(max(need if cap is None else int(cap), 1), np.uint8)
        offsets = np.zeros(len(recs) + 1, np.uint64)
        self._check(self.L.och_png_encoder_encode(self.h, len(recs), arr, int(on_device), int(bool(base64)), out.ctypes.data,
                                                  out.size if cap is None else int(cap), offsets.ctypes.data))
        files = [out[int(offsets[i]):int(offsets[i + 1])].tobytes() for i in range(len(recs))]
        return [f.decode("ascii") for f in files] if base64 else files


def encode_png(raster, ctx=None, bgr=False):
    """The PNG file of one image (PngEncoder in one call)"""
    with PngEncoder(ctx) as e:
        return e.encode([raster], bgr=bgr)[0]


def save_png(target, raster, ctx=None, bgr=False):
    """encode_png into a path or a binary file object; the runner's thumb.png is save_png(path,
    orthomosaic_thumbnail(...)["rgba"]) (DESIGN.md §4.20 on the channel order)"""
    data = encode_png(raster, ctx=ctx, bgr=bgr)
    if hasattr(target, "write"):
        target.write(data)
    else:
        with open(target, "wb") as f:
            f.write(data)
    return len(data)


def png_filter(raster, bgr=False):
    """The filtered payload of an image, h rows of the filter type and w * c bytes: what the file's stream inflates to"""
    rec, keep, on_device = _png_image(raster, bgr, None)
    if on_device:
        raise ValueError("png_filter takes a numpy array")
    out = np.empty(rec.height * (1 + rec.width * rec.channels), np.uint8)
    L = load()
    if L.och_png_filter(C.byref(rec), out.ctypes.data, out.size) != 0:
        raise capi.OchipError(L.och_png_last_error().decode())
    return out


def _png_info_dict(rec):
    return dict(width=int(rec.width), height=int(rec.height), bit_depth=int(rec.bit_depth), color_type=int(rec.color_type),
                interlace=int(rec.interlace), channels=int(rec.channels), status=int(rec.status))


def png_info(data):
    """The signature and IHDR of a PNG file: a dict with width, height, bit_depth, color_type, interlace, channels and status
    (PNG_OK: decode_png takes it, PNG_UNSUPPORTED, PNG_CORRUPT)"""
    raw = bytes(data) if data is not None else b""
    rec = PngFileInfo()
    load().och_png_info(raw if raw else None, len(raw), C.byref(rec))
    return _png_info_dict(rec)


def decode_png(data):
    """The picture of a PNG file, (h, w) or (h, w, c) uint8 in the file's channels (host code only).  PngError with the
    status for a file that is not taken: never a wrong or a partial picture."""
    raw = bytes(data) if data is not None else b""
    L = load()
    rec, px = PngFileInfo(), C.c_void_p()
    if L.och_png_decode(raw if raw else None, len(raw), C.byref(rec), C.byref(px)) != 0:
        raise capi.OchipError(L.och_png_last_error().decode())
    if rec.status != PNG_OK:
        raise PngError(int(rec.status), "an unsupported PNG file (palette, 16 bits, fewer than 8 bits or interlaced)"
                       if rec.status == PNG_UNSUPPORTED else "a corrupt PNG file")
    try:
        n = rec.height * rec.width * rec.channels
        out = np.ctypeslib.as_array(C.cast(px, C.POINTER(C.c_uint8)), (n,)).copy()
    finally:
        L.och_png_free(px)
    return out.reshape(rec.height, rec.width) if rec.channels == 1 else out.reshape(rec.height, rec.width, rec.channels)


def blend_chamfer(boundary):
    """The sequential two-pass 3 x 3 chamfer of a boundary mask, int32 in 1e-4 units."""
    m = np.ascontiguousarray(boundary, np.uint8)
    d = np.zeros(m.shape, np.int32)
    load().och_blend_chamfer(m.shape[0], m.shape[1], m.ctypes.data, d.ctypes.data)
    return d


def blend_pyr(image, up=False, size=None):
    """pyrDown (to ((w + 1) / 2, (h + 1) / 2)) or pyrUp (to size = (H, W)) of a float32 (h, w) or (h, w, 3) image as the
    blend defines them."""
    src = np.ascontiguousarray(image, np.float32)
    h, w = src.shape[:2]
    ch = 1 if src.ndim == 2 else src.shape[2]
    H, W = size if up else ((h + 1) // 2, (w + 1) // 2)
    out = np.zeros((H, W) + src.shape[2:], np.float32)
    load().och_blend_pyr(int(up), ch, w, h, W, H, src.ctypes.data, out.ctypes.data)
    return out


def blend_math(values, mode):
    """The blend's restated functions: mode "exp" (float32 -> float32), "falloff" (N x 2 (steepness, d) -> float32) or
    "lab2bgr8" (N x 3 float Lab -> uint8 BGR)."""
    m = {"exp": 0, "falloff": 1, "lab2bgr8": 2}[mode]
    v = np.ascontiguousarray(values, np.float32)
    n = v.size if m == 0 else v.size // (2 if m == 1 else 3)
    out = np.zeros((n, 3), np.uint8) if m == 2 else np.zeros(n, np.float32)
    load().och_blend_math(m, n, v.ctypes.data, out.ctypes.data)
    return out


def ortho_patch_sample(cam28, image, gsd, xyz):
    """PatchSampler::sampleWithJacobian (src/ortho/ortho.cpp:117-213) of one camera record (ortho_layers_cameras) at a
    world point: (bgr or None, pixel, J)."""
    img = np.ascontiguousarray(image, np.uint8)
    cam = np.ascontiguousarray(cam28, np.float64)
    if img.shape != (int(cam[21]), int(cam[20]), 3):
        raise ValueError("the image must be the model's pixels_rows x pixels_cols x 3")
    xyz = np.ascontiguousarray(xyz, np.float64)
    bgr, pixel, J = np.zeros(3, np.uint8), np.zeros(2), np.zeros(4)
    ok = load().och_ortho_patch_sample(cam.ctypes.data, img.ctypes.data, float(gsd), xyz.ctypes.data, bgr.ctypes.data,
                                       pixel.ctypes.data, J.ctypes.data)
    return (bgr if ok else None), pixel, J.reshape(2, 2)


def ortho_sample_fields(pixel_x, pixel_y, width, height, camera_distance, cos_view=1.0):
    """normalizedImageRadius, normalizedImagePosition, computeBlendWeight and the view angle as the layered render
    computes them: float32 (radius, x, y, weight, angle)."""
    out = np.zeros(5, np.float32)
    load().och_ortho_sample_fields(float(pixel_x), float(pixel_y), int(width), int(height), float(camera_distance),
                                   float(cos_view), out.ctypes.data)
    return out


def relax(ctx, node_pos, node_ori, model10, features, pose_node, pose_ori, packed_edges, options, grid_fraction=0.1,
          opt_edges=None, previous=None, cam_model=None, edge_poses=None, points_mode=-1):
    """relax(graph, nodes, cam_models, edges, config, previousSurfaces) on the device, any flavour.  features: per node
    an (k x 2) array of feature locations; packed_edges as for relax_ground_plane plus 'feat' (inliers x 2 feature
    indices).  edge_poses (n_edges x 4 x 8): the edges' homography decompositions (relative-orientation flavour);
    points_mode 0 / 1 / 2 with POINTS_3D: set up the 3-D point problem and leave it / solve it / run
    relaxObservedModelOnly, returning the points before and after (test/test_relax.cpp:470-483)."""
    L = load()
    node_pos = np.ascontiguousarray(node_pos, np.float64)
    node_ori = np.ascontiguousarray(node_ori, np.float64)
    pose_node = np.ascontiguousarray(pose_node, np.uint64)
    pose_ori = np.ascontiguousarray(pose_ori, np.float64).copy()
    feat_off = np.concatenate([[0], np.cumsum([len(f) for f in features])]).astype(np.uint64)
    feat_xy = np.ascontiguousarray(np.concatenate([np.asarray(f, np.float64).reshape(-1, 2) for f in features])
                                   if feat_off[-1] else np.zeros((1, 2)))
    pk = packed_edges
    n_edges = len(pk["src"])
    opt = np.ascontiguousarray(np.arange(n_edges) if opt_edges is None else opt_edges, np.uint64)
    summary = np.zeros(12)
    out_surface = Surface()
    cm = np.ascontiguousarray(model10 if cam_model is None else cam_model, np.float64).copy()
    ep = None if edge_poses is None else np.ascontiguousarray(edge_poses, np.float64).reshape(-1, 32)
    cap = 1 << 20
    before = after = None
    n_pts = C.c_size_t(0)
    if points_mode >= 0:
        before, after = np.zeros((cap, 3)), np.zeros((cap, 3))
    rc = L.och_relax_ex(ctx.h, len(node_pos), node_pos, node_ori, np.ascontiguousarray(model10, np.float64), feat_off, feat_xy,
                        len(pose_node), pose_node, pose_ori, n_edges, pk["src"], pk["dst"], pk["H"].ctypes.data, pk["is_h"],
                        pk["inl_off"], pk["px"], np.ascontiguousarray(pk["feat"], np.uint64), pk["match_index"],
                        pk["dist_off"].ctypes.data, pk["dist"].ctypes.data, len(opt), opt if len(opt) else np.zeros(1, np.uint64),
                        options, grid_fraction, previous.h if previous is not None else None, out_surface.h, summary,
                        cm.ctypes.data, None if ep is None else ep.ctypes.data, points_mode,
                        None if before is None else before.ctypes.data, None if after is None else after.ctypes.data,
                        cap if before is not None else 0, C.byref(n_pts))
    if rc != 0:
        raise capi.OchipError("relax failed: " + L.och_relax_last_error().decode())
    out = dict(zip(RELAX_SUMMARY12, summary.tolist()))
    out.update(orientation=pose_ori, surface=out_surface, cam_model=cm)
    if before is not None:
        out.update(points_before=before[:n_pts.value].copy(), points_after=after[:n_pts.value].copy())
    for k in ("solves", "iterations_total", "last_iterations", "residual_blocks", "track_blocks", "two_ray_blocks",
              "mesh_vertices", "unknowns"):
        out[k] = int(out[k])
    return out


def relax_setup_check(on=-1):
    """Test hook (och_debug_relax_setup_check): on=1 makes every ground-plane relax set-up also run the host's grid filter
    and block assembly and fail unless the device's blocks equal them bit for bit.  Returns the set-ups compared so far."""
    return int(load().och_debug_relax_setup_check(int(on)))


def relax_ground_plane(ctx, node_pos, node_ori, model10, pose_node, pose_ori, packed_edges, opt_edges=None):
    """relax(graph, nodes, cam_models, edges, {ORIENTATION, GROUND_PLANE}, {}) on the device.  `packed_edges` is
    the dict of flat arrays (src, dst, H, is_h, inl_off, px, match_index, dist_off, dist)."""
    L = load()
    node_pos = np.ascontiguousarray(node_pos, np.float64)
    node_ori = np.ascontiguousarray(node_ori, np.float64)
    pose_node = np.ascontiguousarray(pose_node, np.uint64)
    pose_ori = np.ascontiguousarray(pose_ori, np.float64).copy()
    pk = packed_edges
    n_edges = len(pk["src"])
    opt = np.ascontiguousarray(np.arange(n_edges) if opt_edges is None else opt_edges, np.uint64)
    plane, summary = np.zeros(9), np.zeros(8)
    rc = L.och_relax_ground_plane(ctx.h, len(node_pos), node_pos, node_ori, np.ascontiguousarray(model10, np.float64),
                                  len(pose_node), pose_node, pose_ori, n_edges, pk["src"], pk["dst"], pk["H"], pk["is_h"],
                                  pk["inl_off"], pk["px"], pk["match_index"], pk["dist_off"].ctypes.data,
                                  pk["dist"].ctypes.data, len(opt), opt, plane, summary)
    if rc != 0:
        raise capi.OchipError("relax failed: " + L.och_relax_last_error().decode())
    out = dict(zip(RELAX_SUMMARY_NAMES, summary.tolist()))
    out.update(orientation=pose_ori, plane=plane.reshape(3, 3))
    for k in ("solves", "iterations_total", "last_iterations", "residual_blocks"):
        out[k] = int(out[k])
    return out


LINK_TIMER_NAMES = ["link_init", "subsample", "upload", "match_device", "match_host", "ransac_device",
                    "decompose_host", "link_finalize"]


class Graph:
    """MeasurementGraph + stage drivers (opencalibration_amd/csrc/host)."""

    def __init__(self):
        self.L = load()
        self.h = C.c_void_p(self.L.och_graph_create())
        self.node_ids = []
        self.geo = None             # the local frame's GeoCoord once load_survey (or the caller) has set one
        self._survey_cameras = {}   # load_survey: camera_info -> model index

    def close(self):
        if getattr(self, "h", None):
            self.L.och_graph_destroy(self.h)
            self.h = None

    # ---- graph.json (src/io/serialize_MeasurementGraph.cpp, src/io/deserialize_MeasurementGraph.cpp)
    def to_json(self):
        n = C.c_size_t(0)
        ptr = self.L.och_graph_to_json(self.h, C.byref(n))
        if not ptr:
            raise MemoryError("serialize failed")
        try:
            return C.string_at(ptr, n.value).decode("utf-8")
        finally:
            self.L.och_free(ptr)

    def _refresh_ids(self):
        ids = np.zeros(max(self.L.och_graph_num_nodes(self.h), 1), np.uint64)
        self.L.och_graph_node_ids(self.h, ids)
        self.node_ids = [int(i) for i in ids[:self.L.och_graph_num_nodes(self.h)]]

    def from_json(self, text):
        """deserialize(json, graph): replaces this graph.  Raises ValueError on anything but a version-1 document."""
        raw = text.encode("utf-8") if isinstance(text, str) else bytes(text)
        if self.L.och_graph_from_json(self.h, raw, len(raw)) != 0:
            raise ValueError(self.L.och_last_error(self.h).decode())
        self._refresh_ids()
        return self

    def save_json(self, path):
        if self.L.och_graph_save_json(self.h, str(path).encode()) != 0:
            raise IOError(self.L.och_last_error(self.h).decode())

    def load_json(self, path):
        if self.L.och_graph_load_json(self.h, str(path).encode()) != 0:
            raise ValueError(self.L.och_last_error(self.h).decode())
        self._refresh_ids()
        return self

    def densify_mesh(self, ctx, surface, want_matches=False, match_cap=1 << 22):
        """densifyMesh (src/dense/dense_stereo.cpp:66-403): dense guided matching on the device against `surface`'s mesh;
        the triangulated points become one more cloud of `surface`.  Returns the stats (and the accepted matches)."""
        stats = np.zeros(10)
        pairs = np.zeros((match_cap if want_matches else 1, 2), np.uint64)
        rc = self.L.och_densify_mesh(self.h, ctx.h, surface.h, stats, pairs.ctypes.data if want_matches else None,
                                     match_cap if want_matches else 0)
        if rc != 0:
            raise capi.OchipError("densify failed: " + self.L.och_last_error(self.h).decode())
        names = ["images", "dense_features", "queries", "matches", "tracks", "points", "index_s", "rays_s", "device_s", "tracks_s"]
        out = dict(zip(names, stats.tolist()))
        for k in names[:6]:
            out[k] = int(out[k])
        if want_matches:
            out["match_pairs"] = pairs[:min(out["matches"], match_cap)].copy()
        return out

    def mesh_refinement(self, ctx, surface=None, max_steps=40):
        """The pipeline's MESH_REFINEMENT state (src/pipeline/pipeline.cpp:666-819) run to its end: returns (surface, log)."""
        surface = Surface() if surface is None else surface
        log = np.zeros((max_steps, 8))
        n = self.L.och_mesh_refinement_run(self.h, ctx.h, surface.h, max_steps, log)
        if n < 0:
            raise capi.OchipError("mesh refinement failed: " + self.L.och_last_error(self.h).decode())
        names = ["level", "grid_fraction", "gsd", "above_threshold", "max_points", "created", "vertices", "repeat"]
        return surface, [dict(zip(names, row)) for row in log[:n].tolist()]

    def dense_mesh_relax(self, surface, ctx=None, max_steps=40):
        """The pipeline's DENSE_MESH_RELAX state (src/pipeline/pipeline.cpp:844-924) run to its end on `surface` (mesh +
        the dense cloud): refine by point density at the gsd's thresholds until nothing is created, at most 21 runs.  ctx:
        the points are counted on the device (the cloud uploaded once), else on the host.  Returns (surface, log)."""
        log = np.zeros((max(max_steps, 1), 6))
        n = self.L.och_dense_mesh_relax_run(self.h, ctx.h if ctx is not None else None, surface.h, max_steps, log)
        if n < 0:
            raise capi.OchipError("dense mesh relax failed: " + self.L.och_last_error(self.h).decode())
        names = ["run", "gsd", "reduced_gsd", "above_threshold", "created", "vertices"]
        return surface, [dict(zip(names, row)) for row in log[:n].tolist()]

    def node_table(self):
        """Per node in graph order: id, index into models(), number of features, number of sparse features."""
        n = self.L.och_graph_num_nodes(self.h)
        ids, mi = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32)
        nf, ns = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint64)
        self.L.och_graph_node_table(self.h, ids.ctypes.data, mi.ctypes.data, nf.ctypes.data, ns.ctypes.data)
        return dict(id=ids[:n], model=mi[:n], features=nf[:n], sparse=ns[:n])

    def node_payload(self, index):
        """Features (loc, strength, desc), position, orientation and path of the index-th node."""
        n = int(self.node_table()["features"][index])
        loc, st, de = np.zeros((max(n, 1), 2)), np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 8), np.uint64)
        pos, ori = np.zeros(3), np.zeros(4)
        self.L.och_graph_node_payload(self.h, index, loc.ctypes.data, st.ctypes.data, de.ctypes.data, pos.ctypes.data,
                                      ori.ctypes.data)
        return dict(loc=loc[:n], strength=st[:n], desc=de[:n], position=pos, orientation=ori,
                    path=self.L.och_graph_node_path(self.h, index).decode("utf-8"))

    def set_node_path(self, index, path):
        self.L.och_graph_set_node_path(self.h, index, path.encode("utf-8"))

    def models(self):
        """The graph's camera models: rows of och_graph_add_model's ten numbers followed by the model id."""
        out = np.zeros((self.L.och_graph_num_models(self.h), 11))
        for i in range(len(out)):
            self.L.och_graph_get_model(self.h, i, out[i])
        return out

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_model(self, model10):
        return self.L.och_graph_add_model(self.h, np.ascontiguousarray(model10, np.float64))

    def set_model(self, model, model10):
        """Replace the intrinsics of camera model `model` (what a relax with free intrinsics writes back)."""
        if self.L.och_graph_set_model(self.h, int(model), np.ascontiguousarray(model10, np.float64)) != 0:
            raise capi.OchipError("och_graph_set_model: bad model index")

    def refit_edges(self, ctx):
        """RelaxGroup::finalize's edge loop after a model change (relax_group.cpp:137-177): every edge re-fitted on its
        previous inliers with the current camera models."""
        if self.L.och_graph_refit_edges(self.h, ctx.h) != 0:
            raise capi.OchipError("refit failed: " + self.L.och_last_error(self.h).decode())

    def add_image(self, loc, strength, desc, num_sparse, model, position):
        nid = self.L.och_graph_add_image(self.h, np.ascontiguousarray(loc, np.float64),
                                         np.ascontiguousarray(strength, np.float32),
                                         np.ascontiguousarray(desc, np.uint64), len(strength), int(num_sparse), model,
                                         np.ascontiguousarray(position, np.float64))
        self.node_ids.append(nid)
        return nid

    def make_thumbnails(self, images_bgr, node_ids, ctx=None, device_shape=None):
        """image_thumbnails of the batch, stored on the nodes `node_ids` (one id per image) for the orthomosaic preview."""
        keep, src, n, h, w, on_dev = _image_batch(images_bgr, device_shape)
        ids = np.ascontiguousarray(node_ids, np.uint64).reshape(-1)
        if len(ids) != n:
            raise ValueError("one node id per image")
        ids = ids if n else np.zeros(1, np.uint64)
        if self.L.och_graph_make_thumbnails(self.h, ctx.h if ctx is not None else None, src, n, w, h, on_dev, ids) != 0:
            raise capi.OchipError("make_thumbnails failed: " + self.L.och_last_error(self.h).decode())
        del keep

    def load_images(self, ctx, images_bgr, model, positions, max_keypoints=30000, device_shape=None, thumbnails=False):
        """The load stage for a batch of equally sized images: extract_features on the device, one node per image.
        images_bgr: (n, h, w, 3) uint8 host array or, with device_shape=(n, h, w), a device pointer.  thumbnails=True:
        the same buffer's thumbnails (make_thumbnails, on the device) go onto the new nodes after the extraction.  Returns
        (mean features per image, mean sparse features per image)."""
        if device_shape is None:
            imgs = np.ascontiguousarray(images_bgr, np.uint8)
            n, h, w, _ = imgs.shape
            src, on_dev = imgs.ctypes.data, 0
        else:
            n, h, w = device_shape
            src, on_dev = int(images_bgr), 1
        ids, totals = np.zeros(max(n, 1), np.uint64), np.zeros(2)
        rc = self.L.och_graph_load_images(self.h, ctx.h, src, n, w, h, max_keypoints, on_dev, model,
                                          np.ascontiguousarray(positions, np.float64).reshape(-1, 3), ids, totals)
        if rc != 0:
            raise capi.OchipError("load_images failed: " + self.L.och_last_error(self.h).decode())
        self.node_ids += [int(i) for i in ids[:n]]
        if thumbnails:
            self.make_thumbnails(images_bgr, ids[:n], ctx, device_shape)
        return totals[0] / max(n, 1), totals[1] / max(n, 1)

    def load_jpegs(self, ctx, files, model, positions, max_keypoints=30000, thumbnails=False, chunk=None):
        """load_images from JPEG files (bytes objects or paths), all of one decoded size: decoded on ctx's device in chunks
        of `chunk` images (None: as many as JPEG_LOAD_PIXEL_BUDGET pixels hold) and extracted from the same buffer, which
        also gives the thumbnails.  A file the decoder refuses raises OchipError naming the file and its status before
        anything of its chunk is loaded.  Returns load_images' means over all files."""
        files = list(files)
        n = len(files)
        pos = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        if len(pos) != n:
            raise ValueError("one position per file")

        def name(i):
            return f"file {i}" if isinstance(files[i], (bytes, bytearray, memoryview)) else f"file {i} ({os.fspath(files[i])})"

        import torch

        shape, at, sums, pixels = None, 0, np.zeros(2), None
        with JpegDecoder(ctx) as dec:
            while at < n:
                if shape is None:
                    first = jpeg_info(files[at])
                    if first["status"] != "ok":
                        raise capi.OchipError(f"load_jpegs: {name(at)} is {first['status']}")
                    shape = (first["height"], first["width"])
                step = int(chunk) if chunk else max(1, JPEG_LOAD_PIXEL_BUDGET // (shape[0] * shape[1]))
                m = min(step, n - at)
                if pixels is None or pixels.numel() < m * shape[0] * shape[1] * 3:
                    pixels = torch.empty(m * shape[0] * shape[1] * 3, dtype=torch.uint8, device=f"cuda:{ctx.device}")
                    torch.cuda.current_stream(pixels.device).synchronize()
                try:
                    batch = dec.decode(files[at:at + step], out=pixels)  # one pass over each file's bytes
                except capi.OchipError as e:
                    if "the output holds" not in str(e):
                        raise
                    batch = dec.decode(files[at:at + step])  # a file of another size: decoded apart so it can be named
                m = len(batch.status)
                for i in range(m):
                    if batch.status[i] != "ok":
                        raise capi.OchipError(f"load_jpegs: {name(at + i)} is {batch.status[i]}")
                    if batch.shapes[i] != shape:
                        raise capi.OchipError(f"load_jpegs: {name(at + i)} is {batch.shapes[i][1]} x {batch.shapes[i][0]}, "
                                              f"the first file {shape[1]} x {shape[0]}")
                f, s = self.load_images(ctx, batch.pixels.data_ptr(), model, pos[at:at + m], max_keypoints,
                                        device_shape=(m, shape[0], shape[1]), thumbnails=thumbnails)
                sums += (f * m, s * m)
                del batch
                at += m
        return sums[0] / max(n, 1), sums[1] / max(n, 1)

    def load_survey(self, ctx, files, max_keypoints=30000, thumbnails=False, chunk=None, geo=None):
        """The load stage from JPEG files alone (bytes objects or paths): each file's jpeg_metadata gives
        its camera and its position.  The local frame is `geo` (a GeoCoord or an (lat, lon) origin), else graph.geo, else
        one about the first file's position (load_stage.cpp:71-74), and is kept as graph.geo.  Files whose camera_info
        compare equal (size, make, model, serial number, lens, focal length) share one model: focal length and size from
        the metadata, the principal point at (cols, rows) / 2, no distortion.  Positions are geo.to_local of latitude,
        longitude and altitude.  Decode and extraction are load_jpegs', one call per run of consecutive files of one model;
        each node gets its file's path (when it was one) and its metadata.  A file without latitude / longitude, without a
        focal length, with a metadata size of 0 or one that differs from the decoded (oriented) size, or one the decoder
        does not call "ok" raises OchipError naming it before anything is launched or the graph is touched.  Returns
        load_jpegs' means."""
        files = list(files)
        blobs = [_jpeg_bytes(f) for f in files]

        def name(i):
            return f"file {i}" if isinstance(files[i], (bytes, bytearray, memoryview)) else f"file {i} ({os.fspath(files[i])})"

        metas = []
        for i, blob in enumerate(blobs):
            md = jpeg_metadata(blob)
            cam, cap = md["camera_info"], md["capture_info"]
            if not (np.isfinite(cap["latitude"]) and np.isfinite(cap["longitude"])):
                raise capi.OchipError(f"load_survey: {name(i)} has no latitude / longitude")
            if not np.isfinite(cam["focal_length_px"]):
                raise capi.OchipError(f"load_survey: {name(i)} has no focal length")
            w, h = cam["dimensions"]
            if w == 0 or h == 0:
                raise capi.OchipError(f"load_survey: {name(i)} has no image size in its metadata")
            info = jpeg_info(blob)
            if info["status"] != "ok":
                raise capi.OchipError(f"load_survey: {name(i)} is {info['status']}")
            if (info["width"], info["height"]) != (w, h):
                raise capi.OchipError(f"load_survey: {name(i)} decodes to {info['width']} x {info['height']}, its metadata says "
                                      f"{w} x {h}")
            metas.append(md)
        if ctx is None:
            raise capi.OchipError("load_survey: the extraction needs a device context")
        geo = _geo_coord(geo) or self.geo
        if geo is None and metas:
            geo = GeoCoord(metas[0]["capture_info"]["latitude"], metas[0]["capture_info"]["longitude"])
        self.geo = geo

        def camera_key(cam):  # camera_info_t::operator== (types/image_metadata.hpp:22-35): the principal point is not in it
            return (tuple(cam["dimensions"]), cam["make"], cam["model"], cam["serial_no"], cam["lens_make"], cam["lens_model"],
                    cam["focal_length_px"])

        models = []
        for md in metas:
            cam = md["camera_info"]
            key = camera_key(cam)
            if key not in self._survey_cameras:
                w, h = cam["dimensions"]
                self._survey_cameras[key] = self.add_model([cam["focal_length_px"], w / 2, h / 2, 0, 0, 0, 0, 0, w, h])
            models.append(self._survey_cameras[key])
        cap = [md["capture_info"] for md in metas]
        pos = geo.to_local([c["latitude"] for c in cap], [c["longitude"] for c in cap], [c["altitude"] for c in cap]) \
            if metas else np.zeros((0, 3))
        at, sums, n = 0, np.zeros(2), len(files)
        while at < n:
            end = at + 1
            while end < n and models[end] == models[at]:
                end += 1
            first = self.num_nodes
            f, s = self.load_jpegs(ctx, blobs[at:end], models[at], pos[at:end], max_keypoints, thumbnails, chunk)
            sums += (f * (end - at), s * (end - at))
            for i in range(at, end):
                if not isinstance(files[i], (bytes, bytearray, memoryview)):
                    self.set_node_path(first + i - at, os.fspath(files[i]))
                self.set_node_metadata(first + i - at, metas[i])
            at = end
        return sums[0] / max(n, 1), sums[1] / max(n, 1)

    def set_node_metadata(self, index, metadata):
        """The "metadata" object of the index-th node in graph.json: a dict (jpeg_metadata's) or JSON text."""
        import json

        text = metadata if isinstance(metadata, str) else json.dumps(metadata)
        raw = text.encode("utf-8")
        if self.L.och_graph_set_node_metadata(self.h, int(index), raw, len(raw)) != 0:
            raise ValueError(self.L.och_last_error(self.h).decode())

    def node_metadata(self, index):
        """The index-th node's metadata as a dict (NaN for absent numbers), or None where the node carries none."""
        import json

        text = self.L.och_graph_node_metadata(self.h, int(index)).decode("utf-8")
        return json.loads(text) if text else None

    def to_geojson(self, geo=None, node_ids=None, edge_ids=None):
        """toVisualizedGeoJson (src/io/serialize_MeasurementGraph.cpp:62-209): a FeatureCollection of one Point per node,
        then one LineString per edge with its inlier count, coordinates (longitude, latitude, altitude) through `geo` (a
        GeoCoord or an (lat, lon) origin; None: graph.geo, and without one the local coordinates as they are).  node_ids /
        edge_ids: None for all of them sorted by id, else those in the given order."""
        geo = _geo_coord(geo) or self.geo
        nodes = None if node_ids is None else np.ascontiguousarray(node_ids, np.uint64).reshape(-1)
        edges = None if edge_ids is None else np.ascontiguousarray(edge_ids, np.uint64).reshape(-1)
        n = C.c_size_t(0)
        ptr = self.L.och_graph_geojson(self.h, geo.h if geo is not None else None,
                                       None if nodes is None else nodes.ctypes.data, 0 if nodes is None else len(nodes),
                                       None if edges is None else edges.ctypes.data, 0 if edges is None else len(edges), C.byref(n))
        if not ptr:
            raise ValueError(self.L.och_last_error(self.h).decode())
        try:
            return C.string_at(ptr, n.value).decode("utf-8")
        finally:
            self.L.och_free(ptr)

    def load_link_images(self, ctx, images_bgr, model, positions, orientations=None, max_keypoints=30000, device_shape=None):
        """Load and link overlapped (och_graph_load_link_images): extraction streams in chunks and ranges of links run
        on their own device contexts as soon as their images are ready.  Same graph as load_images() + link().
        Returns (mean features per image, mean sparse features per image, link timers, (extract_s, total_s))."""
        if device_shape is None:
            imgs = np.ascontiguousarray(images_bgr, np.uint8)
            n, h, w, _ = imgs.shape
            src, on_dev = imgs.ctypes.data, 0
        else:
            n, h, w = device_shape
            src, on_dev = int(images_bgr), 1
        ids, totals, timers, stage = np.zeros(max(n, 1), np.uint64), np.zeros(2), np.zeros(8), np.zeros(2)
        ori = None if orientations is None else np.ascontiguousarray(orientations, np.float64)
        rc = self.L.och_graph_load_link_images(self.h, ctx.h, src, n, w, h, max_keypoints, on_dev, model,
                                               np.ascontiguousarray(positions, np.float64).reshape(-1, 3),
                                               None if ori is None else ori.ctypes.data, ids, totals, timers, stage)
        if rc != 0:
            raise capi.OchipError("load_link_images failed: " + self.L.och_last_error(self.h).decode())
        self.node_ids += [int(i) for i in ids[:n]]
        return totals[0] / max(n, 1), totals[1] / max(n, 1), dict(zip(LINK_TIMER_NAMES, timers.tolist())), (stage[0], stage[1])

    def initial_processing(self, ctx):
        """Pipeline::Impl::initial_processing's stepper (och_initial_processing_*): see InitialProcessing."""
        return InitialProcessing(self, ctx)

    @classmethod
    def from_synthetic(cls, grid):
        g = cls()
        m = g.add_model(grid.model)
        for i in range(grid.n_images):
            loc, st, de, _ = grid.image(i)
            g.add_image(loc, st, de, grid.num_sparse[i], m, grid.position[i])
        return g

    def add_edge(self, source_id, dest_id, px, f1, f2, match_index=None, H=None, dist=None, poses=None, match_idx=None,
                 is_homography=None):
        """graph.addEdge from arrays: px n x 4 inlier pixels, f1 / f2 feature indices, match distances (and the matches'
        feature index pairs)."""
        px = np.ascontiguousarray(px, np.float64).reshape(-1, 4)
        n = len(px)
        idx = np.zeros((max(n, 1), 3), np.uint64)
        idx[:n, 0], idx[:n, 1] = f1, f2
        idx[:n, 2] = np.arange(n) if match_index is None else match_index
        Hc = None if H is None else np.ascontiguousarray(H, np.float64)
        d = None if dist is None or len(dist) == 0 else np.ascontiguousarray(dist, np.float64)
        pc = None if poses is None else np.ascontiguousarray(poses, np.float64)
        mi2 = None if match_idx is None or d is None else np.ascontiguousarray(match_idx, np.uint64).reshape(-1, 2)
        e = self.L.och_graph_add_edge(self.h, int(source_id), int(dest_id), None if Hc is None else Hc.ctypes.data,
                                      int(H is not None if is_homography is None else is_homography), n,
                                      px if n else np.zeros((1, 4)), idx, 0 if d is None else len(d),
                                      None if mi2 is None else mi2.ctypes.data, None if d is None else d.ctypes.data,
                                      None if pc is None else pc.ctypes.data)
        if e == 0:
            raise capi.OchipError(self.L.och_last_error(self.h).decode())
        return e

    def match_work(self):
        """{pairs, distances needed, subset features} of the last link stage's match step."""
        out = np.zeros(3)
        self.L.och_link_match_work(self.h, out)
        return dict(pairs=out[0], distances=out[1], subset_features=out[2])

    def orientations(self):
        out = np.zeros((max(self.num_nodes, 1), 4))
        self.L.och_graph_get_orientations(self.h, out)
        return out[:self.num_nodes]

    @property
    def num_nodes(self):
        return self.L.och_graph_num_nodes(self.h)

    @property
    def num_edges(self):
        return self.L.och_graph_num_edges(self.h)

    def link(self, ctx, node_ids=None, keep_debug=False):
        """LinkStage init -> runner -> finalize on the device owned by `ctx`; returns the stage timers."""
        ids = np.ascontiguousarray(self.node_ids if node_ids is None else node_ids, np.uint64)
        timers = np.zeros(8)
        rc = self.L.och_link_stage_run(self.h, ctx.h, ids, len(ids), int(keep_debug), timers)
        if rc != 0:
            raise capi.OchipError("link stage failed: " + self.L.och_last_error(self.h).decode())
        return dict(zip(LINK_TIMER_NAMES, timers.tolist()))

    def relax_ground_plane(self, ctx, orientations, shard=None):
        """All nodes as one relax group, every edge whitelisted; updates and returns the orientations.
        shard = (rank, world, exchange): evaluate only this rank's share of the residual blocks; `exchange` is a
        RELAX_EXCHANGE_FN (parallel.relax_exchange builds one on torch.distributed) or a capi.RcclComm created on `ctx`
        (the native transport: RCCL all-gathers on the context's stream), and every rank gets the same, bit-identical
        result."""
        ori = np.ascontiguousarray(orientations, np.float64).copy()
        if ori.shape != (self.num_nodes, 4):
            raise ValueError("orientations must be %d x 4, got %r" % (self.num_nodes, ori.shape))
        plane, summary = np.zeros(9), np.zeros(8)
        if shard is None:
            rc = self.L.och_graph_relax_ground_plane(self.h, ctx.h, ori, plane, summary)
        else:
            rank, world, exchange = shard
            if isinstance(exchange, capi.RcclComm):
                fn, user = exchange.exchange
            else:
                fn, user = C.cast(exchange, C.c_void_p).value, None
            rc = self.L.och_graph_relax_ground_plane_sharded(self.h, ctx.h, ori, plane, summary, rank, world, fn, user)
        if rc != 0:
            raise capi.OchipError("relax failed: " + self.L.och_last_error(self.h).decode())
        out = dict(zip(RELAX_SUMMARY_NAMES, summary.tolist()))
        out.update(orientation=ori, plane=plane.reshape(3, 3))
        return out

    def relax(self, ctx, orientations, options, grid_fraction=0.1, previous=None, shard=None):
        """All nodes as one relax group, every edge whitelisted, any flavour (options: relax_options(...)).
        shard = (rank, world, exchange) as for relax_ground_plane: the residual blocks' evaluation over the ranks."""
        ori = np.ascontiguousarray(orientations, np.float64).copy()
        summary = np.zeros(12)
        surface = Surface()
        prev = previous.h if previous is not None else None
        if shard is None:
            rc = self.L.och_graph_relax(self.h, ctx.h, ori, options, grid_fraction, prev, surface.h, summary)
        else:
            rank, world, exchange = shard
            if isinstance(exchange, capi.RcclComm):
                fn, user = exchange.exchange
            else:
                fn, user = C.cast(exchange, C.c_void_p).value, None
            rc = self.L.och_graph_relax_sharded(self.h, ctx.h, ori, options, grid_fraction, prev, surface.h, summary, rank, world,
                                                fn, user)
        if rc != 0:
            raise capi.OchipError("relax failed: " + self.L.och_last_error(self.h).decode())
        out = dict(zip(RELAX_SUMMARY12, summary.tolist()))
        out.update(orientation=ori, surface=surface)
        return out

    def relax_stage(self, ctx, options, grid_fraction=0.1, node_ids=None, disable_parallelism=False, max_groups=0,
                    previous=None, shard=None):
        """RelaxStage::init + runners + finalize (relax_stage.cpp): node_ids None = relax_all.  Returns the summary, the
        merged surface, the graph's orientations afterwards and the group of every node (-1: not a primary node).
        shard = (rank, world, all_gather): this rank runs groups rank, rank + world, ... and all_gather(bytes) -> list of
        every rank's bytes (parallel.all_gather_bytes) carries the groups' results; every rank ends with the
        single-process result."""
        ids = None if node_ids is None else np.ascontiguousarray(node_ids, np.uint64)
        summary = np.zeros(13)
        groups = np.full(max(self.num_nodes, 1), -1, np.int64)
        surface = Surface()
        if shard is None:
            rc = self.L.och_relax_stage_run(self.h, ctx.h, None if ids is None else ids.ctypes.data, 0 if ids is None else len(ids),
                                            int(ids is None), int(disable_parallelism), options, grid_fraction, max_groups,
                                            previous.h if previous is not None else None, surface.h, groups, summary)
        else:
            rank, world, all_gather = shard
            st = self.L.och_relax_stage_begin(self.h, None if ids is None else ids.ctypes.data, 0 if ids is None else len(ids),
                                              int(ids is None), int(disable_parallelism), options, grid_fraction, max_groups,
                                              previous.h if previous is not None else None, groups)
            if not st:
                raise MemoryError("och_relax_stage_begin")
            self.L.och_relax_stage_run_groups(st, ctx.h, rank, world)
            ptr, n = C.c_void_p(0), C.c_uint64(0)
            self.L.och_relax_stage_export(st, rank, world, C.byref(ptr), C.byref(n))
            mine = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n.value,)) if n.value else np.zeros(0, np.uint8)
            rc = 0
            for r, part in enumerate(all_gather(mine)):
                if r != rank and len(part):
                    part = np.ascontiguousarray(part, np.uint8)
                    rc = rc or self.L.och_relax_stage_import(st, part.ctypes.data, len(part))
            rc = self.L.och_relax_stage_end(st, surface.h, summary) or rc
        if rc != 0:
            raise capi.OchipError("relax stage failed: " + self.L.och_last_error(self.h).decode())
        out = dict(zip(RELAX_SUMMARY12 + ["groups"], summary.tolist()))
        out.update(surface=surface, group_of_node=groups[:self.num_nodes].copy())
        return out

    def relax_partition(self, num_groups, ordered=False):
        """The spectral / k-means partition of RelaxStage::init alone (host only)."""
        groups, pos = np.full(max(self.num_nodes, 1), -1, np.int64), np.full(max(self.num_nodes, 1), -1, np.int64)
        n = self.L.och_relax_partition(self.h, num_groups, groups, pos)
        groups, pos = groups[:self.num_nodes].copy(), pos[:self.num_nodes].copy()
        if ordered:
            return [[int(i) for i in sorted(np.flatnonzero(groups == g), key=lambda i: pos[i])] for g in range(n)]
        return n, groups

    def link_debug(self):
        out = []
        for p in range(self.L.och_link_debug_count(self.h)):
            ids, n, score, it = np.zeros(2, np.uint64), np.zeros(1, np.uint64), np.zeros(1), np.zeros(3, np.uint32)
            self.L.och_link_debug_pair(self.h, p, ids, n, score, it)
            m = max(int(n[0]), 1)
            i1, i2, d, inl = np.zeros(m, np.uint64), np.zeros(m, np.uint64), np.zeros(m), np.zeros(m, np.uint8)
            self.L.och_link_debug_matches(self.h, p, i1, i2, d, inl)
            k = int(n[0])
            out.append(dict(node=int(ids[0]), match_node=int(ids[1]), i1=i1[:k], i2=i2[:k], dist=d[:k], inliers=inl[:k],
                            score=float(score[0]), iterations=int(it[0]), improvements=int(it[1]),
                            can_decompose=bool(it[2])))
        return out

    def edges(self, with_distances=False):
        out = []
        for e in range(self.num_edges):
            ids, cnt, H, poses = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros((3, 3)), np.zeros((4, 8))
            self.L.och_graph_edge_info(self.h, e, ids, cnt, H, poses)
            k = max(int(cnt[1]), 1)
            f1, f2, mi, px = np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros(k, np.uint64), np.zeros((k, 4))
            self.L.och_graph_edge_inliers(self.h, e, f1, f2, mi, px)
            k = int(cnt[1])
            dist = np.zeros(max(int(cnt[0]), 1))
            midx = np.zeros((max(int(cnt[0]), 1), 2), np.uint64)
            is_h = C.c_int(0)
            if with_distances:
                self.L.och_graph_edge_matches(self.h, e, midx.ctypes.data, dist.ctypes.data, C.byref(is_h))
            out.append(dict(source=int(ids[0]), dest=int(ids[1]), n_matches=int(cnt[0]), n_inliers=k, H=H, poses=poses,
                            f1=f1[:k], f2=f2[:k], match_index=mi[:k], px=px[:k], dist=dist[:int(cnt[0])],
                            match_idx=midx[:int(cnt[0])], is_homography=bool(is_h.value)))
        return out

    def set_orientations(self, ori):
        self.L.och_graph_set_orientations(self.h, np.ascontiguousarray(ori, np.float64))

    def set_thumbnail(self, index, rgb):
        """The decoded thumbnail (rows x cols x 3 uint8, layers in the caller's order) of the node at `index` (node
        order) that the orthomosaic preview samples."""
        rgb = np.ascontiguousarray(rgb, np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise ValueError("a thumbnail is rows x cols x 3")
        if self.L.och_graph_set_thumbnail(self.h, int(index), rgb.shape[0], rgb.shape[1], rgb.ctypes.data) != 0:
            raise ValueError(self.L.och_last_error(self.h).decode())

    def thumbnail(self, index):
        """The decoded thumbnail of the node at `index` (rows x cols x 3 uint8), or None where it has none"""
        rows, cols = C.c_size_t(0), C.c_size_t(0)
        if self.L.och_graph_get_thumbnail(self.h, int(index), C.byref(rows), C.byref(cols), None) != 0:
            raise ValueError(self.L.och_last_error(self.h).decode())
        if rows.value == 0:
            return None
        out = np.empty((rows.value, cols.value, 3), np.uint8)
        self.L.och_graph_get_thumbnail(self.h, int(index), C.byref(rows), C.byref(cols), out.ctypes.data)
        return out

    def encode_thumbnails(self, ctx=None):
        """Every node's decoded thumbnail to the base64 PNG text graph.json carries (colour type 2, the three bytes as
        stored), all nodes in one batch; ctx: on that device, None: the CPU route - the same text.  Returns their number."""
        k = self.L.och_graph_encode_thumbnails(self.h, ctx.h if ctx is not None else None)
        if k < 0:
            raise capi.OchipError(self.L.och_last_error(self.h).decode())
        return int(k)

    def decode_thumbnails(self):
        """Every node's thumbnail text to the pixels the preview samples (three channels: gray replicated, alpha dropped;
        host code).  Returns the per-node statuses: -1 no text, PNG_OK, PNG_UNSUPPORTED, PNG_CORRUPT; a refused node is left
        as it was."""
        st = np.full(max(len(self.node_ids), 1), -1, np.int32)
        if self.L.och_graph_decode_thumbnails(self.h, st.ctypes.data) < 0:
            raise capi.OchipError(self.L.och_last_error(self.h).decode())
        return [int(v) for v in st[:len(self.node_ids)]]

    def edges_flat(self, node_subset=None):
        """The linked edges as flat dicts (src/dst node index, H, inlier pixel pairs, match indices, match
        distances): the form the stand-alone relax entry points and the parity checker take; optionally
        restricted to edges inside a node-index subset."""
        index_of = {nid: i for i, nid in enumerate(self.node_ids)}
        keep = None if node_subset is None else set(int(i) for i in node_subset)
        out = []
        for ed in self.edges(with_distances=True):
            s, d = index_of[ed["source"]], index_of[ed["dest"]]
            if keep is not None and (s not in keep or d not in keep):
                continue
            out.append(dict(src=s, dst=d, H=ed["H"], px=ed["px"], match_index=ed["match_index"], dist=ed["dist"]))
        return out


SHARD_SECONDS = ["extract", "block_linked", "subsets_export", "subsets_import", "remote_links", "edges_export",
                 "edges_import", "finalize", "stage"]


def shard_block(n_images, rank, world):
    """(first, count) of the contiguous image block of `rank` (och_shard_block)."""
    a, b = C.c_uint32(0), C.c_uint32(0)
    load().och_shard_block(n_images, rank, world, C.byref(a), C.byref(b))
    return a.value, b.value


class Shard:
    """One survey's load + link stages on rank `rank` of `world` (include/oc_host.h, och_shard_*): the caller moves the two
    buffers between the ranks (parallel.survey_sharded does it with torch.distributed)."""

    def __init__(self, graph, ctx, model, positions, orientations, rank, world):
        self.g, self.L = graph, graph.L
        pos = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
        ori = None if orientations is None else np.ascontiguousarray(orientations, np.float64)
        ids = np.zeros(max(len(pos), 1), np.uint64)
        self.h = self.L.och_shard_begin(graph.h, ctx.h, len(pos), model, pos, None if ori is None else ori.ctypes.data, rank, world, ids)
        if not self.h:
            raise capi.OchipError("och_shard_begin: " + self.L.och_last_error(graph.h).decode())
        graph.node_ids += [int(i) for i in ids[:len(pos)]]
        self.first, self.count = shard_block(len(pos), rank, world)

    def close(self):
        if getattr(self, "h", None):
            self.L.och_shard_destroy(self.h)
            self.h = None

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise capi.OchipError(what + " failed: " + self.L.och_last_error(self.g.h).decode())

    def counts(self):
        out = np.zeros(4, np.uint64)
        self.L.och_shard_counts(self.h, out)
        return dict(zip(["images", "pairs_in_block", "pairs_across_blocks", "halo_images"], (int(v) for v in out)))

    def load_link_local(self, images_block, width, height, max_keypoints=30000, on_device=True):
        """images_block: device pointer (on_device) or (count, h, w, 3) uint8 host array of the BLOCK's images."""
        src = int(images_block) if on_device else np.ascontiguousarray(images_block, np.uint8).ctypes.data
        self._check(self.L.och_shard_load_link_local(self.h, src, width, height, max_keypoints, int(on_device)), "load + link of the block")

    def _export(self, fn):
        ptr, n = C.c_void_p(0), C.c_uint64(0)
        self._check(fn(self.h, C.byref(ptr), C.byref(n)), "export")
        if n.value == 0:
            return np.zeros(0, np.uint8)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(n.value,))   # a view: copy before the next export

    def subsets_export(self):
        return self._export(self.L.och_shard_subsets_export)

    def edges_export(self):
        return self._export(self.L.och_shard_edges_export)

    @staticmethod
    def _aligned(buf):
        buf = np.ascontiguousarray(buf, np.uint8)
        if buf.ctypes.data % 8:
            tmp = np.zeros(len(buf) + 8, np.uint8)
            off = (-tmp.ctypes.data) % 8
            tmp[off:off + len(buf)] = buf
            buf = tmp[off:off + len(buf)]
        return buf

    def subsets_import(self, buf):
        buf = self._aligned(buf)
        self._check(self.L.och_shard_subsets_import(self.h, buf.ctypes.data, len(buf)), "subset import")

    def edges_import(self, buf):
        buf = self._aligned(buf)
        self._check(self.L.och_shard_edges_import(self.h, buf.ctypes.data, len(buf)), "edge import")

    def link_remote(self):
        self._check(self.L.och_shard_link_remote(self.h), "links across blocks")

    def finalize(self):
        """Returns (features, sparse features of the block, link timers, stage seconds)."""
        totals, timers, secs = np.zeros(2), np.zeros(8), np.zeros(9)
        self._check(self.L.och_shard_finalize(self.h, totals, timers, secs), "finalize")
        return totals[0], totals[1], dict(zip(LINK_TIMER_NAMES, timers.tolist())), dict(zip(SHARD_SECONDS, secs.tolist()))


def ransac_epipolar(ctx, model, rays, quality=None, threshold=0.01):
    """ransac<fundamental_matrix_model> (model 0) / ransac<essential_matrix_model> (model 1) on the device.  rays: n x 6
    {measurement1, measurement2}.  Returns (score, matrix 3 x 3, inliers, iterations, improvements)."""
    rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 6)
    n = len(rays)
    M, inl, counts = np.zeros((3, 3)), np.zeros(max(n, 1), np.uint8), np.zeros(3, np.uint32)
    q = None if quality is None else np.ascontiguousarray(quality, np.float64)
    score = load().och_ransac_epipolar(ctx.h, model, rays if n else np.zeros((1, 6)), None if q is None else q.ctypes.data, n,
                                       float(threshold), M.reshape(9), inl, counts)
    if score != score and n:
        raise capi.OchipError("epipolar RANSAC failed: " + ctx.last_error() if hasattr(ctx, "last_error") else "epipolar RANSAC failed")
    return score, M, inl[:n].astype(bool), int(counts[0]), int(counts[1])


def extract_tail(kp6, desc, scale):
    """The host tail of extract_features on given keypoints (detection order): (loc, strength, desc, num_sparse)."""
    L = load()
    kp6 = np.ascontiguousarray(kp6, np.float32).reshape(-1, 6)
    desc = np.ascontiguousarray(desc, np.uint64).reshape(-1, 8)
    n = len(kp6)
    loc, st, d, ns = np.zeros((n + 1, 2)), np.zeros(n + 1, np.float32), np.zeros((n + 1, 8), np.uint64), np.zeros(1, np.uint64)  # the seed keypoint appears twice
    m = L.och_extract_tail(kp6 if n else np.zeros((1, 6), np.float32), desc if n else np.zeros((1, 8), np.uint64), n, float(scale), loc, st, d, ns)
    return loc[:m].copy(), st[:m].copy(), d[:m].copy(), int(ns[0])


def extract_tail_prepared(lists, scale, force_host_nms=False):
    """The host tail on lists the device prepared (capi.Context.feature_lists): (loc, strength, desc, num_sparse)."""
    L = load()
    n = len(lists["response"])
    loc, st, d, ns = np.zeros((n + 1, 2)), np.zeros(n + 1, np.float32), np.zeros((n + 1, 8), np.uint64), np.zeros(1, np.uint64)
    rec = np.ascontiguousarray(lists["records"], np.uint8) if n else np.zeros((1, 88), np.uint8)
    resp = np.ascontiguousarray(lists["response"], np.float32) if n else np.zeros(1, np.float32)
    slot = np.ascontiguousarray(lists["slot"], np.uint32) if n else np.zeros(1, np.uint32)
    m = L.och_extract_tail_prepared(rec.ctypes.data, resp, slot.ctypes.data, int(lists["num_sparse"]),
                                    int(bool(lists["conflict"]) or force_host_nms), n, float(scale), loc, st, d, ns)
    return loc[:m].copy(), st[:m].copy(), d[:m].copy(), int(ns[0])


def decompose(H, m1, m2):
    """homography_model::decompose on inlier rays m1, m2 (n x 3 each): (can_decompose, poses 4 x 8)."""
    rays = np.ascontiguousarray(np.concatenate([np.asarray(m1, np.float64).reshape(-1, 3), np.asarray(m2, np.float64).reshape(-1, 3)], 1))
    poses = np.zeros((4, 8))
    ok = load().och_homography_decompose(np.ascontiguousarray(H, np.float64).reshape(9), rays if len(rays) else np.zeros((1, 6)), len(rays), poses)
    return bool(ok), poses


def image_to_3d(px, model10):
    px = np.ascontiguousarray(px, np.float64).reshape(-1, 2)
    rays = np.zeros((len(px), 3))
    if len(px):
        load().och_image_to_3d(px, len(px), np.ascontiguousarray(model10, np.float64), rays)
    return rays


def subsample(loc, strength, spacing, count=0):
    loc = np.ascontiguousarray(loc, np.float64)
    strength = np.ascontiguousarray(strength, np.float32)
    out = np.zeros(max(len(strength), 1), np.uint64)
    n = load().och_subsample(loc, strength, len(strength), spacing, count, out)
    return out[:n].copy()


def matches_from_device(raw, idx1, idx2):
    """raw: MATCH_DTYPE rows of one pair (len == len(idx1))."""
    raw = np.ascontiguousarray(raw, capi.MATCH_DTYPE)
    idx1 = np.ascontiguousarray(idx1, np.uint64)
    idx2 = np.ascontiguousarray(idx2, np.uint64)
    n = max(len(idx1), 1)
    i1, i2, d = np.zeros(n, np.uint64), np.zeros(n, np.uint64), np.zeros(n, np.float64)
    if len(raw) < len(idx1):
        raise ValueError("raw shorter than idx1")
    m = load().och_matches_from_device(raw.ctypes.data, idx1, len(idx1), idx2, len(idx2), i1, i2, d)
    return i1[:m].copy(), i2[:m].copy(), d[:m].copy()


IP_STATS16 = ["step_s", "init_s", "runners_s", "finalize_s", "load_runner_s", "link_runner_s", "relax_runner_s", "features", "sparse_features",
              "images_linked", "images_relaxed", "relax_solves", "relax_iterations", "relax_setup_host_s", "relax_device_s", "images_to_relax_next"]


class InitialProcessing:
    """INITIAL_PROCESSING as the reference pipelines it (src/pipeline/pipeline.cpp:522-570): step(batch) loads the batch, links
    the batch before and relaxes the batch before that, side by side; step() without images drains."""

    def __init__(self, graph, ctx):
        self.g, self.ctx = graph, ctx
        self.h = graph.L.och_initial_processing_create(graph.h, ctx.h)
        if not self.h:
            raise MemoryError("och_initial_processing_create")

    def close(self):
        if self.h:
            self.g.L.och_initial_processing_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    @property
    def pending(self):
        return bool(self.g.L.och_initial_processing_pending(self.h))

    def step(self, images_bgr=None, model=0, positions=None, max_keypoints=30000, device_shape=None, sequential=False):
        if images_bgr is None:
            n, h, w, src, on_dev, pos, ids = 0, 0, 0, None, 0, None, None
        else:
            if device_shape is None:
                imgs = np.ascontiguousarray(images_bgr, np.uint8)
                n, h, w, _ = imgs.shape
                src, on_dev = imgs.ctypes.data, 0
            else:
                n, h, w = device_shape
                src, on_dev = int(images_bgr), 1
            pos = np.ascontiguousarray(positions, np.float64).reshape(-1, 3)
            ids = np.zeros(max(n, 1), np.uint64)
        stats = np.zeros(16)
        rc = self.g.L.och_initial_processing_step(self.h, src, n, w, h, max_keypoints, on_dev, model,
                                                  None if pos is None else pos.ctypes.data, int(sequential),
                                                  None if ids is None else ids.ctypes.data, stats)
        if rc != 0:
            raise capi.OchipError("initial processing step failed: " + self.g.L.och_last_error(self.g.h).decode())
        if n:
            self.g.node_ids += [int(i) for i in ids[:n]]
        return dict(zip(IP_STATS16, stats.tolist()))
