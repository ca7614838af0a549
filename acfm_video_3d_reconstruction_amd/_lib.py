"""ctypes binding of libacfm_hip.so (C ABI declared in include/acfm_hip.h).

This is the only place the shared library is loaded.  It fails loudly: a missing library or
a CPU tensor is an error, never a silent fallback."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# ACFM_LIB: an alternative build of the same C ABI (the diagnostic build libacfm_hip_diag.so, or a kernel
# variant under test in tools/variants.py); never a fallback -- the path must exist.
SO_PATH = os.environ.get("ACFM_LIB") or os.path.join(_HERE, "libacfm_hip.so")
CSRC = os.path.join(_HERE, "csrc")

ABI_VERSION = 2000  # acfm_version() of the header these signatures mirror; lib() refuses any other build

_vp, _i, _f, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t
# Device pointers with the header's element type: ctypes binds them as c_void_p, call() checks a tensor's dtype against
# them (size and float-versus-integer; signedness is not told apart).  _vp takes a tensor of any dtype: void*, the
# mirrored structures, pointer tables and host out-parameters.
_pf, _pd, _p1, _p4, _p8 = "float*", "double*", "int8*", "int32*", "int64*"
_ELEMENTS = {_pf: (torch.float32,), _pd: (torch.float64,), _p1: (torch.uint8, torch.int8, torch.bool),
             _p4: (torch.int32, torch.uint32), _p8: (torch.int64, torch.uint64)}

# name -> (restype, parameters); must list every symbol of include/acfm_hip.h
SIGNATURES = {
    "acfm_version": (_i, []),
    "acfm_arch": (ctypes.c_char_p, []),
    "acfm_prof_enable": (_i, [_i]),
    "acfm_prof_collect": (_i, [_vp, _vp, _i]),
    "acfm_prof_name": (ctypes.c_char_p, [_i]),
    "acfm_project": (_i, [_pf, _pf, _i, _i, _f, _pf, _vp]),
    "acfm_project_backward": (_i, [_pf, _pf, _pf, _i, _i, _pf, _pf, _vp]),
    "acfm_project_xy": (_i, [_pf, _pf, _i, _i, _f, _pf, _vp]),
    "acfm_project_xy_backward": (_i, [_pf, _pf, _pf, _i, _i, _pf, _pf, _vp]),
    "acfm_deform_apply": (_i, [_pf, _pf, _pf, _i, _i, _i, _pf, _vp]),
    "acfm_deform_apply_backward": (_i, [_pf, _pf, _pf, _i, _i, _i, _pf, _pf, _pf, _vp]),
    "acfm_deform_presolve_sums_f64": (_i, [_pf, _pf, _i, _i, _i, _pd, _pd, _pf, _vp]),
    "acfm_symmetrize": (_i, [_pf, _i, _i, _i, _pf, _vp]),
    "acfm_symmetrize_backward": (_i, [_pf, _i, _i, _i, _pf, _vp]),
    "acfm_correlation_forward": (_i, [_pf, _pf, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_correlation_channel_split": (_i, [_i, _i, _i, _i]),
    "acfm_correlation_backward": (_i, [_pf, _pf, _pf, _i, _i, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_deform_conv2d_forward": (_i, [_pf, _pf, _pf, _pf, _i, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_deform_conv2d_channel_tile": (_i, [_i, _i, _i, _i]),
    "acfm_deform_conv2d_backward_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "acfm_deform_conv2d_backward": (_i, [_pf, _pf, _pf, _pf, _i, _i, _i, _i, _i, _i, _pf, _pf, _pf, _pf, _vp, _sz, _vp]),
    "acfm_of_loss": (_i, [_pf, _pf, _pf, _p1, _i, _i, _i, _i, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_of_loss_backward": (_i, [_pf, _pf, _pf, _p1, _pf, _pf, _i, _i, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_camera_pipeline": (_i, [_pf, _p8, _pf, _i, _i, _f, _pf, _vp]),
    "acfm_camera_pipeline_backward": (_i, [_pf, _p8, _pf, _pf, _i, _i, _f, _pf, _vp]),
    "acfm_camera_mirror": (_i, [_pf, _i, _pf, _vp]),
    "acfm_camera_pipeline_tables": (_i, [_vp, _i, _i, _p8, _p8, _p8, _pf, _i, _i, _f, _pf, _vp]),
    "acfm_camera_pipeline_tables_backward": (_i, [_vp, _i, _i, _p8, _p8, _p8, _pf, _pf, _i, _i, _f, _vp, _vp]),
    "acfm_camera_pipeline_azel": (_i, [_pf, _p8, _pf, _i, _i, _f, _f, _f, _f, _f, _pf, _vp]),
    "acfm_camera_pipeline_azel_backward": (_i, [_pf, _p8, _pf, _pf, _i, _i, _f, _f, _f, _f, _f, _pf, _vp]),
    "acfm_camera_pipeline_azel_tables": (_i, [_vp, _i, _i, _p8, _p8, _p8, _pf, _i, _i, _f, _f, _f, _f, _f, _pf, _vp]),
    "acfm_camera_pipeline_azel_tables_backward": (_i, [_vp, _i, _i, _p8, _p8, _p8, _pf, _pf, _i, _i, _f, _f, _f, _f, _f,
                                                       _vp, _vp]),
    "acfm_camera_normalize": (_i, [_pf, _i, _pf, _vp]),
    "acfm_camera_normalize_backward": (_i, [_pf, _pf, _i, _pf, _vp]),
    "acfm_deform_solve_workspace_bytes": (_sz, [_i, _i]),
    "acfm_deform_solve": (_i, [_pf, _pf, _i, _i, _pf, _vp, _sz, _vp]),
    "acfm_deform_solve_backward": (_i, [_pf, _i, _i, _vp, _sz, _pf, _vp]),
    "acfm_deform_solve_info": (_i, [_vp, _sz, _i, _vp, _vp]),
    "acfm_deform_solve_info_offset": (_sz, [_i]),
    "acfm_raster_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "acfm_stream_capture_id": (_i, [_vp, _vp]),
    "acfm_sil_forward": (_i, [_pf, _p8, _pf, _i, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _p8, _p1, _vp,
                              _sz, _vp, _vp, _vp]),
    "acfm_sil_backward": (_i, [_pf, _p8, _pf, _vp, _p8, _pf, _i, _i, _i, _i, _f, _f, _f, _pf, _pf, _vp,
                               _sz, _i, _vp, _vp, _vp]),
    "acfm_sil_loss_forward": (_i, [_pf, _p8, _pf, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _p8,
                                   _p1, _pf, _vp, _sz, _vp, _vp, _vp]),
    "acfm_sil_loss_backward": (_i, [_pf, _p8, _pf, _vp, _p8, _vp, _vp, _i, _pf, _i, _i, _i, _i, _f, _f, _f, _pf,
                                    _pf, _vp, _sz, _i, _vp, _vp, _vp]),
    "acfm_hard_raster": (_i, [_pf, _p8, _i, _i, _i, _i, _p8, _p1, _vp, _sz, _vp, _vp]),
    "acfm_rasterize_fragments_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "acfm_rasterize_fragments": (_i, [_pf, _p8, _i, _i, _i, _i, _i, _f, _i, _p8, _pf, _pf, _pf, _vp, _sz, _vp, _vp]),
    "acfm_rasterize_fragments_backward": (_i, [_pf, _p8, _p8, _pf, _pf, _pf, _i, _i, _i, _i, _i, _f, _i, _pf, _vp,
                                               _sz, _i, _vp, _vp]),
    "acfm_sigmoid_alpha_blend": (_i, [_p8, _pf, _pf, _sz, _i, _f, _pf, _vp, _vp]),
    "acfm_sigmoid_alpha_blend_backward": (_i, [_p8, _pf, _pf, _sz, _i, _f, _pf, _pf, _vp, _vp]),
    "acfm_softmax_rgb_blend": (_i, [_p8, _pf, _pf, _pf, _pf, _pf, _i, _i, _pf, _sz, _i, _i, _vp, _pf, _vp, _vp]),
    "acfm_softmax_rgb_blend_backward": (_i, [_p8, _pf, _pf, _pf, _pf, _pf, _i, _i, _pf, _sz, _i, _i, _vp, _pf, _pf,
                                             _pf, _pf, _pf, _vp, _sz, _vp, _vp]),
    "acfm_interpolate_face_attributes": (_i, [_p8, _pf, _pf, _sz, _i, _i, _i, _pf, _vp, _vp]),
    "acfm_interpolate_face_attributes_backward": (_i, [_p8, _pf, _pf, _pf, _sz, _i, _i, _i, _pf, _pf, _vp, _sz, _vp,
                                                       _vp]),
    "acfm_uv_texels": (_i, [_p8, _pf, _pf, _pf, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _pf, _vp, _vp]),
    "acfm_uv_texels_backward": (_i, [_p8, _pf, _pf, _pf, _pf, _sz, _i, _i, _i, _i, _i, _i, _i, _i, _pf, _pf, _pf, _vp,
                                     _sz, _vp, _vp]),
    "acfm_vertex_normals": (_i, [_pf, _p8, _p4, _p4, _i, _i, _pf, _pf, _vp]),
    "acfm_vertex_normals_backward": (_i, [_pf, _p8, _p4, _p4, _pf, _pf, _i, _i, _pf, _vp, _sz, _vp]),
    "acfm_light_points": (_i, [_pf, _pf, _pf, _p8, _pf, _i, _i, _i, _pf, _vp]),
    "acfm_light_points_backward": (_i, [_pf, _pf, _pf, _p8, _pf, _i, _pf, _i, _i, _pf, _pf, _pf, _vp]),
    "acfm_phong_shade": (_i, [_p8, _pf, _pf, _pf, _p8, _pf, _pf, _i, _i, _sz, _i, _i, _i, _i, _i, _pf, _vp, _vp]),
    "acfm_phong_shade_backward": (_i, [_p8, _pf, _pf, _pf, _p8, _pf, _pf, _i, _i, _pf, _sz, _i, _i, _i, _i, _i, _pf,
                                       _pf, _pf, _vp, _sz, _vp, _vp]),
    "acfm_corner_gather": (_i, [_pf, _p4, _p4, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_tex_forward": (_i, [_pf, _p8, _pf, _vp, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _vp, _p4,
                              _vp, _sz, _i, _f, _i, _vp, _vp]),
    "acfm_vertex_color_forward": (_i, [_pf, _p8, _pf, _pf, _i, _i, _i, _i, _f, _f, _f, _pf, _pf, _p8, _vp, _sz,
                                       _i, _f, _vp, _vp]),
    "acfm_tex_backward": (_i, [_pf, _p4, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_tex_backward_faces": (_i, [_pf, _p4, _vp, _sz, _f, _i, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_tex_mse_forward": (_i, [_pf, _p8, _pf, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _f, _f, _vp, _vp, _vp, _p4,
                                  _pf, _vp, _sz, _i, _f, _i, _vp, _vp]),
    "acfm_tex_mse_backward_faces": (_i, [_vp, _vp, _vp, _i, _pf, _p4, _vp, _sz, _f, _i, _i, _i, _i, _i, _i, _pf, _vp,
                                         _vp]),
    "acfm_combine_losses": (_i, [_vp, _p4, _pf, _i, _i, _pf, _vp]),
    "acfm_combine_losses_backward": (_i, [_pf, _vp, _p4, _pf, _i, _i, _vp]),
    "acfm_hypothesis_total": (_i, [_vp, _pf, _p4, _pf, _i, _i, _i, _pf, _pf, _pf, _pf, _pf, _vp]),
    "acfm_hypothesis_total_backward": (_i, [_pf, _pf, _pf, _i, _i, _i, _vp, _vp]),
    "acfm_texture_cycle_scratch_floats": (_sz, [_i, _i, _i, _i]),
    "acfm_texture_cycle": (_i, [_pf, _i, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_texture_cycle_backward": (_i, [_pf, _pf, _pf, _i, _i, _i, _i, _pf, _vp]),
    "acfm_loss_partial_floats": (_sz, [_i, _i, _i]),
    "acfm_mask_losses": (_i, [_pf, _pf, _pf, _i, _i, _i, _pf, _p4, _pf, _sz, _vp]),
    "acfm_step_losses_ws": (_sz, [_i, _i, _i, _i, _vp]),
    "acfm_step_losses_forward": (_i, [_vp, _vp, _vp, _vp, _i, _p4, _pf, _sz, _vp]),
    "acfm_mask_losses_backward": (_i, [_pf, _pf, _pf, _pf, _i, _i, _i, _pf, _vp]),
    "acfm_tex_mse": (_i, [_pf, _pf, _pf, _i, _i, _i, _pf, _p4, _pf, _sz, _vp]),
    "acfm_tex_mse_backward": (_i, [_pf, _pf, _pf, _pf, _i, _i, _i, _pf, _vp]),
    "acfm_cot_laplacian": (_i, [_pf, _p8, _i, _i, _pf, _vp]),
    "acfm_laplacian_smoothing_state_floats": (_sz, [_i, _i]),
    "acfm_laplacian_smoothing": (_i, [_pf, _p8, _pf, _i, _i, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_laplacian_smoothing_backward": (_i, [_p8, _pf, _pf, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_edge_rigidity": (_i, [_pf, _p8, _pf, _p8, _i, _pf, _vp]),
    "acfm_edge_rigidity_backward": (_i, [_pf, _p8, _pf, _p8, _i, _i, _i, _i, _pf, _pf, _pf, _vp]),
    "acfm_edt_workspace_bytes": (_sz, [_i, _i, _i]),
    "acfm_edt": (_i, [_pf, _i, _i, _i, _i, _pf, _vp, _sz, _vp]),
    "acfm_boundaries": (_i, [_pf, _i, _i, _i, _i, _pf, _p4, _vp]),
    "acfm_visible_vertices": (_i, [_p8, _p8, _i, _i, _i, _i, _i, _p1, _vp]),
    "acfm_bds_loss": (_i, [_pf, _pf, _p1, _p4, _i, _i, _i, _i, _i, _i, _pf, _p4, _p4, _pf, _sz, _vp]),
    "acfm_bds_loss_backward": (_i, [_pf, _pf, _p4, _p4, _pf, _i, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_boundary_subset": (_i, [_p8, _p4, _i, _i, _i, _i, _p4, _vp]),
    "acfm_surface_sample_workspace_bytes": (_sz, [_i, _i]),
    "acfm_surface_sample": (_i, [_p8, _pf, _p8, _p8, _vp, _i, _i, _i, _i, _pf, _p4, _pf, _vp, _sz, _vp]),
    "acfm_surface_sample_backward": (_i, [_pf, _p4, _pf, _p8, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_chamfer_partial_floats": (_sz, [_i, _i, _i]),
    "acfm_chamfer": (_i, [_pf, _pf, _p8, _p8, _i, _i, _i, _pf, _p4, _p4, _p4, _pf, _sz, _vp]),
    "acfm_chamfer_backward": (_i, [_pf, _pf, _p8, _p8, _p4, _p4, _pf, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_knn_points": (_i, [_pf, _pf, _p8, _p8, _i, _i, _i, _i, _pf, _p8, _vp]),
    "acfm_knn_points_backward": (_i, [_pf, _pf, _p8, _p8, _p8, _pf, _i, _i, _i, _i, _pf, _pf, _vp]),
    "acfm_knn_gather": (_i, [_pf, _vp, _i, _p8, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_knn_gather_backward": (_i, [_pf, _vp, _i, _p8, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_mesh_term_partial_floats": (_sz, [_i]),
    "acfm_edge_length_loss": (_i, [_pf, _p8, _pf, _i, _i, _f, _pf, _p4, _pf, _sz, _vp]),
    "acfm_edge_length_loss_backward": (_i, [_pf, _p8, _pf, _pf, _i, _i, _f, _pf, _vp]),
    "acfm_normal_consistency": (_i, [_pf, _p8, _pf, _i, _i, _pf, _p4, _pf, _sz, _vp]),
    "acfm_normal_consistency_backward": (_i, [_pf, _p8, _pf, _pf, _i, _i, _pf, _vp]),
    "acfm_uv_atlas_forward": (_i, [_pf, _pf, _i, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_uv_atlas_taps": (_i, [_pf, _i, _i, _i, _p4, _vp]),
    "acfm_uv_atlas_backward": (_i, [_pf, _pf, _pf, _p4, _p4, _i, _i, _i, _i, _i, _i, _i, _pf, _vp]),
    "acfm_geodesic_lds_bytes": (_sz, [_i, _i, _i]),
    "acfm_geodesic_distances": (_i, [_pf, _p4, _p4, _p4, _i, _i, _i, _i, _i, _p4, _i, _pf, _p4, _vp]),
    "acfm_geodesic_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "acfm_geodesic_distances_dev": (_i, [_pf, _p4, _p4, _p4, _i, _i, _i, _i, _i, _p4, _i, _pf, _p4, _i, _vp, _sz, _vp]),
    "acfm_lpips_input_forward": (_i, [_pf, _pf, _i, _i, _i, _i, _pf, _vp]),
    "acfm_lpips_input_backward": (_i, [_pf, _pf, _i, _i, _i, _i, _pf, _vp]),
    "acfm_lpips_layer_forward": (_i, [_pf, _pf, _pf, _i, _i, _i, _i, _pf, _sz, _vp]),
    "acfm_lpips_layer_backward": (_i, [_pf, _pf, _pf, _pf, _sz, _i, _i, _i, _i, _pf, _vp]),
    "acfm_lpips_mask_weights": (_i, [_pf, _i, _i, _i, _p4, _i, _pf, _vp]),
    "acfm_lpips_masked_mean_forward": (_i, [_pf, _pf, _i, _i, _i, _pf, _vp]),
    "acfm_lpips_masked_mean_backward": (_i, [_pf, _pf, _i, _i, _i, _pf, _vp]),
    "acfm_kp_weights_forward": (_i, [_pf, _i, _i, _pf, _pf, _pf, _vp]),
    "acfm_kp_weights_backward": (_i, [_pf, _pf, _pf, _pf, _pf, _i, _i, _pf, _vp]),
    "acfm_kp_head_forward": (_i, [_pf, _pf, _pf, _pf, _i, _i, _i, _i, _i, _f, _pf, _pf, _pf, _pf, _vp]),
    "acfm_kp_head_workspace_bytes": (_sz, [_i, _i]),
    "acfm_kp_head_backward": (_i, [_pf, _pf, _pf, _pf, _pf, _pf, _pf, _pf, _pf, _i, _i, _i, _i, _i, _pf, _pf, _pf, _vp,
                                   _sz, _vp]),
    "acfm_camera_loss_forward": (_i, [_pf, _pf, _pf, _pf, _i, _i, _f, _pf, _p8, _vp]),
    "acfm_camera_loss_backward": (_i, [_pf, _pf, _pf, _p8, _pf, _i, _f, _pf, _vp]),
}

_ERR = {1: "ACFM_E_BADARG (shape/parameter outside what the kernels support)",
        2: "ACFM_E_LAUNCH (HIP launch failed)", 3: "ACFM_E_WORKSPACE (workspace too small)"}

_LIB = None
_BOUND = {}   # name -> (bound function, pointer_kinds of its parameters), filled by lib()


def build(verbose=False):
    """Compile libacfm_hip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    import subprocess
    out = None if verbose else subprocess.DEVNULL
    subprocess.check_call(["make", "-C", CSRC, "-j4"], stdout=out)
    return SO_PATH


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(SO_PATH):
            raise RuntimeError(
                "libacfm_hip.so is missing (%s). Build it with `python -c \"import __graft_entry__ "
                "as g; g.build()\"` or `make -C %s`. There is no CPU fallback." % (SO_PATH, CSRC))
        handle = ctypes.CDLL(SO_PATH)
        handle.acfm_version.restype, handle.acfm_version.argtypes = SIGNATURES["acfm_version"]
        found = handle.acfm_version()
        if found != ABI_VERSION:   # before any other symbol: same names, other argument lists
            raise RuntimeError(
                "%s reports acfm_version() = %d, this package binds version %d of include/acfm_hip.h: the library is "
                "a build of another tree. Rebuild it with `make -C %s`." % (SO_PATH, found, ABI_VERSION, CSRC))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
            fn.restype, fn.argtypes = res, [_vp if type(a) is str else a for a in args]
            _BOUND[name] = (fn, pointer_kinds(args))
        _LIB = handle
    return _LIB


PROF_NKERNELS = 24  # ACFM_PROF_NKERNELS


def prof_collect():
    """-> {kernel name: (total ms, launches)} since acfm_prof_enable(1) / the last collect."""
    ms = (ctypes.c_float * PROF_NKERNELS)()
    cnt = (ctypes.c_int * PROF_NKERNELS)()
    check(lib().acfm_prof_collect(ms, cnt, PROF_NKERNELS), "acfm_prof_collect")
    return {lib().acfm_prof_name(i).decode(): (ms[i], cnt[i]) for i in range(PROF_NKERNELS) if cnt[i]}


def ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def cur_stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed: %s" % (what, _ERR.get(rc, "error %d" % rc)))


def pointer_kinds(params):
    """What marshal() needs of a SIGNATURES entry's parameters: (their number, ((position, label, dtypes), ...) of the
    pointers in front of the last parameter, the stream; dtypes None where any element type will do)."""
    return len(params), tuple((i, "void*", None) if a is _vp else (i, a, _ELEMENTS[a])
                              for i, a in enumerate(params[:-1]) if a is _vp or type(a) is str)


def marshal(name, kinds, device, args):
    """`args` of entry point `name` (all but the stream) as ctypes takes them: a tensor in a pointer position becomes
    its address if it is on `device`, contiguous and of the element type the header declares (kinds = pointer_kinds of
    the entry); None, ctypes values and numbers pass as they are.  Nothing is copied or converted.  Of a tensor only
    get_device / is_contiguous / dtype / data_ptr / numel are asked, which a PendingTerm answers without its values."""
    count, pointers = kinds
    if len(args) + 1 != count:
        raise TypeError("%s takes %d arguments, the stream included; got %d and the stream" % (name, count, len(args)))
    out = list(args)
    index = device.index if device.type == "cuda" else -1
    for i, label, dtypes in pointers:
        a = out[i]
        if a is None or not isinstance(a, torch.Tensor):
            continue
        what = None
        if a.get_device() != index:          # (-1 for a CPU tensor)
            what = ValueError, "a tensor on %s in a call on %s" % (a.device, device)
        elif not a.is_contiguous():
            what = ValueError, "a non-contiguous tensor, shape %s strides %s" % (tuple(a.shape), a.stride())
        elif dtypes is not None and a.dtype not in dtypes:
            what = TypeError, "a %s tensor" % a.dtype
        else:
            out[i] = a.data_ptr()
            if not out[i] and a.numel():   # a LazyGrad / LazyPixToFace: the caller was to form it, or not to pass it
                what = ValueError, "a %s without storage" % type(a).__name__
        if what:
            raise what[0]("%s, parameter %d: the header declares %s, got %s" % (name, i, label, what[1]))
    return out


def call(name, device, *args):
    """Entry point `name` on `device`, ordered on its current stream (appended as the last argument); tensors are
    passed as they are and checked by marshal(); raises on a nonzero return code."""
    if _LIB is None:
        lib()
    fn, kinds = _BOUND[name]
    args = marshal(name, kinds, device, args)
    with torch.cuda.device(device):
        check(fn(*args, cur_stream(device)), name)


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("acfm_video_3d_reconstruction_amd ops run on the GPU only "
                               "(got a %s tensor); there is no CPU fallback" % t.device)


class StepMaskJob(ctypes.Structure):
    """acfm_step_mask_job of include/acfm_hip.h (and below: the other jobs of acfm_step_losses_forward)."""
    _fields_ = [("mask", _vp), ("gt", _vp), ("edt", _vp), ("out", _vp), ("HW", _i), ("ref_batch", _i)]


class StepTexJob(ctypes.Structure):
    _fields_ = [("tex", _vp), ("img", _vp), ("mask", _vp), ("out", _vp), ("HW", _i), ("ref_batch", _i)]


class StepBdsJob(ctypes.Structure):
    _fields_ = [("verts_xy", _vp), ("bds", _vp), ("vis", _vp), ("sel", _vp), ("loss", _vp), ("argmin", _vp),
                ("V", _i), ("P", _i), ("ref_batch", _i), ("rows", _i), ("S", _i)]


class StepTotalJob(ctypes.Structure):
    _fields_ = [("terms", _vp), ("cols", _vp), ("weights", _vp), ("nterms", _i), ("total", _vp)]


class RasterTuning(ctypes.Structure):
    """AcfmRasterTuning of include/acfm_hip.h (per call; results never depend on it)."""
    _fields_ = [("split_mode", _i), ("grid_div", _i * 3), ("flags", _i)]


_TUNE = __import__("threading").local()


class raster_tuning:
    """with raster_tuning(split=0, grid_div=(1, 0, 0)): ...   -- every raster op called inside the block
    (on this thread) passes this tuning to the C ABI; outside any block the library defaults apply.
    Tests use it to force the split / unsplit kernels and every grid divisor; the library itself keeps
    no tuning state."""

    def __init__(self, split=-5, grid_div=(0, 0, 0), deterministic=False, record_cover=None):
        """deterministic=True: the silhouette backward accumulates in fixed point (bit-reproducible run to run).
        record_cover: True / False forces ACFM_RECORD_COVER (the silhouette render leaves the nearest covering face
        per pixel for a texture render that takes its workspace over) on / off; None lets ops/render.py decide -- on while
        texture renders do follow the silhouette renders on this device.
        (Bit 1 of the flags, half storage, is not set here: it changes buffer types, so the ops that support it take
        storage="f16" and set it themselves -- with_f16() below.)"""
        self.t = RasterTuning(int(split), (_i * 3)(*[int(d) for d in grid_div]), 1 if deterministic else 0)
        self.t.record_cover = record_cover   # (a Python attribute: not part of the C structure)

    def __enter__(self):
        self.prev = getattr(_TUNE, "cur", None)
        _TUNE.cur = self.t
        return self

    def __exit__(self, *exc):
        _TUNE.cur = self.prev


def tuning():
    """-> (ctypes pointer or None, the structure to keep alive / to save for the backward)."""
    t = getattr(_TUNE, "cur", None)
    return (ctypes.byref(t) if t is not None else None), t


def tuning_ptr(t):
    return ctypes.byref(t) if t is not None else None


def with_f16(t, on):
    """The tuning in effect with flags bit 1 (ACFM_STORE_F16) set or cleared: a fresh structure."""
    if t is None:
        return RasterTuning(-5, (_i * 3)(0, 0, 0), 2) if on else None
    return RasterTuning(t.split_mode, (_i * 3)(*t.grid_div), (t.flags & ~2) | (2 if on else 0))


def with_cover(t, on):
    """The tuning in effect with flags bit 2 (ACFM_RECORD_COVER) set or cleared: a fresh structure (None = defaults)."""
    if t is None:
        return RasterTuning(-5, (_i * 3)(0, 0, 0), 4) if on else None
    if bool(t.flags & 4) == bool(on):
        return t
    return RasterTuning(t.split_mode, (_i * 3)(*t.grid_div), (t.flags & ~4) | (4 if on else 0))


class SilExtras(ctypes.Structure):
    """AcfmSilExtras of include/acfm_hip.h (every field optional)."""
    _fields_ = [("proj_xy", _vp), ("grad_proj_xy", _vp), ("tex_imgs", _vp), ("tex_sil", _vp), ("tex_pix_to_face", _vp),
                ("tex_texel_idx", _vp)]


def sil_extras(proj_xy=None, grad_proj_xy=None, prefill=None):
    """-> (ctypes pointer, the structure to keep alive) for the `extras` of the silhouette entry points; tensors or None."""
    p = lambda t: None if t is None else t.data_ptr()
    pf = prefill or (None, None, None, None)
    e = SilExtras(p(proj_xy), p(grad_proj_xy), p(pf[0]), p(pf[1]), p(pf[2]), p(pf[3]))
    return ctypes.byref(e), e


class BlendParams(ctypes.Structure):
    """AcfmBlendParams of include/acfm_hip.h (host structure, read at call time)."""
    _fields_ = [("sigma", _f), ("gamma", _f), ("background", _f * 3), ("znear", _f), ("zfar", _f)]


_CONSTS = {}


def const(values, device, dtype=None):
    """Small constant tensor on `device`, uploaded once per (values, device, dtype): a fresh
    torch.tensor(..., device=cuda) is a pageable host-to-device copy, which is not allowed while
    a stream is being captured into a hipGraph."""
    import torch
    dtype = dtype or torch.float32
    key = (tuple(values), str(device), dtype)
    t = _CONSTS.get(key)
    if t is None:
        t = _CONSTS[key] = torch.tensor(values, dtype=dtype, device=device)
    return t
