"""Host only, imports only: the `ops` package keeps the namespace the single-file module had, and every piece of
process-wide state reached as `ops.NAME` is the very container its defining module reads."""
import importlib

import pytest

from acfm_video_3d_reconstruction_amd import ops

# every name of ops.py before it became a package (modules it happened to import aside)
PARENT_NAMES = [
    'FRAGMENT_K', 'GEODESIC_LDS_MAX', 'GEODESIC_MAX_STEINER', 'GEODESIC_MEMORY', 'KP_MAX_K', 'KP_MAX_N', 'KP_MAX_V',
    'LAZY_GRADS', 'LPIPS_EPS', 'LPIPS_SCALE', 'LPIPS_SHIFT', 'LazyGrad', 'LazyPixToFace', 'PREFILL_TEX', 'PendingTerm',
    'SIL_BLUR', 'SIL_K', 'SIL_SIGMA', 'SOLVE_INFO_HANDOFF', 'TEX_BWD_GATHER', 'UVAtlasTable', 'UV_PADDING_MODES',
    '_BdsLoss', '_BdsLossSel', '_COVER', '_CameraLoss', '_CameraNormalize', '_CameraPipeline', '_CameraPipelineTables',
    '_Chamfer', '_Combine', '_Correlation', '_DEFER', '_DeformApply', '_DeformConv2d', '_DeformSolve', '_EPOCH',
    '_EdgeLength', '_EdgeRigidity', '_FACES', '_FLOW_TRAINABLE', '_FORWARD_ONLY', '_FUSED_LAST', '_Fragments',
    '_HypTotal', '_Interpolate', '_KpHead', '_KpWeights', '_LOCK', '_LOSS_BDS', '_LOSS_CHAMFER', '_LOSS_EDGE_LEN',
    '_LOSS_MASK', '_LOSS_NORMAL', '_LOSS_SCRATCH', '_LOSS_TEX_MSE', '_LaplacianSmoothing', '_LpipsInput',
    '_LpipsLayers', '_LpipsMaskedMean', '_MaskLosses', '_NormalConsistency', '_OFLoss', '_PENDING', '_PENDING_META',
    '_PRESOLVE_SINKS', '_PendingJob', '_Project', '_ProjectXY', '_SETUP', '_SHARE', '_SOLVE_PENDING', '_Setup',
    '_SigmoidBlend', '_SilRender', '_SoftmaxBlend', '_TICKET_CHUNKS', '_TICKET_CHUNK_WORDS', '_TexCycle', '_TexMSE',
    '_TexRender', '_UVAtlas', '_UvTexels', '_a16', '_capture_id', '_correlation_args', '_correlation_forward',
    '_cover_taken', '_cover_tuning', '_dconv_args', '_dconv_forward', '_deferring', '_det_ws', '_f32c', '_frag_planes',
    '_i64c', '_is_f16', '_kp_f32', '_kp_limits', '_launch_step_tail', '_lazy_pix_to_face', '_lengths', '_loss_scratch',
    '_lpips_batches', '_lpips_layer_host', '_once', '_pending_terms', '_proj_key', '_ptr_at', '_raw', '_real',
    '_ref_batch', '_remember_setup', '_row_scratch', '_same_tensor', '_setup_key', '_shade_storage', '_shared_setup',
    '_sil_apply', '_step_scratch', '_take_prefill', '_ticket_words', '_uv_table_from_taps', '_workspace',
    'atlas_softmax_blend', 'bds_loss_per_mesh', 'blend_struct', 'boundary_subset', 'camera_loss', 'camera_mirror',
    'camera_normalize', 'camera_pipeline', 'camera_pipeline_tables', 'chamfer_nearest', 'chamfer_sums',
    'combine_losses', 'correlation', 'cot_laplacian', 'decode_solve_info', 'defer_losses', 'deform_apply',
    'deform_conv2d', 'deform_solve', 'drop_presolve_sink', 'edge_length_sum', 'edge_rigidity_sum', 'expand_faces',
    'flush_pending_losses', 'geodesic_device_workgroups', 'geodesic_distances', 'geodesic_max_steiner',
    'geodesic_memory', 'graph_replay', 'hard_raster', 'hypothesis_total', 'interpolate_face_attributes',
    'invalidate_setups', 'kp_head', 'kp_weights', 'laplacian_smoothing_sum', 'launch_pending_together',
    'loss_tickets_clean', 'lpips_input', 'lpips_layer', 'lpips_layers', 'lpips_mask_weights', 'lpips_masked_mean',
    'mask_losses', 'normal_consistency_sum', 'of_loss', 'project', 'project_xy', 'rasterize_fragments',
    'register_presolve_sink', 'reset_loss_scratch', 'share_setup', 'sigmoid_alpha_blend', 'sil_render',
    'sil_render_losses', 'softmax_rgb_blend', 'solve_status', 'tex_mse', 'tex_render', 'tex_render_mse',
    'texture_cycle', 'uv_atlas', 'uv_atlas_table', 'uv_texels', 'vertex_color_render', 'visible_vertices']

# process-wide state and switches -> the module that defines and reads them
STATE = {
    "_LOCK": "base", "_FACES": "base", "_LOSS_SCRATCH": "base", "_TICKET_CHUNKS": "base", "LAZY_GRADS": "base",
    "_DEFER": "pending", "_PENDING": "pending", "_FUSED_LAST": "pending", "_PENDING_META": "pending",
    "_SETUP": "render", "_COVER": "render", "_EPOCH": "render", "_SHARE": "render", "PREFILL_TEX": "render",
    "TEX_BWD_GATHER": "render",
    "_PRESOLVE_SINKS": "geometry", "_SOLVE_PENDING": "geometry",
    "_FLOW_TRAINABLE": "flow",
}


def test_every_parent_name_resolves():
    assert hasattr(ops, "__path__")
    assert len(PARENT_NAMES) == len(set(PARENT_NAMES)) == 190
    assert [n for n in PARENT_NAMES if not hasattr(ops, n)] == []


@pytest.mark.parametrize("name", sorted(STATE))
def test_state_is_one_mutable_object(name):
    home = importlib.import_module("%s.%s" % (ops.__name__, STATE[name]))
    assert getattr(ops, name) is getattr(home, name)
    # a scalar or a tuple could only be changed by rebinding the name, which a re-export does not follow
    assert not isinstance(getattr(ops, name), (bool, int, float, str, tuple))
