"""torch.autograd bindings of the C ABI (include/acfm_hip.h).

torch is used here for device memory, streams and autograd bookkeeping only; every op body
is one or more stream-ordered calls into libacfm_hip.so."""
# One module per operator family; `ops.NAME` is the interface, private names included.  Imports go one way only:
#   1. base         helpers, LazyGrad, _LOCK, the face-list memo and the ticket / partials scratch: imports _lib only
#   2. the core, which shares process-wide state:
#        pending      deferred loss terms and the step tail                          <- base
#        step_losses  mask_losses, tex_mse, bds_loss_per_mesh, combine_losses        <- base, pending
#        render       setup / cover / prefill caches, LazyPixToFace, the renders     <- base, pending
#   3. the leaves, plain "allocate, call, return" bindings, each <- base only:
#        geometry, flow, fragments, hypotheses, mesh_terms, geodesic, uvatlas, lpips, keypoint_loss, symmetry, surface
#        and neighbours (knn_points, knn_gather), which takes _lengths from mesh_terms, and lighting (vertex_normals,
#        light_points, phong_shade), which takes the fragment checks from fragments
#      (geodesic_distances alone looks up pytorch3d_shim's Meshes when called: the shim is built on this package)
# State is reached through containers that are mutated in place (dicts, one-element lists), never rebound: a
# re-export below copies the binding, so `ops.X = ...` would not reach the module that reads X.
from .base import (LAZY_GRADS, LazyGrad, _FACES, _LOCK, _LOSS_BDS, _LOSS_CHAMFER, _LOSS_EDGE_LEN, _LOSS_MASK,
                   _LOSS_NORMAL, _LOSS_SCRATCH, _LOSS_TEX_MSE, _TICKET_CHUNKS, _TICKET_CHUNK_WORDS, _a16, _capture_id,
                   _f32c, _i64c, _is_f16, _loss_scratch, _real, _ref_batch, _row_scratch, _same_tensor, _ticket_words,
                   _workspace, expand_faces, loss_tickets_clean, reset_loss_scratch)
from .pending import (PendingTerm, _DEFER, _FUSED_LAST, _PENDING, _PENDING_META, _PendingJob, _deferring,
                      _launch_step_tail, _pending_terms, _raw, _step_scratch, defer_losses, flush_pending_losses,
                      launch_pending_together)
from .step_losses import (_BdsLoss, _BdsLossSel, _Combine, _MaskLosses, _TexMSE, bds_loss_per_mesh, boundary_subset,
                          combine_losses, mask_losses, tex_mse)
from .render import (LazyPixToFace, PREFILL_TEX, SIL_BLUR, SIL_K, SIL_SIGMA, TEX_BWD_GATHER, _COVER, _EPOCH, _SETUP,
                     _SHARE, _Setup, _SilRender, _TexRender, _cover_taken, _cover_tuning, _lazy_pix_to_face, _proj_key,
                     _proj_serves, _remember_setup, _setup_key, _shared_setup, _sil_apply, _take_prefill, graph_replay, hard_raster,
                     invalidate_setups, share_setup, sil_render, sil_render_losses, tex_render, tex_render_mse,
                     vertex_color_render, visible_vertices)
from .geometry import (SOLVE_INFO_HANDOFF, _CameraNormalize, _CameraPipeline, _CameraPipelineTables, _DeformApply,
                       _DeformSolve, _PRESOLVE_SINKS, _Project, _ProjectXY, _SOLVE_PENDING, _azel_params,
                       _check_table_ids, camera_mirror, camera_normalize, camera_pipeline, camera_pipeline_azel,
                       camera_pipeline_azel_tables, camera_pipeline_tables, decode_solve_info, deform_apply,
                       deform_solve, drop_presolve_sink, project, project_xy, register_presolve_sink, solve_status)
from .flow import (_Correlation, _DeformConv2d, _FLOW_TRAINABLE, _FORWARD_ONLY, _OFLoss, _correlation_args,
                   _correlation_forward, _dconv_args, _dconv_forward, _once, correlation, deform_conv2d, of_loss)
from .fragments import (FRAGMENT_K, UV_PADDING_MODES, _Fragments, _Interpolate, _SigmoidBlend, _SoftmaxBlend, _UvTexels,
                        _det_ws, _frag_planes, _shade_storage, atlas_softmax_blend, blend_struct,
                        interpolate_face_attributes, rasterize_fragments, sigmoid_alpha_blend, softmax_rgb_blend,
                        uv_texels)
from .hypotheses import _HypTotal, _TexCycle, hypothesis_total, texture_cycle
from .mesh_terms import (_Chamfer, _EdgeLength, _EdgeRigidity, _LaplacianSmoothing, _NormalConsistency, _lengths,
                         chamfer_nearest, chamfer_sums, cot_laplacian, edge_length_sum, edge_rigidity_sum,
                         laplacian_smoothing_sum, normal_consistency_sum)
from .geodesic import (GEODESIC_LDS_MAX, GEODESIC_MAX_STEINER, GEODESIC_MEMORY, geodesic_device_workgroups,
                       geodesic_distances, geodesic_max_steiner, geodesic_memory)
from .uvatlas import UVAtlasTable, _UVAtlas, _uv_table_from_taps, uv_atlas, uv_atlas_table
from .lpips import (LPIPS_EPS, LPIPS_SCALE, LPIPS_SHIFT, _LpipsInput, _LpipsLayers, _LpipsMaskedMean, _lpips_batches,
                    _lpips_layer_host, _ptr_at, lpips_input, lpips_layer, lpips_layers, lpips_mask_weights,
                    lpips_masked_mean)
from .keypoint_loss import (KP_MAX_K, KP_MAX_N, KP_MAX_V, _CameraLoss, _KpHead, _KpWeights, _kp_f32, _kp_limits,
                            camera_loss, kp_head, kp_weights)
from .symmetry import _Symmetrize, symmetrize, symmetrize_fold
from .surface import _SurfaceSample, sample_surface, sample_surface_uv
from .neighbours import KNN_MAX_K, _KnnGather, _KnnPoints, knn_gather, knn_points
from .lighting import (SHADE_MODES, IncidenceTable, LightConstants, _LightPoints, _PhongShade, _VertexNormals,
                       incidence_table, light_constants, light_points, phong_shade, vertex_normals)
