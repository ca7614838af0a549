/*
 * acfm_hip.h -- C ABI of libacfm_hip.so, the MI355X (gfx950) implementation of ACFM's
 * differentiable-render hot path.
 *
 * The reference (fkokkinos/acfm_video_3d_reconstruction) has no C ABI for this path: its
 * boundary is Python (multiframe/nnutils/nmr.py, geom_utils.py, loss_utils.py) on top of
 * the third-party PyTorch3D 0.3.0 extension `pytorch3d._C`.  Each entry point below names
 * the reference interface it replaces; the Python operator surface that mirrors the
 * reference's own signatures lives in acfm_video_3d_reconstruction_amd/nnutils/ and binds
 * these symbols with ctypes.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless the name ends in _host;
 *     tensors are dense, row-major, fp32 / int64 / int32 as declared;
 *   - the caller owns every buffer, outputs and workspace are pre-allocated
 *     (no allocation, no host synchronisation inside: all entry points are stream-ordered
 *     and hipGraph-capturable);
 *   - `stream` is a hipStream_t passed as void* (NULL = the legacy default stream);
 *   - return value: 0 = ok, ACFM_E_* otherwise (the Python layer raises RuntimeError);
 *   - workspace sizes come from the matching *_workspace_bytes() query.
 *
 * Geometry conventions: cams [N,7] = (scale, tx, ty, qw, qx, qy, qz);
 * rendered image row/column grow with +y_p/+x_p of orthographic_proj_withz; packed face id
 * = n*F + f, -1 = empty; top-K ordered by ascending depth, ties -> smaller face id.
 */
#ifndef ACFM_HIP_H_
#define ACFM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACFM_OK 0
#define ACFM_E_BADARG 1   /* shape / parameter outside what the kernels support */
#define ACFM_E_LAUNCH 2   /* hipLaunch or a preceding asynchronous error */
#define ACFM_E_WORKSPACE 3 /* workspace too small */

#define ACFM_MAX_K 32      /* faces_per_pixel upper bound */
#define ACFM_MAX_FACES 65535 /* faces per mesh (16-bit local ids in the per-pixel lists) */
#define ACFM_DETERMINISTIC 1 /* AcfmRasterTuning.flags */
#define ACFM_STORE_F16 2
#define ACFM_RECORD_COVER 4

/* library / device info ------------------------------------------------------------- */
/* acfm_version: 1000*major + minor, 2000 here.  The 2.x signatures are incompatible with 1.x: the entry points that 1.x
 * had in a short and a long form keep the short name with the long argument list.  A caller compares the version with
 * the header it was written against before it uses any other symbol (_lib.lib() does). */
int acfm_version(void);
const char* acfm_arch(void);         /* "gfx950" */

/* 0 when `stream` is not being captured into a hipGraph, else the (non-zero) id of the capture
 * (hipStreamGetCaptureInfo).  The Python layer uses it so that a cached face setup is never shared
 * across a graph boundary (ops._SETUP); no reference counterpart. */
int acfm_stream_capture_id(void* stream, unsigned long long* id_host);

/* ---- per-kernel timing (measurement aid, off by default) -------------------------------
 * When enabled, every kernel launch inside the entry points is bracketed by hipEvents on
 * the launch stream (ring of ACFM_PROF_RING pairs).  acfm_prof_collect synchronises those
 * events and returns, per kernel id, the summed duration in ms and the launch count since
 * the last collect/enable.  Not for use under hipGraph capture.  The ring is one per process
 * (all devices and threads share it, guarded by a mutex): a diagnostic, not a product feature. */
#define ACFM_PROF_SETUP 0
#define ACFM_PROF_SIL_FWD 1
#define ACFM_PROF_SIL_BWD 2
#define ACFM_PROF_PROJ_BWD 3
#define ACFM_PROF_TEX_FWD 4
#define ACFM_PROF_HARD_FWD 5
#define ACFM_PROF_TEX_BWD 6
#define ACFM_PROF_MASK_LOSS 7
#define ACFM_PROF_MASK_LOSS_BWD 8
#define ACFM_PROF_VISIBLE 9
#define ACFM_PROF_BDS 10
#define ACFM_PROF_BDS_BWD 11
#define ACFM_PROF_PROJECT 12
#define ACFM_PROF_TEX_MSE 13
#define ACFM_PROF_TEX_MSE_BWD 14
#define ACFM_PROF_DEFORM 15
#define ACFM_PROF_DEFORM_BWD 16
#define ACFM_PROF_SOLVE 17
#define ACFM_PROF_SOLVE_BWD 18
#define ACFM_PROF_FRAG_FWD 19
#define ACFM_PROF_FRAG_BWD 20
#define ACFM_PROF_BDS_SUBSET 21
#define ACFM_PROF_STEP_TAIL 22
#define ACFM_PROF_NKERNELS 24
#define ACFM_PROF_RING 8192
int acfm_prof_enable(int on);
int acfm_prof_collect(float* ms_host, int* count_host, int n);
const char* acfm_prof_name(int id);

/* ---- projection ------------------------------------------------------------------
 * replaces geom_utils.orthographic_proj_withz / orthographic_proj / quat_rotate
 * (multiframe/nnutils/geom_utils.py:48-79, 134-152) and NeuralRenderer.project_points
 * (multiframe/nnutils/nmr.py:127-129).
 * verts [N,V,3], cams [N,7] -> proj [N,V,3] = (s*rot(q,X).xy + t, s*rot(q,X).z + offset_z) */
int acfm_project(const float* verts, const float* cams, int N, int V, float offset_z,
                 float* proj, void* stream);
/* grad_proj [N,V,3] -> grad_verts [N,V,3] (may be NULL), grad_cams [N,7] (may be NULL) */
int acfm_project_backward(const float* verts, const float* cams, const float* grad_proj, int N,
                          int V, float* grad_verts, float* grad_cams, void* stream);
/* The (x, y) part only, [N,V,2]: geom_utils.orthographic_proj (geom_utils.py:48-59) and
 * NeuralRenderer.project_points (nmr.py:127-129) without the [:, :, :2] slice and, backward, without the
 * zero-padded [N,V,3] gradient the slice's autograd builds. */
int acfm_project_xy(const float* verts, const float* cams, int N, int V, float offset_z, float* proj_xy,
                    void* stream);
int acfm_project_xy_backward(const float* verts, const float* cams, const float* grad_proj_xy, int N, int V,
                             float* grad_verts, float* grad_cams, void* stream);

/* ---- template deformation --------------------------------------------------------------
 * replaces the per-frame Cholesky solve of multiframe/main.py:586-609 (== predictor.py:260-276,
 * 313-315, monocular/main.py:204-218) once P = (L^T L + A^T A)^-1 A^T [V,K_h] is known
 * (factorised once per optimiser step, see deform.py):  verts[n] = mean_v + P delta[n].
 *   mean_v [V,3], P [V,K_h], delta [N,K_h,3] -> verts [N,V,3]   (f32 MFMA 16x16x4)
 * backward: grad_verts [N,V,3] -> grad_delta [N,K_h,3] = P^T g_n, grad_mean [V,3] = sum_n g_n,
 *   grad_P [V,K_h] = sum_n g_n delta_n^T (each may be NULL).  grad_delta and grad_mean come from one launch of
 *   ceil(K_h/16) ceil(3N/16) + ceil(3V/1024) workgroups: ACFM_E_BADARG if that passes 2^31 - 1. */
int acfm_deform_apply(const float* mean_v, const float* P, const float* delta, int N, int V, int Kh,
                      float* verts, void* stream);
int acfm_deform_apply_backward(const float* P, const float* delta, const float* grad_verts, int N, int V,
                               int Kh, float* grad_delta, float* grad_mean, float* grad_P, void* stream);
/* The pre-solve sums of a frame-sharded step in double (the buffer [G = sum_n g_n delta_n^T | sum_n g_n | ..]
 * that the ranks all-reduce): G64 [V,K_h] and, optionally, mean64 [V,3], accumulated in double in a fixed order;
 * grad_P (optional) = G64 rounded to float, the same figure acfm_deform_apply_backward's grad_P approximates in
 * float arithmetic.  d lbs = acfm_deform_solve_backward(G) amplifies the rounding of G by the conditioning of the
 * system: with doubles through the exchange and ONE rounding behind it, the split of the frames over the ranks no
 * longer shows in the handle-weight gradient. */
int acfm_deform_presolve_sums_f64(const float* delta, const float* grad_verts, int N, int V, int Kh, double* G64,
                                  double* mean64, float* grad_P, void* stream);
/* The symmetric template (--symmetric True, mesh_net.py:462-484): the learned mean shape holds the n_indept rows on the
 * mirror plane and the n_sym right-hand rows, the shape that is deformed and rendered appends the right-hand rows once
 * more, mirrored.
 * full[b] = [ half[b] ; (-x, y, z) of half[b][n_half - n_sym : n_half] ],  n_half = n_indept + n_sym,
 * half [B,n_half,3] -> full [B,n_half + n_sym,3]   (mesh_net.py:573-591) */
int acfm_symmetrize(const float* half, int B, int n_indept, int n_sym, float* full, void* stream);
/* grad_half[b][i] = g[b][i] for i < n_indept,
 *                 = g[b][i] + (-1, 1, 1) * g[b][i + n_sym] for i >= n_indept.
 * One float addition per element, every element written.
 * Both: one thread per output float, no atomics, no workspace; bit-reproducible and equal, bit for bit, to the torch
 * lines they replace.  ACFM_E_BADARG for B < 1, a negative count, n_half == 0 or 3 B (n_half + n_sym) > 2^31 - 1;
 * n_sym == 0 is a plain copy. */
int acfm_symmetrize_backward(const float* grad_full, int B, int n_indept, int n_sym, float* grad_half, void* stream);

/* ---- correlation cost volume -------------------------------------------------------------
 * replaces correlation_cuda.forward as MaskFlownet calls it (multiframe/data/optical_flow/model/
 * correlation_package/correlation_cuda_kernel.cu:73-147, correlation.py:20-37; MaskFlownet.py:116,
 * 416: pad_size = max_displacement = md, kernel_size = 1, stride1 = stride2 = 1, corr_multiply = 1):
 *   f1, f2 [N,C,H,W] f32 -> out [N,(2md+1)^2,H,W],
 *   out[n,(tj+md)(2md+1)+(ti+md),y,x] = mean_c f1[n,c,y,x] f2[n,c,y+tj,x+ti]  (zero outside), md in 1..4.
 * The flow network is frozen in ACFM (flows are precomputed by the optical_flow scripts); the backward below is for
 * fine-tuning it (the reference's CorrelationFunction.backward, correlation.py:38-52). */
int acfm_correlation_forward(const float* f1, const float* f2, int N, int C, int H, int W, int md, float* out,
                             void* stream);
/* Host only, launches nothing: the number of workgroups the forward splits the channel range of one 16 x 16 tile over
 * (whole chunks of 8 channels, so at most ceil(C / 8)).  1: every output element is stored once, bit-reproducible;
 * > 1 (fewer than 768 tiles in the batch): zero fill and float atomics.  0 for arguments the forward refuses. */
int acfm_correlation_channel_split(int N, int C, int H, int W);
/* grad_out [N,(2md+1)^2,H,W] -> grad_f1, grad_f2 [N,C,H,W]; either may be NULL (that side is not computed, and its
 * partner map -- f2 for grad_f1, f1 for grad_f2 -- need not be given).  With d = (tj+md)(2md+1)+(ti+md):
 *   grad_f1[n,c,y,x] = 1/C sum_d grad_out[n,d,y,x]       f2[n,c,y+tj,x+ti]   (0 outside)
 *   grad_f2[n,c,y,x] = 1/C sum_d grad_out[n,d,y-tj,x-ti] f1[n,c,y-tj,x-ti]   (0 where the shifted pixel is outside)
 * Gathers in a fixed order, no atomics, no zero fill: bit-reproducible, and a side computed alone has the bits of the
 * same side computed with the other.  Same argument ranges as the forward. */
int acfm_correlation_backward(const float* grad_out, const float* f1, const float* f2, int N, int C, int H, int W,
                              int md, float* grad_f1, float* grad_f2, void* stream);

/* ---- deformable convolution --------------------------------------------------------------
 * replaces torchvision.ops.deform_conv2d as MaskFlownet calls it (MaskFlownet.py:36-37, 488-492, 558-640: kernel 3x3,
 * stride 1, padding 1, dilation 1, groups 1, one offset group, no mask), fp32:
 *   input [N,Cin,H,W], offset [N,18,H,W], weight [Cout,Cin,3,3] (torchvision's layout, read as it is), bias [Cout] or
 *   NULL -> out [N,Cout,H,W],
 *   out[n,co,y,x] = bias[co] + sum_{ci,ky,kx} weight[co,ci,ky,kx] S(input[n,ci], y+ky-1+off[n,2t,y,x], x+kx-1+off[n,2t+1,y,x]),
 *   t = 3 ky + kx; S(plane,h,w) = 0 for h <= -1, h >= H, w <= -1 or w >= W, else the bilinear interpolation of the four
 *   neighbours with those outside the map counted as 0.
 * shared_offset != 0: offset is [N,2,H,W] and every tap reads its channels 0 (rows) and 1 (columns): the result of
 * offset.repeat(1, 9, 1, 1) (MaskFlownet's unsqueeze(1), repeat_interleave(.., 9, 1), view) handed to the 18-channel
 * form, bit for bit, without that copy.
 * Cin, Cout >= 1 arbitrary.  The columns are never written to device memory and nothing is added atomically: results
 * are bit-reproducible.  The flow network is frozen in ACFM; the backward below is for fine-tuning it. */
int acfm_deform_conv2d_forward(const float* input, const float* offset, const float* weight, const float* bias, int N,
                               int Cin, int H, int W, int Cout, int shared_offset, float* out, void* stream);
/* Host only, launches nothing: the output channels per workgroup the forward picks for this shape -- 64, 32 or 16, the
 * widest that is not wider than Cout needs and still leaves 256 workgroups (the split is over Cout only: the bits of an
 * output element do not depend on it).  0 for arguments the forward refuses. */
int acfm_deform_conv2d_channel_tile(int N, int H, int W, int Cout);
/* Backward: grad_out [N,Cout,H,W] -> grad_input [N,Cin,H,W], grad_offset [N,18,H,W] (shared_offset: [N,2,H,W], the sum
 * over the nine taps), grad_weight [Cout,Cin,3,3], grad_bias [Cout]; every one of the four may be NULL and is then not
 * computed (no weight-gradient kernel for a frozen weight).  Nothing of the forward is saved: the sampling is recomputed
 * from input and offset.  At an integer sample coordinate the offset gradient is that of the floor cell (the forward
 * difference towards the +1 neighbour, torchvision's convention); it is 0 for a position outside (-1,H) x (-1,W).
 *   grad_input is a data-dependent scatter: float atomics into a buffer the call zero-fills -- NOT bit-reproducible;
 *   grad_offset, grad_weight and grad_bias are reduced in a fixed order: bit-reproducible.
 * ws: acfm_deform_conv2d_backward_workspace_bytes(N, Cin, H, W, Cout) bytes on the device, any contents (the partial
 * weight gradients of the pixel ranges); needed only with grad_weight (NULL: ACFM_E_BADARG, too small:
 * ACFM_E_WORKSPACE).  The query returns 0 for arguments out of range.  Same argument ranges as the forward. */
size_t acfm_deform_conv2d_backward_workspace_bytes(int N, int Cin, int H, int W, int Cout);
int acfm_deform_conv2d_backward(const float* grad_out, const float* input, const float* offset, const float* weight,
                                int N, int Cin, int H, int W, int Cout, int shared_offset, float* grad_input,
                                float* grad_offset, float* grad_weight, float* grad_bias, void* ws, size_t ws_bytes,
                                void* stream);

/* ---- optical-flow loss -----------------------------------------------------------------
 * replaces the tail of loss_utils.optical_flow_loss (multiframe/nnutils/loss_utils.py:445-474):
 *   proj [B*T,V,3] projected vertices (proj_fn output, x/y in [-1,1]), flows [B*T,H,W,2] GT flow
 *   images, vis [B*T,V] visible-vertex bitmap of the hard raster  ->  loss [B,T-1]:
 *   sum over the kept vertices of |gt - (pix[k-1] - pix[k])|_1 / H / (kept + 1), gt = nearest pixel
 *   (grid_sample nearest, align_corners False, zeros), kept = visible in frame k and gt != 0;
 *   count [B,T-1] is saved for the backward pass (grad_loss [B,T-1] -> grad_proj [B*T,V,3]).
 * The GT flows are read as the data loader holds them (multiframe/main.py:676-686 flips them in time, masks them and
 * repeats them for the G hypotheses every step; the loss reads V pixels per frame): flows [clips,T,H,W,2], clip c of the
 * B = G*clips rendered ones reads clip c % clips, frame k reads frame T-1-k if flip_t, and the value is multiplied by
 * masks [clips*T,H,W] at the same pixel of frame k if masks is not NULL.  masks = NULL, clips = B, flip_t = 0: flows
 * [B*T,H,W,2] as they are. */
int acfm_of_loss(const float* proj, const float* flows, const float* masks, const uint8_t* vis, int B, int T, int V,
                 int H, int W, int clips, int flip_t, float* loss, float* count, void* stream);
int acfm_of_loss_backward(const float* proj, const float* flows, const float* masks, const uint8_t* vis,
                          const float* count, const float* grad_loss, int B, int T, int V, int H, int W, int clips,
                          int flip_t, float* grad_proj, void* stream);

/* ---- camera hypothesis pipeline --------------------------------------------------------
 * replaces the camera decode + mirror_cameras + transform_cameras chain of ShapeTrainer.forward /
 * warmup (multiframe/main.py:551-584, 452-466; the functions at :97-138): per camera row
 *   (s, t, q) = (relu(decay*e0 + 1) + 1e-12, e1..2, normalize(e3..6));
 *   blended by the frame's mirror flag with (s, -tx, ty, standardize(q_y(pi) * standardize(q)));
 *   then (s*a, tx*a + dx, ty*a + dy, q) blended by the frame's transform flag.
 *   emb [R,7] f32 (R = G*N rows, row r belongs to frame r % N), mirror_flag [N] i64,
 *   transforms [N,4] f32 (a, dx, dy, flag) -> cams [R,7];  backward: grad_cams -> grad_emb. */
int acfm_camera_pipeline(const float* emb, const int64_t* mirror_flag, const float* transforms, int R, int N,
                         float scale_lr_decay, float* cams, void* stream);
int acfm_camera_pipeline_backward(const float* emb, const int64_t* mirror_flag, const float* transforms,
                                  const float* grad_cams, int R, int N, float scale_lr_decay, float* grad_emb,
                                  void* stream);
/* pose of the horizontally flipped image of decoded cameras [R,7] (multiframe/main.py:97-125 with the flag set; the
 * texture branch renders every frame once more under it, main.py:627-636): (s, -tx, ty, standardize(q_y(pi) *
 * standardize(q))).  Forward only: the texture render sends no gradient to its cameras. */
int acfm_camera_mirror(const float* cams, int R, float* out, void* stream);
/* the same straight from the per-hypothesis embedding tables (multiframe/nnutils/mesh_net.py:436-444: one
 * nn.Embedding(frames, 7) per hypothesis; main.py:551-570 looks every one of them up and stacks / gathers the rows):
 * row r = g*N + n reads tables[selected ? selected[r] : g][frames_idx[n]] (tables: HOST array of n_tables <= 32 device
 * pointers to [n_frames,7] f32; selected [R] i64 or NULL: main.py:541-548's top-k choice).  backward: grad_tables[t]
 * ([n_frames,7], HOST array of device pointers, NULL entries skipped) are WRITTEN -- zero except the rows the batch
 * looked up, like nn.Embedding's dense gradient.
 * Out-of-range ids (frames_idx outside [0, n_frames), selected outside [0, n_tables): nn.Embedding raises there) are never
 * dereferenced: the forward writes a NaN camera for such a row, the backward skips it. */
int acfm_camera_pipeline_tables(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                const int64_t* selected, const int64_t* mirror_flag, const float* transforms, int R,
                                int N, float scale_lr_decay, float* cams, void* stream);
int acfm_camera_pipeline_tables_backward(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                         const int64_t* selected, const int64_t* mirror_flag, const float* transforms,
                                         const float* grad_cams, int R, int N, float scale_lr_decay,
                                         void* const* grad_tables, void* stream);
/* the four entry points above for the 6-float embedding of --az_el_cam (multiframe/main.py:442-450, 554-566;
 * nnutils/mesh_net.py:310-385, 405-422): emb / tables / grad_emb / grad_tables have 6 columns (scale, tx, ty, azimuth,
 * elevation, cyclo-rotation), everything else is as above.  Per row, with the ranges in RADIANS:
 *   s = scale_lr_decay*e0 + scale_bias (no relu: a negative scale passes through), t = e1..2;
 *   az = az_range*e3, el = pi - el_range*e4, cyc = cyc_range*e5;
 *   q = q_cyc (x) (q_el (x) q_az), q_az = (cos az/2, 0, sin az/2, 0), q_el = (cos el/2, sin el/2, 0, 0),
 *   q_cyc = (cos cyc/2, 0, 0, sin cyc/2): Hamilton products on (w, x, y, z), not renormalised;
 *   then the same mirror blend and transform blend.  The parameters are per call; the library keeps none.
 * One launch per call, the tables' backward included: it fills the dense gradients cell by cell, each the sum of the
 * batch rows that looked it up in a fixed order (no atomics, no zero fill in front; bit-reproducible). */
int acfm_camera_pipeline_azel(const float* emb, const int64_t* mirror_flag, const float* transforms, int R, int N,
                              float scale_lr_decay, float scale_bias, float az_range, float el_range, float cyc_range,
                              float* cams, void* stream);
int acfm_camera_pipeline_azel_backward(const float* emb, const int64_t* mirror_flag, const float* transforms,
                                       const float* grad_cams, int R, int N, float scale_lr_decay, float scale_bias,
                                       float az_range, float el_range, float cyc_range, float* grad_emb, void* stream);
int acfm_camera_pipeline_azel_tables(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                     const int64_t* selected, const int64_t* mirror_flag, const float* transforms, int R,
                                     int N, float scale_lr_decay, float scale_bias, float az_range, float el_range,
                                     float cyc_range, float* cams, void* stream);
int acfm_camera_pipeline_azel_tables_backward(const void* const* tables, int n_tables, int n_frames,
                                              const int64_t* frames_idx, const int64_t* selected,
                                              const int64_t* mirror_flag, const float* transforms,
                                              const float* grad_cams, int R, int N, float scale_lr_decay,
                                              float scale_bias, float az_range, float el_range, float cyc_range,
                                              void* const* grad_tables, void* stream);

/* cam = (s, tx, ty, q / max(|q|, 1e-12)) of a raw [N,7] camera parameter: the per-iteration
 * torch.cat([scale, trans, F.normalize(quat)]) of the refinement loop (nnutils/predictor.py:301-308). */
int acfm_camera_normalize(const float* cam_raw, int N, float* cams, void* stream);
int acfm_camera_normalize_backward(const float* cam_raw, const float* grad_cams, int N, float* grad_raw,
                                   void* stream);

/* ---- template deformation solve ------------------------------------------------------
 * replaces the per-frame torch.cholesky / torch.cholesky_solve of multiframe/main.py:586-609
 * (also optimization/main.py:474-496, nnutils/predictor.py:260-276): with A = softmax(lbs, dim 0)^T
 * [K_h,V] (mesh_net.py:597-599) and the dense cotangent Laplacian L [V,V] of the mean shape,
 *   P = (L^T L + A^T A)^-1 A^T   [V,K_h]
 * by a blocked fp64 Cholesky on the matrix cores; once per optimiser step for all frames
 * (pred_v_n = mean_v + P delta_n, acfm_deform_apply).  K_h <= 128 and V <= 16384 (ACFM_E_BADARG beyond; the
 * workspace query returns 0): the handles are right-hand sides in panels of 32, ceil(K_h / 32) tile rows of the same
 * single launch, and up to 32 handles compute what one panel always did, bit for bit.
 * The workspace keeps the factor: acfm_deform_solve_backward turns grad_P [V,K_h] into
 * grad_lbs [V,K_h] (L carries no gradient, geom_utils.py:245).  acfm_deform_solve_info copies
 * the factorisation status to the host and synchronises the stream: 0 = ok; bit ACFM_SOLVE_INFO_HANDOFF set = a
 * hand-off wait of the single-launch factorisation expired (a starved wave: P holds NaNs; re-run the solve);
 * otherwise the low bits are 1 + first row of the 32-row tile with a non-positive pivot (the reference's
 * torch.cholesky raises there).  acfm_deform_solve_info_offset: byte offset of that int32 status word inside the
 * workspace, for callers that copy it without blocking (ops.py polls it that way between steps).  The offset depends
 * on V alone, and acfm_deform_solve_info accepts any workspace of at least acfm_deform_solve_workspace_bytes(V, 1). */
#define ACFM_SOLVE_INFO_HANDOFF 0x40000000
size_t acfm_deform_solve_workspace_bytes(int V, int Kh);
int acfm_deform_solve(const float* L, const float* lbs, int V, int Kh, float* P, void* ws, size_t ws_bytes,
                      void* stream);
int acfm_deform_solve_backward(const float* grad_P, int V, int Kh, void* ws, size_t ws_bytes, float* grad_lbs,
                               void* stream);
int acfm_deform_solve_info(const void* ws, size_t ws_bytes, int V, int* info_host, void* stream);
size_t acfm_deform_solve_info_offset(int V);

/* ---- rasterisation workspace -------------------------------------------------------
 * Scratch of one render call of N meshes with V verts and F faces each at H x H pixels
 * (face records, NDC verts, per-mesh boxes, tile schedule, gradient scratch). */
size_t acfm_raster_workspace_bytes(int N, int V, int F, int H);
/* Vertices per mesh: the face setup of every render entry point (sil / sil_loss / tex / vertex_color / hard_raster /
 * rasterize_fragments) keeps a mesh's projected vertices in dynamic LDS, 12 B each, next to its tile counters (4 B per
 * 8x8-pixel block while H <= 512) and, while they fit in 64 KB, its face slice's coarse masks (4 B x ceil(H/16)^2 x
 * slice faces / 32, a slice = F / 4, 8 or 16 faces rounded up to 64), and launches with at most 150 KB of it (the CU
 * has 160 KB; launches past 64 KB need no opt-in on this runtime and are exercised by the tests).  Beyond that the
 * call returns ACFM_E_BADARG.  Bird template (F = 1280), two meshes, H = 64: 12 V + 512 <= 153,600, V <= 12,757. */

/* Per-call launch tuning of the raster entry points (pure speed: results never depend on it, `flags` apart).
 * NULL = the defaults.  There is no process-global tuning state in the library.
 *   split_mode: the heaviest 8x8 blocks of a launch are rendered by four workgroups each (a launch lasts at least as
 *               long as its longest block: all of a small launch's heavy blocks, the top few dozen of a large one);
 *               < 0 automatic: decided on the device from the cost histogram, a block is split when its cost exceeds
 *               (-split_mode / 4) x the mean work per wave slot (default -5: 1.25 x), 0 never, 1 always;
 *   grid_div:   workgroups per XCD group = entries / div for [0] the K-nearest forward, [1] the
 *               nearest-face (K = 1) forward, [2] the silhouette backward; 0 = default (4, 2, 4).
 *   flags:      bit 0 = deterministic silhouette backward: vertex gradients are accumulated in 64-bit fixed point
 *               (2^-36 units) with integer atomics, so the sums do not depend on the order in which blocks are
 *               served -- two runs are bit-identical, within 1e-6 of the default floating-point atomics (which are
 *               reproducible only to ~1e-6 relative);
 *               bit 1 = ACFM_STORE_F16 (BASELINE config 5, "fp16 render with fp32 loss accumulate"): the buffers
 *               declared `void*` [real] below hold IEEE half instead of float (rendered masks, images, silhouettes,
 *               atlases and the reference masks / distance transforms / images of the fused operators), and
 *               pix_to_face is an int32 [N,H,H] nearest-face plane (k_out must be 1).  Only storage changes: every
 *               accept / reject decision, depth, blend and loss sum stays fp32, so face ids are identical to the
 *               fp32 build and losses differ by the half rounding of what is stored (IoU drift < 1e-4).
 *               Gradients (grad_mask, grad_losses, grad_atlas, grad_verts, grad_cams) are always float.
 *               These two bits are the only fields that are not pure speed.
 *               bit 2 = ACFM_RECORD_COVER (pure speed): acfm_sil_forward / acfm_sil_loss_forward also leave, in the
 *               workspace, the nearest face that COVERS each pixel -- the answer of the hard K = 1 render of the same
 *               geometry (nmr.py:173-200: blur 0, clipped barycentrics), found during the walk the K-nearest render
 *               does anyway.  A texture render that takes the workspace over with ws_ready = 2 shades from that plane
 *               instead of binning and walking the faces again: identical outputs, bit for bit.
 * A backward call must pass the tuning of the forward whose workspace it takes over. */
typedef struct AcfmRasterTuning {
  int split_mode;
  int grid_div[3];
  int flags;
} AcfmRasterTuning;

/* ---- soft silhouette ---------------------------------------------------------------
 * replaces NeuralRenderer.forward, mask branch (multiframe/nnutils/nmr.py:143-172):
 * proj_fn -> y flip -> view (R=diag(-1,1,1), T=(0,0,2.732)) -> PyTorch3D
 * rasterize_meshes(K, blur_radius, bin_size=None) -> sigmoid_alpha_blend(sigma).
 *   verts_world [N,V,3] f32, faces [N,F,3] i64, cams [N,7] f32
 *   -> mask [N,H,H] f32, pix_to_face [N,H,H,k_out] i64 (packed ids, ascending depth, -1 empty)
 *      k_out = K: every kept face, as PyTorch3D returns them; k_out = 1: only the nearest-face
 *      plane (the K faces are still found and blended; it is the one slot the reference's
 *      callers read, loss_utils.py:214,431, and saves 8*(K-1) bytes per pixel of HBM writes)
 *   -> kth [N,H,H] u64 (optional, NULL to skip): state for acfm_sil_backward -- the
 *      (depth bits << 32 | face) key of the K-th kept face where K faces were kept, else ~0; defined where
 *      mask != 0 (all the backward reads) -- the 8x8 blocks no face comes near are not written
 *   -> vis [N,V] u8 (optional): 1 for every vertex of a face that is nearest in some pixel,
 *      i.e. the visible-vertex set of loss_utils.bds_loss (:214-224), fused into the raster
 * K in {2,4,8,10,20,32}.
 *
 * AcfmSilExtras, the last argument but one of the four silhouette entry points (acfm_sil_forward, acfm_sil_backward,
 * acfm_sil_loss_forward, acfm_sil_loss_backward): what the reference's callers do NEXT TO the render with the same
 * vertices and cameras.  extras == NULL, or a NULL field: not wanted.
 *   proj_xy         forward out [N,V,2]: NeuralRenderer.project_points(vertices, cams) (nmr.py:127-129), which the
 *                   trainer calls on the prediction it has just rendered (main.py:715, predictor.py:319): the face
 *                   setup projects the vertices anyway, so it hands (x, y) out instead of a second projection kernel;
 *   grad_proj_xy    backward in [N,V,2]: the upstream gradient of that proj_xy (the boundary loss's), added inside the
 *                   ONE projection backward of the silhouette render -- no second projection backward, no sum of two
 *                   [N,V,3] / [N,7] gradients afterwards;
 *   tex_*           forward: the pair renderer(...) / tex_renderer(...) on one prediction (main.py:620-626): besides its
 *                   own outputs the silhouette kernel stores the CONSTANT outputs of that texture render -- imgs 0, sil 0,
 *                   pix_to_face -1, texel_idx -1 -- on the 8x8 blocks no face comes near (~80 % of a frame) into the
 *                   caller's buffers for them (all four or none; needs ACFM_RECORD_COVER and float storage);
 *                   acfm_tex_forward(ws_ready = 3) on the same workspace then writes only the blocks with work. */
typedef struct AcfmSilExtras {
  float* proj_xy;
  const float* grad_proj_xy;
  float* tex_imgs;            /* [N,3,H,H] */
  float* tex_sil;             /* [N,H,H] */
  int64_t* tex_pix_to_face;   /* [N,H,H,1] */
  int32_t* tex_texel_idx;     /* [N,H,H] */
} AcfmSilExtras;
int acfm_sil_forward(const float* verts_world, const int64_t* faces, const float* cams, int N,
                     int V, int F, int H, int K, int k_out, float blur_radius, float sigma,
                     float offset_z, void* mask /* [real] */, void* pix_to_face /* int64, or the int32 plane */,
                     uint64_t* kth, uint8_t* vis, void* ws, size_t ws_bytes, const AcfmRasterTuning* tuning,
                     const AcfmSilExtras* extras, void* stream);

/* replaces autograd through SoftSilhouetteShader + pytorch3d._C.rasterize_meshes_backward
 * (dists path) + the projection chain.  mask / kth are the forward's outputs;
 * grad_mask [N,H,H] -> grad_verts [N,V,3], grad_cams [N,7] (either may be NULL).
 * ws_from_forward != 0: `ws` is the untouched workspace of the matching acfm_sil_forward call
 * (same verts/faces/cams/H/blur) and the face setup is not repeated; 0: it is rebuilt here. */
int acfm_sil_backward(const float* verts_world, const int64_t* faces, const float* cams,
                      const void* mask /* [real] */, const uint64_t* kth, const float* grad_mask, int N, int V,
                      int F, int H, float blur_radius, float sigma, float offset_z,
                      float* grad_verts, float* grad_cams, void* ws, size_t ws_bytes,
                      int ws_from_forward, const AcfmRasterTuning* tuning, const AcfmSilExtras* extras, void* stream);

/* ---- fused soft silhouette + silhouette losses (opt-in) --------------------------------
 * acfm_sil_forward and acfm_mask_losses as ONE operator: the reference consumes the rendered mask at once
 * (multiframe/main.py:644-645, 715-716: l1_loss / edt_loss of mask_pred; predictor.py:317-320), so the loss terms
 * are summed in the raster kernel's epilogue (per-block partial sums, then summed per mesh in fixed order together
 * with sum(gt): deterministic, no atomics) and the backward forms d loss / d mask on the fly from gt / edt and
 * the per-mesh gradients -- the separate passes over the mask (acfm_mask_losses, acfm_mask_losses_backward)
 * and the [N,H,H] grad_mask buffer disappear.  Same outputs as acfm_sil_forward plus
 *   losses [N,4] = (mean|m - gt|, sum m gt, sum(m + gt - m gt), mean edt m)   (acfm_mask_losses' vector);
 * gt / edt [ref_batch,H,H] (either may be NULL = zeros), prediction n <-> reference n % ref_batch.
 * backward: grad_losses [N,4] -> grad_verts / grad_cams. */
int acfm_sil_loss_forward(const float* verts_world, const int64_t* faces, const float* cams, const void* gt /* [real] */,
                          const void* edt /* [real] */, int ref_batch, int N, int V, int F, int H, int K, int k_out,
                          float blur_radius, float sigma, float offset_z, void* mask /* [real] */, void* pix_to_face,
                          uint64_t* kth, uint8_t* vis, float* losses, void* ws, size_t ws_bytes,
                          const AcfmRasterTuning* tuning, const AcfmSilExtras* extras, void* stream);
int acfm_sil_loss_backward(const float* verts_world, const int64_t* faces, const float* cams, const void* mask,
                           const uint64_t* kth, const void* gt, const void* edt, int ref_batch,
                           const float* grad_losses, int N, int V, int F, int H, float blur_radius, float sigma,
                           float offset_z, float* grad_verts, float* grad_cams, void* ws, size_t ws_bytes,
                           int ws_from_forward, const AcfmRasterTuning* tuning, const AcfmSilExtras* extras,
                           void* stream);

/* ---- hard rasteriser (K = 1, blur 0) -------------------------------------------------
 * replaces OF_NeuralRenderer.forward (multiframe/nnutils/nmr.py:224-238): verts are
 * ALREADY projected by proj_fn; no y flip; view R=diag(-1,1,1), T=(0,0,2.732).
 * -> pix_to_face [N,H,H,1] i64 */
int acfm_hard_raster(const float* verts_proj, const int64_t* faces, int N, int V, int F, int H,
                     int64_t* pix_to_face, uint8_t* vis /* optional [N,V], as above */, void* ws,
                     size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream);

/* ---- rasterizer fragments ------------------------------------------------------------
 * PyTorch3D 0.3.0 rasterize_meshes (the naive path, which oracle_rasterize restates) over
 * vertices already in NDC / view space: verts_ndc [N,V,3] = (NDC x, NDC y, view z), faces [N,F,3] i64.  Pixel
 * (y, x) of the H x H image sits at NDC (pix_to_ndc(H-1-x), pix_to_ndc(H-1-y)); a face is kept at a pixel when its
 * interpolated depth is >= 0 and the pixel is inside it or its squared distance to the face is < blur_radius;
 * the K nearest are kept in ascending (depth, packed id) order.  Per (pixel, slot), -1 in all four where empty:
 *   -> pix_to_face [N,H,H,K] i64   packed n*F + f
 *   -> zbuf        [N,H,H,K] f32   interpolated view z (clipped barycentrics with clip_bary)
 *   -> bary        [N,H,H,K,3] f32 barycentrics, clamped to [0,1] and renormalised by max(sum, 1e-5) with clip_bary
 *                                  (16-byte aligned)
 *   -> dists       [N,H,H,K] f32   squared distance to the nearest edge, negative inside
 * K in {1,2,4,8,10,20,32}; tuning flags bit 1 (half storage) is refused. */
size_t acfm_rasterize_fragments_workspace_bytes(int N, int V, int F, int H);
int acfm_rasterize_fragments(const float* verts_ndc, const int64_t* faces, int N, int V, int F, int H, int K,
                             float blur_radius, int clip_bary, int64_t* pix_to_face, float* zbuf, float* bary,
                             float* dists, void* ws, size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream);

/* RasterizeMeshesBackward: upstream gradients of zbuf / bary / dists (each may be NULL: that path
 * is skipped, nothing is read) -> grad_verts [N,V,3] (d / d verts_ndc, overwritten).  dists: PointLineDistanceBackward
 * of the arg-min edge with the clamped segment parameter held constant, sign -1 inside; zbuf: d zbuf / d z_i = b_i
 * plus z_i into the gradient of b_i; bary: through the clamp-and-renormalise (clip_bary) and w_i = edge_i / (area +
 * kEps), area included.  pix_to_face is the forward's; ws_from_forward != 0: ws holds the face setup of that forward
 * (same verts / faces / H / blur / tuning).  Tuning flags bit 0: deterministic -- every contribution is split into
 * two integers (units 2^-4 and 2^-40) summed with integer atomics: bit-identical runs, range |gradient| < 2^59,
 * resolution 2^-40 (barycentric gradients scale like 1 / area and reach 1e9 near degenerate faces). */
int acfm_rasterize_fragments_backward(const float* verts_ndc, const int64_t* faces, const int64_t* pix_to_face,
                                      const float* grad_zbuf, const float* grad_bary, const float* grad_dists, int N,
                                      int V, int F, int H, int K, float blur_radius, int clip_bary, float* grad_verts,
                                      void* ws, size_t ws_bytes, int ws_from_forward,
                                      const AcfmRasterTuning* tuning, void* stream);

/* ---- shaders over fragments ---------------------------------------------------------------
 * The shading half of PyTorch3D 0.3.0's mesh renderer over the outputs of
 * acfm_rasterize_fragments, flattened: P = N*H*W pixels, K slots per pixel (K in {1,2,4,8,10,20,32}),
 * pix_to_face [P,K] i64 (packed n*F + f, -1 empty), dists / zbuf [P,K], bary [P,K,3], RGBA [P,4] (16-byte aligned).
 * Tuning flags bit 1 (half storage) is refused; bit 0 makes the two scattering backwards (grad_atlas,
 * grad_face_attrs) bit-reproducible (integer-split sums as acfm_rasterize_fragments_backward, in `ws`, which then
 * needs 16 bytes per gradient element; ws is unused otherwise and may be NULL).  Every gradient output is nullable
 * (that path is skipped) and overwritten. */
typedef struct AcfmBlendParams {   /* BlendParams + the znear / zfar of softmax_rgb_blend (host structure) */
  float sigma;
  float gamma;
  float background[3];
  float znear;
  float zfar;
} AcfmBlendParams;

/* sigmoid_alpha_blend: RGB = colors[p,0,:] (1 where colors is NULL: SoftSilhouetteShader), A = 1 - prod_k (1 - p_k),
 * p_k = sigmoid(-dists / sigma) [pix_to_face >= 0].  Backward: grad_dists [P,K] by the closed form
 * -(1 - A) p_k / sigma (App-A.5), grad_colors [P,K,3] (slot 0 only, zeros elsewhere). */
int acfm_sigmoid_alpha_blend(const int64_t* pix_to_face, const float* dists, const float* colors, size_t P, int K,
                             float sigma, float* rgba, const AcfmRasterTuning* tuning, void* stream);
int acfm_sigmoid_alpha_blend_backward(const int64_t* pix_to_face, const float* dists, const float* grad_rgba,
                                      size_t P, int K, float sigma, float* grad_dists, float* grad_colors,
                                      const AcfmRasterTuning* tuning, void* stream);
/* softmax_rgb_blend (App-A.6, A.10).  Colours come from exactly one source: `colors` [P,K,3], or `atlas`
 * [F_packed,R,R,3] sampled at `bary` as TexturesAtlas.sample_textures does (no [P,K,3] texel tensor), times
 * `ambient` [N,3] of mesh p / pix_per_mesh when given.  Backward: grad_dists, grad_zbuf [P,K], grad_colors [P,K,3]
 * (dense source) or grad_atlas [F_packed,R,R,3] (atlas source, scattered); nothing flows to bary or ambient. */
int acfm_softmax_rgb_blend(const int64_t* pix_to_face, const float* dists, const float* zbuf, const float* bary,
                           const float* colors, const float* atlas, int R, int F_packed, const float* ambient,
                           size_t P, int K, int pix_per_mesh, const AcfmBlendParams* blend, float* rgba,
                           const AcfmRasterTuning* tuning, void* stream);
int acfm_softmax_rgb_blend_backward(const int64_t* pix_to_face, const float* dists, const float* zbuf,
                                    const float* bary, const float* colors, const float* atlas, int R, int F_packed,
                                    const float* ambient, size_t P, int K, int pix_per_mesh,
                                    const AcfmBlendParams* blend, const float* grad_rgba, float* grad_dists,
                                    float* grad_zbuf, float* grad_colors, float* grad_atlas, void* ws,
                                    size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream);
/* interpolate_face_attributes: face_attrs [F_packed,3,D] -> out [P,K,D] = sum_i bary_i face_attrs[f,i,:], 0 in empty
 * slots.  Backward: grad_bary [P,K,3], grad_face_attrs [F_packed,3,D] (scattered). */
int acfm_interpolate_face_attributes(const int64_t* pix_to_face, const float* bary, const float* face_attrs,
                                     size_t P, int K, int F_packed, int D, float* out,
                                     const AcfmRasterTuning* tuning, void* stream);
int acfm_interpolate_face_attributes_backward(const int64_t* pix_to_face, const float* bary, const float* face_attrs,
                                              const float* grad_out, size_t P, int K, int F_packed, int D,
                                              float* grad_bary, float* grad_face_attrs, void* ws, size_t ws_bytes,
                                              const AcfmRasterTuning* tuning, void* stream);
/* TexturesUV.sample_textures (App-A.11): texels [P,K,3] = grid_sample(maps[n] flipped along its height, 2 uv - 1,
 * bilinear) at uv = sum_i bary_i faces_verts_uvs[f,i,:] ((0,0) in empty slots, which are not zeroed), with
 * faces_verts_uvs [F_packed,3,2], maps [N,Hm,Wm,3] read in place and n = p / pix_per_mesh (P = N pix_per_mesh).
 * align_corners 0 / 1 (then Hm, Wm >= 2); padding_mode 0 = "border", 1 = "zeros"; Hm, Wm <= 16384. */
int acfm_uv_texels(const int64_t* pix_to_face, const float* bary, const float* faces_verts_uvs, const float* maps,
                   size_t P, int K, int pix_per_mesh, int F_packed, int N, int Hm, int Wm, int align_corners,
                   int padding_mode, float* texels, const AcfmRasterTuning* tuning, void* stream);
/* Backward of the above (App-A.11), recomputed from the same inputs; each output may be NULL: grad_maps [N,Hm,Wm,3]
 * and grad_faces_verts_uvs [F_packed,3,2] (scattered: float atomics, or in deterministic mode integer pairs in `ws`,
 * 16 bytes per element of the requested ones, grad_maps first), grad_bary [P,K,3] (0 in empty slots). */
int acfm_uv_texels_backward(const int64_t* pix_to_face, const float* bary, const float* faces_verts_uvs,
                            const float* maps, const float* grad_texels, size_t P, int K, int pix_per_mesh,
                            int F_packed, int N, int Hm, int Wm, int align_corners, int padding_mode, float* grad_maps,
                            float* grad_bary, float* grad_faces_verts_uvs, void* ws, size_t ws_bytes,
                            const AcfmRasterTuning* tuning, void* stream);

/* ---- lit shading -------------------------------------------------------------
 * acfm_vertex_normals: Meshes.verts_normals_packed / faces_normals_packed of PyTorch3D 0.3.0.  verts [V,3] f32 and
 *   faces [F,3] i64, packed; (offsets [V+1], corners [3F]) i32: for every vertex the corners 3 f + i that hold it,
 *   ascending (CSR; built once per faces tensor on the host).  verts_normals [V,3] = x / max(|x|, 1e-6) of the sum, in
 *   table order, of the unnormalised cross products (v[i+1] - v[i]) x (v[i+2] - v[i]) taken at the vertex's own corner;
 *   faces_normals [F,3] = normalize((v2 - v1) x (v0 - v1)).  Either output may be NULL.  A face with a vertex id outside
 *   [0, V) contributes nothing.  A gather per vertex: no atomics, no valence cap, the same bits on every run.
 * acfm_vertex_normals_backward: grad_verts [V,3] from grad_verts_normals and / or grad_faces_normals (either may be
 *   NULL), again a gather per vertex in two launches; ws: 12 V bytes when grad_verts_normals is given. */
int acfm_vertex_normals(const float* verts, const int64_t* faces, const int* offsets, const int* corners, int V, int F,
                        float* verts_normals, float* faces_normals, void* stream);
int acfm_vertex_normals_backward(const float* verts, const int64_t* faces, const int* offsets, const int* corners,
                                 const float* grad_verts_normals, const float* grad_faces_normals, int V, int F,
                                 float* grad_verts, void* ws, size_t ws_bytes, void* stream);
/* acfm_light_points: the lighting function of pytorch3d.renderer.lighting (DirectionalLights / PointLights .diffuse and
 *   .specular) at M points: out = (ambient + diffuse relu(n.l)) colour + specular relu(v.r)^shininess [n.l > 0], with
 *   n, l = (point_light ? L - p : L), v = camera - p normalised as x / max(|x|, 1e-6) and r = 2 (n.l) n - l.  points,
 *   normals, colours, out [M,3]; mesh_idx [M] i64 (NULL: mesh 0; outside [0, N): zeros); consts [N,16] per mesh = the
 *   ambient, diffuse and specular products light colour x material colour, the light vector L (direction or location),
 *   the camera centre (3 floats each) and the shininess.  Lights, materials and camera are constants: no gradient.
 * acfm_light_points_backward: dense, one thread per point; each of grad_points / grad_normals / grad_colours may be
 *   NULL.  Where relu(v.r) or the n.l > 0 mask is closed the specular term sends 0 (never inf x 0). */
int acfm_light_points(const float* points, const float* normals, const float* colours, const int64_t* mesh_idx,
                      const float* consts, int point_light, int M, int N, float* out, void* stream);
int acfm_light_points_backward(const float* points, const float* normals, const float* colours,
                               const int64_t* mesh_idx, const float* consts, int point_light,
                               const float* grad_out, int M, int N, float* grad_points, float* grad_normals,
                               float* grad_colours, void* stream);
/* acfm_phong_shade: pytorch3d.renderer.mesh.shading.phong_shading (flat = 0) / flat_shading (flat = 1) over Fragments,
 *   one thread per slot: colors [P,K,3] = the lighting function above at the slot's position and normal, with texels
 *   [P,K,3] as the colour and the constants of mesh p / pix_per_mesh (P = N pix_per_mesh).  flat = 0: position and
 *   normal are sum_i bary_i verts[faces[f,i]] and sum_i bary_i normals[faces[f,i]] (normals [V_packed,3]), formed in the
 *   kernel: neither verts[faces], normals[faces] nor the two interpolated tensors exist.  flat = 1: the face's mean
 *   position and normals[f] (normals [F_packed,3]; bary may be NULL).  A slot with pix_to_face outside [0, F_packed)
 *   (or a face with a vertex id outside [0, V_packed)) is shaded at position and normal 0, as the composition does.
 * acfm_phong_shade_backward: grad_texels [P,K,3] and grad_bary [P,K,3] (0 when flat) dense, grad_corners
 *   [F_packed,3,6] = (position, normal) gradient per face corner (flat: a third of the position gradient per corner,
 *   the normal gradient in corner 0); each may be NULL.  The corner sums are scattered: runs of equal faces along 64
 *   consecutive pixels of one slot index are summed inside the wave first, then added with float atomics, or in
 *   deterministic mode as integer pairs in `ws` (16 bytes per element of grad_corners), bit-reproducible.
 * acfm_corner_gather: grad_corners -> grad_verts [V,3] (position part, summed over a vertex's corners through the
 *   incidence table of acfm_vertex_normals) and grad_normals ([V,3] summed likewise, or flat: [F,3] corner 0's). */
int acfm_phong_shade(const int64_t* pix_to_face, const float* bary, const float* texels, const float* verts,
                     const int64_t* faces, const float* normals, const float* consts, int point_light, int flat,
                     size_t P, int K, int pix_per_mesh, int F_packed, int V_packed, int N, float* colors,
                     const AcfmRasterTuning* tuning, void* stream);
int acfm_phong_shade_backward(const int64_t* pix_to_face, const float* bary, const float* texels, const float* verts,
                              const int64_t* faces, const float* normals, const float* consts, int point_light,
                              int flat, const float* grad_colors, size_t P, int K, int pix_per_mesh, int F_packed,
                              int V_packed, int N, float* grad_texels, float* grad_bary, float* grad_corners, void* ws,
                              size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream);
int acfm_corner_gather(const float* grad_corners, const int* offsets, const int* corners, int V, int F, int flat,
                       float* grad_verts, float* grad_normals, void* stream);

/* ---- atlas-textured render -----------------------------------------------------------
 * replaces NeuralRenderer.forward, texture branch with atlas=True
 * (multiframe/nnutils/nmr.py:173-200): hard raster K=1, clip_barycentric_coords=True,
 * TexturesAtlas.sample_textures, ambient-only SoftPhongShader, softmax_rgb_blend.
 *   atlas [N,F,R,R,3] f32 -> imgs [N,3,H,H], sil [N,H,H], pix_to_face [N,H,H,1] i64,
 *   texel_idx [N,H,H] i32 (linear texel index n*F*R*R + f*R*R + y*R + x, -1 empty;
 *   saved for the backward pass).
 * ws_ready != 0: `ws` already holds the face setup of THE SAME verts / faces / cams / H /
 * offset_z, left there by acfm_sil_forward with blur_radius = ws_blur (the reference renders the
 * silhouette and the texture of one prediction back to back, main.py:616-636): projection and
 * face setup are skipped and the blur-expanded boxes tightened by sqrt(ws_blur).
 * ws_ready == 2: that acfm_sil_forward ran with ACFM_RECORD_COVER (and the same tuning is passed here): the nearest
 * covering face of every pixel is read from the workspace, nothing is binned or walked.
 * ws_ready == 3: as 2, and that render was given THESE imgs / sil / pix_to_face / texel_idx buffers in
 * AcfmSilExtras.tex_*: the blocks no face comes near hold their constants already and are not written again.
 * atlas_batch: number of distinct atlases, atlas [atlas_batch,F,R,R,3]; mesh n samples atlas
 * n % atlas_batch (the trainer renders G camera hypotheses of every frame with the frame's one
 * texture, textures.repeat(G, ...) at main.py:627-636: atlas_batch = N / G spares the copies, and
 * the backward accumulates the G renders straight into the one gradient). */
int acfm_tex_forward(const float* verts_world, const int64_t* faces, const float* cams,
                     const void* atlas /* [real] */, int N, int V, int F, int H, int R, float sigma,
                     float gamma, float offset_z, void* imgs /* [real] */, void* sil /* [real] */, void* pix_to_face,
                     int32_t* texel_idx, void* ws, size_t ws_bytes, int ws_ready, float ws_blur,
                     int atlas_batch, const AcfmRasterTuning* tuning, void* stream);
/* NeuralRenderer.forward with atlas=False (multiframe/nnutils/nmr.py:177-179, used by
 * utils/bird_vis.py for visualisation): Textures(verts_rgb) = barycentric interpolation of
 * per-vertex colours verts_rgb [N,V,3]; forward only.  Workspace: raster workspace + 4*N*H*H. */
int acfm_vertex_color_forward(const float* verts_world, const int64_t* faces, const float* cams,
                              const float* verts_rgb, int N, int V, int F, int H, float sigma,
                              float gamma, float offset_z, float* imgs, float* sil,
                              int64_t* pix_to_face, void* ws, size_t ws_bytes, int ws_ready, float ws_blur,
                              const AcfmRasterTuning* tuning, void* stream);
/* grad_imgs [N,3,H,H] -> grad_atlas [N,F,R,R,3] (zeroed here, then scatter-added).
 * Integer texel indexing sends no gradient to geometry. */
int acfm_tex_backward(const float* grad_imgs, const int32_t* texel_idx, int N, int F, int H, int R, int atlas_batch,
                      float* grad_atlas, void* stream);
/* Same gradient in gather form (R <= 8): one wave per (atlas, face) sums the pixels of the face's box
 * whose texel belongs to it and stores all its texels -- no global atomics, no zero fill.  ws = the
 * workspace acfm_tex_forward ran on (its face boxes), ws_blur = the blur it was set up with (0 unless
 * taken over from a silhouette render, ws_ready).  Replaces the TexturesAtlas index_put backward. */
int acfm_tex_backward_faces(const float* grad_imgs, const int32_t* texel_idx, const void* ws, size_t ws_bytes,
                            float ws_blur, int N, int V, int F, int H, int R, int atlas_batch, float* grad_atlas,
                            void* stream);

/* ---- fused atlas-textured render + masked texture MSE (opt-in) ---------------------------
 * acfm_tex_forward and acfm_tex_mse as ONE operator (multiframe/main.py:627-636 renders texture_pred and :655-662
 * takes F.mse_loss(texture_pred * mask, imgs * mask).mean((1,2,3)) of it at once): the squared differences are summed
 * in the raster kernel's epilogue (per-block partials, fixed-order sums: deterministic), and the atlas gradient is
 * gathered per face straight from (imgs, ref_img, ref_mask, grad_loss) -- no [N,3,H,H] gradient image, no separate
 * passes (acfm_tex_mse, acfm_tex_mse_backward).  Outputs of acfm_tex_forward plus loss [N];
 * ref_img [ref_batch,3,H,H], ref_mask [ref_batch,H,H], prediction n <-> reference n % ref_batch.  R <= 8. */
int acfm_tex_mse_forward(const float* verts_world, const int64_t* faces, const float* cams, const void* atlas,
                         const void* ref_img, const void* ref_mask, int ref_batch, int N, int V, int F, int H, int R,
                         float sigma, float gamma, float offset_z, void* imgs, void* sil, void* pix_to_face,
                         int32_t* texel_idx, float* loss, void* ws, size_t ws_bytes, int ws_ready, float ws_blur,
                         int atlas_batch, const AcfmRasterTuning* tuning, void* stream);
int acfm_tex_mse_backward_faces(const void* imgs, const void* ref_img, const void* ref_mask, int ref_batch,
                                const float* grad_loss, const int32_t* texel_idx, const void* ws, size_t ws_bytes,
                                float ws_blur, int N, int V, int F, int H, int R, int atlas_batch, float* grad_atlas,
                                const AcfmRasterTuning* tuning, void* stream);

/* ---- loss combination ------------------------------------------------------------------
 * replaces the elementwise tail of the trainer's total loss (multiframe/main.py:716-746, 749-765:
 * weight * term + ... then .mean() over the batch): total = (1/N) sum_n sum_t sum_c w[t][c] T_t[n,c]
 * for up to 4 terms T_t [N, cols[t]] (cols <= 4, dense row-major), one launch each way.
 * terms / grads / cols / weights are HOST arrays (device pointers inside terms and grads; weights
 * flattened term by term); a NULL grads[t] skips that term. */
int acfm_combine_losses(const void* const* terms, const int* cols, const float* weights, int nterms, int N,
                        float* total, void* stream);
int acfm_combine_losses_backward(const float* grad_total, void* const* grads, const int* cols,
                                 const float* weights, int nterms, int N, void* stream);

/* ---- total per hypothesis + hypothesis weighting --------------------------------------------------
 * replaces the per-hypothesis total of ShapeTrainer.forward and its softmax weighting (multiframe/main.py:716-746:
 * weight * term + ..., probs = softmax(-total, dim 0).detach(), (total * probs).sum(0).mean()) by one launch each way:
 *   total[g,n] = sum_t w_t T_t[g,n]  for nterms <= 8 terms T_t [G*N] f32 (row g*N + n);
 *   probs[g,n] = softmax over g of -total[.,n];   out[0] = (1/N) sum_n sum_g probs total (the weighted loss),
 *   out[1] = mean total (what the reference logs as camera_loss), out[2..3] = means of the two auxiliary sums
 *   aux_k[g,n] = sum_{t: aux_group[t] == k} aux_weights[t] T_t[g,n] (logged terms such as sil_cons; aux0 / aux1 and
 *   aux_group / aux_weights may be NULL), out[4 + t] = mean of term t.  out: 12 floats.
 * backward: grads[t][g,n] = grad_weighted * w_t * probs[g,n] / N (NULL grads[t] skipped); probs carry no gradient.
 * terms / grads / weights / aux_* are HOST arrays (device pointers inside terms and grads). */
int acfm_hypothesis_total(const void* const* terms, const float* weights, const int* aux_group, const float* aux_weights,
                          int nterms, int G, int N, float* total, float* probs, float* aux0, float* aux1, float* out,
                          void* stream);
int acfm_hypothesis_total_backward(const float* grad_weighted, const float* probs, const float* weights, int nterms,
                                   int G, int N, void* const* grads, void* stream);

/* ---- texture temporal-consistency term ------------------------------------------------------------
 * replaces multiframe/main.py:705-711 as written there: the per-frame atlases textures [B*T,F,R,R,3] regrouped as
 * [B,F,R,R,T,3], that buffer reshaped to rows [-1,R,R], loss = mean over (row block m, i < R-1) of the L2 norm over
 * j of X[m,i,j] - X[m,i+1,j] (zero norms contribute no gradient, as torch.norm's backward).
 * scratch: acfm_texture_cycle_scratch_floats(B,T,F,R) floats (the norms, kept for the backward, + partial sums);
 * any B, T, F; R >= 2.  Sums in a fixed order: reproducible. */
size_t acfm_texture_cycle_scratch_floats(int B, int T, int F, int R);
int acfm_texture_cycle(const float* textures, int B, int T, int F, int R, float* scratch, float* loss, void* stream);
int acfm_texture_cycle_backward(const float* textures, const float* scratch, const float* grad_loss, int B, int T, int F,
                                int R, float* grad_textures, void* stream);

/* ---- fused silhouette losses ---------------------------------------------------------
 * replaces loss_utils.l1_loss / iou / iou_loss / edt_loss with reduce=False
 * (multiframe/nnutils/loss_utils.py:18-32, 72-77, 245-253) in one pass over the mask:
 *   out [N,4] = (mean|m-gt|, sum m*gt, sum (m+gt-m*gt), mean edt*m); gt / edt may be NULL.
 * With HW % 4 == 0 edt is read only where the four mask values of an aligned group of four pixels are not all zero
 * (edt*m is +0 elsewhere for finite edt: the same bits); a NaN or infinity in edt under such a group does not reach out[3].
 * ref_batch (here and in the losses below): the number of distinct references; prediction n is
 * compared with reference n % ref_batch (gt, edt [ref_batch,HW]).  The trainer scores G camera
 * hypotheses per frame against the frame's one ground truth (masks.repeat(G, 1, 1) at
 * main.py:472-479, 644-662): ref_batch = N / G spares those copies; ref_batch = N is the plain case.
 *
 * The finish of the three per-mesh loss sums (acfm_mask_losses, acfm_tex_mse, acfm_bds_loss), chosen by their
 * `tickets` / `partials` arguments; inputs and outputs are the same either way.
 *   tickets == partials == NULL: the call zeroes the output with a launch of its own and the workgroups add their sums
 *     to it with float atomics, in the order they arrive.  Only one of the two NULL: ACFM_E_BADARG.
 *   Both given: ONE launch.  Every workgroup hands its sums over in `partials`, counts itself in `tickets`, and the
 *     workgroup that finishes a mesh last adds the sums in workgroup order: no fill, and the same inputs give the same
 *     bits on every run.
 *   tickets: N words, ALL ZERO before their first use; every launch leaves them at zero again, so any of the
 *     three entry points, with any shape of at most that many meshes, can follow on them.  (A launch that is
 *     killed midway leaves them undefined: zero them again.)
 *   partials: partial_floats >= acfm_loss_partial_floats(which, N, n) floats, n = HW for the two image losses and
 *     the number of points per mesh for the boundary loss; any contents.  Too small: ACFM_E_WORKSPACE.
 *   Calls that can be in flight at the same time (different streams) need tickets and partials each. */
enum { ACFM_LOSS_MASK = 0, ACFM_LOSS_TEX_MSE = 1, ACFM_LOSS_BDS = 2 };
size_t acfm_loss_partial_floats(int which, int N, int n);
int acfm_mask_losses(const float* mask, const float* gt, const float* edt, int N, int HW, int ref_batch,
                     float* out, uint32_t* tickets, float* partials, size_t partial_floats, void* stream);
/* grad_mask [N,HW] = w_l1[n]*sign(m-gt)/HW + w_edt[n]*edt/HW + IoU term
 * (w_inter[n]*gt + w_union[n]*(1-gt)); weights are per-mesh upstream gradients [N,4]. */
int acfm_mask_losses_backward(const float* mask, const float* gt, const float* edt,
                              const float* grad_out, int N, int HW, int ref_batch, float* grad_mask,
                              void* stream);

/* ---- masked texture MSE ---------------------------------------------------------------
 * replaces the inline texture term of multiframe/main.py:655-662,
 * F.mse_loss(texture_pred * mask, imgs * mask, reduction='none').mean((1,2,3)):
 *   tex [N,3,HW], img [ref_batch,3,HW], mask [ref_batch,HW] f32 -> out [N]; backward -> grad_tex [N,3,HW].
 * The forward reads the mask first and tex / img only where it is not zero: with HW % 4 == 0 where the four mask
 * values of an aligned group of four pixels are not all zero, else per pixel.  For finite tex and img the result is
 * bit for bit the sum over every pixel ((t m - g m)^2 is +0 under m == 0).  A NaN or infinity in tex or img where
 * the mask is zero does NOT reach the result unless a non-zero mask value shares its group of four, whereas
 * F.mse_loss(tex * mask, img * mask) returns NaN for it.  acfm_tex_mse_backward reads every pixel. */
int acfm_tex_mse(const float* tex, const float* img, const float* mask, int N, int HW, int ref_batch,
                 float* out, uint32_t* tickets, float* partials, size_t partial_floats,
                 void* stream);                                    /* tickets / partials: see acfm_mask_losses */
int acfm_tex_mse_backward(const float* tex, const float* img, const float* mask,
                          const float* grad_out, int N, int HW, int ref_batch, float* grad_tex, void* stream);

/* ---- visibility + boundary loss ------------------------------------------------------
 * visible-vertex bitmap shared by loss_utils.bds_loss (:214-224) and optical_flow_loss
 * (:432-443): vis [N,V] u8 = 1 for every vertex of a face that appears in
 * pix_to_face[..., 0].  pix_to_face has `K` ids per pixel (only slot 0 is read). */
int acfm_visible_vertices(const int64_t* pix_to_face, const int64_t* faces, int N, int V, int F,
                          int HW, int K, uint8_t* vis, void* stream);
/* loss_utils.bds_loss (:204-237) given vis: for each boundary point the squared distance to
 * the nearest visible projected vertex (1000 where none), times the point's valid flag,
 * summed per mesh.  verts_xy [N,V,2], bds [ref_batch,P,3] -> loss [N], argmin i32 (saved).
 *   sel == NULL: every point of the reference; argmin [N,P], rows and S are ignored, scratch is sized with n = P
 *   (acfm_loss_partial_floats(ACFM_LOSS_BDS, N, P); tickets / partials: see acfm_mask_losses).
 *   sel != NULL: a SUBSET of each reference's points, named by slot lists (acfm_boundary_subset below) instead of a
 *   gathered copy -- replaces `indices = torch.randperm(P)[:n_samples]; bds = bds[..., indices, :]` of
 *   loss_utils.bds_loss (:211-213) together with the distance search that follows it (:226-237).
 *   sel [rows,S] i32, rows = 1 (one list for every reference) or rows = ref_batch (reference b reads row b): entry p
 *   names slot sel[((n % ref_batch) % rows) S + p] of bds [ref_batch,P,3]; an entry < 0 (or >= P) is empty: it adds 0
 *   and its argmin is -1.  argmin [N,S]; scratch is sized with n = S.
 * The backward takes the sel (and rows, S) of its forward: grad_loss [N] -> grad_verts_xy [N,V,2].
 * The forward keeps 12 B per vertex in dynamic LDS, the backward 8 B, at most 150 KB: V <= 12,800 forward (so the
 * backward's V <= 19,200 is never the limit); a larger V returns ACFM_E_BADARG. */
int acfm_bds_loss(const float* verts_xy, const float* bds, const uint8_t* vis, const int32_t* sel, int N, int V, int P,
                  int ref_batch, int rows, int S, float* loss, int32_t* argmin, uint32_t* tickets, float* partials,
                  size_t partial_floats, void* stream);
int acfm_bds_loss_backward(const float* verts_xy, const float* bds, const int32_t* sel, const int32_t* argmin,
                           const float* grad_loss, int N, int V, int P, int ref_batch, int rows, int S,
                           float* grad_verts_xy, void* stream);
/* acfm_boundary_subset: the draw itself, `torch.randperm(P)[:n_samples]` of loss_utils.bds_loss (:211), on the device:
 * a uniform random subset of min(n_samples, P_r) of the slots [0, P_r) of every row r, without replacement, written
 * in ascending slot order and followed by -1.  sel [rows,n_samples] i32.
 *   state  int64[2] on the device = (seed, draw).  The call uses draw = state[1] and leaves state[1] one higher (a
 *          launch of its own behind the draw, in stream order: no host synchronisation, and a captured call draws
 *          a fresh subset at every replay, as the reference redraws at every call).
 *   counts i32 [n_counts] true list lengths (acfm_boundaries), or NULL with n_counts = 0.
 *   rows = 1        one subset for the whole batch, as in the reference: P_0 = min(P, max(counts)), or P without counts;
 *   rows = n_counts one subset per reference over ITS OWN points: P_r = min(P, counts[r]) -- every frame gets n_samples
 *                   real points instead of spending draws on the padding.
 *   A row with P_r = 0 is all -1.
 * Definition: slot i of row r in draw t has the 64-bit key x0 << 32 | x1 of Philox4x32-10 (Salmon et al., SC'11) with
 * key (seed's low word, seed's high word) and counter (i, r, t's low word, t's high word); the subset is the slots
 * with the min(n_samples, P_r) smallest (key, i).  boundary_sampling.subset_host restates this in numpy and is the
 * specification: the kernel equals it index for index.  The draws follow the reference's DISTRIBUTION, not its
 * random stream (as pytorch3d_shim's sample_points_from_meshes).  P <= 2^30; one workgroup per row, no storage
 * sized by P. */
int acfm_boundary_subset(int64_t* state, const int32_t* counts, int n_counts, int rows, int P, int n_samples,
                         int32_t* sel, void* stream);
/* acfm_surface_sample: pytorch3d.ops.sample_points_from_meshes (utils/geometry.py:110-111) on the device: per mesh, S
 * faces drawn with replacement in proportion to their area, and a uniform point of each.  Packed meshes: verts_packed
 * [P,3] f32, faces_packed [F,3] i64 (packed vertex ids), faces_first_idx [N+1] i64 ON THE DEVICE (mesh m = faces
 * [first[m], first[m+1])).  -> points [N,S,3] f32, face_idx [N,S] i32 (row of faces_packed, or -1), uv [N,S,2] f32.
 *   state  int64[2] = (seed, draw) on the device, used and advanced exactly as by acfm_boundary_subset.
 * Definition (surface_sampling.surface_sample_host restates it in numpy and is the specification; the kernels equal
 * it bit for bit, the library being compiled without contraction and with correctly rounded division and sqrt):
 *   n_f = sqrt((cx cx + cy cy) + cz cz), (cx, cy, cz) = (b - a) x (c - a), in f32 with every operation rounded; 0 when
 *         not finite or when the face names a vertex outside [0, P);
 *   q_f = floor((n_f / n_max) 2^24) with n_max the mesh's largest n_f; cdf = the inclusive prefix sum of q in 64-bit
 *         integers.  A face below 2^-24 of its mesh's largest face is therefore never drawn, and the probabilities of
 *         the others are those of their areas to within 2^-24 of the largest.
 *   sample s of mesh m in draw t: (x0, x1, x2, x3) = Philox4x32-10, key (seed lo, seed hi), counter (s, m, t lo, t hi);
 *         target = ((x0 << 32 | x1) total) >> 64 with total = cdf[last]; the face is the first f with cdf_f > target
 *         (faces of weight 0 are skipped wherever they lie); u = (x2 >> 8) 2^-24, v = (x3 >> 8) 2^-24;
 *         su = sqrt(u), (w0, w1, w2) = (1 - su, su (1 - v), su v), point = (w0 a + w1 b) + w2 c.
 *   A mesh without faces, or whose faces all have weight 0: points 0, face_idx -1, uv 0.
 * Three launches on the one stream: the CDF (one workgroup per mesh), the samples (one thread each), the counter.  No
 * host read, no allocation: capturable, and a captured call draws afresh at every replay.
 *   workspace: acfm_surface_sample_workspace_bytes(N, F) bytes, 256-byte aligned, any contents (8 B per face); fewer is
 *   ACFM_E_WORKSPACE.  The query returns 0 for sizes the call refuses.
 *   faces_first_idx_host: NULL, or the caller's HOST copy of the table, which is then checked: ACFM_E_BADARG unless
 *   0 <= first[0] <= ... <= first[N] <= F.  The kernels clamp the device table the same way, so a table that does not
 *   describe the arrays never leads outside them.
 *   ACFM_E_BADARG also for N < 1, N > 65535, S < 1, P < 1, F < 0, or 3 P, 3 F or 3 N S past 2^31 - 1.  F = 0 is allowed
 *   (faces_packed may then be NULL).
 * acfm_surface_sample_backward: grad_points [N,S,3] -> grad_verts [P,3] = sum over the samples of w_k grad_point at the
 *   three vertices of its face; EVERY row is written.  verts_per_mesh > 0: the packed arrays are N equal-sized meshes
 *   one after the other (mesh m = vertices [m vpm, (m+1) vpm), and its faces name only those): one workgroup per mesh
 *   adds in LDS, 12 B per vertex, at most 150 KB: verts_per_mesh <= 12,800.  0, larger meshes and a verts_per_mesh with
 *   N verts_per_mesh != P: a zero fill and global float atomics, same result.  Either way the order of the float
 *   additions varies from run to run: the gradient is NOT bit-reproducible. */
size_t acfm_surface_sample_workspace_bytes(int N, int F);
int acfm_surface_sample(int64_t* state, const float* verts_packed, const int64_t* faces_packed,
                        const int64_t* faces_first_idx, const int64_t* faces_first_idx_host, int N, int S, int P, int F,
                        float* points, int32_t* face_idx, float* uv, void* workspace, size_t workspace_bytes,
                        void* stream);
int acfm_surface_sample_backward(const float* grad_points, const int32_t* face_idx, const float* uv,
                                 const int64_t* faces_packed, int N, int S, int P, int F, int verts_per_mesh,
                                 float* grad_verts, void* stream);

/* ---- the step's tail in one launch ------------------------------------------------------------------------------
 * acfm_step_losses_forward: any of acfm_mask_losses, acfm_tex_mse and acfm_bds_loss (each in its ticket form) on
 * the same N meshes, and optionally acfm_combine_losses over their outputs, as ONE kernel (k_step_tail): the three
 * sums are short launches far below the memory and issue limits, and as roles of one grid their latencies overlap.
 * Every job computes what its own entry point computes, bit for bit (same pixel partition, same order of sums); the
 * fields of a job are that entry point's arguments.  mask / tex / bds: NULL = that term is not computed (at least
 * one must be given).  bds->sel: as acfm_bds_loss's sel (NULL: rows and S are ignored).
 * total: NULL, or the arguments of acfm_combine_losses; its terms are usually the outputs of the jobs of this call
 * (the kernel evaluates the total once the last of them is finished), and any other term must have been finished by
 * an earlier launch on the stream.  Same expression in the same order as acfm_combine_losses: the same bits.
 * Scratch: tickets, acfm_step_losses_ws's *ticket_words words (3 N + 1), ALL ZERO before their first use and left at
 * zero by every launch; partials, the returned number of floats, any contents (HW_mask / HW_tex / S = 0 for an absent
 * job; S = P without a slot list).  Too small: ACFM_E_WORKSPACE.  Stream-ordered, no host synchronisation: capturable. */
typedef struct {
  const float* mask; const float* gt; const float* edt;   /* gt / edt may be NULL */
  float* out;                                              /* [N,4] */
  int HW, ref_batch;
} acfm_step_mask_job;
typedef struct {
  const float* tex; const float* img; const float* mask;
  float* out;                                              /* [N] */
  int HW, ref_batch;
} acfm_step_tex_job;
typedef struct {
  const float* verts_xy; const float* bds; const uint8_t* vis;
  const int32_t* sel;                                      /* NULL, or [rows,S] */
  float* loss; int32_t* argmin;                            /* [N], [N,P] (with sel: [N,S]) */
  int V, P, ref_batch, rows, S;
} acfm_step_bds_job;
typedef struct {
  const void* const* terms; const int* cols; const float* weights;
  int nterms;
  float* total;
} acfm_step_total_job;
size_t acfm_step_losses_ws(int N, int HW_mask, int HW_tex, int S, size_t* ticket_words);
int acfm_step_losses_forward(const acfm_step_mask_job* mask, const acfm_step_tex_job* tex, const acfm_step_bds_job* bds,
                             const acfm_step_total_job* total, int N, uint32_t* tickets, float* partials,
                             size_t partial_floats, void* stream);

/* ---- mesh priors -------------------------------------------------------------------------
 * Packed meshes: verts [P,3] f32, faces [F,3] / edges [E,2] i64 with packed vertex ids.
 * acfm_cot_laplacian: geom_utils.mesh_laplacian(mesh, 'cot') (multiframe/nnutils/geom_utils.py:
 *   158-324) for ONE mesh: dense L [V,V] = W - diag(rowsum W), W_ij = (cot a_ij + cot b_ij)/4. */
int acfm_cot_laplacian(const float* verts, const int64_t* faces, int V, int F, float* L, void* stream);
/* acfm_laplacian_smoothing: pytorch3d.loss.mesh_laplacian_smoothing (multiframe/main.py:699-704):
 *   method 0 'cot' (conn = faces [F,3]): loss = sum_v vweight[v] * |(W v)_v / rowsum_v - v_v|;
 *   method 1 'uniform' (conn = unique edges [F,2]): W_ij = 1 on edges.
 *   vweight [P] = 1 / (verts of the vertex's mesh); the caller divides the sum by the mesh count.
 *   verts_per_mesh / faces_per_mesh > 0 (method 0): the packed arrays are equal-sized meshes one after the
 *   other (mesh m = vertices [m vpm, (m+1) vpm), faces [m fpm, (m+1) fpm)): one workgroup per mesh accumulates
 *   in LDS, one launch each way; 0 = unknown layout (global atomics).  16 B of dynamic LDS per vertex, at most
 *   150 KB: verts_per_mesh <= 9,600.  Larger meshes, and hints that do not describe the arrays (verts_per_mesh not
 *   dividing P, P / verts_per_mesh != F / faces_per_mesh), take the global-atomic kernels: same result, no error.
 *   loss: 1 float (device); state: acfm_laplacian_smoothing_state_floats(P, F) floats kept for
 *   the backward, which takes the upstream gradient as a DEVICE scalar. */
size_t acfm_laplacian_smoothing_state_floats(int P, int F);
int acfm_laplacian_smoothing(const float* verts, const int64_t* conn, const float* vweight, int P, int F,
                             int method, int verts_per_mesh, int faces_per_mesh, float* loss, float* state,
                             void* stream);
int acfm_laplacian_smoothing_backward(const int64_t* conn, const float* state, const float* grad_loss, int P,
                                      int F, int method, int verts_per_mesh, int faces_per_mesh,
                                      float* grad_verts, void* stream);
/* acfm_edge_rigidity: loss_utils.locally_rigid_fn (multiframe/nnutils/loss_utils.py:150-164):
 *   loss = sum_e (|v[e0]-v[e1]| - |vt[et0]-vt[et1]|)^2 (the caller divides by the mesh count). */
int acfm_edge_rigidity(const float* verts, const int64_t* edges, const float* verts_t, const int64_t* edges_t,
                       int E, float* loss, void* stream);
int acfm_edge_rigidity_backward(const float* verts, const int64_t* edges, const float* verts_t,
                                const int64_t* edges_t, int E, int P, int Pt, int verts_per_mesh,
                                const float* grad_loss, float* grad_verts, float* grad_verts_t, void* stream);
/* verts_per_mesh > 0: equal-sized meshes and `edges` sorted by its first vertex (Meshes.edges_packed()):
 * one workgroup per mesh accumulates in LDS (used when only grad_verts is asked for); 0: unknown layout.
 * 12 B of dynamic LDS per vertex, at most 150 KB: verts_per_mesh <= 12,800; larger meshes, and a verts_per_mesh that
 * does not divide P, take the global-atomic kernel: same result, no error. */

/* ---- template fit (utils/geometry.py:75-140, fit_verts_to_mesh) ------------------------------
 * acfm_chamfer: the sums of pytorch3d.loss.chamfer_distance.  x [N,P1,3], y [N,P2,3] f32; x_len, y_len [N] i64 on the
 *   device or NULL (= P1 / P2; values are clamped to [0, P]).  Rows at or past a length are never read.
 *     sums[n,0] = sum_{i < x_len[n]} min_{j < y_len[n]} |x_i - y_j|^2,   sums[n,1] = the same with x and y exchanged,
 *     idx_x [N,P1], idx_y [N,P2] i32: the index of that nearest point, the lowest one among equal distances, -1 if the
 *     other cloud has length 0 (then the sum is 0); rows at or past the length are not written.
 *   |.|^2 = (dx dx + dy dy) + dz dz in f32, each operation rounded.  Both directions are one launch; the candidates
 *   stream through a fixed 16 KB of LDS, so P1 and P2 are bounded by int only; N <= 65535.
 *   Scratch as for the ticket form of acfm_mask_losses, but 2 N ticket words (all zero before the first use, zero again
 *   after every launch) and acfm_chamfer_partial_floats(N, P1, P2) floats of any contents, both required: no zero fill of
 *   `sums`, no float atomics, the same bits on every run.
 * acfm_chamfer_backward: grad_sums [N,2] (device) -> grad_x [N,P1,3], grad_y [N,P2,3]; EVERY row is written (zeros
 *   at and past the lengths).  A point receives 2 g (p - nn(p)) for its own nearest neighbour and 2 g' (p - r) from
 *   every point r of the other cloud that chose it.  One workgroup per (pair, side) sums in LDS, 12 B per point, at
 *   most 150 KB: max(P1, P2) <= 12,800; larger clouds take two launches with global atomics, same result.  Either way
 *   the order of the float additions varies from run to run: the gradients are NOT bit-reproducible. */
size_t acfm_chamfer_partial_floats(int N, int P1, int P2);
int acfm_chamfer(const float* x, const float* y, const int64_t* x_len, const int64_t* y_len, int N, int P1, int P2,
                 float* sums, int32_t* idx_x, int32_t* idx_y, uint32_t* tickets, float* partials,
                 size_t partial_floats, void* stream);
int acfm_chamfer_backward(const float* x, const float* y, const int64_t* x_len, const int64_t* y_len,
                          const int32_t* idx_x, const int32_t* idx_y, const float* grad_sums, int N, int P1, int P2,
                          float* grad_x, float* grad_y, void* stream);
/* ---- point sets (PyTorch3D 0.3.0's pytorch3d.ops.knn) ------------------------------------------
 * acfm_knn_points: pytorch3d.ops.knn_points.  p1 [N,P1,3], p2 [N,P2,3] f32; lengths1, lengths2 [N] i64 on the device
 *   or NULL (= P1 / P2; values are clamped to [0, P]); 1 <= K <= 32; N <= 65535.  Rows at or past a length are never
 *   read.  dists [N,P1,K] f32, idx [N,P1,K] i64: slot (n, i, k) with i < lengths1[n] and k < min(K, lengths2[n]) holds
 *   the k-th smallest |p1_i - p2_j|^2 = (dx dx + dy dy) + dz dz (f32, each operation rounded, as acfm_chamfer) and
 *   its j; ascending, the lower index first among equal distances.  EVERY other slot is written with 0 / 0 (PyTorch3D's
 *   padding), and so is a slot that no finite distance reached.  No workspace, no atomics: the same bits on every run.
 * acfm_knn_points_backward: grad_dists [N,P1,K] -> grad_p1 [N,P1,3] = sum_k 2 g (p1_i - p2[idx]) over the valid
 *   slots, and grad_p2 [N,P2,3], which receives the negated terms; EVERY row of both is written (zeros at and past the
 *   lengths); grad_dists is read at valid slots only, a slot whose index is outside [0, lengths2[n]) sends nothing.
 *   P2 <= 12,800 and P1 K <= 16,384: one workgroup per cloud sums grad_p2 in LDS (12 B per point, at most 150 KB);
 *   larger clouds or more slots: global float atomics behind a zero fill, same result.  Either way grad_p2 is NOT
 *   bit-reproducible (grad_p1 is).
 * acfm_knn_gather: pytorch3d.ops.knn_gather.  x [N,M,U] f32 (U >= 1), idx [N,L,K] i64 (idx_is_int64 != 0) or i32,
 *   lengths [N] i64 of x's clouds or NULL (= M; clamped to [0, M]) -> out [N,L,K,U], out[n,l,k] = x[n, idx[n,l,k]].
 *   Where k >= lengths[n] or the index is outside [0, M) zeros are written and x is not read.
 * acfm_knn_gather_backward: grad_out [N,L,K,U] -> grad_x [N,M,U], zeroed first, then added into with float atomics
 *   under the same two tests (NOT bit-reproducible where an index occurs more than once).
 * All four: ACFM_E_BADARG for K outside its range, non-positive sizes or sizes whose element counts overflow. */
int acfm_knn_points(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int N, int P1,
                    int P2, int K, float* dists, int64_t* idx, void* stream);
int acfm_knn_points_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                             const int64_t* idx, const float* grad_dists, int N, int P1, int P2, int K, float* grad_p1,
                             float* grad_p2, void* stream);
int acfm_knn_gather(const float* x, const void* idx, int idx_is_int64, const int64_t* lengths, int N, int M, int U,
                    int L, int K, float* out, void* stream);
int acfm_knn_gather_backward(const float* grad_out, const void* idx, int idx_is_int64, const int64_t* lengths, int N,
                             int M, int U, int L, int K, float* grad_x, void* stream);
/* acfm_edge_length_loss: pytorch3d.loss.mesh_edge_loss on packed meshes: loss = sum_e eweight[e] (|v_a - v_b| - target)^2
 *   (eweight = 1 / edges of the edge's mesh; the caller divides by the mesh count).  verts [P,3], edges [E,2] i64,
 *   eweight [E].  An edge with a vertex outside [0, P) is skipped; the subgradient at a zero-length edge is 0.
 * acfm_normal_consistency: pytorch3d.loss.mesh_normal_consistency: quads [Q,4] i64 = (a, b, c, d), the two faces
 *   (a, b, c) and (a, b, d) on the edge a-b; loss = sum_q qweight[q] (1 - n0.n1 / max(|n0| |n1|, 1e-8)) with
 *   n0 = (c - a) x (b - a), n1 = -((d - a) x (b - a)).
 * Both: one launch, the workgroups' sums meet in a ticket finish (1 ticket word, zero between launches, and
 *   acfm_mesh_term_partial_floats(E or Q) floats, both required); loss is 1 float on the device.  The backward takes
 *   the upstream gradient as a device scalar and adds into grad_verts [P,3], which it zeroes first (float atomics). */
size_t acfm_mesh_term_partial_floats(int count);
int acfm_edge_length_loss(const float* verts, const int64_t* edges, const float* eweight, int P, int E, float target,
                          float* loss, uint32_t* tickets, float* partials, size_t partial_floats, void* stream);
int acfm_edge_length_loss_backward(const float* verts, const int64_t* edges, const float* eweight,
                                   const float* grad_loss, int P, int E, float target, float* grad_verts,
                                   void* stream);
int acfm_normal_consistency(const float* verts, const int64_t* quads, const float* qweight, int P, int Q, float* loss,
                            uint32_t* tickets, float* partials, size_t partial_floats, void* stream);
int acfm_normal_consistency_backward(const float* verts, const int64_t* quads, const float* qweight,
                                     const float* grad_loss, int P, int Q, float* grad_verts, void* stream);

/* ---- texture head: UV image -> face atlas (multiframe/nnutils/mesh_net.py:169-179) ---------------
 * replaces F.grid_sample(uvimage, uv_sampler.repeat(B,1,1,1), align_corners=True) -> reshape / permute to
 * [B,Fp,T,T,3] -> (tanh + 1) / 2 -> cat([tex, tex[:, -nsym:]], 1), and its backward.  float32, 3 channels.
 *   uvimage [B,3,Hu,Wu]; sampler [Fp,T,T,2] = (u, v) in the grid_sample convention (utils/mesh.py:206-232), finite,
 *   constant for the life of the model; atlas [B,Fp+nsym,T,T,3]: face Fp + j holds what face Fp - nsym + j holds.
 *   B, Fp, T >= 1; 0 <= nsym <= Fp; Hu, Wu >= 2; Fp T T <= 2^28, Hu Wu <= 2^30.
 *   Bilinear taps with zero padding: x = ((u + 1) / 2) (Wu - 1), y likewise, corners nw, ne, sw, se of (floor x,
 *   floor y), weights as ATen's, accumulated in that order by fused multiply-adds (as ATen's HIP kernel is built); a
 *   corner outside the image contributes nothing.
 * acfm_uv_atlas_forward: one launch; every element of the atlas is written (no fill needed before it).
 * acfm_uv_atlas_taps: tap_pixel [n_samples,4] i32 = pixel y Wu + x of each sample's four corners, -1 outside -- by
 *   the same device function the forward evaluates.  The caller transposes it ONCE per sampler into the per-pixel
 *   lists the backward walks: pix_start [Hu Wu + 1] i32 (offsets), pix_taps [n_entries] i32 = sample * 4 + corner.
 * acfm_uv_atlas_backward: grad_uvimage[b,c,p] = sum over pixel p's entries, in list order, of
 *   weight * 2 y (1 - y) * (grad_atlas[b,f',t,c] + grad_atlas[b,mirror of f',t,c]), y = atlas[b,f',t,c] as the forward
 *   left it.  One launch, a gather: no float atomics, no zero fill, EVERY pixel written (0 for an empty list), the same
 *   bits on every run.  A list of more than 32 entries is summed by a whole wave (lane-strided partial sums, then a
 *   fixed butterfly); lists may have any length.  n_entries = pix_start[Hu Wu] <= 4 Fp T T; entries outside
 *   [0, 4 Fp T T) are skipped. */
int acfm_uv_atlas_forward(const float* uvimage, const float* sampler, int B, int Hu, int Wu, int Fp, int T, int nsym,
                          float* atlas, void* stream);
int acfm_uv_atlas_taps(const float* sampler, int n_samples, int Hu, int Wu, int32_t* tap_pixel, void* stream);
int acfm_uv_atlas_backward(const float* grad_atlas, const float* atlas, const float* sampler, const int32_t* pix_start,
                           const int32_t* pix_taps, int n_entries, int B, int Hu, int Wu, int Fp, int T, int nsym,
                           float* grad_uvimage, void* stream);

/* ---- geodesic handles: the distances of the lbs initialisation (multiframe/nnutils/mesh_net.py:69-85, 523-544) ----
 * replaces gdist.local_gdist_matrix(verts, faces) there -- by shortest paths on the edge-Steiner graph of the mesh, a
 * certified UPPER BOUND of the exact polyhedral geodesic that gdist computes, not its values (DESIGN.md "Geodesic
 * handles" has the definition and the measured error; nothing could be checked against the gdist package).
 *   verts [N,V,3] f32: N sets of positions on ONE topology.  faces [F,3], edges [E,2] = (lo, hi), lo < hi, in
 *   Meshes.edges_packed() order, face_edges [F,3] = the rows of `edges` of each face's edges: int32 tables the caller
 *   builds once per faces tensor (mesh_net.py:523-544 runs once per model).
 *   Nodes: the V vertices, then m = 0..ACFM_GEODESIC_MAX_STEINER points per edge, node V + e m + (j - 1), j = 1..m, at
 *   a + (j / (m + 1)) (b - a), a = verts[lo], b = verts[hi].  Arcs: inside every face all pairs of the 3 + 3 m nodes on
 *   its boundary (one wave's lanes), length sqrt((dx dx + dy dy) + dz dz), every operation rounded.
 *   out [N,S,V]: out[n,s,v] = the shortest path from vertex sources[s] (i32 [S] on the device; NULL = all V in order,
 *   then S must be V) to vertex v in f32, every hop rounded; 0 at the source, +inf where there is no path.  Every
 *   element is written.  The result is the least fixed point of d_v = min(d_v, fl(d_u + w_uv)), which does not depend
 *   on the order of the relaxations: the same bits on every run.
 * One launch, one workgroup per (source, mesh): all node distances in dynamic LDS, acfm_geodesic_lds_bytes(V, E, m) =
 *   16 + 4 (V + m E) bytes (0 for arguments out of range), at most ACFM_GEODESIC_LDS_MAX; a graph that does not fit is
 *   ACFM_E_BADARG here -- acfm_geodesic_distances_dev below takes it.  No global atomics, nothing shared between
 *   workgroups.
 * status: one i32 on the device, ZERO before the call.  It stays 0 unless a workgroup gave up: 1 = not converged after
 *   V + m E sweeps (the Bellman-Ford bound: cannot happen with arcs >= 0), 2 = a source outside [0, V); that
 *   workgroup's row is NaN.  A face with a table entry out of range is left out of the graph, never dereferenced. */
#define ACFM_GEODESIC_MAX_STEINER 20
#define ACFM_GEODESIC_LDS_MAX 153600
size_t acfm_geodesic_lds_bytes(int V, int E, int m);
int acfm_geodesic_distances(const float* verts, const int32_t* faces, const int32_t* edges, const int32_t* face_edges,
                            int N, int V, int F, int E, int m, const int32_t* sources, int S, float* out,
                            int32_t* status, void* stream);
/* The same distances, bit for bit (the least fixed point of the same operator with the same arc arithmetic), for a graph
 * of any size: the node distances of a workgroup's current (source, mesh) item live in its own row of `ws`, LDS holds
 * only the sweep flags and the clean-face signatures.  One launch of G = min(S N, max_workgroups) persistent
 * workgroups (max_workgroups = 0: two per CU of the current device); workgroup g takes items g, g + G, ... in order and
 * refills its row with +inf for each.  Rows are private, there are no tickets; distances are read, filled and lowered
 * with agent-scope atomics only (the loads bypass the CU's L1: DESIGN.md "Geodesic handles").
 * acfm_geodesic_workspace_bytes: G rows of 4 (V + m E) bytes, each rounded up to 128; 0 for arguments out of range.
 *   ws: that many bytes on the device, 128-byte aligned, any contents; fewer is ACFM_E_WORKSPACE.
 * Arguments, out, status: as acfm_geodesic_distances. */
size_t acfm_geodesic_workspace_bytes(int N, int V, int E, int m, int S, int max_workgroups);
int acfm_geodesic_distances_dev(const float* verts, const int32_t* faces, const int32_t* edges,
                                const int32_t* face_edges, int N, int V, int F, int E, int m, const int32_t* sources,
                                int S, float* out, int32_t* status, int max_workgroups, void* ws, size_t ws_bytes,
                                void* stream);

/* ---- perceptual texture loss: the tail of LPIPS (multiframe/nnutils/loss_utils.py:359-383) --------
 * replaces everything lpips.LPIPS(net='alex', lpips=False, spatial=True) and its caller do around AlexNet's five
 * convolutions (which stay with the framework).  float32, contiguous NCHW.  The definition is restated in DESIGN.md
 * ("Perceptual texture loss"); it could not be checked against the lpips package.
 * References broadcast: prediction n reads reference n mod Nr, N % Nr == 0 (Nr = N / G: once per frame).
 * acfm_lpips_input_forward: x[n,c] = ((2 (img[n,c] m) - 1) - shift_c) / scale_c, m = mask[n mod Nr] [H,W],
 *   shift = (-.030, -.088, -.188), scale = (.458, .448, .450): the bits of that chain of operations.  img is not
 *   read where m == 0 (a NaN there does not propagate, unlike img * 0).
 * acfm_lpips_input_backward: grad_img = ((grad_x / scale_c) 2) m; grad_x is not read where m == 0.
 * acfm_lpips_layer_forward: fa [N,C,hw], fb [Nr,C,hw], lin [C] or NULL (= 1) ->
 *   d[n * d_row_stride + p] = sum_c lin_c (a_c / (|a| + 1e-10) - b_c / (|b| + 1e-10))^2, |.| over the channels of
 *   the pixel.  d_row_stride >= hw: d may be a column block of a wider [N,P] buffer.  C, hw >= 1 arbitrary.
 * acfm_lpips_layer_backward: grad_fa [N,C,hw] from grad_d (same addressing as d), every element written:
 *   q_c = 2 lin_c (u_c - v_c) g,  grad_a_c = q_c / (|a| + eps) - a_c (sum_k q_k a_k) / (|a| (|a| + eps)^2), the second
 *   term 0 where |a| = 0 (there u = 0 by definition and the gradient stays finite; lpips's autograd gives NaN).
 *   d is symmetric: with Nr == N the reference's gradient is the same call with fa and fb exchanged.
 * acfm_lpips_mask_weights: mask [Nr,H,W]; layer_hw = n_layers (<= 8) pairs (h_l, w_l) in HOST memory, read before
 *   the call returns -> M [Nr,P], P = sum h_l w_l, layer l at column sum_{k<l} h_k w_k:
 *   M_l = U_l^T (mask / (H W)), U_l = bilinear upsampling (h_l,w_l) -> (H,W) with align_corners=False as PyTorch
 *   defines it.  Then mean_{H,W}(mask sum_l U_l d_l) = sum_p d[p] M[p].  One launch, every element written.
 * acfm_lpips_masked_mean_forward: loss[n] = sum_p d[n,p] M[n mod Nr,p], d [N,P]; written, never accumulated.
 * acfm_lpips_masked_mean_backward: grad_d[n,p] = grad_loss[n] M[n mod Nr,p].
 * No float atomics, fixed summation orders (bit-reproducible), nothing allocated: every call can be captured. */
int acfm_lpips_input_forward(const float* img, const float* mask, int N, int Nr, int H, int W, float* x, void* stream);
int acfm_lpips_input_backward(const float* grad_x, const float* mask, int N, int Nr, int H, int W, float* grad_img,
                              void* stream);
int acfm_lpips_layer_forward(const float* fa, const float* fb, const float* lin, int N, int Nr, int C, int hw, float* d,
                             size_t d_row_stride, void* stream);
int acfm_lpips_layer_backward(const float* fa, const float* fb, const float* lin, const float* grad_d,
                              size_t grad_d_row_stride, int N, int Nr, int C, int hw, float* grad_fa, void* stream);
int acfm_lpips_mask_weights(const float* mask, int Nr, int H, int W, const int32_t* layer_hw, int n_layers, float* M,
                            void* stream);
int acfm_lpips_masked_mean_forward(const float* d, const float* M, int N, int Nr, int P, float* loss, void* stream);
int acfm_lpips_masked_mean_backward(const float* grad_loss, const float* M, int N, int Nr, int P, float* grad_d,
                                    void* stream);

/* ---- keypoint supervision (multiframe/main.py:503-511, 690-696, 753-762; loss_utils.py:256-289, 330-356) -------------
 * replaces softmax(vert2kp) @ pred_v -> project_points -> kp_l2_loss, the vert2kp entropy prior, the camera head's
 * loss against the most probable hypothesis (or a given camera) and evaluate.py:156-158's pixel error, with their
 * autograd backward.  float32, contiguous.  Limits (else ACFM_E_BADARG): 1 <= K <= 64 keypoints, 1 <= V <= 65535,
 * N <= 65535, N % Nv == 0, N % Ng == 0.  N == 0: returns 0, launches nothing.  No float atomics, no workgroup waits on
 * another, fixed summation orders (bit-reproducible), nothing allocated: every call can be captured.
 * acfm_kp_weights_forward: logits [K,V] -> A = softmax(logits, 1) [K,V]; stats [K,2] = (row maximum, log sum exp of
 *   the shifted row), kept for the backward; entropy [1] = mean_k(-sum_v A logA), logA = (logit - max) - log sum: the
 *   log-softmax form of entropy_loss(A), finite where A underflows to 0.  One launch.
 * acfm_kp_weights_backward: grad_A [K,V] and grad_entropy [1] (device scalar), either may be NULL -> grad_logits [K,V].
 * acfm_kp_head_forward: A [K,V], verts [Nv,V,3], cams [N,7], kp_gt [Ng,K,3] or NULL ->
 *   kp_verts [Nv,K,3] = A @ verts[r]; kp_pred [N,K,2] = (x, y) of orthographic_proj_withz(kp_verts[n % Nv], cams[n], 0):
 *   the bits of acfm_project_xy on kp_verts; with kp_gt (row n % Ng; vis_k = kp_gt[..,2] > 0)
 *   loss [N] = mean_k(vis_k (|dx| + |dy|)) / (mean_k vis_k + 1e-4)  (kp_l2_loss, reduction='none'), and, if kp_err is
 *   not NULL, kp_err [N,K] = sqrt(dx^2 + dy^2) img_size / 2.  Hypothesis n of frame n % Nv: the G = N / Nv hypotheses
 *   of a frame share its vertices (and ground truth); no repeated copy is read.  One launch of Nv workgroups.
 * acfm_kp_head_backward: grad_loss [N], grad_kp_pred [N,K,2], grad_kp_verts [Nv,K,3] (each may be NULL; d|x| at 0 is
 *   0) -> grad_A [K,V], grad_verts [Nv,V,3], grad_cams [N,7] (each may be NULL: not computed).  ws: at least
 *   acfm_kp_head_workspace_bytes(K, Nv) bytes, any contents (fewer: ACFM_E_WORKSPACE).  Two launches, one without grad_A.
 * acfm_camera_loss_forward: cam_pred [N,7] against cam_ref [N,7], or (cam_ref NULL) against row g*(n) N + n of
 *   cams [G N,7] with g*(n) = the first maximum over g of probs [G,N], written to best [N] (int64) ->
 *   loss [1] = mean_n max(1 - |Re(q_pred (x) conj(q_ref))| - margin, 0) + mean_{3N} max((pred - ref)[:3]^2 - margin, 0)
 *   (loss_utils.camera_loss).  One workgroup.
 * acfm_camera_loss_backward: grad_loss [1] -> grad_cam_pred [N,7] (the reference camera gets none); at a hinge tie the
 *   slope is 1/2 (torch.max(a, zeros)), d|x| at 0 is 0.  best: what the forward wrote (cam_ref NULL). */
int acfm_kp_weights_forward(const float* logits, int K, int V, float* A, float* entropy, float* stats, void* stream);
int acfm_kp_weights_backward(const float* logits, const float* A, const float* stats, const float* grad_A,
                             const float* grad_entropy, int K, int V, float* grad_logits, void* stream);
int acfm_kp_head_forward(const float* A, const float* verts, const float* cams, const float* kp_gt, int K, int V, int N,
                         int Nv, int Ng, float img_size, float* kp_verts, float* kp_pred, float* loss, float* kp_err,
                         void* stream);
size_t acfm_kp_head_workspace_bytes(int K, int Nv);
int acfm_kp_head_backward(const float* A, const float* verts, const float* cams, const float* kp_gt,
                          const float* kp_verts, const float* kp_pred, const float* grad_loss, const float* grad_kp_pred,
                          const float* grad_kp_verts, int K, int V, int N, int Nv, int Ng, float* grad_A,
                          float* grad_verts, float* grad_cams, void* ws, size_t ws_bytes, void* stream);
int acfm_camera_loss_forward(const float* cam_pred, const float* cam_ref, const float* cams, const float* probs, int N,
                             int G, float margin, float* loss, int64_t* best, void* stream);
int acfm_camera_loss_backward(const float* cam_pred, const float* cam_ref, const float* cams, const int64_t* best,
                              const float* grad_loss, int N, float margin, float* grad_cam_pred, void* stream);

/* ---- on-device input preparation ----------------------------------------
 * replaces the per-batch CPU work of ShapeTrainer.set_input (multiframe/main.py:365-377) and
 * its device->host->device round trip of the masks.
 * acfm_edt: scipy.ndimage.distance_transform_edt(1 - mask) / divisor for every mask of the batch
 *   (multiframe/utils/image.py:94-102; divisor = 1 for norm=False, max(H,W) for norm=True):
 *   Euclidean distance of every pixel to the nearest pixel with mask == 1 (0 on those pixels).
 *   Exact integer squared distances, sqrt in fp64, one rounding to fp32.
 *   mask [N,H,W] f32 (0/1) -> out [N,H,W] f32. */
size_t acfm_edt_workspace_bytes(int N, int H, int W);
int acfm_edt(const float* mask, int N, int H, int W, int divisor, float* out, void* ws, size_t ws_bytes,
             void* stream);
/* acfm_boundaries: skimage.segmentation.find_boundaries(mask) (mode='thick', connectivity=1) +
 *   the point list of compute_boundaries (multiframe/utils/image.py:122-146): for every mask
 *   the boundary pixels in row-major order as (x, y, valid) with x = (col/W - 0.5)*2,
 *   y = (row/H - 0.5)*2; rows beyond the count are (-1, -1, 0) like the reference's padding.
 *   mask [N,H,W] f32 -> out [N,cap,3] f32 (first min(count, cap) points), counts [N] i32. */
int acfm_boundaries(const float* mask, int N, int H, int W, int cap, float* out, int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACFM_HIP_H_ */
