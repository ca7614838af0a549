// Entry points of the silhouette, hard and texture renders (acfm_sil_*, acfm_hard_raster, acfm_tex_forward,
// acfm_tex_mse_forward, acfm_vertex_color_forward): argument checks, the workspace, and the sequence of launchers
// (acfm_raster.h) of a call -- what NeuralRenderer.forward (nmr.py:143-200, 224-238) strings together from
// PyTorch3D calls; and the finish kernels of the fused losses, which only these entry points launch.
#include "acfm_raster.h"

namespace acfm {

// Fused render + loss, finish: per mesh, the block partials of the raster kernel and sum(gt) over the whole image
// (the blocks without work have m = 0: |m - g| = g, m + g - m g = g) -> out[n] = (mean|m - g|, sum m g,
// sum(m + g - m g), mean e m), the [N,4] vector of k_mask_losses.  Two short launches, FIN_CHUNKS workgroups per mesh
// in the first (one workgroup per mesh was latency-bound: 45 us for 64 meshes); every sum is formed in a fixed
// order (thread-strided partial sums, a fixed tree, then the chunks in order): deterministic, no atomics.
constexpr int FIN_MAX_CHUNKS = 64;   // (sizes ws.lpart2)
static int fin_chunks(int N) {       // enough workgroups to fill the chip at any batch size: ~2048 in all
  int c = 8;
  while (c < FIN_MAX_CHUNKS && c * N < 2048) c *= 2;
  return c;
}
__global__ __launch_bounds__(TPB) void k_sil_loss_finish1(const float4* __restrict__ lpart, const void* __restrict__ gt,
                                                           int tt, int HW, int RB, int h16, float* __restrict__ part2) {
  __shared__ float s_red[TPB][5];
  const int n = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, FIN_CHUNKS = gridDim.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, gs = 0.f;
  const float4* p = lpart + (size_t)n * tt * 4;
  const int np = tt * 4, p_lo = (int)((long long)np * ch / FIN_CHUNKS), p_hi = (int)((long long)np * (ch + 1) / FIN_CHUNKS);
  for (int i = p_lo + tid; i < p_hi; i += TPB) {
    const float4 v = p[i];
    a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
  }
  if (gt) {
    const size_t go = (size_t)(n % RB) * HW;
    if ((HW & 3) == 0) {
      const int q = HW / 4, q_lo = (int)((long long)q * ch / FIN_CHUNKS), q_hi = (int)((long long)q * (ch + 1) / FIN_CHUNKS);
      constexpr int U = 8;                       // loads of a round in flight together
      for (int i0 = q_lo + tid; i0 < q_hi; i0 += TPB * U) {
        float4 v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int i = i0 + u * TPB;
          v[u] = i < q_hi ? ld4_real(gt, go / 4 + i, h16) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) gs += (v[u].x + v[u].y) + (v[u].z + v[u].w);
      }
    } else {
      const int g_lo = (int)((long long)HW * ch / FIN_CHUNKS), g_hi = (int)((long long)HW * (ch + 1) / FIN_CHUNKS);
      for (int i = g_lo + tid; i < g_hi; i += TPB) gs += ld_real(gt, go + i, h16);
    }
  }
  s_red[tid][0] = a0; s_red[tid][1] = a1; s_red[tid][2] = a2; s_red[tid][3] = a3; s_red[tid][4] = gs;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int k = 0; k < 5; ++k) s_red[tid][k] += s_red[tid + s][k];
    __syncthreads();
  }
  if (tid < 5) part2[((size_t)n * FIN_CHUNKS + ch) * 5 + tid] = s_red[0][tid];
}
__global__ void k_sil_loss_finish2(const float* __restrict__ part2, int N, int HW, int FIN_CHUNKS, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float a[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < FIN_CHUNKS; ++c)
#pragma unroll
    for (int k = 0; k < 5; ++k) a[k] += part2[((size_t)n * FIN_CHUNKS + c) * 5 + k];
  const float hw = (float)HW;
  out[4 * (size_t)n + 0] = (a[4] + a[0]) / hw;
  out[4 * (size_t)n + 1] = a[1];
  out[4 * (size_t)n + 2] = a[4] + a[2];
  out[4 * (size_t)n + 3] = a[3] / hw;
}

// Fused texture render + masked MSE, finish: out[n] = (sum over the mesh's blocks of their partial
// + sum_c sum_px (img_c m)^2) / (3 HW) -- the second term is what an uncovered pixel (tex = 0) contributes.
__global__ __launch_bounds__(TPB) void k_tex_loss_finish1(const float4* __restrict__ lpart, const void* __restrict__ timg,
                                                           const void* __restrict__ tmask, int tt, int HW, int RB,
                                                           int h16, float* __restrict__ part2) {
  __shared__ float s_red[TPB];
  const int n = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, FIN_CHUNKS = gridDim.x;
  float acc = 0.f;
  const float4* p = lpart + (size_t)n * tt * 4;
  const int t_lo = (int)((long long)tt * ch / FIN_CHUNKS), t_hi = (int)((long long)tt * (ch + 1) / FIN_CHUNKS);
  for (int i = t_lo + tid; i < t_hi; i += TPB) acc += p[4 * (size_t)i].x;
  const size_t rn = (size_t)(n % RB);
  const size_t mo = rn * HW, io = rn * 3 * HW;
  if ((HW & 3) == 0) {
    const int q = HW / 4, q_lo = (int)((long long)q * ch / FIN_CHUNKS), q_hi = (int)((long long)q * (ch + 1) / FIN_CHUNKS);
    constexpr int U = 4;
    for (int i0 = q_lo + tid; i0 < q_hi; i0 += TPB * U) {
      float4 mk[U], c0[U], c1[U], c2[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u * TPB;
        const bool in = i < q_hi;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        mk[u] = in ? ld4_real(tmask, mo / 4 + i, h16) : z;
        c0[u] = in ? ld4_real(timg, io / 4 + i, h16) : z;
        c1[u] = in ? ld4_real(timg, (io + HW) / 4 + i, h16) : z;
        c2[u] = in ? ld4_real(timg, (io + 2 * (size_t)HW) / 4 + i, h16) : z;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        auto sq = [](float a, float b) { const float v = a * b; return v * v; };
        acc += (sq(c0[u].x, mk[u].x) + sq(c1[u].x, mk[u].x) + sq(c2[u].x, mk[u].x)) +
               (sq(c0[u].y, mk[u].y) + sq(c1[u].y, mk[u].y) + sq(c2[u].y, mk[u].y)) +
               (sq(c0[u].z, mk[u].z) + sq(c1[u].z, mk[u].z) + sq(c2[u].z, mk[u].z)) +
               (sq(c0[u].w, mk[u].w) + sq(c1[u].w, mk[u].w) + sq(c2[u].w, mk[u].w));
      }
    }
  } else {
    const int g_lo = (int)((long long)HW * ch / FIN_CHUNKS), g_hi = (int)((long long)HW * (ch + 1) / FIN_CHUNKS);
    for (int i = g_lo + tid; i < g_hi; i += TPB) {
      const float mk = ld_real(tmask, mo + i, h16);
      const float b0 = ld_real(timg, io + i, h16) * mk, b1 = ld_real(timg, io + HW + i, h16) * mk,
                  b2 = ld_real(timg, io + 2 * (size_t)HW + i, h16) * mk;
      acc += b0 * b0 + b1 * b1 + b2 * b2;
    }
  }
  s_red[tid] = acc;
  __syncthreads();
  for (int s = TPB / 2; s > 0; s >>= 1) {
    if (tid < s) s_red[tid] += s_red[tid + s];
    __syncthreads();
  }
  if (tid == 0) part2[(size_t)n * FIN_CHUNKS + ch] = s_red[0];
}
__global__ void k_tex_loss_finish2(const float* __restrict__ part2, int N, int HW, int FIN_CHUNKS, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  float a = 0.f;
  for (int c = 0; c < FIN_CHUNKS; ++c) a += part2[(size_t)n * FIN_CHUNKS + c];
  out[n] = a / (3.0f * (float)HW);
}

}  // namespace acfm

using namespace acfm;

extern "C" {

static int sil_forward_impl(const float* verts_world, const int64_t* faces, const float* cams, int N, int V,
                            int F, int H, int K, int k_out, float blur_radius, float sigma, float offset_z,
                            void* mask, void* pix_to_face, uint64_t* kth, uint8_t* vis, void* wsp,
                            size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream, bool fused,
                            const void* gt, const void* edt, int ref_batch, float* losses,
                            const AcfmSilExtras* ex) {
  float* pf_imgs = ex ? ex->tex_imgs : nullptr;
  float* pf_sil = ex ? ex->tex_sil : nullptr;
  int64_t* pf_p2f = ex ? ex->tex_pix_to_face : nullptr;
  int32_t* pf_tidx = ex ? ex->tex_texel_idx : nullptr;
  if (!verts_world || !faces || !cams || !mask || !pix_to_face || !wsp) return ACFM_E_BADARG;
  if (fused && (!losses || ref_batch <= 0 || N % ref_batch != 0)) return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || K < 2 || K > ACFM_MAX_K || !(sigma > 0.f) || blur_radius < 0.f ||
      (k_out != K && k_out != 1))
    return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn)) return ACFM_E_BADARG;
  if (tn.f16 && k_out != 1) return ACFM_E_BADARG;      // half storage goes with the int32 nearest-face plane
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);
  if (ws.bytes > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_setup(verts_world, faces, cams, N, V, F, H, offset_z, 0, blur_radius, ws, tn, st, vis,
                        ex ? ex->proj_xy : nullptr);
  if (rc) return rc;
  FwdOut out = {};
  out.dbg = stamp_buffer();
  out.h16 = tn.f16 ? 1 : 0;
  out.mask = mask;
  out.p2f = pix_to_face;
  out.kout = k_out;
  out.kth = reinterpret_cast<unsigned long long*>(kth);
  out.vis = vis;
  out.V = V;
  out.sig_scale = 1.44269504088896341f / sigma;
  out.lrb = 1;
  if (tn.cover) out.cover_out = ws.cover;
  if (pf_imgs || pf_sil || pf_p2f || pf_tidx) {   // all four or none; only with the cover plane (the texture render it prepares shades from it) and float storage
    if (!pf_sil || !pf_p2f || !pf_tidx || !tn.cover || tn.f16) return ACFM_E_BADARG;
    out.pf_imgs = pf_imgs; out.pf_sil = pf_sil; out.pf_p2f = pf_p2f; out.pf_tidx = pf_tidx;
  }
  if (fused) { out.lgt = gt; out.ledt = edt; out.lrb = ref_batch; out.lpart = ws.lpart; }
  rc = launch_sil_fwd(K, ws, N, F, H, blur_radius, sigma, out, tn, st);   // supported K: 2, 4, 8, 10, 20, 32
  if (rc || !fused) return rc;
  const int tiles = (H + RBLK - 1) / RBLK;
  ProfScope ps(ACFM_PROF_MASK_LOSS, st);
  const int fc = fin_chunks(N);
  hipLaunchKernelGGL(k_sil_loss_finish1, dim3(fc, N), dim3(TPB), 0, st, ws.lpart, gt, tiles * tiles, H * H,
                     ref_batch, out.h16, ws.lpart2);
  hipLaunchKernelGGL(k_sil_loss_finish2, dim3((N + 63) / 64), dim3(64), 0, st, ws.lpart2, N, H * H, fc, losses);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_sil_forward(const float* verts_world, const int64_t* faces, const float* cams, int N, int V,
                     int F, int H, int K, int k_out, float blur_radius, float sigma, float offset_z,
                     void* mask, void* pix_to_face, uint64_t* kth, uint8_t* vis, void* wsp,
                     size_t ws_bytes, const AcfmRasterTuning* tuning, const AcfmSilExtras* extras, void* stream) {
  return sil_forward_impl(verts_world, faces, cams, N, V, F, H, K, k_out, blur_radius, sigma, offset_z, mask,
                          pix_to_face, kth, vis, wsp, ws_bytes, tuning, stream, false, nullptr, nullptr, 1, nullptr, extras);
}

int acfm_sil_loss_forward(const float* verts_world, const int64_t* faces, const float* cams, const void* gt,
                          const void* edt, int ref_batch, int N, int V, int F, int H, int K, int k_out,
                          float blur_radius, float sigma, float offset_z, void* mask, void* pix_to_face,
                          uint64_t* kth, uint8_t* vis, float* losses, void* wsp, size_t ws_bytes,
                          const AcfmRasterTuning* tuning, const AcfmSilExtras* extras, void* stream) {
  return sil_forward_impl(verts_world, faces, cams, N, V, F, H, K, k_out, blur_radius, sigma, offset_z, mask,
                          pix_to_face, kth, vis, wsp, ws_bytes, tuning, stream, true, gt, edt, ref_batch, losses, extras);
}

static int sil_backward_impl(const float* verts_world, const int64_t* faces, const float* cams,
                             const void* mask, const uint64_t* kth, BwdGrad bg, int N, int V,
                             int F, int H, float blur_radius, float sigma, float offset_z, float* grad_verts,
                             float* grad_cams, void* wsp, size_t ws_bytes, int ws_from_forward,
                             const AcfmRasterTuning* tuning, void* stream, const float* gproj) {
  if (!verts_world || !faces || !cams || !mask || !kth || !wsp) return ACFM_E_BADARG;
  if (!bg.grad_mask && (!bg.go || bg.lrb <= 0 || N % bg.lrb != 0)) return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || !(sigma > 0.f) || blur_radius < 0.f) return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn)) return ACFM_E_BADARG;
  bg.h16 = tn.f16 ? 1 : 0;
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);   // (same tuning as the forward whose workspace this is)
  if (ws.bytes > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (!ws_from_forward) {
    int rc = launch_setup(verts_world, faces, cams, N, V, F, H, offset_z, 0, blur_radius, ws, tn, st);
    if (rc) return rc;
  }
  if (!grad_verts && !grad_cams) return ACFM_OK;   // nothing asked for
  // ws.grad_ndc is zero here: k_setup cleared it, and every k_project_bwd<1> clears it again after reading
  {
    ProfScope ps(ACFM_PROF_SIL_BWD, st);
    launch_sil_bwd(ws, mask, reinterpret_cast<const unsigned long long*>(kth), bg, N, V, F, H, blur_radius, sigma, tn, st);
  }
  ACFM_CHECK_LAUNCH();
  if (grad_verts || grad_cams) {
    ProfScope ps(ACFM_PROF_PROJ_BWD, st);
    launch_project_bwd_ndc(tn.deterministic, verts_world, cams, ws, N, V, grad_verts, grad_cams, gproj, st);
    ACFM_CHECK_LAUNCH();
  }
  return ACFM_OK;
}

int acfm_sil_backward(const float* verts_world, const int64_t* faces, const float* cams,
                      const void* mask, const uint64_t* kth, const float* grad_mask, int N, int V,
                      int F, int H, float blur_radius, float sigma, float offset_z, float* grad_verts,
                      float* grad_cams, void* wsp, size_t ws_bytes, int ws_from_forward,
                      const AcfmRasterTuning* tuning, const AcfmSilExtras* extras, void* stream) {
  if (!grad_mask) return ACFM_E_BADARG;
  BwdGrad bg = {};
  bg.grad_mask = grad_mask;
  bg.lrb = 1;
  return sil_backward_impl(verts_world, faces, cams, mask, kth, bg, N, V, F, H, blur_radius, sigma, offset_z,
                           grad_verts, grad_cams, wsp, ws_bytes, ws_from_forward, tuning, stream,
                           extras ? extras->grad_proj_xy : nullptr);
}

int acfm_sil_loss_backward(const float* verts_world, const int64_t* faces, const float* cams, const void* mask,
                           const uint64_t* kth, const void* gt, const void* edt, int ref_batch,
                           const float* grad_losses, int N, int V, int F, int H, float blur_radius, float sigma,
                           float offset_z, float* grad_verts, float* grad_cams, void* wsp, size_t ws_bytes,
                           int ws_from_forward, const AcfmRasterTuning* tuning, const AcfmSilExtras* extras,
                           void* stream) {
  if (!grad_losses) return ACFM_E_BADARG;
  BwdGrad bg = {};
  bg.lgt = gt; bg.ledt = edt; bg.go = grad_losses; bg.lrb = ref_batch;
  return sil_backward_impl(verts_world, faces, cams, mask, kth, bg, N, V, F, H, blur_radius, sigma, offset_z,
                           grad_verts, grad_cams, wsp, ws_bytes, ws_from_forward, tuning, stream,
                           extras ? extras->grad_proj_xy : nullptr);
}

int acfm_hard_raster(const float* verts_proj, const int64_t* faces, int N, int V, int F, int H,
                     int64_t* pix_to_face, uint8_t* vis, void* wsp, size_t ws_bytes,
                     const AcfmRasterTuning* tuning, void* stream) {
  if (!verts_proj || !faces || !pix_to_face || !wsp || bad_dims(N, V, F, H)) return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn) || tn.f16) return ACFM_E_BADARG;
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);
  if (ws.bytes > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_setup(verts_proj, faces, nullptr, N, V, F, H, 0.f, 1, 0.f, ws, tn, st, vis);
  if (rc) return rc;
  FwdOut out = {};
  out.dbg = stamp_buffer();
  out.p2f = pix_to_face;
  out.vis = vis;
  out.V = V;
  ProfScope ps(ACFM_PROF_HARD_FWD, st);
  launch_k1_fwd(false, ws, N, F, H, 1e-4f, out, tn, st);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

static int tex_forward_impl(const float* verts_world, const int64_t* faces, const float* cams,
                            const void* atlas, int N, int V, int F, int H, int R, float sigma, float gamma,
                            float offset_z, void* imgs, void* sil, void* pix_to_face, int32_t* texel_idx,
                            void* wsp, size_t ws_bytes, int ws_ready, float ws_blur, int atlas_batch,
                            const AcfmRasterTuning* tuning, void* stream, const void* ref_img,
                            const void* ref_mask, int ref_batch, float* loss) {
  if (!verts_world || !faces || !cams || !atlas || !imgs || !sil || !pix_to_face || !texel_idx || !wsp)
    return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || R <= 0 || R > 256 || !(sigma > 0.f) || !(gamma > 0.f)) return ACFM_E_BADARG;
  if (atlas_batch <= 0 || N % atlas_batch != 0) return ACFM_E_BADARG;
  if ((size_t)atlas_batch * F * R * R > 0x7fffffffull) return ACFM_E_BADARG;  // texel_idx is int32
  Tune tn;
  if (!tune_from(tuning, tn)) return ACFM_E_BADARG;
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);
  if (ws.bytes > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (ws_ready && !(ws_blur >= 0.f)) return ACFM_E_BADARG;
  if (!ws_ready) {
    int rc = launch_setup(verts_world, faces, cams, N, V, F, H, offset_z, 0, 0.f, ws, tn, st);
    if (rc) return rc;
  }
  FwdOut out = {};
  out.dbg = stamp_buffer();
  out.p2f = pix_to_face;
  out.atlas = atlas; out.imgs = imgs; out.sil = sil; out.tidx = texel_idx; out.R = R; out.gamma = gamma;
  out.atlas_n = atlas_batch;
  out.h16 = tn.f16 ? 1 : 0;
  out.box_shrink = ws_ready ? sqrtf(ws_blur) * (1.0f - 1e-5f) : 0.f;
  out.lrb = 1;
  if (ws_ready < 0 || ws_ready > 3) return ACFM_E_BADARG;
  if (ws_ready >= 2) {
    if (!tn.cover) return ACFM_E_BADARG;   // the tuning of the render that filled the workspace says whether the plane is there
    out.cover_in = ws.cover;
    if (ws_ready == 3) {                   // ... and that render (acfm_sil_forward_prefill) stored the empty blocks' constants
      if (tn.f16) return ACFM_E_BADARG;
      out.prefilled = 1;
    }
  }
  if (loss) {
    if (!ref_img || !ref_mask || ref_batch <= 0 || N % ref_batch != 0) return ACFM_E_BADARG;
    out.timg = ref_img; out.tmask = ref_mask; out.lrb = ref_batch; out.lpart = ws.lpart;
  }
  {
    ProfScope ps(ACFM_PROF_TEX_FWD, st);
    if (out.cover_in) launch_tex_cover(ws, N, F, H, sigma, out, tn, st);
    else launch_k1_fwd(true, ws, N, F, H, sigma, out, tn, st);
    ACFM_CHECK_LAUNCH();
  }
  if (loss) {
    const int tiles = (H + RBLK - 1) / RBLK;
    ProfScope ps(ACFM_PROF_TEX_MSE, st);
    const int fc = fin_chunks(N);
    hipLaunchKernelGGL(k_tex_loss_finish1, dim3(fc, N), dim3(TPB), 0, st, ws.lpart, ref_img, ref_mask,
                       tiles * tiles, H * H, ref_batch, out.h16, ws.lpart2);
    hipLaunchKernelGGL(k_tex_loss_finish2, dim3((N + 63) / 64), dim3(64), 0, st, ws.lpart2, N, H * H, fc, loss);
    ACFM_CHECK_LAUNCH();
  }
  return ACFM_OK;
}

int acfm_tex_forward(const float* verts_world, const int64_t* faces, const float* cams,
                     const void* atlas, int N, int V, int F, int H, int R, float sigma, float gamma,
                     float offset_z, void* imgs, void* sil, void* pix_to_face, int32_t* texel_idx,
                     void* wsp, size_t ws_bytes, int ws_ready, float ws_blur, int atlas_batch,
                     const AcfmRasterTuning* tuning, void* stream) {
  return tex_forward_impl(verts_world, faces, cams, atlas, N, V, F, H, R, sigma, gamma, offset_z, imgs, sil,
                          pix_to_face, texel_idx, wsp, ws_bytes, ws_ready, ws_blur, atlas_batch, tuning, stream,
                          nullptr, nullptr, 1, nullptr);
}

int acfm_tex_mse_forward(const float* verts_world, const int64_t* faces, const float* cams, const void* atlas,
                         const void* ref_img, const void* ref_mask, int ref_batch, int N, int V, int F, int H, int R,
                         float sigma, float gamma, float offset_z, void* imgs, void* sil, void* pix_to_face,
                         int32_t* texel_idx, float* loss, void* wsp, size_t ws_bytes, int ws_ready, float ws_blur,
                         int atlas_batch, const AcfmRasterTuning* tuning, void* stream) {
  if (!loss) return ACFM_E_BADARG;
  return tex_forward_impl(verts_world, faces, cams, atlas, N, V, F, H, R, sigma, gamma, offset_z, imgs, sil,
                          pix_to_face, texel_idx, wsp, ws_bytes, ws_ready, ws_blur, atlas_batch, tuning, stream,
                          ref_img, ref_mask, ref_batch, loss);
}

int acfm_vertex_color_forward(const float* verts_world, const int64_t* faces, const float* cams,
                              const float* verts_rgb, int N, int V, int F, int H, float sigma, float gamma,
                              float offset_z, float* imgs, float* sil, int64_t* pix_to_face, void* wsp,
                              size_t ws_bytes, int ws_ready, float ws_blur, const AcfmRasterTuning* tuning,
                              void* stream) {
  if (!verts_world || !faces || !cams || !verts_rgb || !imgs || !sil || !pix_to_face || !wsp) return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || !(sigma > 0.f) || !(gamma > 0.f)) return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn) || tn.f16) return ACFM_E_BADARG;
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);
  if (ws.bytes + sizeof(int32_t) * (size_t)N * H * H > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (ws_ready && !(ws_blur >= 0.f)) return ACFM_E_BADARG;
  if (!ws_ready) {
    int rc = launch_setup(verts_world, faces, cams, N, V, F, H, offset_z, 0, 0.f, ws, tn, st);
    if (rc) return rc;
  }
  FwdOut out = {};
  out.dbg = stamp_buffer();
  out.p2f = pix_to_face;
  out.vrgb = verts_rgb; out.V = V; out.atlas_n = N;
  out.box_shrink = ws_ready ? sqrtf(ws_blur) * (1.0f - 1e-5f) : 0.f;
  out.imgs = imgs; out.sil = sil; out.tidx = (int32_t*)((char*)wsp + ws.bytes); out.R = 1; out.gamma = gamma;
  out.atlas = verts_rgb;  // never dereferenced when vrgb is set
  ProfScope ps(ACFM_PROF_TEX_FWD, st);
  launch_k1_fwd(true, ws, N, F, H, sigma, out, tn, st);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
