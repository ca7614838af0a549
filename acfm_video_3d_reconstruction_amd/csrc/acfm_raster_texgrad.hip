// Gradient of the texture render with respect to the atlas: k_tex_bwd, k_tex_bwd_faces and the acfm_tex_backward*
// entry points.  Replaces the autograd backward through TexturesAtlas.sample_textures and the K = 1 blend.
//   * k_tex_bwd_faces: the atlas gradient as a per-face gather over the face's box (no global
//     atomics); k_tex_bwd: the scatter form (one atomic per covered pixel and channel).
#include "acfm_raster.h"

namespace acfm {

// ------------------------------------------------------------------------------- texture bwd
__global__ void k_tex_bwd(const float* __restrict__ grad_imgs, const int32_t* __restrict__ tidx,
                          size_t HW, size_t total, float* __restrict__ grad_atlas) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int32_t t = tidx[i];
  if (t < 0) return;
  const size_t n = i / HW, p = i % HW;
  const float* g = grad_imgs + n * 3 * HW + p;
  // d rgb / d texel = wnum / (wnum + delta) = 1 in fp32 (wnum >= 0.5, delta = 1e-10)
  atomicAdd(&grad_atlas[(size_t)t * 3 + 0], g[0]);
  atomicAdd(&grad_atlas[(size_t)t * 3 + 1], g[HW]);
  atomicAdd(&grad_atlas[(size_t)t * 3 + 2], g[2 * HW]);
}
// Gather form of the same gradient, one wave per four (atlas, face) slots: for each it visits the pixels of the
// face's box in every mesh that samples this atlas (the G hypotheses of a frame), adds the
// gradients of the pixels whose texel belongs to the face into 3 R^2 LDS accumulators and stores
// the face's texels -- zeros included -- with plain coalesced stores.  No global atomics (agent-
// scope float atomics execute at the memory side on this multi-XCD part: 2 M of them took 87 us)
// and no zero fill of the 35 MB gradient.  Needs the face boxes of the forward's workspace.
// i / w and i % w for 0 <= i < 2^23, 0 < w < 2^12 without the ~35-instruction integer division
__device__ __forceinline__ void divmod_small(int i, int w, float rw, int& q, int& r) {
  q = (int)((float)i * rw);
  r = i - q * w;
  if (r < 0) { --q; r += w; }
  if (r >= w) { ++q; r -= w; }
}
constexpr int TEXG_MAX_R = 8;
constexpr int TEXG_FPW = 4;      // faces per wave: their boxes, texel indices and gradients are loaded side by side
constexpr int TEXG_U = 2;        // big boxes: 64 U pixels per round, all their loads in flight together
constexpr int TEXG_WAVES = 8;    // waves per SIMD (U = 2 at 8 waves: 39.8 us per launch; U = 4 at 6 waves 41.4; U = 8 at 5 waves -- 92 VGPRs -- 45.2)
// Upstream gradient of the rendered image: given ([N,3,H,H]) or, for the fused texture render + masked MSE, formed
// on the fly from the rendered image, the reference image and mask and the per-mesh gradient of the loss --
// k_tex_mse_bwd's expression: w (tex m - img m) m with w = go[n] 2 / (3 HW).
struct TexGrad {
  const float* grad_imgs;    // [N,3,H,H] (always float), or null: fused
  const void* imgs;          // [N,3,H,H] real_t, the forward's output
  const void* timg;          // [rb,3,H,H] real_t
  const void* tmask;         // [rb,H,H] real_t
  const float* go;           // [N]
  int rb;
  int h16;
};
struct TexGradN {            // the same for one mesh n
  const float* g;
  const void *im, *ri, *rm;
  size_t io, ro, mo;
  float w;
  size_t HW;
  int h16;
  __device__ __forceinline__ void load(size_t p, float& r, float& gg, float& b) const {
    if (g) { r = g[p]; gg = g[HW + p]; b = g[2 * HW + p]; return; }
    const float mk = ld_real(rm, mo + p, h16);
    r = w * (ld_real(im, io + p, h16) * mk - ld_real(ri, ro + p, h16) * mk) * mk;
    gg = w * (ld_real(im, io + HW + p, h16) * mk - ld_real(ri, ro + HW + p, h16) * mk) * mk;
    b = w * (ld_real(im, io + 2 * HW + p, h16) * mk - ld_real(ri, ro + 2 * HW + p, h16) * mk) * mk;
  }
};
__device__ __forceinline__ TexGradN tex_grad_of(const TexGrad& tg, int n, size_t HW) {
  TexGradN t = {};
  t.HW = HW;
  if (tg.grad_imgs) { t.g = tg.grad_imgs + (size_t)n * 3 * HW; return t; }
  const size_t rn = (size_t)(n % tg.rb);
  t.im = tg.imgs; t.ri = tg.timg; t.rm = tg.tmask; t.h16 = tg.h16;
  t.io = (size_t)n * 3 * HW; t.ro = rn * 3 * HW; t.mo = rn * HW;
  t.w = tg.go[n] * 2.0f / (3.0f * (float)HW);
  return t;
}
__global__ __launch_bounds__(256, TEXG_WAVES) void k_tex_bwd_faces(RasterWs ws, TexGrad tgrad,
                                                       const int32_t* __restrict__ tidx, int N, int F, int H,
                                                       int R, int NA, float box_shrink,
                                                       float* __restrict__ grad_atlas) {
  __shared__ float s_acc[4][TEXG_FPW][3 * TEXG_MAX_R * TEXG_MAX_R];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // Wave q of the launch takes the faces q, q + Q, q + 2Q, q + 3Q of one atlas (Q = ceil(F / FPW)):
  // neighbouring faces of a mesh tend to be large together, and a wave walks its faces' boxes one
  // after the other, so they are dealt to different waves.
  const int Q = (F + TEXG_FPW - 1) / TEXG_FPW;
  const long long wq = (long long)blockIdx.x * 4 + wv;
  if (wq >= (long long)NA * Q) return;                       // (whole wave; no workgroup barriers below)
  const int a = (int)(wq / Q), f0 = (int)(wq % Q);
  const int R2 = R * R, n3 = 3 * R2;
  float (*acc)[3 * TEXG_MAX_R * TEXG_MAX_R] = s_acc[wv];
#pragma unroll
  for (int k = 0; k < TEXG_FPW; ++k)
    for (int i = lane; i < n3; i += 64) acc[k][i] = 0.f;
  wave_lds_sync();
  const size_t HW = (size_t)H * H;
  const float hf = (float)H;
  // lane k < FPW looks after face f0 + k Q
  const int my_f = f0 + (lane < TEXG_FPW ? lane : 0) * Q;
  const bool my_live = lane < TEXG_FPW && my_f < F;
  const int G = N / NA;
  for (int g = 0; g < G; ++g) {
    // the FPW boxes (mesh a + g NA), one per lane, turned into pixel ranges (k_setup's formula, one pixel of slack)
    int xa = 0, ya = 0, w = 1, cnt = 0;
    const int n = a + g * NA;
    if (my_live && ws.fvis[(size_t)n * F + my_f]) {          // (a face no pixel shows has no gradient: zeros)
      float4 b = ws.rec[(size_t)n * F + my_f].box;
      b.x += box_shrink; b.y -= box_shrink; b.z += box_shrink; b.w -= box_shrink;
      if (b.x <= b.y && b.z <= b.w) {                        // not a degenerate face (inf, -inf, ..) or an emptied box
        // pixel range of the box: k_setup's formula with one pixel of slack, then tightened to the
        // pixels that pass the forward's own test (pixel centre inside the box, same float expressions)
        xa = (int)floorf(hf - 1.0f - ((b.y + 1.0f) * hf - 1.0f) * 0.5f) - 1;
        int xb = (int)ceilf(hf - 1.0f - ((b.x + 1.0f) * hf - 1.0f) * 0.5f) + 1;
        ya = (int)floorf(hf - 1.0f - ((b.w + 1.0f) * hf - 1.0f) * 0.5f) - 1;
        int yb = (int)ceilf(hf - 1.0f - ((b.z + 1.0f) * hf - 1.0f) * 0.5f) + 1;
        if (!(xb < 0 || yb < 0 || xa >= H || ya >= H)) {
          xa = max(xa, 0); ya = max(ya, 0); xb = min(xb, H - 1); yb = min(yb, H - 1);
          for (int it = 0; it < 3 && xa <= xb && pix_to_ndc(H - 1 - xa, H) > b.y; ++it) ++xa;
          for (int it = 0; it < 3 && xa <= xb && pix_to_ndc(H - 1 - xb, H) < b.x; ++it) --xb;
          for (int it = 0; it < 3 && ya <= yb && pix_to_ndc(H - 1 - ya, H) > b.w; ++it) ++ya;
          for (int it = 0; it < 3 && ya <= yb && pix_to_ndc(H - 1 - yb, H) < b.z; ++it) --yb;
          if (xa <= xb && ya <= yb) { w = xb - xa + 1; cnt = w * (yb - ya + 1); }
        }
      }
    }
    const int32_t* tn = tidx + (size_t)n * HW;
    const TexGradN gn = tex_grad_of(tgrad, n, HW);
    int cmax = 0;
    int t[TEXG_FPW];
    size_t pp[TEXG_FPW];
#pragma unroll
    for (int k = 0; k < TEXG_FPW; ++k) {                     // all texel-index loads first ...
      const int kxa = __shfl(xa, k, 64), kya = __shfl(ya, k, 64), kw = __shfl(w, k, 64), kc = __shfl(cnt, k, 64);
      const int kbase = (a * F + f0 + k * Q) * R2;           // first texel index of the face (< 2^31: host check)
      cmax = max(cmax, kc);
      t[k] = -1;
      pp[k] = 0;
      if (lane < kc) {
        int qy, qx;
        divmod_small(lane, kw, __builtin_amdgcn_rcpf((float)kw), qy, qx);
        pp[k] = (size_t)(kya + qy) * H + (kxa + qx);
        t[k] = tn[pp[k]] - kbase;
      }
    }
#pragma unroll
    for (int k = 0; k < TEXG_FPW; ++k) {                     // ... then the gradients of the pixels that belong to the face
      if (t[k] >= 0 && t[k] < R2) {
        // d rgb / d texel = wnum / (wnum + delta) = 1 in fp32 (wnum >= 0.5, delta = 1e-10)
        float r, gg, bb;
        gn.load(pp[k], r, gg, bb);
        atomicAdd(&acc[k][3 * t[k] + 0], r);
        atomicAdd(&acc[k][3 * t[k] + 1], gg);
        atomicAdd(&acc[k][3 * t[k] + 2], bb);
      }
    }
    if (cmax > 64) {   // boxes of more than 64 pixels (a third of the bird's): the rest face by face, 64 U pixels per round
      for (int k = 0; k < TEXG_FPW; ++k) {
        const int kxa = __shfl(xa, k, 64), kya = __shfl(ya, k, 64), kw = __shfl(w, k, 64), kc = __shfl(cnt, k, 64);
        const int kbase = (a * F + f0 + k * Q) * R2;
        const float rw = __builtin_amdgcn_rcpf((float)kw);
        for (int i0 = 64 + lane; i0 < kc + lane; i0 += 64 * TEXG_U) {   // (i0 - lane is wave-uniform)
          int tt[TEXG_U];
          float cr[TEXG_U], cg[TEXG_U], cb[TEXG_U];
#pragma unroll
          for (int u = 0; u < TEXG_U; ++u) {
            const int i = i0 + 64 * u;
            tt[u] = -1; cr[u] = 0.f; cg[u] = 0.f; cb[u] = 0.f;
            if (i < kc) {
              int qy, qx;
              divmod_small(i, kw, rw, qy, qx);
              const size_t p = (size_t)(kya + qy) * H + (kxa + qx);
              tt[u] = tn[p] - kbase;
              gn.load(p, cr[u], cg[u], cb[u]);                              // unconditionally: one round trip per round
            }
          }
#pragma unroll
          for (int u = 0; u < TEXG_U; ++u)
            if (tt[u] >= 0 && tt[u] < R2) {
              atomicAdd(&acc[k][3 * tt[u] + 0], cr[u]);
              atomicAdd(&acc[k][3 * tt[u] + 1], cg[u]);
              atomicAdd(&acc[k][3 * tt[u] + 2], cb[u]);
            }
        }
      }
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < TEXG_FPW; ++k) {
    if (f0 + k * Q >= F) break;
    float* o = grad_atlas + (size_t)(a * F + f0 + k * Q) * n3;
    for (int i = lane; i < n3; i += 64) o[i] = acc[k][i];
  }
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_tex_backward(const float* grad_imgs, const int32_t* texel_idx, int N, int F, int H, int R,
                      int atlas_batch, float* grad_atlas, void* stream) {
  if (!grad_imgs || !texel_idx || !grad_atlas || N <= 0 || F <= 0 || H <= 0 || R <= 0 || atlas_batch <= 0 ||
      N % atlas_batch != 0)
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t total = (size_t)N * H * H;
  if (zero_async(grad_atlas, sizeof(float) * 3 * (size_t)atlas_batch * F * R * R, st) != ACFM_OK)
    return ACFM_E_LAUNCH;
  ProfScope ps(ACFM_PROF_TEX_BWD, st);
  hipLaunchKernelGGL(k_tex_bwd, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, grad_imgs,
                     texel_idx, (size_t)H * H, total, grad_atlas);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

static int tex_backward_faces_impl(const TexGrad& tgrad, const int32_t* texel_idx, const void* wsp, size_t ws_bytes,
                                   float ws_blur, int N, int V, int F, int H, int R, int atlas_batch,
                                   float* grad_atlas, void* stream) {
  if (!texel_idx || !grad_atlas || !wsp) return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || R <= 0 || R > TEXG_MAX_R || atlas_batch <= 0 || N % atlas_batch != 0 || !(ws_blur >= 0.f))
    return ACFM_E_BADARG;
  if ((size_t)atlas_batch * F * R * R > 0x7fffffffull) return ACFM_E_BADARG;
  const RasterWs ws = carve_ws(const_cast<void*>(wsp), N, V, F, H);
  if (ws.bytes > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const size_t waves = (size_t)atlas_batch * ((F + TEXG_FPW - 1) / TEXG_FPW);
  ProfScope ps(ACFM_PROF_TEX_BWD, st);
  hipLaunchKernelGGL(k_tex_bwd_faces, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, ws, tgrad, texel_idx,
                     N, F, H, R, atlas_batch, ws_blur > 0.f ? sqrtf(ws_blur) * (1.0f - 1e-5f) : 0.f, grad_atlas);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_tex_backward_faces(const float* grad_imgs, const int32_t* texel_idx, const void* wsp, size_t ws_bytes,
                            float ws_blur, int N, int V, int F, int H, int R, int atlas_batch, float* grad_atlas,
                            void* stream) {
  if (!grad_imgs) return ACFM_E_BADARG;
  TexGrad tg = {};
  tg.grad_imgs = grad_imgs;
  tg.rb = 1;
  return tex_backward_faces_impl(tg, texel_idx, wsp, ws_bytes, ws_blur, N, V, F, H, R, atlas_batch, grad_atlas, stream);
}

int acfm_tex_mse_backward_faces(const void* imgs, const void* ref_img, const void* ref_mask, int ref_batch,
                                const float* grad_loss, const int32_t* texel_idx, const void* wsp, size_t ws_bytes,
                                float ws_blur, int N, int V, int F, int H, int R, int atlas_batch, float* grad_atlas,
                                const AcfmRasterTuning* tuning, void* stream) {
  if (!imgs || !ref_img || !ref_mask || !grad_loss || ref_batch <= 0 || N <= 0 || N % ref_batch != 0) return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn)) return ACFM_E_BADARG;
  TexGrad tg = {};
  tg.h16 = tn.f16 ? 1 : 0;
  tg.imgs = imgs; tg.timg = ref_img; tg.tmask = ref_mask; tg.go = grad_loss; tg.rb = ref_batch;
  return tex_backward_faces_impl(tg, texel_idx, wsp, ws_bytes, ws_blur, N, V, F, H, R, atlas_batch, grad_atlas, stream);
}

}  // extern "C"
