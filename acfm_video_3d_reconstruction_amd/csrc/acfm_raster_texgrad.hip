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
// the face's texels -- zeros included -- with plain coalesced stores.  Per mesh a wave makes two load round
// trips: the four flags and boxes together, then -- the four boxes as one list of (face, pixel) items, 64 U
// items per round -- the texel indices and gradient operands of a round's items together.  No global atomics (agent-
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
// (us per launch below: the fused-MSE form on the 64-frame bird launch, by events; profiles/r06_atlas_grad_ab.txt)
constexpr int TEXG_FPW = 4;      // faces per wave: their box pixels form ONE list that the wave walks (4: 38.1 us; 8: 40.2; 2: 45)
constexpr int TEXG_U = 2;        // 64 U items of the list per round, all their loads in flight together (U = 1: 39.5 us, 2: 38.4, 3: 38.6, 4: 38.8, 8 -- spills -- 76)
constexpr int TEXG_WAVES = 8;    // waves per SIMD: a wave's load chain is hidden by occupancy, not by deeper unrolling
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
// element p (< H^2 <= 2^24) of a plane whose base is wave-uniform: a 32-bit byte offset, so that every load of a pixel
// shares one offset register (scalar base + vector offset addressing)
__device__ __forceinline__ float ld_plane(const char* base, unsigned p, int h16) {
  return h16 ? (float)*reinterpret_cast<const half_t*>(base + p * 2u) : *reinterpret_cast<const float*>(base + p * 4u);
}
enum { TEXG_GIVEN = 0, TEXG_MSE_F32 = 1, TEXG_MSE_F16 = 2 };   // the kernel's three forms: one instantiation each
struct TexGradN {            // the same for one mesh n: the planes' bases
  const char *g0, *g1, *g2;            // given gradient (float), or null
  const char *rm, *im0, *im1, *im2, *ri0, *ri1, *ri2;
  float w;
  // The operands of pixel p as loaded (fetch) and the gradient formed from them (grad): two steps, so that a wave
  // can request the operands of many pixels before it waits for the first.
  template <int MODE> struct Raw { float v[MODE == TEXG_GIVEN ? 3 : 7]; };   // rgb (image or given gradient); rgb of the reference, mask
  template <int MODE>
  __device__ __forceinline__ void fetch(unsigned p, Raw<MODE>& x) const {
    if (MODE == TEXG_GIVEN) { x.v[0] = ld_plane(g0, p, 0); x.v[1] = ld_plane(g1, p, 0); x.v[2] = ld_plane(g2, p, 0); return; }
    constexpr int h16 = MODE == TEXG_MSE_F16;
    x.v[0] = ld_plane(im0, p, h16); x.v[1] = ld_plane(im1, p, h16); x.v[2] = ld_plane(im2, p, h16);
    // (MODE ? k : 0: a constant index inside the given form's three floats, on lines that form never reaches)
    x.v[MODE ? 3 : 0] = ld_plane(ri0, p, h16); x.v[MODE ? 4 : 0] = ld_plane(ri1, p, h16); x.v[MODE ? 5 : 0] = ld_plane(ri2, p, h16);
    x.v[MODE ? 6 : 0] = ld_plane(rm, p, h16);
  }
  template <int MODE>
  __device__ __forceinline__ void grad(const Raw<MODE>& x, float& r, float& gg, float& b) const {
    if (MODE == TEXG_GIVEN) { r = x.v[0]; gg = x.v[1]; b = x.v[2]; return; }
    const float mk = x.v[MODE ? 6 : 0];
    r = w * (x.v[0] * mk - x.v[MODE ? 3 : 0] * mk) * mk;
    gg = w * (x.v[1] * mk - x.v[MODE ? 4 : 0] * mk) * mk;
    b = w * (x.v[2] * mk - x.v[MODE ? 5 : 0] * mk) * mk;
  }
};
__device__ __forceinline__ TexGradN tex_grad_of(const TexGrad& tg, int n, size_t HW, float gon) {   // gon = tg.go[n]
  TexGradN t = {};
  if (tg.grad_imgs) {
    t.g0 = reinterpret_cast<const char*>(tg.grad_imgs + (size_t)n * 3 * HW);
    t.g1 = t.g0 + 4 * HW; t.g2 = t.g1 + 4 * HW;
    return t;
  }
  const size_t rn = (size_t)(n % tg.rb), es = tg.h16 ? 2 : 4;
  t.rm = reinterpret_cast<const char*>(tg.tmask) + es * rn * HW;
  t.im0 = reinterpret_cast<const char*>(tg.imgs) + es * (size_t)n * 3 * HW;
  t.im1 = t.im0 + es * HW; t.im2 = t.im1 + es * HW;
  t.ri0 = reinterpret_cast<const char*>(tg.timg) + es * rn * 3 * HW;
  t.ri1 = t.ri0 + es * HW; t.ri2 = t.ri1 + es * HW;
  t.w = gon * 2.0f / (3.0f * (float)HW);
  return t;
}
// Dynamic LDS: [4 waves][FPW][3 R^2] floats (sized by the launch's R).  place: workgroup b belongs to XCD group b % 8
// and takes the atlases a % 8 == b % 8, whose texture outputs that XCD has just written (needs NA % 8 == 0); any
// mapping gives the same result.
template <int MODE>
__global__ __launch_bounds__(256, TEXG_WAVES) void k_tex_bwd_faces(RasterWs ws, TexGrad tgrad,
                                                       const int32_t* __restrict__ tidx, int N, int F, int H,
                                                       int R, int NA, int place, float box_shrink,
                                                       float* __restrict__ grad_atlas) {
  extern __shared__ float s_acc[];
  // (the wave's number through readfirstlane: everything derived from it -- atlas, faces, plane bases, box
  // parameters -- is then kept in scalar registers)
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // A wave takes the faces f0, f0 + Q, .., f0 + (FPW - 1) Q of one atlas (Q = ceil(F / FPW)): neighbouring faces
  // of a mesh tend to be large together, so they are dealt to different waves.
  const int Q = (F + TEXG_FPW - 1) / TEXG_FPW;
  int a, f0;
  if (place) {
    const long long wg = (long long)(blockIdx.x >> 3) * 4 + wv;
    if (wg >= (long long)(NA >> 3) * Q) return;              // (whole wave; no workgroup barriers below)
    a = (int)(blockIdx.x & 7) + 8 * (int)(wg / Q); f0 = (int)(wg % Q);
  } else {
    const long long wq = (long long)blockIdx.x * 4 + wv;
    if (wq >= (long long)NA * Q) return;
    a = (int)(wq / Q); f0 = (int)(wq % Q);
  }
  const int R2 = R * R, n3 = 3 * R2;
  float* acc = s_acc + wv * TEXG_FPW * n3;
  for (int i = lane; i < TEXG_FPW * n3; i += 64) acc[i] = 0.f;
  wave_lds_sync();
  const size_t HW = (size_t)H * H;
  const float hf = (float)H;
  // lane k < FPW looks after face f0 + k Q
  const int my_f = f0 + (lane < TEXG_FPW ? lane : 0) * Q;
  const bool my_live = lane < TEXG_FPW && my_f < F;
  const int base0 = (a * F + f0) * R2;                       // first texel index of face f0 (< 2^31: host check)
  const int G = N / NA;
  for (int g = 0; g < G; ++g) {
    // the FPW boxes (mesh a + g NA), one per lane, turned into pixel ranges (k_setup's formula, one pixel of slack)
    int xa = 0, ya = 0, w = 1, cnt = 0;
    const int n = a + g * NA;
    // Flag, box and (fused form) the mesh's loss gradient together: one round trip.  Lanes without a face read face
    // f0's, which exists.
    const size_t fi = (size_t)n * F + (my_live ? my_f : f0);
    int visi = ws.fvis[fi];
    float4 b = ws.rec[fi].box;
    float gon = MODE == TEXG_GIVEN ? 0.f : tgrad.go[n];
    asm volatile("" : "+v"(visi), "+v"(b.x), "+v"(b.y), "+v"(b.z), "+v"(b.w), "+v"(gon));   // (all issued before the first is waited for)
    if (!my_live) visi = 0;
    if (visi) {                                               // (a face no pixel shows has no gradient: zeros)
      b.x += box_shrink; b.y -= box_shrink; b.z += box_shrink; b.w -= box_shrink;
      if (b.x <= b.y && b.z <= b.w) {                        // not a degenerate face (inf, -inf, ..) or an emptied box
        // pixel range of the box: k_setup's formula with one pixel of slack, then tightened to the
        // pixels that pass the forward's own test (pixel centre inside the box, same float expressions)
        xa = (int)floorf(ndc_to_pix_held(b.y, hf)) - 1;
        int xb = (int)ceilf(ndc_to_pix_held(b.x, hf)) + 1;
        ya = (int)floorf(ndc_to_pix_held(b.w, hf)) - 1;
        int yb = (int)ceilf(ndc_to_pix_held(b.z, hf)) + 1;
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
    const char* tn = reinterpret_cast<const char*>(tidx + (size_t)n * HW);
    const TexGradN gn = tex_grad_of(tgrad, n, HW, gon);
    // One list of the wave's (face k, pixel i) items, faces in order and the pixels of a face in order: item j belongs
    // to the face k with pre[k] <= j < pre[k + 1].  Every texel so receives its addends in pixel order.
    int sp0[TEXG_FPW], sw[TEXG_FPW], pre[TEXG_FPW + 1];
    pre[0] = 0;
#pragma unroll
    for (int k = 0; k < TEXG_FPW; ++k) {
      sp0[k] = __builtin_amdgcn_readlane(ya, k) * H + __builtin_amdgcn_readlane(xa, k);   // first pixel of the box
      sw[k] = __builtin_amdgcn_readlane(w, k);
      pre[k + 1] = pre[k] + __builtin_amdgcn_readlane(cnt, k);
    }
    const int total = pre[TEXG_FPW];
    for (int j0 = 0; j0 < total; j0 += 64 * TEXG_U) {
      int tr[TEXG_U], kq[TEXG_U];
      TexGradN::Raw<MODE> raw[TEXG_U];
#pragma unroll
      for (int u = 0; u < TEXG_U; ++u) {
        const int j = j0 + 64 * u + lane;
        int kp0 = sp0[0], kw = sw[0], i = j;
        kq[u] = 0;
#pragma unroll
        for (int q = 1; q < TEXG_FPW; ++q) {
          const bool ge = j >= pre[q];
          kp0 = ge ? sp0[q] : kp0; kw = ge ? sw[q] : kw; i = ge ? j - pre[q] : i; kq[u] = ge ? q : kq[u];
        }
        int qy, qx;
        divmod_small(i, kw, __builtin_amdgcn_rcpf((float)kw), qy, qx);
        const unsigned p = (unsigned)(kp0 + qy * H + qx);
        tr[u] = -1;
        raw[u] = {};
        if (j < total) {      // texel index and gradient operands together, unconditionally: one round trip per round
          tr[u] = *reinterpret_cast<const int32_t*>(tn + p * 4u);
          gn.template fetch<MODE>(p, raw[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < TEXG_U; ++u) {
        const int t = tr[u] - (base0 + kq[u] * (Q * R2));    // texel of the item's own face?  (-1: no texel, or no item)
        if (t >= 0 && t < R2) {
          // d rgb / d texel = wnum / (wnum + delta) = 1 in fp32 (wnum >= 0.5, delta = 1e-10)
          float cr, cg, cb;
          gn.template grad<MODE>(raw[u], cr, cg, cb);
          float* o = acc + kq[u] * n3 + 3 * t;
          atomicAdd(o + 0, cr);
          atomicAdd(o + 1, cg);
          atomicAdd(o + 2, cb);
        }
      }
    }
  }
  wave_lds_sync();
#pragma unroll
  for (int k = 0; k < TEXG_FPW; ++k) {
    if (f0 + k * Q >= F) break;
    float* o = grad_atlas + (size_t)(a * F + f0 + k * Q) * n3;
    for (int i = lane; i < n3; i += 64) o[i] = acc[k * n3 + i];
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
  const size_t Q = (size_t)(F + TEXG_FPW - 1) / TEXG_FPW;
  const int place = atlas_batch % 8 == 0;    // per XCD group its own atlases, as the raster kernels deal meshes
  const size_t wgs = place ? 8 * (((size_t)(atlas_batch / 8) * Q + 3) / 4) : ((size_t)atlas_batch * Q + 3) / 4;
  const size_t lds = sizeof(float) * 4 * TEXG_FPW * 3 * (size_t)R * R;
  ProfScope ps(ACFM_PROF_TEX_BWD, st);
  const float shrink = ws_blur > 0.f ? sqrtf(ws_blur) * (1.0f - 1e-5f) : 0.f;
  auto kern = tgrad.grad_imgs ? k_tex_bwd_faces<TEXG_GIVEN> : tgrad.h16 ? k_tex_bwd_faces<TEXG_MSE_F16> : k_tex_bwd_faces<TEXG_MSE_F32>;
  hipLaunchKernelGGL(kern, dim3((unsigned)wgs), dim3(256), lds, st, ws, tgrad, texel_idx, N, F, H, R, atlas_batch,
                     place, shrink, grad_atlas);
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
