// The tail of the LPIPS texture term (multiframe/nnutils/loss_utils.py:359-383 around lpips.LPIPS(net='alex',
// lpips=False, spatial=True)) as gfx950 kernels; the AlexNet convolutions between them stay with torch.
//   acfm_lpips_input_*        mask multiply, 2x - 1 and the scaling layer in one pass over the image
//   acfm_lpips_layer_*        per pixel of a feature layer: unit-normalise both channel vectors, d = sum_c w_c (u_c - v_c)^2
//   acfm_lpips_mask_weights   M_l = U_l^T (mask / (H W)) for every layer: the adjoint of the bilinear upsampling applied
//                             to the ground-truth mask, so that mean(mask sum_l upsample(d_l)) = sum_l sum_p d_l[p] M_l[p]
//                             and neither the upsampled maps nor their sum are ever formed
//   acfm_lpips_masked_mean_*  loss[n] = sum_p d[n,p] M[n mod Nr,p]
// References (features of the image, mask, M) may be given once per frame: prediction n reads reference n mod Nr.
// No float atomics, no zero fills, fixed summation orders: the same inputs give the same bits.
#include "acfm_common.h"

namespace acfm {

constexpr int LP_TPB = 256;
constexpr int LP_WAVES = LP_TPB / ACFM_WAVE;
constexpr int LP_MAX_LAYERS = 8;
#define ACFM_LPIPS_EPS 1e-10f   // lpips.normalize_tensor

// ---- input ----------------------------------------------------------------------------------------------------------
// x = ((2 (img m) - 1) - shift_c) / scale_c, the operations of loss_utils.py:370-375 and lpips's ScalingLayer one by
// one (the same bits as that chain).  img is not read where m == 0 (img m = 0 for every finite img).
__device__ __forceinline__ float lp_shift(int c) { return c == 0 ? -0.030f : c == 1 ? -0.088f : -0.188f; }
__device__ __forceinline__ float lp_scale(int c) { return c == 0 ? 0.458f : c == 1 ? 0.448f : 0.450f; }

template <int V>   // V = 4: HW is a multiple of 4 and every plane starts 16-byte aligned
__global__ __launch_bounds__(LP_TPB) void k_lpips_input_fwd(const float* __restrict__ img, const float* __restrict__ mask,
                                                            int N, int Nr, int HW, float* __restrict__ x) {
  const size_t per = (size_t)(HW / V);
  const size_t i = (size_t)blockIdx.x * LP_TPB + threadIdx.x;
  if (i >= (size_t)N * 3 * per) return;
  const size_t nc = i / per;
  const int n = (int)(nc / 3), c = (int)(nc - (size_t)n * 3);
  const size_t p = (i - nc * per) * V;
  const float* __restrict__ m = mask + (size_t)(n % Nr) * HW + p;
  const size_t o = nc * (size_t)HW + p;
  const float sh = lp_shift(c), sc = lp_scale(c);
  float mv[V], iv[V], ov[V];
  if (V == 4) *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m);
  else mv[0] = m[0];
  bool any = false;
#pragma unroll
  for (int k = 0; k < V; ++k) any |= mv[k] != 0.0f;
#pragma unroll
  for (int k = 0; k < V; ++k) iv[k] = 0.0f;
  if (any) {
    if (V == 4) *reinterpret_cast<float4*>(iv) = *reinterpret_cast<const float4*>(img + o);
    else iv[0] = img[o];
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const float t = mv[k] != 0.0f ? iv[k] * mv[k] : 0.0f;
    ov[k] = ((2.0f * t - 1.0f) - sh) / sc;
  }
  if (V == 4) *reinterpret_cast<float4*>(x + o) = *reinterpret_cast<const float4*>(ov);
  else x[o] = ov[0];
}

// g_img = ((g_x / scale_c) 2) m, autograd's order through the same chain; g_x is not read where m == 0.
template <int V>
__global__ __launch_bounds__(LP_TPB) void k_lpips_input_bwd(const float* __restrict__ gx, const float* __restrict__ mask,
                                                            int N, int Nr, int HW, float* __restrict__ gimg) {
  const size_t per = (size_t)(HW / V);
  const size_t i = (size_t)blockIdx.x * LP_TPB + threadIdx.x;
  if (i >= (size_t)N * 3 * per) return;
  const size_t nc = i / per;
  const int n = (int)(nc / 3), c = (int)(nc - (size_t)n * 3);
  const size_t p = (i - nc * per) * V;
  const float* __restrict__ m = mask + (size_t)(n % Nr) * HW + p;
  const size_t o = nc * (size_t)HW + p;
  const float sc = lp_scale(c);
  float mv[V], gv[V], ov[V];
  if (V == 4) *reinterpret_cast<float4*>(mv) = *reinterpret_cast<const float4*>(m);
  else mv[0] = m[0];
  bool any = false;
#pragma unroll
  for (int k = 0; k < V; ++k) any |= mv[k] != 0.0f;
#pragma unroll
  for (int k = 0; k < V; ++k) gv[k] = 0.0f;
  if (any) {
    if (V == 4) *reinterpret_cast<float4*>(gv) = *reinterpret_cast<const float4*>(gx + o);
    else gv[0] = gx[o];
  }
#pragma unroll
  for (int k = 0; k < V; ++k) ov[k] = mv[k] != 0.0f ? ((gv[k] / sc) * 2.0f) * mv[k] : 0.0f;
  if (V == 4) *reinterpret_cast<float4*>(gimg + o) = *reinterpret_cast<const float4*>(ov);
  else gimg[o] = ov[0];
}

// ---- layer distance -------------------------------------------------------------------------------------------------
// Lanes run along the pixels of the whole batch (pixel g = n hw + p: contiguous in NCHW inside an image, so a wave's
// load of one channel is one 256-byte run, or a few where it crosses images); the channels are dealt to the WAVES waves
// of the workgroup (wave w takes c = w, w + WAVES, ...) and the per-wave sums meet in LDS, added in wave order.
// WAVES = 4 where the layer has pixels enough to fill the machine (N hw / 64 >= LP_WIDE_BELOW tiles), else 16: a
// 15 x 15 layer of 384 channels of 96 images has 338 tiles, and with four waves each every wave walked 96 channels, a
// chain of 24 dependent rounds of loads, with hardly more than one wave per SIMD to hide it (measured: 58 us for 33 MB).
// The direct form: norms first, then the weighted squared difference of the normalised values (the expanded form
// cancels when u ~ v).  The second (and, backward, third) read of the 64-pixel tile comes from cache.
struct LpPix {
  bool live;
  size_t a0, b0;   // offsets of channel 0 of the pixel in fa / fb
  int n, p;
};
__device__ __forceinline__ LpPix lp_pixel(int N, int Nr, int C, int hw) {
  LpPix q;
  const size_t g = (size_t)blockIdx.x * ACFM_WAVE + (threadIdx.x & (ACFM_WAVE - 1));
  q.live = g < (size_t)N * hw;
  q.n = q.live ? (int)(g / hw) : 0;
  q.p = q.live ? (int)(g - (size_t)q.n * hw) : 0;
  q.a0 = (size_t)q.n * C * hw + q.p;
  q.b0 = (size_t)(q.n % Nr) * C * hw + q.p;
  return q;
}
// sum over the waves of the workgroup of K values per lane, in wave order; every thread gets the sums
template <int WAVES, int K>
__device__ __forceinline__ void lp_combine(float (*red)[K][ACFM_WAVE], float v[K]) {
  const int w = threadIdx.x / ACFM_WAVE, lane = threadIdx.x & (ACFM_WAVE - 1);
  __syncthreads();   // (the previous round's reads are over)
#pragma unroll
  for (int k = 0; k < K; ++k) red[w][k][lane] = v[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = red[0][k][lane];
#pragma unroll
    for (int j = 1; j < WAVES; ++j) s += red[j][k][lane];
    v[k] = s;
  }
}

// this wave's share of sum_c a_c^2 and sum_c b_c^2: four running sums each (channel c = w + WAVES j goes to sum j mod 4),
// added pairwise at the end -- four independent chains for the loads to overlap, and shorter chains to round
constexpr int LP_ACC = 4;
#ifndef ACFM_LPIPS_WIDE_BELOW   // (a VARIANT build of the Makefile may set it, to time one form against the other)
#define ACFM_LPIPS_WIDE_BELOW 2048
#endif
constexpr int LP_WIDE_BELOW = ACFM_LPIPS_WIDE_BELOW;   // fewer 64-pixel tiles than this: 16 waves per tile instead of 4
template <int WAVES>
__device__ __forceinline__ void lp_norms(const float* __restrict__ fa, const float* __restrict__ fb, const LpPix& q, int w,
                                         int C, int hw, float s[2]) {
  float sa[LP_ACC] = {0.0f, 0.0f, 0.0f, 0.0f}, sb[LP_ACC] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.live) {
    for (int c0 = w; c0 < C; c0 += WAVES * LP_ACC) {
#pragma unroll
      for (int k = 0; k < LP_ACC; ++k) {
        const int c = c0 + k * WAVES;
        if (c < C) {   // (the same in every lane)
          const float a = fa[q.a0 + (size_t)c * hw], b = fb[q.b0 + (size_t)c * hw];
          sa[k] += a * a;
          sb[k] += b * b;
        }
      }
    }
  }
  s[0] = (sa[0] + sa[1]) + (sa[2] + sa[3]);
  s[1] = (sb[0] + sb[1]) + (sb[2] + sb[3]);
}

template <int WAVES>
__global__ __launch_bounds__(WAVES * ACFM_WAVE) void k_lpips_layer_fwd(const float* __restrict__ fa,
                                                                       const float* __restrict__ fb,
                                                                       const float* __restrict__ lin, int N, int Nr, int C,
                                                                       int hw, float* __restrict__ d, size_t d_stride) {
  __shared__ float red[WAVES][2][ACFM_WAVE];
  __shared__ float red1[WAVES][1][ACFM_WAVE];
  const LpPix q = lp_pixel(N, Nr, C, hw);
  const int w = threadIdx.x / ACFM_WAVE;
  float s[2];
  lp_norms<WAVES>(fa, fb, q, w, C, hw, s);
  lp_combine<WAVES, 2>(red, s);
  const float da = sqrtf(s[0]) + ACFM_LPIPS_EPS, db = sqrtf(s[1]) + ACFM_LPIPS_EPS;
  float t4[LP_ACC] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.live) {
    for (int c0 = w; c0 < C; c0 += WAVES * LP_ACC) {
#pragma unroll
      for (int k = 0; k < LP_ACC; ++k) {
        const int c = c0 + k * WAVES;
        if (c < C) {   // (the same in every lane)
          const float a = fa[q.a0 + (size_t)c * hw], b = fb[q.b0 + (size_t)c * hw];
          const float df = a / da - b / db;
          t4[k] += lin ? lin[c] * (df * df) : df * df;
        }
      }
    }
  }
  float t[1] = {(t4[0] + t4[1]) + (t4[2] + t4[3])};
  lp_combine<WAVES, 1>(red1, t);
  if (q.live && w == 0) d[(size_t)q.n * d_stride + q.p] = t[0];
}

// g_a_c = q_c / (n_a + eps) - a_c (sum_k q_k a_k) / (n_a (n_a + eps)^2), q_c = 2 w_c (u_c - v_c) g; the second term is
// dropped where n_a = 0 (u = 0 there by definition: lpips's autograd has 0/0 at such a pixel).  Every element of g_fa is
// written by the one workgroup that owns its pixel.
template <int WAVES>
__global__ __launch_bounds__(WAVES * ACFM_WAVE) void k_lpips_layer_bwd(const float* __restrict__ fa,
                                                                       const float* __restrict__ fb,
                                                                       const float* __restrict__ lin,
                                                                       const float* __restrict__ gd, size_t gd_stride, int N,
                                                                       int Nr, int C, int hw, float* __restrict__ gfa) {
  __shared__ float red[WAVES][2][ACFM_WAVE];
  __shared__ float red1[WAVES][1][ACFM_WAVE];
  const LpPix q = lp_pixel(N, Nr, C, hw);
  const int w = threadIdx.x / ACFM_WAVE;
  float s[2];
  lp_norms<WAVES>(fa, fb, q, w, C, hw, s);
  lp_combine<WAVES, 2>(red, s);
  const float na = sqrtf(s[0]);
  const float da = na + ACFM_LPIPS_EPS, db = sqrtf(s[1]) + ACFM_LPIPS_EPS;
  const float g2 = q.live ? 2.0f * gd[(size_t)q.n * gd_stride + q.p] : 0.0f;
  float t4[LP_ACC] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (q.live) {
    for (int c0 = w; c0 < C; c0 += WAVES * LP_ACC) {
#pragma unroll
      for (int k = 0; k < LP_ACC; ++k) {
        const int c = c0 + k * WAVES;
        if (c < C) {
          const float a = fa[q.a0 + (size_t)c * hw], b = fb[q.b0 + (size_t)c * hw];
          const float df = a / da - b / db;
          const float qc = lin ? (lin[c] * df) * g2 : df * g2;
          t4[k] += qc * a;
        }
      }
    }
  }
  float t[1] = {(t4[0] + t4[1]) + (t4[2] + t4[3])};
  lp_combine<WAVES, 1>(red1, t);
  const float k2 = na > 0.0f ? t[0] / (na * (da * da)) : 0.0f;
  if (q.live) {
#pragma unroll 4
    for (int c = w; c < C; c += WAVES) {
      const float a = fa[q.a0 + (size_t)c * hw], b = fb[q.b0 + (size_t)c * hw];
      const float df = a / da - b / db;
      const float qc = lin ? (lin[c] * df) * g2 : df * g2;
      gfa[q.a0 + (size_t)c * hw] = qc / da - a * k2;
    }
  }
}

// ---- mask weights ---------------------------------------------------------------------------------------------------
// PyTorch's upsample_bilinear2d, align_corners=False, along one axis: destination i of `out` reads sources i0 and i1
// with weights 1 - l and l (area_pixel_compute_source_index: scale = in / out in float, source (i + 0.5) scale - 0.5
// clamped below at 0; the second tap clamped at in - 1).  lp_axis_weight is the weight destination i gives source s.
__device__ __forceinline__ float lp_axis_weight(int i, int s, int in, float scale) {
  float src = scale * ((float)i + 0.5f) - 0.5f;
  src = src < 0.0f ? 0.0f : src;
  int i0 = (int)src;
  i0 = i0 > in - 1 ? in - 1 : i0;
  const int i1 = i0 + (i0 < in - 1 ? 1 : 0);
  const float l1 = src - (float)i0, l0 = 1.0f - l1;
  return (i0 == s ? l0 : 0.0f) + (i1 == s ? l1 : 0.0f);
}
// destinations that can read source s: |source index - s| < 1 before the clamps, widened by one each way; the clamps
// only move taps onto sources 0 and in - 1, whose ranges reach the image's edge
__device__ __forceinline__ void lp_axis_range(int s, int in, int out, int& lo, int& hi) {
  const float inv = (float)out / (float)in;
  lo = s == 0 ? 0 : max(0, (int)floorf(((float)s - 0.5f) * inv - 0.5f) - 1);
  hi = s == in - 1 ? out - 1 : min(out - 1, (int)ceilf(((float)s + 1.5f) * inv - 0.5f) + 1);
}

struct LpLayers {
  int L, P;
  int h[LP_MAX_LAYERS], w[LP_MAX_LAYERS], off[LP_MAX_LAYERS];
};

// One wave per low-resolution pixel (r, layer, y, x): a gather over the mask pixels whose upsampling taps reach it.
// Lane l owns the columns X = x_lo + l, x_lo + l + 64, ...: it adds its columns' rows from top to bottom, then the 64
// lane sums meet in the xor butterfly -- a fixed order.
__global__ __launch_bounds__(ACFM_WAVE) void k_lpips_mask_weights(const float* __restrict__ mask, LpLayers ly, int H,
                                                                  int W, float* __restrict__ M) {
  const int r = blockIdx.y;
  const int o = blockIdx.x;   // < P
  int l = 0;
#pragma unroll
  for (int k = 1; k < LP_MAX_LAYERS; ++k)
    if (k < ly.L && o >= ly.off[k]) l = k;
  const int h = ly.h[l], w = ly.w[l];
  const int pp = o - ly.off[l];
  const int sy = pp / w, sx = pp - sy * w;
  const float scy = (float)h / (float)H, scx = (float)w / (float)W;
  int ylo, yhi, xlo, xhi;
  lp_axis_range(sy, h, H, ylo, yhi);
  lp_axis_range(sx, w, W, xlo, xhi);
  const float* __restrict__ m = mask + (size_t)r * H * W;
  float acc = 0.0f;
  for (int X = xlo + (int)threadIdx.x; X <= xhi; X += ACFM_WAVE) {
    const float wx = lp_axis_weight(X, sx, w, scx);
    if (wx == 0.0f) continue;
    float col = 0.0f;
    for (int Y = ylo; Y <= yhi; ++Y) col += lp_axis_weight(Y, sy, h, scy) * m[(size_t)Y * W + X];
    acc += wx * col;
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) M[(size_t)r * ly.P + o] = acc / ((float)H * (float)W);
}

// ---- masked mean ----------------------------------------------------------------------------------------------------
// One workgroup per prediction: thread t adds p = t, t + 256, ... in order, the wave butterfly, then the four waves in
// order.  The output is written, not accumulated: it needs no prior contents.
__global__ __launch_bounds__(LP_TPB) void k_lpips_masked_mean_fwd(const float* __restrict__ d, const float* __restrict__ M,
                                                                  int Nr, int P, float* __restrict__ loss) {
  __shared__ float red[LP_WAVES];
  const int n = blockIdx.x;
  const float* __restrict__ dr = d + (size_t)n * P;
  const float* __restrict__ mr = M + (size_t)(n % Nr) * P;
  float acc = 0.0f;
  for (int p = threadIdx.x; p < P; p += LP_TPB) acc += dr[p] * mr[p];
  acc = wave_sum(acc);
  if ((threadIdx.x & (ACFM_WAVE - 1)) == 0) red[threadIdx.x / ACFM_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = red[0];
#pragma unroll
    for (int j = 1; j < LP_WAVES; ++j) s += red[j];
    loss[n] = s;
  }
}

__global__ __launch_bounds__(LP_TPB) void k_lpips_masked_mean_bwd(const float* __restrict__ g, const float* __restrict__ M,
                                                                  int N, int Nr, int P, float* __restrict__ gd) {
  const size_t i = (size_t)blockIdx.x * LP_TPB + threadIdx.x;
  if (i >= (size_t)N * P) return;
  const int n = (int)(i / P);
  const int p = (int)(i - (size_t)n * P);
  gd[i] = g[n] * M[(size_t)(n % Nr) * P + p];
}

static bool lp_batch_ok(int N, int Nr) { return N >= 1 && Nr >= 1 && N % Nr == 0; }
static unsigned lp_blocks(size_t n, int per) { return (unsigned)((n + per - 1) / per); }

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_lpips_input_forward(const float* img, const float* mask, int N, int Nr, int H, int W, float* x, void* stream) {
  if (!img || !mask || !x || !lp_batch_ok(N, Nr) || H < 1 || W < 1 || (size_t)H * W > (size_t)1 << 30) return ACFM_E_BADARG;
  const int HW = H * W;
  if ((size_t)N * 3 * HW > (size_t)1 << 38) return ACFM_E_BADARG;   // grid.x
  const bool v4 = HW % 4 == 0 && (((uintptr_t)img | (uintptr_t)mask | (uintptr_t)x) & 15) == 0;
  const size_t n = (size_t)N * 3 * (v4 ? HW / 4 : HW);
  if (v4)
    hipLaunchKernelGGL(k_lpips_input_fwd<4>, dim3(lp_blocks(n, LP_TPB)), dim3(LP_TPB), 0, (hipStream_t)stream, img, mask,
                       N, Nr, HW, x);
  else
    hipLaunchKernelGGL(k_lpips_input_fwd<1>, dim3(lp_blocks(n, LP_TPB)), dim3(LP_TPB), 0, (hipStream_t)stream, img, mask,
                       N, Nr, HW, x);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_lpips_input_backward(const float* grad_x, const float* mask, int N, int Nr, int H, int W, float* grad_img,
                              void* stream) {
  if (!grad_x || !mask || !grad_img || !lp_batch_ok(N, Nr) || H < 1 || W < 1 || (size_t)H * W > (size_t)1 << 30)
    return ACFM_E_BADARG;
  const int HW = H * W;
  if ((size_t)N * 3 * HW > (size_t)1 << 38) return ACFM_E_BADARG;
  const bool v4 = HW % 4 == 0 && (((uintptr_t)grad_x | (uintptr_t)mask | (uintptr_t)grad_img) & 15) == 0;
  const size_t n = (size_t)N * 3 * (v4 ? HW / 4 : HW);
  if (v4)
    hipLaunchKernelGGL(k_lpips_input_bwd<4>, dim3(lp_blocks(n, LP_TPB)), dim3(LP_TPB), 0, (hipStream_t)stream, grad_x,
                       mask, N, Nr, HW, grad_img);
  else
    hipLaunchKernelGGL(k_lpips_input_bwd<1>, dim3(lp_blocks(n, LP_TPB)), dim3(LP_TPB), 0, (hipStream_t)stream, grad_x,
                       mask, N, Nr, HW, grad_img);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

static bool lp_layer_ok(int N, int Nr, int C, int hw, size_t stride) {
  if (!lp_batch_ok(N, Nr) || C < 1 || hw < 1 || stride < (size_t)hw) return false;
  if ((size_t)C * hw > (size_t)1 << 31) return false;
  return (size_t)N * hw <= (size_t)1 << 36;   // grid.x = N hw / 64
}

int acfm_lpips_layer_forward(const float* fa, const float* fb, const float* lin, int N, int Nr, int C, int hw, float* d,
                             size_t d_row_stride, void* stream) {
  if (!fa || !fb || !d || !lp_layer_ok(N, Nr, C, hw, d_row_stride)) return ACFM_E_BADARG;
  const unsigned tiles = lp_blocks((size_t)N * hw, ACFM_WAVE);
  if (tiles < (unsigned)LP_WIDE_BELOW)
    hipLaunchKernelGGL(k_lpips_layer_fwd<16>, dim3(tiles), dim3(16 * ACFM_WAVE), 0, (hipStream_t)stream, fa, fb, lin, N,
                       Nr, C, hw, d, d_row_stride);
  else
    hipLaunchKernelGGL(k_lpips_layer_fwd<4>, dim3(tiles), dim3(4 * ACFM_WAVE), 0, (hipStream_t)stream, fa, fb, lin, N, Nr,
                       C, hw, d, d_row_stride);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_lpips_layer_backward(const float* fa, const float* fb, const float* lin, const float* grad_d,
                              size_t grad_d_row_stride, int N, int Nr, int C, int hw, float* grad_fa, void* stream) {
  if (!fa || !fb || !grad_d || !grad_fa || !lp_layer_ok(N, Nr, C, hw, grad_d_row_stride)) return ACFM_E_BADARG;
  const unsigned tiles = lp_blocks((size_t)N * hw, ACFM_WAVE);
  if (tiles < (unsigned)LP_WIDE_BELOW)
    hipLaunchKernelGGL(k_lpips_layer_bwd<16>, dim3(tiles), dim3(16 * ACFM_WAVE), 0, (hipStream_t)stream, fa, fb, lin,
                       grad_d, grad_d_row_stride, N, Nr, C, hw, grad_fa);
  else
    hipLaunchKernelGGL(k_lpips_layer_bwd<4>, dim3(tiles), dim3(4 * ACFM_WAVE), 0, (hipStream_t)stream, fa, fb, lin,
                       grad_d, grad_d_row_stride, N, Nr, C, hw, grad_fa);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_lpips_mask_weights(const float* mask, int Nr, int H, int W, const int32_t* layer_hw, int n_layers, float* M,
                            void* stream) {
  if (!mask || !layer_hw || !M || Nr < 1 || Nr > 65535 || H < 1 || W < 1 || (size_t)H * W > (size_t)1 << 24 ||
      n_layers < 1 || n_layers > LP_MAX_LAYERS)
    return ACFM_E_BADARG;
  LpLayers ly;
  size_t P = 0;
  for (int l = 0; l < LP_MAX_LAYERS; ++l) {
    const bool on = l < n_layers;
    ly.h[l] = on ? layer_hw[2 * l] : 1;
    ly.w[l] = on ? layer_hw[2 * l + 1] : 1;
    ly.off[l] = (int)P;
    if (on) {
      if (ly.h[l] < 1 || ly.w[l] < 1 || ly.h[l] > (1 << 12) || ly.w[l] > (1 << 12)) return ACFM_E_BADARG;
      P += (size_t)ly.h[l] * ly.w[l];
    }
  }
  if (P > (size_t)1 << 27) return ACFM_E_BADARG;
  ly.L = n_layers;
  ly.P = (int)P;
  hipLaunchKernelGGL(k_lpips_mask_weights, dim3((unsigned)P, (unsigned)Nr), dim3(ACFM_WAVE), 0, (hipStream_t)stream, mask,
                     ly, H, W, M);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_lpips_masked_mean_forward(const float* d, const float* M, int N, int Nr, int P, float* loss, void* stream) {
  if (!d || !M || !loss || !lp_batch_ok(N, Nr) || P < 1) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_lpips_masked_mean_fwd, dim3((unsigned)N), dim3(LP_TPB), 0, (hipStream_t)stream, d, M, Nr, P, loss);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_lpips_masked_mean_backward(const float* grad_loss, const float* M, int N, int Nr, int P, float* grad_d,
                                    void* stream) {
  if (!grad_loss || !M || !grad_d || !lp_batch_ok(N, Nr) || P < 1 || (size_t)N * P > (size_t)1 << 38) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_lpips_masked_mean_bwd, dim3(lp_blocks((size_t)N * P, LP_TPB)), dim3(LP_TPB), 0,
                     (hipStream_t)stream, grad_loss, M, N, Nr, P, grad_d);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
