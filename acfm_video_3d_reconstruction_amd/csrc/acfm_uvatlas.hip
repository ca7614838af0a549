// The tail of TexturePredictorUV.forward (multiframe/nnutils/mesh_net.py:169-179) as gfx950 kernels: UV image
// [B,3,Hu,Wu] -> per-face atlas [B,Fp(+nsym),T,T,3] through the constant sampler of utils/mesh.py:206-232, and the
// gradient back to the UV image.
//   acfm_uv_atlas_forward    grid_sample (bilinear, zero padding, align_corners=True) + (tanh + 1) / 2 + the mirrored
//                            faces' copy, one thread per texel, the atlas written whole
//   acfm_uv_atlas_taps       the pixel each sample's four taps fall on (-1 = outside): what the host transposes, once
//                            per sampler, into per-pixel tap lists
//   acfm_uv_atlas_backward   a GATHER per UV pixel over its tap list: no float atomics, no zero fill, a fixed summation
//                            order -- the same bits on every run
// Taps and weights come from ONE device function (uv_taps) in all three, so the table and the forward cannot disagree
// about a sample that sits on an integer coordinate.
#include "acfm_common.h"

namespace acfm {

constexpr int UV_TPB = 256;

// ATen's grid_sampler_2d, bilinear, align_corners=True, padding_mode="zeros": x = ((u + 1) / 2) (Wu - 1), corners
// nw, ne, sw, se of floor(x), floor(y), weights the opposite areas.  pix = y Wu + x of a corner inside the image, -1
// outside (that corner contributes nothing).  The in-bounds test is made on the floats, so that a coordinate far
// outside (or not finite, which the contract excludes) is never converted to int.
struct UvAxis {
  float x, x0;    // the unnormalised coordinate and its floor
  int i0, i1;     // indices of the corner at floor(x) and of the one after it, -1 outside [0, size)
  // weight of the corner after floor(x) (hi) or at it: x - x0 or (x0 + 1) - x.  One subtraction of selected operands:
  // a select between the two differences was lowered through an indexed two-element array in LDS.
  __device__ __forceinline__ float w(bool hi) const { return (hi ? x : x0 + 1.0f) - (hi ? x0 : x); }
};
__device__ __forceinline__ UvAxis uv_axis(float c, int size) {
  UvAxis a;
  a.x = ((c + 1.0f) / 2.0f) * (float)(size - 1);
  a.x0 = floorf(a.x);
  const float x1 = a.x0 + 1.0f, xm = (float)(size - 1);
  a.i0 = a.x0 >= 0.0f && a.x0 <= xm ? (int)a.x0 : -1;
  a.i1 = x1 >= 0.0f && x1 <= xm ? (int)x1 : -1;
  return a;
}
struct UvTaps {
  UvAxis x, y;
  // corner k = 0..3 = nw, ne, sw, se
  __device__ __forceinline__ float w(int k) const { return x.w(k & 1) * y.w(k & 2); }
  __device__ __forceinline__ int pix(int k, int Wu) const {
    const int ix = (k & 1) ? x.i1 : x.i0, iy = (k & 2) ? y.i1 : y.i0;
    return ix >= 0 && iy >= 0 ? iy * Wu + ix : -1;
  }
};
__device__ __forceinline__ UvTaps uv_taps(float u, float v, int Hu, int Wu) {
  return UvTaps{uv_axis(u, Wu), uv_axis(v, Hu)};
}

// ---- forward ------------------------------------------------------------------------------------------------------
// One thread per texel (b, f', t), t fastest: a wave stores 768 contiguous bytes.  The 12 taps are gathers into three
// planes of at most a few hundred KB, which the L2 holds.
// The four products are added with fused multiply-adds, nw to se: that is how ATen's own HIP grid sampler is built
// (its `out_acc += value * weight` is contracted), so the pre-activation has the bits of the operator this replaces;
// everything else in this unit rounds every operation (acfm_common.h).
__global__ __launch_bounds__(UV_TPB) void k_uv_atlas_fwd(const float* __restrict__ uvimage,
                                                         const float* __restrict__ sampler, int B, int Hu, int Wu,
                                                         int Fp, int TT, int nsym, float* __restrict__ atlas) {
  const size_t per_b = (size_t)Fp * TT;
  const size_t i = (size_t)blockIdx.x * UV_TPB + threadIdx.x;
  if (i >= (size_t)B * per_b) return;
  const int b = (int)(i / per_b);
  const size_t s = i - (size_t)b * per_b;   // sample = f' TT + t
  const int f = (int)(s / TT);
  const UvTaps tp = uv_taps(sampler[2 * s], sampler[2 * s + 1], Hu, Wu);
  const size_t plane = (size_t)Hu * Wu;
  const float* __restrict__ img = uvimage + (size_t)b * 3 * plane;
  const int px[4] = {tp.pix(0, Wu), tp.pix(1, Wu), tp.pix(2, Wu), tp.pix(3, Wu)};   // (unrolled below: registers)
  const float wt[4] = {tp.w(0), tp.w(1), tp.w(2), tp.w(3)};
  float o[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (px[k] >= 0) acc = __builtin_fmaf(img[c * plane + px[k]], wt[k], acc);
    o[c] = (tanhf(acc) + 1.0f) / 2.0f;
  }
  const size_t Ft = (size_t)Fp + nsym;
  float* __restrict__ d = atlas + (((size_t)b * Ft) * TT + s) * 3;
  d[0] = o[0]; d[1] = o[1]; d[2] = o[2];
  if (f >= Fp - nsym) {   // tex_pred[:, -nsym:] once more behind the Fp faces
    float* __restrict__ m = d + (size_t)nsym * TT * 3;   // face Fp + (f - (Fp - nsym)) = f + nsym
    m[0] = o[0]; m[1] = o[1]; m[2] = o[2];
  }
}

__global__ __launch_bounds__(UV_TPB) void k_uv_atlas_taps(const float* __restrict__ sampler, int n_samples, int Hu,
                                                          int Wu, int4* __restrict__ tap_pixel) {
  const int s = blockIdx.x * UV_TPB + threadIdx.x;
  if (s >= n_samples) return;
  const UvTaps tp = uv_taps(sampler[2 * (size_t)s], sampler[2 * (size_t)s + 1], Hu, Wu);
  tap_pixel[s] = make_int4(tp.pix(0, Wu), tp.pix(1, Wu), tp.pix(2, Wu), tp.pix(3, Wu));
}

// ---- backward -----------------------------------------------------------------------------------------------------
// d atlas[b,f',t,c] / d pre-activation = 2 y (1 - y) with y the saved atlas value ((tanh + 1) / 2 differentiated); a
// mirrored face's gradient reaches the image through its source face's taps.
struct UvBwd {
  const float* grad_atlas; const float* atlas; const float* sampler;
  const int* pix_start; const int* pix_taps;
  int n_entries, n_samples, Hu, Wu, Fp, TT, nsym;
};
__device__ __forceinline__ void uv_bwd_term(const UvBwd& a, size_t batch_off, int e, float acc[3]) {
  const unsigned ent = (unsigned)a.pix_taps[e];
  if (ent >= 4u * (unsigned)a.n_samples) return;   // (a table of this library never holds one)
  const int s = (int)(ent >> 2), k = (int)(ent & 3u);
  const UvTaps tp = uv_taps(a.sampler[2 * (size_t)s], a.sampler[2 * (size_t)s + 1], a.Hu, a.Wu);
  const float w = tp.w(k);
  const size_t o = (batch_off + s) * 3;
  const int f = s / a.TT;
  float g[3] = {a.grad_atlas[o], a.grad_atlas[o + 1], a.grad_atlas[o + 2]};
  if (f >= a.Fp - a.nsym) {
    const size_t m = o + (size_t)a.nsym * a.TT * 3;
    g[0] += a.grad_atlas[m]; g[1] += a.grad_atlas[m + 1]; g[2] += a.grad_atlas[m + 2];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float y = a.atlas[o + c];
    acc[c] += (w * (2.0f * y * (1.0f - y))) * g[c];
  }
}

// One lane per (b, pixel), pixel fastest, so the three stores of a wave are 256 contiguous bytes each.  The real
// samplers give a pixel 0 to 30 taps (mean 3): a lane walks such a list alone, in list order.  A list longer than
// UV_SERIAL (samplers that pile samples up on a pixel) is walked by the whole wave instead -- lane l takes entries
// l, l + 64, ... in order and the 64 partial sums meet in the xor butterfly of wave_sum -- so a wave never waits for
// one lane's thousands of entries, and no list length is too long.  Both orders are fixed: the same bits every run.
constexpr int UV_SERIAL = 32;

__global__ __launch_bounds__(UV_TPB) void k_uv_atlas_bwd(UvBwd a, int B, float* __restrict__ grad_uvimage) {
  const size_t plane = (size_t)a.Hu * a.Wu;
  const size_t i = (size_t)blockIdx.x * UV_TPB + threadIdx.x;
  const bool live = i < (size_t)B * plane;
  const int b = live ? (int)(i / plane) : 0;
  const int p = live ? (int)(i - (size_t)b * plane) : 0;
  int e0 = 0, e1 = 0;
  if (live) {
    e0 = max(a.pix_start[p], 0);
    e1 = min(a.pix_start[p + 1], a.n_entries);
  }
  const size_t Ft = (size_t)a.Fp + a.nsym;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  const bool wide = e1 - e0 > UV_SERIAL;
  if (!wide)
    for (int e = e0; e < e1; ++e) uv_bwd_term(a, (size_t)b * Ft * a.TT, e, acc);
  unsigned long long todo = __ballot(wide);   // (the same in every lane: the loop below is wave-uniform)
  const int lane = threadIdx.x & (ACFM_WAVE - 1);
  while (todo) {
    const int src = __builtin_ctzll(todo);
    todo &= todo - 1;
    const int wb = __shfl(b, src, ACFM_WAVE), w0 = __shfl(e0, src, ACFM_WAVE), w1 = __shfl(e1, src, ACFM_WAVE);
    float part[3] = {0.0f, 0.0f, 0.0f};
    for (int e = w0 + lane; e < w1; e += ACFM_WAVE) uv_bwd_term(a, (size_t)wb * Ft * a.TT, e, part);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float sum = wave_sum(part[c]);
      if (lane == src) acc[c] = sum;
    }
  }
  if (live) {
    float* __restrict__ d = grad_uvimage + (size_t)b * 3 * plane + p;
    d[0] = acc[0]; d[plane] = acc[1]; d[2 * plane] = acc[2];
  }
}

static bool uv_shape_ok(int B, int Hu, int Wu, int Fp, int T, int nsym) {
  if (B < 1 || Hu < 2 || Wu < 2 || Fp < 1 || T < 1 || nsym < 0 || nsym > Fp) return false;
  if ((size_t)Hu * Wu > (size_t)1 << 30) return false;                      // pixel indices and the table in int32
  if ((size_t)Fp * T * T > (size_t)1 << 28) return false;                   // sample * 4 + corner in int32
  if ((size_t)B * Fp * T * T > (size_t)1 << 38 || (size_t)B * Hu * Wu > (size_t)1 << 38) return false;   // grid.x
  return true;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_uv_atlas_forward(const float* uvimage, const float* sampler, int B, int Hu, int Wu, int Fp, int T, int nsym,
                          float* atlas, void* stream) {
  if (!uvimage || !sampler || !atlas || !uv_shape_ok(B, Hu, Wu, Fp, T, nsym)) return ACFM_E_BADARG;
  const size_t n = (size_t)B * Fp * T * T;
  hipLaunchKernelGGL(k_uv_atlas_fwd, dim3((unsigned)((n + UV_TPB - 1) / UV_TPB)), dim3(UV_TPB), 0, (hipStream_t)stream,
                     uvimage, sampler, B, Hu, Wu, Fp, T * T, nsym, atlas);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_uv_atlas_taps(const float* sampler, int n_samples, int Hu, int Wu, int32_t* tap_pixel, void* stream) {
  if (!sampler || !tap_pixel || n_samples < 1 || n_samples > (1 << 28) || !uv_shape_ok(1, Hu, Wu, 1, 1, 0))
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_uv_atlas_taps, dim3((n_samples + UV_TPB - 1) / UV_TPB), dim3(UV_TPB), 0, (hipStream_t)stream,
                     sampler, n_samples, Hu, Wu, (int4*)tap_pixel);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_uv_atlas_backward(const float* grad_atlas, const float* atlas, const float* sampler, const int32_t* pix_start,
                           const int32_t* pix_taps, int n_entries, int B, int Hu, int Wu, int Fp, int T, int nsym,
                           float* grad_uvimage, void* stream) {
  if (!grad_atlas || !atlas || !sampler || !pix_start || !grad_uvimage || !uv_shape_ok(B, Hu, Wu, Fp, T, nsym))
    return ACFM_E_BADARG;
  if (n_entries < 0 || (size_t)n_entries > (size_t)4 * Fp * T * T || (n_entries > 0 && !pix_taps)) return ACFM_E_BADARG;
  UvBwd a{grad_atlas, atlas, sampler, pix_start, pix_taps, n_entries, Fp * T * T, Hu, Wu, Fp, T * T, nsym};
  const size_t n = (size_t)B * Hu * Wu;
  hipLaunchKernelGGL(k_uv_atlas_bwd, dim3((unsigned)((n + UV_TPB - 1) / UV_TPB)), dim3(UV_TPB), 0, (hipStream_t)stream,
                     a, B, grad_uvimage);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
