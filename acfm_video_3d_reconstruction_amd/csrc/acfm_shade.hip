// The shading half of PyTorch3D 0.3.0's mesh renderer over Fragments:
// sigmoid_alpha_blend, softmax_rgb_blend (dense colours, or a TexturesAtlas sampled in the kernel) and
// interpolate_face_attributes, forward and backward.  P = N H W pixels, K slots per pixel in the Fragments layout
// (pix_to_face [P,K] i64 packed n F + f, -1 empty; dists / zbuf [P,K]; bary [P,K,3]).
//
// Blends: one wave per 64 pixels, one lane per pixel.  The [64,K] planes of the wave (ids, dists, zbuf) are staged
// through LDS with coalesced loads (a lane's own K values are K x 4 bytes apart in memory: read per lane they would
// touch 64 lines per load instruction); rows are padded to K + 1 words so that lane l reading word l (K + 1) + k is
// free of bank conflicts.  Colours, barycentrics and texels are read per lane only for slots whose blend weight is
// not exactly zero (with gamma = 1e-4 nearly every slot behind the nearest has weight 0).  The backwards recompute
// the forward from the same inputs and write grad_dists / grad_zbuf back through the same LDS rows.
//
// Scattering backwards (atlas, face attributes): float atomics, zero contributions skipped; deterministic mode
// (AcfmRasterTuning.flags bit 0) sums every contribution as two integers (frag_split, as k_frag_bwd) into the
// workspace and converts once at the end.
#include <climits>
#include <type_traits>

#include "acfm_common.h"

namespace acfm {

constexpr int SH_TPB = 64;      // blend kernels: one wave, one pixel per lane
constexpr int SH_ITPB = 256;    // interpolation / conversion kernels: one slot (or element) per thread
constexpr float SH_EPS = 1e-10f;   // softmax_rgb_blend eps

// [64, K] plane of the wave's pixels -> LDS rows of K + 1 words (int64 ids: the low word; ids fit an int)
template <int K, typename T, typename S>
__device__ __forceinline__ void stage_rows(S* __restrict__ dst, const T* __restrict__ src, size_t p0, size_t P,
                                           int lane) {
  const size_t n = (P - p0 < (size_t)SH_TPB ? P - p0 : (size_t)SH_TPB) * K;
  const T* s = src + p0 * K;
  for (size_t t = lane; t < n; t += SH_TPB) dst[(t / K) * (K + 1) + t % K] = (S)s[t];
}
template <int K, typename S>
__device__ __forceinline__ void unstage_rows(float* __restrict__ dst, const S* __restrict__ src, size_t p0, size_t P,
                                             int lane) {
  const size_t n = (P - p0 < (size_t)SH_TPB ? P - p0 : (size_t)SH_TPB) * K;
  float* d = dst + p0 * K;
  for (size_t t = lane; t < n; t += SH_TPB) d[t] = src[(t / K) * (K + 1) + t % K];
}

// TexturesAtlas.sample_textures (oracle_atlas_shade): w_xy = (int)(w01 R) (truncation, as PyTorch3D's .to(int64)),
// mirrored above the diagonal, clamped to [0, R - 1] -> linear texel index f R^2 + y R + x
__device__ __forceinline__ size_t atlas_texel(int f, float w0, float w1, int R) {
  int ix = (int)(w0 * (float)R), iy = (int)(w1 * (float)R);
  if (!(((w0 + w1) * (float)R - ((float)ix + (float)iy)) <= 1.0f)) {
    ix = R - 1 - ix;
    iy = R - 1 - iy;
  }
  ix = ix < 0 ? 0 : (ix > R - 1 ? R - 1 : ix);
  iy = iy < 0 ? 0 : (iy > R - 1 ? R - 1 : iy);
  return ((size_t)f * R + iy) * R + ix;
}

struct ShadeArgs {
  const int64_t* p2f;
  const float* dists;
  const float* zbuf;
  const float* bary;      // atlas source
  const float* colors;    // dense source [P,K,3] (NULL: atlas)
  const float* atlas;     // [F_packed,R,R,3]
  const float* ambient;   // [N,3] or NULL
  size_t P;
  int pix_per_mesh, R, F_packed;   // F_packed: faces the ids may name (INT_MAX for dense colours)
  float sigma, gamma, bg[3], znear, zfar;
};

// colour of slot k of pixel p (face f >= 0): the dense tensor, or the atlas texel times the mesh's ambient factor
template <bool ATLAS>
__device__ __forceinline__ float3 slot_color(const ShadeArgs& a, size_t p, int K, int k, int f, size_t* ti) {
  const size_t s = p * K + k;
  if constexpr (ATLAS) {
    *ti = atlas_texel(f, a.bary[3 * s], a.bary[3 * s + 1], a.R);
    float3 c = make_float3(a.atlas[3 * *ti], a.atlas[3 * *ti + 1], a.atlas[3 * *ti + 2]);
    if (a.ambient) {
      const float* am = a.ambient + 3 * (p / (size_t)a.pix_per_mesh);
      c = make_float3(am[0] * c.x, am[1] * c.y, am[2] * c.z);
    }
    return c;
  } else {
    return make_float3(a.colors[3 * s], a.colors[3 * s + 1], a.colors[3 * s + 2]);
  }
}

// ------------------------------------------------------------------------------ sigmoid_alpha_blend
// RGB = colour of slot 0 (1 without colours: the silhouette shader), A = 1 - prod_k (1 - p_k),
// p_k = sigmoid(-dists_k / sigma) [f_k >= 0]
template <int K>
__global__ __launch_bounds__(SH_TPB) void k_sigmoid_blend_fwd(const int64_t* __restrict__ p2f,
                                                              const float* __restrict__ dists,
                                                              const float* __restrict__ colors, size_t P, float sigma,
                                                              float4* __restrict__ rgba) {
  __shared__ int s_f[SH_TPB * (K + 1)];
  __shared__ float s_d[SH_TPB * (K + 1)];
  const int lane = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * SH_TPB, p = p0 + lane;
  stage_rows<K>(s_f, p2f, p0, P, lane);
  stage_rows<K>(s_d, dists, p0, P, lane);
  __syncthreads();
  if (p >= P) return;
  float prod = 1.0f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int o = lane * (K + 1) + k;
    const float pk = s_f[o] >= 0 ? sigmoid_neg(s_d[o], sigma) : 0.0f;
    prod *= 1.0f - pk;
  }
  float4 out = make_float4(1.0f, 1.0f, 1.0f, 1.0f - prod);
  if (colors) {
    out.x = colors[3 * p * K];
    out.y = colors[3 * p * K + 1];
    out.z = colors[3 * p * K + 2];
  }
  rgba[p] = out;
}

// d A / d dists_k = -(1 - A) p_k / sigma (the closed form of App-A.5: no division by 1 - p_k); d RGB / d colours of
// slot 0 = 1, other slots 0
template <int K>
__global__ __launch_bounds__(SH_TPB) void k_sigmoid_blend_bwd(const int64_t* __restrict__ p2f,
                                                              const float* __restrict__ dists,
                                                              const float4* __restrict__ g_rgba, size_t P, float sigma,
                                                              float* __restrict__ g_dists,
                                                              float* __restrict__ g_colors) {
  __shared__ int s_f[SH_TPB * (K + 1)];
  __shared__ float s_d[SH_TPB * (K + 1)];
  const int lane = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * SH_TPB, p = p0 + lane;
  float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
  if (p < P) g = g_rgba[p];
  if (g_dists) {
    stage_rows<K>(s_f, p2f, p0, P, lane);
    stage_rows<K>(s_d, dists, p0, P, lane);
    __syncthreads();
    if (p < P) {
      float pk[K];
      float prod = 1.0f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const int o = lane * (K + 1) + k;
        pk[k] = s_f[o] >= 0 ? sigmoid_neg(s_d[o], sigma) : 0.0f;
        prod *= 1.0f - pk[k];
      }
      const float c = -g.w * prod / sigma;
#pragma unroll
      for (int k = 0; k < K; ++k) s_d[lane * (K + 1) + k] = c * pk[k];
    }
    __syncthreads();
    unstage_rows<K>(g_dists, s_d, p0, P, lane);
  }
  if (g_colors && p < P) {
    float* gc = g_colors + 3 * p * K;
    gc[0] = g.x;
    gc[1] = g.y;
    gc[2] = g.z;
#pragma unroll
    for (int k = 1; k < K; ++k) gc[3 * k] = gc[3 * k + 1] = gc[3 * k + 2] = 0.0f;
  }
}

// ------------------------------------------------------------------------------ softmax_rgb_blend
// Per pixel, from the staged rows: p_k, w_k, z_max (and its first arg-max), delta, prod (1 - p_k).  z_inv and the
// exponents are formed in float64: (z_inv_k - z_max) / gamma magnifies the float32 rounding of z_inv by 1 / gamma
// (1e4), which would move w_k by 6e-4 of itself; the exponentials themselves are float32.
template <int K>
struct SoftPix {
  float pk[K], w[K];
  float delta;
  bool zmax_live, delta_live;   // the clamps of z_max and delta pass gradient (not at their floor)
  int kmax;
  float prod;
};
template <int K>
__device__ __forceinline__ void soft_pix(const int* s_f, const float* s_d, const float* s_z, int lane,
                                         const ShadeArgs& a, SoftPix<K>& q) {
  double zi[K];
  double zmax_raw = -INFINITY;
  q.kmax = 0;
  q.prod = 1.0f;
  const double zfar = a.zfar, range = (double)a.zfar - (double)a.znear, eps = SH_EPS, gamma = a.gamma;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int o = lane * (K + 1) + k;
    const bool m = s_f[o] >= 0 && s_f[o] < a.F_packed;
    q.pk[k] = m ? sigmoid_neg(s_d[o], a.sigma) : 0.0f;
    zi[k] = m ? (zfar - (double)s_z[o]) / range : 0.0;   // (zfar - z) / (zfar - znear) * mask
    if (zi[k] > zmax_raw) {                             // strict: the first maximal slot, as torch.max
      zmax_raw = zi[k];
      q.kmax = k;
    }
    q.prod *= 1.0f - q.pk[k];
  }
  const double zmax = fmax(zmax_raw, eps);
#pragma unroll
  for (int k = 0; k < K; ++k) q.w[k] = q.pk[k] * expf((float)((zi[k] - zmax) / gamma));
  const float delta_raw = expf((float)((eps - zmax) / gamma));
  q.delta = fmaxf(delta_raw, SH_EPS);
  q.zmax_live = zmax_raw >= eps;
  q.delta_live = delta_raw >= SH_EPS;
}

template <int K, bool ATLAS>
__global__ __launch_bounds__(SH_TPB) void k_softmax_blend_fwd(ShadeArgs a, float4* __restrict__ rgba) {
  __shared__ int s_f[SH_TPB * (K + 1)];
  __shared__ float s_d[SH_TPB * (K + 1)];
  __shared__ float s_z[SH_TPB * (K + 1)];
  const int lane = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * SH_TPB, p = p0 + lane;
  stage_rows<K>(s_f, a.p2f, p0, a.P, lane);
  stage_rows<K>(s_d, a.dists, p0, a.P, lane);
  stage_rows<K>(s_z, a.zbuf, p0, a.P, lane);
  __syncthreads();
  if (p >= a.P) return;
  SoftPix<K> q;
  soft_pix<K>(s_f, s_d, s_z, lane, a, q);
  float S = 0.f, cr = 0.f, cg = 0.f, cb = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    S += q.w[k];
    if (q.w[k] != 0.0f) {
      size_t ti;
      const float3 c = slot_color<ATLAS>(a, p, K, k, s_f[lane * (K + 1) + k], &ti);
      cr += q.w[k] * c.x;
      cg += q.w[k] * c.y;
      cb += q.w[k] * c.z;
    }
  }
  const float D = S + q.delta;
  rgba[p] = make_float4((cr + q.delta * a.bg[0]) / D, (cg + q.delta * a.bg[1]) / D, (cb + q.delta * a.bg[2]) / D,
                        1.0f - q.prod);
}

// Backward (App-A.10).  With q_k = g . c_k and q_bg = g . bg (g = grad RGB), D = sum w + delta:
//   d L / d w_k   = (sum_j w_j (q_k - q_j) + delta (q_k - q_bg)) / D^2      (c_k - rgb written without cancellation)
//   d L / d z_max = -(delta / gamma) (sum_j w_j q_j - S q_bg) / D^2 while delta sits at its clamp, else 0 (the two
//                   z_max paths cancel exactly); it goes to the first maximal slot, and only while z_max >= eps
//   d L / d zbuf_k  = -(gw_k w_k / gamma + [k = kmax] gzmax) [f_k >= 0] / (zfar - znear)
//   d L / d dists_k = -(gw_k w_k (1 - p_k) + gA prod p_k) / sigma
//   d L / d colour_k = g w_k / D   (dense: [P,K,3] overwritten, w_k / D and g go through LDS so that the wave stores
//                                   its 64 x 3K floats contiguously; atlas: times the ambient factor, scattered)
template <int K, bool ATLAS, bool DET>
__global__ __launch_bounds__(SH_TPB) void k_softmax_blend_bwd(ShadeArgs a, const float4* __restrict__ g_rgba,
                                                              float* __restrict__ g_dists, float* __restrict__ g_zbuf,
                                                              float* __restrict__ g_colors, void* __restrict__ g_atlas) {
  __shared__ int s_f[SH_TPB * (K + 1)];
  __shared__ float s_d[SH_TPB * (K + 1)];
  __shared__ float s_z[SH_TPB * (K + 1)];
  __shared__ float4 s_g[ATLAS ? 1 : SH_TPB];   // dense: grad RGBA of the wave's pixels
  const int lane = threadIdx.x;
  const size_t p0 = (size_t)blockIdx.x * SH_TPB, p = p0 + lane;
  stage_rows<K>(s_f, a.p2f, p0, a.P, lane);
  stage_rows<K>(s_d, a.dists, p0, a.P, lane);
  stage_rows<K>(s_z, a.zbuf, p0, a.P, lane);
  __syncthreads();
  if (p < a.P) {
    const float4 g = g_rgba[p];
    if constexpr (!ATLAS) s_g[lane] = g;
    SoftPix<K> q;
    soft_pix<K>(s_f, s_d, s_z, lane, a, q);
    float qk[K];
    float S = 0.f, Qw = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      qk[k] = 0.0f;
      S += q.w[k];
      if (q.w[k] != 0.0f) {
        size_t ti;
        const float3 c = slot_color<ATLAS>(a, p, K, k, s_f[lane * (K + 1) + k], &ti);
        qk[k] = g.x * c.x + g.y * c.y + g.z * c.z;
        Qw += q.w[k] * qk[k];
      }
    }
    const float D = S + q.delta, D2 = D * D;
    const float qbg = g.x * a.bg[0] + g.y * a.bg[1] + g.z * a.bg[2];
    const float gzmax = (q.zmax_live && !q.delta_live) ? -(q.delta / a.gamma) * ((Qw - S * qbg) / D2) : 0.0f;
    const float range = a.zfar - a.znear;
    const float gA = g.w;
    const float* am = (ATLAS && a.ambient) ? a.ambient + 3 * (p / (size_t)a.pix_per_mesh) : nullptr;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int o = lane * (K + 1) + k;
      const int f = s_f[o];
      float gww = 0.0f;   // d L / d w_k times w_k
      if (q.w[k] != 0.0f) {
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (q.w[j] != 0.0f && j != k) acc += q.w[j] * (qk[k] - qk[j]);
        gww = q.w[k] * ((acc + q.delta * (qk[k] - qbg)) / D2);
      }
      const float gzi = gww / a.gamma + (k == q.kmax ? gzmax : 0.0f);
      s_z[o] = f >= 0 ? -gzi / range : 0.0f;
      s_d[o] = -(gww * (1.0f - q.pk[k]) + gA * q.prod * q.pk[k]) / a.sigma;
      if constexpr (!ATLAS) {
        s_f[o] = __float_as_int(q.w[k] / D);   // this lane's row: its face id has been read above
      } else {
        if (g_atlas && q.w[k] != 0.0f) {
          const size_t s = p * K + k;
          const size_t ti = atlas_texel(f, a.bary[3 * s], a.bary[3 * s + 1], a.R);
          const float sc = q.w[k] / D;
          const float v[3] = {g.x * sc * (am ? am[0] : 1.0f), g.y * sc * (am ? am[1] : 1.0f),
                              g.z * sc * (am ? am[2] : 1.0f)};
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            if (v[c] == 0.0f) continue;
            if constexpr (DET) {
              const FragFix x = frag_split((double)v[c]);
              unsigned long long* acc = reinterpret_cast<unsigned long long*>(g_atlas) + 2 * (3 * ti + c);
              if (x.hi) atomicAdd(acc, (unsigned long long)x.hi);
              if (x.lo) atomicAdd(acc + 1, (unsigned long long)x.lo);
            } else {
              atomicAdd(reinterpret_cast<float*>(g_atlas) + 3 * ti + c, v[c]);
            }
          }
        }
      }
    }
  }
  __syncthreads();
  if (g_dists) unstage_rows<K>(g_dists, s_d, p0, a.P, lane);
  if (g_zbuf) unstage_rows<K>(g_zbuf, s_z, p0, a.P, lane);
  if constexpr (!ATLAS) {
    if (g_colors) {   // grad_colors [p, k, c] = g_c(p) w_k / D, the wave's 3 K floats per pixel stored contiguously
      const int npix = a.P - p0 < (size_t)SH_TPB ? (int)(a.P - p0) : SH_TPB;
      float* gc = g_colors + 3 * p0 * K;
      for (int t = lane; t < npix * 3 * K; t += SH_TPB) {
        const int px = t / (3 * K), r = t - px * 3 * K, k = r / 3, c = r - 3 * k;
        const float4 g = s_g[px];
        gc[t] = (c == 0 ? g.x : c == 1 ? g.y : g.z) * __int_as_float(s_f[px * (K + 1) + k]);
      }
    }
  }
}

// ------------------------------------------------------------------------------ interpolate_face_attributes
// one thread per (pixel, slot): out[s, d] = sum_i bary[s, i] attrs[f, i, d], 0 where empty
__global__ __launch_bounds__(SH_ITPB) void k_interp_fwd(const int64_t* __restrict__ p2f, const float* __restrict__ bary,
                                                        const float* __restrict__ attrs, size_t PK, int D, int F_packed,
                                                        float* __restrict__ out) {
  const size_t s = (size_t)blockIdx.x * SH_ITPB + threadIdx.x;
  if (s >= PK) return;
  const int64_t f = p2f[s];
  float* o = out + s * D;
  if (f < 0 || f >= F_packed) {
    for (int d = 0; d < D; ++d) o[d] = 0.0f;
    return;
  }
  const float b0 = bary[3 * s], b1 = bary[3 * s + 1], b2 = bary[3 * s + 2];
  const float* A = attrs + (size_t)f * 3 * D;
  for (int d = 0; d < D; ++d) o[d] = b0 * A[d] + b1 * A[D + d] + b2 * A[2 * D + d];
}

template <bool DET>
__global__ __launch_bounds__(SH_ITPB) void k_interp_bwd(const int64_t* __restrict__ p2f, const float* __restrict__ bary,
                                                        const float* __restrict__ attrs, const float* __restrict__ g_out,
                                                        size_t PK, int D, int F_packed, float* __restrict__ g_bary,
                                                        void* __restrict__ g_attrs) {
  const size_t s = (size_t)blockIdx.x * SH_ITPB + threadIdx.x;
  if (s >= PK) return;
  const int64_t f = p2f[s];
  if (f < 0 || f >= F_packed) {
    if (g_bary) g_bary[3 * s] = g_bary[3 * s + 1] = g_bary[3 * s + 2] = 0.0f;
    return;
  }
  const float* g = g_out + s * D;
  if (g_bary) {
    const float* A = attrs + (size_t)f * 3 * D;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int d = 0; d < D; ++d) {
      const float gd = g[d];
      a0 += gd * A[d];
      a1 += gd * A[D + d];
      a2 += gd * A[2 * D + d];
    }
    g_bary[3 * s] = a0;
    g_bary[3 * s + 1] = a1;
    g_bary[3 * s + 2] = a2;
  }
  if (g_attrs) {
    const float b[3] = {bary[3 * s], bary[3 * s + 1], bary[3 * s + 2]};
    const size_t base = (size_t)f * 3 * D;
    for (int d = 0; d < D; ++d) {
      const float gd = g[d];
      if (gd == 0.0f) continue;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        const float v = gd * b[i];
        if (v == 0.0f) continue;
        const size_t e = base + (size_t)i * D + d;
        if constexpr (DET) {
          const FragFix x = frag_split((double)v);
          unsigned long long* acc = reinterpret_cast<unsigned long long*>(g_attrs) + 2 * e;
          if (x.hi) atomicAdd(acc, (unsigned long long)x.hi);
          if (x.lo) atomicAdd(acc + 1, (unsigned long long)x.lo);
        } else {
          atomicAdd(reinterpret_cast<float*>(g_attrs) + e, v);
        }
      }
    }
  }
}

// deterministic mode: the (hi, lo) integer sums -> float
__global__ __launch_bounds__(SH_ITPB) void k_shade_fix_finish(const long long* __restrict__ fix, size_t n,
                                                              float* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * SH_ITPB + threadIdx.x;
  if (j < n) out[j] = frag_unsplit(fix[2 * j], fix[2 * j + 1]);
}

// ------------------------------------------------------------------------------ host side
template <class Fn>
static int with_k(int K, Fn&& fn) {
  switch (K) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    case 8: fn(std::integral_constant<int, 8>{}); break;
    case 10: fn(std::integral_constant<int, 10>{}); break;
    case 20: fn(std::integral_constant<int, 20>{}); break;
    case 32: fn(std::integral_constant<int, 32>{}); break;
    default: return ACFM_E_BADARG;
  }
  return ACFM_OK;
}

// the rules of every fragments entry point: P K within the raster's bound, K in the fragment set, no half storage
static bool shade_tune(const AcfmRasterTuning* tuning, Tune& tn) { return tune_from(tuning, tn) && !tn.f16; }
static bool bad_pk(size_t P, int K) { return P == 0 || P * (size_t)(K > 0 ? K : 1) > ((size_t)1 << 40); }
static unsigned blocks_of(size_t n, int tpb) { return (unsigned)((n + tpb - 1) / tpb); }

static bool bad_blend(const AcfmBlendParams* b) {
  return !b || !(b->sigma > 0.f) || !(b->gamma > 0.f) || !(b->zfar != b->znear);
}

static int shade_args(const int64_t* p2f, const float* dists, const float* zbuf, const float* bary, const float* colors,
                      const float* atlas, int R, int F_packed, const float* ambient, size_t P, int pix_per_mesh,
                      const AcfmBlendParams* b, ShadeArgs& a) {
  if (!p2f || !dists || !zbuf || bad_blend(b)) return ACFM_E_BADARG;
  if ((colors != nullptr) == (atlas != nullptr)) return ACFM_E_BADARG;   // exactly one colour source
  if (atlas && (!bary || R <= 0 || R > 256 || F_packed <= 0)) return ACFM_E_BADARG;
  if (atlas && (size_t)F_packed * R * R > ((size_t)1 << 36)) return ACFM_E_BADARG;
  if (ambient && (pix_per_mesh <= 0 || P % (size_t)pix_per_mesh != 0)) return ACFM_E_BADARG;
  a = ShadeArgs{p2f, dists, zbuf, bary, colors, atlas, ambient, P, pix_per_mesh > 0 ? pix_per_mesh : 1, R,
                atlas ? F_packed : INT_MAX,
                b->sigma, b->gamma, {b->background[0], b->background[1], b->background[2]}, b->znear, b->zfar};
  return ACFM_OK;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_sigmoid_alpha_blend(const int64_t* pix_to_face, const float* dists, const float* colors, size_t P, int K,
                             float sigma, float* rgba, const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  if (!pix_to_face || !dists || !rgba || bad_pk(P, K) || !(sigma > 0.f) || !shade_tune(tuning, tn))
    return ACFM_E_BADARG;
  if (((uintptr_t)rgba & 15) != 0) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = with_k(K, [&](auto kc) {
    hipLaunchKernelGGL((k_sigmoid_blend_fwd<decltype(kc)::value>), dim3(blocks_of(P, SH_TPB)), dim3(SH_TPB), 0, st,
                       pix_to_face, dists, colors, P, sigma, reinterpret_cast<float4*>(rgba));
  });
  if (rc) return rc;
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_sigmoid_alpha_blend_backward(const int64_t* pix_to_face, const float* dists, const float* grad_rgba,
                                      size_t P, int K, float sigma, float* grad_dists, float* grad_colors,
                                      const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  if (!pix_to_face || !dists || !grad_rgba || bad_pk(P, K) || !(sigma > 0.f) || !shade_tune(tuning, tn))
    return ACFM_E_BADARG;
  if (((uintptr_t)grad_rgba & 15) != 0) return ACFM_E_BADARG;
  if (!grad_dists && !grad_colors) return ACFM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int rc = with_k(K, [&](auto kc) {
    hipLaunchKernelGGL((k_sigmoid_blend_bwd<decltype(kc)::value>), dim3(blocks_of(P, SH_TPB)), dim3(SH_TPB), 0, st,
                       pix_to_face, dists, reinterpret_cast<const float4*>(grad_rgba), P, sigma, grad_dists,
                       grad_colors);
  });
  if (rc) return rc;
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_softmax_rgb_blend(const int64_t* pix_to_face, const float* dists, const float* zbuf, const float* bary,
                           const float* colors, const float* atlas, int R, int F_packed, const float* ambient,
                           size_t P, int K, int pix_per_mesh, const AcfmBlendParams* blend, float* rgba,
                           const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  ShadeArgs a;
  if (!rgba || ((uintptr_t)rgba & 15) != 0 || bad_pk(P, K) || !shade_tune(tuning, tn)) return ACFM_E_BADARG;
  if (shade_args(pix_to_face, dists, zbuf, bary, colors, atlas, R, F_packed, ambient, P, pix_per_mesh, blend, a))
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int rc = with_k(K, [&](auto kc) {
    constexpr int KK = decltype(kc)::value;
    if (atlas)
      hipLaunchKernelGGL((k_softmax_blend_fwd<KK, true>), dim3(blocks_of(P, SH_TPB)), dim3(SH_TPB), 0, st, a,
                         reinterpret_cast<float4*>(rgba));
    else
      hipLaunchKernelGGL((k_softmax_blend_fwd<KK, false>), dim3(blocks_of(P, SH_TPB)), dim3(SH_TPB), 0, st, a,
                         reinterpret_cast<float4*>(rgba));
  });
  if (rc) return rc;
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_softmax_rgb_blend_backward(const int64_t* pix_to_face, const float* dists, const float* zbuf,
                                    const float* bary, const float* colors, const float* atlas, int R, int F_packed,
                                    const float* ambient, size_t P, int K, int pix_per_mesh,
                                    const AcfmBlendParams* blend, const float* grad_rgba, float* grad_dists,
                                    float* grad_zbuf, float* grad_colors, float* grad_atlas, void* ws,
                                    size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  ShadeArgs a;
  if (!grad_rgba || ((uintptr_t)grad_rgba & 15) != 0 || bad_pk(P, K) || !shade_tune(tuning, tn)) return ACFM_E_BADARG;
  if (shade_args(pix_to_face, dists, zbuf, bary, colors, atlas, R, F_packed, ambient, P, pix_per_mesh, blend, a))
    return ACFM_E_BADARG;
  if (grad_colors && !colors) return ACFM_E_BADARG;   // grad_colors belongs to the dense source,
  if (grad_atlas && !atlas) return ACFM_E_BADARG;     // grad_atlas to the atlas
  if (!grad_dists && !grad_zbuf && !grad_colors && !grad_atlas) return ACFM_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t n_atlas = atlas ? (size_t)F_packed * R * R * 3 : 0;
  const bool det = tn.deterministic && grad_atlas;
  void* acc = grad_atlas;
  if (grad_atlas) {
    if (det) {
      if (!ws || ws_bytes < 2 * sizeof(long long) * n_atlas) return ACFM_E_WORKSPACE;
      acc = ws;
      if (zero_async(ws, 2 * sizeof(long long) * n_atlas, st)) return ACFM_E_LAUNCH;
    } else if (zero_async(grad_atlas, sizeof(float) * n_atlas, st)) {
      return ACFM_E_LAUNCH;
    }
  }
  const int rc = with_k(K, [&](auto kc) {
    constexpr int KK = decltype(kc)::value;
    const dim3 grid(blocks_of(P, SH_TPB)), blk(SH_TPB);
    const float4* g = reinterpret_cast<const float4*>(grad_rgba);
    if (!atlas)
      hipLaunchKernelGGL((k_softmax_blend_bwd<KK, false, false>), grid, blk, 0, st, a, g, grad_dists, grad_zbuf,
                         grad_colors, nullptr);
    else if (det)
      hipLaunchKernelGGL((k_softmax_blend_bwd<KK, true, true>), grid, blk, 0, st, a, g, grad_dists, grad_zbuf,
                         nullptr, acc);
    else
      hipLaunchKernelGGL((k_softmax_blend_bwd<KK, true, false>), grid, blk, 0, st, a, g, grad_dists, grad_zbuf,
                         nullptr, acc);
  });
  if (rc) return rc;
  if (det)
    hipLaunchKernelGGL(k_shade_fix_finish, dim3(blocks_of(n_atlas, SH_ITPB)), dim3(SH_ITPB), 0, st,
                       reinterpret_cast<const long long*>(ws), n_atlas, grad_atlas);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_interpolate_face_attributes(const int64_t* pix_to_face, const float* bary, const float* face_attrs,
                                     size_t P, int K, int F_packed, int D, float* out,
                                     const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  if (!pix_to_face || !bary || !face_attrs || !out || bad_pk(P, K) || K <= 0 || K > ACFM_MAX_K || F_packed <= 0 ||
      D <= 0 || !shade_tune(tuning, tn))
    return ACFM_E_BADARG;
  const size_t PK = P * K;
  hipLaunchKernelGGL(k_interp_fwd, dim3(blocks_of(PK, SH_ITPB)), dim3(SH_ITPB), 0, (hipStream_t)stream, pix_to_face,
                     bary, face_attrs, PK, D, F_packed, out);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_interpolate_face_attributes_backward(const int64_t* pix_to_face, const float* bary, const float* face_attrs,
                                              const float* grad_out, size_t P, int K, int F_packed, int D,
                                              float* grad_bary, float* grad_face_attrs, void* ws, size_t ws_bytes,
                                              const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  if (!pix_to_face || !bary || !face_attrs || !grad_out || bad_pk(P, K) || K <= 0 || K > ACFM_MAX_K ||
      F_packed <= 0 || D <= 0 || !shade_tune(tuning, tn))
    return ACFM_E_BADARG;
  if (!grad_bary && !grad_face_attrs) return ACFM_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t PK = P * K, n_attr = (size_t)F_packed * 3 * D;
  const bool det = tn.deterministic && grad_face_attrs;
  void* acc = grad_face_attrs;
  if (grad_face_attrs) {
    if (det) {
      if (!ws || ws_bytes < 2 * sizeof(long long) * n_attr) return ACFM_E_WORKSPACE;
      acc = ws;
      if (zero_async(ws, 2 * sizeof(long long) * n_attr, st)) return ACFM_E_LAUNCH;
    } else if (zero_async(grad_face_attrs, sizeof(float) * n_attr, st)) {
      return ACFM_E_LAUNCH;
    }
  }
  if (det)
    hipLaunchKernelGGL(k_interp_bwd<true>, dim3(blocks_of(PK, SH_ITPB)), dim3(SH_ITPB), 0, st, pix_to_face, bary,
                       face_attrs, grad_out, PK, D, F_packed, grad_bary, acc);
  else
    hipLaunchKernelGGL(k_interp_bwd<false>, dim3(blocks_of(PK, SH_ITPB)), dim3(SH_ITPB), 0, st, pix_to_face, bary,
                       face_attrs, grad_out, PK, D, F_packed, grad_bary, acc);
  if (det)
    hipLaunchKernelGGL(k_shade_fix_finish, dim3(blocks_of(n_attr, SH_ITPB)), dim3(SH_ITPB), 0, st,
                       reinterpret_cast<const long long*>(ws), n_attr, grad_face_attrs);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
