// Backward of the deformable convolution of acfm_dconv.hip (same configuration, fp32), for fine-tuning the flow network.
// With col[k = 9 ci + t, p] the sampled column of the forward and gcol[k, p] = sum_co W[co, k] go[co, p]:
//   grad_input  : bw_corner(t, p) gcol[ci, t, p] scattered to the four corners of the sample cell;
//   grad_offset : sum_ci gcol[ci, t, p] dS/dh and dS/dw, dS/dh = uw (v10 - v00) + lw (v11 - v01),
//                 dS/dw = uh (v01 - v00) + lh (v11 - v10), corners outside the map counting 0 and the whole gradient 0
//                 for a position outside (-1, H) x (-1, W).  At an integer coordinate lh = h - floor(h) = 0: the cell is
//                 the floor cell, the derivative the forward difference towards the +1 neighbour (torchvision's);
//   grad_weight : gw[co, k] = sum_{n, p} go[n, co, p] col[k, n, p];   grad_bias[co] = sum_{n, p} go[n, co, p].
// Nothing of the forward is saved: both kernels recompute the tap table (corner indices, fractions) as the forward does.
//
// k_dconv_bwd_data owns DB_TP = 32 pixels of one image.  Per chunk of DB_CC = 16 input channels (DB_KC = 144 rows of
// gcol = nine 16-row MFMA subtiles) it streams `weight` as it lies in memory in DB_CO = 64 output-channel slabs next to
// the matching go[64, 32] slab, forms gcol[144, 32] with v_mfma_f32_16x16x4_f32 (exact fp32; the reduction runs over co
// in index order), parks it in LDS over the weight slab and consumes it at once: thread (pixel, channel lane cl of 8)
// takes channels cl and cl + 8 of the chunk and all nine taps, adds the four corner terms to grad_input with float
// atomics (a data-dependent scatter into a zero-filled buffer: THIS gradient does not repeat its bits) and keeps the
// offset derivative of its channels in 18 registers.  After the last chunk the eight channel lanes are added through LDS
// in a fixed order: grad_offset has no atomics and repeats its bits.  The shared form (2-channel offset) reads another
// offset address and adds the nine taps before the store: the gradient of the flow itself.
//
// k_dconv_bwd_weight is a GEMM reduced over pixels: a workgroup owns a [64 co, 144 k] tile of gw and a range of
// 32-pixel tiles; per pixel tile it resamples the column chunk into LDS as the forward does, loads go[64, 32] and runs
// the matrix cores over the 32 pixels (wave w: output channels 16 w .. 16 w + 15, nine k subtiles: one go operand feeds
// nine accumulators).  The partial sums of the pixel ranges go to a workspace [parts, Cout, 9 Cin] and
// k_dconv_bwd_wreduce adds them in index order: no atomics, the same bits on every run.  k_dconv_bwd_bias is a
// fixed-order reduction of go per output channel.
#include "acfm_common.h"

namespace acfm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DB_TP = 32;             // pixels per workgroup tile
constexpr int DB_CC = 16;             // input channels per chunk
constexpr int DB_KC = 9 * DB_CC;      // rows of gcol / col per chunk: 9 subtiles of 16
constexpr int DB_CO = 64;             // output channels per slab (data kernel) / per workgroup tile (weight kernel)
// LDS strides in floats.  ds_read_b32 serves lanes 0-31 and 32-63 separately; an operand read [4 s + (l >> 4)][l & 15]
// wants a stride = 16 mod 32 (144, 48), an operand read [l & 15][4 s + (l >> 4)] a stride = 2 mod 32 (34).
constexpr int DB_WS = DB_KC;          // weight slab [co][k]
constexpr int DB_GS = 48;             // go slab [co][pixel] of the data kernel
constexpr int DB_PS = 33;             // parked gcol [k][pixel]
constexpr int DB_TS = 34;             // go tile [co][pixel] and column chunk [k][pixel] of the weight kernel
static_assert(DB_WS % 32 == 16 && DB_GS % 32 == 16 && DB_TS % 32 == 2 && DB_TP == 32 && DB_KC % 16 == 0, "tile constants");
static_assert(DB_KC * DB_PS <= DB_CO * DB_WS && 8 * 18 * DB_TP <= DB_CO * DB_WS, "gcol and the lane sums fit over the slab");

// corner plane offsets (-1 = outside the map) and the fractions (lh, lw) of tap t at pixel p; a position outside
// (-1, H) x (-1, W) (or NaN) has no corner at all, so every term that follows is 0
template <bool SHARED>
__device__ __forceinline__ void tap_entry(const float* __restrict__ off, int n, int t, int p, int H, int W, int HW, int4& ix,
                                          float2& fr) {
  ix = int4{-1, -1, -1, -1};
  fr = float2{0.f, 0.f};
  if (p >= HW) return;
  const int y = p / W, x = p - y * W, ky = t / 3, kx = t - 3 * ky;
  const float* o = off + (size_t)n * (SHARED ? 2 : 18) * HW + (SHARED ? 0 : (size_t)(2 * t) * HW) + p;
  const float h = (float)(y - 1 + ky) + o[0];
  const float w = (float)(x - 1 + kx) + o[HW];
  if (h > -1.0f && h < (float)H && w > -1.0f && w < (float)W) {
    const float hf = floorf(h), wf = floorf(w);
    const int hl = (int)hf, wl = (int)wf, hh = hl + 1, wh = wl + 1;
    if (hl >= 0 && wl >= 0) ix.x = hl * W + wl;
    if (hl >= 0 && wh <= W - 1) ix.y = hl * W + wh;
    if (hh <= H - 1 && wl >= 0) ix.z = hh * W + wl;
    if (hh <= H - 1 && wh <= W - 1) ix.w = hh * W + wh;
    fr = float2{h - hf, w - wf};
  }
}

template <bool SHARED>
__global__ __launch_bounds__(256) void k_dconv_bwd_data(const float* __restrict__ go, const float* __restrict__ in,
                                                        const float* __restrict__ off, const float* __restrict__ wgt,
                                                        int Cin, int H, int W, int Cout, int tiles,
                                                        float* __restrict__ gin, float* __restrict__ goff) {
  __shared__ int4 s_idx[9 * DB_TP];
  __shared__ float2 s_fr[9 * DB_TP];
  __shared__ float s_go[DB_CO][DB_GS];
  __shared__ float s_w[DB_CO * DB_WS];                  // the weight slab; then gcol [144][33]; at the end the lane sums
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = blockIdx.x / tiles, p0 = (blockIdx.x % tiles) * DB_TP;
  const int HW = H * W, K = 9 * Cin;
  const float* img = in + (size_t)n * Cin * HW;
  const float* gon = go + (size_t)n * Cout * HW;

  for (int e = tid; e < 9 * DB_TP; e += 256) {
    int4 ix;
    float2 fr;
    tap_entry<SHARED>(off, n, e / DB_TP, p0 + (e % DB_TP), H, W, HW, ix, fr);
    s_idx[e] = ix;
    s_fr[e] = fr;
  }

  const int li = lane & 15, lk = lane >> 4;
  const int pxs = (wv & 1) * 16, j0 = wv >> 1;          // this wave's pixel half; its k subtiles are j0, j0 + 2, ..
  const int px = tid & 31, cl = tid >> 5;               // the consumer's pixel and channel lane
  float dh[9], dw[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) dh[t] = dw[t] = 0.f;

  for (int c0 = 0; c0 < Cin; c0 += DB_CC) {
    f32x4 acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int cb = 0; cb < Cout; cb += DB_CO) {
      __syncthreads();                                   // the slab (or the parked gcol) has been read by everyone
      for (int e = tid; e < DB_CO * DB_KC; e += 256) {
        const int row = e / DB_KC, kk = e - row * DB_KC, co = cb + row, k = 9 * c0 + kk;
        s_w[row * DB_WS + kk] = (co < Cout && k < K) ? wgt[(size_t)co * K + k] : 0.f;
      }
      for (int e = tid; e < DB_CO * DB_TP; e += 256) {
        const int row = e >> 5, q = e & 31, co = cb + row, p = p0 + q;
        s_go[row][q] = (co < Cout && p < HW) ? gon[(size_t)co * HW + p] : 0.f;
      }
      __syncthreads();
#pragma unroll 4
      for (int s = 0; s < DB_CO / 4; ++s) {
        const float b = s_go[4 * s + lk][pxs + li];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
          const int j = j0 + 2 * i;
          if (j < 9)                                     // (wave-uniform: waves 2, 3 own four subtiles)
            acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[(4 * s + lk) * DB_WS + 16 * j + li], b, acc[i], 0, 0, 0);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      const int j = j0 + 2 * i;
      if (j < 9) {
#pragma unroll
        for (int r = 0; r < 4; ++r) s_w[(16 * j + 4 * lk + r) * DB_PS + pxs + li] = acc[i][r];
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int cc = cl + 8 * q, ci = c0 + cc;
      if (ci >= Cin) continue;
      const float* pl = img + (size_t)ci * HW;
      float* gpl = gin ? gin + ((size_t)n * Cin + ci) * HW : nullptr;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int4 ix = s_idx[t * DB_TP + px];
        const float2 fr = s_fr[t * DB_TP + px];
        const float g = s_w[(9 * cc + t) * DB_PS + px];
        const float lh = fr.x, lw = fr.y, uh = 1.0f - lh, uw = 1.0f - lw;
        if (gpl) {
          if (ix.x >= 0) atomicAdd(gpl + ix.x, uh * uw * g);
          if (ix.y >= 0) atomicAdd(gpl + ix.y, uh * lw * g);
          if (ix.z >= 0) atomicAdd(gpl + ix.z, lh * uw * g);
          if (ix.w >= 0) atomicAdd(gpl + ix.w, lh * lw * g);
        }
        if (goff) {
          const float v00 = ix.x >= 0 ? pl[ix.x] : 0.f, v01 = ix.y >= 0 ? pl[ix.y] : 0.f;
          const float v10 = ix.z >= 0 ? pl[ix.z] : 0.f, v11 = ix.w >= 0 ? pl[ix.w] : 0.f;
          dh[t] += g * (uw * (v10 - v00) + lw * (v11 - v01));
          dw[t] += g * (uh * (v01 - v00) + lh * (v11 - v10));
        }
      }
    }
  }
  if (!goff) return;                                     // (uniform)
  __syncthreads();
  float* s_red = s_w;                                    // [8 lanes][18][32]
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    s_red[(cl * 18 + t) * DB_TP + px] = dh[t];
    s_red[(cl * 18 + 9 + t) * DB_TP + px] = dw[t];
  }
  __syncthreads();
  if (SHARED) {
    if (tid < 2 * DB_TP) {
      const int comp = tid >> 5, p = p0 + px;
      float sum = 0.f;
      for (int t = 0; t < 9; ++t) {
        float st = 0.f;
        for (int c = 0; c < 8; ++c) st += s_red[(c * 18 + 9 * comp + t) * DB_TP + px];
        sum += st;
      }
      if (p < HW) goff[((size_t)n * 2 + comp) * HW + p] = sum;
    }
  } else {
    for (int e = tid; e < 18 * DB_TP; e += 256) {
      const int row = e >> 5, q = e & 31, p = p0 + q;
      float st = 0.f;
      for (int c = 0; c < 8; ++c) st += s_red[(c * 18 + row) * DB_TP + q];
      const int ch = row < 9 ? 2 * row : 2 * (row - 9) + 1;
      if (p < HW) goff[((size_t)n * 18 + ch) * HW + p] = st;
    }
  }
}

template <bool SHARED>
__global__ __launch_bounds__(256) void k_dconv_bwd_weight(const float* __restrict__ go, const float* __restrict__ in,
                                                          const float* __restrict__ off, int N, int Cin, int H, int W,
                                                          int Cout, int tiles, int per, float* __restrict__ ws) {
  __shared__ int4 s_idx[9 * DB_TP];
  __shared__ float4 s_bw[9 * DB_TP];
  __shared__ float s_go[DB_CO][DB_TS];
  __shared__ float s_col[DB_KC][DB_TS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c0 = blockIdx.x * DB_CC, co0 = blockIdx.y * DB_CO, part = blockIdx.z;
  const int HW = H * W, K = 9 * Cin;
  const int total = N * tiles;
  const int t_lo = part * per, t_hi = min(total, t_lo + per);
  const int li = lane & 15, lk = lane >> 4;
  const bool active = co0 + 16 * wv < Cout;              // (wave-uniform)
  f32x4 acc[9];
#pragma unroll
  for (int j = 0; j < 9; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int tile = t_lo; tile < t_hi; ++tile) {
    const int n = tile / tiles, p0 = (tile - n * tiles) * DB_TP;
    const float* img = in + (size_t)n * Cin * HW;
    __syncthreads();                                     // the previous tile has been read by every wave
    for (int e = tid; e < 9 * DB_TP; e += 256) {
      int4 ix;
      float2 fr;
      tap_entry<SHARED>(off, n, e / DB_TP, p0 + (e % DB_TP), H, W, HW, ix, fr);
      const float lh = fr.x, lw = fr.y, uh = 1.0f - lh, uw = 1.0f - lw;
      s_idx[e] = ix;
      s_bw[e] = float4{uh * uw, uh * lw, lh * uw, lh * lw};
    }
    for (int e = tid; e < DB_CO * DB_TP; e += 256) {
      const int row = e >> 5, q = e & 31, co = co0 + row, p = p0 + q;
      s_go[row][q] = (co < Cout && p < HW) ? go[((size_t)n * Cout + co) * HW + p] : 0.f;
    }
    __syncthreads();
#pragma unroll 6
    for (int j = 0; j < DB_KC * DB_TP / 256; ++j) {
      const int r = (tid >> 5) + 8 * j, cc = r / 9, t = r - 9 * cc, ci = c0 + cc;
      const int4 ix = s_idx[t * DB_TP + (tid & 31)];
      const float4 bw = s_bw[t * DB_TP + (tid & 31)];
      float v = 0.f;
      if (ci < Cin) {
        const float* pl = img + (size_t)ci * HW;
        const float v0 = ix.x >= 0 ? pl[ix.x] : 0.f, v1 = ix.y >= 0 ? pl[ix.y] : 0.f;
        const float v2 = ix.z >= 0 ? pl[ix.z] : 0.f, v3 = ix.w >= 0 ? pl[ix.w] : 0.f;
        v = bw.x * v0 + bw.y * v1 + bw.z * v2 + bw.w * v3;   // the forward's column element, bit for bit
      }
      s_col[r][tid & 31] = v;
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int s = 0; s < DB_TP / 4; ++s) {
        const float a = s_go[16 * wv + li][4 * s + lk];
#pragma unroll
        for (int j = 0; j < 9; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, s_col[16 * j + li][4 * s + lk], acc[j], 0, 0, 0);
      }
    }
  }
  // every (part, co, k) of the workspace is written by exactly one workgroup (zeros for an empty pixel range)
  float* o = ws + (size_t)part * Cout * K;
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    const int k = 9 * c0 + 16 * j + li;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * wv + 4 * lk + r;
      if (co < Cout && k < K) o[(size_t)co * K + k] = acc[j][r];
    }
  }
}

__global__ __launch_bounds__(256) void k_dconv_bwd_wreduce(const float* __restrict__ ws, int parts, size_t CK,
                                                           float* __restrict__ gw) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= CK) return;
  float s = 0.f;
  for (int p = 0; p < parts; ++p) s += ws[(size_t)p * CK + i];
  gw[i] = s;
}

__global__ __launch_bounds__(256) void k_dconv_bwd_bias(const float* __restrict__ go, int N, int Cout, int HW,
                                                        float* __restrict__ gb) {
  __shared__ float s[256];
  const int co = blockIdx.x, tid = threadIdx.x;
  float a = 0.f;
  for (int n = 0; n < N; ++n) {
    const float* g = go + ((size_t)n * Cout + co) * HW;
    for (int p = tid; p < HW; p += 256) a += g[p];
  }
  s[tid] = a;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) s[tid] += s[tid + h];
    __syncthreads();
  }
  if (tid == 0) gb[co] = s[0];
}

}  // namespace acfm

using namespace acfm;

// pixel ranges of the weight gradient: enough workgroups for the chip, never more ranges than pixel tiles
static int wgrad_parts(int N, int Cin, int H, int W, int Cout) {
  const long total = (long)((H * W + DB_TP - 1) / DB_TP) * N;
  const long tiles_out = (long)((Cin + DB_CC - 1) / DB_CC) * ((Cout + DB_CO - 1) / DB_CO);
  long parts = (1024 + tiles_out - 1) / tiles_out;
  if (parts > total) parts = total;
  if (parts > 1024) parts = 1024;
  return parts < 1 ? 1 : (int)parts;
}

static bool dconv_bwd_args_ok(int N, int Cin, int H, int W, int Cout) {
  if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return false;
  // plane offsets and k are ints; grids: pixel tiles x images in x, channel chunks in x / y (65535 in y)
  if ((size_t)H * W > 0x7fffffffull - DB_TP || (size_t)Cin * 9 > 0x7fffffffull || Cout > 16 * 65535 ||
      ((size_t)H * W + DB_TP - 1) / DB_TP * (size_t)N > 0x7fffffffull)
    return false;
  return true;
}

extern "C" size_t acfm_deform_conv2d_backward_workspace_bytes(int N, int Cin, int H, int W, int Cout) {
  if (!dconv_bwd_args_ok(N, Cin, H, W, Cout)) return 0;
  return sizeof(float) * (size_t)wgrad_parts(N, Cin, H, W, Cout) * (size_t)Cout * 9 * (size_t)Cin;
}

extern "C" int acfm_deform_conv2d_backward(const float* grad_out, const float* input, const float* offset,
                                           const float* weight, int N, int Cin, int H, int W, int Cout,
                                           int shared_offset, float* grad_input, float* grad_offset, float* grad_weight,
                                           float* grad_bias, void* ws, size_t ws_bytes, void* stream) {
  if (!grad_out || !input || !offset || !weight || !dconv_bwd_args_ok(N, Cin, H, W, Cout)) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int tiles = (H * W + DB_TP - 1) / DB_TP, HW = H * W;
  if (grad_weight) {
    if (!ws) return ACFM_E_BADARG;
    if (ws_bytes < acfm_deform_conv2d_backward_workspace_bytes(N, Cin, H, W, Cout)) return ACFM_E_WORKSPACE;
  }
  if (grad_input || grad_offset) {
    if (grad_input && zero_async(grad_input, sizeof(float) * (size_t)N * Cin * HW, st) != ACFM_OK) return ACFM_E_LAUNCH;
    const dim3 grid((unsigned)((long)tiles * N));
    if (shared_offset)
      hipLaunchKernelGGL((k_dconv_bwd_data<true>), grid, dim3(256), 0, st, grad_out, input, offset, weight, Cin, H, W,
                         Cout, tiles, grad_input, grad_offset);
    else
      hipLaunchKernelGGL((k_dconv_bwd_data<false>), grid, dim3(256), 0, st, grad_out, input, offset, weight, Cin, H, W,
                         Cout, tiles, grad_input, grad_offset);
  }
  if (grad_weight) {
    const int parts = wgrad_parts(N, Cin, H, W, Cout);
    const int per = (int)(((long)tiles * N + parts - 1) / parts);
    const dim3 grid((unsigned)((Cin + DB_CC - 1) / DB_CC), (unsigned)((Cout + DB_CO - 1) / DB_CO), (unsigned)parts);
    if (shared_offset)
      hipLaunchKernelGGL((k_dconv_bwd_weight<true>), grid, dim3(256), 0, st, grad_out, input, offset, N, Cin, H, W, Cout,
                         tiles, per, (float*)ws);
    else
      hipLaunchKernelGGL((k_dconv_bwd_weight<false>), grid, dim3(256), 0, st, grad_out, input, offset, N, Cin, H, W, Cout,
                         tiles, per, (float*)ws);
    const size_t CK = (size_t)Cout * 9 * Cin;
    hipLaunchKernelGGL(k_dconv_bwd_wreduce, dim3((unsigned)((CK + 255) / 256)), dim3(256), 0, st, (const float*)ws, parts,
                       CK, grad_weight);
  }
  if (grad_bias)
    hipLaunchKernelGGL(k_dconv_bwd_bias, dim3((unsigned)Cout), dim3(256), 0, st, grad_out, N, Cout, HW, grad_bias);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}
