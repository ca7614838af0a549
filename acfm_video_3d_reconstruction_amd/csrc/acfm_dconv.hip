// Deformable convolution of the frozen optical-flow network (torchvision.ops.DeformConv2d as MaskFlownet.py:36-37,
// 488-492, 558-640 uses it: 3x3, stride 1, padding 1, dilation 1, one group, one offset group, no mask), forward only:
//   out[n,co,y,x] = bias[co] + sum_{ci,t} weight[co,ci,t] * S(input[n,ci], y + ky - 1 + off[n,2t,y,x], x + kx - 1 + off[n,2t+1,y,x])
// with t = 3 ky + kx and S the bilinear sample that is 0 at or beyond one pixel outside the map.
//
// torchvision writes the sampled columns [Cin*9, H*W] to device memory and runs a GEMM over them.  Here the GEMM
// out[co, p] = sum_k W[co, k] col[k, p] (k = 9 ci + t, exactly the order weight [Cout,Cin,3,3] is stored in) is tiled
// as DC_TP pixels x 16 NCO output channels per 256-thread workgroup, and the columns exist only as one chunk of DC_CC
// input channels (DC_KC = 9 DC_CC rows) in LDS:
//   * the corner indices and the bilinear weights of a (tap, pixel) pair do not depend on the channel: the workgroup
//     computes them once into an LDS table (9 DC_TP entries of 4 indices + 4 weights);
//   * per chunk every thread gathers the 4 corners of 9 column elements into registers and reads its share of the
//     weight tile (rows of 9 DC_CC consecutive floats of `weight` as it lies in memory: no repacked copy anywhere);
//     both are issued BEFORE the matrix-core pass over the previous chunk, so the gather latency hides behind it;
//   * the four waves then run v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered FMA chain) over the chunk: wave w owns the
//     pixel half w & 1 and the 16-channel subtiles (w >> 1) + 2 j, so one column operand feeds all its accumulators.
// Nothing is split along k and nothing is added atomically: the result is bit-reproducible, and the shared-offset
// form (every tap reads channels 0, 1 of a two-channel offset: MaskFlownet's repeat_interleave(flow.unsqueeze(1), 9, 1)
// without the copy) is the same kernel with another offset address, hence the same bits.
// Small maps have few pixel tiles (6x12: 3 per image); the launch then narrows the channel tile (64 -> 32 -> 16) until
// there is a workgroup per compute unit: the split is over Cout, every workgroup still runs the whole reduction.
#include "acfm_common.h"

namespace acfm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DC_TP = 32;            // pixels per workgroup (consecutive in the flattened map of one image)
constexpr int DC_CC = 8;             // input channels per LDS chunk
constexpr int DC_KC = 9 * DC_CC;     // rows of the column chunk = k steps per chunk (a multiple of the MFMA's 4)
constexpr int DC_EPT = DC_KC * DC_TP / 256;   // column elements per thread and chunk
// LDS row strides in floats, chosen for conflict-free ds_read_b32 of the MFMA operands (32 banks, lanes 0-31 and 32-63
// are served separately): the column operand reads [k + (l >> 4)][l & 15] -- 48 = 16 mod 32 puts lanes 16-31 on the
// other half of the banks; the weight operand reads [l & 15][k + (l >> 4)] -- 74 = 2 * 37 spreads the 16 rows over the
// even banks and the next k over the odd ones.
constexpr int DC_CS = 48;
constexpr int DC_WS = DC_KC + 2;
static_assert(DC_KC % 4 == 0 && DC_EPT * 256 == DC_KC * DC_TP && DC_TP == 32, "tile constants");

template <bool SHARED, int NCO>
__global__ __launch_bounds__(256) void k_dconv_fwd(const float* __restrict__ in, const float* __restrict__ off,
                                                   const float* __restrict__ wgt, const float* __restrict__ bias,
                                                   int Cin, int H, int W, int Cout, int tiles,
                                                   float* __restrict__ out) {
  constexpr int TCO = 16 * NCO;                        // output channels per workgroup
  constexpr int WEL = (TCO * DC_KC + 255) / 256;       // weight elements per thread and chunk
  constexpr int TPW = (2 * NCO + 3) / 4;               // 16x16 tiles per wave (2 NCO tiles over 4 waves)
  __shared__ int4 s_idx[9 * DC_TP];                    // per (tap, pixel): plane offsets of the 4 corners, -1 = outside
  __shared__ float4 s_bw[9 * DC_TP];                   // and their bilinear weights
  __shared__ float s_col[DC_KC][DC_CS];
  __shared__ float s_w[TCO][DC_WS];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = blockIdx.x / tiles, p0 = (blockIdx.x % tiles) * DC_TP;
  const int co0 = blockIdx.y * TCO;
  const int HW = H * W, K = 9 * Cin;
  const float* img = in + (size_t)n * Cin * HW;

  for (int e = tid; e < 9 * DC_TP; e += 256) {
    const int t = e / DC_TP, p = p0 + (e % DC_TP);
    int4 ix = {-1, -1, -1, -1};
    float4 bw = {0.f, 0.f, 0.f, 0.f};
    if (p < HW) {
      const int y = p / W, x = p - y * W, ky = t / 3, kx = t - 3 * ky;
      const float* o = off + (size_t)n * (SHARED ? 2 : 18) * HW + (SHARED ? 0 : (size_t)(2 * t) * HW) + p;
      const float h = (float)(y - 1 + ky) + o[0];
      const float w = (float)(x - 1 + kx) + o[HW];
      if (h > -1.0f && h < (float)H && w > -1.0f && w < (float)W) {   // (false for NaN as well: nothing is indexed)
        const float hf = floorf(h), wf = floorf(w);
        const int hl = (int)hf, wl = (int)wf, hh = hl + 1, wh = wl + 1;
        const float lh = h - hf, lw = w - wf, uh = 1.0f - lh, uw = 1.0f - lw;
        if (hl >= 0 && wl >= 0) ix.x = hl * W + wl;
        if (hl >= 0 && wh <= W - 1) ix.y = hl * W + wh;
        if (hh <= H - 1 && wl >= 0) ix.z = hh * W + wl;
        if (hh <= H - 1 && wh <= W - 1) ix.w = hh * W + wh;
        bw = float4{uh * uw, uh * lw, lh * uw, lh * lw};
      }
    }
    s_idx[e] = ix;
    s_bw[e] = bw;
  }
  __syncthreads();

  // the chunk in flight: 4 corner values per column element, and this thread's share of the weight tile
  float cv[DC_EPT][4], wr[WEL];
  // Loads are unconditional (a corner outside the map, or a channel past the last, reads element 0 of a plane that
  // exists): no branch per load, all of a chunk's loads in flight at once.  commit() drops what must not count.
  auto fetch = [&](int c0) {
#pragma unroll
    for (int j = 0; j < DC_EPT; ++j) {
      const int r = (tid >> 5) + 8 * j, cc = r / 9, t = r - 9 * cc;
      const int4 ix = s_idx[t * DC_TP + (tid & 31)];
      const float* pl = img + (size_t)min(c0 + cc, Cin - 1) * HW;
      cv[j][0] = pl[max(ix.x, 0)];
      cv[j][1] = pl[max(ix.y, 0)];
      cv[j][2] = pl[max(ix.z, 0)];
      cv[j][3] = pl[max(ix.w, 0)];
    }
#pragma unroll
    for (int j = 0; j < WEL; ++j) {
      const int e = tid + 256 * j, row = e / DC_KC, k = 9 * c0 + (e - row * DC_KC), co = co0 + row;
      const float v = wgt[(size_t)min(co, Cout - 1) * K + min(k, K - 1)];
      wr[j] = (row < TCO && co < Cout && k < K) ? v : 0.f;
    }
  };
  auto commit = [&](int c0) {
#pragma unroll
    for (int j = 0; j < DC_EPT; ++j) {
      const int r = (tid >> 5) + 8 * j, cc = r / 9, t = r - 9 * cc;
      const int4 ix = s_idx[t * DC_TP + (tid & 31)];
      const float4 bw = s_bw[t * DC_TP + (tid & 31)];
      const bool ok = c0 + cc < Cin;
      const float v0 = (ok && ix.x >= 0) ? cv[j][0] : 0.f, v1 = (ok && ix.y >= 0) ? cv[j][1] : 0.f;
      const float v2 = (ok && ix.z >= 0) ? cv[j][2] : 0.f, v3 = (ok && ix.w >= 0) ? cv[j][3] : 0.f;
      s_col[r][tid & 31] = bw.x * v0 + bw.y * v1 + bw.z * v2 + bw.w * v3;
    }
#pragma unroll
    for (int j = 0; j < WEL; ++j) {
      const int e = tid + 256 * j, row = e / DC_KC;
      if (row < TCO) s_w[row][e - row * DC_KC] = wr[j];
    }
  };

  f32x4 acc[TPW];
#pragma unroll
  for (int j = 0; j < TPW; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int li = lane & 15, lk = lane >> 4;
  const int pxs = (wv & 1) * 16, cs0 = wv >> 1;          // this wave's pixel half and first channel subtile
  const bool active = cs0 < NCO && co0 + 16 * cs0 < Cout;   // (with one subtile per workgroup two waves only gather)
  static_assert(TPW == 1 || 2 * (TPW - 1) + 1 < NCO, "every further subtile of a wave lies inside the tile");

  fetch(0);
  for (int c0 = 0; c0 < Cin; c0 += DC_CC) {
    __syncthreads();                                     // the previous chunk has been read by every wave
    commit(c0);
    __syncthreads();
    if (c0 + DC_CC < Cin) fetch(c0 + DC_CC);
    // all DC_KC rows every time (rows past the last channel hold zeros on both sides): a constant trip count lets the
    // operand reads of the whole chunk be issued ahead of the MFMAs that consume them.  A second subtile past Cout
    // multiplies zero rows of s_w and is not stored.
    if (active) {                                        // (wave-uniform)
#pragma unroll
      for (int s = 0; s < DC_KC / 4; ++s) {
        const float b = s_col[4 * s + lk][pxs + li];
#pragma unroll
        for (int j = 0; j < TPW; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_w[16 * (cs0 + 2 * j) + li][4 * s + lk], b, acc[j], 0, 0, 0);
      }
    }
  }

  const int p = p0 + pxs + li;
  if (p >= HW) return;
#pragma unroll
  for (int j = 0; j < TPW; ++j) {
    const int cs = cs0 + 2 * j;
    if (cs >= NCO) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int co = co0 + 16 * cs + 4 * lk + r;
      if (co < Cout) out[((size_t)n * Cout + co) * HW + p] = bias ? acc[j][r] + bias[co] : acc[j][r];
    }
  }
}

}  // namespace acfm

using namespace acfm;

// Refusals of the forward: plane offsets and k are ints; the grid's x is pixel tiles x images, its y channel tiles of at
// least 16.
static bool dconv_fwd_args_ok(int N, int Cin, int H, int W, int Cout) {
  if (N <= 0 || Cin <= 0 || H <= 0 || W <= 0 || Cout <= 0) return false;
  if ((size_t)H * W > 0x7fffffffull - DC_TP || (size_t)Cin * 9 > 0x7fffffffull || Cout > 16 * 65535 ||
      ((size_t)H * W + DC_TP - 1) / DC_TP * (size_t)N > 0x7fffffffull)
    return false;
  return true;
}

// the widest channel tile that still leaves a workgroup per compute unit (256 of them); never wider than Cout needs
static int dconv_channel_tile(int N, int H, int W, int Cout) {
  const long px_wgs = (long)((H * W + DC_TP - 1) / DC_TP) * N;
  int tco = 64;
  while (tco > 16 && (tco / 2 >= Cout || px_wgs * ((Cout + tco - 1) / tco) < 256)) tco >>= 1;
  return tco;
}

extern "C" int acfm_deform_conv2d_channel_tile(int N, int H, int W, int Cout) {
  return dconv_fwd_args_ok(N, 1, H, W, Cout) ? dconv_channel_tile(N, H, W, Cout) : 0;
}

template <bool SHARED>
static void launch_dconv(const float* in, const float* off, const float* wgt, const float* bias, int N, int Cin, int H,
                         int W, int Cout, float* out, hipStream_t st) {
  const int tiles = (H * W + DC_TP - 1) / DC_TP;
  const long px_wgs = (long)tiles * N;
  const int tco = dconv_channel_tile(N, H, W, Cout);
  const dim3 grid((unsigned)px_wgs, (unsigned)((Cout + tco - 1) / tco));
  if (tco == 64)
    hipLaunchKernelGGL((k_dconv_fwd<SHARED, 4>), grid, dim3(256), 0, st, in, off, wgt, bias, Cin, H, W, Cout, tiles, out);
  else if (tco == 32)
    hipLaunchKernelGGL((k_dconv_fwd<SHARED, 2>), grid, dim3(256), 0, st, in, off, wgt, bias, Cin, H, W, Cout, tiles, out);
  else
    hipLaunchKernelGGL((k_dconv_fwd<SHARED, 1>), grid, dim3(256), 0, st, in, off, wgt, bias, Cin, H, W, Cout, tiles, out);
}

extern "C" int acfm_deform_conv2d_forward(const float* input, const float* offset, const float* weight,
                                          const float* bias, int N, int Cin, int H, int W, int Cout, int shared_offset,
                                          float* out, void* stream) {
  if (!input || !offset || !weight || !out || !dconv_fwd_args_ok(N, Cin, H, W, Cout)) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (shared_offset) launch_dconv<true>(input, offset, weight, bias, N, Cin, H, W, Cout, out, st);
  else launch_dconv<false>(input, offset, weight, bias, N, Cin, H, W, Cout, out, st);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}
