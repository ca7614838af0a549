// Reprojection-loss kernels for gfx950 (HBM-bound streaming reductions):
//   fused silhouette losses  <- loss_utils.l1_loss / iou / edt_loss   (loss_utils.py:18-32, 72-77, 245-253)
//   visible-vertex bitmap    <- loss_utils.bds_loss :214-224 / optical_flow_loss :432-443
//   boundary loss            <- loss_utils.bds_loss :204-237
//   boundary loss on a subset named by slot lists (acfm_sample.hip draws them) <- :211-213 + :226-237
#include "acfm_common.h"
#include "acfm_row_finish.h"

namespace acfm {

constexpr int LTPB = 256;
constexpr int PIX_PER_BLOCK = 2048;  // 8 px per thread: 2 x float4
// The two forward reductions take 8192 pixels per workgroup where that still leaves two workgroups for each of the
// chip's 256 CUs (N * ceil(HW / 8192) >= 512), else 2048.  The workgroups of a mesh meet in one ticket word: at 256^2
// the narrow form sends 32 of them there at about the same time, which cost k_mask_losses 9 us; with 8 the
// one-launch form is faster than fill + atomics (profiles/r04_loss_in_graph.txt).  Below the threshold the wide
// form would leave CUs without a workgroup, which costs more bandwidth than the tickets do.
constexpr int PIX_PER_BLOCK_WIDE = 8192;
static inline int fwd_pix_per_block(int N, int HW) {
  constexpr size_t CUS = 256;
  return (size_t)N * ((HW + PIX_PER_BLOCK_WIDE - 1) / PIX_PER_BLOCK_WIDE) >= 2 * CUS ? PIX_PER_BLOCK_WIDE : PIX_PER_BLOCK;
}

// A workgroup's run of at most 8192 consecutive floats as a raw buffer: a 16-byte load whose byte offset does not lie
// inside [0, bytes - 16] returns zeros and touches no memory.  (word 3: 32-bit data format, as for every untyped
// buffer access on gfx9)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t pixel_range(const float* base, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, (int)bytes, 0x00020000);
}
constexpr int OUT_OF_RANGE = 0x7ffffff0;   // a byte offset past every such range, and adding 15 to it does not wrap
__device__ __forceinline__ float4 load16_in_range(__amdgpu_buffer_rsrc_t r, int byte_offset) {
  typedef float f4 __attribute__((ext_vector_type(4)));
  const f4 v = __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_offset, 0, 0));
  return make_float4(v.x, v.y, v.z, v.w);
}

// out[n] = (sum|m-gt|/HW, sum m*gt, sum(m+gt-m*gt), sum edt*m/HW); one pass over the mask.
// (prediction n is compared with reference n % RB: the G camera hypotheses of a frame share the
// frame's ground truth, so the trainer's gt.repeat(G, ...) copies are never made)
// k_mask_losses's body for workgroup `blk` of mesh n also runs as a role of k_step_tail: mask_losses_block leaves the
// four waves' sums in s_red behind a barrier, mask_losses_value is what wave 0 hands to the finish in lane c < 4.
// The body is ONE text, acfm_loss_body_mask.inc, #included in the kernel and in mask_losses_block -- not a function
// that both call: called from the kernel, the function changed its register allocation and schedule, and its machine
// code is pinned (tools/isa_diff.py against the parent; DESIGN.md, "The step's tail in one launch").  One text under
// -ffp-contract=off: the same bits (tests/test_gpu_step_tail.py compares them).  (mask_losses_value the kernel does
// call: that leaves its machine code as it is.)
template <int PIX_FWD>
__device__ __forceinline__ void mask_losses_block(const float* __restrict__ mask, const float* __restrict__ gt,
                                                  const float* __restrict__ edt, int HW, int RB, int n, int blk,
                                                  float (&s_red)[4][4]) {
#include "acfm_loss_body_mask.inc"
}
__device__ __forceinline__ float mask_losses_value(const float (&s_red)[4][4], int HW) {
  const int tid = threadIdx.x;
  float v = 0.f;
  if (tid < 4) {
    v = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
    if (tid == 0 || tid == 3) v = v / (float)HW;
  }
  return v;
}
template <int PIX_FWD>
__global__ __launch_bounds__(LTPB) void k_mask_losses(const float* __restrict__ mask,
                                                      const float* __restrict__ gt,
                                                      const float* __restrict__ edt, int HW, int RB,
                                                      float* __restrict__ out, RowScratch sc) {
  __shared__ float s_red[4][4];
  const int n = blockIdx.y;
  const unsigned blk = blockIdx.x;
#include "acfm_loss_body_mask.inc"
  if (tid >= 64) return;
  const float v = mask_losses_value(s_red, HW);
  if (sc.tickets) row_finish<4>(sc, n, (int)gridDim.x, (int)blockIdx.x, v, out + 4 * (size_t)n);
  else if (tid < 4) atomicAdd(&out[4 * (size_t)n + tid], v);
}

// grad_mask = go0*sign(m-gt)/HW + go1*gt + go2*(1-gt) + go3*edt/HW
__global__ __launch_bounds__(LTPB) void k_mask_losses_bwd(const float* __restrict__ mask,
                                                          const float* __restrict__ gt,
                                                          const float* __restrict__ edt,
                                                          const float* __restrict__ go, int HW, int RB,
                                                          float* __restrict__ grad_mask) {
  const int n = blockIdx.y;
  const size_t base = (size_t)n * HW, rbase = (size_t)(n % RB) * HW;
  const float inv = 1.0f / (float)HW;
  const float g0 = go[4 * n] * inv, g1 = go[4 * n + 1], g2 = go[4 * n + 2], g3 = go[4 * n + 3] * inv;
  const int start = blockIdx.x * PIX_PER_BLOCK;
  const int end = min(start + PIX_PER_BLOCK, HW);
  auto one = [&](float m, float g, float e) {
    const float df = m - g;
    const float sgn = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
    return g0 * sgn + g1 * g + g2 * (1.0f - g) + g3 * e;
  };
  if ((HW & 3) == 0) {   // 16-byte loads and stores
    for (int i = start + threadIdx.x * 4; i < end; i += LTPB * 4) {
      const float4 m = *reinterpret_cast<const float4*>(mask + base + i);
      float4 g = make_float4(0, 0, 0, 0), e = make_float4(0, 0, 0, 0);
      if (gt) g = *reinterpret_cast<const float4*>(gt + rbase + i);
      if (edt) e = *reinterpret_cast<const float4*>(edt + rbase + i);
      *reinterpret_cast<float4*>(grad_mask + base + i) =
          make_float4(one(m.x, g.x, e.x), one(m.y, g.y, e.y), one(m.z, g.z, e.z), one(m.w, g.w, e.w));
    }
    return;
  }
  for (int i = start + threadIdx.x; i < end; i += LTPB) {
    const float m = mask[base + i], g = gt ? gt[rbase + i] : 0.f, e = edt ? edt[rbase + i] : 0.f;
    grad_mask[base + i] = one(m, g, e);
  }
}

// masked texture MSE (multiframe/main.py:655-662): per mesh mean over (3,H,W) of
// (tex*m - img*m)^2; the workgroups' sums are added by row_finish (or, without scratch, one atomic per workgroup).
// (tex_mse_block: k_tex_mse's body for workgroup `blk` of mesh n up to the four waves' sums in s_red, for k_step_tail.
// One text, acfm_loss_body_tex_mse.inc, included in both for the reason given at mask_losses_block.)
template <int PIX_FWD>
__device__ __forceinline__ void tex_mse_block(const float* __restrict__ tex, const float* __restrict__ img,
                                              const float* __restrict__ m, int HW, int RB, int n, int blk,
                                              float (&s_red)[4]) {
#include "acfm_loss_body_tex_mse.inc"
}
template <int PIX_FWD>
__global__ __launch_bounds__(LTPB) void k_tex_mse(const float* __restrict__ tex,
                                                  const float* __restrict__ img,
                                                  const float* __restrict__ m, int HW, int RB,
                                                  float* __restrict__ out, RowScratch sc) {
  __shared__ float s_red[4];
  const int n = blockIdx.y;
  const unsigned blk = blockIdx.x;
#include "acfm_loss_body_tex_mse.inc"
  if (tid >= 64) return;
  const float v = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (3.0f * (float)HW);
  if (sc.tickets) row_finish<1>(sc, n, (int)gridDim.x, (int)blockIdx.x, v, out + n);
  else if (tid == 0) atomicAdd(&out[n], v);
}

__global__ __launch_bounds__(LTPB) void k_tex_mse_bwd(const float* __restrict__ tex,
                                                      const float* __restrict__ img,
                                                      const float* __restrict__ m,
                                                      const float* __restrict__ go, int HW, int RB,
                                                      float* __restrict__ gtex) {
  const int n = blockIdx.y;
  const size_t b3 = (size_t)n * 3 * HW, r3 = (size_t)(n % RB) * 3 * HW, b1 = (size_t)(n % RB) * HW;
  const float w = go[n] * 2.0f / (3.0f * (float)HW);
  const int start = blockIdx.x * PIX_PER_BLOCK;
  const int end = min(start + PIX_PER_BLOCK, HW);
  if ((HW & 3) == 0) {   // 16-byte loads and stores
    for (int i = start + threadIdx.x * 4; i < end; i += LTPB * 4) {
      const float4 mk = *reinterpret_cast<const float4*>(m + b1 + i);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const size_t o = b3 + (size_t)c * HW + i;
        const float4 t = *reinterpret_cast<const float4*>(tex + o);
        const float4 g = *reinterpret_cast<const float4*>(img + r3 + (size_t)c * HW + i);
        *reinterpret_cast<float4*>(gtex + o) =
            make_float4(w * (t.x * mk.x - g.x * mk.x) * mk.x, w * (t.y * mk.y - g.y * mk.y) * mk.y,
                        w * (t.z * mk.z - g.z * mk.z) * mk.z, w * (t.w * mk.w - g.w * mk.w) * mk.w);
      }
    }
    return;
  }
  for (int i = start + threadIdx.x; i < end; i += LTPB) {
    const float mk = m[b1 + i];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const size_t o = b3 + (size_t)c * HW + i;
      gtex[o] = w * (tex[o] * mk - img[r3 + (size_t)c * HW + i] * mk) * mk;
    }
  }
}

__global__ void k_visible(const int64_t* __restrict__ p2f, const int64_t* __restrict__ faces, int V,
                          int F, int HW, int K, uint8_t* __restrict__ vis) {
  const int n = blockIdx.y;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const int64_t fp = p2f[((size_t)n * HW + p) * K];
  if (fp < 0) return;
  int f = (int)(fp - (int64_t)n * F);
  f = min(max(f, 0), F - 1);
  const int64_t* fi = faces + ((size_t)n * F + f) * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const int v = min(max((int)fi[j], 0), V - 1);
    vis[(size_t)n * V + v] = 1;
  }
}

// One workgroup = 64 boundary points x all vertices: its four waves search a quarter of the vertices
// each (the search is a chain of dependent compare-selects per point: one wave per SIMD left the
// chip idle for 20 us) and wave 0 merges the four partial minima in vertex order, so the first
// nearest vertex wins exactly as in a single ascending scan.
// Only VISIBLE vertices are searched (half of a closed mesh is never seen): every wave stages its own quarter
// straight from memory into LDS, 64 vertices a round, keeping the visible ones packed in ascending order
// (ballot + prefix count) next to the index each came from.  A wave reads no other wave's quarter, so no
// workgroup barrier stands between the staging and the search.
// SEL: the lane's point is read through a slot list, sel [rows][S] (acfm_boundary_subset): lane p < S takes slot
// s = sel[((n % RB) % rows) S + p] of its reference's P points; s < 0 is an empty entry (adds 0, argmin -1).  argmin
// is then [N][S], and no gathered copy of the points exists.
// ONE text, in two fragments, for k_bds_loss, k_bds_loss_sel and k_step_tail's role bds_block<SEL>:
// acfm_loss_body_bds_search.inc up to the barrier behind the four waves' minima, acfm_loss_body_bds_merge.inc for wave
// 0 behind it.  The fragments are #included at each of the three places, not called: with the body in a common
// function (or the two kernels as one template) the compiler allocated the kernels' registers differently, and their
// machine code is pinned (tools/isa_diff.py against the parent; DESIGN.md, "The step's tail in one launch").  What
// differs stands in the including function: its LDS arrays, n and blk, SEL with sel / rows / S, where `contrib`
// lives, and every return.
// (bds_block: true in wave 0, which then carries the workgroup's sum in `contrib`.)
template <bool SEL>
__device__ __forceinline__ bool bds_block(const float* __restrict__ verts_xy, const float* __restrict__ bds,
                                          const uint8_t* __restrict__ vis, int V, int P, int RB, int n, int blk,
                                          int32_t* __restrict__ argmin, const int32_t* __restrict__ sel, int rows, int S,
                                          float (&s_best)[4][64], int (&s_bi)[4][64], float& contrib) {
#include "acfm_loss_body_bds_search.inc"
  if (wv != 0) return false;
#include "acfm_loss_body_bds_merge.inc"
  return true;
}
__global__ __launch_bounds__(LTPB) void k_bds_loss(const float* __restrict__ verts_xy,
                                                   const float* __restrict__ bds,
                                                   const uint8_t* __restrict__ vis, int V, int P, int RB,
                                                   float* __restrict__ loss, int32_t* __restrict__ argmin,
                                                   RowScratch sc) {
  __shared__ float s_best[4][64];
  __shared__ int s_bi[4][64];
  constexpr bool SEL = false;
  const int32_t* sel = nullptr;
  const int rows = 0, S = 0;
  const int n = blockIdx.y;
  const unsigned blk = blockIdx.x;
#include "acfm_loss_body_bds_search.inc"
  if (wv != 0) return;
  float contrib;
#include "acfm_loss_body_bds_merge.inc"
  if (sc.tickets) row_finish<1>(sc, n, (int)gridDim.x, (int)blockIdx.x, contrib, loss + n);
  else if (lane == 0) atomicAdd(&loss[n], contrib);
}

// k_bds_loss with the lane's point read through the slot list (SEL above).
__global__ __launch_bounds__(LTPB) void k_bds_loss_sel(const float* __restrict__ verts_xy,
                                                       const float* __restrict__ bds,
                                                       const uint8_t* __restrict__ vis, int V, int P, int RB,
                                                       float* __restrict__ loss, int32_t* __restrict__ argmin,
                                                       RowScratch sc, const int32_t* __restrict__ sel, int rows,
                                                       int S) {
  __shared__ float s_best[4][64];
  __shared__ int s_bi[4][64];
  constexpr bool SEL = true;
  const int n = blockIdx.y;
  const unsigned blk = blockIdx.x;
#include "acfm_loss_body_bds_search.inc"
  if (wv != 0) return;
  float contrib;
#include "acfm_loss_body_bds_merge.inc"
  if (sc.tickets) row_finish<1>(sc, n, (int)gridDim.x, (int)blockIdx.x, contrib, loss + n);
  else if (lane == 0) atomicAdd(&loss[n], contrib);
}

// One workgroup per mesh: the points' contributions are summed per vertex in LDS (P <= ~1000 points
// onto V vertices) and the whole [V,2] gradient row is stored, zeros included -- no global atomics
// (64 k scattered memory-side atomics took 13 us) and no zero fill of the output.
// (one text for both kernels, acfm_loss_body_bds_bwd.inc: two kernels that include it, not one template, for the
// reason given at the forward kernels)
__global__ __launch_bounds__(256) void k_bds_loss_bwd(const float* __restrict__ verts_xy,
                                                      const float* __restrict__ bds,
                                                      const int32_t* __restrict__ argmin,
                                                      const float* __restrict__ gl, int V, int P, int RB,
                                                      float* __restrict__ gv) {
  constexpr bool SEL = false;
  const int32_t* sel = nullptr;
  const int rows = 0, S = 0;
#include "acfm_loss_body_bds_bwd.inc"
}

// k_bds_loss_bwd over the entries of argmin [N][S]: entry p belongs to slot sel[((n % RB) % rows) S + p] (see
// k_bds_loss_sel).
__global__ __launch_bounds__(256) void k_bds_loss_sel_bwd(const float* __restrict__ verts_xy,
                                                          const float* __restrict__ bds,
                                                          const int32_t* __restrict__ argmin,
                                                          const float* __restrict__ gl, int V, int P, int RB,
                                                          float* __restrict__ gv, const int32_t* __restrict__ sel,
                                                          int rows, int S) {
  constexpr bool SEL = true;
#include "acfm_loss_body_bds_bwd.inc"
}

// ---- optical-flow loss (loss_utils.py:419-474), one workgroup per (clip, frame k >= 1) --------------
// per vertex: GT flow = nearest pixel of the frame's flow image at the projected vertex
// (grid_sample, mode nearest, align_corners False, zero padding), predicted flow = pixel
// displacement of the vertex between frame k-1 and k, both counted where the vertex is visible in
// frame k and the GT flow is non-zero;  loss[c,k-1] = sum |gt - pred|_1 / H / (count + 1).
// Where the GT flow of (clip c, frame k) comes from: flows holds `clips` clips of T frames (clip c reads c % clips:
// the G hypotheses of a clip share its data), frame k reads T-1-k if flip_t (main.py:680: torch.flip(flows, dims=[1])),
// and the value is multiplied by masks[(c % clips) T + k] at the same pixel if masks is given (main.py:680-681).
struct OfSrc {
  const float* flows;
  const float* masks;
  int clips, flip_t;
};
__device__ __forceinline__ bool of_term(const float* __restrict__ proj, const OfSrc& src,
                                        const uint8_t* __restrict__ vis, int c, int k, int v, int T, int V,
                                        int H, int W, float& dx, float& dy) {
  const size_t fk = (size_t)c * T + k;
  const float* pk = proj + (fk * V + v) * 3;
  const float* pp = proj + ((fk - 1) * V + v) * 3;
  const float x = pk[0], y = pk[1];
  const float ixf = rintf(((x + 1.0f) * (float)W - 1.0f) / 2.0f), iyf = rintf(((y + 1.0f) * (float)H - 1.0f) / 2.0f);
  float gx = 0.f, gy = 0.f;
  if (ixf >= 0.f && ixf <= (float)(W - 1) && iyf >= 0.f && iyf <= (float)(H - 1)) {
    const size_t cs = (size_t)(c % src.clips) * T;
    const size_t pixel = (size_t)(int)iyf * W + (int)ixf;
    const float* g = src.flows + ((cs + (src.flip_t ? T - 1 - k : k)) * H * (size_t)W + pixel) * 2;
    gx = g[0]; gy = g[1];
    if (src.masks) {
      const float m = src.masks[(cs + k) * H * (size_t)W + pixel];
      gx *= m; gy *= m;
    }
  }
  const bool keep = (fabsf(gx) + fabsf(gy) != 0.0f) && vis[fk * V + v] != 0;
  const float fw = (float)W;
  const float fpx = fw * (pp[0] + 1.0f) / 2.0f - fw * (x + 1.0f) / 2.0f;
  const float fpy = fw * (pp[1] + 1.0f) / 2.0f - fw * (y + 1.0f) / 2.0f;
  dx = gx - fpx; dy = gy - fpy;
  return keep;
}

__global__ __launch_bounds__(LTPB) void k_of_loss(const float* __restrict__ proj, OfSrc flows,
                                                  const uint8_t* __restrict__ vis, int T, int V, int H, int W,
                                                  float* __restrict__ loss, float* __restrict__ count) {
  __shared__ float s_red[4][2];
  const int k = blockIdx.x + 1, c = blockIdx.y, tid = threadIdx.x;
  float sum = 0.f, cnt = 0.f;
  for (int v = tid; v < V; v += LTPB) {
    float dx, dy;
    if (of_term(proj, flows, vis, c, k, v, T, V, H, W, dx, dy)) { sum += fabsf(dx) + fabsf(dy); cnt += 1.0f; }
  }
  sum = wave_sum(sum); cnt = wave_sum(cnt);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = sum; s_red[tid >> 6][1] = cnt; }
  __syncthreads();
  if (tid == 0) {
    const float s = s_red[0][0] + s_red[1][0] + s_red[2][0] + s_red[3][0];
    const float n = s_red[0][1] + s_red[1][1] + s_red[2][1] + s_red[3][1];
    loss[(size_t)c * (T - 1) + k - 1] = s / (float)H / (n + 1.0f);
    count[(size_t)c * (T - 1) + k - 1] = n;
  }
}

__global__ __launch_bounds__(LTPB) void k_of_loss_bwd(const float* __restrict__ proj, OfSrc flows,
                                                      const uint8_t* __restrict__ vis, const float* __restrict__ count,
                                                      const float* __restrict__ gl, int T, int V, int H, int W,
                                                      float* __restrict__ gproj) {
  const int k = blockIdx.y + 1, c = blockIdx.z;
  const int v = blockIdx.x * LTPB + threadIdx.x;
  if (v >= V) return;
  float dx, dy;
  if (!of_term(proj, flows, vis, c, k, v, T, V, H, W, dx, dy)) return;
  const size_t o = (size_t)c * (T - 1) + k - 1;
  // d|gt - pred| / d pred = -sign(gt - pred);  pred = pix[k-1] - pix[k],  pix = W (xy + 1) / 2
  const float g = gl[o] / (float)H / (count[o] + 1.0f) * (float)W / 2.0f;
  const float sx = dx > 0.f ? 1.f : (dx < 0.f ? -1.f : 0.f), sy = dy > 0.f ? 1.f : (dy < 0.f ? -1.f : 0.f);
  const size_t fk = (size_t)c * T + k;
  float* gk = gproj + (fk * V + v) * 3;
  float* gp = gproj + ((fk - 1) * V + v) * 3;
  atomicAdd(&gp[0], -sx * g); atomicAdd(&gp[1], -sy * g);
  atomicAdd(&gk[0], sx * g); atomicAdd(&gk[1], sy * g);
}

// total = (1/N) sum_n sum_t sum_c w[t][c] T_t[n,c]: the weighted sum of per-mesh loss terms and its mean
// over the batch (multiframe/main.py:716-746 without the hypothesis weights) as ONE launch each way
// instead of ~13 elementwise / reduction launches on 64-element vectors forward and as many backward.
struct CombArgs {
  const float* t[4];
  float* g[4];
  int cols[4];
  float w[4][4];
  int nterms;
};
__global__ __launch_bounds__(256) void k_combine(CombArgs a, int N, float* __restrict__ total) {
  __shared__ float s_red[4];
  float acc = 0.f;
  for (int n = threadIdx.x; n < N; n += 256)
    for (int t = 0; t < a.nterms; ++t)
      for (int c = 0; c < a.cols[t]; ++c)
        if (a.w[t][c] != 0.f) acc += a.w[t][c] * a.t[t][(size_t)n * a.cols[t] + c];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) total[0] = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (float)N;
}
__global__ __launch_bounds__(256) void k_combine_bwd(CombArgs a, int N, const float* __restrict__ go) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  const float g = go[0] / (float)N;
  for (int t = 0; t < a.nterms; ++t)
    if (a.g[t])
      for (int c = 0; c < a.cols[t]; ++c) a.g[t][(size_t)n * a.cols[t] + c] = a.w[t][c] * g;
}

// ---- the step's tail in one launch: boundary loss, silhouette losses, texture MSE and their weighted total ----------
// k_step_tail's grid is the workgroups of k_bds_loss[_sel], k_mask_losses and k_tex_mse one after the other (the
// boundary loss first: it is the chain of latencies, so it starts first); every workgroup runs the body of the kernel
// it stands for (bds_block, mask_losses_block, tex_mse_block) on the same pixel partition and finishes its row through
// the same tickets in the same order, so each term has the bits the separate launch gives.  A role with nb == 0 is
// absent.  The three launches were short for what they are, not for their bytes (ramp, a few dependent loads, ticket,
// drain): as roles of one grid those chains overlap.
// The total: a row that is finished is published (row_finish_published) and counted in one more ticket word,
// `done`, which wraps at rows = N x (roles present); the wave that counts the last row evaluates k_combine's
// expression on the finished rows -- the 256 threads of k_combine as four passes of its 64 lanes, added in
// k_combine's order -- reading every term with device-scope loads.  Terms that no role of this launch writes are
// read the same way (an earlier launch finished them).
struct TailBds {
  const float* verts_xy; const float* bds; const uint8_t* vis; const int32_t* sel;
  float* loss; int32_t* argmin; RowScratch sc;
  int V, P, RB, rows, S, nb;
};
struct TailMask {
  const float* mask; const float* gt; const float* edt;
  float* out; RowScratch sc;
  int HW, RB, nb, wide;
};
struct TailTex {
  const float* tex; const float* img; const float* mask;
  float* out; RowScratch sc;
  int HW, RB, nb, wide;
};
struct TailTotal {
  CombArgs a;
  float* total;        // nullptr: no total
  unsigned* done;      // one word, zero between launches
  unsigned rows;
};
__device__ __forceinline__ void tail_row_done(const TailTotal& t, int N) {
  const int lane = threadIdx.x & 63;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  unsigned ticket = 0u;
  if (lane == 0) ticket = atomicInc(t.done, t.rows - 1u);
  ticket = __shfl(ticket, 0, 64);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (ticket != t.rows - 1u) return;
  float s[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    float acc = 0.f;
    for (int n = w * 64 + lane; n < N; n += 256)
      for (int k = 0; k < t.a.nterms; ++k)
        for (int c = 0; c < t.a.cols[k]; ++c)
          if (t.a.w[k][c] != 0.f)
            acc += t.a.w[k][c] * __uint_as_float(__hip_atomic_load(
                                     reinterpret_cast<const unsigned*>(t.a.t[k]) + (size_t)n * t.a.cols[k] + c,
                                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    s[w] = wave_sum(acc);
  }
  if (lane == 0) t.total[0] = (s[0] + s[1] + s[2] + s[3]) / (float)N;
}
__global__ __launch_bounds__(LTPB) __attribute__((amdgpu_waves_per_eu(4))) void k_step_tail(TailBds B, TailMask M, TailTex T, TailTotal tot, int N) {
  __shared__ float s_best[4][64];
  __shared__ int s_bi[4][64];
  __shared__ float s_red4[4][4];
  __shared__ float s_red[4];
  const int tid = threadIdx.x;
  int b = blockIdx.x;
  bool finished;
  if (b < B.nb * N) {
    const int n = b / B.nb, blk = b - n * B.nb;
    float contrib;
    const bool wave0 = B.sel ? bds_block<true>(B.verts_xy, B.bds, B.vis, B.V, B.P, B.RB, n, blk, B.argmin, B.sel, B.rows,
                                               B.S, s_best, s_bi, contrib)
                             : bds_block<false>(B.verts_xy, B.bds, B.vis, B.V, B.P, B.RB, n, blk, B.argmin, nullptr, 0, 0,
                                                s_best, s_bi, contrib);
    if (!wave0) return;
    finished = row_finish_published<1>(B.sc, n, B.nb, blk, contrib, B.loss + n);
  } else if ((b -= B.nb * N) < M.nb * N) {
    const int n = b / M.nb, blk = b - n * M.nb;
    if (M.wide) mask_losses_block<PIX_PER_BLOCK_WIDE>(M.mask, M.gt, M.edt, M.HW, M.RB, n, blk, s_red4);
    else mask_losses_block<PIX_PER_BLOCK>(M.mask, M.gt, M.edt, M.HW, M.RB, n, blk, s_red4);
    if (tid >= 64) return;
    const float v = mask_losses_value(s_red4, M.HW);
    finished = row_finish_published<4>(M.sc, n, M.nb, blk, v, M.out + 4 * (size_t)n);
  } else {
    b -= M.nb * N;
    const int n = b / T.nb, blk = b - n * T.nb;
    if (T.wide) tex_mse_block<PIX_PER_BLOCK_WIDE>(T.tex, T.img, T.mask, T.HW, T.RB, n, blk, s_red);
    else tex_mse_block<PIX_PER_BLOCK>(T.tex, T.img, T.mask, T.HW, T.RB, n, blk, s_red);
    if (tid >= 64) return;
    const float v = (s_red[0] + s_red[1] + s_red[2] + s_red[3]) / (3.0f * (float)T.HW);
    finished = row_finish_published<1>(T.sc, n, T.nb, blk, v, T.out + n);
  }
  if (finished && tot.total) tail_row_done(tot, N);
}

// ---- total per hypothesis, softmax weighting over the hypotheses, weighted mean: one launch each way ---------
// multiframe/main.py:716-746.  One thread per frame n walks its G hypotheses; everything is summed in a fixed
// order (one workgroup), so the result is reproducible.
constexpr int HYP_MAX_TERMS = 8;
struct HypArgs {
  const float* t[HYP_MAX_TERMS];
  float* g[HYP_MAX_TERMS];
  float w[HYP_MAX_TERMS];
  float aux_w[HYP_MAX_TERMS];
  int aux_group[HYP_MAX_TERMS];   // -1, 0 or 1: which auxiliary sum the term also enters (with aux_w)
  int nterms;
};
__global__ __launch_bounds__(256) void k_hyp_total(HypArgs a, int G, int N, float* __restrict__ total,
                                                   float* __restrict__ probs, float* __restrict__ aux0,
                                                   float* __restrict__ aux1, float* __restrict__ out) {
  __shared__ float s_red[4][4 + HYP_MAX_TERMS];
  float acc_w = 0.f, acc_t = 0.f, acc_a0 = 0.f, acc_a1 = 0.f, acc_term[HYP_MAX_TERMS];
#pragma unroll
  for (int t = 0; t < HYP_MAX_TERMS; ++t) acc_term[t] = 0.f;
  for (int n = threadIdx.x; n < N; n += 256) {
    float lmin = __builtin_inff();
    for (int g = 0; g < G; ++g) {
      const size_t i = (size_t)g * N + n;
      float tot = 0.f, x0 = 0.f, x1 = 0.f;
#pragma unroll
      for (int t = 0; t < HYP_MAX_TERMS; ++t) {
        if (t >= a.nterms) break;
        const float v = a.t[t][i];
        tot += a.w[t] * v;
        acc_term[t] += v;
        if (a.aux_group[t] == 0) x0 += a.aux_w[t] * v;
        if (a.aux_group[t] == 1) x1 += a.aux_w[t] * v;
      }
      total[i] = tot;
      if (aux0) aux0[i] = x0;
      if (aux1) aux1[i] = x1;
      acc_t += tot; acc_a0 += x0; acc_a1 += x1;
      lmin = fminf(lmin, tot);
    }
    float den = 0.f;
    for (int g = 0; g < G; ++g) den += expf(-(total[(size_t)g * N + n] - lmin));   // softmax(-total) over g
    float wsum = 0.f;
    for (int g = 0; g < G; ++g) {
      const size_t i = (size_t)g * N + n;
      const float p = expf(-(total[i] - lmin)) / den;
      probs[i] = p;
      wsum += p * total[i];
    }
    acc_w += wsum;
  }
  // out: [0] weighted loss, [1] mean total, [2] mean aux0, [3] mean aux1, [4 + t] mean of term t
  float vals[4 + HYP_MAX_TERMS] = {acc_w, acc_t, acc_a0, acc_a1};
#pragma unroll
  for (int t = 0; t < HYP_MAX_TERMS; ++t) vals[4 + t] = acc_term[t];
#pragma unroll
  for (int k = 0; k < 4 + HYP_MAX_TERMS; ++k) {
    const float v = wave_sum(vals[k]);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6][k] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4 + HYP_MAX_TERMS) {
    const int k = threadIdx.x;
    const float v = s_red[0][k] + s_red[1][k] + s_red[2][k] + s_red[3][k];
    out[k] = v / (k == 0 ? (float)N : (float)N * (float)G);
  }
}
__global__ __launch_bounds__(256) void k_hyp_total_bwd(HypArgs a, int GN, int N, const float* __restrict__ go,
                                                       const float* __restrict__ probs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= GN) return;
  const float g = go[0] * probs[i] / (float)N;   // the probabilities carry no gradient (detached in the reference)
#pragma unroll
  for (int t = 0; t < HYP_MAX_TERMS; ++t) {
    if (t >= a.nterms) break;
    if (a.g[t]) a.g[t][i] = a.w[t] * g;
  }
}

// ---- texture temporal-consistency term (multiframe/main.py:705-711), as written there ---------------------------
// The atlases [B*T,F,R,R,3] are regrouped as [B,F,R,R,T,3], that buffer is RESHAPED to rows [-1,R,R] (the reference's
// own regrouping of the trailing (R,T,3) block; reproduced, not "fixed"), and the loss is the mean L2 norm over the
// last axis of the differences of neighbouring rows i, i+1.  X[m,i,j] below is element m R^2 + i R + j of the regrouped
// buffer; cyc_src maps it back to its place in the atlases.  Forward: one thread per (m, i) writes the norm and a
// partial sum per workgroup, a second small kernel adds the partials in order.  Backward: one thread per element
// (every atlas entry is written exactly once: no atomics, no zero fill).
struct CycDims { int B, T, F, R; };
// (index arithmetic in 32 bits whenever the atlas batch has fewer than 2^31 entries: the decode below is five
// divisions per element and 64-bit ones made these kernels 3x longer than the tensor traffic)
template <class I>
__device__ __forceinline__ I cyc_src(I q, const CycDims& d) {
  const I c = q % 3; q /= 3;
  const I t = q % (I)d.T; q /= (I)d.T;
  const I r2 = q % (I)d.R; q /= (I)d.R;
  const I r1 = q % (I)d.R; q /= (I)d.R;
  const I f = q % (I)d.F; q /= (I)d.F;
  const I b = q;
  return ((((b * (I)d.T + t) * (I)d.F + f) * (I)d.R + r1) * (I)d.R + r2) * 3 + c;
}
template <class I>
__global__ __launch_bounds__(256) void k_tex_cycle(const float* __restrict__ tex, CycDims d, size_t pairs,
                                                   float* __restrict__ norms, float* __restrict__ partial) {
  __shared__ float s_red[4];
  const I p = (I)blockIdx.x * 256 + threadIdx.x;   // pair (m, i), i < R - 1
  float nrm = 0.f;
  if ((size_t)p < pairs) {
    const I m = p / (I)(d.R - 1);
    const I i = p % (I)(d.R - 1);
    const I q0 = (m * (I)d.R + i) * (I)d.R;
    float acc = 0.f;
    for (int j = 0; j < d.R; ++j) {
      const float df = tex[cyc_src<I>(q0 + (I)j, d)] - tex[cyc_src<I>(q0 + (I)d.R + (I)j, d)];
      acc += df * df;
    }
    nrm = sqrtf(acc);
    norms[p] = nrm;
  }
  const float v = wave_sum(nrm);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) partial[blockIdx.x] = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
}
__global__ __launch_bounds__(256) void k_tex_cycle_finish(const float* __restrict__ partial, int nblocks, float scale,
                                                          float* __restrict__ out) {
  __shared__ float s_red[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < nblocks; i += 256) acc += partial[i];
  const float v = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) * scale;
}
template <class I>
__global__ __launch_bounds__(256) void k_tex_cycle_bwd(const float* __restrict__ tex, const float* __restrict__ norms,
                                                       const float* __restrict__ go, CycDims d, size_t total, float scale,
                                                       float* __restrict__ grad) {
  const I q = (I)blockIdx.x * 256 + threadIdx.x;   // element (m, i, j) of the regrouped buffer
  if ((size_t)q >= total) return;
  const I i = (q / (I)d.R) % (I)d.R;
  const I m = q / ((I)d.R * (I)d.R);
  const I src = cyc_src<I>(q, d);
  const float x = tex[src];
  float g = 0.f;
  if (i + 1 < (I)d.R) {         // pair (m, i): d norm / d x = (x - x_below) / norm
    const float n = norms[m * (I)(d.R - 1) + i];
    if (n > 0.f) g += (x - tex[cyc_src<I>(q + (I)d.R, d)]) / n;
  }
  if (i > 0) {                  // pair (m, i - 1): d norm / d x = -(x_above - x) / norm
    const float n = norms[m * (I)(d.R - 1) + i - 1];
    if (n > 0.f) g -= (tex[cyc_src<I>(q - (I)d.R, d)] - x) / n;
  }
  grad[src] = g * go[0] * scale;
}

// Scratch of the three per-mesh loss sums: `tickets`, one word per mesh, zero between launches; `partials`, [N][nblk][C]
// floats of any contents (sized for the most workgroups a launch of that shape can have).
static inline int loss_blocks(int which, int n) {
  return which == ACFM_LOSS_BDS ? (n + 63) / 64 : (n + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK;
}
static inline size_t loss_partial_floats(int which, int N, int n) {
  return (which == ACFM_LOSS_MASK ? 4 : 1) * (size_t)N * loss_blocks(which, n);
}
// -> ACFM_OK; both pointers null select the atomics form behind a zero fill (sc.tickets == nullptr)
static inline int row_scratch(int which, int N, int n, uint32_t* tickets, float* partials, size_t partial_floats,
                              RowScratch& sc) {
  sc.tickets = nullptr; sc.partials = nullptr;
  if (!tickets && !partials) return ACFM_OK;
  if (!tickets || !partials) return ACFM_E_BADARG;
  if (partial_floats < loss_partial_floats(which, N, n)) return ACFM_E_WORKSPACE;
  sc.tickets = tickets; sc.partials = partials;
  return ACFM_OK;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

size_t acfm_loss_partial_floats(int which, int N, int n) {
  if (which < ACFM_LOSS_MASK || which > ACFM_LOSS_BDS || N <= 0 || n <= 0) return 0;
  return loss_partial_floats(which, N, n);
}

int acfm_mask_losses(const float* mask, const float* gt, const float* edt, int N, int HW, int ref_batch,
                     float* out, uint32_t* tickets, float* partials, size_t partial_floats, void* stream) {
  if (!mask || !out || N <= 0 || N > 65535 || HW <= 0 || ref_batch <= 0 || N % ref_batch != 0) return ACFM_E_BADARG;
  RowScratch sc;
  if (const int rc = row_scratch(ACFM_LOSS_MASK, N, HW, tickets, partials, partial_floats, sc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!sc.tickets && zero_async(out, sizeof(float) * 4 * (size_t)N, st) != ACFM_OK) return ACFM_E_LAUNCH;
  const int ppb = fwd_pix_per_block(N, HW), chunks = (HW + ppb - 1) / ppb;
  ProfScope ps(ACFM_PROF_MASK_LOSS, st);
  if (ppb == PIX_PER_BLOCK_WIDE)
    hipLaunchKernelGGL(k_mask_losses<PIX_PER_BLOCK_WIDE>, dim3(chunks, N), dim3(LTPB), 0, st, mask, gt, edt, HW, ref_batch, out, sc);
  else
    hipLaunchKernelGGL(k_mask_losses<PIX_PER_BLOCK>, dim3(chunks, N), dim3(LTPB), 0, st, mask, gt, edt, HW, ref_batch, out, sc);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_mask_losses_backward(const float* mask, const float* gt, const float* edt,
                              const float* grad_out, int N, int HW, int ref_batch, float* grad_mask,
                              void* stream) {
  if (!mask || !grad_out || !grad_mask || N <= 0 || N > 65535 || HW <= 0 || ref_batch <= 0 || N % ref_batch != 0)
    return ACFM_E_BADARG;
  const int chunks = (HW + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK;
  ProfScope ps(ACFM_PROF_MASK_LOSS_BWD, (hipStream_t)stream);
  hipLaunchKernelGGL(k_mask_losses_bwd, dim3(chunks, N), dim3(LTPB), 0, (hipStream_t)stream, mask, gt,
                     edt, grad_out, HW, ref_batch, grad_mask);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_tex_mse(const float* tex, const float* img, const float* mask, int N, int HW, int ref_batch,
                 float* out, uint32_t* tickets, float* partials, size_t partial_floats, void* stream) {
  if (!tex || !img || !mask || !out || N <= 0 || N > 65535 || HW <= 0 || ref_batch <= 0 || N % ref_batch != 0)
    return ACFM_E_BADARG;
  RowScratch sc;
  if (const int rc = row_scratch(ACFM_LOSS_TEX_MSE, N, HW, tickets, partials, partial_floats, sc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!sc.tickets && zero_async(out, sizeof(float) * (size_t)N, st) != ACFM_OK) return ACFM_E_LAUNCH;
  const int ppb = fwd_pix_per_block(N, HW), chunks = (HW + ppb - 1) / ppb;
  ProfScope ps(ACFM_PROF_TEX_MSE, st);
  if (ppb == PIX_PER_BLOCK_WIDE)
    hipLaunchKernelGGL(k_tex_mse<PIX_PER_BLOCK_WIDE>, dim3(chunks, N), dim3(LTPB), 0, st, tex, img, mask, HW, ref_batch, out, sc);
  else
    hipLaunchKernelGGL(k_tex_mse<PIX_PER_BLOCK>, dim3(chunks, N), dim3(LTPB), 0, st, tex, img, mask, HW, ref_batch, out, sc);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_tex_mse_backward(const float* tex, const float* img, const float* mask, const float* grad_out,
                          int N, int HW, int ref_batch, float* grad_tex, void* stream) {
  if (!tex || !img || !mask || !grad_out || !grad_tex || N <= 0 || N > 65535 || HW <= 0 || ref_batch <= 0 ||
      N % ref_batch != 0)
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ACFM_PROF_TEX_MSE_BWD, st);
  hipLaunchKernelGGL(k_tex_mse_bwd, dim3((HW + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK, N), dim3(LTPB), 0, st,
                     tex, img, mask, grad_out, HW, ref_batch, grad_tex);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

static int fill_comb(CombArgs& a, const void* const* terms, void* const* grads, const int* cols,
                     const float* weights, int nterms) {
  if (!cols || !weights || nterms <= 0 || nterms > 4) return ACFM_E_BADARG;
  a.nterms = nterms;
  int o = 0;
  for (int t = 0; t < 4; ++t) {
    a.t[t] = nullptr; a.g[t] = nullptr; a.cols[t] = 0;
    for (int c = 0; c < 4; ++c) a.w[t][c] = 0.f;
    if (t >= nterms) continue;
    if (cols[t] <= 0 || cols[t] > 4) return ACFM_E_BADARG;
    a.cols[t] = cols[t];
    if (terms) { if (!terms[t]) return ACFM_E_BADARG; a.t[t] = (const float*)terms[t]; }
    if (grads) a.g[t] = (float*)grads[t];
    for (int c = 0; c < cols[t]; ++c) a.w[t][c] = weights[o++];
  }
  return ACFM_OK;
}

int acfm_combine_losses(const void* const* terms, const int* cols, const float* weights, int nterms, int N,
                        float* total, void* stream) {
  CombArgs a;
  if (!terms || !total || N <= 0 || fill_comb(a, terms, nullptr, cols, weights, nterms) != ACFM_OK)
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_combine, dim3(1), dim3(256), 0, (hipStream_t)stream, a, N, total);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

size_t acfm_step_losses_ws(int N, int HW_mask, int HW_tex, int S, size_t* ticket_words) {
  if (N <= 0 || HW_mask < 0 || HW_tex < 0 || S < 0) return 0;
  if (ticket_words) *ticket_words = 3 * (size_t)N + 1;
  return (HW_mask ? loss_partial_floats(ACFM_LOSS_MASK, N, HW_mask) : 0) +
         (HW_tex ? loss_partial_floats(ACFM_LOSS_TEX_MSE, N, HW_tex) : 0) + (S ? loss_partial_floats(ACFM_LOSS_BDS, N, S) : 0);
}

int acfm_step_losses_forward(const acfm_step_mask_job* mask, const acfm_step_tex_job* tex, const acfm_step_bds_job* bds,
                             const acfm_step_total_job* total, int N, uint32_t* tickets, float* partials,
                             size_t partial_floats, void* stream) {
  if ((!mask && !tex && !bds) || N <= 0 || N > 65535 || !tickets || !partials) return ACFM_E_BADARG;
  const int S = bds ? (bds->sel ? bds->S : bds->P) : 0;
  if (mask && (!mask->mask || !mask->out || mask->HW <= 0 || mask->ref_batch <= 0 || N % mask->ref_batch != 0))
    return ACFM_E_BADARG;
  if (tex && (!tex->tex || !tex->img || !tex->mask || !tex->out || tex->HW <= 0 || tex->ref_batch <= 0 ||
              N % tex->ref_batch != 0))
    return ACFM_E_BADARG;
  if (bds && (!bds->verts_xy || !bds->bds || !bds->vis || !bds->loss || !bds->argmin || bds->V <= 0 || bds->P <= 0 ||
              S <= 0 || bds->ref_batch <= 0 || N % bds->ref_batch != 0 ||
              (bds->sel && bds->rows != 1 && bds->rows != bds->ref_batch)))
    return ACFM_E_BADARG;
  const size_t lds = bds ? sizeof(float) * 3 * (size_t)bds->V : 0;   // as acfm_bds_loss
  if (lds > 150 * 1024) return ACFM_E_BADARG;
  if (partial_floats < acfm_step_losses_ws(N, mask ? mask->HW : 0, tex ? tex->HW : 0, S, nullptr)) return ACFM_E_WORKSPACE;
  TailBds B = {};
  TailMask M = {};
  TailTex T = {};
  TailTotal tot = {};
  float* part = partials;
  if (mask) {
    const int ppb = fwd_pix_per_block(N, mask->HW);
    M = {mask->mask, mask->gt, mask->edt, mask->out, {tickets, part}, mask->HW, mask->ref_batch,
         (mask->HW + ppb - 1) / ppb, ppb == PIX_PER_BLOCK_WIDE};
    part += loss_partial_floats(ACFM_LOSS_MASK, N, mask->HW);
  }
  if (tex) {
    const int ppb = fwd_pix_per_block(N, tex->HW);
    T = {tex->tex, tex->img, tex->mask, tex->out, {tickets + N, part}, tex->HW, tex->ref_batch,
         (tex->HW + ppb - 1) / ppb, ppb == PIX_PER_BLOCK_WIDE};
    part += loss_partial_floats(ACFM_LOSS_TEX_MSE, N, tex->HW);
  }
  if (bds)
    B = {bds->verts_xy, bds->bds, bds->vis, bds->sel, bds->loss, bds->argmin, {tickets + 2 * (size_t)N, part},
         bds->V, bds->P, bds->ref_batch, bds->sel ? bds->rows : 0, bds->sel ? bds->S : 0, (S + 63) / 64};
  if (total) {
    if (!total->total || fill_comb(tot.a, total->terms, nullptr, total->cols, total->weights, total->nterms) != ACFM_OK)
      return ACFM_E_BADARG;
    tot.total = total->total;
    tot.done = tickets + 3 * (size_t)N;
    tot.rows = (unsigned)N * (unsigned)((mask != nullptr) + (tex != nullptr) + (bds != nullptr));
  }
  const size_t blocks = (size_t)N * ((size_t)B.nb + (size_t)M.nb + (size_t)T.nb);
  if (blocks > 0x7fffffffull) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ACFM_PROF_STEP_TAIL, st);
  hipLaunchKernelGGL(k_step_tail, dim3((unsigned)blocks), dim3(LTPB), lds, st, B, M, T, tot, N);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_combine_losses_backward(const float* grad_total, void* const* grads, const int* cols,
                                 const float* weights, int nterms, int N, void* stream) {
  CombArgs a;
  if (!grad_total || !grads || N <= 0 || fill_comb(a, nullptr, grads, cols, weights, nterms) != ACFM_OK)
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_combine_bwd, dim3((N + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, N, grad_total);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_hypothesis_total(const void* const* terms, const float* weights, const int* aux_group, const float* aux_weights,
                          int nterms, int G, int N, float* total, float* probs, float* aux0, float* aux1, float* out,
                          void* stream) {
  if (!terms || !weights || !total || !probs || !out || nterms < 1 || nterms > HYP_MAX_TERMS || G <= 0 || G > 4096 ||
      N <= 0 || (size_t)G * N > 0x7fffffffull)
    return ACFM_E_BADARG;
  HypArgs a;
  for (int t = 0; t < HYP_MAX_TERMS; ++t) {
    a.t[t] = t < nterms ? (const float*)terms[t] : nullptr;
    a.g[t] = nullptr;
    a.w[t] = t < nterms ? weights[t] : 0.f;
    a.aux_group[t] = (t < nterms && aux_group) ? aux_group[t] : -1;
    a.aux_w[t] = (t < nterms && aux_weights) ? aux_weights[t] : 0.f;
    if (t < nterms && !a.t[t]) return ACFM_E_BADARG;
    if (a.aux_group[t] < -1 || a.aux_group[t] > 1) return ACFM_E_BADARG;
  }
  a.nterms = nterms;
  hipLaunchKernelGGL(k_hyp_total, dim3(1), dim3(256), 0, (hipStream_t)stream, a, G, N, total, probs, aux0, aux1, out);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_hypothesis_total_backward(const float* grad_weighted, const float* probs, const float* weights, int nterms,
                                   int G, int N, void* const* grads, void* stream) {
  if (!grad_weighted || !probs || !weights || !grads || nterms < 1 || nterms > HYP_MAX_TERMS || G <= 0 || N <= 0 ||
      (size_t)G * N > 0x7fffffffull)
    return ACFM_E_BADARG;
  HypArgs a;
  for (int t = 0; t < HYP_MAX_TERMS; ++t) {
    a.t[t] = nullptr;
    a.g[t] = t < nterms ? (float*)grads[t] : nullptr;
    a.w[t] = t < nterms ? weights[t] : 0.f;
    a.aux_group[t] = -1;
    a.aux_w[t] = 0.f;
  }
  a.nterms = nterms;
  const int GN = G * N;
  hipLaunchKernelGGL(k_hyp_total_bwd, dim3((GN + 255) / 256), dim3(256), 0, (hipStream_t)stream, a, GN, N,
                     grad_weighted, probs);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

size_t acfm_texture_cycle_scratch_floats(int B, int T, int F, int R) {
  if (B <= 0 || T <= 0 || F <= 0 || R < 2) return 0;
  const size_t total = (size_t)B * T * F * R * R * 3, pairs = total / ((size_t)R * R) * (R - 1);
  return pairs + (pairs + 255) / 256;
}

int acfm_texture_cycle(const float* textures, int B, int T, int F, int R, float* scratch, float* loss, void* stream) {
  if (!textures || !scratch || !loss || B <= 0 || T <= 0 || F <= 0 || R < 2) return ACFM_E_BADARG;
  const size_t total = (size_t)B * T * F * R * R * 3, pairs = total / ((size_t)R * R) * (R - 1);
  const size_t nblocks = (pairs + 255) / 256;
  if (nblocks > 0x7fffffffull) return ACFM_E_BADARG;
  const CycDims d = {B, T, F, R};
  hipStream_t st = (hipStream_t)stream;
  if (total < 0x7fffffffull)
    hipLaunchKernelGGL(k_tex_cycle<unsigned>, dim3((unsigned)nblocks), dim3(256), 0, st, textures, d, pairs, scratch, scratch + pairs);
  else
    hipLaunchKernelGGL(k_tex_cycle<size_t>, dim3((unsigned)nblocks), dim3(256), 0, st, textures, d, pairs, scratch, scratch + pairs);
  hipLaunchKernelGGL(k_tex_cycle_finish, dim3(1), dim3(256), 0, st, scratch + pairs, (int)nblocks, 1.0f / (float)pairs, loss);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_texture_cycle_backward(const float* textures, const float* scratch, const float* grad_loss, int B, int T, int F,
                                int R, float* grad_textures, void* stream) {
  if (!textures || !scratch || !grad_loss || !grad_textures || B <= 0 || T <= 0 || F <= 0 || R < 2) return ACFM_E_BADARG;
  const size_t total = (size_t)B * T * F * R * R * 3, pairs = total / ((size_t)R * R) * (R - 1);
  const size_t nblocks = (total + 255) / 256;
  if (nblocks > 0x7fffffffull) return ACFM_E_BADARG;
  const CycDims d = {B, T, F, R};
  if (total < 0x7fffffffull)
    hipLaunchKernelGGL(k_tex_cycle_bwd<unsigned>, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, textures, scratch,
                       grad_loss, d, total, 1.0f / (float)pairs, grad_textures);
  else
    hipLaunchKernelGGL(k_tex_cycle_bwd<size_t>, dim3((unsigned)nblocks), dim3(256), 0, (hipStream_t)stream, textures, scratch,
                       grad_loss, d, total, 1.0f / (float)pairs, grad_textures);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_visible_vertices(const int64_t* pix_to_face, const int64_t* faces, int N, int V, int F, int HW,
                          int K, uint8_t* vis, void* stream) {
  if (!pix_to_face || !faces || !vis || N <= 0 || N > 65535 || V <= 0 || F <= 0 || HW <= 0 || K <= 0)
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_async(vis, (size_t)N * V, st) != ACFM_OK) return ACFM_E_LAUNCH;
  ProfScope ps(ACFM_PROF_VISIBLE, st);
  hipLaunchKernelGGL(k_visible, dim3((HW + 255) / 256, N), dim3(256), 0, st, pix_to_face, faces, V, F,
                     HW, K, vis);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_bds_loss(const float* verts_xy, const float* bds, const uint8_t* vis, const int32_t* sel, int N, int V,
                  int P, int ref_batch, int rows, int S, float* loss, int32_t* argmin, uint32_t* tickets,
                  float* partials, size_t partial_floats, void* stream) {
  if (!verts_xy || !bds || !vis || !loss || !argmin || N <= 0 || N > 65535 || V <= 0 || P <= 0 || ref_batch <= 0 ||
      N % ref_batch != 0 || (sel && (S <= 0 || (rows != 1 && rows != ref_batch))))
    return ACFM_E_BADARG;
  const size_t lds = sizeof(float) * 3 * (size_t)V;   // (x, y) per vertex + the index a packed vertex came from
  if (lds > 150 * 1024) return ACFM_E_BADARG;
  const int n = sel ? S : P;   // points per mesh
  RowScratch sc;
  if (const int rc = row_scratch(ACFM_LOSS_BDS, N, n, tickets, partials, partial_floats, sc)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!sc.tickets && zero_async(loss, sizeof(float) * (size_t)N, st) != ACFM_OK) return ACFM_E_LAUNCH;
  ProfScope ps(ACFM_PROF_BDS, st);
  if (sel)
    hipLaunchKernelGGL(k_bds_loss_sel, dim3((n + 63) / 64, N), dim3(LTPB), lds, st, verts_xy, bds, vis,
                       V, P, ref_batch, loss, argmin, sc, sel, rows, S);
  else
    hipLaunchKernelGGL(k_bds_loss, dim3((n + 63) / 64, N), dim3(LTPB), lds, st, verts_xy, bds, vis,
                       V, P, ref_batch, loss, argmin, sc);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_bds_loss_backward(const float* verts_xy, const float* bds, const int32_t* sel, const int32_t* argmin,
                           const float* grad_loss, int N, int V, int P, int ref_batch, int rows, int S,
                           float* grad_verts_xy, void* stream) {
  if (!verts_xy || !bds || !argmin || !grad_loss || !grad_verts_xy || N <= 0 || N > 65535 || V <= 0 ||
      P <= 0 || ref_batch <= 0 || N % ref_batch != 0 || (sel && (S <= 0 || (rows != 1 && rows != ref_batch))))
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = sizeof(float) * 2 * (size_t)V;
  if (lds > 150 * 1024) return ACFM_E_BADARG;
  ProfScope ps(ACFM_PROF_BDS_BWD, st);
  if (sel)
    hipLaunchKernelGGL(k_bds_loss_sel_bwd, dim3(N), dim3(256), lds, st, verts_xy, bds, argmin, grad_loss, V, P,
                       ref_batch, grad_verts_xy, sel, rows, S);
  else
    hipLaunchKernelGGL(k_bds_loss_bwd, dim3(N), dim3(256), lds, st, verts_xy, bds, argmin,
                       grad_loss, V, P, ref_batch, grad_verts_xy);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_of_loss(const float* proj, const float* flows, const float* masks, const uint8_t* vis, int B, int T,
                 int V, int H, int W, int clips, int flip_t, float* loss, float* count, void* stream) {
  if (!proj || !flows || !vis || !loss || !count || B <= 0 || B > 65535 || T < 2 || T > 65535 || V <= 0 || H <= 0 ||
      W <= 0 || clips <= 0 || B % clips != 0)
    return ACFM_E_BADARG;
  const OfSrc src = {flows, masks, clips, flip_t ? 1 : 0};
  hipLaunchKernelGGL(k_of_loss, dim3(T - 1, B), dim3(LTPB), 0, (hipStream_t)stream, proj, src, vis, T, V, H, W,
                     loss, count);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_of_loss_backward(const float* proj, const float* flows, const float* masks, const uint8_t* vis,
                          const float* count, const float* grad_loss, int B, int T, int V, int H, int W, int clips,
                          int flip_t, float* grad_proj, void* stream) {
  if (!proj || !flows || !vis || !count || !grad_loss || !grad_proj || B <= 0 || B > 65535 || T < 2 || T > 65535 ||
      V <= 0 || H <= 0 || W <= 0 || clips <= 0 || B % clips != 0)
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_async(grad_proj, sizeof(float) * 3 * (size_t)B * T * V, st) != ACFM_OK) return ACFM_E_LAUNCH;
  const OfSrc src = {flows, masks, clips, flip_t ? 1 : 0};
  hipLaunchKernelGGL(k_of_loss_bwd, dim3((V + LTPB - 1) / LTPB, T - 1, B), dim3(LTPB), 0, st, proj, src, vis, count,
                     grad_loss, T, V, H, W, grad_proj);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
