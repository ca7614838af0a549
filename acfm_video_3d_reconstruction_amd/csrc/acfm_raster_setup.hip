// Face setup and scheduling of the raster workspace: k_setup, k_order, launch_setup, acfm_raster_workspace_bytes.
// Replaces the vertex transform and the coarse (binning) half of PyTorch3D 0.3.0's rasterize_meshes.
//
// Design:
//   * k_setup: 4, 8 or 16 workgroups per mesh (face slices) project the V vertices into LDS
//     (weak-perspective camera, y flip, view transform) and write one 128-byte record per face
//     (blur-expanded box, vertices, depths, per-edge constants), the face bitmask of every 16x16
//     coarse tile and a cost count per 8x8 block, counted in LDS and stored as one plane per slice
//     (no zero fill, no atomics in memory); k_order adds the planes, sorts every XCD group's
//     (mesh, block) entries heavy-first (counting sort, no atomics) and puts the blocks no face
//     box comes near at the end.
#include "acfm_raster.h"

namespace acfm {

// ------------------------------------------------------------------------------- setup
// mode 0: verts are world coordinates -> project with cams, flip y   (nmr.py:145-149)
// mode 1: verts are already projected, no y flip                     (nmr.py:224-238)
// mode 2: verts are already NDC x, NDC y, view z: taken as they are (acfm_rasterize_fragments)
// Grid (N, ws.slices): every workgroup projects the mesh's V vertices into LDS (cheap, and it
// keeps the slices independent) and handles one slice of the faces; slice boundaries are multiples
// of 64 faces, so each slice owns whole words of the coarse masks and builds them in LDS without
// talking to the others.  Tile counters are kept in LDS and leave as one plane per slice with plain
// stores (k_order adds the planes: no zero fill, no global atomics); only images beyond 512^2 fall
// back to global atomics on a zeroed ws.tile_cnt.  The mesh box is left as one box per slice (the
// raster kernels take the union of four; k_order joins 8 or 16 into the first slot).
__host__ __device__ __forceinline__ int setup_slice_faces(int F, int slices) {
  return ((F + slices - 1) / slices + 63) / 64 * 64;
}

template <int SLICES>   // face slices per mesh (grid y): 4, 8 or 16 -- a template so that the slice arithmetic stays compile-time
__global__ __launch_bounds__(TPB) void k_setup(const float* __restrict__ verts,
                                               const int64_t* __restrict__ faces,
                                               const float* __restrict__ cams, int V, int F, int H,
                                               float offset_z, int mode, float margin, RasterWs ws,
                                               uint8_t* __restrict__ vis, float* __restrict__ proj_xy) {
  extern __shared__ float s_v[];  // [V][3], then [tiles^2] int counters and this slice's mask words (if they fit)
  __shared__ float s_red[4][4];
  const int n = blockIdx.x, slice = blockIdx.y, tid = threadIdx.x;
  const float* cam = cams ? cams + 7 * (size_t)n : nullptr;
  const int tiles_ = (H + CNT_TILE - 1) / CNT_TILE, tt_ = tiles_ * tiles_;
  const bool lds_cnt = tt_ <= SETUP_LDS_TILES;
  int* s_cnt = reinterpret_cast<int*>(s_v + 3 * V);
  if (lds_cnt)
    for (int i = tid; i < tt_; i += TPB) s_cnt[i] = 0;
  const int q = setup_slice_faces(F, SLICES);
  const int f_lo = slice * q, f_hi = min(F, f_lo + q);
  // coarse face masks: bit f of row (cty, ctx) <=> the box of face f may touch that CTILE x CTILE tile
  const int ctiles_ = (H + CTILE - 1) / CTILE, mwords = 2 * ((F + 63) / 64);  // u32 words per row
  const int rows = ctiles_ * ctiles_;
  const int w_lo = f_lo >> 5, w_n = max(0, min(mwords, (f_lo + q) >> 5) - w_lo);  // this slice's words of a row
  const bool lds_mask = (size_t)rows * w_n * sizeof(unsigned) <= (size_t)SETUP_LDS_MASK_BYTES;
  unsigned* g_mask = ws.cmask + (size_t)n * rows * mwords;              // zeroed by the host if !lds_mask
  unsigned* s_mask = reinterpret_cast<unsigned*>(s_cnt + (lds_cnt ? tt_ : 0));
  if (lds_mask)
    for (int i = tid; i < rows * w_n; i += TPB) s_mask[i] = 0u;
  for (int v = tid; v < V; v += TPB) {
    const float* x = verts + ((size_t)n * V + v) * 3;
    float px, py, pz;
    if (mode == 0) {
      project_point(cam, x[0], x[1], x[2], offset_z, px, py, pz);
      // NeuralRenderer.project_points of the same vertices and cameras (nmr.py:127-129: proj_fn(...)[:, :, :2]) is
      // this very (px, py): handed out on request (AcfmSilExtras.proj_xy) instead of being projected again
      if (proj_xy && slice == 0) { proj_xy[((size_t)n * V + v) * 2] = px; proj_xy[((size_t)n * V + v) * 2 + 1] = py; }
      py = py * -1.0f;
    } else {
      px = x[0]; py = x[1]; pz = x[2];
    }
    if (mode != 2) {
      px = -px;               // view R = diag(-1, 1, 1)
      pz = pz + ACFM_EYE_Z;   // view T = (0, 0, 2.732)
    }
    s_v[3 * v + 0] = px; s_v[3 * v + 1] = py; s_v[3 * v + 2] = pz;
    if (slice == 0) {
      float* o = ws.ndc + ((size_t)n * V + v) * 3;
      o[0] = px; o[1] = py; o[2] = pz;
      // zeroed here instead of by launches of their own: the visible-vertex bytes the raster kernel
      // marks, and the NDC-gradient scratch the backward accumulates into (k_project_bwd<1> leaves
      // it zeroed again after reading it)
      if (vis) vis[(size_t)n * V + v] = 0;
      ws.grad_ndc[((size_t)n * V + v) * 2] = 0.f;
      ws.grad_ndc[((size_t)n * V + v) * 2 + 1] = 0.f;
      ws.grad_fix[((size_t)n * V + v) * 2] = 0;
      ws.grad_fix[((size_t)n * V + v) * 2 + 1] = 0;
    }
  }
  __syncthreads();
  const float INF = __builtin_inff();
  float bx0 = INF, bx1 = -INF, by0 = INF, by1 = -INF;
  bool big = false;
  auto count_box = [&](int xa, int ya, int xb, int yb) {   // pixel range (clamped to the image) -> +1 on its 8x8 blocks
    xa /= CNT_TILE; ya /= CNT_TILE; xb /= CNT_TILE; yb /= CNT_TILE;
    if ((xb - xa + 1) * (yb - ya + 1) > 256) {
      big = true;  // too many tiles to count one by one: every tile of the mesh gets +1 below
    } else
      for (int ty = ya; ty <= yb; ++ty)
        for (int tx = xa; tx <= xb; ++tx) {
          if (lds_cnt) atomicAdd(&s_cnt[ty * tiles_ + tx], 1);
          else atomicAdd(&ws.tile_cnt[((size_t)n * tiles_ + ty) * tiles_ + tx], 1);
        }
  };
  for (int f = f_lo + tid; f < f_hi; f += TPB) {
    const int64_t* fi = faces + ((size_t)n * F + f) * 3;
    int i0 = (int)fi[0], i1 = (int)fi[1], i2 = (int)fi[2];
    i0 = min(max(i0, 0), V - 1); i1 = min(max(i1, 0), V - 1); i2 = min(max(i2, 0), V - 1);
    const float x0 = s_v[3 * i0], y0 = s_v[3 * i0 + 1], z0 = s_v[3 * i0 + 2];
    const float x1 = s_v[3 * i1], y1 = s_v[3 * i1 + 1], z1 = s_v[3 * i1 + 2];
    const float x2 = s_v[3 * i2], y2 = s_v[3 * i2 + 1], z2 = s_v[3 * i2 + 2];
    const float area = edge_fn(x2, y2, x0, y0, x1, y1);
    const bool degenerate = (area <= ACFM_K_EPS && area >= -1.0f * ACFM_K_EPS);
    float4 b;
    b.x = min3f(x0, x1, x2) - margin; b.y = max3f(x0, x1, x2) + margin;
    b.z = min3f(y0, y1, y2) - margin; b.w = max3f(y0, y1, y2) + margin;
    if (degenerate) {
      b = make_float4(INF, -INF, INF, -INF);  // fails every "inside box" test
    } else {
      bx0 = fminf(bx0, b.x); bx1 = fmaxf(bx1, b.y); by0 = fminf(by0, b.z); by1 = fmaxf(by1, b.w);
    }
    const size_t o = (size_t)n * F + f;
    // (x1, x2) and (y1, y2) sit in aligned register pairs after the 16-byte LDS reads: operands of the packed fp32 pipe
    FaceRec& r = ws.rec[o];
    r.box = b;
    r.a = make_float4(x0, y0, x1, x2);
    r.b = make_float4(y1, y2, z0, z1);
    {
      const float denom = area + ACFM_K_EPS;
      r.c = make_float4(z2, area, denom, recip_refined(denom));
      // point_line_dist's own operations on (a, b) = (v0, v1), (v0, v2), (v1, v2): bax = bx - ax, l2 = bax bax + bay bay
      const float e01x = x1 - x0, e01y = y1 - y0, e02x = x2 - x0, e02y = y2 - y0, e12x = x2 - x1, e12y = y2 - y1;
      const float l01 = e01x * e01x + e01y * e01y, l02 = e02x * e02x + e02y * e02y, l12 = e12x * e12x + e12y * e12y;
      const bool deg = (l01 <= ACFM_K_EPS) || (l02 <= ACFM_K_EPS) || (l12 <= ACFM_K_EPS);
      r.e0 = make_float4(l01, l02, recip_refined(l01), recip_refined(l02));
      r.e1 = make_float4(l12, recip_refined(l12), deg ? 1.0f : 0.0f, 0.0f);
    }
    ws.vidx[o] = make_int4(i0, i1, i2, 0);
    ws.fvis[o] = 0;
    if (!degenerate) {
      // pixel index of an NDC coordinate (ndc_to_pix_held); one pixel of slack
      const float hf = (float)H;
      int xa = (int)floorf(ndc_to_pix_held(b.y, hf)) - 1;
      int xb = (int)ceilf(ndc_to_pix_held(b.x, hf)) + 1;
      int ya = (int)floorf(ndc_to_pix_held(b.w, hf)) - 1;
      int yb = (int)ceilf(ndc_to_pix_held(b.z, hf)) + 1;
      if (xb >= 0 && yb >= 0 && xa < H && ya < H) {
        xa = max(xa, 0); ya = max(ya, 0); xb = min(xb, H - 1); yb = min(yb, H - 1);
        const unsigned bit = 1u << (f & 31);
        for (int cy = ya / CTILE; cy <= yb / CTILE; ++cy)
          for (int cx = xa / CTILE; cx <= xb / CTILE; ++cx) {
            const int row = cy * ctiles_ + cx;
            if (lds_mask) atomicOr(&s_mask[row * w_n + ((f >> 5) - w_lo)], bit);
            else atomicOr(&g_mask[(size_t)row * mwords + (f >> 5)], bit);
          }
        // cost estimate for heavy-first scheduling: +1 on every 8x8 block the box may touch.  With the counters in LDS
        // (images up to 512^2) every slice counts its own faces and stores its plane of ws.tile_part (k_order adds the
        // four planes): no zero fill, no global atomics; larger images: every slice adds its faces to the zeroed ws.tile_cnt
        count_box(xa, ya, xb, yb);
      }
    }
  }
  bx0 = wave_min(bx0); bx1 = wave_max(bx1); by0 = wave_min(by0); by1 = wave_max(by1);
  const int w = tid >> 6;
  if ((tid & 63) == 0) { s_red[w][0] = bx0; s_red[w][1] = bx1; s_red[w][2] = by0; s_red[w][3] = by1; }
  const int any_big = __syncthreads_or(big) ? 1 : 0;  // (also the barrier before the copies below)
  if (lds_cnt) {
    int* part = ws.tile_part + ((size_t)slice * gridDim.x + n) * tt_;
    for (int i = tid; i < tt_; i += TPB) part[i] = s_cnt[i] + any_big;   // this slice's faces: plain stores
  } else {
    for (int i = tid; i < tt_; i += TPB)                // ws.tile_cnt was zeroed by the host
      if (any_big) atomicAdd(&ws.tile_cnt[(size_t)n * tt_ + i], any_big);
  }
  if (lds_mask)
    for (int i = tid; i < rows * w_n; i += TPB)
      g_mask[(size_t)(i / w_n) * mwords + w_lo + (i % w_n)] = s_mask[i];
  if (tid == 0) {
    for (int i = 1; i < 4; ++i) {
      bx0 = fminf(bx0, s_red[i][0]); bx1 = fmaxf(bx1, s_red[i][1]);
      by0 = fminf(by0, s_red[i][2]); by1 = fmaxf(by1, s_red[i][3]);
    }
    ws.mbox[(size_t)n * SLICES + slice] = make_float4(bx0, bx1, by0, by1);
  }
}

// ------------------------------------------------------------------------------- scheduling
// Heavy-first order.  Per-block work is heavy-tailed (dense clusters of tiny faces: a block can
// take 20x the average), so every XCD group visits its (mesh, block) entries in descending cost
// class; the long blocks start first and the short ones fill in behind them.
// Entry e of group g  <->  mesh (e / tt) * G + g, block e % tt   (G = 8 groups if N % 8 == 0, else 1).
// The cost of a block is the face count of its 16x16 tile (k_setup); count 0 = no face box comes
// near: the entry is flagged and the raster kernels write that block's zeros without looking at
// the mesh at all.
constexpr int NCLASS = 10;
constexpr int ORDER_MAX_WGS = 128;   // workgroups of a k_order launch (launch_setup)
// (the classes above 160 exist to ORDER the heaviest blocks: at 64 frames the blocks of >= 240 face boxes -- 89 of
// 15 474, 3 % of the work -- start first and still run for the whole launch; see the split rule in k_order.  Every
// class costs k_order a ballot per entry and pass: 12 classes measured 18.1 us per launch against 13.3 with 8)
__device__ __forceinline__ int cost_class(int c) {
  return c >= 240 ? 0 : c >= 200 ? 1 : c >= 160 ? 2 : c >= 112 ? 3 : c >= 80 ? 4 : c >= 56 ? 5 : c >= 36 ? 6 : c >= 20 ? 7 : c >= 1 ? 8 : 9;
}
template <bool MORE>   // MORE: k_setup ran 8 or 16 face slices per mesh (few meshes); false: the usual four
__global__ __launch_bounds__(1024) void k_order(RasterWs ws, int N, int tt, int H, int g_split_dev, int mpw) {
  // Counting sort by cost class without atomics.  Grid (G, W): workgroup (g, w) places the entries of the meshes
  // w mpw .. w mpw + mpw - 1 of XCD group g (mpw = 1, a workgroup per mesh, up to ORDER_MAX_WGS workgroups in the
  // launch; one workgroup per group beyond N = 8 ORDER_MAX_WGS).  An entry's position is
  //     the class's base in the group  +  the entries of that class in the group's earlier meshes  +  its rank among
  //     the workgroup's own entries
  // The first two come from the cost planes of the group's OTHER meshes, which every workgroup of the group classifies
  // for itself (ballots, wave-uniform counters): no workgroup waits for another.  The rank is the old scheme on the
  // workgroup's own entries: every wave counts its entries per class, the counts are prefix-summed over (class, wave),
  // every wave scatters from its own running offsets.  Deterministic order: class, workgroup, wave, entry.
  // Every cost plane is loaded once per workgroup, as it was when one workgroup per group did all of this (18.7 us on 8
  // CUs at 64 frames @256^2; 10.7 us with 64 workgroups); the launch as a whole reads them W times, from L2.
  constexpr int NW = 16;   // waves of the workgroup
  __shared__ int s_cnt[NCLASS][NW], s_off[NCLASS][NW], s_all[NCLASS][NW], s_bef[NCLASS][NW], s_hist[NCLASS], s_before[NCLASS], s_split;
  const int G = gridDim.x, g = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int M = N / G, per = M * tt;
  const int m_lo = (int)blockIdx.y * mpw, m_hi = min(M, m_lo + mpw);
  const int lo = m_lo * tt, hi = m_hi * tt;   // this workgroup's entries: lo .. hi - 1
  // entry e = m tt + bl  <->  mesh m G + g, block bl; its cost is tile_cnt[mesh][bl] (CNT_TILE == RBLK).
  static_assert(CNT_TILE == RBLK, "cost counters are per raster block");
  if constexpr (MORE) {
    // the mesh boxes: k_setup left one box per face slice; the raster kernels test a block against the mesh's box: with
    // more than four slices it is joined here, once, into the first slot
    for (int m = m_lo + (int)threadIdx.x; m < m_hi; m += blockDim.x) {
      float4* mb = ws.mbox + (size_t)(m * G + g) * ws.slices;
      float4 u = mb[0];
      for (int i = 1; i < ws.slices; ++i) {
        const float4 m2 = mb[i];
        u.x = fminf(u.x, m2.x); u.y = fmaxf(u.y, m2.y); u.z = fminf(u.z, m2.z); u.w = fmaxf(u.w, m2.w);
      }
      mb[0] = u;
    }
  }
  const bool parts = tt <= SETUP_LDS_TILES;   // k_setup kept its counters in LDS: one plane per face slice
  // cost of block bl of the group's mesh mm: the sum of the face slices' planes (k_setup), or the finished counter
  auto cost = [&](int mm, int bl) {
    const size_t o = (size_t)(mm * G + g) * tt + bl;
    if (!parts) return ws.tile_cnt[o];
    const size_t plane = (size_t)N * tt;
    int c = (ws.tile_part[o] + ws.tile_part[plane + o]) + (ws.tile_part[2 * plane + o] + ws.tile_part[3 * plane + o]);
    if constexpr (MORE)
      for (int sl = 4; sl < ws.slices; sl += 4)     // 8 or 16 planes
        c += (ws.tile_part[sl * plane + o] + ws.tile_part[(sl + 1) * plane + o]) +
             (ws.tile_part[(sl + 2) * plane + o] + ws.tile_part[(sl + 3) * plane + o]);
    return c;
  };
  // (mm, bl) advance with e: no integer divisions in the loops (they were 2000 VALU instructions per wave)
  // pass 1a, the workgroup's own entries: one per thread while there are at most 1024, a loop above that.  The sum of the
  // planes is kept for the later readers (k_tex_cover, the stamps) and for the scatter below.
  const int own_iters = (hi - lo + (int)blockDim.x - 1) / (int)blockDim.x;
  int cnt[NCLASS];
#pragma unroll
  for (int c = 0; c < NCLASS; ++c) cnt[c] = 0;
  int cst_first = -1;
  {
    int m1 = m_lo + (int)threadIdx.x / tt, bl1 = (int)threadIdx.x % tt;
    for (int it = 0; it < own_iters; ++it) {
      const int e = lo + it * (int)blockDim.x + (int)threadIdx.x;
      int cs = -1;
      if (e < hi) {
        cs = cost(m1, bl1);
        if (parts) ws.tile_cnt[(size_t)(m1 * G + g) * tt + bl1] = cs;
      }
      bl1 += blockDim.x;
      while (bl1 >= tt) { bl1 -= tt; ++m1; }
      if (it == 0) cst_first = cs;
      const int cl = cs < 0 ? -1 : cost_class(cs);
#pragma unroll
      for (int c = 0; c < NCLASS; ++c) cnt[c] += __popcll(__ballot(cl == c));
    }
  }
  // pass 1b, the other meshes of the group: entries per class, and of those the ones of the earlier meshes (e < lo).
  // (nothing to do for a workgroup that owns the whole group)
  constexpr int OCH = 8;   // entries per thread whose cost loads are in flight together
  const int iters = (lo == 0 && hi == per) ? 0 : (per + (int)blockDim.x - 1) / (int)blockDim.x;
  int all[NCLASS], bef[NCLASS];
#pragma unroll
  for (int c = 0; c < NCLASS; ++c) { all[c] = 0; bef[c] = 0; }
  int m1 = (int)threadIdx.x / tt, bl1 = (int)threadIdx.x % tt;
  for (int it0 = 0; it0 < iters; it0 += OCH) {
    int cst[OCH];
#pragma unroll
    for (int u = 0; u < OCH; ++u) {
      const int e = (it0 + u) * blockDim.x + threadIdx.x;
      cst[u] = (it0 + u < iters && e < per && (e < lo || e >= hi)) ? cost(m1, bl1) : -1;
      bl1 += blockDim.x;
      while (bl1 >= tt) { bl1 -= tt; ++m1; }
    }
#pragma unroll
    for (int u = 0; u < OCH; ++u) {
      const int e = (it0 + u) * blockDim.x + threadIdx.x;
      const int e_w0 = (it0 + u) * (int)blockDim.x + wv * 64;   // the wave's first entry (wave-uniform)
      const int cl = cst[u] < 0 ? -1 : cost_class(cst[u]);      // (-1: no entry, or one of the workgroup's own)
      if (e_w0 + 63 < lo) {            // the whole wave stands before the workgroup's entries
#pragma unroll
        for (int c = 0; c < NCLASS; ++c) { const int k = __popcll(__ballot(cl == c)); all[c] += k; bef[c] += k; }
      } else if (e_w0 >= lo) {         // none of it does
#pragma unroll
        for (int c = 0; c < NCLASS; ++c) all[c] += __popcll(__ballot(cl == c));
      } else {
#pragma unroll
        for (int c = 0; c < NCLASS; ++c) {
          all[c] += __popcll(__ballot(cl == c));
          bef[c] += __popcll(__ballot(cl == c && e < lo));
        }
      }
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < NCLASS; ++c) { s_cnt[c][wv] = cnt[c]; s_all[c][wv] = all[c]; s_bef[c][wv] = bef[c]; }
  }
  __syncthreads();
  const int nwaves = (int)blockDim.x >> 6;
  if (threadIdx.x < NCLASS) {   // per class: the group's total (the other meshes' and the own entries) and the share of the earlier meshes
    int t = 0, b = 0;
    for (int w = 0; w < nwaves; ++w) { t += s_all[threadIdx.x][w] + s_cnt[threadIdx.x][w]; b += s_bef[threadIdx.x][w]; }
    s_hist[threadIdx.x] = t;
    s_before[threadIdx.x] = b;
  }
  __syncthreads();
  if (threadIdx.x < NCLASS) {   // the offsets of this mesh's waves inside the class
    int acc = s_before[threadIdx.x];
    for (int c = 0; c < (int)threadIdx.x; ++c) acc += s_hist[c];
    for (int w = 0; w < nwaves; ++w) { s_off[threadIdx.x][w] = acc; acc += s_cnt[threadIdx.x][w]; }
  }
  if (threadIdx.x == 0) {
    int nw = 0;
    for (int c = 0; c < NCLASS - 1; ++c) nw += s_hist[c];
    if (blockIdx.y == 0) ws.n_work[g] = nw;   // the flagged-empty class sits at the end of the order; one workgroup per group publishes
    // Split the heaviest blocks over four workgroups each?  It adds ~25 % work to those blocks and shortens them about
    // 3x.  A launch lasts at least as long as its longest block (per-block stamps at 64 frames @256^2: the blocks of
    // ~300 face boxes start at t = 0 and end with the kernel, 225 us, while the work spread over the wave slots comes to
    // 195 us), so a block is split when its cost exceeds `ratio` x the group's mean work per wave slot (512 slots per
    // XCD at 16 one-wave workgroups per CU): a whole small launch, the top few dozen blocks of a large one.
    // split_mode < 0: ratio = -split_mode / 4 (default -5: 1.25).
    // (a function of the group's histogram alone: every workgroup of the group arrives at the same class)
    const int mid[NCLASS] = {290, 220, 180, 136, 96, 68, 46, 28, 10, 0};
    long total = 0;
    for (int c = 0; c < NCLASS; ++c) total += (long)s_hist[c] * mid[c];
    int max_class = -1;                      // split the classes 0 .. max_class
    if (ws.split_slots > 0) {
      if (g_split_dev > 0) max_class = SPLIT_MAX_CLASS;
      else if (g_split_dev < 0)
        for (int c = 0; c <= SPLIT_MAX_CLASS; ++c)
          if (4L * mid[c] * 512 > (long)(-g_split_dev) * total) max_class = c;
    }
    s_split = max_class;
  }
  __syncthreads();
  const int split_slots = ws.split_slots, split_class = s_split;
  // pass 2: scatter the workgroup's own entries (order inside a class is arbitrary: results never depend on it)
  int off[NCLASS];
#pragma unroll
  for (int c = 0; c < NCLASS; ++c) off[c] = s_off[c][wv];
  const unsigned long long lt = (1ull << lane) - 1ull;
  int* ord = ws.order + (size_t)g * per;
  m1 = m_lo + (int)threadIdx.x / tt; bl1 = (int)threadIdx.x % tt;
  for (int it = 0; it < own_iters; ++it) {
    const int e = lo + it * (int)blockDim.x + (int)threadIdx.x;
    const int cs = it == 0 ? cst_first : (e < hi ? ws.tile_cnt[(size_t)(m1 * G + g) * tt + bl1] : -1);
    bl1 += blockDim.x;
    while (bl1 >= tt) { bl1 -= tt; ++m1; }
    const int cls = cs < 0 ? -1 : cost_class(cs);
#pragma unroll
    for (int c = 0; c < NCLASS; ++c) {
      const unsigned long long mk = __ballot(cls == c);
      if (cls == c) {
        const int pos = off[c] + __popcll(mk & lt);
        ord[pos] = e | (c == NCLASS - 1 ? ENTRY_EMPTY : 0) | ((c <= split_class && pos < split_slots) ? ENTRY_SPLIT : 0);
      }
      off[c] += __popcll(mk);
    }
  }
}

// ------------------------------------------------------------------------------- host side
int launch_setup(const float* verts, const int64_t* faces, const float* cams, int N, int V,
                        int F, int H, float offset_z, int mode, float blur, const RasterWs& ws,
                        const Tune& tn, hipStream_t st, uint8_t* vis, float* proj_xy) {
  const float margin = sqrtf(blur);
  const int tiles = (H + CNT_TILE - 1) / CNT_TILE;
  const int tt = tiles * tiles;                 // cost counters
  const int blocks = (H + RBLK - 1) / RBLK;
  const int ctiles = (H + CTILE - 1) / CTILE;
  const size_t mwords = 2 * (((size_t)F + 63) / 64);
  const size_t slice_words = (size_t)setup_slice_faces(F, ws.slices) / 32;
  const size_t slice_mask_bytes = sizeof(unsigned) * (size_t)ctiles * ctiles * (slice_words < mwords ? slice_words : mwords);
  const bool lds_mask = slice_mask_bytes <= (size_t)SETUP_LDS_MASK_BYTES;
  const size_t lds = sizeof(float) * 3 * (size_t)V + (tt <= SETUP_LDS_TILES ? sizeof(int) * (size_t)tt : 0) +
                     (lds_mask ? slice_mask_bytes : 0);
  if (lds > 150 * 1024) return ACFM_E_BADARG;
  if (!lds_mask && zero_async(ws.cmask, sizeof(unsigned) * (size_t)N * ctiles * ctiles * mwords, st)) return ACFM_E_LAUNCH;
  // (counters in LDS: every slice of k_setup stores its own plane of ws.tile_part, nothing to zero)
  if (tt > SETUP_LDS_TILES && zero_async(ws.tile_cnt, sizeof(int) * (size_t)N * tt, st)) return ACFM_E_LAUNCH;
  ProfScope ps(ACFM_PROF_SETUP, st);
  switch (ws.slices) {
    case 4: hipLaunchKernelGGL(k_setup<4>, dim3(N, 4), dim3(TPB), lds, st, verts, faces, cams, V, F, H, offset_z, mode,
                               margin, ws, vis, proj_xy); break;
    case 8: hipLaunchKernelGGL(k_setup<8>, dim3(N, 8), dim3(TPB), lds, st, verts, faces, cams, V, F, H, offset_z, mode,
                               margin, ws, vis, proj_xy); break;
    default: hipLaunchKernelGGL(k_setup<16>, dim3(N, 16), dim3(TPB), lds, st, verts, faces, cams, V, F, H, offset_z, mode,
                                margin, ws, vis, proj_xy); break;
  }
  // one workgroup per mesh while that is at most ORDER_MAX_WGS workgroups: all of them are resident at once (two
  // 1024-thread workgroups per CU), each loads the group's planes once, and the launch reads them W times from L2
  // (8 MB at 64 frames @256^2, 33 MB at 128).  Larger batches: mpw meshes per workgroup, the same number of workgroups.
  const int groups = (N & 7) == 0 ? 8 : 1, M = N / groups;
  const int wmax = ORDER_MAX_WGS / groups < 1 ? 1 : ORDER_MAX_WGS / groups;   // workgroups per group
  const int mpw = (M + wmax - 1) / wmax;
  const dim3 order_grid(groups, (M + mpw - 1) / mpw);
  if (ws.slices > 4)
    hipLaunchKernelGGL(k_order<true>, order_grid, dim3(1024), 0, st, ws, N, blocks * blocks, H, tn.split, mpw);
  else
    hipLaunchKernelGGL(k_order<false>, order_grid, dim3(1024), 0, st, ws, N, blocks * blocks, H, tn.split, mpw);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

size_t acfm_raster_workspace_bytes(int N, int V, int F, int H) {
  if (N <= 0 || V <= 0 || F <= 0 || H <= 0) return 0;
  return carve_ws(nullptr, N, V, F, H).bytes;
}

}  // extern "C"
