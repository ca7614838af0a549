// The walk kernels of the rasteriser for gfx950: tiled top-K forward (soft silhouette K<=32, hard K=1 with
// optional atlas shading) and the silhouette backward, with their launchers (acfm_raster.h).  The forward and the
// backward stay in ONE unit, forward first: compiled apart they come out different.  The other
// units of the rasteriser: acfm_raster_setup.hip (k_setup, k_order), acfm_raster_api.hip (entry points),
// acfm_raster_frag.hip, acfm_raster_texgrad.hip, acfm_project.hip.
//
// Replaces PyTorch3D 0.3.0's rasterize_meshes coarse/fine/backward CUDA kernels and the
// blending shaders as used by multiframe/nnutils/nmr.py:143-200, 224-238 (semantics:
// SURVEY.md App-A; the CPU oracle in oracle/acfm_oracle.c is the bit-level spec).
//
// Design:
//   * k_raster_fwd / k_sil_bwd share one skeleton: a ONE-WAVE workgroup owns an 8x8 pixel
//     block (four 4x4 blocks, one per 16-lane group).  Faces are binned against the block with
//     wave ballots into an LDS candidate list (deterministic, face-ordered, no barriers); the
//     groups then walk their own sub-lists.  A launch has entries / div workgroups per group:
//     workgroup j renders the entries j, j + stride, .. that have work and, in the forward,
//     first stores the constant outputs of its share of the empty blocks (struct Sched).
//   * forward, K > 1: every lane keeps its pixel's K nearest (depth|face) keys and blend
//     factors SORTED in registers (shift insertion on static register indices, 4-slot
//     blocks no lane's element can enter are skipped): no per-pixel LDS or memory lists, no final
//     sort, the blend product runs over exactly the kept faces; the block's candidates are walked
//     roughly front to back (8 depth classes); ids leave through LDS as 16-byte stores in image
//     order.  128 VGPRs, 4 waves per SIMD.
//   * forward, K = 1 (blur 0): only the winner's edge distances are evaluated; 6 waves per SIMD.
//   * backward: the same walk; membership of a face in a pixel's top-K is `key <= kth[pixel]`
//     (kth saved by the forward), gradients of a candidate are summed over the 16 lanes of its
//     group (pair swap, then DPP row shifts on three values per lane) and TWO lanes add them to the
//     candidate's LDS accumulator, which is flushed with one global float atomic per touched
//     coordinate.  5 waves per SIMD.
//   * forward, K > 1, ACFM_RECORD_COVER: the walk also keeps the nearest COVERING face per pixel (the
//     hard K = 1 render's answer); k_tex_cover shades the texture render of the same geometry from it.
//   * workgroups are dealt so that all blocks of a mesh run on one XCD (its face records stay
//     in that XCD's L2).
#include "acfm_raster.h"

#include <type_traits>

namespace acfm {

// Diagnostic event counters (make VARIANT=count EXTRA="-DACFM_DIAG -DACFM_DIAG_COUNT", tools/count_events.py): what a
// launch of the K-nearest forward actually executes -- walk iterations, how many reach each stage, with how many
// live lanes, how many 4-slot blocks of the sorted insertion run.  Not in the shipping build.
#ifdef ACFM_DIAG_COUNT
__device__ unsigned long long g_diag[16];
#define DIAG_ADD(i, v)                                                                              \
  do {                                                                                              \
    const unsigned long long v_ = (unsigned long long)(v);   /* (evaluated by every active lane: v may hold a ballot) */ \
    const unsigned long long m_ = __ballot(true);                                                   \
    if ((int)(threadIdx.x & 63) == (int)__builtin_ctzll(m_)) atomicAdd(&g_diag[i], v_);             \
  } while (0)
#else
#define DIAG_ADD(i, v) do {} while (0)
#endif

// cost count of a block (k_setup, k_order): goes into the stamps of the diagnostic build
__device__ __forceinline__ int block_cost(const RasterWs& ws, int n, int bl, int H) {
  const int blocks = (H + RBLK - 1) / RBLK, tiles = (H + CNT_TILE - 1) / CNT_TILE;
  const int by = bl / blocks, bx = bl % blocks;
  return ws.tile_cnt[((size_t)n * tiles + by * RBLK / CNT_TILE) * tiles + bx * RBLK / CNT_TILE];
}

// ------------------------------------------------------------------------------- tile skeleton
struct Tile {
  int n, tid, wv, lane, yi, xi;
  bool valid, empty, none;  // none: nothing to do for this workgroup
  int sub;                   // >= 0: split role, this wave renders 4x4 pixels (group `sub` of the block) with its four
                             // 16-lane groups taking every fourth candidate each; -1: the whole 8x8 block
  float xf, yf;
  size_t pix;
  float t_xmin, t_xmax, t_ymin, t_ymax;
};

// Workgroup (= one wave) -> entries of the heavy-first order of its XCD group.
// Workgroups are dealt round-robin over the 8 XCDs, so with N % 8 == 0 group g = b % 8 owns the
// meshes n % 8 == g (one XCD's L2 then holds the records of the meshes it renders).  Pure speed:
// any mapping gives the same result.
// A group of `per` entries gets stride = ceil(per / div) workgroups (+ 4 per split slot in front).
// Workgroup j renders the entries j, j + stride, ... that have work (e < n_work: normally just
// one, the order is heavy-first and most of a frame is empty) and, in the forward kernels, first
// stores the constant outputs of the flagged-empty entries n_work + j, n_work + j + stride, ...:
// those stores drain while the block is rendered, and an empty block costs no workgroup dispatch
// (65 536 one-wave workgroups per 64 frames took ~90 us of the chip's dispatcher by themselves).
struct Sched {
  int G, g, per, j0, stride, e_end, n_work, sub;
};
__device__ __forceinline__ Sched make_sched(const RasterWs& ws, int N, int H, bool with_split) {
  Sched s;
  const int tiles = (H + RBLK - 1) / RBLK;
  const int tt = tiles * tiles;
  s.G = (N & 7) == 0 ? 8 : 1;
  s.per = (N / s.G) * tt;
  const int nsplit = with_split ? s.G * ws.split_slots * 4 : 0;
  int b = (int)blockIdx.x;
  s.sub = -1;
  if (b < nsplit) {          // split role: workgroups 4 slot .. 4 slot + 3 of a group take the four 4x4 groups of entry `slot`
    s.g = s.G == 8 ? (b & 7) : 0;
    const int q = s.G == 8 ? (b >> 3) : b;
    s.j0 = q >> 2;
    s.sub = q & 3;
    s.stride = 1;
    s.n_work = ws.n_work[s.g];
    s.e_end = min(s.j0 + 1, s.n_work);
  } else {
    b -= nsplit;
    s.g = s.G == 8 ? (b & 7) : 0;
    s.j0 = s.G == 8 ? (b >> 3) : b;
    s.stride = ((int)gridDim.x - nsplit) / s.G;
    s.n_work = ws.n_work[s.g];
    s.e_end = s.n_work;
  }
  return s;
}

// order entry -> (mesh, first pixel row, first pixel column) of its 8x8 block
__device__ __forceinline__ void entry_block(int eo, const Sched& s, int H, int& n, int& by, int& bx) {
  const int tiles = (H + RBLK - 1) / RBLK;
  const int tt = tiles * tiles;
  const int e = eo & ~ENTRY_FLAGS;
  n = (e / tt) * s.G + s.g;
  const int tl = e % tt;
  by = (tl / tiles) * RBLK; bx = (tl % tiles) * RBLK;
}

__device__ __forceinline__ Tile make_tile(const RasterWs& ws, const Sched& s, int j, int N, int H, bool with_split) {
  Tile t;
  const int tiles = (H + RBLK - 1) / RBLK;
  const int tt = tiles * tiles;
  const int G = s.G, g = s.g, per = s.per;
  t.none = false;
  t.sub = s.sub;
  const int eo = ws.order[(size_t)g * per + j];
  if (t.sub >= 0 && !(eo & ENTRY_SPLIT)) t.none = true;
  if (t.sub < 0 && with_split && (eo & ENTRY_SPLIT)) t.none = true;   // rendered by its four split workgroups
  const int e = eo & ~ENTRY_FLAGS;
  t.empty = (eo & ENTRY_EMPTY) != 0;
  const int n = (e / tt) * G + g, tl = e % tt;
  t.n = n;
  // (opaque to the optimiser: lane-derived addressing stays inside the per-block code instead of
  // being hoisted out of the workgroup's block loop into long-lived registers)
  int tid_ = threadIdx.x;
  asm volatile("" : "+v"(tid_));
  t.tid = tid_; t.wv = 0; t.lane = t.tid & 63;
  const int ty = tl / tiles, tx = tl % tiles;
  // the 8x8 pixels = four 4x4 blocks, one per 16-lane group (= one DPP row); split role: all four
  // 16-lane groups hold the same 4x4 pixels
  const int grp = t.sub >= 0 ? t.sub : (t.lane >> 4), jj = t.lane & 15;
  t.yi = ty * RBLK + (grp >> 1) * 4 + (jj >> 2);
  t.xi = tx * RBLK + (grp & 1) * 4 + (jj & 3);
  t.valid = (t.yi < H) && (t.xi < H);
  t.yf = pix_to_ndc(H - 1 - t.yi, H);
  t.xf = pix_to_ndc(H - 1 - t.xi, H);
  t.pix = ((size_t)n * H + t.yi) * H + t.xi;
  // extent of the block (split role: of the 4x4 group) in NDC (pixel centres; x/y decrease with the pixel index)
  const int ex0 = tx * RBLK + (t.sub >= 0 ? (t.sub & 1) * 4 : 0), ey0 = ty * RBLK + (t.sub >= 0 ? (t.sub >> 1) * 4 : 0);
  const int ext = t.sub >= 0 ? 3 : RBLK - 1;
  t.t_xmax = pix_to_ndc(H - 1 - ex0, H); t.t_xmin = pix_to_ndc(H - 1 - (ex0 + ext), H);
  t.t_ymax = pix_to_ndc(H - 1 - ey0, H); t.t_ymin = pix_to_ndc(H - 1 - (ey0 + ext), H);
  return t;
}

template <int CAP_>
struct CandListT {
  static constexpr int CAP = CAP_;
  float4 box[CAP_], a[CAP_], b[CAP_];
  float4 c[CAP_];    // (z2, denom = area + kEps, refined 1 / denom, face id as bits)
  unsigned char sub[4][CAP_];  // per 16-lane group: candidates meeting its 4x4 pixels (list positions < CAP <= 256)
};


struct Cand {
  float4 box, a, b;
  float2 c;      // (z2, denom = area + kEps)
  float rden;    // refined 1 / denom (k_setup's, the very operations the per-pixel code used to repeat)
  int fid, idx;  // idx: list position (the K-nearest walk reads L.e0 / L.e1[idx] when it reaches the distance stage)
};

template <class LT, class = void> struct has_edge_const : std::false_type {};
template <class LT> struct has_edge_const<LT, std::void_t<decltype(std::declval<LT&>().e0)>> : std::true_type {};

template <class LT>
__device__ __forceinline__ Cand load_cand(const LT& L, int i) {
  Cand r;
  r.box = L.box[i]; r.a = L.a[i]; r.b = L.b[i];
  const float4 c = L.c[i];   // one 16-byte read
  r.c = make_float2(c.x, c.y); r.rden = c.z; r.fid = __float_as_int(c.w); r.idx = i;
  return r;
}

// Which of four pixel blocks (centres (cx0|cx1, cy0|cy1), half extents hx, hy) lie entirely
// farther than r outside one edge line of the triangle (a = x0 y0 x1 y1, b = x2 y2 ..): no pixel
// of such a block is inside the face or within r of it, so the pair can be dropped.  Conservative
// (separating axis on the three edge normals only); r carries a 1e-3 slack over sqrt(blur), far
// above the rounding of the per-pixel distance.  bit0 x0y0, bit1 x1y0, bit2 x0y1, bit3 x1y1.
__device__ __forceinline__ unsigned edge_cull4(const float4 a, const float4 b, float cx0, float cx1,
                                               float cy0, float cy1, float hx, float hy, float r) {
  const float px[3] = {a.x, a.z, a.w}, py[3] = {a.y, b.x, b.y};
  unsigned out = 0u;
#pragma unroll
  for (int e = 0; e < 3; ++e) {
    const int q = (e + 1) % 3, o = (e + 2) % 3;
    float nx = py[q] - py[e], ny = px[e] - px[q];
    const float side = nx * (px[o] - px[e]) + ny * (py[o] - py[e]);
    if (side > 0.f) { nx = -nx; ny = -ny; }  // outward: away from the third vertex
    const float thr2 = r * r * (nx * nx + ny * ny);
    const float ext = fabsf(nx) * hx + fabsf(ny) * hy;
    const float ax0 = nx * (cx0 - px[e]) - ext, ax1 = nx * (cx1 - px[e]) - ext;
    const float ay0 = ny * (cy0 - py[e]), ay1 = ny * (cy1 - py[e]);
    float m;
    m = ax0 + ay0; if (m > 0.f && m * m > thr2) out |= 1u;
    m = ax1 + ay0; if (m > 0.f && m * m > thr2) out |= 2u;
    m = ax0 + ay1; if (m > 0.f && m * m > thr2) out |= 4u;
    m = ax1 + ay1; if (m > 0.f && m * m > thr2) out |= 8u;
  }
  return out;
}

// Second-level cull + walk.  A wave covers 8x8 pixels as four 4x4 blocks, one per 16-lane
// group.  (A) 64 candidates at a time, lane i tests candidate i's box against each of the four
// blocks and the survivors are compacted (one ballot per group) into that group's own sub-list;
// with EDGE_CULL in two steps: (A1) box of the 8x8 block -> the wave's list, (A2) per 4x4 block the
// box and then the edge-line test above, which drops ~17 % of the pairs the boxes keep.  (B) the four groups then walk THEIR OWN lists side by side -- in one iteration the
// groups work on four different faces -- which keeps more lanes busy than walking the union of
// the lists (a 4x4 block meets ~25 faces, the 8x8 block ~41).  body(cand, in_box, ordinal) runs
// for every lane; in_box = the lane has a face this iteration and its pixel is inside the face's box.
// EDGE_CULL pays for itself only where a kept pair is expensive (the K-nearest forward walk:
// -4.5 %); the backward and nearest-face walks drop most pairs on a cheap key / depth compare and
// were measured slower with it (+7 %, +2 %).
// SHARE (the backward): the four sub-lists are of different lengths (50 of 64 lanes have a face in an average
// iteration), and a group that has run out used to idle until the longest list ended.  The groups are paired --
// longest with shortest, the two middle ones -- and the shorter group of a pair, once through its own list, takes the
// faces of its partner's list from the END, for the PARTNER's pixels (lane j of the helper stands in for lane j of the
// partner: same face for the 16 lanes of a row, so the row reduction of the gradient is unchanged); the pair then needs
// ceil((n_A + n_B) / 2) iterations instead of n_A.  prep(partner_lane) is called once per walk with the lane whose
// pixel this lane takes over when it helps (-1: never); body gets (cand, in_box, ordinal, helping, xf, yf).
struct NoPrep { __device__ __forceinline__ void operator()(int) const {} };
template <bool EDGE_CULL, bool SHARE = false, class LT, class Body, class Prep = NoPrep>
__device__ __forceinline__ void walk_wave(LT& L, const Tile& t, int H, int list_n, float blur,
                                          unsigned char* wl /* [2 CAP], EDGE_CULL only */,
                                          Body&& body, Prep&& prep = NoPrep()) {
  const int by = (t.yi & ~7), bx = (t.xi & ~7);
  const int grp = t.lane >> 4;
  // NDC extents (pixel centres) of the four 4x4 blocks: x by column pair, y by row pair
  const float xa0 = pix_to_ndc(H - 1 - bx, H), xi0 = pix_to_ndc(H - 1 - (bx + 3), H);
  const float xa1 = pix_to_ndc(H - 1 - (bx + 4), H), xi1 = pix_to_ndc(H - 1 - (bx + 7), H);
  const float ya0 = pix_to_ndc(H - 1 - by, H), yi0 = pix_to_ndc(H - 1 - (by + 3), H);
  const float ya1 = pix_to_ndc(H - 1 - (by + 4), H), yi1 = pix_to_ndc(H - 1 - (by + 7), H);
  static_assert(LT::CAP <= 256, "sub-list entries are bytes");
  unsigned char* sub0 = L.sub[0];
  const unsigned long long lt = (1ull << t.lane) - 1ull;
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
  const bool split = t.sub >= 0;
  if (split) {
    // split role: the list was binned against this 4x4 group already; 16-lane group s takes the
    // candidates s, s+4, s+8, ... (no sub-lists)
    n0 = (list_n + 3) >> 2; n1 = (list_n + 2) >> 2; n2 = (list_n + 1) >> 2; n3 = list_n >> 2;
  } else if constexpr (!EDGE_CULL) {
    // one pass: lane i tests candidate i's box against the four 4x4 blocks
    for (int base = 0; base < list_n; base += 64) {
      const int c = base + t.lane;
      bool hx0 = false, hx1 = false, hy0 = false, hy1 = false;
      if (c < list_n) {
        const float4 b = L.box[c];
        hx0 = !((xi0 > b.y) | (xa0 < b.x)); hx1 = !((xi1 > b.y) | (xa1 < b.x));
        hy0 = !((yi0 > b.w) | (ya0 < b.z)); hy1 = !((yi1 > b.w) | (ya1 < b.z));
      }
      const unsigned long long b0 = __ballot(hx0 & hy0), b1 = __ballot(hx1 & hy0);
      const unsigned long long b2 = __ballot(hx0 & hy1), b3 = __ballot(hx1 & hy1);
      if (hx0 & hy0) sub0[0 * LT::CAP + n0 + __popcll(b0 & lt)] = (unsigned char)c;
      if (hx1 & hy0) sub0[1 * LT::CAP + n1 + __popcll(b1 & lt)] = (unsigned char)c;
      if (hx0 & hy1) sub0[2 * LT::CAP + n2 + __popcll(b2 & lt)] = (unsigned char)c;
      if (hx1 & hy1) sub0[3 * LT::CAP + n3 + __popcll(b3 & lt)] = (unsigned char)c;
      n0 += __popcll(b0); n1 += __popcll(b1); n2 += __popcll(b2); n3 += __popcll(b3);
    }
  } else {
    // (A1) box of the whole 8x8 block -> the wave's list
    int nw = 0;
    for (int base = 0; base < list_n; base += 64) {
      const int c = base + t.lane;
      bool hit = false;
      if (c < list_n) {
        const float4 b = L.box[c];
        hit = !((xi1 > b.y) | (xa0 < b.x) | (yi1 > b.w) | (ya0 < b.z));
      }
      const unsigned long long bw = __ballot(hit);
      if (hit) wl[nw + __popcll(bw & lt)] = (unsigned char)c;
      nw += __popcll(bw);
    }
    if (nw == 0) return;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // (A1') front to back, roughly: the wave's list is dealt into 8 depth classes (nearest vertex of
    // the face, classes between the block's nearest and farthest) by a counting sort with ballots.
    // Results never depend on the order of the candidates, the cost of the walk does: a face that
    // arrives after the nearer ones enters a pixel's sorted list near its end, the insertion
    // skips the leading 4-slot blocks it cannot touch, and once a list is full the faces behind it
    // fail the depth test before their edge distances are computed.
    if (nw > 8) {
      static_assert(LT::CAP <= 128, "two list entries per lane");
      const int i0 = t.lane, i1 = t.lane + 64;
      const int c0 = i0 < nw ? (int)wl[i0] : 0, c1 = i1 < nw ? (int)wl[i1] : 0;
      const float INF = __builtin_inff();
      const float z0 = i0 < nw ? min3f(L.b[c0].z, L.b[c0].w, L.c[c0].x) : INF;
      const float z1 = i1 < nw ? min3f(L.b[c1].z, L.b[c1].w, L.c[c1].x) : INF;
      const float zlo = wave_min(fminf(z0, z1));
      const float zhi = wave_max(fmaxf(i0 < nw ? z0 : -INF, i1 < nw ? z1 : -INF));
      const float sc = 8.0f / fmaxf(zhi - zlo, 1e-12f);
      const int b0 = i0 < nw ? min(7, (int)((z0 - zlo) * sc)) : -1;
      const int b1 = i1 < nw ? min(7, (int)((z1 - zlo) * sc)) : -1;
      unsigned char* wl2 = wl + LT::CAP;
      int base = 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const unsigned long long m0 = __ballot(b0 == c), m1 = __ballot(b1 == c);
        if (b0 == c) wl2[base + __popcll(m0 & lt)] = (unsigned char)c0;
        if (b1 == c) wl2[base + __popcll(m0) + __popcll(m1 & lt)] = (unsigned char)c1;
        base += __popcll(m0) + __popcll(m1);
      }
      wl = wl2;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    // (A2) per 4x4 block: box, then the edge-line test
    const float cx0 = 0.5f * (xa0 + xi0), cx1 = 0.5f * (xa1 + xi1);
    const float cy0 = 0.5f * (ya0 + yi0), cy1 = 0.5f * (ya1 + yi1);
    const float hx = 0.5f * (xa0 - xi0), hy = 0.5f * (ya0 - yi0);
    const float r_cull = sqrtf(blur) * 1.001f;
    for (int base = 0; base < nw; base += 64) {
      const int i = base + t.lane;
      bool k0 = false, k1 = false, k2 = false, k3 = false;
      int c = 0;
      if (i < nw) {
        c = wl[i];
        const float4 b = L.box[c];
        const bool hx0 = !((xi0 > b.y) | (xa0 < b.x)), hx1 = !((xi1 > b.y) | (xa1 < b.x));
        const bool hy0 = !((yi0 > b.w) | (ya0 < b.z)), hy1 = !((yi1 > b.w) | (ya1 < b.z));
        const unsigned far = edge_cull4(L.a[c], L.b[c], cx0, cx1, cy0, cy1, hx, hy, r_cull);
        k0 = hx0 & hy0 & !(far & 1u); k1 = hx1 & hy0 & !(far & 2u);
        k2 = hx0 & hy1 & !(far & 4u); k3 = hx1 & hy1 & !(far & 8u);
      }
      const unsigned long long b0 = __ballot(k0), b1 = __ballot(k1);
      const unsigned long long b2 = __ballot(k2), b3 = __ballot(k3);
      if (k0) sub0[0 * LT::CAP + n0 + __popcll(b0 & lt)] = (unsigned char)c;
      if (k1) sub0[1 * LT::CAP + n1 + __popcll(b1 & lt)] = (unsigned char)c;
      if (k2) sub0[2 * LT::CAP + n2 + __popcll(b2 & lt)] = (unsigned char)c;
      if (k3) sub0[3 * LT::CAP + n3 + __popcll(b3 & lt)] = (unsigned char)c;
      n0 += __popcll(b0); n1 += __popcll(b1); n2 += __popcll(b2); n3 += __popcll(b3);
    }
  }
  const int n_max = max(max(n0, n1), max(n2, n3));
  if (n_max == 0) return;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const int my_n = (grp == 0) ? n0 : (grp == 1) ? n1 : (grp == 2) ? n2 : n3;
  const unsigned char* sub = sub0 + grp * LT::CAP;
  if constexpr (SHARE) {
    if (!split) {
      // pairs (wave-uniform): a = the longest list, d = the shortest, b >= c the other two
      int a = 0, na = n0;
      if (n1 > na) { a = 1; na = n1; }
      if (n2 > na) { a = 2; na = n2; }
      if (n3 > na) { a = 3; na = n3; }
      int d = a == 0 ? 1 : 0, nd = a == 0 ? n1 : n0;
      if (a != 1 && n1 < nd) { d = 1; nd = n1; }
      if (a != 2 && n2 < nd) { d = 2; nd = n2; }
      if (a != 3 && n3 < nd) { d = 3; nd = n3; }
      int b = -1, c = -1;
#pragma unroll
      for (int g = 0; g < 4; ++g)
        if (g != a && g != d) { if (b < 0) b = g; else c = g; }
      int nb = b == 0 ? n0 : b == 1 ? n1 : b == 2 ? n2 : n3, nc = c == 0 ? n0 : c == 1 ? n1 : c == 2 ? n2 : n3;
      if (nc > nb) { const int tg = b; b = c; c = tg; const int tn = nb; nb = nc; nc = tn; }
      const int xa = (na + nd + 1) >> 1, xb = (nb + nc + 1) >> 1;   // the longer group of a pair keeps its first x faces
      // per lane: own faces [0, own_n), then faces [h0, h0 + h_n) of group `pg`'s list for that group's pixels
      const int own_n = grp == a ? xa : grp == b ? xb : my_n;
      const int pg = grp == d ? a : grp == c ? b : -1;
      const int h0 = grp == d ? xa : xb;
      const int h_n = grp == d ? na - xa : grp == c ? nb - xb : 0;
      const int n_it = max(xa, xb);
      const int jj = t.lane & 15;
      prep(pg >= 0 ? pg * 16 + jj : -1);
      // the partner's pixel (4x4 block pg of the 8x8 block, same position inside it)
      const int pyi = by + ((pg >= 0 ? pg : grp) >> 1) * 4 + (jj >> 2), pxi = bx + ((pg >= 0 ? pg : grp) & 1) * 4 + (jj & 3);
      const float pxf = pix_to_ndc(H - 1 - pxi, H), pyf = pix_to_ndc(H - 1 - pyi, H);
      const bool pvalid = (pyi < H) && (pxi < H);
      const unsigned char* hsub = sub0 + (pg >= 0 ? pg : grp) * LT::CAP + h0;
      for (int i = 0; i < n_it; ++i) {
        const bool own = i < own_n;
        const bool help = !own && (i - own_n) < h_n;
        const int ci = own ? (int)sub[i] : (help ? (int)hsub[i - own_n] : 0);
        const Cand cur = load_cand(L, ci);
        const float exf = help ? pxf : t.xf, eyf = help ? pyf : t.yf;
        const bool have = own || (help && pvalid);
        const bool in_box = have && !((exf > cur.box.y) | (exf < cur.box.x) | (eyf > cur.box.w) | (eyf < cur.box.z));
        DIAG_ADD(3, 1); DIAG_ADD(4, __popcll(__ballot(in_box))); DIAG_ADD(10, __popcll(__ballot(have)));
        DIAG_ADD(12, __popcll(__ballot(have) & 0x0001000100010001ull));
        body(cur, in_box, i, help, exf, eyf);
      }
      return;
    }
  }
  // a group that has run out of faces (or has none) keeps loading its last (or the tile's
  // first) record: harmless, the lanes are masked by `have`.  (Prefetching the next record one
  // iteration ahead was measured: +16 VGPRs, no change in time.  Reading only the list position of
  // the next candidate one iteration ahead -- one LDS round trip per iteration instead of two -- was
  // measured too (64 frames, A/B on one box, twice): 192.7 / 193.4 us with it, 189.9 / 192.5 without.)
  const int last = max(my_n - 1, 0);
  if constexpr (SHARE) prep(-1);
  for (int i = 0; i < n_max; ++i) {
    const int li = min(i, last);
    const Cand cur = load_cand(L, my_n > 0 ? (split ? 4 * li + grp : (int)sub[li]) : 0);
    const bool have = i < my_n;
    const bool in_box = have &&
        !((t.xf > cur.box.y) | (t.xf < cur.box.x) | (t.yf > cur.box.w) | (t.yf < cur.box.z));
    DIAG_ADD(3, 1); DIAG_ADD(4, __popcll(__ballot(in_box))); DIAG_ADD(10, __popcll(__ballot(have)));
    DIAG_ADD(12, __popcll(__ballot(have) & 0x0001000100010001ull));   // (group, face) pairs walked
    if constexpr (SHARE) body(cur, in_box, i, false, t.xf, t.yf);
    else body(cur, in_box, i);
  }
}

// Bins the faces of mesh t.n against the wave's 8x8 block and calls walk(count) whenever the LDS
// list is FULL (count == LT::CAP) or complete.  The faces come from the bitmask of the block's 16x16
// coarse tile (k_setup): lane i expands mask word i into the wave's face-id list (ascending), then
// 64 ids per round lane i tests face i's box; survivors are compacted with one ballot, face
// order kept.  A round appends only the survivors that fit; when some do not, the id cursor is put
// back to the first of them and the round after the walk starts there (its box is loaded again: no
// per-lane state lives through the walk).  Every walk but a block's last therefore runs on a full
// list: a walk's shell (sub-list passes, depth deal, barriers, pairing, flush) is paid
// ceil(candidates / CAP) times per block, and the 16-lane groups are balanced over CAP candidates
// at a time.  Progress: a round either takes 64 ids or fills the list and takes at least one.
// No barriers: the workgroup is one wave.
__device__ __forceinline__ int wave_inclusive_scan(int x, int lane) {
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// The mesh-box early-out in front of the mask loads looks redundant beside k_order's empty flag, but the flag comes
// from counts per 16x16 pixels: without the test the K = 20 kernels measured 6-7 us slower each (blocks next to the
// mesh that bin a mask row to find nothing), the K = 1 kernel 2 us faster.
template <class LT, class Walk>
__device__ __forceinline__ void bin_and_walk(const RasterWs& ws, const Tile& t, int F, int H, LT& L,
                                             fl_t* s_fl /* [FLCAP] */, float box_shrink, Walk&& walk) {
  if (t.empty) return;  // flagged by k_order: no face box near this block
  {
  // the mesh's box: the four slices' boxes (the usual case), or slot 0 where k_order joined 8 or 16 of them
  float4 mb = ws.mbox[(size_t)t.n * ws.slices];
  if (ws.slices == 4) {
#pragma unroll
    for (int i = 1; i < 4; ++i) {
      const float4 m2 = ws.mbox[(size_t)t.n * 4 + i];
      mb.x = fminf(mb.x, m2.x); mb.y = fmaxf(mb.y, m2.y); mb.z = fminf(mb.z, m2.z); mb.w = fmaxf(mb.w, m2.w);
    }
  }
  if (t.t_xmin > mb.y || t.t_xmax < mb.x || t.t_ymin > mb.w || t.t_ymax < mb.z) return;
  }
  const unsigned long long lt = (1ull << t.lane) - 1ull;
  const int ctiles = (H + CTILE - 1) / CTILE, words = (F + 63) / 64;
  const int cty = (t.yi & ~7) / CTILE, ctx = (t.xi & ~7) / CTILE;
  const unsigned long long* mrow = reinterpret_cast<const unsigned long long*>(ws.cmask) +
                                   ((size_t)t.n * ctiles * ctiles + (size_t)cty * ctiles + ctx) * words;
  int list_n = 0;
  // one loop with a single walk() site (the walk body is large and holds the per-pixel lists in
  // registers: a second inlined copy costs registers): refill the id list from the next mask
  // chunk when it runs dry, take up to 64 ids, test + append what fits, walk when the list is full
  // or everything has been appended.  (s_fl is refilled only once i0 >= total, so a cursor that
  // was put back never reads a refilled list.)
  int w0 = -64, total = 0, i0 = 0, f0 = 0, fe = 0;
  bool direct = false, done = false;
#pragma unroll 1
  for (;;) {
#pragma unroll 1
    while (!done && !(direct ? f0 < fe : i0 < total)) {
      w0 += 64;
      if (w0 >= words) { done = true; break; }
      unsigned long long m = (w0 + t.lane < words) ? mrow[w0 + t.lane] : 0ull;
      const int cnt = __popcll(m);
      const int incl = wave_inclusive_scan(cnt, t.lane);
      total = __builtin_amdgcn_readlane(incl, 63);
      i0 = 0;
      direct = total > FLCAP;  // a coarse tile crowded beyond the id list: test these 4096 faces directly
      if (direct) {
        f0 = w0 * 64; fe = min(F, (w0 + 64) * 64); total = 0;
      } else if (total > 0) {
        int pos = incl - cnt;
        const int fbase = (w0 + t.lane) * 64;
#pragma unroll 1
        while (m != 0ull) {
          s_fl[pos++] = (fl_t)(fbase + (int)__ffsll((long long)m) - 1);
          m &= m - 1ull;
        }
        wave_lds_sync();
      }
    }
    if (!done) {
      int f;
      if (direct) { f = (f0 + t.lane < fe) ? f0 + t.lane : -1; f0 += RT; }
      else { f = (i0 + t.lane < total) ? (int)s_fl[i0 + t.lane] : -1; i0 += RT; }
      bool pass = false;
      float4 b = make_float4(0, 0, 0, 0);
      if (f >= 0) {
        // (the box first, the rest of the record only for a face that passes: loading the whole 64-byte record
        // up front removes a dependent gather but measured +2.5 us on the K = 1 kernel and +7 us on the K = 20
        // one: the binning is bound by gather transactions, not by their latency)
        b = ws.rec[(size_t)t.n * F + f].box;
        // a workspace shared with a render of larger blur: tighten the (margin-expanded) box; a
        // degenerate face's (inf, -inf, inf, -inf) stays what it is
        b.x += box_shrink; b.y -= box_shrink; b.z += box_shrink; b.w -= box_shrink;
        pass = !(t.t_xmin > b.y || t.t_xmax < b.x || t.t_ymin > b.w || t.t_ymax < b.z);
      }
      const unsigned long long bal = __ballot(pass);
      const int pos = list_n + __popcll(bal & lt);
      if (pass && pos < LT::CAP) {
        const size_t o = (size_t)t.n * F + f;
        L.box[pos] = b;
        L.a[pos] = ws.rec[o].a;
        L.b[pos] = ws.rec[o].b;
        const float4 c4 = ws.rec[o].c;
        L.c[pos] = make_float4(c4.x, c4.z, c4.w, __int_as_float(f));
        if constexpr (has_edge_const<LT>::value) { L.e0[pos] = ws.rec[o].e0; L.e1[pos] = ws.rec[o].e1; }
      }
      list_n += __popcll(bal);
      if (list_n > LT::CAP) {
        // more survivors than room: the list is full, the cursor goes back to the first survivor that did not fit and
        // the next round tests the ids from there again (a few box loads; nothing of the round lives through the walk)
        const int back = RT + 1 - (int)__ffsll((long long)__ballot(pass && pos >= LT::CAP));
        if (direct) f0 -= back; else i0 -= back;
        list_n = LT::CAP;
      }
    }
    if (list_n == LT::CAP || (done && list_n > 0)) {
      wave_lds_sync();
      walk(list_n);
      wave_lds_sync();
      list_n = 0;
    }
    if (done) break;
  }
}

// The same with the per-edge constants of the candidate: E0 = (|e01|^2, |e02|^2, r01, r02),
// E1 = (|e12|^2, r12, degenerate flag, -).  Operation for operation point_line_dist / point_line_dist2 minus what does
// not depend on the pixel; a face with a degenerate edge (flag) must take test_face_dist (its distance-to-endpoint branch).
__device__ __forceinline__ bool test_face_dist_e(float xf, float yf, const float4& A, const float4& B, const float4& E0,
                                                 const float4& E1, float blur, bool inside, Hit& h, float* tpar = nullptr) {
  const float x0 = A.x, y0 = A.y, x1 = A.z, x2 = A.w, y1 = B.x, y2 = B.y;
  {
    const v2f ax = {x0, x0}, ay = {y0, y0}, bx = {A.z, A.w}, by = {B.x, B.y};
    const v2f l2 = {E0.x, E0.y}, r = {E0.z, E0.w};
    const v2f bax = bx - ax, bay = by - ay;
    const v2f num = bax * (xf - ax) + bay * (yf - ay);
    v2f t = num * r;
    t = fma2(fma2(-l2, t, num), r, t);
    t = fma2(fma2(-l2, t, num), r, t);
    t.x = fminf(fmaxf(t.x, 0.0f), 1.0f); t.y = fminf(fmaxf(t.y, 0.0f), 1.0f);
    const v2f qx = ax + t * bax, qy = ay + t * bay;
    const v2f dx = qx - xf, dy = qy - yf;
    const v2f d = dx * dx + dy * dy;
    h.d01 = d.x; h.d02 = d.y;
    if (tpar) { tpar[0] = t.x; tpar[1] = t.y; }
  }
  {
    const float bax = x2 - x1, bay = y2 - y1;
    float t = div_by(bax * (xf - x1) + bay * (yf - y1), E1.x, E1.y);
    t = fminf(fmaxf(t, 0.0f), 1.0f);
    if (tpar) tpar[2] = t;
    const float qx = x1 + t * bax, qy = y1 + t * bay;
    const float dx = qx - xf, dy = qy - yf;
    h.d12 = dx * dx + dy * dy;
  }
  const float d = fminf(fminf(h.d01, h.d02), h.d12);
  h.sd = inside ? -d : d;
  return inside || !(d >= blur);
}

// blend probability sigmoid(-sd/sigma) = 1 / (1 + 2^(sd * log2(e)/sigma)) as mul + v_exp_f32 + add +
// v_rcp_f32 (4 instructions; the IEEE division sd/sigma + library expf + reciprocal were 33, most of them
// half-rate selects / compares -- tools/ubench/valu_rates.hip).  Error budget against the oracle's exact
// expf: the product rounds once (|arg| <= 13.3 up to the blur radius: 5.5e-7 relative on 2^arg where
// p ~ 1e-4, nothing where p ~ 0.5), v_exp_f32 and v_rcp_f32 are 1 ulp each: |dp| <= p (1 - p) 2e-7 + 6e-8 p
// <= 1e-7 per face; measured on the parity sweep: masks within 4e-7 (bar 1e-6).  Inside faces (sd < 0, far
// from the edge) underflow to p = 1 exactly like expf does.  Face ids never depend on p.  (The library form,
// sigmoid_neg of acfm_common.h, stays where a pixel evaluates it once: k1_finish, acfm_shade.hip.)
__device__ __forceinline__ float sigmoid_scale(float sigma) {   // wave-uniform: kept in an SGPR
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(1.44269504088896341f / sigma)));
}
__device__ __forceinline__ float sigmoid_neg_fast(float sd, float sigma, float scale) {
  return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(sd * scale));
}

// (depth, face) key: pz >= 0 so its bit pattern orders like the float; +0.0f folds -0.0 into
// +0.0.  Smaller face id wins a depth tie.
__device__ __forceinline__ unsigned long long make_key(float pz, int fid) {
  return ((unsigned long long)__float_as_uint(pz + 0.0f) << 32) | (unsigned)fid;
}

// ------------------------------------------------------------------------------- forward
__device__ __forceinline__ void mark_visible(const RasterWs& ws, const FwdOut& out, int n, int F, int f) {
  const int4 vi = ws.vidx[(size_t)n * F + f];
  uint8_t* v = out.vis + (size_t)n * out.V;
  v[vi.x] = 1; v[vi.y] = 1; v[vi.z] = 1;
}

// Insertion of (x, xq) into the sorted register list, four slots at a time.
// `lim` (wave-uniform) bounds the number of faces any lane of the wave can hold so far: slots
// at or beyond it are still empty in every lane, so blocks that lie wholly beyond it are skipped
// with scalar branches while every register index stays a compile-time constant.
//
// SHIFT form, top block first (called as shift_insert_block<K, (K - 1) / 4>).  With P_k = (x < key[k]) the new list is
//   key'[k] = P_k ? (P_{k-1} ? key[k-1] : x) : key[k]        (P_{-1} = false; sorted list: P_{k-1} implies P_k)
// evaluated for k descending, in place: slot k reads only the OLD slots k and k-1 and x itself never changes.
// Per slot one 64-bit compare + six selects.  The walk is top-down, so the first block no lane's element enters ENDS
// the insertion (everything below holds smaller keys).  Lanes that do not insert are masked by exec (their compare
// bits are 0).  The compare goes through the wave mask + inverse ballot: a plain `x < key[k]` lets the two selects of
// a pair be canonicalised into a 64-bit umin / umax, which the backend expands into two compares plus register copies.
// (It replaced a bubble form -- compare-exchange from slot 0 upwards, carrying the displaced element -- which cost
// 4 v_mov_b64 + 4 v_mov_b32 of register copies per 4-slot block and tested every block below the insertion point.)
__device__ __forceinline__ unsigned long long key_lt_mask(unsigned long long x, unsigned long long k) {
  return __builtin_amdgcn_uicmpl(x, k, 36 /* ICMP_ULT */);   // one v_cmp_lt_u64 into an SGPR pair (lanes off: 0)
}
template <int K, int B>   // block B = slots [4B, min(4B + 4, K)), called for B = top .. 0
__device__ __forceinline__ void shift_insert_block(unsigned long long (&key)[K], float (&q)[K], const unsigned long long x,
                                                   const float xq, int lim) {
  constexpr int LO = 4 * B, HI = (LO + 4 < K ? LO + 4 : K);
  // (the list holds at most lim entries after this insertion: slots >= lim stay empty in every lane.  `lim` counts the
  // faces WALKED, a loose bound on the faces a pixel KEPT; also testing whether slot LO - 1 is still empty in every
  // inserting lane measured 197.1 us against 197.5 without, A/B on one box: within noise, and it costs three registers)
  // (a flag and its negation, not `if (lim > LO)`: the two compile to different code for K >= 8 -- the direct form came
  // out ~30 instructions shorter per kernel, unmeasured -- and this is the form the recorded timings belong to)
  bool beyond = lim <= LO;
  if (!beyond) {
    DIAG_ADD(9, 1);
    unsigned long long pk = key_lt_mask(x, key[HI - 1]);
    if (pk == 0ull) return;            // no lane's element enters this block, hence none enters a lower one
    DIAG_ADD(8, 1);
#pragma unroll
    for (int k = HI - 1; k >= LO; --k) {
      const unsigned long long pm = k > 0 ? key_lt_mask(x, key[k > 0 ? k - 1 : 0]) : 0ull;
      const bool below = __builtin_amdgcn_inverse_ballot_w64(pm);   // the element goes below slot k: slot k takes k-1's
      const bool here = __builtin_amdgcn_inverse_ballot_w64(pk);    // slot k changes at all
      const unsigned long long sk = below ? key[k > 0 ? k - 1 : 0] : x;
      const float sq = below ? q[k > 0 ? k - 1 : 0] : xq;
      key[k] = here ? sk : key[k];
      q[k] = here ? sq : q[k];
      pk = pm;
    }
  }
  if constexpr (B > 0) shift_insert_block<K, B - 1>(key, q, x, xq, lim);
}

// LDS of a forward workgroup (one wave).  The nearest-face kernels keep a 64-slot candidate list
// (5.5 KB: the register budget, not LDS, then bounds the waves per SIMD -- measured on the
// backward: 13.8 KB -> 6.9 KB per wave = 292 -> 256 us); the K-nearest kernels are register-bound
// at 4 waves per SIMD and get 10 240 B each (16 one-wave workgroups per CU): with every slot of pix_to_face stored
// (k_out = K) that is exactly the staging area of the block's ids, a union with the lists.
// (The per-pixel-list forward walk of round 2 lives in tools/variants/fwd_v2_per_pixel_lists.inc.)
//
// Per-edge constants (K-nearest kernels): a candidate carries, besides its record, what the exact per-pixel distance
// test needs per EDGE and not per pixel -- |e|^2 and the refined reciprocal 1/|e|^2 of the three edges (operands of
// the IEEE-exact division of point_line_dist) and a flag for an edge with |e|^2 <= kEps -- computed once per face by
// k_setup with the very operations the walk used to repeat for every (pixel, face) pair: two more 16-byte LDS
// entries per candidate (32 B), ~33 instruction slots fewer per walk iteration, bit-identical values.
// K-nearest candidate list: 96 B x 88 + sub-lists + id list + cull lists = 10 208 B <= 10 240.  bin_and_walk fills it to
// the last slot before a walk (a block with more than 88 candidates walks ceil(n / 88) times), so the limits of
// walk_wave -- byte-sized sub-list entries, two list entries per lane in the depth deal (CAP <= 128) -- are met by
// every full walk, not only by rare overflows.
constexpr int FWD_CAP = 88;
template <int CAP_>
struct CandListET : CandListT<CAP_> {
  float4 e0[CAP_];   // FaceRec::e0: (|e01|^2, |e02|^2, 1/|e01|^2, 1/|e02|^2)   -- the pair the packed pipe evaluates together
  float4 e1[CAP_];   // FaceRec::e1: (|e12|^2, 1/|e12|^2, degenerate flag, -)
};
template <int CAP, int MIN_BYTES, bool EDGE>
struct FwdLdsT {
  struct Lists {
    typename std::conditional<EDGE, CandListET<CAP>, CandListT<CAP>>::type L;
    fl_t fl[FLCAP];
    unsigned char wl[2 * CAP];   // the wave's list of the edge cull, and the same in depth order (list positions < CAP <= 256)
  };
  union {
    Lists s;
    char stage[MIN_BYTES > 16 ? MIN_BYTES : 16];   // the block's K ids in image order (the lists are dead by then)
  };
};
template <int K> using FwdLdsK = FwdLdsT<(K > 1 ? FWD_CAP : 64), (K > 1 ? 64 * K * 8 : 0), (K > 1)>;
static_assert(sizeof(FwdLdsK<20>) <= 10240, "the K = 20 forward runs 16 one-wave workgroups per CU: 10 240 B of LDS each");


// Constant outputs of a flagged-empty 8x8 block (no face box comes near it): exactly what
// fwd_block leaves for a block without candidates.  Lane i owns pixel (i / 8, i % 8) of the block;
// the K ids of the soft kernel go out as 16-byte pieces in image order (8 rows of 64 K bytes).
// The K-slot pix_to_face stores (160 B per pixel at K = 20: whole lines, never read by this library) go out
// non-temporal: -7 us on the K = 20 forward.  The 4-byte-per-pixel planes must NOT (non-temporal st_real / st_face
// measured 75 -> 123 us on the texture forward): a block row of such a plane is a 32-byte fragment and the four
// fragments of a line meet in L2.
#define P2F_STORE(ptr, val) __builtin_nontemporal_store((val), (ptr))
template <int K, bool TEX>
__device__ __forceinline__ void fwd_fill_block(const FwdOut& out, int n, int by, int bx, int H, int lane) {
  const int yi = by + (lane >> 3), xi = bx + (lane & 7);
  const bool valid = (yi < H) && (xi < H);
  const size_t pix = ((size_t)n * H + yi) * H + xi;
  if constexpr (K == 1) {
    if (TEX && out.lpart && lane == 0) {
      const int tiles = (H + RBLK - 1) / RBLK;
      out.lpart[(((size_t)n * tiles + by / RBLK) * tiles + bx / RBLK) * 4] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (!valid) return;
    st_face(out.p2f, pix, -1, out.h16);
    if (TEX) {
      const size_t HW = (size_t)H * H;
      const size_t io = (size_t)n * 3 * HW + (size_t)yi * H + xi;
      st_real(out.imgs, io, 0.f, out.h16); st_real(out.imgs, io + HW, 0.f, out.h16); st_real(out.imgs, io + 2 * HW, 0.f, out.h16);
      st_real(out.sil, pix, 0.f, out.h16);
      out.tidx[pix] = -1;
    }
  } else {
    if (valid) {
      // (kth is left alone: the backward reads it only where mask != 0, and mask is 0 on this whole block)
      st_real(out.mask, pix, 0.0f, out.h16);
      if (out.kout == 1) st_face(out.p2f, pix, -1, out.h16);
      if (out.pf_imgs) {
        const size_t HW = (size_t)H * H, io = (size_t)n * 3 * HW + (size_t)yi * H + xi;
        out.pf_imgs[io] = 0.f; out.pf_imgs[io + HW] = 0.f; out.pf_imgs[io + 2 * HW] = 0.f;
        out.pf_sil[pix] = 0.f; out.pf_tidx[pix] = -1; out.pf_p2f[pix] = -1;
      }
    }
    if (out.lpart && lane < 4) {   // mask = 0 on the whole block: nothing beyond the finish kernel's sum of gt
      const int tiles = (H + RBLK - 1) / RBLK;
      out.lpart[(((size_t)n * tiles + by / RBLK) * tiles + bx / RBLK) * 4 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (out.kout == 1) return;
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    constexpr int CH = K / 2;
    ll2 v; v.x = -1; v.y = -1;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = i * 64 + lane;             // piece index: 8 rows x (8 pixels x CH pieces)
      const int r = c / (8 * CH), off = c % (8 * CH);
      if (by + r < H && bx + off / CH < H)
        P2F_STORE(&reinterpret_cast<ll2*>(reinterpret_cast<int64_t*>(out.p2f) + (((size_t)n * H + by + r) * H + bx) * K)[off], v);
    }
  }
}

// The same for images whose side is a multiple of 8 (every block whole), which is where the fills matter: 80 % of
// the blocks of a batch are empty and the generic routine above spends ~130 VALU instructions per block, a third of
// them 64-bit multiplies, on addresses that differ from block to block only by a wave-uniform base.  Here every
// lane's byte offsets inside a block are computed once per workgroup (FillLane) and a block costs one scalar base
// per output plus the stores (global_store with an SGPR base and a VGPR offset).
template <int K>
struct FillLane {
  unsigned pix;                        // (lane / 8) * H + lane % 8: the lane's pixel inside the block
  unsigned piece[K > 1 ? K / 2 : 1];   // K > 1: byte offset of the lane's i-th 16-byte piece of the K-slot id rows
};
template <int K>
__device__ __forceinline__ FillLane<K> make_fill_lane(int H, int lane) {
  FillLane<K> f;
  f.pix = (unsigned)((lane >> 3) * H + (lane & 7));
  if constexpr (K > 1) {
    constexpr int CH = K / 2;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = i * 64 + lane;             // piece index: 8 rows x (8 pixels x CH pieces)
      const int r = c / (8 * CH), off = c % (8 * CH);
      f.piece[i] = (unsigned)(r * H * K * 8 + off * 16);
    }
  } else {
    f.piece[0] = 0;
  }
  return f;
}
template <int K, bool TEX>
__device__ __forceinline__ void fwd_fill_block_whole(const FwdOut& out, int n, int by, int bx, int H, int lane,
                                                     const FillLane<K>& fl) {
  // wave-uniform: first pixel of the block, and the tiles index of its partial-sum record
  const size_t pix0 = ((size_t)n * H + by) * H + bx;
  const size_t pix = pix0 + fl.pix;
  if constexpr (K == 1) {
    if (TEX && out.lpart && lane == 0) {
      const int tiles = H / RBLK;
      out.lpart[(((size_t)n * tiles + by / RBLK) * tiles + bx / RBLK) * 4] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    st_face(out.p2f, pix, -1, out.h16);
    if (TEX) {
      const size_t HW = (size_t)H * H;
      const size_t io = pix + (size_t)n * 2 * HW;   // [N,3,H,W]: n 3 HW + y W + x
      st_real(out.imgs, io, 0.f, out.h16); st_real(out.imgs, io + HW, 0.f, out.h16); st_real(out.imgs, io + 2 * HW, 0.f, out.h16);
      st_real(out.sil, pix, 0.f, out.h16);
      out.tidx[pix] = -1;
    }
  } else {
    st_real(out.mask, pix, 0.0f, out.h16);   // (kth: see fwd_fill_block)
    if (out.kout == 1) st_face(out.p2f, pix, -1, out.h16);
    if (out.pf_imgs) {
      const size_t HW = (size_t)H * H, io = pix + (size_t)n * 2 * HW;
      out.pf_imgs[io] = 0.f; out.pf_imgs[io + HW] = 0.f; out.pf_imgs[io + 2 * HW] = 0.f;
      out.pf_sil[pix] = 0.f; out.pf_tidx[pix] = -1; out.pf_p2f[pix] = -1;
    }
    if (out.lpart && lane < 4) {   // mask = 0 on the whole block: nothing beyond the finish kernel's sum of gt
      const int tiles = H / RBLK;
      out.lpart[(((size_t)n * tiles + by / RBLK) * tiles + bx / RBLK) * 4 + lane] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (out.kout == 1) return;
    typedef long long ll2 __attribute__((ext_vector_type(2)));
    constexpr int CH = K / 2;
    ll2 v; v.x = -1; v.y = -1;
    char* base = reinterpret_cast<char*>(reinterpret_cast<int64_t*>(out.p2f) + pix0 * K);
#pragma unroll
    for (int i = 0; i < CH; ++i) P2F_STORE(reinterpret_cast<ll2*>(base + fl.piece[i]), v);
  }
}

// What the nearest-face (K = 1) forward does with a pixel's winner: face id, visibility, and for the texture branch
// the atlas lookup, blend and optional fused MSE partial.  Shared by the walking kernel (fwd_block) and by the
// kernel that reads the winner from the cover plane (k_tex_cover).
template <bool CLIP, bool TEX>
__device__ __forceinline__ void k1_finish(const RasterWs& ws, const Tile& t, int F, int H, float sigma, const FwdOut& out,
                                          unsigned long long bestkey, float bestsd, float bestb0, float bestb1,
                                          float bestb2, bool dist_late) {
  const int n = t.n;
  const int64_t fbase = (int64_t)n * F;
    float tacc = 0.f;     // fused texture MSE: this pixel's (tex m - img m)^2 - (img m)^2 over the three channels
    if (t.valid) {
    const bool hit = (bestkey != KEY_NONE);
    const int f = (int)(bestkey & 0xffffffffu);
    if (TEX && dist_late && hit) {
      const size_t o = (size_t)n * F + f;
      Hit h;
      test_face_dist(t.xf, t.yf, ws.rec[o].a, ws.rec[o].b, 0.0f, true, h);
      bestsd = h.sd;
    }
    st_face(out.p2f, t.pix, hit ? fbase + f : (int64_t)-1, out.h16);
    if (out.vis && hit) mark_visible(ws, out, n, F, f);
    if (TEX) {
      // TexturesAtlas.sample_textures + ambient-only Phong + softmax_rgb_blend, K = 1
      // (oracle_atlas_shade is the line-by-line spec)
      const size_t HW = (size_t)H * H;
      const size_t io = (size_t)n * 3 * HW + (size_t)t.yi * H + t.xi;
      if (!hit) {
        st_real(out.imgs, io, 0.f, out.h16); st_real(out.imgs, io + HW, 0.f, out.h16); st_real(out.imgs, io + 2 * HW, 0.f, out.h16);
        st_real(out.sil, t.pix, 0.f, out.h16);
        out.tidx[t.pix] = -1;
      } else {
        const int R = out.R;
        const float zb = __uint_as_float((unsigned)(bestkey >> 32));
        int ix = (int)(bestb0 * (float)R), iy = (int)(bestb1 * (float)R);
        const bool below = ((bestb0 + bestb1) * (float)R - ((float)ix + (float)iy)) <= 1.0f;
        if (!below) { ix = R - 1 - ix; iy = R - 1 - iy; }
        ix = min(max(ix, 0), R - 1); iy = min(max(iy, 0), R - 1);
        const size_t ti = ((((size_t)(n % out.atlas_n) * F + f) * R + iy) * R + ix);
        const float eps = 1e-10f, znear = 1.0f, zfar = 100.0f;
        const float prob = sigmoid_neg(bestsd, sigma);
        const float z_inv = (zfar - zb) / (zfar - znear);
        const float z_inv_max = fmaxf(z_inv, eps);
        const float wnum = prob * expf((z_inv - z_inv_max) / out.gamma);
        const float delta = fmaxf(expf((eps - z_inv_max) / out.gamma), eps);
        const float den = wnum + delta;
        float cr, cg, cb;
        if (out.vrgb) {
          // Textures(verts_rgb) (nmr.py:177-179): barycentric interpolation of the face's vertex colours
          const int4 vi = ws.vidx[(size_t)n * F + f];
          const float* c0 = out.vrgb + ((size_t)n * out.V + vi.x) * 3;
          const float* c1 = out.vrgb + ((size_t)n * out.V + vi.y) * 3;
          const float* c2 = out.vrgb + ((size_t)n * out.V + vi.z) * 3;
          const float b2 = bestb2;
          cr = bestb0 * c0[0] + bestb1 * c1[0] + b2 * c2[0];
          cg = bestb0 * c0[1] + bestb1 * c1[1] + b2 * c2[1];
          cb = bestb0 * c0[2] + bestb1 * c1[2] + b2 * c2[2];
        } else {
          cr = ld_real(out.atlas, ti * 3, out.h16); cg = ld_real(out.atlas, ti * 3 + 1, out.h16);
          cb = ld_real(out.atlas, ti * 3 + 2, out.h16);
        }
        const float vr = (wnum * cr + delta * 0.0f) / den, vg = (wnum * cg + delta * 0.0f) / den,
                    vb = (wnum * cb + delta * 0.0f) / den;
        st_real(out.imgs, io, vr, out.h16); st_real(out.imgs, io + HW, vg, out.h16); st_real(out.imgs, io + 2 * HW, vb, out.h16);
        st_real(out.sil, t.pix, 1.0f - (1.0f - prob), out.h16);
        out.tidx[t.pix] = (int32_t)ti;
        ws.fvis[(size_t)n * F + f] = 1;   // the atlas gradient (k_tex_bwd_faces) visits only faces that were seen
        if (out.lpart) {
          const size_t pp = (size_t)t.yi * H + t.xi, rn = (size_t)(n % out.lrb);
          const float mk = ld_real(out.tmask, rn * HW + pp, out.h16);
          const size_t ro = rn * 3 * HW + pp;
          const float b0 = ld_real(out.timg, ro, out.h16) * mk, b1 = ld_real(out.timg, ro + HW, out.h16) * mk,
                      b2 = ld_real(out.timg, ro + 2 * HW, out.h16) * mk;
          const float d0 = vr * mk - b0, d1 = vg * mk - b1, d2 = vb * mk - b2;
          tacc = (d0 * d0 - b0 * b0) + (d1 * d1 - b1 * b1) + (d2 * d2 - b2 * b2);
        }
      }
    }
    }   // t.valid
    if (TEX && out.lpart) {
      tacc = wave_sum(tacc);
      if (t.lane == 0) {
        const int tiles = (H + RBLK - 1) / RBLK;
        out.lpart[(((size_t)n * tiles + t.yi / RBLK) * tiles + t.xi / RBLK) * 4] = make_float4(tacc, 0.f, 0.f, 0.f);
      }
    }
}

template <int K, bool CLIP, bool TEX>
__device__ __forceinline__ void fwd_block(const RasterWs& ws, const Tile& t, int F, int H, float blur, float sigma,
                                          const FwdOut& out, FwdLdsK<K>& S) {
  auto& L = S.s.L;
  fl_t* s_fl = S.s.fl;
  const int n = t.n;
  const int64_t fbase = (int64_t)n * F;

  if constexpr (K == 1) {
    unsigned long long bestkey = KEY_NONE;
    float bestsd = 0.f, bestb0 = 0.f, bestb1 = 0.f, bestb2 = 0.f;
    // blur == 0 (every hard render of the reference): a face is accepted iff the pixel is inside it,
    // so the three edge distances decide nothing; only the winner's signed distance is ever used
    // (the blend weight of the texture branch) and is evaluated once per pixel after the walk.
    const bool dist_late = !(blur > 0.0f);
    bin_and_walk(ws, t, F, H, L, s_fl, out.box_shrink, [&](int list_n) {
      walk_wave<false>(L, t, H, list_n, blur, nullptr, [&](const Cand& cd, bool in_box, int ord) {
        if (!(in_box && t.valid)) return;
        Hit h;
        h.sd = 0.f;
        bool inside = false;
        if (dist_late) {
          if (!test_face_depth<CLIP, true>(t.xf, t.yf, cd.a, cd.b, cd.c.x, cd.c.y, cd.rden, h, inside)) return;
        } else {
          if (!test_face_depth<CLIP>(t.xf, t.yf, cd.a, cd.b, cd.c.x, cd.c.y, cd.rden, h, inside)) return;
          if (!test_face_dist(t.xf, t.yf, cd.a, cd.b, blur, inside, h)) return;
        }
        const unsigned long long key = make_key(h.pz, cd.fid);
        if (key < bestkey) { bestkey = key; bestsd = h.sd; bestb0 = h.c0; bestb1 = h.c1; bestb2 = h.c2; }
      });
    });
    k1_finish<CLIP, TEX>(ws, t, F, H, sigma, out, bestkey, bestsd, bestb0, bestb1, bestb2, dist_late);
  } else {
    // Per-pixel top-K list: K (depth|face) keys + their blend factors (1 - p), kept SORTED in
    // registers.  A new face is inserted with compares and selects on static
    // register indices (shift_insert_block; the farthest entry falls off the end), so there is no LDS or
    // memory list, no final sort and the kept set is exactly the K nearest at every moment.
    const float sig_scale = out.sig_scale;
    unsigned long long key[K];
    float q[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { key[k] = KEY_NONE; q[k] = 1.0f; }
    int seen = 0;  // faces walked so far by this wave (uniform): no lane holds more than that
    unsigned long long cbest = KEY_NONE;   // ACFM_RECORD_COVER: nearest covering face so far
    unsigned char* s_wl = S.s.wl;  // first stage of the edge cull
    DIAG_ADD(0, 1);
    bin_and_walk(ws, t, F, H, L, s_fl, out.box_shrink, [&](int list_n) {
      DIAG_ADD(1, 1); DIAG_ADD(2, list_n);
      walk_wave<true>(L, t, H, list_n, blur, s_wl, [&](const Cand& cd, bool in_box, int ord) {
        // stage 1 (depth): a face that is not nearer than the K-th kept face of a full list
        // cannot enter it; when that holds for every lane of the wave the face is dropped
        // before its edge distances are computed (empty slots hold ~0, so x < key[K-1] is
        // always true for a list that is not full yet)
        Hit h;
        bool inside = false;
        bool live = in_box && t.valid &&
                    test_face_depth<CLIP>(t.xf, t.yf, cd.a, cd.b, cd.c.x, cd.c.y, cd.rden, h, inside);
        if (out.cover_out) {
          // the hard K = 1 render's candidate test for this pair (test_face_depth<true, true>): strictly inside,
          // depth from the CLIPPED barycentrics (h.c* hold the unclipped ones here), not negative.  Before the
          // K-th-key filter below: the nearest covering face need not be among the K nearest kept faces.
          // (a face that cannot win is dropped before the divisions: clipping an inside pixel's barycentrics divides
          // them by their sum s = area / (area + kEps) -- above 1 for a back-facing face -- so pzc = pz / s up to
          // rounding, and pz (1 - 1e-5) > best s means pzc > best.  With the walk roughly front to back this spares
          // most of the back layer.  cbest still empty: its depth bits are a NaN and the comparison is false.)
          const bool cin = in_box && t.valid && inside &&
                           !(h.pz * 0.99999f > __uint_as_float((unsigned)(cbest >> 32)) * (h.c0 + h.c1 + h.c2));
          if (__ballot(cin) != 0ull) {
            float c0 = h.c0, c1 = h.c1, c2 = h.c2;
            clip_bary(c0, c1, c2);
            const float pzc = bary_depth(c0, c1, c2, cd.b.z, cd.b.w, cd.c.x);
            const unsigned long long xc = make_key(pzc, cd.fid);
            if (cin && !(pzc < 0.0f) && xc < cbest) cbest = xc;
          }
        }
        unsigned long long x = make_key(h.pz, cd.fid);
        live = live && (x < key[K - 1]);
        if (__ballot(live) == 0ull) return;
        DIAG_ADD(5, 1); DIAG_ADD(6, __popcll(__ballot(live)));
        if (!live) return;
        // (read here, not with the record: 8 registers that need not live through the depth stage)
        const float4 e1 = L.e1[cd.idx];
        if (__ballot(e1.z != 0.0f) != 0ull) {   // (rare: some lane's face has an edge shorter than sqrt(kEps))
          if (!test_face_dist(t.xf, t.yf, cd.a, cd.b, blur, inside, h)) return;
        } else {
          if (!test_face_dist_e(t.xf, t.yf, cd.a, cd.b, L.e0[cd.idx], e1, blur, inside, h)) return;
        }
        DIAG_ADD(7, __popcll(__ballot(true))); DIAG_ADD(11, 1);
#ifdef ACFM_DIAG_COUNT
        {   // (group, face) pairs with at least one accepting pixel
          const unsigned long long am = __ballot(true);
          DIAG_ADD(13, ((am & 0xffffull) != 0) + ((am & 0xffff0000ull) != 0) + ((am & 0xffff00000000ull) != 0) + ((am >> 48) != 0));
        }
#endif
        float xq = 1.0f - sigmoid_neg_fast(h.sd, sigma, sig_scale);
        shift_insert_block<K, (K - 1) / 4>(key, q, x, xq, __builtin_amdgcn_readfirstlane(seen + ord + 1));
      });
      seen += list_n;
    });
    const bool split = t.sub >= 0;
    if (split) {
      // The four 16-lane groups hold the K nearest of their quarter of the candidates for the same
      // 16 pixels.  Merge: group 0 takes group 1's entries and group 2 takes group 3's, then group 0
      // takes group 2's; an entry enters by the same insertion (the K nearest of a union are
      // the K nearest of the two K-nearest lists).  Senders keep their lists untouched while they
      // are being read; lists are sorted, so a round ends at the first empty slot of every sender.
#pragma unroll
      for (int round = 0; round < 2; ++round) {
        const int mask = round == 0 ? 16 : 32;
        const bool recv = round == 0 ? ((t.lane & 16) == 0) : ((t.lane & 48) == 0);
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(key[k] & 0xffffffffull), mask, 64);
          const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(key[k] >> 32), mask, 64);
          float oq = __shfl_xor(q[k], mask, 64);
          unsigned long long ok = recv ? (((unsigned long long)hi << 32) | lo) : KEY_NONE;
          if (__ballot(ok != KEY_NONE) != 0ull) shift_insert_block<K, (K - 1) / 4>(key, q, ok, oq, K);
        }
      }
    }
    const bool out_valid = t.valid && (!split || t.lane < 16);
    if (out.cover_out) {
      if (split) {   // the four 16-lane groups saw different candidates of the same 16 pixels
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
          const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)(cbest & 0xffffffffull), m, 64);
          const unsigned hi = (unsigned)__shfl_xor((int)(unsigned)(cbest >> 32), m, 64);
          const unsigned long long o = ((unsigned long long)hi << 32) | lo;
          if (o < cbest) cbest = o;
        }
      }
      if (out_valid) out.cover_out[t.pix] = cbest != KEY_NONE ? (int)(cbest & 0xffffffffu) : -1;
    }
    float lmask = 0.f, lg = 0.f, le = 0.f;
    if (out.lpart && out_valid) {
      const size_t rp = t.pix - (size_t)n * H * H + (size_t)(n % out.lrb) * H * H;
      if (out.lgt) lg = ld_real(out.lgt, rp, out.h16);
      if (out.ledt) le = ld_real(out.ledt, rp, out.h16);
    }
    if (out_valid) {
      float alpha = 1.0f;  // sigmoid_alpha_blend over the kept faces in ascending depth; empty slots hold 1
#pragma unroll
      for (int k = 0; k < K; ++k) alpha = alpha * q[k];
      st_real(out.mask, t.pix, 1.0f - alpha, out.h16);
      if (out.kth) out.kth[t.pix] = key[K - 1];  // ~0 unless K faces are kept
      lmask = 1.0f - alpha;
      if (out.vis && key[0] != KEY_NONE) mark_visible(ws, out, n, F, (int)(key[0] & 0xffffffffu));
      // lean output: only the nearest-face plane, the one slot any caller of the reference
      // reads (loss_utils.py:214, 431); the other K-1 ids stay in registers
      if (out.kout == 1)
        st_face(out.p2f, t.pix, (key[0] != KEY_NONE) ? fbase + (long long)(key[0] & 0xffffffffu) : (long long)-1, out.h16);
    }
    // Fused silhouette losses: with m = 0 outside the blocks that have work, sum|m - g| = sum g + sum(|m - g| - g),
    // sum(m + g - m g) = sum g + sum(m - m g); the finish kernels add sum g.  One 16-byte store per block (and
    // split role), no atomics: the per-mesh sums are formed in fixed order (deterministic).  Called last, after the
    // block's ids are on their way: the references were requested before the outputs (lg, le above).
    auto losses_out = [&]() {
      if (!out.lpart) return;
      float t0 = 0.f, t1 = 0.f, t2 = 0.f, t3 = 0.f;
      if (out_valid) { t0 = fabsf(lmask - lg) - lg; t1 = lmask * lg; t2 = lmask - lmask * lg; t3 = le * lmask; }
      t0 = wave_sum(t0); t1 = wave_sum(t1); t2 = wave_sum(t2); t3 = wave_sum(t3);
      if (t.lane < 4) {
        const int tiles = (H + RBLK - 1) / RBLK;
        // (yi / 8, xi / 8 are the block's own for every lane)
        const size_t slot = (((size_t)n * tiles + t.yi / RBLK) * tiles + t.xi / RBLK) * 4;
        if (split) { if (t.lane == 0) out.lpart[slot + t.sub] = make_float4(t0, t1, t2, t3); }
        else out.lpart[slot + t.lane] = t.lane == 0 ? make_float4(t0, t1, t2, t3) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    if (out.kout == 1) { losses_out(); return; }
    typedef long long ll2 __attribute__((ext_vector_type(2)));  // K even -> 16-byte pieces
    constexpr int CH = K / 2;                                   // pieces per pixel
    constexpr bool STAGED = sizeof(FwdLdsK<K>) >= (size_t)64 * K * 8;
    if (STAGED && !split) {
      // The K ids of a pixel are 8K contiguous bytes, so a lane storing its own row hits 64
      // different cache lines per instruction.  The block's ids are therefore staged in LDS (the
      // candidate lists are dead by now) in image order -- 8 rows of 64K contiguous bytes -- and
      // written out with consecutive lanes on consecutive 16-byte pieces.
      wave_lds_sync();
      ll2* so = reinterpret_cast<ll2*>(&S.stage[0]);
      const int slot = (t.yi & 7) * 8 + (t.xi & 7);
#pragma unroll
      for (int k2 = 0; k2 < CH; ++k2) {
        ll2 v;
        v.x = (key[2 * k2] != KEY_NONE) ? fbase + (long long)(key[2 * k2] & 0xffffffffu) : (long long)-1;
        v.y = (key[2 * k2 + 1] != KEY_NONE) ? fbase + (long long)(key[2 * k2 + 1] & 0xffffffffu) : (long long)-1;
        so[slot * CH + k2] = v;
      }
      wave_lds_sync();
      const int by = t.yi & ~7, bx = t.xi & ~7;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = i * 64 + t.lane;             // piece index: 8 rows x (8 pixels x CH pieces)
        const int r = c / (8 * CH), off = c % (8 * CH);
        if (by + r < H && bx + off / CH < H)
          P2F_STORE(&reinterpret_cast<ll2*>(reinterpret_cast<int64_t*>(out.p2f) + (((size_t)n * H + by + r) * H + bx) * K)[off], so[c]);
      }
    } else if (out_valid) {
      ll2* o2 = reinterpret_cast<ll2*>(reinterpret_cast<int64_t*>(out.p2f) + t.pix * K);
#pragma unroll
      for (int k2 = 0; k2 < CH; ++k2) {
        ll2 v;
        v.x = (key[2 * k2] != KEY_NONE) ? fbase + (long long)(key[2 * k2] & 0xffffffffu) : (long long)-1;
        v.y = (key[2 * k2 + 1] != KEY_NONE) ? fbase + (long long)(key[2 * k2 + 1] & 0xffffffffu) : (long long)-1;
        o2[k2] = v;
      }
    }
    losses_out();
  }
}

// waves per SIMD the K = 1 kernels are compiled for: 4, 5 and 6 measured the same 70 us on the texture forward (it is
// VALU-issue bound, 78 % busy, not latency bound), 7 and 8 spill (75 and 90 us)
constexpr int K1_WAVES = 6;
template <int K, bool CLIP, bool TEX>
__global__ __launch_bounds__(RT, K > 20 ? 2 : K == 1 ? K1_WAVES : 4) void k_raster_fwd(RasterWs ws, int N, int F, int H, float blur,
                                                    float sigma, FwdOut out) {
  __shared__ __attribute__((aligned(16))) FwdLdsK<K> S;
  const Sched sc = make_sched(ws, N, H, K > 1);   // the K-nearest kernels split their heaviest blocks
  struct Stamp {   // diagnostic build: (t_start, t_end, hw | xcc << 32 | (sub + 1) << 36 | cost << 40, t_work_start, t_work_end) per workgroup
    unsigned long long* p; unsigned long long t0, tw, tf; int sub, cost;
    __device__ Stamp(unsigned long long* q) : p(q), t0(q ? __builtin_amdgcn_s_memrealtime() : 0), tw(0), tf(0), sub(-1), cost(0) {}
    __device__ void work(int sub_, int cost_) { if (p) { tw = __builtin_amdgcn_s_memrealtime(); sub = sub_; cost = cost_; } }
    __device__ void work_end() { if (p) tf = __builtin_amdgcn_s_memrealtime(); }
    __device__ ~Stamp() {
      if (p && threadIdx.x == 0) {
        unsigned hw = __builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));   // HW_REG_HW_ID
        unsigned xcc = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));  // HW_REG_XCC_ID
        p[5 * (size_t)blockIdx.x] = t0; p[5 * (size_t)blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
        p[5 * (size_t)blockIdx.x + 2] = ((unsigned long long)(cost & 0xffff) << 40) | ((unsigned long long)(sub + 1) << 36) |
                                        ((unsigned long long)xcc << 32) | hw;
        p[5 * (size_t)blockIdx.x + 3] = tw; p[5 * (size_t)blockIdx.x + 4] = tf;
      }
    }
  } stamp(out.dbg);
  const int lane = threadIdx.x & 63;
  if (sc.sub < 0) {
    // this workgroup's share of the flagged-empty blocks: fire-and-forget stores, issued first
    // a contiguous run of them: the empty entries end the order in ascending block index, so a wave's consecutive
    // blocks are neighbours in the image and their 32-byte row fragments meet in L2 as whole lines
    const int n_empty = sc.per - sc.n_work, chunk = (n_empty + sc.stride - 1) / sc.stride;
    const int e0 = sc.n_work + sc.j0 * chunk, e1 = min(sc.per, e0 + chunk);
    if ((H & (RBLK - 1)) == 0) {
      const FillLane<K> fl = make_fill_lane<K>(H, lane);
#pragma unroll 1
      for (int e = e0; e < e1; ++e) {
        int n, by, bx;
        entry_block(ws.order[(size_t)sc.g * sc.per + e], sc, H, n, by, bx);
        fwd_fill_block_whole<K, TEX>(out, n, by, bx, H, lane, fl);
      }
    } else {
#pragma unroll 1
      for (int e = e0; e < e1; ++e) {
        int n, by, bx;
        entry_block(ws.order[(size_t)sc.g * sc.per + e], sc, H, n, by, bx);
        fwd_fill_block<K, TEX>(out, n, by, bx, H, lane);
      }
    }
  }
#pragma unroll 1
  for (int e = sc.j0; e < sc.e_end; e += sc.stride) {
    const Tile t = make_tile(ws, sc, e, N, H, K > 1);
    if (!t.none) {
#ifdef ACFM_DIAG
      if (out.dbg) {
        const int tiles_ = (H + RBLK - 1) / RBLK;
        stamp.work(t.sub, block_cost(ws, t.n, __builtin_amdgcn_readfirstlane((t.yi / RBLK) * tiles_ + t.xi / RBLK), H));
      }
#endif
      fwd_block<K, CLIP, TEX>(ws, t, F, H, blur, sigma, out, S);
    }
    wave_lds_sync();   // the next block reuses the LDS lists
  }
#ifdef ACFM_DIAG
  stamp.work_end();
#endif
}

// Texture forward from the cover plane (ACFM_RECORD_COVER, acfm_tex_forward ws_ready = 2): the K-nearest render of this
// geometry left the nearest covering face of every pixel of its work blocks in ws.cover -- same inside test, same
// clipped depth, same tie-break as the K = 1 walk -- so a block is one dependent chain (id -> face record -> texel)
// per pixel and no binning.  Same schedule as k_raster_fwd (the order's work entries, then a contiguous run of the
// flagged-empty ones per wave); the unit is a WAVE of a four-wave workgroup and there is no LDS.  What is left is
// mostly the constant stores of the ~80 % empty blocks (24 us by themselves at 64 frames @256^2).
constexpr int COVER_WPB = 4;   // waves per workgroup
template <bool CLIP>
__global__ __launch_bounds__(64 * COVER_WPB) void k_tex_cover(RasterWs ws, int N, int F, int H, float sigma, FwdOut out) {
  const int tiles = (H + RBLK - 1) / RBLK;
  Sched sc;
  sc.G = (N & 7) == 0 ? 8 : 1;
  sc.per = (N / sc.G) * tiles * tiles;
  sc.g = sc.G == 8 ? ((int)blockIdx.x & 7) : 0;
  const int wg = sc.G == 8 ? ((int)blockIdx.x >> 3) : (int)blockIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  sc.j0 = wg * COVER_WPB + wave;
  sc.stride = ((int)gridDim.x / sc.G) * COVER_WPB;
  sc.n_work = ws.n_work[sc.g];
  sc.e_end = sc.n_work;
  sc.sub = -1;
  const int lane = threadIdx.x & 63;
  // Empty blocks.  Images whose side is a multiple of 32, float storage: by QUADS of four horizontally adjacent
  // blocks (32 x 8 pixels): a row of a quad is a whole 128-byte line of every 4-byte plane, so a plane of the quad
  // is ONE 16-byte store per lane instead of four 4-byte ones whose 32-byte fragments have to meet in L2.  A block
  // is empty iff its cost count is 0 (k_order's rule for the flag), read here by position instead of through the
  // order; quads with a working block fall back to single-block fills.  Waves at the low end of the group fill,
  // waves at the high end render (below), so that no wave queues both.
  const bool quads = (H & 31) == 0 && !out.h16;
  int work_j0 = sc.j0;
  if (out.prefilled) {
    // the silhouette render that left the cover plane stored these blocks' constants too (acfm_sil_forward_prefill);
    // only the fused MSE's partial-sum records of the empty blocks remain
    if (out.lpart) {
      const int n_empty = sc.per - sc.n_work;
      for (int e = sc.n_work + sc.j0 * 64 + lane; e < sc.per; e += sc.stride * 64) {
        int n, by, bx;
        entry_block(ws.order[(size_t)sc.g * sc.per + e], sc, H, n, by, bx);
        out.lpart[(((size_t)n * tiles + by / RBLK) * tiles + bx / RBLK) * 4] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
      (void)n_empty;
    }
  } else if (quads) {
    const FillLane<1> fl = make_fill_lane<1>(H, lane);
    const int qrow = tiles / 4, units = (N / sc.G) * tiles * qrow;
    const size_t HW = (size_t)H * H;
    const unsigned off4 = (unsigned)((lane >> 3) * H + (lane & 7) * 4);
#pragma unroll 1
    for (int u = sc.j0; u < units; u += sc.stride) {
      const int m = u / (tiles * qrow), rem = u - m * (tiles * qrow);
      const int byb = rem / qrow, bxb = (rem - byb * qrow) * 4;
      const int n = m * sc.G + sc.g;
      const int cnt = lane < 4 ? ws.tile_cnt[((size_t)n * tiles + byb) * tiles + bxb + lane] : 1;
      const unsigned em = (unsigned)__ballot(cnt == 0) & 15u;
      const int by = byb * RBLK, bx = bxb * RBLK;
      if (em == 15u) {
        const size_t pix0 = ((size_t)n * H + by) * H + bx;
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float* im = reinterpret_cast<float*>(out.imgs) + pix0 + (size_t)n * 2 * HW + off4;
        *reinterpret_cast<float4*>(im) = z;
        *reinterpret_cast<float4*>(im + HW) = z;
        *reinterpret_cast<float4*>(im + 2 * HW) = z;
        *reinterpret_cast<float4*>(reinterpret_cast<float*>(out.sil) + pix0 + off4) = z;
        *reinterpret_cast<int4*>(out.tidx + pix0 + off4) = make_int4(-1, -1, -1, -1);
        typedef long long ll2 __attribute__((ext_vector_type(2)));
        ll2 v; v.x = -1; v.y = -1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int i = lane + 64 * j;               // 16-byte piece of the quad's 8 rows x 256 bytes of ids
          *reinterpret_cast<ll2*>(reinterpret_cast<int64_t*>(out.p2f) + pix0 + (size_t)(i >> 4) * H + 2 * (i & 15)) = v;
        }
        if (out.lpart && lane < 4)
          out.lpart[(((size_t)n * tiles + byb) * tiles + bxb + lane) * 4] = make_float4(0.f, 0.f, 0.f, 0.f);
      } else {
#pragma unroll 1
        for (int b = 0; b < 4; ++b)
          if ((em >> b) & 1u) fwd_fill_block_whole<1, true>(out, n, by, bx + b * RBLK, H, lane, fl);
      }
    }
    work_j0 = sc.stride - 1 - sc.j0;
  } else {
    const int n_empty = sc.per - sc.n_work, chunk = (n_empty + sc.stride - 1) / sc.stride;
    const int e0 = sc.n_work + sc.j0 * chunk, e1 = min(sc.per, e0 + chunk);
    if ((H & (RBLK - 1)) == 0) {
      const FillLane<1> fl = make_fill_lane<1>(H, lane);
#pragma unroll 1
      for (int e = e0; e < e1; ++e) {
        int n, by, bx;
        entry_block(ws.order[(size_t)sc.g * sc.per + e], sc, H, n, by, bx);
        fwd_fill_block_whole<1, true>(out, n, by, bx, H, lane, fl);
      }
    } else {
#pragma unroll 1
      for (int e = e0; e < e1; ++e) {
        int n, by, bx;
        entry_block(ws.order[(size_t)sc.g * sc.per + e], sc, H, n, by, bx);
        fwd_fill_block<1, true>(out, n, by, bx, H, lane);
      }
    }
  }
#pragma unroll 1
  for (int e = work_j0; e < sc.e_end; e += sc.stride) {
    const Tile t = make_tile(ws, sc, e, N, H, false);
    unsigned long long bestkey = KEY_NONE;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f;
    if (t.valid) {
      const int f = out.cover_in[t.pix];
      if (f >= 0) {
        const FaceRec& r = ws.rec[(size_t)t.n * F + f];
        const float4 ra = r.a, rb = r.b, rc = r.c;
        Hit h;
        bool inside = false;
        test_face_depth<CLIP, true>(t.xf, t.yf, ra, rb, rc.x, rc.z, rc.w, h, inside);
        bestkey = make_key(h.pz, f); b0 = h.c0; b1 = h.c1; b2 = h.c2;
      }
    }
    k1_finish<CLIP, true>(ws, t, F, H, sigma, out, bestkey, 0.f, b0, b1, b2, true);
  }
}

// ------------------------------------------------------------------------------- backward
// candidate-list capacity of the backward (LDS per wave: 108 B per slot).  bin_and_walk walks on a full list, so every
// walk but a block's last sees all 64 slots: s_acc has one row per slot, the flush loop covers list_n <= 64 in one pass
constexpr int BWD_CAP = 64;
using BwdList = CandListT<BWD_CAP>;
__device__ __forceinline__ void acc_add(float* p, float v) { atomicAdd(p, v); }
__device__ __forceinline__ void acc_add(long long* p, float v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)__float2ll_rn(v * FIX_SCALE));
}
__device__ __forceinline__ void acc_add_raw(float* p, float v) { atomicAdd(p, v); }
__device__ __forceinline__ void acc_add_raw(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}
template <class AccT>
__device__ __forceinline__ void sil_bwd_block(const RasterWs& ws, const Tile& t, const void* __restrict__ mask,
                                              const unsigned long long* __restrict__ kth,
                                              const BwdGrad& bg, int V, int F, int H, float blur,
                                              float sigma, BwdList& L, fl_t* s_fl, AccT (*s_acc)[6]) {
  // d mask / d sd_k = -(1 - mask) * p_k / sigma   (robust form).  mask == 0
  // exactly means no face contributes (every p_k is 0 or the pixel is empty): no gradient.
  float coef = 0.f;
  unsigned long long kthkey = KEY_NONE;
  const float sig_scale = sigmoid_scale(sigma);
  if (t.empty) return;  // the forward wrote mask = 0 here
  if (t.valid) {
    const float m = ld_real(mask, t.pix, bg.h16);
    if (m != 0.0f) {
      float gm;
      if (bg.grad_mask) {
        gm = bg.grad_mask[t.pix];
      } else {
        const size_t HW = (size_t)H * H;
        const size_t rp = t.pix - (size_t)t.n * HW + (size_t)(t.n % bg.lrb) * HW;
        const float g = bg.lgt ? ld_real(bg.lgt, rp, bg.h16) : 0.f, e = bg.ledt ? ld_real(bg.ledt, rp, bg.h16) : 0.f;
        const float inv = 1.0f / (float)HW;
        const float* go = bg.go + 4 * (size_t)t.n;
        const float g0 = go[0] * inv, g1 = go[1], g2 = go[2], g3 = go[3] * inv;
        const float df = m - g;
        const float sgn = (df > 0.f) ? 1.f : ((df < 0.f) ? -1.f : 0.f);
        gm = g0 * sgn + g1 * g + g2 * (1.0f - g) + g3 * e;
      }
      coef = -gm * (1.0f - m) / sigma;
      kthkey = kth[t.pix];
    }
  }
  const bool work = (coef != 0.0f);
  if (__ballot(work) == 0ull) return;

  for (int i = t.tid; i < BWD_CAP * 6; i += RT) (&s_acc[0][0])[i] = (AccT)0;
  wave_lds_sync();
  AccT* gout;
  if constexpr (sizeof(AccT) == 8) gout = reinterpret_cast<AccT*>(ws.grad_fix) + (size_t)t.n * V * 2;
  else gout = reinterpret_cast<AccT*>(ws.grad_ndc) + (size_t)t.n * V * 2;

  // the pixel this lane stands in for when its group helps its partner group (walk_wave<.., SHARE>): that lane's
  // gradient coefficient and K-th key, fetched once per walk
  float coef_p = 0.f;
  unsigned long long kth_p = KEY_NONE;
  bin_and_walk(ws, t, F, H, L, s_fl, 0.f, [&](int list_n) {
    DIAG_ADD(1, 1); DIAG_ADD(2, list_n);
    walk_wave<false, true>(L, t, H, list_n, blur, nullptr,
                           [&](const Cand& cd, bool in_box, int ord, bool helping, float exf, float eyf) {
      const float coef_e = helping ? coef_p : coef;
      const unsigned long long kth_e = helping ? kth_p : kthkey;
      bool member = (coef_e != 0.0f) && in_box;
      if (__ballot(member) == 0ull) return;
      // the per-edge constants (|e|^2, refined 1/|e|^2) of the face from its record in memory (L2-resident: 128 B x
      // 1280 faces per mesh) instead of recomputing them per pixel -- measured 180.8 -> 171.4 us per 64-frame launch;
      // requested before the depth stage so that its ~100 instructions cover the latency
      const FaceRec& grec = ws.rec[(size_t)t.n * F + cd.fid];
      const float4 e0g = grec.e0, e1g = grec.e1;
      const float4 A = cd.a, B = cd.b;
      Hit h;
      h.pz = 0.f; h.sd = 0.f; h.d01 = 0.f; h.d02 = 0.f; h.d12 = 0.f;
      bool inside = false;
      // stage 1 (depth): only faces at or before the pixel's K-th kept face took part in the
      // blend; the others are dropped before their edge distances are computed
      member = member && test_face_depth<false>(exf, eyf, A, B, cd.c.x, cd.c.y, cd.rden, h, inside);
      member = member && (make_key(h.pz, cd.fid) <= kth_e);
      if (__ballot(member) == 0ull) return;
      float tpar[3] = {0.f, 0.f, 0.f};
      if (__ballot(e1g.z != 0.0f) != 0ull) {   // a face with a degenerate edge takes the unfactored path
        if (member) member = test_face_dist(exf, eyf, A, B, blur, inside, h, tpar);
      } else {
        if (member) member = test_face_dist_e(exf, eyf, A, B, e0g, e1g, blur, inside, h, tpar);
      }
      if (__ballot(member) == 0ull) return;
      float g0x = 0.f, g0y = 0.f, g1x = 0.f, g1y = 0.f, g2x = 0.f, g2y = 0.f;
      if (member) {
        const float x0 = A.x, y0 = A.y, x1 = A.z, x2 = A.w, y1 = B.x, y2 = B.y;
        // inside <=> sd < 0: an inside pixel lies on no edge, so d > 0 and sd = -d < 0
        const bool inside = h.sd < 0.0f;
        // (1-ulp reciprocal in the sigmoid: 1e-7 relative on a gradient checked to 1e-4)
        const float gs = coef_e * sigmoid_neg_fast(h.sd, sigma, sig_scale);   // dL / d sd
        const float gd = inside ? -gs : gs;                      // sd = inside ? -d : d
        // the arg-min edge (01 first, then 02, then 12: SURVEY App-A.4), chosen with selects so that the
        // wave runs ONE distance backward instead of up to three divergent copies of it
        const bool e01 = h.d01 <= h.d02 && h.d01 <= h.d12;
        const bool e02 = !e01 && h.d02 <= h.d01 && h.d02 <= h.d12;
        const float ax = (e01 || e02) ? x0 : x1, ay = (e01 || e02) ? y0 : y1;
        const float bx = e01 ? x1 : x2, by = e01 ? y1 : y2;
        const float tq = e01 ? tpar[0] : (e02 ? tpar[1] : tpar[2]);
        float ax_, ay_, bx_, by_;
        point_line_dist_bwd(exf, eyf, ax, ay, bx, by, tq, gd, ax_, ay_, bx_, by_);
        if (e01) { g0x = ax_; g0y = ay_; g1x = bx_; g1y = by_; }
        else if (e02) { g0x = ax_; g0y = ay_; g2x = bx_; g2y = by_; }
        else { g1x = ax_; g1y = ay_; g2x = bx_; g2y = by_; }
      }
      // The 16 lanes of a row share the face: sum their six contributions.  First the two lanes of a pair swap
      // halves -- the even lane keeps (g0x, g0y, g1x) of both, the odd lane (g1y, g2x, g2y) -- then three values
      // instead of six go through the row shifts (by 2, 4, 8: lanes of one parity): 6 selects + 12 DPP adds instead
      // of 24, and lanes 14 and 15 of the row add three sums each.  A fixed tree: deterministic.
      {
        const bool odd = (t.lane & 1) != 0;
        float k0 = odd ? g1y : g0x, k1 = odd ? g2x : g0y, k2 = odd ? g2y : g1x;
        const float s0 = odd ? g0x : g1y, s1 = odd ? g0y : g2x, s2 = odd ? g1x : g2y;
#define ACFM_DPP_GET(v, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, true))
        k0 += ACFM_DPP_GET(s0, 0xb1); k1 += ACFM_DPP_GET(s1, 0xb1); k2 += ACFM_DPP_GET(s2, 0xb1);   // quad_perm:[1,0,3,2]
        k0 += ACFM_DPP_GET(k0, 0x112); k1 += ACFM_DPP_GET(k1, 0x112); k2 += ACFM_DPP_GET(k2, 0x112); // row_shr:2
        k0 += ACFM_DPP_GET(k0, 0x114); k1 += ACFM_DPP_GET(k1, 0x114); k2 += ACFM_DPP_GET(k2, 0x114); // row_shr:4
        k0 += ACFM_DPP_GET(k0, 0x118); k1 += ACFM_DPP_GET(k1, 0x118); k2 += ACFM_DPP_GET(k2, 0x118); // row_shr:8
#undef ACFM_DPP_GET
        // (a row without a face this iteration, or without members, sums to exact zeros)
        if ((t.lane & 15) >= 14) {
          AccT* acc = s_acc[cd.idx] + (odd ? 3 : 0);   // two groups can hold the same face in one iteration: atomics
          if (k0 != 0.f) acc_add(&acc[0], k0);
          if (k1 != 0.f) acc_add(&acc[1], k1);
          if (k2 != 0.f) acc_add(&acc[2], k2);
        }
      }
    }
    , [&](int partner_lane) {
      const int src = partner_lane >= 0 ? partner_lane : t.lane;
      coef_p = __shfl(coef, src, 64);
      const unsigned lo = (unsigned)__shfl((int)(unsigned)(kthkey & 0xffffffffull), src, 64);
      const unsigned hi = (unsigned)__shfl((int)(unsigned)(kthkey >> 32), src, 64);
      kth_p = ((unsigned long long)hi << 32) | lo;
    }
    );
    wave_lds_sync();
    for (int c = t.lane; c < list_n; c += RT) {
      AccT* acc = s_acc[c];
      const AccT z = (AccT)0;
      const AccT a0 = acc[0], a1 = acc[1], a2 = acc[2], a3 = acc[3], a4 = acc[4], a5 = acc[5];
      if (a0 != z || a1 != z || a2 != z || a3 != z || a4 != z || a5 != z) {
        const int4 vi = ws.vidx[(size_t)t.n * F + __float_as_int(L.c[c].w)];
        if (a0 != z) acc_add_raw(&gout[2 * vi.x], a0);
        if (a1 != z) acc_add_raw(&gout[2 * vi.x + 1], a1);
        if (a2 != z) acc_add_raw(&gout[2 * vi.y], a2);
        if (a3 != z) acc_add_raw(&gout[2 * vi.y + 1], a3);
        if (a4 != z) acc_add_raw(&gout[2 * vi.z], a4);
        if (a5 != z) acc_add_raw(&gout[2 * vi.z + 1], a5);
        acc[0] = z; acc[1] = z; acc[2] = z; acc[3] = z; acc[4] = z; acc[5] = z;
      }
    }
  });
}

// waves per SIMD the backward is compiled for: with the shared walk 5 (no spills; 156.9 us in the benchmark step) beats
// 6 (80 VGPRs + 28 B of scratch; 160.5 us); without it 6 had measured best
constexpr int BWD_WAVES = 5;
template <class AccT>
__global__ __launch_bounds__(RT, BWD_WAVES) void k_sil_bwd(RasterWs ws, const void* __restrict__ mask,
                                                 const unsigned long long* __restrict__ kth,
                                                 BwdGrad grad_mask, int N, int V,
                                                 int F, int H, float blur, float sigma) {
  __shared__ BwdList L;
  __shared__ fl_t s_fl[FLCAP];
  // gradient accumulator per list slot: (d/dx0, d/dy0, d/dx1, d/dy1, d/dx2, d/dy2) of that face,
  // summed over the block's pixels; flushed (global float atomics on the face's three vertices)
  // and cleared after every walk.  (A [V][2] vertex accumulator per block merges more before
  // going to memory but costs 5 KB of LDS per wave at V = 642 and a clear + scan per block.)
  __shared__ AccT s_acc[BWD_CAP][6];
  const Sched sc = make_sched(ws, N, H, true);
#pragma unroll 1
  for (int e = sc.j0; e < sc.e_end; e += sc.stride) {
    const Tile t = make_tile(ws, sc, e, N, H, true);
    if (!t.none) sil_bwd_block(ws, t, mask, kth, grad_mask, V, F, H, blur, sigma, L, s_fl, s_acc);
    wave_lds_sync();
  }
}

// ------------------------------------------------------------------------------- host side
// The launchers of acfm_raster.h: the only places these kernels are launched from.
#ifdef ACFM_DIAG
static unsigned long long* g_dbg = nullptr;   // acfm_debug_set_stamp_buffer
#else
static unsigned long long* const g_dbg = nullptr;
#endif
unsigned long long* stamp_buffer() { return g_dbg; }

// workgroups of a raster launch: per XCD group ceil(entries / div) (+ 4 per split slot), see Sched
static unsigned tile_grid(int N, int H, int div, int split_slots = 0) {
  const int tiles = (H + RBLK - 1) / RBLK;
  const size_t G = (N & 7) == 0 ? 8 : 1;
  const size_t per = (size_t)tiles * tiles * (N / G);
  const size_t d = div < 1 ? 1 : (size_t)div;
  return (unsigned)(G * ((per + d - 1) / d + (size_t)split_slots * 4));
}

template <int K>
static int launch_sil_fwd(const RasterWs& ws, int N, int F, int H, float blur, float sigma,
                          const FwdOut& out, const Tune& tn, hipStream_t st) {
  ProfScope ps(ACFM_PROF_SIL_FWD, st);
  hipLaunchKernelGGL((k_raster_fwd<K, false, false>), dim3(tile_grid(N, H, tn.div[0], ws.split_slots)), dim3(RT), 0, st, ws, N, F,
                     H, blur, sigma, out);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}
int launch_sil_fwd(int K, const RasterWs& ws, int N, int F, int H, float blur, float sigma, const FwdOut& out,
                   const Tune& tn, hipStream_t st) {
  switch (K) {
    case 20: return launch_sil_fwd<20>(ws, N, F, H, blur, sigma, out, tn, st);
    case 10: return launch_sil_fwd<10>(ws, N, F, H, blur, sigma, out, tn, st);
    case 8: return launch_sil_fwd<8>(ws, N, F, H, blur, sigma, out, tn, st);
    case 4: return launch_sil_fwd<4>(ws, N, F, H, blur, sigma, out, tn, st);
    case 2: return launch_sil_fwd<2>(ws, N, F, H, blur, sigma, out, tn, st);
    case 32: return launch_sil_fwd<32>(ws, N, F, H, blur, sigma, out, tn, st);
    default: return ACFM_E_BADARG;  // supported K: 2, 4, 8, 10, 20, 32
  }
}

void launch_sil_bwd(const RasterWs& ws, const void* mask, const unsigned long long* kth, const BwdGrad& bg, int N,
                    int V, int F, int H, float blur, float sigma, const Tune& tn, hipStream_t st) {
  if (tn.deterministic)
    hipLaunchKernelGGL(k_sil_bwd<long long>, dim3(tile_grid(N, H, tn.div[2], ws.split_slots)), dim3(RT), 0, st, ws,
                       mask, kth, bg, N, V, F, H, blur, sigma);
  else
    hipLaunchKernelGGL(k_sil_bwd<float>, dim3(tile_grid(N, H, tn.div[2], ws.split_slots)), dim3(RT), 0, st, ws,
                       mask, kth, bg, N, V, F, H, blur, sigma);
}

// the nearest-face walk (K = 1, blur 0): ids only (acfm_hard_raster), or the texture / vertex-colour render
void launch_k1_fwd(bool tex, const RasterWs& ws, int N, int F, int H, float sigma, const FwdOut& out, const Tune& tn,
                   hipStream_t st) {
  if (tex)
    hipLaunchKernelGGL((k_raster_fwd<1, true, true>), dim3(tile_grid(N, H, tn.div[1])), dim3(RT), 0, st, ws, N, F, H,
                       0.f, sigma, out);
  else
    hipLaunchKernelGGL((k_raster_fwd<1, false, false>), dim3(tile_grid(N, H, tn.div[1])), dim3(RT), 0, st, ws, N, F,
                       H, 0.f, sigma, out);
}

void launch_tex_cover(const RasterWs& ws, int N, int F, int H, float sigma, const FwdOut& out, const Tune& tn,
                      hipStream_t st) {
  // one wave per div entries of the order (measured at 64 frames @256^2, entries per wave 0.5 / 1 / 2 / 4 / 8:
  // 47 / 35 / 31 / 43 / 45 us: fewer waves leave the stores of the empty blocks to too few issuers)
  const size_t G = (N & 7) == 0 ? 8 : 1;
  const size_t per = (size_t)((H + RBLK - 1) / RBLK) * ((H + RBLK - 1) / RBLK) * (N / G);
  const size_t d = (size_t)(tn.div[1] < 1 ? 1 : tn.div[1]) * COVER_WPB;
  hipLaunchKernelGGL((k_tex_cover<true>), dim3((unsigned)(G * ((per + d - 1) / d))), dim3(64 * COVER_WPB), 0, st, ws,
                     N, F, H, sigma, out);
}

// fragments (acfm_rasterize_fragments, acfm_raster_frag.hip): the walk that leaves the K packed ids of every pixel
template <int K, bool CLIP>
static void launch_frag_walk(const RasterWs& ws, int N, int F, int H, float blur, const FwdOut& out, const Tune& tn,
                             hipStream_t st) {
  hipLaunchKernelGGL((k_raster_fwd<K, CLIP, false>), dim3(tile_grid(N, H, tn.div[0], ws.split_slots)), dim3(RT), 0, st,
                     ws, N, F, H, blur, 1e-4f, out);
}

template <bool CLIP>
static int frag_walk(const RasterWs& ws, int N, int F, int H, int K, float blur, FwdOut out, const Tune& tn,
                     hipStream_t st) {
  if (K == 1 && !(blur > 0.0f)) {
    // blur 0: the nearest-face walk (a face is kept iff the pixel is inside it, as in oracle_rasterize)
    hipLaunchKernelGGL((k_raster_fwd<1, CLIP, false>), dim3(tile_grid(N, H, tn.div[1])), dim3(RT), 0, st, ws, N, F, H,
                       0.f, 1e-4f, out);
    return ACFM_OK;
  }
  // the K-nearest walk stores all K ids (kout = K), or slot 0 of the K = 2 walk for K = 1 with blur (slot 0 of a
  // K-nearest list does not depend on K); its blended mask goes to the workspace's cover plane (unused here)
  out.mask = ws.cover;
  out.kout = K == 1 ? 1 : K;
  out.sig_scale = 1.44269504088896341f / 1e-4f;
  switch (K) {
    case 1: case 2: launch_frag_walk<2, CLIP>(ws, N, F, H, blur, out, tn, st); break;
    case 4: launch_frag_walk<4, CLIP>(ws, N, F, H, blur, out, tn, st); break;
    case 8: launch_frag_walk<8, CLIP>(ws, N, F, H, blur, out, tn, st); break;
    case 10: launch_frag_walk<10, CLIP>(ws, N, F, H, blur, out, tn, st); break;
    case 20: launch_frag_walk<20, CLIP>(ws, N, F, H, blur, out, tn, st); break;
    case 32: launch_frag_walk<32, CLIP>(ws, N, F, H, blur, out, tn, st); break;
    default: return ACFM_E_BADARG;
  }
  return ACFM_OK;
}
int frag_walk(bool clip, const RasterWs& ws, int N, int F, int H, int K, float blur, const FwdOut& out, const Tune& tn,
              hipStream_t st) {
  return clip ? frag_walk<true>(ws, N, F, H, K, blur, out, tn, st) : frag_walk<false>(ws, N, F, H, K, blur, out, tn, st);
}

}  // namespace acfm

using namespace acfm;

extern "C" {

// Diagnostic builds only (make DIAG=1 -> libacfm_hip_diag.so, used by tools/stamps.py and tools/occ_probe.py):
// per-workgroup time stamps and the occupancy query.  The shipping library has no such state.
#ifdef ACFM_DIAG_COUNT
int acfm_debug_counters(unsigned long long* host16, int reset) {
  if (host16 && hipMemcpyFromSymbol(host16, HIP_SYMBOL(acfm::g_diag), sizeof(unsigned long long) * 16) != hipSuccess) return ACFM_E_LAUNCH;
  if (reset) {
    unsigned long long z[16] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(acfm::g_diag), z, sizeof(z)) != hipSuccess) return ACFM_E_LAUNCH;
  }
  return ACFM_OK;
}
#endif
#ifdef ACFM_DIAG
int acfm_debug_set_stamp_buffer(void* p) { g_dbg = (unsigned long long*)p; return 0; }
int acfm_debug_occupancy(int which, int dyn_lds) {
  int n = -1;
  hipError_t e = hipSuccess;
  if (which == 0) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_raster_fwd<20, false, false>, RT, 0);
  else if (which == 1) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_raster_fwd<1, true, true>, RT, 0);
  else e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k_sil_bwd<float>, RT, 0);
  return e == hipSuccess ? n : -1;
}
#endif

}  // extern "C"
