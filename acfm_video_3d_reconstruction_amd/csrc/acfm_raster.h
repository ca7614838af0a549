// What the units of the rasteriser share: acfm_raster.hip (the walk kernels), acfm_raster_setup.hip,
// acfm_raster_api.hip, acfm_raster_frag.hip, acfm_raster_texgrad.hip and acfm_project.hip.
// Block constants, storage helpers, the per-pixel face tests, the argument structs of the walk kernels, and the host
// launchers: a kernel is launched only from the unit that defines it (a template instantiation comes into being where
// it is launched and the build has no relocatable device code), so every other unit goes through these.
#pragma once
#include "acfm_common.h"

namespace acfm {

// A raster launch has entries / div workgroups per XCD group (see Sched; div = Tune::div of the call): the
// flagged-empty blocks -- 70 % of a 256^2 frame of the bird -- cost no workgroup dispatch of their own.
constexpr int RBLK = 8;       // pixels per block side: one wave64 per block
constexpr int RT = 64;        // threads per raster workgroup = RBLK*RBLK
constexpr int TPB = 256;      // threads per workgroup of the per-mesh kernels (setup, projection)
constexpr unsigned long long KEY_NONE = ~0ull;
constexpr int CNT_TILE = 8;   // cost counters per 8x8 pixels (= per raster block)
constexpr int SETUP_LDS_TILES = 4096;  // counters kept in LDS up to 512x512 images (64^2 blocks)
constexpr int ENTRY_EMPTY = 1 << 30;   // order entry flag: no face box comes near this block
constexpr int ENTRY_SPLIT = 1 << 29;   // order entry flag: a heavy block, rendered by four workgroups (one per 4x4 pixels)
constexpr int ENTRY_FLAGS = ENTRY_EMPTY | ENTRY_SPLIT;
constexpr int SPLIT_MAX_CLASS = 4;     // ... if their cost class is at most this (>= 80 face boxes)
constexpr int SETUP_LDS_MASK_BYTES = 64 * 1024;  // coarse masks built in LDS up to this size
typedef unsigned short fl_t;  // face ids of one mesh (F <= ACFM_MAX_FACES = 65535)
constexpr int FLCAP = 512;    // LDS face-id list of one wave (faces of its coarse tile, 4096 faces at a time)

// one-wave workgroups: LDS written by some lanes is read by others without a barrier
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Pixel coordinate of an NDC coordinate, i = H-1 - ((c+1)H - 1)/2, held to [-2, H + 1] so that its floor / ceil fits
// an int with the pixel of slack the callers add: a vertex far outside the image (|c| H / 2 beyond 2^31) saturated the
// conversion and the slack overflowed.  The callers test "< 0" and ">= H" and then clamp to [0, H - 1]: all of that
// comes out the same for the held value.
__device__ __forceinline__ float ndc_to_pix_held(float c, float hf) {
  return fminf(fmaxf(hf - 1.0f - ((c + 1.0f) * hf - 1.0f) * 0.5f, -2.0f), hf + 1.0f);
}

// ------------------------------------------------------------------------------- face tests
struct Hit { float pz, sd, c0, c1, c2, d01, d02, d12; };

// One pixel against one face, split in two stages so callers can drop a face after the cheap
// half.  Every rejection of the oracle (oracle_rasterize) is a pure filter, so evaluating
// them in a different order keeps the accepted set -- and every accepted value -- identical.
//   stage 1: barycentrics (IEEE divisions), depth pz, inside flag;  rejects pz < 0
//   stage 2: the three edge distances;  rejects !inside && d >= blur
// INSIDE_ONLY: the caller keeps only pixels inside the face (blur == 0): the others leave before
// the clipped barycentrics and the depth are computed.
// clip_barycentric_coords (the texture branch): clamp to [0,1], renormalise by max(sum, 1e-5); and the depth
// interpolated with whichever barycentrics apply.  One definition each: the K-nearest forward evaluates the
// clipped depth of a covering face too (ACFM_RECORD_COVER) and must land on the bits of the K = 1 render.
__device__ __forceinline__ void clip_bary(float& c0, float& c1, float& c2) {
  c0 = fmaxf(fminf(c0, 1.0f), 0.0f);
  c1 = fmaxf(fminf(c1, 1.0f), 0.0f);
  c2 = fmaxf(fminf(c2, 1.0f), 0.0f);
  const float s = fmaxf(c0 + c1 + c2, 1e-5f);
  const float rs = recip_refined(s);
  c0 = div_by(c0, s, rs); c1 = div_by(c1, s, rs); c2 = div_by(c2, s, rs);
}
__device__ __forceinline__ float bary_depth(float c0, float c1, float c2, float z0, float z1, float z2) {
  return c0 * z0 + c1 * z1 + c2 * z2;
}

template <bool CLIP, bool INSIDE_ONLY = false>
__device__ __forceinline__ bool test_face_depth(float xf, float yf, const float4& A, const float4& B,
                                                float z2, float denom, float r, Hit& h, bool& inside) {
  const float x0 = A.x, y0 = A.y, x1 = A.z, x2 = A.w, y1 = B.x, y2 = B.y;
  const float z0 = B.z, z1 = B.w;
  // three IEEE divisions by the same denominator denom = area + kEps share one refined reciprocal r (acfm_common.h),
  // both computed once per face by k_setup (FaceRec.c) with these very operations
  auto div = [&](float x) { return div_by(x, denom, r); };
  const float w0 = div(edge_fn(xf, yf, x1, y1, x2, y2));
  const float w1 = div(edge_fn(xf, yf, x2, y2, x0, y0));
  const float w2 = div(edge_fn(xf, yf, x0, y0, x1, y1));
  float c0 = w0, c1 = w1, c2 = w2;
  inside = (w0 > 0.0f) && (w1 > 0.0f) && (w2 > 0.0f);
  if (INSIDE_ONLY && !inside) return false;
  if (CLIP) clip_bary(c0, c1, c2);
  const float pz = bary_depth(c0, c1, c2, z0, z1, z2);
  h.pz = pz; h.c0 = c0; h.c1 = c1; h.c2 = c2;
  return !(pz < 0.0f);
}

// tpar (optional): the clamped segment parameters of the three edges (01, 02, 12), for the backward
__device__ __forceinline__ bool test_face_dist(float xf, float yf, const float4& A, const float4& B,
                                               float blur, bool inside, Hit& h, float* tpar = nullptr) {
  const float x0 = A.x, y0 = A.y, x1 = A.z, x2 = A.w, y1 = B.x, y2 = B.y;
  // edges 01 and 02 (both start at vertex 0) share the packed pipe, edge 12 goes through the scalar one
  const v2f ax = {x0, x0}, ay = {y0, y0}, bx = {A.z, A.w}, by = {B.x, B.y};
  v2f t2;
  const v2f d2 = point_line_dist2(xf, yf, ax, ay, bx, by, tpar ? &t2 : nullptr);
  h.d01 = d2.x;
  h.d02 = d2.y;
  h.d12 = point_line_dist(xf, yf, x1, y1, x2, y2, tpar ? tpar + 2 : nullptr);
  if (tpar) { tpar[0] = t2.x; tpar[1] = t2.y; }
  const float d = fminf(fminf(h.d01, h.d02), h.d12);
  h.sd = inside ? -d : d;
  return inside || !(d >= blur);
}

// ------------------------------------------------------------------------------- storage
// Storage type of images and masks: float, or IEEE half with ACFM_STORE_F16 (AcfmRasterTuning.flags bit 1, BASELINE
// config 5 "fp16 render with fp32 loss accumulate").  Only what is STORED changes: every accept / reject decision,
// depth, blend factor and loss sum is computed in fp32 exactly as in the fp32 build, so face ids are identical.
typedef _Float16 half_t;
__device__ __forceinline__ float ld_real(const void* p, size_t i, int h16) {
  return h16 ? (float)reinterpret_cast<const half_t*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}
// (plain stores, also in st_face: non-temporal ones on these 4-byte-per-pixel planes measured 75 -> 123 us on the
// texture forward, see fwd_fill_block)
__device__ __forceinline__ void st_real(void* p, size_t i, float v, int h16) {
  if (h16) reinterpret_cast<half_t*>(p)[i] = (half_t)v;
  else reinterpret_cast<float*>(p)[i] = v;
}
__device__ __forceinline__ float4 ld4_real(const void* p, size_t i4, int h16) {   // elements 4 i4 .. 4 i4 + 3 (aligned)
  if (!h16) return reinterpret_cast<const float4*>(p)[i4];
  typedef half_t h4 __attribute__((ext_vector_type(4)));
  const h4 v = reinterpret_cast<const h4*>(p)[i4];
  return make_float4((float)v.x, (float)v.y, (float)v.z, (float)v.w);
}
__device__ __forceinline__ void st_face(void* p, size_t i, long long id, int h16) {   // nearest-face plane
  if (h16) reinterpret_cast<int32_t*>(p)[i] = (int32_t)id;
  else reinterpret_cast<int64_t*>(p)[i] = (int64_t)id;
}

struct FwdOut {
  unsigned long long* dbg;   // diagnostic build only: per-block (t_start, t_end, hw_id) stamps
  int h16;                   // ACFM_STORE_F16: mask / imgs / sil / atlas / references are IEEE half, p2f is an int32 [N,H,H] plane
  void* mask;                // soft: [N,H,H] (real_t = float, or half with h16)
  void* p2f;                 // [N,H,H,kout] int64; h16: [N,H,H] int32 (kout = 1)
  int kout;                  // soft: K (all kept faces) or 1 (nearest face only)
  unsigned long long* kth;   // soft, optional: [N,H,H] largest kept key if K faces kept, else ~0
  uint8_t* vis;              // optional: [N,V] vertices of every nearest face
  int V;
  // texture branch (TEX)
  const float* vrgb;         // optional [N,V,3]: per-vertex colours instead of an atlas (viz)
  const void* atlas;         // [N,F,R,R,3] real_t
  void* imgs;                // [N,3,H,H] real_t
  void* sil;                 // [N,H,H] real_t
  int32_t* tidx;             // [N,H,H]
  int R;
  float gamma;
  float box_shrink;          // > 0: the workspace was set up with a larger blur margin; boxes are tightened by this much
  int atlas_n;               // number of distinct atlases: mesh n samples atlas n % atlas_n
  float sig_scale;           // log2(e) / sigma (sigmoid_scale), computed on the host: a kernel argument can be re-read
                             // from the kernarg segment with a scalar load where a computed value would be spilled
  // fused render + silhouette losses (acfm_sil_loss_forward): the block's partial sums of the loss terms leave
  // with the mask; lpart == null: plain render
  const void* lgt;           // [lrb,H,H] real_t ground-truth masks (may be null)
  const void* ledt;          // [lrb,H,H] real_t distance transforms (may be null)
  int lrb;                   // references: mesh n is compared with reference n % lrb
  float4* lpart;             // [N,blocks^2,4] (ws.lpart)
  // fused texture render + masked MSE (acfm_tex_mse_forward): lpart[..].x takes the block's sum of
  // (tex m - img m)^2 - (img m)^2 over its covered pixels (elsewhere tex = 0 and the difference vanishes)
  const void* timg;          // [lrb,3,H,H] real_t reference images
  const void* tmask;         // [lrb,H,H] real_t reference masks
  // ACFM_RECORD_COVER: the K-nearest forward writes ws.cover (cover_out), the texture forward that takes the
  // workspace over reads it (cover_in) instead of walking the faces
  int* cover_out;
  const int* cover_in;
  // acfm_sil_forward_prefill: the K-nearest forward also stores the CONSTANT outputs of the texture render that will
  // take this workspace over (acfm_tex_forward ws_ready = 3) on the blocks no face comes near -- the same blocks that
  // render would fill (one emptiness rule: the cost counts of this workspace); here the stores drain behind the walk
  // of the blocks with work, there they were 24 of the kernel's 36 us.  float storage only.
  float* pf_imgs;            // [N,3,H,H] -> 0
  float* pf_sil;             // [N,H,H] -> 0
  int64_t* pf_p2f;           // [N,H,H,1] -> -1
  int32_t* pf_tidx;          // [N,H,H] -> -1
  int prefilled;             // texture forward from the cover plane: the empty blocks hold their constants already
};

// PointLineDistanceBackward with the clamped t held constant.  t is the forward's own clamped
// parameter (point_line_dist, same expression; 1 for a degenerate segment: then q = b exactly, the gradient of a
// is g 0 e = 0 and that of b is g 2 (b - p) = -2 (p - b) g, the degenerate branch of the reference bit for bit).
__device__ __forceinline__ void point_line_dist_bwd(float px, float py, float ax, float ay, float bx,
                                                    float by, float t, float g, float& gax, float& gay,
                                                    float& gbx, float& gby) {
  const float qx = (1.0f - t) * ax + t * bx, qy = (1.0f - t) * ay + t * by;
  const float ex = 2.0f * (qx - px), ey = 2.0f * (qy - py);
  gax = g * (1.0f - t) * ex; gay = g * (1.0f - t) * ey;
  gbx = g * t * ex; gby = g * t * ey;
}

// Upstream gradient of the mask: either given per pixel (grad_mask) or, for the fused render+loss operator,
// formed on the fly from the references and the per-mesh gradients of the four loss terms -- k_mask_losses_bwd's
// expression, operation for operation: go0 sign(m - g) / HW + go1 g + go2 (1 - g) + go3 e / HW.
struct BwdGrad {
  const float* grad_mask;    // [N,H,H] (always float), or null: fused
  const void* lgt;           // [lrb,H,H] real_t (may be null)
  const void* ledt;          // [lrb,H,H] real_t (may be null)
  const float* go;           // [N,4]
  int lrb;
  int h16;                   // mask / lgt / ledt are half
};
// Deterministic accumulation (AcfmRasterTuning.flags bit 0): every row sum (a fixed DPP tree of values that are
// themselves computed deterministically) is converted to 64-bit fixed point (2^-36 units) before it is added to
// the candidate's LDS accumulator and, from there, to the vertex's accumulator in memory -- integer addition is
// associative, so the result does not depend on the order in which blocks, rows and atomics happen to be
// served: two runs are bit-identical.  Rounding each contribution to 2^-36 (1.5e-11) keeps it within 1e-6 of the
// floating-point mode at the gradient scales of this problem (contributions up to ~1, sums up to ~1e3 of 2^27).
constexpr float FIX_SCALE = 68719476736.0f;          // 2^36
constexpr float FIX_INV = 1.0f / 68719476736.0f;

// ------------------------------------------------------------------------------- host side
static inline bool bad_dims(int N, int V, int F, int H) {
  return N <= 0 || N > 65535 || V <= 0 || F <= 0 || F > ACFM_MAX_FACES || H <= 0 || H > 4096 ||
         (size_t)N * F > 0x7fffffffull ||
         (size_t)N * ((H + RBLK - 1) / RBLK) * ((H + RBLK - 1) / RBLK) > 0x7fffffffull;
}

// acfm_raster_setup.hip: k_setup + k_order on a carved workspace
int launch_setup(const float* verts, const int64_t* faces, const float* cams, int N, int V, int F, int H,
                 float offset_z, int mode, float blur, const RasterWs& ws, const Tune& tn, hipStream_t st,
                 uint8_t* vis = nullptr, float* proj_xy = nullptr);
// acfm_raster.hip: the walk kernels.  The void ones only launch (the caller brackets and checks them).
unsigned long long* stamp_buffer();   // FwdOut::dbg of every render: null outside the diagnostic build
int launch_sil_fwd(int K, const RasterWs& ws, int N, int F, int H, float blur, float sigma, const FwdOut& out,
                   const Tune& tn, hipStream_t st);                       // k_raster_fwd<K, false, false>, K > 1
void launch_k1_fwd(bool tex, const RasterWs& ws, int N, int F, int H, float sigma, const FwdOut& out, const Tune& tn,
                   hipStream_t st);                                       // k_raster_fwd<1, tex, tex>
void launch_tex_cover(const RasterWs& ws, int N, int F, int H, float sigma, const FwdOut& out, const Tune& tn,
                      hipStream_t st);                                    // k_tex_cover<true>
int frag_walk(bool clip, const RasterWs& ws, int N, int F, int H, int K, float blur, const FwdOut& out, const Tune& tn,
              hipStream_t st);                                            // k_raster_fwd<K, clip, false>
void launch_sil_bwd(const RasterWs& ws, const void* mask, const unsigned long long* kth, const BwdGrad& bg, int N,
                    int V, int F, int H, float blur, float sigma, const Tune& tn, hipStream_t st);   // k_sil_bwd
// acfm_project.hip: k_project_bwd<1> / <3> on the workspace's NDC-gradient scratch (cleared after reading)
void launch_project_bwd_ndc(bool deterministic, const float* verts, const float* cams, const RasterWs& ws, int N,
                            int V, float* grad_verts, float* grad_cams, const float* gproj, hipStream_t st);

}  // namespace acfm
