// PyTorch3D Fragments (pix_to_face, zbuf, bary_coords, dists) and their backward: k_frag_fwd, k_frag_bwd,
// k_frag_fix_finish and the acfm_rasterize_fragments* entry points.  The ids come from the K-nearest walk of
// acfm_raster.hip (frag_walk).  Replaces rasterize_meshes' per-slot outputs and RasterizeMeshesBackward.
#include "acfm_raster.h"

#include <type_traits>

namespace acfm {

// ------------------------------------------------------------------------------- fragments
// acfm_rasterize_fragments: PyTorch3D's full rasterizer state per (pixel, slot) -- pix_to_face, zbuf, bary_coords,
// dists -- over vertices already in NDC / view space (k_setup mode 2).  The K-nearest walk (k_raster_fwd, the very
// instantiations the silhouette renders use, CLIP as asked) leaves the K packed ids of every pixel, empty blocks
// included (fwd_fill_block*); k_frag_fwd then expands every slot from its face record with the walk's own expressions
// (test_face_depth, clip_bary, bary_depth, test_face_dist), so zbuf is bit for bit the depth half of the walk's sort
// key and every value is the oracle's (oracle_rasterize).  One thread per (pixel, slot), in memory order: the id
// read and the zbuf / dists stores are contiguous across the wave, the 12-byte barycentric triples are regrouped in
// LDS and leave as whole 16-byte pieces of one contiguous 3 KB run per workgroup.
constexpr int FRAG_TPB = 256;
template <bool CLIP>
__global__ __launch_bounds__(FRAG_TPB) void k_frag_fwd(const FaceRec* __restrict__ rec, const int64_t* __restrict__ p2f,
                                                       int H, int K, size_t total, float* __restrict__ zbuf,
                                                       float* __restrict__ bary, float* __restrict__ dists) {
  __shared__ float s_b[FRAG_TPB * 3];
  const int tid = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * FRAG_TPB + tid;
  float z = -1.0f, b0 = -1.0f, b1 = -1.0f, b2 = -1.0f, d = -1.0f;
  if (i < total) {
    const int64_t f = p2f[i];
    if (f >= 0) {
      const size_t p = i / (size_t)K;
      const int xi = (int)(p % (size_t)H), yi = (int)((p / (size_t)H) % (size_t)H);
      const float xf = pix_to_ndc(H - 1 - xi, H), yf = pix_to_ndc(H - 1 - yi, H);
      const FaceRec& r = rec[f];
      const float4 A = r.a, B = r.b, C = r.c;
      Hit h;
      bool inside = false;
      test_face_depth<CLIP>(xf, yf, A, B, C.x, C.z, C.w, h, inside);
      test_face_dist(xf, yf, A, B, 0.0f, inside, h);
      z = h.pz + 0.0f;   // make_key's depth bits
      b0 = h.c0; b1 = h.c1; b2 = h.c2; d = h.sd;
    }
    zbuf[i] = z;
    dists[i] = d;
  }
  s_b[3 * tid] = b0; s_b[3 * tid + 1] = b1; s_b[3 * tid + 2] = b2;
  __syncthreads();
  // the workgroup's 3 x 256 floats are contiguous in `bary` (16-byte aligned: 3 KB per workgroup)
  const size_t e0 = (size_t)blockIdx.x * FRAG_TPB * 3 + 4 * (size_t)tid, e_end = 3 * total;
  if (tid < FRAG_TPB * 3 / 4) {
    if (e0 + 4 <= e_end) {
      *reinterpret_cast<float4*>(bary + e0) = make_float4(s_b[4 * tid], s_b[4 * tid + 1], s_b[4 * tid + 2], s_b[4 * tid + 3]);
    } else {
      for (int c = 0; c < 4; ++c)
        if (e0 + c < e_end) bary[e0 + c] = s_b[4 * tid + c];
    }
  }
}

// acfm_rasterize_fragments_backward: grad_zbuf / grad_bary / grad_dists (each optional) -> d / d verts_ndc.
// One thread per (pixel, slot) with a face, in memory order (FRAG_ITER x 256 consecutive slots per workgroup: a few
// image rows, whose faces repeat from pixel to pixel).  The nine coordinate gradients of a (pixel, slot) go into an
// LDS table of the workgroup's faces (open addressing on the packed id, LDS atomics); at the end every face of the
// table is flushed with one global atomic per non-zero coordinate of its three vertices -- no per-lane global atomics
// at scattered vertices.  A face that finds no table slot within FRAG_PROBES probes goes to memory directly (correct,
// slower; not met at the sizes measured).  AccT = long long: deterministic mode, 2^-36 fixed point as k_sil_bwd.
constexpr int FRAG_ITER = 8;
constexpr int FRAG_PROBES = 32;
// Accumulators.  Float mode: grad_verts [N,V,3] itself, float atomics (table of 512 faces in LDS).  Deterministic
// mode (AcfmRasterTuning.flags bit 0): barycentric gradients scale like 1 / area -- near-degenerate faces reach 1e9
// and more where blur_radius > 0 keeps pixels outside them -- which no single 64-bit fixed-point format covers
// together with the 1e-6 resolution of small gradients.  Every contribution v is therefore split exactly into
// v_hi = rint(v 2^4) 2^-4 and v_lo = v - v_hi, summed as two integers in units of 2^-4 and 2^-40: range |sum| < 2^59
// (5.8e17), resolution 2^-40 (9.1e-13), integer atomics only (table of 256 faces in LDS, [N,V,3] x 2 in memory).
// (FragFix / frag_split: acfm_common.h, shared with the shader backwards of acfm_shade.hip.)
template <bool DET>
__device__ __forceinline__ void frag_add(void* acc, size_t o, double v) {   // o: element [N,V,3] index (memory or LDS slot)
  if constexpr (DET) {
    const FragFix x = frag_split(v);
    long long* a = reinterpret_cast<long long*>(acc) + 2 * o;
    if (x.hi) atomicAdd(reinterpret_cast<unsigned long long*>(a), (unsigned long long)x.hi);
    if (x.lo) atomicAdd(reinterpret_cast<unsigned long long*>(a + 1), (unsigned long long)x.lo);
  } else {
    atomicAdd(reinterpret_cast<float*>(acc) + o, (float)v);
  }
}
// The per-(pixel, slot) gradient is formed in float64 from the float32 vertices and pixel centre: d w_i / d vertex is
// a difference of terms of size 1 / area (and of z_i / area on the zbuf path) whose float32 rounding, not the result,
// would set the error for small faces.
template <bool DET, bool CLIP>
__global__ __launch_bounds__(FRAG_TPB) void k_frag_bwd(const FaceRec* __restrict__ rec, const int4* __restrict__ vidx,
                                                       const int64_t* __restrict__ p2f, const float* __restrict__ g_z,
                                                       const float* __restrict__ g_b, const float* __restrict__ g_d,
                                                       int V, int F, int H, int K, size_t total, void* acc) {
  constexpr int TBL = DET ? 256 : 512, LOG_TBL = DET ? 8 : 9, W = DET ? 2 : 1;   // W: accumulator words per value
  typedef typename std::conditional<DET, long long, float>::type AccT;
  __shared__ int s_key[TBL];
  __shared__ AccT s_acc[9 * W][TBL];
  const int tid = threadIdx.x;
  for (int s = tid; s < TBL; s += FRAG_TPB) {
    s_key[s] = -1;
#pragma unroll
    for (int c = 0; c < 9 * W; ++c) s_acc[c][s] = (AccT)0;
  }
  __syncthreads();
  const size_t base = (size_t)blockIdx.x * FRAG_TPB * FRAG_ITER;
#pragma unroll 1
  for (int it = 0; it < FRAG_ITER; ++it) {
    const size_t i = base + (size_t)it * FRAG_TPB + tid;
    if (i >= total) break;
    const int64_t f = p2f[i];
    if (f < 0) continue;
    const size_t p = i / (size_t)K;
    const int xi = (int)(p % (size_t)H), yi = (int)((p / (size_t)H) % (size_t)H);
    const float pxf = pix_to_ndc(H - 1 - xi, H), pyf = pix_to_ndc(H - 1 - yi, H);
    const FaceRec& r = rec[f];
    const float4 A = r.a, B = r.b, C = r.c;
    double g[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};   // (x, y, z) of v0, v1, v2
    if (g_d) {
      // dists: PointLineDistanceBackward of the arg-min edge, sign -1 inside (oracle_rasterize_backward_dists), in
      // float32 like the forward's distances
      const float gup = g_d[i];
      if (gup != 0.0f) {
        const float x0 = A.x, y0 = A.y, x1 = A.z, x2 = A.w, y1 = B.x, y2 = B.y;
        const float denom = C.z, rden = C.w;
        const float w0 = div_by(edge_fn(pxf, pyf, x1, y1, x2, y2), denom, rden);
        const float w1 = div_by(edge_fn(pxf, pyf, x2, y2, x0, y0), denom, rden);
        const float w2 = div_by(edge_fn(pxf, pyf, x0, y0, x1, y1), denom, rden);
        const bool inside = (w0 > 0.0f) && (w1 > 0.0f) && (w2 > 0.0f);
        const float gd = inside ? -gup : gup;
        float t01, t02, t12;
        const float d01 = point_line_dist(pxf, pyf, x0, y0, x1, y1, &t01);
        const float d02 = point_line_dist(pxf, pyf, x0, y0, x2, y2, &t02);
        const float d12 = point_line_dist(pxf, pyf, x1, y1, x2, y2, &t12);
        float gax, gay, gbx, gby;
        if (d01 <= d02 && d01 <= d12) {
          point_line_dist_bwd(pxf, pyf, x0, y0, x1, y1, t01, gd, gax, gay, gbx, gby);
          g[0] += gax; g[1] += gay; g[3] += gbx; g[4] += gby;
        } else if (d02 <= d01 && d02 <= d12) {
          point_line_dist_bwd(pxf, pyf, x0, y0, x2, y2, t02, gd, gax, gay, gbx, gby);
          g[0] += gax; g[1] += gay; g[6] += gbx; g[7] += gby;
        } else {
          point_line_dist_bwd(pxf, pyf, x1, y1, x2, y2, t12, gd, gax, gay, gbx, gby);
          g[3] += gax; g[4] += gay; g[6] += gbx; g[7] += gby;
        }
      }
    }
    if (g_z || g_b) {
      const double px = pxf, py = pyf;
      const double x0 = A.x, y0 = A.y, x1 = A.z, x2 = A.w, y1 = B.x, y2 = B.y, z0 = B.z, z1 = B.w, z2 = C.x;
      auto edge = [](double qx, double qy, double ax, double ay, double bx, double by) {
        return (qx - ax) * (by - ay) - (qy - ay) * (bx - ax);
      };
      const double D = edge(x2, y2, x0, y0, x1, y1) + 1e-8;   // area + kEps
      const double w0 = edge(px, py, x1, y1, x2, y2) / D, w1 = edge(px, py, x2, y2, x0, y0) / D,
                   w2 = edge(px, py, x0, y0, x1, y1) / D;
      double b0 = w0, b1 = w1, b2 = w2, k0 = 0., k1 = 0., k2 = 0., sum = 0., s = 1.;
      if (CLIP) {
        // b_i = k_i / s, k_i = clamp(w_i, 0, 1), s = max(k0 + k1 + k2, 1e-5)
        k0 = fmin(fmax(w0, 0.), 1.); k1 = fmin(fmax(w1, 0.), 1.); k2 = fmin(fmax(w2, 0.), 1.);
        sum = k0 + k1 + k2; s = fmax(sum, 1e-5);
        b0 = k0 / s; b1 = k1 / s; b2 = k2 / s;
      }
      double gb0 = 0., gb1 = 0., gb2 = 0.;
      if (g_b) { gb0 = g_b[3 * i]; gb1 = g_b[3 * i + 1]; gb2 = g_b[3 * i + 2]; }
      if (g_z) {
        // zbuf = b0 z0 + b1 z1 + b2 z2: d / d z_i = b_i, and z_i into the gradient of b_i
        const double gz = g_z[i];
        g[2] += gz * b0; g[5] += gz * b1; g[8] += gz * b2;
        gb0 += gz * z0; gb1 += gz * z1; gb2 += gz * z2;
      }
      double gw0 = gb0, gw1 = gb1, gw2 = gb2;
      if (CLIP) {
        const double dsum = sum >= 1e-5 ? (gb0 * k0 + gb1 * k1 + gb2 * k2) / (s * s) : 0.;
        gw0 = (w0 >= 0. && w0 <= 1.) ? gb0 / s - dsum : 0.;
        gw1 = (w1 >= 0. && w1 <= 1.) ? gb1 / s - dsum : 0.;
        gw2 = (w2 >= 0. && w2 <= 1.) ? gb2 / s - dsum : 0.;
      }
      // w_i = e_i / D: dw_i = de_i / D - w_i dD / D.  edge(p, a, b) = (px - ax)(by - ay) - (py - ay)(bx - ax):
      //   d/dax = py - by, d/day = bx - px, d/dbx = ay - py, d/dby = px - ax (and d/dpx = by - ay, d/dpy = ax - bx)
      // e0 = edge(p, v1, v2), e1 = edge(p, v2, v0), e2 = edge(p, v0, v1), D - kEps = edge(v2, v0, v1)
      const double gE0 = gw0 / D, gE1 = gw1 / D, gE2 = gw2 / D;
      const double gD = -(gw0 * w0 + gw1 * w1 + gw2 * w2) / D;
      g[3] += gE0 * (py - y2); g[4] += gE0 * (x2 - px); g[6] += gE0 * (y1 - py); g[7] += gE0 * (px - x1);
      g[6] += gE1 * (py - y0); g[7] += gE1 * (x0 - px); g[0] += gE1 * (y2 - py); g[1] += gE1 * (px - x2);
      g[0] += gE2 * (py - y1); g[1] += gE2 * (x1 - px); g[3] += gE2 * (y0 - py); g[4] += gE2 * (px - x0);
      g[0] += gD * (y2 - y1); g[1] += gD * (x1 - x2); g[3] += gD * (y0 - y2); g[4] += gD * (x2 - x0);
      g[6] += gD * (y1 - y0); g[7] += gD * (x0 - x1);
    }
    bool any = false;
#pragma unroll
    for (int c = 0; c < 9; ++c) any = any || g[c] != 0.;
    if (!any) continue;
    const int key = (int)f;   // packed ids fit an int (bad_dims: N F <= 2^31 - 1)
    unsigned h = ((unsigned)key * 2654435761u) >> (32 - LOG_TBL);
    int slot = -1;
#pragma unroll 1
    for (int probe = 0; probe < FRAG_PROBES; ++probe) {
      const int old = atomicCAS(&s_key[h], -1, key);
      if (old == -1 || old == key) { slot = (int)h; break; }
      h = (h + 1) & (TBL - 1);
    }
    if (slot >= 0) {
#pragma unroll
      for (int c = 0; c < 9; ++c) {
        if (g[c] == 0.) continue;
        if constexpr (DET) {
          const FragFix x = frag_split(g[c]);
          if (x.hi) atomicAdd(reinterpret_cast<unsigned long long*>(&s_acc[2 * c][slot]), (unsigned long long)x.hi);
          if (x.lo) atomicAdd(reinterpret_cast<unsigned long long*>(&s_acc[2 * c + 1][slot]), (unsigned long long)x.lo);
        } else {
          atomicAdd(&s_acc[c][slot], (float)g[c]);
        }
      }
    } else {   // table full: straight to memory
      const int4 vi = vidx[f];
      const size_t row = (size_t)(f / F) * V;
      const int vv[3] = {vi.x, vi.y, vi.z};
#pragma unroll
      for (int c = 0; c < 9; ++c)
        if (g[c] != 0.) frag_add<DET>(acc, (row + vv[c / 3]) * 3 + c % 3, g[c]);
    }
  }
  __syncthreads();
  for (int s = tid; s < TBL; s += FRAG_TPB) {
    const int f = s_key[s];
    if (f < 0) continue;
    const int4 vi = vidx[f];
    const size_t row = (size_t)(f / F) * V;
    const int vv[3] = {vi.x, vi.y, vi.z};
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const size_t o = (row + vv[c / 3]) * 3 + c % 3;
      if constexpr (DET) {
        long long* a = reinterpret_cast<long long*>(acc) + 2 * o;
        const long long hi = s_acc[2 * c][s], lo = s_acc[2 * c + 1][s];
        if (hi) atomicAdd(reinterpret_cast<unsigned long long*>(a), (unsigned long long)hi);
        if (lo) atomicAdd(reinterpret_cast<unsigned long long*>(a + 1), (unsigned long long)lo);
      } else {
        const float a = s_acc[c][s];
        if (a != 0.f) atomicAdd(reinterpret_cast<float*>(acc) + o, a);
      }
    }
  }
}

// deterministic mode: the (hi, lo) integer sums -> grad_verts [N,V,3]
__global__ __launch_bounds__(TPB) void k_frag_fix_finish(const long long* __restrict__ fix, size_t n,
                                                          float* __restrict__ grad_verts) {
  const size_t j = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (j >= n) return;
  grad_verts[j] = (float)((double)fix[2 * j] * 0.0625 + (double)fix[2 * j + 1] * (1.0 / 1099511627776.0));
}

static bool frag_k_ok(int K) {
  return K == 1 || K == 2 || K == 4 || K == 8 || K == 10 || K == 20 || K == 32;
}

template <bool DET>
static void launch_frag_bwd(bool clip, unsigned grid, const RasterWs& ws, const int64_t* p2f, const float* gz,
                            const float* gb, const float* gd, int V, int F, int H, int K, size_t total, void* acc,
                            hipStream_t st) {
  if (clip)
    hipLaunchKernelGGL((k_frag_bwd<DET, true>), dim3(grid), dim3(FRAG_TPB), 0, st, ws.rec, ws.vidx, p2f, gz, gb, gd, V,
                       F, H, K, total, acc);
  else
    hipLaunchKernelGGL((k_frag_bwd<DET, false>), dim3(grid), dim3(FRAG_TPB), 0, st, ws.rec, ws.vidx, p2f, gz, gb, gd,
                       V, F, H, K, total, acc);
}

// workspace of the fragments entry points: the raster workspace, then the deterministic backward's [N,V,3] x 2
// integer accumulators
static size_t frag_ws_bytes(const RasterWs& ws, int N, int V) {
  return ws.bytes + align256(sizeof(long long) * 6 * (size_t)N * V);
}

}  // namespace acfm

using namespace acfm;

extern "C" {

// ---- fragments (PyTorch3D rasterize_meshes / RasterizeMeshesBackward over NDC vertices)
size_t acfm_rasterize_fragments_workspace_bytes(int N, int V, int F, int H) {
  if (N <= 0 || V <= 0 || F <= 0 || H <= 0) return 0;
  return frag_ws_bytes(carve_ws(nullptr, N, V, F, H), N, V);
}

int acfm_rasterize_fragments(const float* verts_ndc, const int64_t* faces, int N, int V, int F, int H, int K,
                             float blur_radius, int clip_bary, int64_t* pix_to_face, float* zbuf, float* bary,
                             float* dists, void* wsp, size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream) {
  if (!verts_ndc || !faces || !pix_to_face || !zbuf || !bary || !dists || !wsp) return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || !frag_k_ok(K) || !(blur_radius >= 0.f)) return ACFM_E_BADARG;
  if ((size_t)N * H * H * K > ((size_t)1 << 40)) return ACFM_E_BADARG;
  if (((uintptr_t)bary & 15) != 0) return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn) || tn.f16) return ACFM_E_BADARG;   // float outputs only
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);
  if (frag_ws_bytes(ws, N, V) > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  int rc = launch_setup(verts_ndc, faces, nullptr, N, V, F, H, 0.f, 2, blur_radius, ws, tn, st);
  if (rc) return rc;
  FwdOut out = {};
  out.dbg = stamp_buffer();
  out.p2f = pix_to_face;
  out.V = V;
  out.lrb = 1;
  {
    ProfScope ps(ACFM_PROF_FRAG_FWD, st);
    rc = frag_walk(clip_bary != 0, ws, N, F, H, K, blur_radius, out, tn, st);
    if (rc) return rc;
    const size_t total = (size_t)N * H * H * K;
    const unsigned grid = (unsigned)((total + FRAG_TPB - 1) / FRAG_TPB);
    if (clip_bary)
      hipLaunchKernelGGL(k_frag_fwd<true>, dim3(grid), dim3(FRAG_TPB), 0, st, ws.rec, pix_to_face, H, K, total, zbuf,
                         bary, dists);
    else
      hipLaunchKernelGGL(k_frag_fwd<false>, dim3(grid), dim3(FRAG_TPB), 0, st, ws.rec, pix_to_face, H, K, total, zbuf,
                         bary, dists);
  }
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_rasterize_fragments_backward(const float* verts_ndc, const int64_t* faces, const int64_t* pix_to_face,
                                      const float* grad_zbuf, const float* grad_bary, const float* grad_dists, int N,
                                      int V, int F, int H, int K, float blur_radius, int clip_bary, float* grad_verts,
                                      void* wsp, size_t ws_bytes, int ws_from_forward,
                                      const AcfmRasterTuning* tuning, void* stream) {
  if (!verts_ndc || !faces || !pix_to_face || !grad_verts || !wsp) return ACFM_E_BADARG;
  if (bad_dims(N, V, F, H) || !frag_k_ok(K) || !(blur_radius >= 0.f)) return ACFM_E_BADARG;
  if ((size_t)N * H * H * K > ((size_t)1 << 40)) return ACFM_E_BADARG;
  Tune tn;
  if (!tune_from(tuning, tn) || tn.f16) return ACFM_E_BADARG;
  const RasterWs ws = carve_ws(wsp, N, V, F, H, tn.split);
  if (frag_ws_bytes(ws, N, V) > ws_bytes) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  if (!ws_from_forward) {
    int rc = launch_setup(verts_ndc, faces, nullptr, N, V, F, H, 0.f, 2, blur_radius, ws, tn, st);
    if (rc) return rc;
  }
  const size_t n3 = (size_t)N * V * 3;
  if (!grad_zbuf && !grad_bary && !grad_dists) return zero_async(grad_verts, sizeof(float) * n3, st);
  const size_t total = (size_t)N * H * H * K;
  const unsigned grid = (unsigned)((total + (size_t)FRAG_TPB * FRAG_ITER - 1) / ((size_t)FRAG_TPB * FRAG_ITER));
  {
    ProfScope ps(ACFM_PROF_FRAG_BWD, st);
    if (tn.deterministic) {
      long long* fix = reinterpret_cast<long long*>((char*)wsp + ws.bytes);
      if (zero_async(fix, sizeof(long long) * 2 * n3, st)) return ACFM_E_LAUNCH;
      launch_frag_bwd<true>(clip_bary != 0, grid, ws, pix_to_face, grad_zbuf, grad_bary, grad_dists, V, F, H, K, total,
                            fix, st);
      hipLaunchKernelGGL(k_frag_fix_finish, dim3((unsigned)((n3 + TPB - 1) / TPB)), dim3(TPB), 0, st, fix, n3,
                         grad_verts);
    } else {
      if (zero_async(grad_verts, sizeof(float) * n3, st)) return ACFM_E_LAUNCH;
      launch_frag_bwd<false>(clip_bary != 0, grid, ws, pix_to_face, grad_zbuf, grad_bary, grad_dists, V, F, H, K,
                             total, grad_verts, st);
    }
  }
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
