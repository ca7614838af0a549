// PyTorch3D 0.3.0's TexturesUV.sample_textures over Fragments, forward and backward:
//   uv = sum_i bary_i faces_verts_uvs[f, i] ((0, 0) in empty slots), g = 2 uv - 1,
//   texel = grid_sample(maps[n] flipped along its height, g, bilinear, padding_mode, align_corners),
// with the mesh n taken from the pixel.  P = N H W pixels, K slots per pixel in the Fragments layout (pix_to_face [P,K]
// i64 packed n F + f, -1 empty; bary [P,K,3]); faces_verts_uvs [F_packed,3,2]; maps [N,Hm,Wm,3]; texels [P,K,3].
//
// One thread per slot, as k_interp_fwd: the id plane and the 12-byte bary records are contiguous in p K + k.  The map
// is read in place (no K-fold copy, no [P,K,2] UV tensor); the four taps are 12-byte RGB reads.  Weights and the
// order of the four products follow grid_sample: nw, ne, sw, se, taps outside the map contribute nothing.
//
// The backward recomputes the forward and is fused: grad_maps (scattered), grad_bary (one plain store per slot) and
// grad_faces_verts_uvs (scattered, the D = 2 case of k_interp_bwd) leave one launch; no grad_uv tensor is written.
// Scatter convention of acfm_shade.hip: float atomics, contributions that are exactly zero skipped (the shaders send
// an exact 0 into every empty slot, and all of those land on the one texel maps[n, Hm-1, 0]); deterministic mode
// (AcfmRasterTuning.flags bit 0) sums frag_split integer pairs into the workspace and converts once at the end.
// Lanes of a wave are neighbouring slots, so their taps are neighbouring texels of a few map rows; taps of one texel
// are not merged across the wave (not measured to pay: DESIGN.md "UV textures").
#include "acfm_common.h"

namespace acfm {

constexpr int UV_TPB = 256;     // one slot per thread
constexpr int UV_MAX_SIDE = 16384;   // map sides: (float)(side - 1) and every tap coordinate are exact in float32

struct UvArgs {
  const int64_t* p2f;
  const float* bary;
  const float* fvuv;   // [F_packed,3,2]
  const float* maps;   // [N,Hm,Wm,3]
  size_t PK, slots_per_mesh;   // H W K
  int F_packed, Hm, Wm;
  int align, zeros;    // align_corners; padding_mode: 0 "border", 1 "zeros"
};

// one axis of grid_sample's source index: t in uv units -> the pixel coordinate x, its two taps i0 and i0 + 1 with
// weights w (= i0 + 1 - x) and e (= x - i0), and d x / d t (0 where border padding clamps, as grid_sample's
// clip_coordinates_set_grad: x <= 0 and x >= S - 1 pass nothing)
struct UvAxis {
  float w, e, mult;
  int i0;
  bool v0, v1;   // tap i0 / i0 + 1 lies inside the map
};
__device__ __forceinline__ UvAxis uv_axis(float t, int S, int align, int zeros) {
  const float g = 2.0f * t - 1.0f;
  UvAxis a;
  float x;
  if (align) {
    x = (g + 1.0f) / 2.0f * (float)(S - 1);
    a.mult = (float)(S - 1);
  } else {
    x = ((g + 1.0f) * (float)S - 1.0f) / 2.0f;
    a.mult = (float)S;
  }
  if (!zeros) {
    if (!(x > 0.0f)) {
      x = 0.0f;
      a.mult = 0.0f;
    } else if (x >= (float)(S - 1)) {
      x = (float)(S - 1);
      a.mult = 0.0f;
    }
  }
  const float xf = floorf(x);
  a.v0 = xf >= 0.0f && xf <= (float)(S - 1);    // compared as floats: a far-off (or NaN) coordinate has no tap
  a.v1 = xf >= -1.0f && xf <= (float)(S - 2);
  a.i0 = (a.v0 || a.v1) ? (int)xf : 0;
  a.w = (xf + 1.0f) - x;
  a.e = x - xf;
  return a;
}

struct UvSlot {
  bool live;          // the slot names a face
  float b[3], A[6];   // its barycentrics and the face's three uv pairs (live slots only)
  UvAxis x, y;
  size_t row0, row1;  // float offsets of map rows Hm-1-y0 and Hm-1-(y0+1) of mesh n (valid with y.v0 / y.v1)
};
__device__ __forceinline__ void uv_slot(const UvArgs& a, size_t s, UvSlot& q) {
  const int64_t f = a.p2f[s];
  q.live = f >= 0 && f < a.F_packed;
  float u = 0.0f, v = 0.0f;
  if (q.live) {
    const float* A = a.fvuv + (size_t)f * 6;
#pragma unroll
    for (int i = 0; i < 3; ++i) q.b[i] = a.bary[3 * s + i];
#pragma unroll
    for (int i = 0; i < 6; ++i) q.A[i] = A[i];
    u = q.b[0] * q.A[0] + q.b[1] * q.A[2] + q.b[2] * q.A[4];
    v = q.b[0] * q.A[1] + q.b[1] * q.A[3] + q.b[2] * q.A[5];
  }
  q.x = uv_axis(u, a.Wm, a.align, a.zeros);
  q.y = uv_axis(v, a.Hm, a.align, a.zeros);
  const size_t n = s / a.slots_per_mesh;
  const size_t base = n * (size_t)a.Hm;
  q.row0 = q.y.v0 ? (base + (size_t)(a.Hm - 1 - q.y.i0)) * a.Wm * 3 : 0;        // the map flipped along its height
  q.row1 = q.y.v1 ? (base + (size_t)(a.Hm - 2 - q.y.i0)) * a.Wm * 3 : 0;
}

// the four taps in grid_sample's order (nw, ne, sw, se): float offset of the texel and its bilinear weight
struct UvTap {
  bool ok;
  size_t off;
  float wgt;
};
__device__ __forceinline__ void uv_taps(const UvSlot& q, UvTap t[4]) {
  const size_t x0 = 3 * (size_t)(q.x.v0 ? q.x.i0 : 0), x1 = 3 * (size_t)(q.x.v1 ? q.x.i0 + 1 : 0);
  t[0] = UvTap{q.x.v0 && q.y.v0, q.row0 + x0, q.x.w * q.y.w};
  t[1] = UvTap{q.x.v1 && q.y.v0, q.row0 + x1, q.x.e * q.y.w};
  t[2] = UvTap{q.x.v0 && q.y.v1, q.row1 + x0, q.x.w * q.y.e};
  t[3] = UvTap{q.x.v1 && q.y.v1, q.row1 + x1, q.x.e * q.y.e};
}

__global__ __launch_bounds__(UV_TPB) void k_uv_fwd(UvArgs a, float* __restrict__ out) {
  const size_t s = (size_t)blockIdx.x * UV_TPB + threadIdx.x;
  if (s >= a.PK) return;
  UvSlot q;
  uv_slot(a, s, q);
  UvTap t[4];
  uv_taps(q, t);
  float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (!t[j].ok) continue;
    const float* m = a.maps + t[j].off;
    r += m[0] * t[j].wgt;
    g += m[1] * t[j].wgt;
    b += m[2] * t[j].wgt;
  }
  out[3 * s] = r;
  out[3 * s + 1] = g;
  out[3 * s + 2] = b;
}

template <bool DET>
__device__ __forceinline__ void uv_scatter(void* acc, size_t e, float v) {
  if (v == 0.0f) return;
  if constexpr (DET) {
    const FragFix x = frag_split((double)v);
    unsigned long long* p = reinterpret_cast<unsigned long long*>(acc) + 2 * e;
    if (x.hi) atomicAdd(p, (unsigned long long)x.hi);
    if (x.lo) atomicAdd(p + 1, (unsigned long long)x.lo);
  } else {
    atomicAdd(reinterpret_cast<float*>(acc) + e, v);
  }
}

// With q_j = grad . texel_j over the taps inside the map (0 outside):
//   d L / d x = (q_ne - q_nw) w_y + (q_se - q_sw) e_y,  d L / d y = (q_sw - q_nw) w_x + (q_se - q_ne) e_x
//   d L / d u = d L / d x  d x / d u, d L / d v likewise;  grad_bary_i = gu u_i + gv v_i;  grad_fvuv[f, i] += (gu, gv) b_i
//   grad_maps[tap_j] += grad w_j
template <bool DET>
__global__ __launch_bounds__(UV_TPB) void k_uv_bwd(UvArgs a, const float* __restrict__ g_out, void* __restrict__ g_maps,
                                                   float* __restrict__ g_bary, void* __restrict__ g_fvuv) {
  const size_t s = (size_t)blockIdx.x * UV_TPB + threadIdx.x;
  if (s >= a.PK) return;
  const float g[3] = {g_out[3 * s], g_out[3 * s + 1], g_out[3 * s + 2]};
  float gb[3] = {0.0f, 0.0f, 0.0f};
  if (g[0] != 0.0f || g[1] != 0.0f || g[2] != 0.0f) {
    UvSlot q;
    uv_slot(a, s, q);
    UvTap t[4];
    uv_taps(q, t);
    if (g_maps) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!t[j].ok) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) uv_scatter<DET>(g_maps, t[j].off + c, g[c] * t[j].wgt);
      }
    }
    if (q.live && (g_bary || g_fvuv)) {
      float qt[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        qt[j] = 0.0f;
        if (t[j].ok) {
          const float* m = a.maps + t[j].off;
          qt[j] = g[0] * m[0] + g[1] * m[1] + g[2] * m[2];
        }
      }
      const float gx = (qt[1] - qt[0]) * q.y.w + (qt[3] - qt[2]) * q.y.e;
      const float gy = (qt[2] - qt[0]) * q.x.w + (qt[3] - qt[1]) * q.x.e;
      const float gu = gx * q.x.mult, gv = gy * q.y.mult;
#pragma unroll
      for (int i = 0; i < 3; ++i) gb[i] = gu * q.A[2 * i] + gv * q.A[2 * i + 1];
      if (g_fvuv) {
        const size_t base = (size_t)a.p2f[s] * 6;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          uv_scatter<DET>(g_fvuv, base + 2 * i, gu * q.b[i]);
          uv_scatter<DET>(g_fvuv, base + 2 * i + 1, gv * q.b[i]);
        }
      }
    }
  }
  if (g_bary) {
    g_bary[3 * s] = gb[0];
    g_bary[3 * s + 1] = gb[1];
    g_bary[3 * s + 2] = gb[2];
  }
}

// deterministic mode: the (hi, lo) integer sums -> float
__global__ __launch_bounds__(UV_TPB) void k_uv_fix_finish(const long long* __restrict__ fix, size_t n,
                                                          float* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * UV_TPB + threadIdx.x;
  if (j < n) out[j] = frag_unsplit(fix[2 * j], fix[2 * j + 1]);
}

static unsigned uv_blocks(size_t n) { return (unsigned)((n + UV_TPB - 1) / UV_TPB); }

// the rules of every fragments entry point (P K within the raster's bound, K up to ACFM_MAX_K, no half storage) and of
// this one: P = N pix_per_mesh, map sides in [1, UV_MAX_SIDE] (>= 2 with align_corners), padding_mode 0 or 1
static int uv_args(const int64_t* p2f, const float* bary, const float* fvuv, const float* maps, size_t P, int K,
                   int pix_per_mesh, int F_packed, int N, int Hm, int Wm, int align_corners, int padding_mode,
                   const AcfmRasterTuning* tuning, Tune& tn, UvArgs& a) {
  if (!p2f || !bary || !fvuv || !maps || P == 0 || K <= 0 || K > ACFM_MAX_K || P * (size_t)K > ((size_t)1 << 40))
    return ACFM_E_BADARG;
  if (!tune_from(tuning, tn) || tn.f16) return ACFM_E_BADARG;
  if (N <= 0 || pix_per_mesh <= 0 || (size_t)N * (size_t)pix_per_mesh != P || F_packed <= 0) return ACFM_E_BADARG;
  if (Hm < 1 || Wm < 1 || Hm > UV_MAX_SIDE || Wm > UV_MAX_SIDE) return ACFM_E_BADARG;
  if (align_corners && (Hm < 2 || Wm < 2)) return ACFM_E_BADARG;
  if (padding_mode != 0 && padding_mode != 1) return ACFM_E_BADARG;
  a = UvArgs{p2f, bary, fvuv, maps, P * (size_t)K, (size_t)pix_per_mesh * (size_t)K, F_packed, Hm, Wm,
             align_corners ? 1 : 0, padding_mode};
  return ACFM_OK;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_uv_texels(const int64_t* pix_to_face, const float* bary, const float* faces_verts_uvs, const float* maps,
                   size_t P, int K, int pix_per_mesh, int F_packed, int N, int Hm, int Wm, int align_corners,
                   int padding_mode, float* texels, const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  UvArgs a;
  if (!texels) return ACFM_E_BADARG;
  if (uv_args(pix_to_face, bary, faces_verts_uvs, maps, P, K, pix_per_mesh, F_packed, N, Hm, Wm, align_corners,
              padding_mode, tuning, tn, a))
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_uv_fwd, dim3(uv_blocks(a.PK)), dim3(UV_TPB), 0, (hipStream_t)stream, a, texels);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_uv_texels_backward(const int64_t* pix_to_face, const float* bary, const float* faces_verts_uvs,
                            const float* maps, const float* grad_texels, size_t P, int K, int pix_per_mesh,
                            int F_packed, int N, int Hm, int Wm, int align_corners, int padding_mode, float* grad_maps,
                            float* grad_bary, float* grad_faces_verts_uvs, void* ws, size_t ws_bytes,
                            const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  UvArgs a;
  if (!grad_texels) return ACFM_E_BADARG;
  if (uv_args(pix_to_face, bary, faces_verts_uvs, maps, P, K, pix_per_mesh, F_packed, N, Hm, Wm, align_corners,
              padding_mode, tuning, tn, a))
    return ACFM_E_BADARG;
  if (!grad_maps && !grad_bary && !grad_faces_verts_uvs) return ACFM_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t n_maps = grad_maps ? (size_t)N * Hm * Wm * 3 : 0, n_fv = grad_faces_verts_uvs ? (size_t)F_packed * 6 : 0;
  const bool det = tn.deterministic && (n_maps + n_fv) > 0;
  void* acc_maps = grad_maps;
  void* acc_fv = grad_faces_verts_uvs;
  if (det) {   // workspace: the integer pairs of grad_maps, then those of grad_faces_verts_uvs
    if (!ws || ws_bytes < 2 * sizeof(long long) * (n_maps + n_fv)) return ACFM_E_WORKSPACE;
    if (zero_async(ws, 2 * sizeof(long long) * (n_maps + n_fv), st)) return ACFM_E_LAUNCH;
    acc_maps = grad_maps ? ws : nullptr;
    acc_fv = grad_faces_verts_uvs ? (void*)((long long*)ws + 2 * n_maps) : nullptr;
  } else {
    if (grad_maps && zero_async(grad_maps, sizeof(float) * n_maps, st)) return ACFM_E_LAUNCH;
    if (grad_faces_verts_uvs && zero_async(grad_faces_verts_uvs, sizeof(float) * n_fv, st)) return ACFM_E_LAUNCH;
  }
  if (det)
    hipLaunchKernelGGL(k_uv_bwd<true>, dim3(uv_blocks(a.PK)), dim3(UV_TPB), 0, st, a, grad_texels, acc_maps, grad_bary,
                       acc_fv);
  else
    hipLaunchKernelGGL(k_uv_bwd<false>, dim3(uv_blocks(a.PK)), dim3(UV_TPB), 0, st, a, grad_texels, acc_maps,
                       grad_bary, acc_fv);
  if (det) {
    if (grad_maps)
      hipLaunchKernelGGL(k_uv_fix_finish, dim3(uv_blocks(n_maps)), dim3(UV_TPB), 0, st,
                         reinterpret_cast<const long long*>(ws), n_maps, grad_maps);
    if (grad_faces_verts_uvs)
      hipLaunchKernelGGL(k_uv_fix_finish, dim3(uv_blocks(n_fv)), dim3(UV_TPB), 0, st,
                         reinterpret_cast<const long long*>(ws) + 2 * n_maps, n_fv, grad_faces_verts_uvs);
  }
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
