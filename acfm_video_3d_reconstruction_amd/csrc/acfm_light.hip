// Lit shading of PyTorch3D 0.3.0's mesh renderer: vertex and face normals (Meshes._compute_normals),
// the lighting function of DirectionalLights / PointLights at arbitrary points (Gouraud's vertex stage), and the
// per-fragment Phong / flat shader that interpolates position and normal inside the kernel, forward and backward.
//
// All arithmetic is float32 under the Makefile's flags: sqrtf and true divisions in the normalisations, powf for the
// specular power (relu(v.r)^64 multiplies rounding error by 64; no approximate intrinsic is used).
//
// Normals: a vertex-to-incident-corner table in CSR form (offsets [V+1], corners [3F] = 3 f + i, ascending) turns both
// directions into gathers per vertex: no atomics, no valence cap, the same bits on every run.
//
// Shader backward: texels' and barycentrics' gradients are dense, from the slot's own thread.  Position and normal
// gradients go to a face-corner buffer [F_packed,3,6] (position, normal per corner); k_corner_gather then sums a
// vertex's corners through the same incidence table.  Only the pixel-to-corner stage scatters.  Sizing it (64 meshes,
// 256^2, K = 8, every slot filled): 33.5 M slots x 18 floats = 2.4 GB of float atomics; at the chip-wide float-atomic
// rate of about 1.3 TB/s that is 1.9 ms at best, and 60 ms at the 0.04 TB/s measured for the unshaped scatter of the
// UV backward, against a 0.6 ms byte floor for the dense traffic.  So what shares a face is summed inside the wave first: the backward lays a
// wave's 64 lanes along 64 consecutive pixels of ONE slot index k (a face's pixels are neighbours along a row), runs of
// equal face ids are summed with a segmented shuffle reduction in a fixed order, and only the head lane of each run
// issues atomics.  Deterministic mode (AcfmRasterTuning.flags bit 0) adds the run sums as integer pairs
// (frag_split) and converts once at the end, like k_interp_bwd<true>.
#include <climits>

#include "acfm_common.h"

namespace acfm {

constexpr int LT_TPB = 256;
constexpr float LT_EPS = 1e-6f;   // F.normalize(eps=1e-6), in the normals and in the lighting terms
constexpr int LT_NC = 16;         // floats per mesh of `consts`: ambient, diffuse, specular products, light vector,
                                  // camera centre (3 each), shininess

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 v3(float x, float y, float z) { return V3{x, y, z}; }
__device__ __forceinline__ V3 ld3(const float* p) { return V3{p[0], p[1], p[2]}; }
__device__ __forceinline__ void st3(float* p, V3 a) { p[0] = a.x; p[1] = a.y; p[2] = a.z; }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return V3{a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 operator*(V3 a, V3 b) { return V3{a.x * b.x, a.y * b.y, a.z * b.z}; }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return V3{s * a.x, s * a.y, s * a.z}; }
__device__ __forceinline__ V3 neg(V3 a) { return V3{-a.x, -a.y, -a.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ V3 cross(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float sum3(V3 a) { return a.x + a.y + a.z; }

// y = x / max(|x|, eps)
__device__ __forceinline__ V3 normalize_eps(V3 x) {
  const float d = fmaxf(sqrtf(dot(x, x)), LT_EPS);
  return V3{x.x / d, x.y / d, x.z / d};
}
// its backward: (g - y (y.g)) / |x| where |x| >= eps, g / eps below (the clamp passes no gradient to the norm)
__device__ __forceinline__ V3 normalize_eps_bwd(V3 x, V3 g) {
  const float len = sqrtf(dot(x, x));
  if (len < LT_EPS) return V3{g.x / LT_EPS, g.y / LT_EPS, g.z / LT_EPS};
  const V3 y = V3{x.x / len, x.y / len, x.z / len};
  const float yg = dot(y, g);
  return V3{(g.x - y.x * yg) / len, (g.y - y.y * yg) / len, (g.z - y.z * yg) / len};
}

// ---------------------------------------------------------------------------------- the lighting function
// out = (ambient + diffuse relu(n.l)) colour + specular relu(v.r)^shininess [n.l > 0], as lighting.py composes it:
// l = normalise(point ? L - p : L), n = normalise(n), v = normalise(camera - p), r = 2 (n.l) n - l.
__device__ __forceinline__ V3 light_eval(const float* __restrict__ C, int point, V3 p, V3 n, V3 col) {
  const V3 L = ld3(C + 9);
  const V3 nn = normalize_eps(n);
  const V3 l = normalize_eps(point ? L - p : L);
  const float c = dot(nn, l);
  const float angle = fmaxf(c, 0.0f);
  const V3 v = normalize_eps(ld3(C + 12) - p);
  const V3 r = neg(l) + 2.0f * (c * nn);
  const float alpha = c > 0.0f ? fmaxf(dot(v, r), 0.0f) : 0.0f;
  const float pw = powf(alpha, C[15]);
  return (ld3(C) + angle * ld3(C + 3)) * col + pw * ld3(C + 6);
}

// gradients of sum(go * out) to the point, the normal and the colour.  At alpha == 0 the power's gradient is torch's,
// s 0^(s-1) (0 for s > 1, 1 for s = 1), and it is selected away -- never multiplied by 0 -- where the relu or the
// n.l > 0 mask is closed, so no inf 0 can form.
__device__ __forceinline__ void light_eval_bwd(const float* __restrict__ C, int point, V3 p, V3 n, V3 col, V3 go,
                                               V3& gp, V3& gn, V3& gc) {
  const V3 L = ld3(C + 9), D = ld3(C + 3), S = ld3(C + 6);
  const float s = C[15];
  const V3 nn = normalize_eps(n);
  const V3 dir = point ? L - p : L;
  const V3 l = normalize_eps(dir);
  const float c = dot(nn, l);
  const float angle = fmaxf(c, 0.0f);
  const V3 vd = ld3(C + 12) - p;
  const V3 v = normalize_eps(vd);
  const V3 r = neg(l) + 2.0f * (c * nn);
  const float vr = dot(v, r);
  const bool open = c > 0.0f && vr > 0.0f;
  gc = go * (ld3(C) + angle * D);
  const float g_angle = sum3(go * D * col);
  float g_vr = 0.0f;
  if (open) g_vr = s == 0.0f ? 0.0f : sum3(go * S) * (s * powf(vr, s - 1.0f));
  const V3 g_v = g_vr * r, g_r = g_vr * v;
  const float g_c = 2.0f * dot(g_r, nn) + (c > 0.0f ? g_angle : 0.0f);
  const V3 g_nn = 2.0f * (c * g_r) + g_c * l;
  const V3 g_l = neg(g_r) + g_c * nn;
  gn = normalize_eps_bwd(n, g_nn);
  gp = neg(normalize_eps_bwd(vd, g_v));
  if (point) gp = gp - normalize_eps_bwd(dir, g_l);
}

// ---------------------------------------------------------------------------------- vertex and face normals
struct Tri { V3 v[3]; int64_t id[3]; bool ok; };
__device__ __forceinline__ Tri load_tri(const float* __restrict__ verts, const int64_t* __restrict__ faces, int64_t f,
                                        int V) {
  Tri t;
  t.ok = true;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t.id[i] = faces[3 * f + i];
    t.ok = t.ok && t.id[i] >= 0 && t.id[i] < V;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) t.v[i] = t.ok ? ld3(verts + 3 * t.id[i]) : v3(0.f, 0.f, 0.f);
  return t;
}
// the unnormalised cross product taken at corner i: (v[i+1] - v[i]) x (v[i+2] - v[i])
__device__ __forceinline__ V3 corner_cross(const Tri& t, int i) {
  const int a = i == 2 ? 0 : i + 1, b = i == 0 ? 2 : i - 1;
  return cross(t.v[a] - t.v[i], t.v[b] - t.v[i]);
}
__device__ __forceinline__ void row_range(const int* __restrict__ offsets, int v, int F, int& lo, int& hi) {
  lo = offsets[v] < 0 ? 0 : offsets[v];
  hi = offsets[v + 1] > 3 * F ? 3 * F : offsets[v + 1];
}
// the raw sum of vertex v: its corners' cross products in table order
__device__ __forceinline__ V3 raw_normal(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                         const int* __restrict__ offsets, const int* __restrict__ corners, int v, int V,
                                         int F) {
  int lo, hi;
  row_range(offsets, v, F, lo, hi);
  V3 raw = v3(0.f, 0.f, 0.f);
  for (int k = lo; k < hi; ++k) {
    const int c = corners[k];
    if (c < 0 || c >= 3 * F) continue;
    const Tri t = load_tri(verts, faces, c / 3, V);
    if (t.ok) raw = raw + corner_cross(t, c % 3);
  }
  return raw;
}

__global__ __launch_bounds__(LT_TPB) void k_vn_fwd(const float* __restrict__ verts, const int64_t* __restrict__ faces,
                                                   const int* __restrict__ offsets, const int* __restrict__ corners,
                                                   int V, int F, float* __restrict__ vn, float* __restrict__ fn) {
  const int t = blockIdx.x * LT_TPB + threadIdx.x;
  if (t < V && vn) st3(vn + 3 * (size_t)t, normalize_eps(raw_normal(verts, faces, offsets, corners, t, V, F)));
  if (t < F && fn) {
    const Tri tr = load_tri(verts, faces, t, V);
    st3(fn + 3 * (size_t)t, normalize_eps(corner_cross(tr, 1)));
  }
}

// backward, stage 1: the gradient of every vertex's raw sum, through the normalisation (recomputed)
__global__ __launch_bounds__(LT_TPB) void k_vn_bwd_raw(const float* __restrict__ verts,
                                                       const int64_t* __restrict__ faces,
                                                       const int* __restrict__ offsets,
                                                       const int* __restrict__ corners, const float* __restrict__ g_vn,
                                                       int V, int F, float* __restrict__ g_raw) {
  const int t = blockIdx.x * LT_TPB + threadIdx.x;
  if (t >= V) return;
  st3(g_raw + 3 * (size_t)t,
      normalize_eps_bwd(raw_normal(verts, faces, offsets, corners, t, V, F), ld3(g_vn + 3 * (size_t)t)));
}

// d(sum G . (a x b)) with a = v[j+1] - v[j], b = v[j+2] - v[j]: b x G to v[j+1], G x a to v[j+2], minus both to v[j];
// the part that falls on corner i
__device__ __forceinline__ V3 cross_bwd_at(const Tri& t, int j, V3 G, int i) {
  const int ia = j == 2 ? 0 : j + 1, ib = j == 0 ? 2 : j - 1;
  const V3 a = t.v[ia] - t.v[j], b = t.v[ib] - t.v[j];
  const V3 ga = cross(b, G), gb = cross(G, a);
  if (i == ia) return ga;
  if (i == ib) return gb;
  return neg(ga + gb);
}

// backward, stage 2: per vertex, over its incident faces, the gradient of all three corners' raw sums (and of the
// face's own normal) with respect to this vertex
__global__ __launch_bounds__(LT_TPB) void k_vn_bwd_verts(const float* __restrict__ verts,
                                                         const int64_t* __restrict__ faces,
                                                         const int* __restrict__ offsets,
                                                         const int* __restrict__ corners,
                                                         const float* __restrict__ g_raw,
                                                         const float* __restrict__ g_fn, int V, int F,
                                                         float* __restrict__ g_verts) {
  const int t = blockIdx.x * LT_TPB + threadIdx.x;
  if (t >= V) return;
  int lo, hi;
  row_range(offsets, t, F, lo, hi);
  V3 acc = v3(0.f, 0.f, 0.f);
  for (int k = lo; k < hi; ++k) {
    const int c = corners[k];
    if (c < 0 || c >= 3 * F) continue;
    const int f = c / 3, i = c % 3;
    const Tri tr = load_tri(verts, faces, f, V);
    if (!tr.ok) continue;
    if (g_raw) {
#pragma unroll
      for (int j = 0; j < 3; ++j) acc = acc + cross_bwd_at(tr, j, ld3(g_raw + 3 * tr.id[j]), i);
    }
    if (g_fn) acc = acc + cross_bwd_at(tr, 1, normalize_eps_bwd(corner_cross(tr, 1), ld3(g_fn + 3 * (size_t)f)), i);
  }
  st3(g_verts + 3 * (size_t)t, acc);
}

// ---------------------------------------------------------------------------------- lighting at points
__global__ __launch_bounds__(LT_TPB) void k_light_points_fwd(const float* __restrict__ points,
                                                             const float* __restrict__ normals,
                                                             const float* __restrict__ colours,
                                                             const int64_t* __restrict__ mesh_idx,
                                                             const float* __restrict__ consts, int point, int M, int N,
                                                             float* __restrict__ out) {
  const int t = blockIdx.x * LT_TPB + threadIdx.x;
  if (t >= M) return;
  const int64_t m = mesh_idx ? mesh_idx[t] : 0;
  V3 o = v3(0.f, 0.f, 0.f);
  if (m >= 0 && m < N)
    o = light_eval(consts + LT_NC * m, point, ld3(points + 3 * (size_t)t), ld3(normals + 3 * (size_t)t),
                   ld3(colours + 3 * (size_t)t));
  st3(out + 3 * (size_t)t, o);
}

__global__ __launch_bounds__(LT_TPB) void k_light_points_bwd(const float* __restrict__ points,
                                                             const float* __restrict__ normals,
                                                             const float* __restrict__ colours,
                                                             const int64_t* __restrict__ mesh_idx,
                                                             const float* __restrict__ consts,
                                                             const float* __restrict__ g_out, int point, int M, int N,
                                                             float* __restrict__ g_points, float* __restrict__ g_normals,
                                                             float* __restrict__ g_colours) {
  const int t = blockIdx.x * LT_TPB + threadIdx.x;
  if (t >= M) return;
  const int64_t m = mesh_idx ? mesh_idx[t] : 0;
  V3 gp = v3(0.f, 0.f, 0.f), gn = gp, gc = gp;
  if (m >= 0 && m < N)
    light_eval_bwd(consts + LT_NC * m, point, ld3(points + 3 * (size_t)t), ld3(normals + 3 * (size_t)t),
                   ld3(colours + 3 * (size_t)t), ld3(g_out + 3 * (size_t)t), gp, gn, gc);
  if (g_points) st3(g_points + 3 * (size_t)t, gp);
  if (g_normals) st3(g_normals + 3 * (size_t)t, gn);
  if (g_colours) st3(g_colours + 3 * (size_t)t, gc);
}

// ---------------------------------------------------------------------------------- the per-fragment shader
struct PhongArgs {
  const int64_t* p2f;
  const float* bary;
  const float* texels;
  const float* verts;
  const int64_t* faces;
  const float* normals;   // [V,3] vertex normals (phong) or [F,3] face normals (flat)
  const float* consts;
  size_t P;
  int K, pix_per_mesh, F, V, N, point;
};

// position and normal of a slot; -> whether the slot holds a face (else both are 0, as the composition shades it)
template <bool FLAT>
__device__ __forceinline__ bool slot_geometry(const PhongArgs& a, size_t s, int64_t f, Tri& t, V3 nv[3], float b[3],
                                              V3& p, V3& n) {
  p = n = v3(0.f, 0.f, 0.f);
  if (f < 0 || f >= a.F) return false;
  t = load_tri(a.verts, a.faces, f, a.V);
  if (!t.ok) return false;
  if constexpr (FLAT) {
    const float third = 1.0f / 3.0f;
    p = third * ((t.v[0] + t.v[1]) + t.v[2]);
    n = ld3(a.normals + 3 * (size_t)f);
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      b[i] = a.bary[3 * s + i];
      nv[i] = ld3(a.normals + 3 * t.id[i]);
    }
    p = (b[0] * t.v[0] + b[1] * t.v[1]) + b[2] * t.v[2];
    n = (b[0] * nv[0] + b[1] * nv[1]) + b[2] * nv[2];
  }
  return true;
}

// one thread per slot, slots in memory order
template <bool FLAT>
__global__ __launch_bounds__(LT_TPB) void k_phong_fwd(PhongArgs a, float* __restrict__ out) {
  const size_t s = (size_t)blockIdx.x * LT_TPB + threadIdx.x;
  if (s >= a.P * a.K) return;
  const int mesh = (int)((s / a.K) / a.pix_per_mesh);
  Tri t;
  V3 nv[3], p, n;
  float b[3];
  slot_geometry<FLAT>(a, s, a.p2f[s], t, nv, b, p, n);
  st3(out + 3 * s, light_eval(a.consts + LT_NC * mesh, a.point, p, n, ld3(a.texels + 3 * s)));
}

// sum of `v` over each run of equal ids along the wave's lanes, left in the run's first lane; `end` = its last lane
__device__ __forceinline__ float run_sum(float v, int lane, int end) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float t = __shfl_down(v, o, 64);
    if (lane + o <= end) v += t;
  }
  return v;
}

template <bool DET>
__device__ __forceinline__ void corner_add(void* __restrict__ acc, size_t e, float v) {
  if (v == 0.0f) return;
  if constexpr (DET) {
    const FragFix x = frag_split((double)v);
    unsigned long long* q = reinterpret_cast<unsigned long long*>(acc) + 2 * e;
    if (x.hi) atomicAdd(q, (unsigned long long)x.hi);
    if (x.lo) atomicAdd(q + 1, (unsigned long long)x.lo);
  } else {
    atomicAdd(reinterpret_cast<float*>(acc) + e, v);
  }
}

// one wave per (64 consecutive pixels, slot index k): lanes along pixels, so that a face's pixels are neighbouring lanes
template <bool FLAT, bool DET>
__global__ __launch_bounds__(LT_TPB) void k_phong_bwd(PhongArgs a, const float* __restrict__ g_out,
                                                      float* __restrict__ g_texels, float* __restrict__ g_bary,
                                                      void* __restrict__ g_corners) {
  const size_t wave = ((size_t)blockIdx.x * LT_TPB + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const size_t pix = (wave / a.K) * 64 + lane;
  const int k = (int)(wave % a.K);
  const bool live = pix < a.P;
  const size_t s = live ? pix * a.K + k : 0;
  int64_t f = live ? a.p2f[s] : -1;
  Tri t;
  V3 nv[3], p, n, gp = v3(0.f, 0.f, 0.f), gn = gp, gc = gp;
  float b[3] = {0.f, 0.f, 0.f};
  bool face = false;
  if (live) {
    const int mesh = (int)(pix / a.pix_per_mesh);
    face = slot_geometry<FLAT>(a, s, f, t, nv, b, p, n);
    light_eval_bwd(a.consts + LT_NC * mesh, a.point, p, n, ld3(a.texels + 3 * s), ld3(g_out + 3 * s), gp, gn, gc);
    if (g_texels) st3(g_texels + 3 * s, gc);
    if (g_bary) {
      V3 gb = v3(0.f, 0.f, 0.f);
      if (face && !FLAT)
        gb = v3(dot(gp, t.v[0]) + dot(gn, nv[0]), dot(gp, t.v[1]) + dot(gn, nv[1]), dot(gp, t.v[2]) + dot(gn, nv[2]));
      st3(g_bary + 3 * s, gb);
    }
  }
  if (!g_corners) return;   // (uniform: a kernel argument)
  const int id = face ? (int)f : -1;
  const int prev = __shfl_up(id, 1, 64);
  const unsigned long long heads = __ballot(lane == 0 || prev != id);
  const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
  const int end = above ? lane + __ffsll((long long)above) - 1 : 63;
  const bool head = (heads >> lane) & 1ull;
  const size_t base = (size_t)(id < 0 ? 0 : id) * 18;
  if constexpr (FLAT) {
    // the face's mean position: a third of the position gradient to each corner; its normal: corner 0's normal slot
    const float third = 1.0f / 3.0f;
    const float q[6] = {third * gp.x, third * gp.y, third * gp.z, gn.x, gn.y, gn.z};
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const float v = run_sum(face ? q[j] : 0.0f, lane, end);
      if (head && id >= 0) {
        if (j < 3) {
          corner_add<DET>(g_corners, base + j, v);
          corner_add<DET>(g_corners, base + 6 + j, v);
          corner_add<DET>(g_corners, base + 12 + j, v);
        } else {
          corner_add<DET>(g_corners, base + j, v);
        }
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float q[6] = {b[i] * gp.x, b[i] * gp.y, b[i] * gp.z, b[i] * gn.x, b[i] * gn.y, b[i] * gn.z};
#pragma unroll
      for (int j = 0; j < 6; ++j) {
        const float v = run_sum(face ? q[j] : 0.0f, lane, end);
        if (head && id >= 0) corner_add<DET>(g_corners, base + 6 * i + j, v);
      }
    }
  }
}

// deterministic mode: the (hi, lo) integer sums -> float (k_shade_fix_finish of acfm_shade.hip)
__global__ __launch_bounds__(LT_TPB) void k_light_fix_finish(const long long* __restrict__ fix, size_t n,
                                                             float* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * LT_TPB + threadIdx.x;
  if (j < n) out[j] = frag_unsplit(fix[2 * j], fix[2 * j + 1]);
}

// face-corner buffer -> vertices: the position part summed over a vertex's corners, and the normal part likewise
// (phong: [V,3]) or read off corner 0 (flat: [F,3])
template <bool FLAT>
__global__ __launch_bounds__(LT_TPB) void k_corner_gather(const float* __restrict__ gc, const int* __restrict__ offsets,
                                                          const int* __restrict__ corners, int V, int F,
                                                          float* __restrict__ g_verts, float* __restrict__ g_normals) {
  const int t = blockIdx.x * LT_TPB + threadIdx.x;
  if (t < V) {
    int lo, hi;
    row_range(offsets, t, F, lo, hi);
    V3 gp = v3(0.f, 0.f, 0.f), gn = gp;
    for (int k = lo; k < hi; ++k) {
      const int c = corners[k];
      if (c < 0 || c >= 3 * F) continue;
      gp = gp + ld3(gc + 6 * (size_t)c);
      if (!FLAT) gn = gn + ld3(gc + 6 * (size_t)c + 3);
    }
    if (g_verts) st3(g_verts + 3 * (size_t)t, gp);
    if (!FLAT && g_normals) st3(g_normals + 3 * (size_t)t, gn);
  }
  if (FLAT && t < F && g_normals) st3(g_normals + 3 * (size_t)t, ld3(gc + 18 * (size_t)t + 3));
}

static unsigned lt_blocks(size_t n) { return (unsigned)((n + LT_TPB - 1) / LT_TPB); }
static bool bad_mesh(int V, int F) { return V <= 0 || F <= 0 || V > (1 << 28) || F > (1 << 28); }

static int phong_args(const int64_t* p2f, const float* bary, const float* texels, const float* verts,
                      const int64_t* faces, const float* normals, const float* consts, int point, int flat, size_t P,
                      int K, int pix_per_mesh, int F, int V, int N, const AcfmRasterTuning* tuning, Tune& tn,
                      PhongArgs& a) {
  if (!p2f || !texels || !verts || !faces || !normals || !consts || (!flat && !bary)) return ACFM_E_BADARG;
  if (P == 0 || K <= 0 || K > ACFM_MAX_K || P * (size_t)K > ((size_t)1 << 40) || bad_mesh(V, F)) return ACFM_E_BADARG;
  if (N <= 0 || pix_per_mesh <= 0 || P != (size_t)N * (size_t)pix_per_mesh) return ACFM_E_BADARG;
  if ((point != 0 && point != 1) || (flat != 0 && flat != 1)) return ACFM_E_BADARG;
  if (!tune_from(tuning, tn) || tn.f16) return ACFM_E_BADARG;
  a = PhongArgs{p2f, bary, texels, verts, faces, normals, consts, P, K, pix_per_mesh, F, V, N, point};
  return ACFM_OK;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_vertex_normals(const float* verts, const int64_t* faces, const int* offsets, const int* corners, int V, int F,
                        float* verts_normals, float* faces_normals, void* stream) {
  if (!verts || !faces || !offsets || !corners || bad_mesh(V, F) || (!verts_normals && !faces_normals))
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_vn_fwd, dim3(lt_blocks(V > F ? V : F)), dim3(LT_TPB), 0, (hipStream_t)stream, verts, faces,
                     offsets, corners, V, F, verts_normals, faces_normals);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_vertex_normals_backward(const float* verts, const int64_t* faces, const int* offsets, const int* corners,
                                 const float* grad_verts_normals, const float* grad_faces_normals, int V, int F,
                                 float* grad_verts, void* ws, size_t ws_bytes, void* stream) {
  if (!verts || !faces || !offsets || !corners || bad_mesh(V, F) || !grad_verts) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  float* g_raw = nullptr;
  if (grad_verts_normals) {
    if (!ws || ws_bytes < sizeof(float) * 3 * (size_t)V) return ACFM_E_WORKSPACE;
    g_raw = reinterpret_cast<float*>(ws);
    hipLaunchKernelGGL(k_vn_bwd_raw, dim3(lt_blocks(V)), dim3(LT_TPB), 0, st, verts, faces, offsets, corners,
                       grad_verts_normals, V, F, g_raw);
  }
  hipLaunchKernelGGL(k_vn_bwd_verts, dim3(lt_blocks(V)), dim3(LT_TPB), 0, st, verts, faces, offsets, corners,
                     (const float*)g_raw, grad_faces_normals, V, F, grad_verts);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_light_points(const float* points, const float* normals, const float* colours, const int64_t* mesh_idx,
                      const float* consts, int point_light, int M, int N, float* out, void* stream) {
  if (!points || !normals || !colours || !consts || !out || M <= 0 || N <= 0 || M > (1 << 28) ||
      (point_light != 0 && point_light != 1))
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_light_points_fwd, dim3(lt_blocks(M)), dim3(LT_TPB), 0, (hipStream_t)stream, points, normals,
                     colours, mesh_idx, consts, point_light, M, N, out);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_light_points_backward(const float* points, const float* normals, const float* colours,
                               const int64_t* mesh_idx, const float* consts, int point_light,
                               const float* grad_out, int M, int N, float* grad_points, float* grad_normals,
                               float* grad_colours, void* stream) {
  if (!points || !normals || !colours || !consts || !grad_out || M <= 0 || N <= 0 || M > (1 << 28) ||
      (point_light != 0 && point_light != 1))
    return ACFM_E_BADARG;
  if (!grad_points && !grad_normals && !grad_colours) return ACFM_OK;
  hipLaunchKernelGGL(k_light_points_bwd, dim3(lt_blocks(M)), dim3(LT_TPB), 0, (hipStream_t)stream, points, normals,
                     colours, mesh_idx, consts, grad_out, point_light, M, N, grad_points, grad_normals, grad_colours);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_phong_shade(const int64_t* pix_to_face, const float* bary, const float* texels, const float* verts,
                     const int64_t* faces, const float* normals, const float* consts, int point_light, int flat,
                     size_t P, int K, int pix_per_mesh, int F_packed, int V_packed, int N, float* colors,
                     const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  PhongArgs a;
  if (!colors || phong_args(pix_to_face, bary, texels, verts, faces, normals, consts, point_light, flat, P, K,
                            pix_per_mesh, F_packed, V_packed, N, tuning, tn, a))
    return ACFM_E_BADARG;
  const dim3 grid(lt_blocks(P * K)), blk(LT_TPB);
  if (flat)
    hipLaunchKernelGGL(k_phong_fwd<true>, grid, blk, 0, (hipStream_t)stream, a, colors);
  else
    hipLaunchKernelGGL(k_phong_fwd<false>, grid, blk, 0, (hipStream_t)stream, a, colors);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_phong_shade_backward(const int64_t* pix_to_face, const float* bary, const float* texels, const float* verts,
                              const int64_t* faces, const float* normals, const float* consts, int point_light,
                              int flat, const float* grad_colors, size_t P, int K, int pix_per_mesh, int F_packed,
                              int V_packed, int N, float* grad_texels, float* grad_bary, float* grad_corners, void* ws,
                              size_t ws_bytes, const AcfmRasterTuning* tuning, void* stream) {
  Tune tn;
  PhongArgs a;
  if (!grad_colors || phong_args(pix_to_face, bary, texels, verts, faces, normals, consts, point_light, flat, P, K,
                                 pix_per_mesh, F_packed, V_packed, N, tuning, tn, a))
    return ACFM_E_BADARG;
  if (!grad_texels && !grad_bary && !grad_corners) return ACFM_OK;
  hipStream_t st = (hipStream_t)stream;
  const size_t n_corner = (size_t)F_packed * 18;
  const bool det = tn.deterministic && grad_corners;
  void* acc = grad_corners;
  if (grad_corners) {
    if (det) {
      if (!ws || ws_bytes < 2 * sizeof(long long) * n_corner) return ACFM_E_WORKSPACE;
      acc = ws;
      if (zero_async(ws, 2 * sizeof(long long) * n_corner, st)) return ACFM_E_LAUNCH;
    } else if (zero_async(grad_corners, sizeof(float) * n_corner, st)) {
      return ACFM_E_LAUNCH;
    }
  }
  const size_t waves = ((P + 63) / 64) * (size_t)K;
  const dim3 grid(lt_blocks(waves * 64)), blk(LT_TPB);
  if (flat && det)
    hipLaunchKernelGGL((k_phong_bwd<true, true>), grid, blk, 0, st, a, grad_colors, grad_texels, grad_bary, acc);
  else if (flat)
    hipLaunchKernelGGL((k_phong_bwd<true, false>), grid, blk, 0, st, a, grad_colors, grad_texels, grad_bary, acc);
  else if (det)
    hipLaunchKernelGGL((k_phong_bwd<false, true>), grid, blk, 0, st, a, grad_colors, grad_texels, grad_bary, acc);
  else
    hipLaunchKernelGGL((k_phong_bwd<false, false>), grid, blk, 0, st, a, grad_colors, grad_texels, grad_bary, acc);
  if (det)
    hipLaunchKernelGGL(k_light_fix_finish, dim3(lt_blocks(n_corner)), dim3(LT_TPB), 0, st,
                       reinterpret_cast<const long long*>(ws), n_corner, grad_corners);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_corner_gather(const float* grad_corners, const int* offsets, const int* corners, int V, int F, int flat,
                       float* grad_verts, float* grad_normals, void* stream) {
  if (!grad_corners || !offsets || !corners || bad_mesh(V, F) || (flat != 0 && flat != 1) ||
      (!grad_verts && !grad_normals))
    return ACFM_E_BADARG;
  const dim3 grid(lt_blocks(V > F ? V : F)), blk(LT_TPB);
  if (flat)
    hipLaunchKernelGGL(k_corner_gather<true>, grid, blk, 0, (hipStream_t)stream, grad_corners, offsets, corners, V, F,
                       grad_verts, grad_normals);
  else
    hipLaunchKernelGGL(k_corner_gather<false>, grid, blk, 0, (hipStream_t)stream, grad_corners, offsets, corners, V, F,
                       grad_verts, grad_normals);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
