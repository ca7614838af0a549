// Camera hypothesis pipeline of the multiframe trainer in one kernel:
//   decode     embedding e[7] -> (s = relu(decay*e0 + 1) + 1e-12, t = e1..2, q = normalize(e3..6))
//              (multiframe/main.py:572-577, == :452-457, predictor.py:248-252), or, with --az_el_cam,
//              embedding e[6] -> (s = decay*e0 + bias, t = e1..2, q = q_cyc * (q_el * q_az)) from three Euler angles
//              (main.py:442-450, 554-566; nnutils/mesh_net.py:310-385)
//   mirror     blend with the pose of the horizontally flipped image by the frame's mirror flag:
//              (s, -tx, ty, q_y(pi) * standardize(q)), standardized      (main.py:97-125)
//   transform  crop/scale augmentation (a, dx, dy, flag) applied to scale and translation
//              (main.py:128-138)
// The reference runs this as ~60 elementwise torch kernels on [G*N, 7] tensors per step plus ~100
// in the backward (the camera embeddings are optimised through it, train_utils.py:186-213); here
// it is one thread per camera, forward and backward.  Row r of the [G*N, 7] batch belongs to frame
// r % N (the reference repeats the per-frame flags G times).
// The kernels are templates over the decode (DecodeQuat, DecodeAzel): the mirror / transform blends and the table
// look-ups exist once.
#include "acfm_common.h"

namespace acfm {

// mirror blend and transform blend of a decoded pose (s, tx, ty, q) -> o[7]; the two signs standardize applied are
// kept for the backward
struct CamBlend {
  float b_sign, raw0_sign;
};

__device__ __forceinline__ void cam_blend(float s, float tx, float ty, const float* __restrict__ q, float m,
                                          const float* __restrict__ tr, float* __restrict__ o, CamBlend& c) {
  // mirrored pose: q_m = standardize(q_y(pi) * standardize(q)), q_y(pi) = (0, 0, 1, 0)
  c.b_sign = q[0] < 0.0f ? -1.0f : 1.0f;
  const float b0 = c.b_sign * q[0], b1 = c.b_sign * q[1], b2 = c.b_sign * q[2], b3 = c.b_sign * q[3];
  float raw[4] = {-b2, b3, b0, -b1};
  c.raw0_sign = raw[0] < 0.0f ? -1.0f : 1.0f;
  const float pose[7] = {s, tx, ty, q[0], q[1], q[2], q[3]};
  const float mir[7] = {s, -tx, ty, c.raw0_sign * raw[0], c.raw0_sign * raw[1], c.raw0_sign * raw[2],
                        c.raw0_sign * raw[3]};
  float p1[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) p1[k] = (1.0f - m) * pose[k] + mir[k] * m;
  const float a = tr[0], dx = tr[1], dy = tr[2], f = tr[3];
  const float nw[7] = {p1[0] * a, p1[1] * a + dx, p1[2] * a + dy, p1[3], p1[4], p1[5], p1[6]};
#pragma unroll
  for (int k = 0; k < 7; ++k) o[k] = (1.0f - f) * p1[k] + nw[k] * f;
}

// d (s, tx, ty, q) from d camera; the derivative of standardize is the sign it applied
__device__ __forceinline__ void cam_blend_backward(const float* __restrict__ g, float m, const float* __restrict__ tr,
                                                   const CamBlend& c, float& gs, float& gtx, float& gty,
                                                   float* __restrict__ gq) {
  const float a = tr[0], f = tr[3];
  // out = (1-f) p1 + f new(p1)
  float gp1[7];
  gp1[0] = (1.0f - f) * g[0] + f * g[0] * a;
  gp1[1] = (1.0f - f) * g[1] + f * g[1] * a;
  gp1[2] = (1.0f - f) * g[2] + f * g[2] * a;
#pragma unroll
  for (int k = 3; k < 7; ++k) gp1[k] = (1.0f - f) * g[k] + f * g[k];
  // p1 = (1-m) pose + m mir
  float gpose[7], gmir[7];
#pragma unroll
  for (int k = 0; k < 7; ++k) { gpose[k] = (1.0f - m) * gp1[k]; gmir[k] = m * gp1[k]; }
  gs = gpose[0] + gmir[0];
  gtx = gpose[1] - gmir[1];
  gty = gpose[2] + gmir[2];
  // mir q = raw0_sign * raw, raw = (-b2, b3, b0, -b1), b = b_sign * q
  const float gr0 = c.raw0_sign * gmir[3], gr1 = c.raw0_sign * gmir[4], gr2 = c.raw0_sign * gmir[5],
              gr3 = c.raw0_sign * gmir[6];
  gq[0] = gpose[3] + c.b_sign * gr2;
  gq[1] = gpose[4] - c.b_sign * gr3;
  gq[2] = gpose[5] - c.b_sign * gr0;
  gq[3] = gpose[6] + c.b_sign * gr1;
}

// (scale, trans, quaternion) embedding: s = relu(decay*e0 + 1) + 1e-12, q = e3..6 / max(|e3..6|, 1e-12)
struct DecodeQuat {
  static constexpr int W = 7;
  float decay;

  __device__ __forceinline__ void forward(const float* __restrict__ e, float m, const float* __restrict__ tr,
                                          float* __restrict__ o) const {
    CamBlend c;
    float q[4], nrm;
    bool relu_on;
    blend(e, m, tr, o, c, q, nrm, relu_on);
  }

  // d embedding from d camera (the forward is re-evaluated)
  __device__ __forceinline__ void backward(const float* __restrict__ e, const float* __restrict__ g, float m,
                                           const float* __restrict__ tr, float* __restrict__ ge) const {
    float o[7], q[4], nrm, gs, gq[4];
    bool relu_on;
    CamBlend c;
    blend(e, m, tr, o, c, q, nrm, relu_on);
    cam_blend_backward(g, m, tr, c, gs, ge[1], ge[2], gq);
    // q = e / max(|e|, eps)
    if (nrm > 1e-12f) {
      const float dot = q[0] * gq[0] + q[1] * gq[1] + q[2] * gq[2] + q[3] * gq[3];
#pragma unroll
      for (int k = 0; k < 4; ++k) ge[3 + k] = (gq[k] - q[k] * dot) / nrm;
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) ge[3 + k] = gq[k] / 1e-12f;
    }
    ge[0] = relu_on ? decay * gs : 0.0f;
  }

 private:
  __device__ __forceinline__ void blend(const float* __restrict__ e, float m, const float* __restrict__ tr,
                                        float* __restrict__ o, CamBlend& c, float* __restrict__ q, float& nrm,
                                        bool& relu_on) const {
    const float pre = decay * e[0] + 1.0f;
    relu_on = pre > 0.0f;
    const float s = fmaxf(pre, 0.0f) + 1e-12f;
    nrm = sqrtf(e[3] * e[3] + e[4] * e[4] + e[5] * e[5] + e[6] * e[6]);
    const float d = fmaxf(nrm, 1e-12f);
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = e[3 + k] / d;
    cam_blend(s, e[1], e[2], q, m, tr, o, c);
  }
};

// (scale, trans, azimuth, elevation, cyclo-rotation) embedding of --az_el_cam (mesh_net.py:310-353): s = decay*e0 + bias
// (no relu: a negative scale passes through), az = az_range e3, el = pi - el_range e4, cyc = cyc_range e5 (ranges in
// radians), q = q_cyc (x) (q_el (x) q_az) with q_az about +y, q_el about +x, q_cyc about +z; Hamilton products on
// (w, x, y, z), not renormalised.  Full-range sincosf: azimuths reach several turns.
struct DecodeAzel {
  static constexpr int W = 6;
  float decay, bias, az_range, el_range, cyc_range;

  __device__ __forceinline__ void forward(const float* __restrict__ e, float m, const float* __restrict__ tr,
                                          float* __restrict__ o) const {
    CamBlend c;
    float p[4], q[4], cc, sc;
    blend(e, m, tr, o, c, p, q, cc, sc);
  }

  __device__ __forceinline__ void backward(const float* __restrict__ e, const float* __restrict__ g, float m,
                                           const float* __restrict__ tr, float* __restrict__ ge) const {
    float o[7], p[4], q[4], cc, sc, gs, gq[4];
    CamBlend c;
    blend(e, m, tr, o, c, p, q, cc, sc);
    cam_blend_backward(g, m, tr, c, gs, ge[1], ge[2], gq);
    // q = q_cyc (x) p: dq / d(cyc/2) = (-q3, -q2, q1, q0)
    const float g_hc = -q[3] * gq[0] - q[2] * gq[1] + q[1] * gq[2] + q[0] * gq[3];
    const float gp[4] = {cc * gq[0] + sc * gq[3], cc * gq[1] + sc * gq[2], cc * gq[2] - sc * gq[1],
                         cc * gq[3] - sc * gq[0]};
    // p = (ce ca, se ca, ce sa, se sa): dp / d(az/2) = (-p2, -p3, p0, p1), dp / d(el/2) = (-p1, p0, -p3, p2)
    const float g_ha = -p[2] * gp[0] - p[3] * gp[1] + p[0] * gp[2] + p[1] * gp[3];
    const float g_he = -p[1] * gp[0] + p[0] * gp[1] - p[3] * gp[2] + p[2] * gp[3];
    ge[0] = decay * gs;
    ge[3] = 0.5f * az_range * g_ha;
    ge[4] = -0.5f * el_range * g_he;
    ge[5] = 0.5f * cyc_range * g_hc;
  }

 private:
  __device__ __forceinline__ void blend(const float* __restrict__ e, float m, const float* __restrict__ tr,
                                        float* __restrict__ o, CamBlend& c, float* __restrict__ p,
                                        float* __restrict__ q, float& cc, float& sc) const {
    const float s = decay * e[0] + bias;
    const float az = az_range * e[3], el = 3.14159265358979323846f - el_range * e[4], cyc = cyc_range * e[5];
    float sa, ca, se, ce;
    sincosf(az / 2.0f, &sa, &ca);
    sincosf(el / 2.0f, &se, &ce);
    sincosf(cyc / 2.0f, &sc, &cc);
    // q_el (x) q_az = (ce, se, 0, 0) (x) (ca, 0, sa, 0)
    p[0] = ce * ca; p[1] = se * ca; p[2] = ce * sa; p[3] = se * sa;
    // (cc, 0, 0, sc) (x) p
    q[0] = cc * p[0] - sc * p[3];
    q[1] = cc * p[1] - sc * p[2];
    q[2] = cc * p[2] + sc * p[1];
    q[3] = cc * p[3] + sc * p[0];
    cam_blend(s, e[1], e[2], q, m, tr, o, c);
  }
};

template <class Decode>
__global__ void k_camera_fwd(const float* __restrict__ emb, const int64_t* __restrict__ mirror,
                             const float* __restrict__ transforms, int R, int N, Decode dec,
                             float* __restrict__ out) {
  constexpr int W = Decode::W;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int n = r % N;
  float e[W], o[7];
#pragma unroll
  for (int k = 0; k < W; ++k) e[k] = emb[(size_t)r * W + k];
  const float tr[4] = {transforms[4 * n], transforms[4 * n + 1], transforms[4 * n + 2], transforms[4 * n + 3]};
  dec.forward(e, (float)mirror[n], tr, o);
#pragma unroll
  for (int k = 0; k < 7; ++k) out[(size_t)r * 7 + k] = o[k];
}

// The same straight from the per-hypothesis embedding tables (mesh_net.py:436-444: one nn.Embedding(frames, 7) per
// hypothesis; :405-416: (frames, 6) with --az_el_cam): row r = g N + n reads tables[sel ? sel[r] : g][frames_idx[n]];
// the backward adds into dense per-table gradients (zeroed by the entry point; float atomics: a frame id that occurs
// twice in the batch, or two hypotheses that select one table for a frame, sum in the cell as nn.Embedding's backward
// does; with distinct ids every cell gets one add and the result does not depend on the order).
// A frame id outside [0, n_frames) or a table id outside [0, n_tables) -- nn.Embedding raises on those (main.py:551-570)
// -- never becomes an address: the forward writes a NaN camera for that row (the loss of the step is then NaN, loudly,
// without a host synchronisation inside a captured step), the backward skips it; ops.camera_pipeline_tables(check=True)
// is the host-side check for data-loader batches.
constexpr int CAM_MAX_TABLES = 32;
struct CamTables {
  const float* t[CAM_MAX_TABLES];
  float* g[CAM_MAX_TABLES];
};
template <class Decode>
__global__ void k_camera_fwd_tables(CamTables tb, const int64_t* __restrict__ frames_idx, const int64_t* __restrict__ sel,
                                    const int64_t* __restrict__ mirror, const float* __restrict__ transforms, int R, int N,
                                    int n_tables, int n_frames, Decode dec, float* __restrict__ out) {
  constexpr int W = Decode::W;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int n = r % N;
  const int64_t table = sel ? sel[r] : (int64_t)(r / N);
  const int64_t frame = frames_idx[n];
  if (table < 0 || table >= n_tables || frame < 0 || frame >= n_frames) {
#pragma unroll
    for (int k = 0; k < 7; ++k) out[(size_t)r * 7 + k] = __builtin_nanf("");
    return;
  }
  const float* src = tb.t[table] + (size_t)frame * W;
  float e[W], o[7];
#pragma unroll
  for (int k = 0; k < W; ++k) e[k] = src[k];
  const float tr[4] = {transforms[4 * n], transforms[4 * n + 1], transforms[4 * n + 2], transforms[4 * n + 3]};
  dec.forward(e, (float)mirror[n], tr, o);
#pragma unroll
  for (int k = 0; k < 7; ++k) out[(size_t)r * 7 + k] = o[k];
}

template <class Decode>
__global__ void k_camera_bwd(const float* __restrict__ emb, const int64_t* __restrict__ mirror,
                             const float* __restrict__ transforms, const float* __restrict__ gout, int R,
                             int N, Decode dec, float* __restrict__ gemb) {
  constexpr int W = Decode::W;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int n = r % N;
  float e[W], g[7], ge[W];
#pragma unroll
  for (int k = 0; k < W; ++k) e[k] = emb[(size_t)r * W + k];
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] = gout[(size_t)r * 7 + k];
  const float tr[4] = {transforms[4 * n], transforms[4 * n + 1], transforms[4 * n + 2], transforms[4 * n + 3]};
  dec.backward(e, g, (float)mirror[n], tr, ge);
#pragma unroll
  for (int k = 0; k < W; ++k) gemb[(size_t)r * W + k] = ge[k];
}

template <class Decode>
__global__ void k_camera_bwd_tables(CamTables tb, const int64_t* __restrict__ frames_idx, const int64_t* __restrict__ sel,
                                    const int64_t* __restrict__ mirror, const float* __restrict__ transforms,
                                    const float* __restrict__ gout, int R, int N, int n_tables, int n_frames,
                                    Decode dec) {
  constexpr int W = Decode::W;
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const int n = r % N;
  const int64_t table = sel ? sel[r] : (int64_t)(r / N);
  const int64_t frame = frames_idx[n];
  if (table < 0 || table >= n_tables || frame < 0 || frame >= n_frames) return;   // (the forward wrote NaN for this row)
  if (!tb.g[table]) return;
  const size_t row = (size_t)frame * W;
  const float* src = tb.t[table] + row;
  float e[W], g[7], ge[W];
#pragma unroll
  for (int k = 0; k < W; ++k) e[k] = src[k];
#pragma unroll
  for (int k = 0; k < 7; ++k) g[k] = gout[(size_t)r * 7 + k];
  const float tr[4] = {transforms[4 * n], transforms[4 * n + 1], transforms[4 * n + 2], transforms[4 * n + 3]};
  dec.backward(e, g, (float)mirror[n], tr, ge);
#pragma unroll
  for (int k = 0; k < W; ++k) atomicAdd(tb.g[table] + row + k, ge[k]);
}

// The table gradients without atomics and without a zero fill in front: one thread per cell row (table, frame) of the
// dense gradients walks the batch -- frames n in order, then hypotheses g in order -- and sums the rows that looked its
// cell up, in that fixed order; a row nobody looked up is written as zeros.  One launch, bit-reproducible; an id outside
// the tables matches no cell, so it contributes nothing and is never an address.  The walk is N index reads per thread
// plus G per matching frame: n_tables n_frames N in all, small beside the dense gradient itself while the batch is.
// (The 7-float tables keep the scatter above: with three or more addends in a cell its sums are in another order.)
template <class Decode>
__global__ void k_camera_bwd_tables_gather(CamTables tb, const int64_t* __restrict__ frames_idx,
                                           const int64_t* __restrict__ sel, const int64_t* __restrict__ mirror,
                                           const float* __restrict__ transforms, const float* __restrict__ gout, int R,
                                           int N, int n_tables, int n_frames, Decode dec) {
  constexpr int W = Decode::W;
  const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (cell >= (int64_t)n_tables * n_frames) return;
  const int table = (int)(cell / n_frames);
  const int64_t frame = cell % n_frames;
  if (!tb.g[table]) return;
  const size_t row = (size_t)frame * W;
  float e[W], acc[W];
#pragma unroll
  for (int k = 0; k < W; ++k) { e[k] = tb.t[table][row + k]; acc[k] = 0.0f; }
  const int G = R / N;
  for (int n = 0; n < N; ++n) {
    if (frames_idx[n] != frame) continue;
    const float tr[4] = {transforms[4 * n], transforms[4 * n + 1], transforms[4 * n + 2], transforms[4 * n + 3]};
    const float m = (float)mirror[n];
    for (int g = 0; g < G; ++g) {
      const int r = g * N + n;
      if ((sel ? sel[r] : (int64_t)g) != table) continue;
      float go[7], ge[W];
#pragma unroll
      for (int k = 0; k < 7; ++k) go[k] = gout[(size_t)r * 7 + k];
      dec.backward(e, go, m, tr, ge);
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] += ge[k];
    }
  }
#pragma unroll
  for (int k = 0; k < W; ++k) tb.g[table][row + k] = acc[k];
}

// host side of the four pipeline entry points, once per decode
template <class Decode>
int camera_pipeline(const float* emb, const int64_t* mirror_flag, const float* transforms, int R, int N, Decode dec,
                    float* cams, void* stream) {
  if (!emb || !mirror_flag || !transforms || !cams || R <= 0 || N <= 0 || R % N != 0) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_fwd<Decode>, dim3((R + 127) / 128), dim3(128), 0, (hipStream_t)stream, emb, mirror_flag,
                     transforms, R, N, dec, cams);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

template <class Decode>
int camera_pipeline_backward(const float* emb, const int64_t* mirror_flag, const float* transforms,
                             const float* grad_cams, int R, int N, Decode dec, float* grad_emb, void* stream) {
  if (!emb || !mirror_flag || !transforms || !grad_cams || !grad_emb || R <= 0 || N <= 0 || R % N != 0)
    return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_bwd<Decode>, dim3((R + 127) / 128), dim3(128), 0, (hipStream_t)stream, emb, mirror_flag,
                     transforms, grad_cams, R, N, dec, grad_emb);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

template <class Decode>
int camera_pipeline_tables(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                           const int64_t* selected, const int64_t* mirror_flag, const float* transforms, int R, int N,
                           Decode dec, float* cams, void* stream) {
  if (!tables || !frames_idx || !mirror_flag || !transforms || !cams || n_tables <= 0 || n_tables > CAM_MAX_TABLES ||
      n_frames <= 0 || R <= 0 || N <= 0 || R % N != 0 || (!selected && R / N > n_tables))
    return ACFM_E_BADARG;
  CamTables tb;
  for (int i = 0; i < CAM_MAX_TABLES; ++i) {
    tb.t[i] = i < n_tables ? (const float*)tables[i] : nullptr;
    tb.g[i] = nullptr;
    if (i < n_tables && !tb.t[i]) return ACFM_E_BADARG;
  }
  hipLaunchKernelGGL(k_camera_fwd_tables<Decode>, dim3((R + 127) / 128), dim3(128), 0, (hipStream_t)stream, tb,
                     frames_idx, selected, mirror_flag, transforms, R, N, n_tables, n_frames, dec, cams);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

// gather = false: zero the dense gradients (one fill per table), then scatter with float atomics (the 7-float tables);
// gather = true: k_camera_bwd_tables_gather, one launch in all (the az/el tables)
template <class Decode, bool gather>
int camera_pipeline_tables_backward(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                    const int64_t* selected, const int64_t* mirror_flag, const float* transforms,
                                    const float* grad_cams, int R, int N, Decode dec, void* const* grad_tables,
                                    void* stream) {
  if (!tables || !grad_tables || !frames_idx || !mirror_flag || !transforms || !grad_cams || n_tables <= 0 ||
      n_tables > CAM_MAX_TABLES || n_frames <= 0 || R <= 0 || N <= 0 || R % N != 0 || (!selected && R / N > n_tables))
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  CamTables tb;
  for (int i = 0; i < CAM_MAX_TABLES; ++i) {
    tb.t[i] = i < n_tables ? (const float*)tables[i] : nullptr;
    tb.g[i] = i < n_tables ? (float*)grad_tables[i] : nullptr;
    if (i < n_tables && !tb.t[i]) return ACFM_E_BADARG;
    if (!gather && tb.g[i] && zero_async(tb.g[i], sizeof(float) * Decode::W * (size_t)n_frames, st) != ACFM_OK)
      return ACFM_E_LAUNCH;
  }
  if (gather) {
    const int64_t cells = (int64_t)n_tables * n_frames;
    if ((cells + 127) / 128 > 0x7fffffffLL) return ACFM_E_BADARG;
    hipLaunchKernelGGL(k_camera_bwd_tables_gather<Decode>, dim3((unsigned)((cells + 127) / 128)), dim3(128), 0, st, tb,
                       frames_idx, selected, mirror_flag, transforms, grad_cams, R, N, n_tables, n_frames, dec);
  } else {
    hipLaunchKernelGGL(k_camera_bwd_tables<Decode>, dim3((R + 127) / 128), dim3(128), 0, st, tb, frames_idx, selected,
                       mirror_flag, transforms, grad_cams, R, N, n_tables, n_frames, dec);
  }
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

// cam = (s, tx, ty, q / max(|q|, 1e-12)): the camera the refinement loop renders with while it
// optimises scale, translation and an unnormalised quaternion (predictor.py:301-308:
// torch.cat([scale, trans, F.normalize(quat)])); one thread per camera, forward and backward
__global__ void k_camera_normalize(const float* __restrict__ raw, int N, float* __restrict__ out) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* e = raw + (size_t)n * 7;
  const float nrm = sqrtf(e[3] * e[3] + e[4] * e[4] + e[5] * e[5] + e[6] * e[6]);
  const float d = fmaxf(nrm, 1e-12f);
  float* o = out + (size_t)n * 7;
  o[0] = e[0]; o[1] = e[1]; o[2] = e[2];
#pragma unroll
  for (int k = 3; k < 7; ++k) o[k] = e[k] / d;
}

__global__ void k_camera_normalize_bwd(const float* __restrict__ raw, const float* __restrict__ gout, int N,
                                       float* __restrict__ graw) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float* e = raw + (size_t)n * 7;
  const float* g = gout + (size_t)n * 7;
  float* o = graw + (size_t)n * 7;
  o[0] = g[0]; o[1] = g[1]; o[2] = g[2];
  const float nrm = sqrtf(e[3] * e[3] + e[4] * e[4] + e[5] * e[5] + e[6] * e[6]);
  if (nrm > 1e-12f) {
    const float q0 = e[3] / nrm, q1 = e[4] / nrm, q2 = e[5] / nrm, q3 = e[6] / nrm;
    const float dot = q0 * g[3] + q1 * g[4] + q2 * g[5] + q3 * g[6];
    o[3] = (g[3] - q0 * dot) / nrm; o[4] = (g[4] - q1 * dot) / nrm;
    o[5] = (g[5] - q2 * dot) / nrm; o[6] = (g[6] - q3 * dot) / nrm;
  } else {
#pragma unroll
    for (int k = 3; k < 7; ++k) o[k] = g[k] / 1e-12f;
  }
}

// pose of the horizontally flipped image of an already decoded camera (multiframe/main.py:97-125 with flag 1):
// (s, tx, ty, q) -> (s, -tx, ty, standardize(q_y(pi) * standardize(q))), q_y(pi) = (0, 0, 1, 0); one thread per camera.
// (The reference's chain of pytorch3d.transforms calls is ~35 elementwise launches on [R,4] tensors.)
__global__ void k_camera_mirror(const float* __restrict__ cams, int R, float* __restrict__ out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= R) return;
  const float* c = cams + (size_t)r * 7;
  const float sg = c[3] < 0.0f ? -1.0f : 1.0f;
  const float b0 = sg * c[3], b1 = sg * c[4], b2 = sg * c[5], b3 = sg * c[6];
  const float raw[4] = {-b2, b3, b0, -b1};
  const float s2 = raw[0] < 0.0f ? -1.0f : 1.0f;
  float* o = out + (size_t)r * 7;
  o[0] = c[0]; o[1] = -c[1]; o[2] = c[2];
  o[3] = s2 * raw[0]; o[4] = s2 * raw[1]; o[5] = s2 * raw[2]; o[6] = s2 * raw[3];
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_camera_pipeline(const float* emb, const int64_t* mirror_flag, const float* transforms, int R, int N,
                         float scale_lr_decay, float* cams, void* stream) {
  return camera_pipeline(emb, mirror_flag, transforms, R, N, DecodeQuat{scale_lr_decay}, cams, stream);
}

int acfm_camera_pipeline_backward(const float* emb, const int64_t* mirror_flag, const float* transforms,
                                  const float* grad_cams, int R, int N, float scale_lr_decay, float* grad_emb,
                                  void* stream) {
  return camera_pipeline_backward(emb, mirror_flag, transforms, grad_cams, R, N, DecodeQuat{scale_lr_decay}, grad_emb,
                                  stream);
}

int acfm_camera_pipeline_tables(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                const int64_t* selected, const int64_t* mirror_flag, const float* transforms, int R,
                                int N, float scale_lr_decay, float* cams, void* stream) {
  return camera_pipeline_tables(tables, n_tables, n_frames, frames_idx, selected, mirror_flag, transforms, R, N,
                                DecodeQuat{scale_lr_decay}, cams, stream);
}

int acfm_camera_pipeline_tables_backward(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                         const int64_t* selected, const int64_t* mirror_flag, const float* transforms,
                                         const float* grad_cams, int R, int N, float scale_lr_decay,
                                         void* const* grad_tables, void* stream) {
  return camera_pipeline_tables_backward<DecodeQuat, false>(tables, n_tables, n_frames, frames_idx, selected, mirror_flag,
                                                            transforms, grad_cams, R, N, DecodeQuat{scale_lr_decay},
                                                            grad_tables, stream);
}

int acfm_camera_pipeline_azel(const float* emb, const int64_t* mirror_flag, const float* transforms, int R, int N,
                              float scale_lr_decay, float scale_bias, float az_range, float el_range, float cyc_range,
                              float* cams, void* stream) {
  return camera_pipeline(emb, mirror_flag, transforms, R, N,
                         DecodeAzel{scale_lr_decay, scale_bias, az_range, el_range, cyc_range}, cams, stream);
}

int acfm_camera_pipeline_azel_backward(const float* emb, const int64_t* mirror_flag, const float* transforms,
                                       const float* grad_cams, int R, int N, float scale_lr_decay, float scale_bias,
                                       float az_range, float el_range, float cyc_range, float* grad_emb, void* stream) {
  return camera_pipeline_backward(emb, mirror_flag, transforms, grad_cams, R, N,
                                  DecodeAzel{scale_lr_decay, scale_bias, az_range, el_range, cyc_range}, grad_emb,
                                  stream);
}

int acfm_camera_pipeline_azel_tables(const void* const* tables, int n_tables, int n_frames, const int64_t* frames_idx,
                                     const int64_t* selected, const int64_t* mirror_flag, const float* transforms, int R,
                                     int N, float scale_lr_decay, float scale_bias, float az_range, float el_range,
                                     float cyc_range, float* cams, void* stream) {
  return camera_pipeline_tables(tables, n_tables, n_frames, frames_idx, selected, mirror_flag, transforms, R, N,
                                DecodeAzel{scale_lr_decay, scale_bias, az_range, el_range, cyc_range}, cams, stream);
}

int acfm_camera_pipeline_azel_tables_backward(const void* const* tables, int n_tables, int n_frames,
                                              const int64_t* frames_idx, const int64_t* selected,
                                              const int64_t* mirror_flag, const float* transforms,
                                              const float* grad_cams, int R, int N, float scale_lr_decay,
                                              float scale_bias, float az_range, float el_range, float cyc_range,
                                              void* const* grad_tables, void* stream) {
  return camera_pipeline_tables_backward<DecodeAzel, true>(
      tables, n_tables, n_frames, frames_idx, selected, mirror_flag, transforms, grad_cams, R, N,
      DecodeAzel{scale_lr_decay, scale_bias, az_range, el_range, cyc_range}, grad_tables, stream);
}

int acfm_camera_mirror(const float* cams, int R, float* out, void* stream) {
  if (!cams || !out || R <= 0) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_mirror, dim3((R + 127) / 128), dim3(128), 0, (hipStream_t)stream, cams, R, out);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_camera_normalize(const float* cam_raw, int N, float* cams, void* stream) {
  if (!cam_raw || !cams || N <= 0) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_normalize, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream, cam_raw, N, cams);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_camera_normalize_backward(const float* cam_raw, const float* grad_cams, int N, float* grad_raw,
                                   void* stream) {
  if (!cam_raw || !grad_cams || !grad_raw || N <= 0) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_normalize_bwd, dim3((N + 127) / 128), dim3(128), 0, (hipStream_t)stream, cam_raw,
                     grad_cams, N, grad_raw);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
