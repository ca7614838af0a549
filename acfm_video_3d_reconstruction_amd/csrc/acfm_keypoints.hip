// Keypoint supervision for gfx950: the vert2kp softmax with its entropy prior, the keypoint head (A @ verts, projection,
// L1 loss, pixel error) and the camera head's loss against the most probable hypothesis, each with its backward.
// Replaces mesh_net.py:504-519's softmax(vert2kp), multiframe/main.py:503-511, 690-696, 753-762, loss_utils.py:256-289,
// 330-356 and evaluate.py:156-158 and their autograd mirrors (about 40 small torch launches each way).
//
// The loops over V, K and Nv are latency bound (a few loads per trip feeding one sum): they are unrolled so that their
// loads are in flight together; every sum keeps the order in which it is written.
// No kernel here waits on another workgroup and none uses a float atomic: every sum across workgroups is a launch of
// its own or a loop in fixed order inside one workgroup, so every output repeats its bits from run to run.
#include "acfm_common.h"

namespace acfm {

constexpr int KP_MAX_K = 64;         // one lane per keypoint
constexpr int KW_TPB = 1024;         // weights: one workgroup, a wave per row of the logits
constexpr int KW_WAVES = KW_TPB / 64;
constexpr int KH_TPB = 1024;         // head: one workgroup per row of verts, a wave per keypoint / per hypothesis
constexpr int KH_WAVES = KH_TPB / 64;
constexpr int KG_TPB = 256;          // grad_A: a thread per (k, v)
constexpr int CL_TPB = 256;          // camera loss: one workgroup
constexpr int CL_WAVES = CL_TPB / 64;

// ---------------------------------------------------------------------------------------------- (a) weights
// A = softmax(logits, 1); stats[k] = (row maximum, log of the row's sum of exp); entropy = mean_k(-sum_v A logA) with
// logA = (logit - max) - log(sum): finite where A underflows to 0 (A logA = 0 there), where log(A) is -inf.
__global__ __launch_bounds__(KW_TPB) void k_kp_weights_fwd(const float* __restrict__ logits, int K, int V,
                                                           float* __restrict__ A, float* __restrict__ entropy,
                                                           float* __restrict__ stats) {
  __shared__ float s_ent[KP_MAX_K];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int k = wv; k < K; k += KW_WAVES) {
    const float* x = logits + (size_t)k * V;
    float m = -INFINITY;
#pragma unroll 8
    for (int v = lane; v < V; v += 64) m = fmaxf(m, x[v]);
    m = wave_max(m);
    float s = 0.f;
#pragma unroll 8
    for (int v = lane; v < V; v += 64) s += expf(x[v] - m);
    s = wave_sum(s);
    const float ls = logf(s);
    float h = 0.f;
#pragma unroll 4
    for (int v = lane; v < V; v += 64) {
      const float d = x[v] - m;
      const float a = expf(d) / s;
      A[(size_t)k * V + v] = a;
      h += a * (d - ls);
    }
    h = wave_sum(h);
    if (lane == 0) {
      s_ent[k] = -h;
      stats[2 * k] = m;
      stats[2 * k + 1] = ls;
    }
  }
  __syncthreads();
  if (tid == 0) {
    float e = 0.f;
    for (int k = 0; k < K; ++k) e += s_ent[k];
    entropy[0] = e / (float)K;
  }
}

// grad_logits = A (g - sum_v A g), g = grad_A - (grad_entropy / K) (logA + 1); either gradient may be absent.
__global__ __launch_bounds__(KW_TPB) void k_kp_weights_bwd(const float* __restrict__ logits, const float* __restrict__ A,
                                                           const float* __restrict__ stats,
                                                           const float* __restrict__ grad_A,
                                                           const float* __restrict__ grad_entropy, int K, int V,
                                                           float* __restrict__ grad_logits) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float ce = grad_entropy ? grad_entropy[0] / (float)K : 0.f;
  for (int k = wv; k < K; k += KW_WAVES) {
    const size_t row = (size_t)k * V;
    const float m = stats[2 * k], ls = stats[2 * k + 1];
    float dot = 0.f;
#pragma unroll 4
    for (int v = lane; v < V; v += 64) {
      float g = grad_A ? grad_A[row + v] : 0.f;
      if (grad_entropy) g -= ce * (((logits[row + v] - m) - ls) + 1.f);
      dot += A[row + v] * g;
    }
    dot = wave_sum(dot);
#pragma unroll 4
    for (int v = lane; v < V; v += 64) {
      float g = grad_A ? grad_A[row + v] : 0.f;
      if (grad_entropy) g -= ce * (((logits[row + v] - m) - ls) + 1.f);
      grad_logits[row + v] = A[row + v] * (g - dot);
    }
  }
}

// ---------------------------------------------------------------------------------------------- (b) head
// Workgroup r: kp_verts[r] = A @ verts[r] (a wave per keypoint, lanes over V), then its hypotheses n = r, r + Nv, ...
// one per wave, a lane per keypoint: projection (project_point, offset 0), L1 loss against kp_gt[n % Ng], pixel error.
__global__ __launch_bounds__(KH_TPB) void k_kp_head_fwd(const float* __restrict__ A, const float* __restrict__ verts,
                                                        const float* __restrict__ cams, const float* __restrict__ kp_gt,
                                                        int K, int V, int N, int Nv, int Ng, float half_size,
                                                        float* __restrict__ kp_verts, float* __restrict__ kp_pred,
                                                        float* __restrict__ loss, float* __restrict__ kp_err) {
  __shared__ float s_kpv[KP_MAX_K * 3];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* X = verts + (size_t)r * V * 3;
  for (int k = wv; k < K; k += KH_WAVES) {
    const float* a = A + (size_t)k * V;
    float sx = 0.f, sy = 0.f, sz = 0.f;
#pragma unroll 4
    for (int v = lane; v < V; v += 64) {
      const float w = a[v];
      sx += w * X[3 * v]; sy += w * X[3 * v + 1]; sz += w * X[3 * v + 2];
    }
    sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz);
    if (lane == 0) {
      s_kpv[3 * k] = sx; s_kpv[3 * k + 1] = sy; s_kpv[3 * k + 2] = sz;
      float* o = kp_verts + ((size_t)r * K + k) * 3;
      o[0] = sx; o[1] = sy; o[2] = sz;
    }
  }
  __syncthreads();
  const bool on = lane < K;
  const float x = on ? s_kpv[3 * lane] : 0.f, y = on ? s_kpv[3 * lane + 1] : 0.f, z = on ? s_kpv[3 * lane + 2] : 0.f;
  for (int n = r + wv * Nv; n < N; n += KH_WAVES * Nv) {      // (wave-uniform: the wave sums below see all 64 lanes)
    float px, py, pz;
    project_point(cams + 7 * (size_t)n, x, y, z, 0.f, px, py, pz);
    if (on) {
      float* o = kp_pred + ((size_t)n * K + lane) * 2;
      o[0] = px; o[1] = py;
    }
    if (!kp_gt) continue;
    float term = 0.f, vis = 0.f;
    if (on) {
      const float* g = kp_gt + ((size_t)(n % Ng) * K + lane) * 3;
      const float dx = px - g[0], dy = py - g[1];
      vis = g[2] > 0.f ? 1.f : 0.f;
      term = (fabsf(dx) + fabsf(dy)) * vis;
      if (kp_err) kp_err[(size_t)n * K + lane] = sqrtf(dx * dx + dy * dy) * half_size;
    }
    term = wave_sum(term);
    vis = wave_sum(vis);
    if (lane == 0 && loss) loss[n] = (term / (float)K) / (vis / (float)K + 1e-4f);
  }
}

// ---------------------------------------------------------------------------------------------- (c) head backward
// The adjoint of (px, py) = project_point(c, X) for the upstream (gx, gy): the arithmetic of k_project_bwd
// (acfm_project.hip) with gz = 0.  acc[7] += d cams row, dX = d point.
__device__ __forceinline__ void project_xy_adjoint(const float* __restrict__ c, float X, float Y, float Z, float gx,
                                                   float gy, float* acc, float& dX, float& dY, float& dZ) {
  const float s = c[0], q0 = c[3], ux = c[4], uy = c[5], uz = c[6];
  const float uu = ux * ux + uy * uy + uz * uz;
  const float a = q0 * q0 - uu;
  const float gz = 0.f;
  const float uX = ux * X + uy * Y + uz * Z;
  const float cx = uy * Z - uz * Y, cy = uz * X - ux * Z, cz = ux * Y - uy * X;  // u x X
  const float rx = a * X + 2.f * uX * ux + 2.f * q0 * cx;
  const float ry = a * Y + 2.f * uX * uy + 2.f * q0 * cy;
  const float rz = a * Z + 2.f * uX * uz + 2.f * q0 * cz;
  acc[0] = gx * rx + gy * ry + gz * rz;
  acc[1] = gx;
  acc[2] = gy;
  const float Gx = s * gx, Gy = s * gy, Gz = s * gz;
  const float GX = Gx * X + Gy * Y + Gz * Z;
  const float Gu = Gx * ux + Gy * uy + Gz * uz;
  acc[3] = 2.f * q0 * GX + 2.f * (Gx * cx + Gy * cy + Gz * cz);
  const float xg_x = Y * Gz - Z * Gy, xg_y = Z * Gx - X * Gz, xg_z = X * Gy - Y * Gx;  // X x G
  acc[4] = -2.f * GX * ux + 2.f * Gu * X + 2.f * uX * Gx + 2.f * q0 * xg_x;
  acc[5] = -2.f * GX * uy + 2.f * Gu * Y + 2.f * uX * Gy + 2.f * q0 * xg_y;
  acc[6] = -2.f * GX * uz + 2.f * Gu * Z + 2.f * uX * Gz + 2.f * q0 * xg_z;
  const float gu_x = Gy * uz - Gz * uy, gu_y = Gz * ux - Gx * uz, gu_z = Gx * uy - Gy * ux;  // G x u
  dX = a * Gx + 2.f * Gu * ux + 2.f * q0 * gu_x;
  dY = a * Gy + 2.f * Gu * uy + 2.f * q0 * gu_y;
  dZ = a * Gz + 2.f * Gu * uz + 2.f * q0 * gu_z;
}

// First launch, the head's grid.  The row's hypotheses are taken KH_WAVES at a time, one per wave and a lane per
// keypoint; each wave leaves its d kp_verts in LDS and wave 0 adds them in ascending n.  Then d kp_verts goes to the
// workspace (the second launch reads it) and grad_verts[r,v] = sum_k A[k,v] dkpv[r,k], a thread per vertex, k ascending.
__global__ __launch_bounds__(KH_TPB) void k_kp_head_bwd(const float* __restrict__ A, const float* __restrict__ cams,
                                                        const float* __restrict__ kp_gt,
                                                        const float* __restrict__ kp_verts,
                                                        const float* __restrict__ kp_pred,
                                                        const float* __restrict__ grad_loss,
                                                        const float* __restrict__ grad_kp_pred,
                                                        const float* __restrict__ grad_kp_verts, int K, int V, int N,
                                                        int Nv, int Ng, float* __restrict__ dkpv,
                                                        float* __restrict__ grad_verts, float* __restrict__ grad_cams) {
  __shared__ float s_part[KH_WAVES][KP_MAX_K * 3];
  __shared__ float s_dkpv[KP_MAX_K * 3];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool on = lane < K;
  const float* kv = kp_verts + ((size_t)r * K + (on ? lane : 0)) * 3;
  const float X = kv[0], Y = kv[1], Z = kv[2];
  float ax = 0.f, ay = 0.f, az = 0.f;            // wave 0: d kp_verts[r, lane] summed over the hypotheses so far
  const bool have_g = (grad_loss && kp_gt) || grad_kp_pred;
  for (int base = r; have_g && base < N; base += KH_WAVES * Nv) {   // (block-uniform: the barriers below are reached by all)
    const int n = base + wv * Nv;
    float dX = 0.f, dY = 0.f, dZ = 0.f;
    if (n < N) {
      float gx = 0.f, gy = 0.f;
      if (on && grad_kp_pred) {
        gx = grad_kp_pred[((size_t)n * K + lane) * 2];
        gy = grad_kp_pred[((size_t)n * K + lane) * 2 + 1];
      }
      if (grad_loss && kp_gt) {
        float vis = 0.f, dx = 0.f, dy = 0.f;
        if (on) {
          const float* g = kp_gt + ((size_t)(n % Ng) * K + lane) * 3;
          const float* p = kp_pred + ((size_t)n * K + lane) * 2;
          dx = p[0] - g[0]; dy = p[1] - g[1];
          vis = g[2] > 0.f ? 1.f : 0.f;
        }
        const float nvis = wave_sum(vis);
        const float w = ((grad_loss[n] / (nvis / (float)K + 1e-4f)) / (float)K) * vis;
        gx += w * (dx > 0.f ? 1.f : dx < 0.f ? -1.f : 0.f);
        gy += w * (dy > 0.f ? 1.f : dy < 0.f ? -1.f : 0.f);
      }
      float acc[7];
      project_xy_adjoint(cams + 7 * (size_t)n, X, Y, Z, gx, gy, acc, dX, dY, dZ);
      if (grad_cams) {
#pragma unroll
        for (int i = 0; i < 7; ++i) acc[i] = wave_sum(on ? acc[i] : 0.f);
        if (lane < 7) {
          float val = acc[0];
#pragma unroll
          for (int i = 1; i < 7; ++i) val = lane == i ? acc[i] : val;
          grad_cams[7 * (size_t)n + lane] = val;
        }
      }
    }
    if (on) { s_part[wv][3 * lane] = dX; s_part[wv][3 * lane + 1] = dY; s_part[wv][3 * lane + 2] = dZ; }
    __syncthreads();
    if (wv == 0 && on)
      for (int w = 0; w < KH_WAVES && base + w * Nv < N; ++w) {
        ax += s_part[w][3 * lane]; ay += s_part[w][3 * lane + 1]; az += s_part[w][3 * lane + 2];
      }
    __syncthreads();
  }
  if (!have_g && grad_cams)
    for (int i = tid; r + (i / 7) * Nv < N; i += KH_TPB) grad_cams[7 * (size_t)(r + (i / 7) * Nv) + i % 7] = 0.f;
  if (wv == 0 && on) {
    if (grad_kp_verts) {
      const float* g = grad_kp_verts + ((size_t)r * K + lane) * 3;
      ax += g[0]; ay += g[1]; az += g[2];
    }
    s_dkpv[3 * lane] = ax; s_dkpv[3 * lane + 1] = ay; s_dkpv[3 * lane + 2] = az;
    float* o = dkpv + ((size_t)r * K + lane) * 3;
    o[0] = ax; o[1] = ay; o[2] = az;
  }
  if (!grad_verts) return;
  __syncthreads();
  for (int v = tid; v < V; v += KH_TPB) {
    float gx = 0.f, gy = 0.f, gz = 0.f;
#pragma unroll 4
    for (int k = 0; k < K; ++k) {
      const float w = A[(size_t)k * V + v];
      gx += w * s_dkpv[3 * k]; gy += w * s_dkpv[3 * k + 1]; gz += w * s_dkpv[3 * k + 2];
    }
    float* o = grad_verts + ((size_t)r * V + v) * 3;
    o[0] = gx; o[1] = gy; o[2] = gz;
  }
}

// Second launch: grad_A[k,v] = sum_r dkpv[r,k,:] . verts[r,v,:], r ascending; a thread per (k, v).
__global__ __launch_bounds__(KG_TPB) void k_kp_head_bwd_weights(const float* __restrict__ verts,
                                                                const float* __restrict__ dkpv, int K, int V, int Nv,
                                                                float* __restrict__ grad_A) {
  const int k = blockIdx.y, v = blockIdx.x * KG_TPB + threadIdx.x;
  if (v >= V) return;
  float s = 0.f;
#pragma unroll 4
  for (int r = 0; r < Nv; ++r) {
    const float* d = dkpv + ((size_t)r * K + k) * 3;
    const float* x = verts + ((size_t)r * V + v) * 3;
    s += d[0] * x[0] + d[1] * x[1] + d[2] * x[2];
  }
  grad_A[(size_t)k * V + v] = s;
}

// ---------------------------------------------------------------------------------------------- (d) camera loss
// The reference camera of frame n: cam_ref[n], or cams[g*(n) N + n] with g*(n) the first maximum of probs[:, n].
__device__ __forceinline__ const float* camera_ref_row(const float* __restrict__ cam_ref, const float* __restrict__ cams,
                                                       const long long* __restrict__ best, int N, int n) {
  return cam_ref ? cam_ref + 7 * (size_t)n : cams + 7 * ((size_t)best[n] * N + n);
}
// Re(q_pred (x) conj(q_ref)) in loss_utils.quat_loss_geodesic's order
__device__ __forceinline__ float quat_real(const float* __restrict__ p, const float* __restrict__ q) {
  const float b1 = -1.f * q[4], b2 = -1.f * q[5], b3 = -1.f * q[6];
  return p[3] * q[3] - p[4] * b1 - p[5] * b2 - p[6] * b3;
}

__global__ __launch_bounds__(CL_TPB) void k_camera_loss_fwd(const float* __restrict__ cam_pred,
                                                            const float* __restrict__ cam_ref,
                                                            const float* __restrict__ cams,
                                                            const float* __restrict__ probs, int N, int G, float margin,
                                                            float* __restrict__ loss, long long* __restrict__ best) {
  __shared__ float s_red[CL_WAVES][2];
  const int tid = threadIdx.x;
  float rot = 0.f, st = 0.f;
  for (int n = tid; n < N; n += CL_TPB) {
    int g_best = 0;
    if (!cam_ref) {
      float p_best = probs[n];
      for (int g = 1; g < G; ++g) {
        const float p = probs[(size_t)g * N + n];
        if (p > p_best) { p_best = p; g_best = g; }      // strict: the smallest g wins a tie
      }
      best[n] = g_best;
    }
    const float* p = cam_pred + 7 * (size_t)n;
    const float* q = cam_ref ? cam_ref + 7 * (size_t)n : cams + 7 * ((size_t)g_best * N + n);
    rot += fmaxf((1.f - fabsf(quat_real(p, q))) - margin, 0.f);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float d = p[i] - q[i];
      st += fmaxf(d * d - margin, 0.f);
    }
  }
  rot = wave_sum(rot); st = wave_sum(st);
  if ((tid & 63) == 0) { s_red[tid >> 6][0] = rot; s_red[tid >> 6][1] = st; }
  __syncthreads();
  if (tid == 0) {
    float r = 0.f, s = 0.f;
    for (int w = 0; w < CL_WAVES; ++w) { r += s_red[w][0]; s += s_red[w][1]; }
    loss[0] = r / (float)N + s / (float)(3 * (size_t)N);
  }
}

// d max(x, 0): 1 above the hinge, 1/2 on it (torch.max(a, zeros) splits a tie), 0 below; d|x| at 0 is 0.
__device__ __forceinline__ float hinge_slope(float x) { return x > 0.f ? 1.f : x == 0.f ? 0.5f : 0.f; }

__global__ __launch_bounds__(CL_TPB) void k_camera_loss_bwd(const float* __restrict__ cam_pred,
                                                            const float* __restrict__ cam_ref,
                                                            const float* __restrict__ cams,
                                                            const long long* __restrict__ best,
                                                            const float* __restrict__ grad_loss, int N, float margin,
                                                            float* __restrict__ grad_pred) {
  const float go = grad_loss[0];
  const float g_rot = go / (float)N, g_st = go / (float)(3 * (size_t)N);
  for (int n = threadIdx.x; n < N; n += CL_TPB) {
    const float* p = cam_pred + 7 * (size_t)n;
    const float* q = camera_ref_row(cam_ref, cams, best, N, n);
    float* o = grad_pred + 7 * (size_t)n;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float d = p[i] - q[i];
      o[i] = (g_st * hinge_slope(d * d - margin)) * (2.f * d);
    }
    const float re = quat_real(p, q);
    const float sgn = re > 0.f ? 1.f : re < 0.f ? -1.f : 0.f;
    const float w = -(g_rot * hinge_slope((1.f - fabsf(re)) - margin)) * sgn;   // d loss / d real
#pragma unroll
    for (int i = 3; i < 7; ++i) o[i] = w * q[i];         // d real / d q_pred = q_ref
  }
}

static bool kp_shape_ok(int K, int V) { return K >= 1 && K <= KP_MAX_K && V >= 1 && V <= 65535; }
static bool kp_batch_ok(int N, int Nv, int Ng, bool have_gt) {
  if (N < 0 || N > 65535) return false;
  if (N == 0) return true;
  if (Nv < 1 || N % Nv) return false;
  return !have_gt || (Ng >= 1 && N % Ng == 0);
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_kp_weights_forward(const float* logits, int K, int V, float* A, float* entropy, float* stats, void* stream) {
  if (!logits || !A || !entropy || !stats || !kp_shape_ok(K, V)) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_kp_weights_fwd, dim3(1), dim3(KW_TPB), 0, (hipStream_t)stream, logits, K, V, A, entropy, stats);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_kp_weights_backward(const float* logits, const float* A, const float* stats, const float* grad_A,
                             const float* grad_entropy, int K, int V, float* grad_logits, void* stream) {
  if (!logits || !A || !stats || !grad_logits || !kp_shape_ok(K, V)) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_kp_weights_bwd, dim3(1), dim3(KW_TPB), 0, (hipStream_t)stream, logits, A, stats, grad_A,
                     grad_entropy, K, V, grad_logits);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_kp_head_forward(const float* A, const float* verts, const float* cams, const float* kp_gt, int K, int V, int N,
                         int Nv, int Ng, float img_size, float* kp_verts, float* kp_pred, float* loss, float* kp_err,
                         void* stream) {
  if (!kp_shape_ok(K, V) || !kp_batch_ok(N, Nv, Ng, kp_gt != nullptr)) return ACFM_E_BADARG;
  if (N == 0) return ACFM_OK;
  if (!A || !verts || !cams || !kp_verts || !kp_pred) return ACFM_E_BADARG;
  if (kp_gt ? !loss : (loss || kp_err)) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_kp_head_fwd, dim3(Nv), dim3(KH_TPB), 0, (hipStream_t)stream, A, verts, cams, kp_gt, K, V, N, Nv,
                     kp_gt ? Ng : 1, img_size / 2.f, kp_verts, kp_pred, loss, kp_err);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

size_t acfm_kp_head_workspace_bytes(int K, int Nv) {
  if (K < 1 || K > KP_MAX_K || Nv < 1 || Nv > 65535) return 0;
  return align256(sizeof(float) * 3 * (size_t)K * Nv);
}

int acfm_kp_head_backward(const float* A, const float* verts, const float* cams, const float* kp_gt,
                          const float* kp_verts, const float* kp_pred, const float* grad_loss, const float* grad_kp_pred,
                          const float* grad_kp_verts, int K, int V, int N, int Nv, int Ng, float* grad_A,
                          float* grad_verts, float* grad_cams, void* ws, size_t ws_bytes, void* stream) {
  if (!kp_shape_ok(K, V) || !kp_batch_ok(N, Nv, Ng, kp_gt != nullptr)) return ACFM_E_BADARG;
  if (N == 0) return ACFM_OK;
  if (!A || !verts || !cams || !kp_verts || !kp_pred || !ws) return ACFM_E_BADARG;
  if (grad_loss && !kp_gt) return ACFM_E_BADARG;
  if (ws_bytes < acfm_kp_head_workspace_bytes(K, Nv)) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_kp_head_bwd, dim3(Nv), dim3(KH_TPB), 0, st, A, cams, kp_gt, kp_verts, kp_pred, grad_loss,
                     grad_kp_pred, grad_kp_verts, K, V, N, Nv, kp_gt ? Ng : 1, (float*)ws, grad_verts, grad_cams);
  if (grad_A)
    hipLaunchKernelGGL(k_kp_head_bwd_weights, dim3((V + KG_TPB - 1) / KG_TPB, K), dim3(KG_TPB), 0, st, verts,
                       (const float*)ws, K, V, Nv, grad_A);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_camera_loss_forward(const float* cam_pred, const float* cam_ref, const float* cams, const float* probs, int N,
                             int G, float margin, float* loss, int64_t* best, void* stream) {
  if (N < 0 || N > 65535) return ACFM_E_BADARG;
  if (N == 0) return ACFM_OK;
  if (!cam_pred || !loss) return ACFM_E_BADARG;
  if (cam_ref ? (cams || probs) : (!cams || !probs || !best || G < 1 || G > 65535)) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_loss_fwd, dim3(1), dim3(CL_TPB), 0, (hipStream_t)stream, cam_pred, cam_ref, cams, probs, N,
                     G, margin, loss, (long long*)best);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_camera_loss_backward(const float* cam_pred, const float* cam_ref, const float* cams, const int64_t* best,
                              const float* grad_loss, int N, float margin, float* grad_cam_pred, void* stream) {
  if (N < 0 || N > 65535) return ACFM_E_BADARG;
  if (N == 0) return ACFM_OK;
  if (!cam_pred || !grad_loss || !grad_cam_pred) return ACFM_E_BADARG;
  if (cam_ref ? (cams != nullptr) : (!cams || !best)) return ACFM_E_BADARG;
  hipLaunchKernelGGL(k_camera_loss_bwd, dim3(1), dim3(CL_TPB), 0, (hipStream_t)stream, cam_pred, cam_ref, cams,
                     (const long long*)best, grad_loss, N, margin, grad_cam_pred);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
