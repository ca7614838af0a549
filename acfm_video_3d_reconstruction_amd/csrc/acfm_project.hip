// Weak-perspective projection and its backward: k_project, k_project_bwd, the four acfm_project* entry points and
// the launcher of the projection backward that ends the silhouette backward.  Replaces the reference's
// geom_utils.orthographic_proj_withz / orthographic_proj / quat_rotate and their autograd backward.
#include "acfm_raster.h"

namespace acfm {

// ------------------------------------------------------------------------------- projection
template <bool XY>   // XY: only (x, y) are stored, [N,V,2] (orthographic_proj / project_points)
__global__ __launch_bounds__(TPB) void k_project(const float* __restrict__ verts,
                                                 const float* __restrict__ cams, int V, float offset_z,
                                                 float* __restrict__ proj) {
  const int n = blockIdx.y;
  const int v = blockIdx.x * TPB + threadIdx.x;
  if (v >= V) return;
  const float* x = verts + ((size_t)n * V + v) * 3;
  float px, py, pz;
  project_point(cams + 7 * (size_t)n, x[0], x[1], x[2], offset_z, px, py, pz);
  if (XY) {
    float* o = proj + ((size_t)n * V + v) * 2;
    o[0] = px; o[1] = py;
  } else {
    float* o = proj + ((size_t)n * V + v) * 3;
    o[0] = px; o[1] = py; o[2] = pz;
  }
}

// Backward of proj = s * rot(q, X) + (tx, ty, offset_z), q not normalised here:
//   r      = (q0^2 - u.u) X + 2 (u.X) u + 2 q0 (u x X)
//   dL/ds  = g.r ; dL/dt = g.xy ; with G = s g:
//   dL/dq0 = 2 q0 (G.X) + 2 G.(u x X)
//   dL/du  = -2 (G.X) u + 2 (G.u) X + 2 (u.X) G + 2 q0 (X x G)
//   dL/dX  = (q0^2 - u.u) G + 2 (G.u) u + 2 q0 (G x u)
// MODE 1 (NDC2): the upstream gradient is grad_ndc [N,V,2] of the rasteriser
// (x_ndc = -x_p, y_ndc = -y_p, no z gradient on the silhouette path); MODE 2: the gradient of the
// (x, y) projection [N,V,2] as it is; MODE 0: all three components [N,V,3].
template <int MODE>
__global__ __launch_bounds__(TPB) void k_project_bwd(const float* __restrict__ verts,
                                                     const float* __restrict__ cams,
                                                     float* gin /* NDC2: cleared after reading */, int V,
                                                     float* __restrict__ grad_verts,
                                                     float* __restrict__ grad_cams,
                                                     const float* __restrict__ gproj = nullptr /* NDC modes: + [N,V,2] */) {
  __shared__ float s_red[4][7];
  const int n = blockIdx.x, tid = threadIdx.x;
  const float* c = cams + 7 * (size_t)n;
  const float s = c[0], q0 = c[3], ux = c[4], uy = c[5], uz = c[6];
  const float uu = ux * ux + uy * uy + uz * uz;
  const float a = q0 * q0 - uu;
  float acc[7] = {0, 0, 0, 0, 0, 0, 0};
  for (int v = tid; v < V; v += TPB) {
    const float* x = verts + ((size_t)n * V + v) * 3;
    const float X = x[0], Y = x[1], Z = x[2];
    float gx, gy, gz;
    if (MODE == 3) {            // NDC2 in 2^-36 fixed point (deterministic backward)
      long long* g = reinterpret_cast<long long*>(gin) + ((size_t)n * V + v) * 2;
      gx = -((float)g[0] * FIX_INV); gy = -((float)g[1] * FIX_INV); gz = 0.f;
      g[0] = 0; g[1] = 0;
      if (gproj) { gx += gproj[((size_t)n * V + v) * 2]; gy += gproj[((size_t)n * V + v) * 2 + 1]; }
    } else if (MODE == 1) {
      float* g = gin + ((size_t)n * V + v) * 2;
      gx = -g[0]; gy = -g[1]; gz = 0.f;
      g[0] = 0.f; g[1] = 0.f;   // the raster workspace's NDC-gradient scratch is left zeroed for the next backward
      // the gradient of the projection the forward handed out (AcfmSilExtras.proj_xy: a second consumer of the same
      // vertices and cameras, e.g. the boundary loss): one projection backward for both, no gradient sum afterwards
      if (gproj) { gx += gproj[((size_t)n * V + v) * 2]; gy += gproj[((size_t)n * V + v) * 2 + 1]; }
    } else if (MODE == 2) {
      const float* g = gin + ((size_t)n * V + v) * 2;
      gx = g[0]; gy = g[1]; gz = 0.f;
    } else {
      const float* g = gin + ((size_t)n * V + v) * 3;
      gx = g[0]; gy = g[1]; gz = g[2];
    }
    const float uX = ux * X + uy * Y + uz * Z;
    const float cx = uy * Z - uz * Y, cy = uz * X - ux * Z, cz = ux * Y - uy * X;  // u x X
    const float rx = a * X + 2.f * uX * ux + 2.f * q0 * cx;
    const float ry = a * Y + 2.f * uX * uy + 2.f * q0 * cy;
    const float rz = a * Z + 2.f * uX * uz + 2.f * q0 * cz;
    acc[0] += gx * rx + gy * ry + gz * rz;
    acc[1] += gx;
    acc[2] += gy;
    const float Gx = s * gx, Gy = s * gy, Gz = s * gz;
    const float GX = Gx * X + Gy * Y + Gz * Z;
    const float Gu = Gx * ux + Gy * uy + Gz * uz;
    acc[3] += 2.f * q0 * GX + 2.f * (Gx * cx + Gy * cy + Gz * cz);
    const float xg_x = Y * Gz - Z * Gy, xg_y = Z * Gx - X * Gz, xg_z = X * Gy - Y * Gx;  // X x G
    acc[4] += -2.f * GX * ux + 2.f * Gu * X + 2.f * uX * Gx + 2.f * q0 * xg_x;
    acc[5] += -2.f * GX * uy + 2.f * Gu * Y + 2.f * uX * Gy + 2.f * q0 * xg_y;
    acc[6] += -2.f * GX * uz + 2.f * Gu * Z + 2.f * uX * Gz + 2.f * q0 * xg_z;
    if (grad_verts) {
      const float gu_x = Gy * uz - Gz * uy, gu_y = Gz * ux - Gx * uz, gu_z = Gx * uy - Gy * ux;  // G x u
      float* o = grad_verts + ((size_t)n * V + v) * 3;
      o[0] = a * Gx + 2.f * Gu * ux + 2.f * q0 * gu_x;
      o[1] = a * Gy + 2.f * Gu * uy + 2.f * q0 * gu_y;
      o[2] = a * Gz + 2.f * Gu * uz + 2.f * q0 * gu_z;
    }
  }
  if (!grad_cams) return;
#pragma unroll
  for (int i = 0; i < 7; ++i) acc[i] = wave_sum(acc[i]);
  const int w = tid >> 6;
  if ((tid & 63) == 0)
    for (int i = 0; i < 7; ++i) s_red[w][i] = acc[i];
  __syncthreads();
  if (tid < 7) grad_cams[7 * (size_t)n + tid] = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
}

void launch_project_bwd_ndc(bool deterministic, const float* verts, const float* cams, const RasterWs& ws, int N,
                            int V, float* grad_verts, float* grad_cams, const float* gproj, hipStream_t st) {
  if (deterministic)
    hipLaunchKernelGGL((k_project_bwd<3>), dim3(N), dim3(TPB), 0, st, verts, cams,
                       reinterpret_cast<float*>(ws.grad_fix), V, grad_verts, grad_cams, gproj);
  else
    hipLaunchKernelGGL((k_project_bwd<1>), dim3(N), dim3(TPB), 0, st, verts, cams,
                       ws.grad_ndc, V, grad_verts, grad_cams, gproj);
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_project(const float* verts, const float* cams, int N, int V, float offset_z, float* proj,
                 void* stream) {
  if (!verts || !cams || !proj || N <= 0 || N > 65535 || V <= 0) return ACFM_E_BADARG;
  ProfScope ps(ACFM_PROF_PROJECT, (hipStream_t)stream);
  hipLaunchKernelGGL((k_project<false>), dim3((V + TPB - 1) / TPB, N), dim3(TPB), 0, (hipStream_t)stream, verts,
                     cams, V, offset_z, proj);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_project_backward(const float* verts, const float* cams, const float* grad_proj, int N, int V,
                          float* grad_verts, float* grad_cams, void* stream) {
  if (!verts || !cams || !grad_proj || N <= 0 || V <= 0) return ACFM_E_BADARG;
  ProfScope ps(ACFM_PROF_PROJ_BWD, (hipStream_t)stream);
  hipLaunchKernelGGL((k_project_bwd<0>), dim3(N), dim3(TPB), 0, (hipStream_t)stream, verts, cams,
                     const_cast<float*>(grad_proj), V, grad_verts, grad_cams);  // (read-only in this instantiation)
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_project_xy(const float* verts, const float* cams, int N, int V, float offset_z, float* proj_xy,
                    void* stream) {
  if (!verts || !cams || !proj_xy || N <= 0 || N > 65535 || V <= 0) return ACFM_E_BADARG;
  ProfScope ps(ACFM_PROF_PROJECT, (hipStream_t)stream);
  hipLaunchKernelGGL((k_project<true>), dim3((V + TPB - 1) / TPB, N), dim3(TPB), 0, (hipStream_t)stream, verts,
                     cams, V, offset_z, proj_xy);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_project_xy_backward(const float* verts, const float* cams, const float* grad_proj_xy, int N, int V,
                             float* grad_verts, float* grad_cams, void* stream) {
  if (!verts || !cams || !grad_proj_xy || N <= 0 || V <= 0) return ACFM_E_BADARG;
  ProfScope ps(ACFM_PROF_PROJ_BWD, (hipStream_t)stream);
  hipLaunchKernelGGL((k_project_bwd<2>), dim3(N), dim3(TPB), 0, (hipStream_t)stream, verts, cams,
                     const_cast<float*>(grad_proj_xy), V, grad_verts, grad_cams);  // (read-only in this instantiation)
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
