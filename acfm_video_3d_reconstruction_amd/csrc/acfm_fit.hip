// The template fit (utils/geometry.py:75-140, fit_verts_to_mesh) as gfx950 kernels:
//   acfm_chamfer{,_backward}               <- pytorch3d.loss.chamfer_distance      (nearest neighbour both ways)
//   acfm_edge_length_loss{,_backward}      <- pytorch3d.loss.mesh_edge_loss
//   acfm_normal_consistency{,_backward}    <- pytorch3d.loss.mesh_normal_consistency
// The forward sums leave through the ticket finish of acfm_row_finish.h: one launch, no zero fill, no float atomics,
// the same bits on every run.  The backward kernels add with float atomics (LDS or global): their sums can differ
// in the last bits from run to run.
#include "acfm_common.h"
#include "acfm_points.h"
#include "acfm_row_finish.h"

namespace acfm {

// ---- chamfer forward ----------------------------------------------------------------------------------------------
// One launch for both directions: workgroups [0, nb1) of a cloud pair search y for 64 points of x each, workgroups
// [nb1, nb1 + nb2) search x for 64 points of y.  As in k_bds_loss the four waves search a quarter of the candidates
// each and wave 0 merges the four minima in wave (= index) order, so the lowest index wins among equal distances
// exactly as in one ascending scan.  Unlike there the candidates do not have to fit in LDS: every wave streams its own
// quarter through a private tile of CH_TILE points (16 KB of static LDS for the workgroup whatever the cloud sizes);
// a wave reads no other wave's tile, so no workgroup barrier stands inside the scan.
// Rows at or past a cloud's length are never loaded, neither as queries nor as candidates (they may hold NaN).
constexpr int CH_TPB = 256;
constexpr int CH_TILE = 256;   // candidates per wave and round: four per lane
constexpr int CH_Q = 64;       // query points per workgroup
// (clamped_len, wave_lds_sync and CH_BWD_LDS_MAX_P: acfm_points.h, shared with acfm_knn.hip)

__global__ __launch_bounds__(CH_TPB) void k_chamfer(const float* __restrict__ x, const float* __restrict__ y,
                                                    const int64_t* __restrict__ x_len, const int64_t* __restrict__ y_len,
                                                    int N, int P1, int P2, int nb1, int nb2, float* __restrict__ sums,
                                                    int32_t* __restrict__ idx_x, int32_t* __restrict__ idx_y,
                                                    RowScratch sc) {
  __shared__ float4 s_c[4][CH_TILE];
  __shared__ float s_best[4][64];
  __shared__ int s_bi[4][64];
  const int n = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int side = (int)blockIdx.x >= nb1 ? 1 : 0;
  const int blk = side ? (int)blockIdx.x - nb1 : (int)blockIdx.x;
  const int PQ = side ? P2 : P1, PC = side ? P1 : P2;
  const int lq = clamped_len(side ? y_len : x_len, n, PQ), lc = clamped_len(side ? x_len : y_len, n, PC);
  const float* __restrict__ q = (side ? y : x) + (size_t)n * PQ * 3;
  const float* __restrict__ c = (side ? x : y) + (size_t)n * PC * 3;
  const long long p = (long long)blk * CH_Q + lane;
  const bool live = p < lq;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (live) { qx = q[3 * p]; qy = q[3 * p + 1]; qz = q[3 * p + 2]; }
  float best = __builtin_inff();
  int bi = -1;
  if ((long long)blk * CH_Q < lq) {   // (the same for the whole workgroup)
    const long long chunk = ((long long)lc + 3) / 4;
    const long long v0 = min(wv * chunk, (long long)lc), v1 = min((long long)lc, v0 + chunk);
    for (long long base = v0; base < v1; base += CH_TILE) {
      float cx[4], cy[4], cz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {     // the four loads of a lane are in flight together
        const long long v = min(base + u * 64 + lane, v1 - 1);
        cx[u] = c[3 * v]; cy[u] = c[3 * v + 1]; cz[u] = c[3 * v + 2];
      }
      wave_lds_sync();                  // the scan of the round before has read the tile
#pragma unroll
      for (int u = 0; u < 4; ++u) s_c[wv][u * 64 + lane] = make_float4(cx[u], cy[u], cz[u], 0.f);
      wave_lds_sync();
      const int cnt = (int)min((long long)CH_TILE, v1 - base);
      const int b0 = (int)base;
#pragma unroll 8
      for (int k = 0; k < cnt; ++k) {
        const float4 t = s_c[wv][k];
        const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (d < best) { best = d; bi = b0 + k; }
      }
    }
  }
  s_best[wv][lane] = best; s_bi[wv][lane] = bi;
  __syncthreads();
  if (wv != 0) return;
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float d = s_best[w][lane];
    if (d < best) { best = d; bi = s_bi[w][lane]; }
  }
  float contrib = 0.f;
  if (live) {
    (side ? idx_y : idx_x)[(size_t)n * PQ + p] = bi;
    if (bi >= 0) contrib = best;       // no candidate (the other cloud has length 0): the sum is 0
  }
  contrib = wave_sum(contrib);
  // the two directions of a pair are two rows of the ticket finish: tickets [2][N], partials [N][nb1] then [N][nb2]
  RowScratch mine;
  mine.tickets = sc.tickets + (side ? N : 0);
  mine.partials = sc.partials + (side ? (size_t)N * nb1 : 0);
  row_finish<1>(mine, n, side ? nb2 : nb1, blk, contrib, sums + 2 * (size_t)n + side);
}

// ---- chamfer backward ---------------------------------------------------------------------------------------------
// d loss / d p for a point p of either cloud = 2 g_own (p - nn(p))  +  sum over the other cloud's points r that chose
// p of 2 g_other (p - r).  As k_bds_loss_bwd: one workgroup per (pair, side) keeps the side's [P,3] gradient in LDS,
// writes every row's own term (zero for rows at or past the length), adds what the other cloud sends back with LDS
// atomics and stores whole rows -- no global atomics, no zero fill.  12 B of LDS per point, at most 150 KB:
// CH_BWD_LDS_MAX_P points on the larger side.  Past that k_chamfer_bwd_own / k_chamfer_bwd_scatter do the same with
// global atomics.  The order of the float additions varies: gradients are not bit-reproducible.
constexpr int CHB_TPB = 512;

struct ChSide {
  const float* own; const float* other;
  const int32_t* idx_own; const int32_t* idx_other;
  float* grad;
  int PO, PT, lo, lt;
  float g_own, g_other;   // 2 x the upstream gradients
};
__device__ __forceinline__ ChSide ch_side(int side, int n, const float* x, const float* y, const int64_t* x_len,
                                          const int64_t* y_len, const int32_t* idx_x, const int32_t* idx_y,
                                          const float* gs, int P1, int P2, float* gx, float* gy) {
  ChSide s;
  s.PO = side ? P2 : P1; s.PT = side ? P1 : P2;
  s.own = (side ? y : x) + (size_t)n * s.PO * 3;
  s.other = (side ? x : y) + (size_t)n * s.PT * 3;
  s.idx_own = (side ? idx_y : idx_x) + (size_t)n * s.PO;
  s.idx_other = (side ? idx_x : idx_y) + (size_t)n * s.PT;
  s.grad = (side ? gy : gx) + (size_t)n * s.PO * 3;
  s.lo = clamped_len(side ? y_len : x_len, n, s.PO);
  s.lt = clamped_len(side ? x_len : y_len, n, s.PT);
  s.g_own = 2.0f * gs[2 * (size_t)n + side];
  s.g_other = 2.0f * gs[2 * (size_t)n + 1 - side];
  return s;
}

__global__ __launch_bounds__(CHB_TPB) void k_chamfer_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                         const int64_t* __restrict__ x_len,
                                                         const int64_t* __restrict__ y_len,
                                                         const int32_t* __restrict__ idx_x,
                                                         const int32_t* __restrict__ idx_y,
                                                         const float* __restrict__ gs, int P1, int P2,
                                                         float* __restrict__ gx, float* __restrict__ gy) {
  extern __shared__ float s_g[];   // [PO][3]
  const int tid = threadIdx.x;
  const ChSide s = ch_side((int)blockIdx.x, (int)blockIdx.y, x, y, x_len, y_len, idx_x, idx_y, gs, P1, P2, gx, gy);
  for (int i = tid; i < s.PO; i += CHB_TPB) {
    float a = 0.f, b = 0.f, c = 0.f;
    if (i < s.lo) {
      const int k = s.idx_own[i];
      if (k >= 0 && k < s.lt) {
        a = s.g_own * (s.own[3 * i] - s.other[3 * (size_t)k]);
        b = s.g_own * (s.own[3 * i + 1] - s.other[3 * (size_t)k + 1]);
        c = s.g_own * (s.own[3 * i + 2] - s.other[3 * (size_t)k + 2]);
      }
    }
    s_g[3 * i] = a; s_g[3 * i + 1] = b; s_g[3 * i + 2] = c;
  }
  __syncthreads();
  for (int j = tid; j < s.lt; j += CHB_TPB) {
    const int k = s.idx_other[j];
    if (k < 0 || k >= s.lo) continue;
    atomicAdd(&s_g[3 * k], s.g_other * (s.own[3 * (size_t)k] - s.other[3 * (size_t)j]));
    atomicAdd(&s_g[3 * k + 1], s.g_other * (s.own[3 * (size_t)k + 1] - s.other[3 * (size_t)j + 1]));
    atomicAdd(&s_g[3 * k + 2], s.g_other * (s.own[3 * (size_t)k + 2] - s.other[3 * (size_t)j + 2]));
  }
  __syncthreads();
  for (int i = tid; i < 3 * s.PO; i += CHB_TPB) s.grad[i] = s_g[i];
}

// the same in two launches for clouds past the LDS bound: every row's own term (zeros included), then the scatter
__global__ __launch_bounds__(256) void k_chamfer_bwd_own(const float* __restrict__ x, const float* __restrict__ y,
                                                         const int64_t* __restrict__ x_len,
                                                         const int64_t* __restrict__ y_len,
                                                         const int32_t* __restrict__ idx_x,
                                                         const int32_t* __restrict__ idx_y,
                                                         const float* __restrict__ gs, int P1, int P2,
                                                         float* __restrict__ gx, float* __restrict__ gy) {
  const ChSide s = ch_side((int)blockIdx.y, (int)blockIdx.z, x, y, x_len, y_len, idx_x, idx_y, gs, P1, P2, gx, gy);
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= s.PO) return;
  float a = 0.f, b = 0.f, c = 0.f;
  if (i < s.lo) {
    const int k = s.idx_own[i];
    if (k >= 0 && k < s.lt) {
      a = s.g_own * (s.own[3 * i] - s.other[3 * (size_t)k]);
      b = s.g_own * (s.own[3 * i + 1] - s.other[3 * (size_t)k + 1]);
      c = s.g_own * (s.own[3 * i + 2] - s.other[3 * (size_t)k + 2]);
    }
  }
  s.grad[3 * i] = a; s.grad[3 * i + 1] = b; s.grad[3 * i + 2] = c;
}
__global__ __launch_bounds__(256) void k_chamfer_bwd_scatter(const float* __restrict__ x, const float* __restrict__ y,
                                                             const int64_t* __restrict__ x_len,
                                                             const int64_t* __restrict__ y_len,
                                                             const int32_t* __restrict__ idx_x,
                                                             const int32_t* __restrict__ idx_y,
                                                             const float* __restrict__ gs, int P1, int P2,
                                                             float* __restrict__ gx, float* __restrict__ gy) {
  const ChSide s = ch_side((int)blockIdx.y, (int)blockIdx.z, x, y, x_len, y_len, idx_x, idx_y, gs, P1, P2, gx, gy);
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= s.lt) return;
  const int k = s.idx_other[j];
  if (k < 0 || k >= s.lo) return;
  atomicAdd(&s.grad[3 * (size_t)k], s.g_other * (s.own[3 * (size_t)k] - s.other[3 * j]));
  atomicAdd(&s.grad[3 * (size_t)k + 1], s.g_other * (s.own[3 * (size_t)k + 1] - s.other[3 * j + 1]));
  atomicAdd(&s.grad[3 * (size_t)k + 2], s.g_other * (s.own[3 * (size_t)k + 2] - s.other[3 * j + 2]));
}

// ---- edge length and normal consistency ---------------------------------------------------------------------------
// One thread per edge / per pair of faces on an edge; the workgroups' sums meet in the ticket finish (one row).
// The backward adds into a zeroed [P,3] with global float atomics, as k_rigid_bwd.
constexpr int FTPB = 256;

__device__ __forceinline__ void block_finish(float c, const RowScratch& sc, float* __restrict__ loss) {
  __shared__ float s_red[FTPB / 64];
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x >= 64) return;
  const float v = (s_red[0] + s_red[1]) + (s_red[2] + s_red[3]);
  row_finish<1>(sc, 0, (int)gridDim.x, (int)blockIdx.x, v, loss);
}

// loss = sum_e w_e (|v_a - v_b| - target)^2
__global__ __launch_bounds__(FTPB) void k_edge_len(const float* __restrict__ v, const int64_t* __restrict__ e,
                                                   const float* __restrict__ w, int P, int E, float target,
                                                   float* __restrict__ loss, RowScratch sc) {
  const int i = blockIdx.x * FTPB + threadIdx.x;
  float c = 0.f;
  if (i < E) {
    const long a = e[2 * (size_t)i], b = e[2 * (size_t)i + 1];
    if (a >= 0 && b >= 0 && a < P && b < P) {
      const float dx = v[3 * a] - v[3 * b], dy = v[3 * a + 1] - v[3 * b + 1], dz = v[3 * a + 2] - v[3 * b + 2];
      const float d = sqrtf(dx * dx + dy * dy + dz * dz) - target;
      c = w[i] * (d * d);
    }
  }
  block_finish(c, sc, loss);
}
__global__ __launch_bounds__(FTPB) void k_edge_len_bwd(const float* __restrict__ v, const int64_t* __restrict__ e,
                                                       const float* __restrict__ w, const float* __restrict__ gop,
                                                       int P, int E, float target, float* __restrict__ gv) {
  const int i = blockIdx.x * FTPB + threadIdx.x;
  if (i >= E) return;
  const long a = e[2 * (size_t)i], b = e[2 * (size_t)i + 1];
  if (a < 0 || b < 0 || a >= P || b >= P) return;
  const float dx = v[3 * a] - v[3 * b], dy = v[3 * a + 1] - v[3 * b + 1], dz = v[3 * a + 2] - v[3 * b + 2];
  const float l = sqrtf(dx * dx + dy * dy + dz * dz);
  const float s = l > 0.f ? gop[0] * w[i] * 2.0f * (l - target) / l : 0.f;   // subgradient 0 at a zero-length edge
  atomicAdd(&gv[3 * a], s * dx); atomicAdd(&gv[3 * a + 1], s * dy); atomicAdd(&gv[3 * a + 2], s * dz);
  atomicAdd(&gv[3 * b], -s * dx); atomicAdd(&gv[3 * b + 1], -s * dy); atomicAdd(&gv[3 * b + 2], -s * dz);
}

struct V3 { float x, y, z; };
__device__ __forceinline__ V3 ld3(const float* __restrict__ v, long i) { return V3{v[3 * i], v[3 * i + 1], v[3 * i + 2]}; }
__device__ __forceinline__ V3 sub3(V3 a, V3 b) { return V3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
  return V3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ float dot3(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ bool quad_ids(const int64_t* __restrict__ q, int i, int P, long id[4]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) { id[k] = q[4 * (size_t)i + k]; ok = ok && id[k] >= 0 && id[k] < P; }
  return ok;
}

// pair (a, b, c, d): the faces (a, b, c) and (a, b, d) on the edge a-b.  n0 = (c - a) x (b - a), n1 = (b - a) x (d - a)
// (= -((d - a) x (b - a))), term = w (1 - n0.n1 / max(|n0| |n1|, 1e-8)).
__global__ __launch_bounds__(FTPB) void k_normal_cons(const float* __restrict__ v, const int64_t* __restrict__ q,
                                                      const float* __restrict__ w, int P, int Q,
                                                      float* __restrict__ loss, RowScratch sc) {
  const int i = blockIdx.x * FTPB + threadIdx.x;
  float c = 0.f;
  long id[4];
  if (i < Q && quad_ids(q, i, P, id)) {
    const V3 a = ld3(v, id[0]);
    const V3 eb = sub3(ld3(v, id[1]), a), ec = sub3(ld3(v, id[2]), a), ed = sub3(ld3(v, id[3]), a);
    const V3 n0 = cross3(ec, eb), n1 = cross3(eb, ed);
    const float den = fmaxf(sqrtf(dot3(n0, n0)) * sqrtf(dot3(n1, n1)), 1e-8f);
    c = w[i] * (1.0f - dot3(n0, n1) / den);
  }
  block_finish(c, sc, loss);
}
__global__ __launch_bounds__(FTPB) void k_normal_cons_bwd(const float* __restrict__ v, const int64_t* __restrict__ q,
                                                          const float* __restrict__ w, const float* __restrict__ gop,
                                                          int P, int Q, float* __restrict__ gv) {
  const int i = blockIdx.x * FTPB + threadIdx.x;
  long id[4];
  if (i >= Q || !quad_ids(q, i, P, id)) return;
  const V3 a = ld3(v, id[0]);
  const V3 eb = sub3(ld3(v, id[1]), a), ec = sub3(ld3(v, id[2]), a), ed = sub3(ld3(v, id[3]), a);
  const V3 n0 = cross3(ec, eb), n1 = cross3(eb, ed);
  const float l0 = sqrtf(dot3(n0, n0)), l1 = sqrtf(dot3(n1, n1)), p = l0 * l1, dt = dot3(n0, n1);
  const float den = fmaxf(p, 1e-8f);
  const float gc = -gop[0] * w[i];               // d term / d cos
  // cos = dt / den;  den = p where p > 1e-8 (then d den / d n0 = l1 n0 / l0), a constant below
  const float k0 = (p > 1e-8f && l0 > 0.f) ? dt / (den * (l0 * l0)) : 0.f;
  const float k1 = (p > 1e-8f && l1 > 0.f) ? dt / (den * (l1 * l1)) : 0.f;
  const V3 g0 = V3{gc * (n1.x / den - k0 * n0.x), gc * (n1.y / den - k0 * n0.y), gc * (n1.z / den - k0 * n0.z)};
  const V3 g1 = V3{gc * (n0.x / den - k1 * n1.x), gc * (n0.y / den - k1 * n1.y), gc * (n0.z / den - k1 * n1.z)};
  // n0 = ec x eb: d/d ec = eb x g0, d/d eb = g0 x ec;  n1 = eb x ed: d/d eb = ed x g1, d/d ed = g1 x eb
  const V3 gcv = cross3(eb, g0), gd = cross3(g1, eb);
  const V3 t0 = cross3(g0, ec), t1 = cross3(ed, g1);
  const V3 gb = V3{t0.x + t1.x, t0.y + t1.y, t0.z + t1.z};
  atomicAdd(&gv[3 * id[1]], gb.x); atomicAdd(&gv[3 * id[1] + 1], gb.y); atomicAdd(&gv[3 * id[1] + 2], gb.z);
  atomicAdd(&gv[3 * id[2]], gcv.x); atomicAdd(&gv[3 * id[2] + 1], gcv.y); atomicAdd(&gv[3 * id[2] + 2], gcv.z);
  atomicAdd(&gv[3 * id[3]], gd.x); atomicAdd(&gv[3 * id[3] + 1], gd.y); atomicAdd(&gv[3 * id[3] + 2], gd.z);
  atomicAdd(&gv[3 * id[0]], -((gb.x + gcv.x) + gd.x)); atomicAdd(&gv[3 * id[0] + 1], -((gb.y + gcv.y) + gd.y));
  atomicAdd(&gv[3 * id[0] + 2], -((gb.z + gcv.z) + gd.z));
}

static inline int ch_blocks(int P) { return (int)(((long long)P + CH_Q - 1) / CH_Q); }
static inline int term_blocks(int n) { return (int)(((long long)n + FTPB - 1) / FTPB); }
static inline int term_scratch(int count, uint32_t* tickets, float* partials, size_t partial_floats, RowScratch& sc) {
  if (!tickets || !partials) return ACFM_E_BADARG;
  if (partial_floats < (size_t)term_blocks(count)) return ACFM_E_WORKSPACE;
  sc.tickets = tickets; sc.partials = partials;
  return ACFM_OK;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

size_t acfm_chamfer_partial_floats(int N, int P1, int P2) {
  if (N <= 0 || P1 <= 0 || P2 <= 0) return 0;
  return (size_t)N * ((size_t)ch_blocks(P1) + (size_t)ch_blocks(P2));
}

int acfm_chamfer(const float* x, const float* y, const int64_t* x_len, const int64_t* y_len, int N, int P1, int P2,
                 float* sums, int32_t* idx_x, int32_t* idx_y, uint32_t* tickets, float* partials,
                 size_t partial_floats, void* stream) {
  if (!x || !y || !sums || !idx_x || !idx_y || !tickets || !partials || N <= 0 || N > 65535 || P1 <= 0 || P2 <= 0)
    return ACFM_E_BADARG;
  if (partial_floats < acfm_chamfer_partial_floats(N, P1, P2)) return ACFM_E_WORKSPACE;
  const int nb1 = ch_blocks(P1), nb2 = ch_blocks(P2);
  RowScratch sc;
  sc.tickets = tickets; sc.partials = partials;
  hipLaunchKernelGGL(k_chamfer, dim3((unsigned)(nb1 + nb2), N), dim3(CH_TPB), 0, (hipStream_t)stream, x, y, x_len, y_len,
                     N, P1, P2, nb1, nb2, sums, idx_x, idx_y, sc);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_chamfer_backward(const float* x, const float* y, const int64_t* x_len, const int64_t* y_len,
                          const int32_t* idx_x, const int32_t* idx_y, const float* grad_sums, int N, int P1, int P2,
                          float* grad_x, float* grad_y, void* stream) {
  if (!x || !y || !idx_x || !idx_y || !grad_sums || !grad_x || !grad_y || N <= 0 || N > 65535 || P1 <= 0 || P2 <= 0)
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const int pm = P1 > P2 ? P1 : P2;
  if (pm <= CH_BWD_LDS_MAX_P) {
    hipLaunchKernelGGL(k_chamfer_bwd, dim3(2, N), dim3(CHB_TPB), sizeof(float) * 3 * (size_t)pm, st, x, y, x_len, y_len,
                       idx_x, idx_y, grad_sums, P1, P2, grad_x, grad_y);
    ACFM_CHECK_LAUNCH();
    return ACFM_OK;
  }
  const dim3 grid((unsigned)(((long long)pm + 255) / 256), 2, N);
  hipLaunchKernelGGL(k_chamfer_bwd_own, grid, dim3(256), 0, st, x, y, x_len, y_len, idx_x, idx_y, grad_sums, P1, P2,
                     grad_x, grad_y);
  hipLaunchKernelGGL(k_chamfer_bwd_scatter, grid, dim3(256), 0, st, x, y, x_len, y_len, idx_x, idx_y, grad_sums, P1, P2,
                     grad_x, grad_y);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

size_t acfm_mesh_term_partial_floats(int count) { return count <= 0 ? 0 : (size_t)term_blocks(count); }

int acfm_edge_length_loss(const float* verts, const int64_t* edges, const float* eweight, int P, int E, float target,
                          float* loss, uint32_t* tickets, float* partials, size_t partial_floats, void* stream) {
  if (!verts || !edges || !eweight || !loss || P <= 0 || E <= 0) return ACFM_E_BADARG;
  RowScratch sc;
  if (const int rc = term_scratch(E, tickets, partials, partial_floats, sc)) return rc;
  hipLaunchKernelGGL(k_edge_len, dim3(term_blocks(E)), dim3(FTPB), 0, (hipStream_t)stream, verts, edges, eweight, P, E,
                     target, loss, sc);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_edge_length_loss_backward(const float* verts, const int64_t* edges, const float* eweight,
                                   const float* grad_loss, int P, int E, float target, float* grad_verts,
                                   void* stream) {
  if (!verts || !edges || !eweight || !grad_loss || !grad_verts || P <= 0 || E <= 0) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_async(grad_verts, sizeof(float) * 3 * (size_t)P, st) != ACFM_OK) return ACFM_E_LAUNCH;
  hipLaunchKernelGGL(k_edge_len_bwd, dim3(term_blocks(E)), dim3(FTPB), 0, st, verts, edges, eweight, grad_loss, P, E,
                     target, grad_verts);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_normal_consistency(const float* verts, const int64_t* quads, const float* qweight, int P, int Q, float* loss,
                            uint32_t* tickets, float* partials, size_t partial_floats, void* stream) {
  if (!verts || !quads || !qweight || !loss || P <= 0 || Q <= 0) return ACFM_E_BADARG;
  RowScratch sc;
  if (const int rc = term_scratch(Q, tickets, partials, partial_floats, sc)) return rc;
  hipLaunchKernelGGL(k_normal_cons, dim3(term_blocks(Q)), dim3(FTPB), 0, (hipStream_t)stream, verts, quads, qweight, P,
                     Q, loss, sc);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_normal_consistency_backward(const float* verts, const int64_t* quads, const float* qweight,
                                     const float* grad_loss, int P, int Q, float* grad_verts, void* stream) {
  if (!verts || !quads || !qweight || !grad_loss || !grad_verts || P <= 0 || Q <= 0) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_async(grad_verts, sizeof(float) * 3 * (size_t)P, st) != ACFM_OK) return ACFM_E_LAUNCH;
  hipLaunchKernelGGL(k_normal_cons_bwd, dim3(term_blocks(Q)), dim3(FTPB), 0, st, verts, quads, qweight, grad_loss, P, Q,
                     grad_verts);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
