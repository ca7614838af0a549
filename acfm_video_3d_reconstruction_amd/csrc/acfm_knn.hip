// PyTorch3D 0.3.0's point-set operators as gfx950 kernels:
//   acfm_knn_points{,_backward}   <- pytorch3d.ops.knn_points   (the K nearest points of p2 for every point of p1)
//   acfm_knn_gather{,_backward}   <- pytorch3d.ops.knn_gather   (rows of x by neighbour index)
// The forward writes every element of its outputs and uses no atomics: the same bits on every run.  The backward
// kernels add with float atomics (LDS or global): their sums can differ in the last bits from run to run.
#include "acfm_common.h"
#include "acfm_points.h"

namespace acfm {

// ---- knn_points forward -------------------------------------------------------------------------------------------
// k_chamfer's layout: a workgroup owns 64 points of p1, one per lane; its four waves scan a quarter of the cloud's
// candidates each, streaming them through a private LDS tile of KNN_TILE points (no workgroup barrier in the scan).
// Every lane keeps its KI best (distance, index) pairs sorted in registers; all loops over the list are unrolled, so
// every access has a constant index (a runtime index would send the list to scratch memory).  A candidate enters with
// d < list[j]: among equal distances the one scanned first -- the lower index -- stays in front.
// An insertion costs about 6 KI VALU operations for the whole wave, however few lanes need it, and with 64 lanes some
// lane nearly always does.  So for KI >= 4 a lane that beats its current worst only appends the candidate to a queue
// of its own in LDS (KNN_QUEUE entries); when any lane's queue is full (one wave-uniform test) every lane inserts its
// queue, oldest first, the lanes with shorter queues idling.  The worst a lane tests against is then out of date --
// too large, never too small -- so the queue holds a superset of what the list accepts, in scan order: the same lists.
// Afterwards waves 1..3 hand their lists over in LDS and wave 0 inserts them into its own, in wave order: the
// quarters are ascending index ranges, so the merged list obeys the same lowest-index rule as one ascending scan.
// The hand-over reuses the LDS of the tiles and queues (behind a workgroup barrier): 16 KB for K <= 2, 32 KB up to
// K = 16, 48 KB at K = 32.
constexpr int KNN_TPB = 256;
constexpr int KNN_TILE = 256;   // candidates per wave and round: four per lane
constexpr int KNN_Q = 64;       // query points per workgroup
constexpr int KNN_MAX_K = 32;
constexpr int KNN_QUEUE = 8;    // queued candidates per lane (4 KB per wave)

template <int KI>
__device__ __forceinline__ void knn_insert(float (&bd)[KI], int (&bi)[KI], float d, int v) {
#pragma unroll
  for (int j = KI - 1; j > 0; --j) {
    const bool up = d < bd[j - 1];      // slot j - 1 moves up into slot j
    const bool here = d < bd[j];        // (up implies here: the list is ascending)
    bd[j] = up ? bd[j - 1] : (here ? d : bd[j]);
    bi[j] = up ? bi[j - 1] : (here ? v : bi[j]);
  }
  if (d < bd[0]) { bd[0] = d; bi[0] = v; }
}

template <int KI>
__global__ __launch_bounds__(KNN_TPB) void k_knn(const float* __restrict__ p1, const float* __restrict__ p2,
                                                 const int64_t* __restrict__ len1, const int64_t* __restrict__ len2,
                                                 int P1, int P2, int K, float* __restrict__ dists,
                                                 int64_t* __restrict__ idx) {
  constexpr bool QUEUED = KI >= 4;                   // (up to two slots the selects cost less than the queue)
  constexpr int QUEUE_F4 = 4 * KNN_QUEUE * 64 * 8 / 16;
  constexpr int TILE_F4 = 4 * KNN_TILE + (QUEUED ? QUEUE_F4 : 0);   // the four tiles, then the four waves' queues
  constexpr int MERGE_F4 = 3 * KI * 64 * 8 / 16;     // three lists of KI (float, int) pairs for 64 lanes
  __shared__ float4 s_raw[TILE_F4 > MERGE_F4 ? TILE_F4 : MERGE_F4];
  const int n = blockIdx.y, tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  const int lq = clamped_len(len1, n, P1), lc = clamped_len(len2, n, P2);
  const float* __restrict__ q = p1 + (size_t)n * P1 * 3;
  const float* __restrict__ c = p2 + (size_t)n * P2 * 3;
  const long long p = (long long)blockIdx.x * KNN_Q + lane;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (p < lq) { qx = q[3 * p]; qy = q[3 * p + 1]; qz = q[3 * p + 2]; }
  float bd[KI];
  int bi[KI];
#pragma unroll
  for (int j = 0; j < KI; ++j) { bd[j] = __builtin_inff(); bi[j] = -1; }
  if ((long long)blockIdx.x * KNN_Q < lq) {   // (the same for the whole workgroup)
    float4* tile = s_raw + wv * KNN_TILE;
    float* qd = reinterpret_cast<float*>(s_raw + (QUEUED ? 4 * KNN_TILE : 0)) + wv * (2 * KNN_QUEUE * 64) + lane;
    int* qi = reinterpret_cast<int*>(qd + KNN_QUEUE * 64);   // this lane's queue: qd / qi [KNN_QUEUE][64]
    int queued = 0;
    auto drain = [&]() {
#pragma unroll 1
      for (int b = 0; b < KNN_QUEUE; ++b) {
        const bool mine = b < queued;
        if (__builtin_amdgcn_ballot_w64(mine) == 0) break;
        knn_insert<KI>(bd, bi, mine ? qd[b * 64] : __builtin_inff(), mine ? qi[b * 64] : -1);
      }
      queued = 0;
    };
    const long long chunk = ((long long)lc + 3) / 4;
    const long long v0 = min(wv * chunk, (long long)lc), v1 = min((long long)lc, v0 + chunk);
    for (long long base = v0; base < v1; base += KNN_TILE) {
      float cx[4], cy[4], cz[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {     // the four loads of a lane are in flight together
        const long long v = min(base + u * 64 + lane, v1 - 1);
        cx[u] = c[3 * v]; cy[u] = c[3 * v + 1]; cz[u] = c[3 * v + 2];
      }
      wave_lds_sync();                  // the scan of the round before has read the tile
#pragma unroll
      for (int u = 0; u < 4; ++u) tile[u * 64 + lane] = make_float4(cx[u], cy[u], cz[u], 0.f);
      wave_lds_sync();
      const int cnt = (int)min((long long)KNN_TILE, v1 - base);
      const int b0 = (int)base;
      for (int k = 0; k < cnt; ++k) {
        const float4 t = tile[k];
        const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
        const float d = (dx * dx + dy * dy) + dz * dz;
        if (!QUEUED) {
          knn_insert<KI>(bd, bi, d, b0 + k);
        } else {
          if (d < bd[KI - 1]) { qd[queued * 64] = d; qi[queued * 64] = b0 + k; ++queued; }
          if (__builtin_amdgcn_ballot_w64(queued == KNN_QUEUE) != 0) drain();
        }
      }
    }
    if (QUEUED) drain();
  }
  float* md = reinterpret_cast<float*>(s_raw);   // [3][KI][64]
  int* mi = reinterpret_cast<int*>(md + 3 * KI * 64);
  __syncthreads();                      // every wave is done with its tile: the lists may overwrite them
  if (wv != 0) {
#pragma unroll
    for (int j = 0; j < KI; ++j) {
      md[((wv - 1) * KI + j) * 64 + lane] = bd[j];
      mi[((wv - 1) * KI + j) * 64 + lane] = bi[j];
    }
  }
  __syncthreads();
  if (wv != 0) return;
#pragma unroll 1
  for (int e = 0; e < 3 * KI; ++e) {    // wave 1's list, then wave 2's, then wave 3's, each in its own order
    const float d = md[e * 64 + lane];
    const int v = mi[e * 64 + lane];
    if (__builtin_amdgcn_ballot_w64(d < bd[KI - 1]) != 0) knn_insert<KI>(bd, bi, d, v);
  }
  if (p >= P1) return;
  // every slot of the row is written: a padded row, the columns past the other cloud's length (and a slot that no
  // finite distance reached) hold 0 / 0
  // (a lane stores its own row: K consecutive elements per lane, K-strided across the wave -- not coalesced.  Its
  // share of the kernel's time is not measured; a transpose through LDS would coalesce it)
  const int kv = p < lq ? min(K, lc) : 0;
  float* __restrict__ od = dists + ((size_t)n * P1 + p) * K;
  int64_t* __restrict__ oi = idx + ((size_t)n * P1 + p) * K;
#pragma unroll
  for (int j = 0; j < KI; ++j) {
    if (j < K) {
      const bool ok = j < kv && bi[j] >= 0;
      od[j] = ok ? bd[j] : 0.f;
      oi[j] = ok ? (int64_t)bi[j] : (int64_t)0;
    }
  }
}

// ---- knn_points backward ------------------------------------------------------------------------------------------
// d / d p1_i = sum_k 2 g_ik (p1_i - p2[idx_ik]) over the valid slots, d / d p2_j = the negated terms of the slots that
// hold j.  As k_chamfer_bwd: one workgroup per cloud keeps grad_p2 [P2,3] in LDS (12 B per point, CH_BWD_LDS_MAX_P
// points at most), adds into it with LDS atomics and stores whole rows; grad_p1 rows are written by their owner.
// Past the bound k_knn_bwd_global does the same with global atomics into a zero-filled grad_p2, one thread per point of
// p1 over the whole grid.  The one workgroup walks all P1 K slots of its cloud (about 3.8 ns per slot on an MI355X), so
// on the device it is ahead of the grid-wide kernel nowhere past a few hundred slots; what it saves is the host's second
// call, 50 us and more of an eager step.  It is therefore kept only up to KNN_BWD_LDS_MAX_SLOTS, a compromise between
// the two (the measurements: DESIGN.md "K nearest neighbours").
// A slot whose index is outside [0, l2) sends nothing.  The order of the float additions varies: grad_p2 is not
// bit-reproducible.
constexpr int KNNB_TPB = 512;
constexpr long long KNN_BWD_LDS_MAX_SLOTS = 16384;

struct KnnRow { float a, b, c; };

__device__ __forceinline__ KnnRow knn_bwd_row(const float* __restrict__ q, const float* __restrict__ c,
                                              const int64_t* __restrict__ idx, const float* __restrict__ g,
                                              long long i, int K, int kv, int lc, float* __restrict__ gc) {
  KnnRow r = {0.f, 0.f, 0.f};
  const float qx = q[3 * i], qy = q[3 * i + 1], qz = q[3 * i + 2];
  for (int k = 0; k < kv; ++k) {
    const int64_t j = idx[(size_t)i * K + k];
    if (j < 0 || j >= lc) continue;
    const float gg = 2.0f * g[(size_t)i * K + k];
    const float tx = gg * (qx - c[3 * j]), ty = gg * (qy - c[3 * j + 1]), tz = gg * (qz - c[3 * j + 2]);
    r.a += tx; r.b += ty; r.c += tz;
    atomicAdd(&gc[3 * j], -tx); atomicAdd(&gc[3 * j + 1], -ty); atomicAdd(&gc[3 * j + 2], -tz);
  }
  return r;
}

__global__ __launch_bounds__(KNNB_TPB) void k_knn_bwd(const float* __restrict__ p1, const float* __restrict__ p2,
                                                      const int64_t* __restrict__ len1,
                                                      const int64_t* __restrict__ len2,
                                                      const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                      int P1, int P2, int K, float* __restrict__ gp1,
                                                      float* __restrict__ gp2) {
  extern __shared__ float s_g[];   // [P2][3]
  const int n = blockIdx.x, tid = threadIdx.x;
  const int lq = clamped_len(len1, n, P1), lc = clamped_len(len2, n, P2);
  const int kv = min(K, lc);
  const float* __restrict__ q = p1 + (size_t)n * P1 * 3;
  const float* __restrict__ c = p2 + (size_t)n * P2 * 3;
  const int64_t* __restrict__ ix = idx + (size_t)n * P1 * K;
  const float* __restrict__ gn = g + (size_t)n * P1 * K;
  float* __restrict__ gq = gp1 + (size_t)n * P1 * 3;
  for (int i = tid; i < 3 * P2; i += KNNB_TPB) s_g[i] = 0.f;
  __syncthreads();
  for (int i = tid; i < P1; i += KNNB_TPB) {
    KnnRow r = {0.f, 0.f, 0.f};
    if (i < lq) r = knn_bwd_row(q, c, ix, gn, i, K, kv, lc, s_g);
    gq[3 * i] = r.a; gq[3 * i + 1] = r.b; gq[3 * i + 2] = r.c;
  }
  __syncthreads();
  float* __restrict__ gcn = gp2 + (size_t)n * P2 * 3;
  for (int i = tid; i < 3 * P2; i += KNNB_TPB) gcn[i] = s_g[i];
}

__global__ __launch_bounds__(256) void k_knn_bwd_global(const float* __restrict__ p1, const float* __restrict__ p2,
                                                        const int64_t* __restrict__ len1,
                                                        const int64_t* __restrict__ len2,
                                                        const int64_t* __restrict__ idx, const float* __restrict__ g,
                                                        int P1, int P2, int K, float* __restrict__ gp1,
                                                        float* __restrict__ gp2) {
  const int n = blockIdx.y;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= P1) return;
  const int lq = clamped_len(len1, n, P1), lc = clamped_len(len2, n, P2);
  KnnRow r = {0.f, 0.f, 0.f};
  if (i < lq)
    r = knn_bwd_row(p1 + (size_t)n * P1 * 3, p2 + (size_t)n * P2 * 3, idx + (size_t)n * P1 * K,
                           g + (size_t)n * P1 * K, i, K, min(K, lc), lc, gp2 + (size_t)n * P2 * 3);
  float* __restrict__ gq = gp1 + ((size_t)n * P1 + i) * 3;
  gq[0] = r.a; gq[1] = r.b; gq[2] = r.c;
}

// ---- knn_gather ---------------------------------------------------------------------------------------------------
// One thread per output element (n, l, k, u).  The index is tested before it is used: a slot with k >= lengths[n] or
// an index outside [0, M) reads nothing, yields 0 and sends no gradient (index rows that another operator left
// unwritten by contract arrive here).
constexpr int KG_TPB = 256;

template <typename I>
__device__ __forceinline__ bool kg_source(const I* __restrict__ idx, const int64_t* __restrict__ len, size_t e, int M,
                                          int U, int K, size_t LK, size_t& src) {
  const size_t s = e / (size_t)U;          // the slot (n, l, k)
  const int u = (int)(e - s * (size_t)U), k = (int)(s % (size_t)K), n = (int)(s / LK);
  if (k >= clamped_len(len, n, M)) return false;
  const long long j = (long long)idx[s];
  if (j < 0 || j >= M) return false;
  src = ((size_t)n * M + (size_t)j) * U + u;
  return true;
}

template <typename I>
__global__ __launch_bounds__(KG_TPB) void k_knn_gather(const float* __restrict__ x, const I* __restrict__ idx,
                                                       const int64_t* __restrict__ len, int M, int U, int K, size_t LK,
                                                       size_t total, float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * KG_TPB + threadIdx.x;
  if (e >= total) return;
  size_t src;
  out[e] = kg_source(idx, len, e, M, U, K, LK, src) ? x[src] : 0.f;
}

template <typename I>
__global__ __launch_bounds__(KG_TPB) void k_knn_gather_bwd(const float* __restrict__ go, const I* __restrict__ idx,
                                                           const int64_t* __restrict__ len, int M, int U, int K,
                                                           size_t LK, size_t total, float* __restrict__ gx) {
  const size_t e = (size_t)blockIdx.x * KG_TPB + threadIdx.x;
  if (e >= total) return;
  size_t src;
  if (kg_source(idx, len, e, M, U, K, LK, src)) atomicAdd(&gx[src], go[e]);
}

static inline bool mul_ok(size_t a, size_t b, size_t& out) { return !__builtin_mul_overflow(a, b, &out); }

// N L K U and N M U as element counts; false if a product overflows or the grid would pass 2^31 - 1 workgroups
static inline bool kg_sizes(int N, int M, int U, int L, int K, size_t& total, size_t& xcount) {
  if (N <= 0 || M <= 0 || U <= 0 || L <= 0 || K <= 0) return false;
  size_t lk, nlk;
  if (!mul_ok((size_t)L, (size_t)K, lk) || !mul_ok((size_t)N, lk, nlk) || !mul_ok(nlk, (size_t)U, total)) return false;
  if (!mul_ok((size_t)N, (size_t)M, xcount) || !mul_ok(xcount, (size_t)U, xcount)) return false;
  size_t bytes;
  if (!mul_ok(total, (size_t)8, bytes) || !mul_ok(xcount, (size_t)4, bytes)) return false;
  return (total + KG_TPB - 1) / KG_TPB <= (size_t)0x7fffffff;
}

template <int KI>
static inline void launch_knn(dim3 grid, hipStream_t st, const float* p1, const float* p2, const int64_t* l1,
                              const int64_t* l2, int P1, int P2, int K, float* dists, int64_t* idx) {
  hipLaunchKernelGGL(k_knn<KI>, grid, dim3(KNN_TPB), 0, st, p1, p2, l1, l2, P1, P2, K, dists, idx);
}

static inline bool knn_sizes(int N, int P1, int P2, int K) {
  if (N <= 0 || N > 65535 || P1 <= 0 || P2 <= 0 || K < 1 || K > KNN_MAX_K) return false;
  size_t slots, bytes;   // N P1 K slots of 8 bytes, N P 3 floats
  if (!mul_ok((size_t)N * (size_t)P1, (size_t)K, slots) || !mul_ok(slots, (size_t)8, bytes)) return false;
  return mul_ok((size_t)N * (size_t)P1, (size_t)12, bytes) && mul_ok((size_t)N * (size_t)P2, (size_t)12, bytes);
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_knn_points(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2, int N, int P1,
                    int P2, int K, float* dists, int64_t* idx, void* stream) {
  if (!p1 || !p2 || !dists || !idx || !knn_sizes(N, P1, P2, K)) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((long long)P1 + KNN_Q - 1) / KNN_Q), (unsigned)N);
  // a K between two instantiations runs the next one and stores its first K columns
  if (K <= 1) launch_knn<1>(grid, st, p1, p2, lengths1, lengths2, P1, P2, K, dists, idx);
  else if (K <= 2) launch_knn<2>(grid, st, p1, p2, lengths1, lengths2, P1, P2, K, dists, idx);
  else if (K <= 4) launch_knn<4>(grid, st, p1, p2, lengths1, lengths2, P1, P2, K, dists, idx);
  else if (K <= 8) launch_knn<8>(grid, st, p1, p2, lengths1, lengths2, P1, P2, K, dists, idx);
  else if (K <= 16) launch_knn<16>(grid, st, p1, p2, lengths1, lengths2, P1, P2, K, dists, idx);
  else launch_knn<32>(grid, st, p1, p2, lengths1, lengths2, P1, P2, K, dists, idx);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_knn_points_backward(const float* p1, const float* p2, const int64_t* lengths1, const int64_t* lengths2,
                             const int64_t* idx, const float* grad_dists, int N, int P1, int P2, int K, float* grad_p1,
                             float* grad_p2, void* stream) {
  if (!p1 || !p2 || !idx || !grad_dists || !grad_p1 || !grad_p2 || !knn_sizes(N, P1, P2, K)) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (P2 <= CH_BWD_LDS_MAX_P && (long long)P1 * K <= KNN_BWD_LDS_MAX_SLOTS) {
    hipLaunchKernelGGL(k_knn_bwd, dim3((unsigned)N), dim3(KNNB_TPB), sizeof(float) * 3 * (size_t)P2, st, p1, p2,
                       lengths1, lengths2, idx, grad_dists, P1, P2, K, grad_p1, grad_p2);
    ACFM_CHECK_LAUNCH();
    return ACFM_OK;
  }
  if (zero_async(grad_p2, sizeof(float) * 3 * (size_t)N * (size_t)P2, st) != ACFM_OK) return ACFM_E_LAUNCH;
  hipLaunchKernelGGL(k_knn_bwd_global, dim3((unsigned)(((long long)P1 + 255) / 256), (unsigned)N), dim3(256), 0, st, p1,
                     p2, lengths1, lengths2, idx, grad_dists, P1, P2, K, grad_p1, grad_p2);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_knn_gather(const float* x, const void* idx, int idx_is_int64, const int64_t* lengths, int N, int M, int U,
                    int L, int K, float* out, void* stream) {
  size_t total, xcount;
  if (!x || !idx || !out || !kg_sizes(N, M, U, L, K, total, xcount)) return ACFM_E_BADARG;
  const dim3 grid((unsigned)((total + KG_TPB - 1) / KG_TPB));
  const size_t LK = (size_t)L * (size_t)K;
  if (idx_is_int64)
    hipLaunchKernelGGL(k_knn_gather<int64_t>, grid, dim3(KG_TPB), 0, (hipStream_t)stream, x, (const int64_t*)idx,
                       lengths, M, U, K, LK, total, out);
  else
    hipLaunchKernelGGL(k_knn_gather<int32_t>, grid, dim3(KG_TPB), 0, (hipStream_t)stream, x, (const int32_t*)idx,
                       lengths, M, U, K, LK, total, out);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_knn_gather_backward(const float* grad_out, const void* idx, int idx_is_int64, const int64_t* lengths, int N,
                             int M, int U, int L, int K, float* grad_x, void* stream) {
  size_t total, xcount;
  if (!grad_out || !idx || !grad_x || !kg_sizes(N, M, U, L, K, total, xcount)) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  if (zero_async(grad_x, sizeof(float) * xcount, st) != ACFM_OK) return ACFM_E_LAUNCH;
  const dim3 grid((unsigned)((total + KG_TPB - 1) / KG_TPB));
  const size_t LK = (size_t)L * (size_t)K;
  if (idx_is_int64)
    hipLaunchKernelGGL(k_knn_gather_bwd<int64_t>, grid, dim3(KG_TPB), 0, st, grad_out, (const int64_t*)idx, lengths, M,
                       U, K, LK, total, grad_x);
  else
    hipLaunchKernelGGL(k_knn_gather_bwd<int32_t>, grid, dim3(KG_TPB), 0, st, grad_out, (const int32_t*)idx, lengths, M,
                       U, K, LK, total, grad_x);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
