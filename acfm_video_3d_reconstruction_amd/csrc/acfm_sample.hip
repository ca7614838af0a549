// Boundary-point sampling for gfx950: the random subset of loss_utils.bds_loss (:211,
// torch.randperm(P)[:n_samples]) drawn on the device, so that the step has no host round trip and
// can be captured into a hipGraph.
//
// Definition (boundary_sampling.subset_host restates it in numpy and is the specification):
//   slot i of row r in draw t has the key  key64 = x0 << 32 | x1,  (x0, x1, x2, x3) = Philox4x32-10 with
//   key (seed lo, seed hi) and counter (i, r, t lo, t hi);  the subset of a row of P_r slots is the
//   min(n, P_r) slots with the smallest (key64, i), written in ascending slot order, then -1.
// Keys are recomputed from the index wherever they are needed: nothing is stored per slot.
//
// Below it, on the same (seed, draw) state and the same generator: the surface samples of the template fit
// (sample_points_from_meshes), their CDF, and their backward.
#include "acfm_common.h"

namespace acfm {

constexpr int STPB = 1024;          // one workgroup per row
constexpr int SWAVES = STPB / 64;

struct Philox4 { unsigned x0, x1, x2, x3; };

__device__ __forceinline__ Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0,
                                                 unsigned k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}

__device__ __forceinline__ unsigned long long philox_key64(unsigned i, unsigned r, unsigned t_lo, unsigned t_hi,
                                                           unsigned k0, unsigned k1) {
  const Philox4 x = philox4x32_10(i, r, t_lo, t_hi, k0, k1);
  return ((unsigned long long)x.x0 << 32) | x.x1;
}

// Pass 1: a radix select over the key's eight digits, most significant first -- a 256-bin histogram in LDS of the
// digit among the slots whose higher digits equal the prefix found so far, then the bin in which the k-th smallest
// key lies.  The search ends as soon as the whole bin is wanted (always the case once the bin holds one key; at
// P = 3000 that is after two or three digits): the threshold is then the largest key with that prefix.
// Pass 2: the slots in ascending order, 1024 at a time; a slot is taken if its key is below the threshold, or equal
// to it while fewer than `need_eq` equal keys precede it (ballot + prefix count, as k_boundaries packs its points).
__global__ __launch_bounds__(STPB) void k_boundary_subset(const long long* __restrict__ state,
                                                          const int* __restrict__ counts, int n_counts, int P,
                                                          int n_samples, int* __restrict__ sel) {
  __shared__ int s_hist[256];
  __shared__ int s_lt[SWAVES], s_eq[SWAVES];
  __shared__ int s_bin, s_k, s_all, s_pr;
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const unsigned long long seed = (unsigned long long)state[0], draw = (unsigned long long)state[1];
  const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32), t_lo = (unsigned)draw, t_hi = (unsigned)(draw >> 32);
  int* out = sel + (size_t)r * n_samples;

  // P_r: the row's own count, or (one shared row) the largest count; without counts the padded length
  int Pr = P;
  if (counts) {
    if (gridDim.x == 1) {
      int m = 0;
      for (int j = tid; j < n_counts; j += STPB) m = max(m, counts[j]);
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o, 64));
      if (tid == 0) s_pr = 0;
      __syncthreads();
      if (lane == 0) atomicMax(&s_pr, m);
      __syncthreads();
      Pr = s_pr;
    } else {
      Pr = counts[r];
    }
    Pr = min(max(Pr, 0), P);
  }
  const int k = min(n_samples, Pr);

  unsigned long long thr = ~0ull;   // Pr <= n_samples: every slot is taken, and no key is computed
  int need_eq = 0x7fffffff;
  const bool all = Pr <= n_samples;
  if (!all) {
    unsigned long long prefix = 0;
    int want = k;                   // rank (from 1) of the wanted key among those that share the prefix
    need_eq = 0;
    for (int d = 7; d >= 0; --d) {
      if (tid < 256) s_hist[tid] = 0;
      __syncthreads();
      const int sh = 8 * d;
      for (int i = tid; i < Pr; i += STPB) {
        const unsigned long long key = philox_key64((unsigned)i, (unsigned)r, t_lo, t_hi, k0, k1);
        if (d == 7 || (key >> (sh + 8)) == (prefix >> (sh + 8))) atomicAdd(&s_hist[(int)(key >> sh) & 255], 1);
      }
      __syncthreads();
      if (wv == 0) {                // the bin of rank `want`: lane l holds bins 4 l .. 4 l + 3
        const int h0 = s_hist[4 * lane], h1 = s_hist[4 * lane + 1], h2 = s_hist[4 * lane + 2], h3 = s_hist[4 * lane + 3];
        const int c = h0 + h1 + h2 + h3;
        int incl = c;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int up = __shfl_up(incl, o, 64);
          if (lane >= o) incl += up;
        }
        const int excl = incl - c;
        if (excl < want && want <= incl) {
          int b = 4 * lane, before = excl, h = h0;
          if (want > before + h) { before += h; ++b; h = h1; }
          if (want > before + h) { before += h; ++b; h = h2; }
          if (want > before + h) { before += h; ++b; h = h3; }
          s_bin = b; s_k = want - before; s_all = (want - before == h) ? 1 : 0;
        }
      }
      __syncthreads();
      prefix |= (unsigned long long)s_bin << sh;
      want = s_k;
      if (s_all) {                  // the whole bin is wanted: every key that starts with the prefix
        thr = prefix | (sh ? ((1ull << sh) - 1ull) : 0ull);
        need_eq = 0x7fffffff;
        break;
      }
      if (d == 0) { thr = prefix; need_eq = want; }
    }
  }

  const unsigned long long lower = (1ull << lane) - 1ull;
  int base_lt = 0, base_eq = 0;     // taken slots, and slots with the threshold key, before this round
  for (int base = 0; base < Pr; base += STPB) {
    const int i = base + tid;
    bool lt = false, eq = false;
    if (i < Pr) {
      if (all) lt = true;
      else {
        const unsigned long long key = philox_key64((unsigned)i, (unsigned)r, t_lo, t_hi, k0, k1);
        lt = key < thr; eq = key == thr;
      }
    }
    const unsigned long long blt = __ballot(lt), beq = __ballot(eq);
    __syncthreads();                // the previous round's counts have been read
    if (lane == 0) { s_lt[wv] = __popcll(blt); s_eq[wv] = __popcll(beq); }
    __syncthreads();
    int eq_before = base_eq, tot_eq = 0;
#pragma unroll
    for (int w = 0; w < SWAVES; ++w) {
      if (w < wv) eq_before += s_eq[w];
      tot_eq += s_eq[w];
    }
    // an equal key is taken while fewer than need_eq precede it: the first need_eq of them in slot order
    const int eq_rank = eq_before + __popcll(beq & lower);
    const bool take = lt || (eq && eq_rank < need_eq);
    // position = taken slots before this one = (lt before) + min(eq before, need_eq)
    int lt_before = base_lt, tot_lt = 0;
#pragma unroll
    for (int w = 0; w < SWAVES; ++w) {
      if (w < wv) lt_before += s_lt[w];
      tot_lt += s_lt[w];
    }
    if (take) {
      const int pos = lt_before + __popcll(blt & lower) + min(eq_rank, need_eq);
      if (pos < n_samples) out[pos] = i;
    }
    base_lt += tot_lt; base_eq += tot_eq;
  }
  for (int i = k + tid; i < n_samples; i += STPB) out[i] = -1;
}

// after every row has read the draw (a launch of its own: no workgroup may read state[1] after another advanced it)
__global__ void k_advance_draw(long long* __restrict__ state) {
  if (threadIdx.x == 0 && blockIdx.x == 0) state[1] = state[1] + 1;
}

// ------------------------------------------------------------------------------------------------------------------
// Surface samples of pytorch3d.ops.sample_points_from_meshes (utils/geometry.py:110-111) drawn on the device.
// Definition (surface_sampling.surface_sample_host restates it in numpy and is the specification):
//   n_f = sqrt((cx cx + cy cy) + cz cz) of (b - a) x (c - a), 0 if not finite or a vertex id lies outside [0, P);
//   q_f = floor((n_f / n_max) 2^24), cdf = inclusive prefix sum of q in 64-bit integers (exact in any order);
//   sample s of mesh m in draw t: (x0, x1, x2, x3) = Philox4x32-10, key (seed lo, seed hi), counter (s, m, t lo, t hi);
//   target = ((x0 << 32 | x1) * total) >> 64, the face is the first f with cdf_f > target;
//   u = (x2 >> 8) 2^-24, v = (x3 >> 8) 2^-24, su = sqrt(u), p = ((1 - su) a + su (1 - v) b) + su v c.
constexpr int SCAN_TPB = 1024;      // k_surface_cdf: one workgroup per mesh, 1024 faces per scan chunk
constexpr int SCAN_WAVES = SCAN_TPB / 64;
constexpr int SS_TPB = 256;         // k_surface_sample / the global backward: one thread per sample
constexpr int SSB_TPB = 1024;       // k_surface_bwd_lds: one workgroup per mesh
constexpr int SS_BWD_LDS_MAX_V = 12800;   // 12 B of LDS per vertex <= 150 KB

struct Tri { float ax, ay, az, bx, by, bz, cx, cy, cz; bool ok; };

__device__ __forceinline__ Tri load_tri(const float* __restrict__ verts, const long long* __restrict__ faces, int f,
                                        int P) {
  Tri t;
  const long long i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
  t.ok = i0 >= 0 && i0 < P && i1 >= 0 && i1 < P && i2 >= 0 && i2 < P;
  if (t.ok) {
    t.ax = verts[3 * i0]; t.ay = verts[3 * i0 + 1]; t.az = verts[3 * i0 + 2];
    t.bx = verts[3 * i1]; t.by = verts[3 * i1 + 1]; t.bz = verts[3 * i1 + 2];
    t.cx = verts[3 * i2]; t.cy = verts[3 * i2 + 1]; t.cz = verts[3 * i2 + 2];
  } else {
    t.ax = t.ay = t.az = t.bx = t.by = t.bz = t.cx = t.cy = t.cz = 0.f;
  }
  return t;
}

// the faces [f0, f1) of mesh m: the table's entries clamped into [0, F] and made non-decreasing, so that a table that
// does not describe the arrays never sends a thread outside them
__device__ __forceinline__ void mesh_faces(const long long* __restrict__ first, int m, int F, int& f0, int& f1) {
  const long long a = first[m], b = first[m + 1];
  f0 = (int)(a < 0 ? 0 : (a > F ? F : a));
  f1 = (int)(b < f0 ? f0 : (b > F ? F : b));
}

// Pass 1: twice the area of every face (kept as float bits in the face's own 64-bit slot of `cdf`) and the mesh's
// maximum.  Pass 2, 1024 faces at a time: the quantised weights, a wave scan, the waves' totals and the carry of the
// earlier chunks through LDS.  A thread reads and writes only the slots f0 + k 1024 + tid: no slot is shared.
__global__ __launch_bounds__(SCAN_TPB) void k_surface_cdf(const float* __restrict__ verts,
                                                          const long long* __restrict__ faces,
                                                          const long long* __restrict__ first, int P, int F,
                                                          unsigned long long* __restrict__ cdf) {
  __shared__ float s_max[SCAN_WAVES];
  __shared__ unsigned long long s_tot[SCAN_WAVES];
  const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  int f0, f1;
  mesh_faces(first, m, F, f0, f1);
  if (f1 <= f0) return;

  float nmax = 0.f;
  for (int f = f0 + tid; f < f1; f += SCAN_TPB) {
    const Tri t = load_tri(verts, faces, f, P);
    const float ux = t.bx - t.ax, uy = t.by - t.ay, uz = t.bz - t.az;
    const float vx = t.cx - t.ax, vy = t.cy - t.ay, vz = t.cz - t.az;
    const float cx = uy * vz - uz * vy, cy = uz * vx - ux * vz, cz = ux * vy - uy * vx;
    float n = sqrtf((cx * cx + cy * cy) + cz * cz);
    if (!t.ok || !(n <= 3.402823466e38f)) n = 0.f;     // NaN and infinity count as no area
    cdf[f] = (unsigned long long)__float_as_uint(n);
    nmax = fmaxf(nmax, n);
  }
  nmax = wave_max(nmax);
  if (lane == 0) s_max[wv] = nmax;
  __syncthreads();
  nmax = s_max[0];
#pragma unroll
  for (int w = 1; w < SCAN_WAVES; ++w) nmax = fmaxf(nmax, s_max[w]);

  unsigned long long carry = 0;
  for (int base = f0; base < f1; base += SCAN_TPB) {
    const int f = base + tid;
    unsigned long long q = 0;
    if (f < f1 && nmax > 0.f) {
      const float n = __uint_as_float((unsigned)cdf[f]);
      q = (unsigned long long)floorf((n / nmax) * 16777216.0f);
    }
    unsigned long long incl = q;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned lo = __shfl_up((unsigned)incl, o, 64), hi = __shfl_up((unsigned)(incl >> 32), o, 64);
      if (lane >= o) incl += ((unsigned long long)hi << 32) | lo;
    }
    __syncthreads();                  // the previous chunk's totals have been read
    if (lane == 63) s_tot[wv] = incl;
    __syncthreads();
    unsigned long long before = carry, all = 0;
#pragma unroll
    for (int w = 0; w < SCAN_WAVES; ++w) {
      if (w < wv) before += s_tot[w];
      all += s_tot[w];
    }
    if (f < f1) cdf[f] = before + incl;
    carry += all;
  }
}

__global__ __launch_bounds__(SS_TPB) void k_surface_sample(const long long* __restrict__ state,
                                                           const float* __restrict__ verts,
                                                           const long long* __restrict__ faces,
                                                           const long long* __restrict__ first, int P, int F, int S,
                                                           const unsigned long long* __restrict__ cdf,
                                                           float* __restrict__ points, int* __restrict__ face_idx,
                                                           float* __restrict__ uv) {
  const int m = blockIdx.y, s = blockIdx.x * SS_TPB + threadIdx.x;
  if (s >= S) return;
  const unsigned long long seed = (unsigned long long)state[0], draw = (unsigned long long)state[1];
  int f0, f1;
  mesh_faces(first, m, F, f0, f1);
  const unsigned long long total = f1 > f0 ? cdf[f1 - 1] : 0ull;
  const size_t o = (size_t)m * S + s;
  if (total == 0ull) {                // no faces, or none with an area
    points[3 * o] = 0.f; points[3 * o + 1] = 0.f; points[3 * o + 2] = 0.f;
    face_idx[o] = -1;
    uv[2 * o] = 0.f; uv[2 * o + 1] = 0.f;
    return;
  }
  const Philox4 x = philox4x32_10((unsigned)s, (unsigned)m, (unsigned)draw, (unsigned)(draw >> 32), (unsigned)seed,
                                  (unsigned)(seed >> 32));
  const unsigned long long target = __umul64hi(((unsigned long long)x.x0 << 32) | x.x1, total);   // < total
  int lo = f0, hi = f1 - 1;           // the first face with cdf > target: cdf[f1 - 1] = total > target
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > target) hi = mid; else lo = mid + 1;
  }
  const float u = (float)(x.x2 >> 8) * 5.9604644775390625e-8f, v = (float)(x.x3 >> 8) * 5.9604644775390625e-8f;
  const float su = sqrtf(u);
  const float w0 = 1.0f - su, w1 = su * (1.0f - v), w2 = su * v;
  const Tri t = load_tri(verts, faces, lo, P);      // (a face with a vertex outside [0, P) has weight 0: never drawn)
  points[3 * o] = (w0 * t.ax + w1 * t.bx) + w2 * t.cx;
  points[3 * o + 1] = (w0 * t.ay + w1 * t.by) + w2 * t.cy;
  points[3 * o + 2] = (w0 * t.az + w1 * t.bz) + w2 * t.cz;
  face_idx[o] = lo;
  uv[2 * o] = u; uv[2 * o + 1] = v;
}

// what sample o adds to the three vertices of its face; false for a sample without a face
__device__ __forceinline__ bool surface_bwd_terms(const float* __restrict__ gp, const int* __restrict__ face_idx,
                                                  const float* __restrict__ uv, const long long* __restrict__ faces,
                                                  size_t o, int P, int F, long long id[3], float w[3], float g[3]) {
  const int f = face_idx[o];
  if (f < 0 || f >= F) return false;
  id[0] = faces[3 * (size_t)f]; id[1] = faces[3 * (size_t)f + 1]; id[2] = faces[3 * (size_t)f + 2];
  if (id[0] < 0 || id[0] >= P || id[1] < 0 || id[1] >= P || id[2] < 0 || id[2] >= P) return false;
  const float u = uv[2 * o], v = uv[2 * o + 1], su = sqrtf(u);
  w[0] = 1.0f - su; w[1] = su * (1.0f - v); w[2] = su * v;
  g[0] = gp[3 * o]; g[1] = gp[3 * o + 1]; g[2] = gp[3 * o + 2];
  return true;
}

// Equal-sized meshes (mesh m = vertices [m Vm, (m + 1) Vm)): one workgroup per mesh adds in LDS and writes every row
// of its mesh once.  What a face of mesh m would add to a vertex of ANOTHER mesh is dropped (packed meshes have no such
// face; the entry point's contract says so).  The order of the additions varies from run to run: NOT bit-reproducible
// (as k_chamfer_bwd).
__global__ __launch_bounds__(SSB_TPB) void k_surface_bwd_lds(const float* __restrict__ gp,
                                                             const int* __restrict__ face_idx,
                                                             const float* __restrict__ uv,
                                                             const long long* __restrict__ faces, int S, int P, int F,
                                                             int Vm, float* __restrict__ gv) {
  extern __shared__ float s_gv[];    // [Vm][3]
  const int m = blockIdx.x, tid = threadIdx.x;
  const long long v0 = (long long)m * Vm;
  for (int i = tid; i < 3 * Vm; i += SSB_TPB) s_gv[i] = 0.f;
  __syncthreads();
  for (int s = tid; s < S; s += SSB_TPB) {
    long long id[3];
    float w[3], g[3];
    if (!surface_bwd_terms(gp, face_idx, uv, faces, (size_t)m * S + s, P, F, id, w, g)) continue;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const long long l = id[k] - v0;
      if (l < 0 || l >= Vm) continue;           // a vertex of another mesh: dropped (see above)
      atomicAdd(&s_gv[3 * l], w[k] * g[0]);
      atomicAdd(&s_gv[3 * l + 1], w[k] * g[1]);
      atomicAdd(&s_gv[3 * l + 2], w[k] * g[2]);
    }
  }
  __syncthreads();
  for (int i = tid; i < 3 * Vm; i += SSB_TPB) gv[3 * (size_t)v0 + i] = s_gv[i];
}

// any layout: after a zero fill, one thread per sample, global float atomics
__global__ __launch_bounds__(SS_TPB) void k_surface_bwd_scatter(const float* __restrict__ gp,
                                                                const int* __restrict__ face_idx,
                                                                const float* __restrict__ uv,
                                                                const long long* __restrict__ faces, size_t NS, int P,
                                                                int F, float* __restrict__ gv) {
  const size_t o = (size_t)blockIdx.x * SS_TPB + threadIdx.x;
  if (o >= NS) return;
  long long id[3];
  float w[3], g[3];
  if (!surface_bwd_terms(gp, face_idx, uv, faces, o, P, F, id, w, g)) return;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicAdd(&gv[3 * id[k]], w[k] * g[0]);
    atomicAdd(&gv[3 * id[k] + 1], w[k] * g[1]);
    atomicAdd(&gv[3 * id[k] + 2], w[k] * g[2]);
  }
}

static bool surface_sizes_ok(int N, int S, int P, int F) {
  const long long lim = 0x7fffffffLL;
  return N > 0 && N <= 65535 && S > 0 && P > 0 && F >= 0 && 3LL * P <= lim && 3LL * F <= lim &&
         3LL * (long long)N * S <= lim;
}

}  // namespace acfm

using namespace acfm;

extern "C" {

int acfm_boundary_subset(int64_t* state, const int32_t* counts, int n_counts, int rows, int P, int n_samples,
                         int32_t* sel, void* stream) {
  if (!state || !sel || rows <= 0 || rows > 65535 || P <= 0 || P > (1 << 30) || n_samples <= 0) return ACFM_E_BADARG;
  if (counts ? (n_counts <= 0 || (rows != 1 && rows != n_counts)) : (n_counts != 0 || rows != 1)) return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  ProfScope ps(ACFM_PROF_BDS_SUBSET, st);
  hipLaunchKernelGGL(k_boundary_subset, dim3(rows), dim3(STPB), 0, st, (const long long*)state, counts, n_counts, P,
                     n_samples, sel);
  hipLaunchKernelGGL(k_advance_draw, dim3(1), dim3(64), 0, st, (long long*)state);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

size_t acfm_surface_sample_workspace_bytes(int N, int F) {
  if (N <= 0 || N > 65535 || F < 0 || 3LL * F > 0x7fffffffLL) return 0;
  return align256(sizeof(unsigned long long) * (size_t)(F > 0 ? F : 1));
}

int acfm_surface_sample(int64_t* state, const float* verts_packed, const int64_t* faces_packed,
                        const int64_t* faces_first_idx, const int64_t* faces_first_idx_host, int N, int S, int P, int F,
                        float* points, int32_t* face_idx, float* uv, void* workspace, size_t workspace_bytes,
                        void* stream) {
  if (!state || !verts_packed || !faces_first_idx || !points || !face_idx || !uv || !workspace ||
      !surface_sizes_ok(N, S, P, F) || (F > 0 && !faces_packed))
    return ACFM_E_BADARG;
  if (faces_first_idx_host) {         // the caller's host copy of the table: 0 <= first[0] <= ... <= first[N] <= F
    long long prev = 0;
    for (int m = 0; m <= N; ++m) {
      const long long cur = faces_first_idx_host[m];
      if (cur < prev || cur > F) return ACFM_E_BADARG;
      prev = cur;
    }
  }
  if (workspace_bytes < acfm_surface_sample_workspace_bytes(N, F)) return ACFM_E_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned long long* cdf = (unsigned long long*)workspace;
  const long long* faces = (const long long*)faces_packed;
  const long long* first = (const long long*)faces_first_idx;
  if (F > 0) hipLaunchKernelGGL(k_surface_cdf, dim3(N), dim3(SCAN_TPB), 0, st, verts_packed, faces, first, P, F, cdf);
  hipLaunchKernelGGL(k_surface_sample, dim3((unsigned)((S + SS_TPB - 1) / SS_TPB), N), dim3(SS_TPB), 0, st,
                     (const long long*)state, verts_packed, faces, first, P, F, S, (const unsigned long long*)cdf,
                     points, face_idx, uv);
  hipLaunchKernelGGL(k_advance_draw, dim3(1), dim3(64), 0, st, (long long*)state);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

int acfm_surface_sample_backward(const float* grad_points, const int32_t* face_idx, const float* uv,
                                 const int64_t* faces_packed, int N, int S, int P, int F, int verts_per_mesh,
                                 float* grad_verts, void* stream) {
  if (!grad_points || !face_idx || !uv || !grad_verts || !surface_sizes_ok(N, S, P, F) || (F > 0 && !faces_packed) ||
      verts_per_mesh < 0)
    return ACFM_E_BADARG;
  hipStream_t st = (hipStream_t)stream;
  const long long* faces = (const long long*)faces_packed;
  if (verts_per_mesh > 0 && verts_per_mesh <= SS_BWD_LDS_MAX_V && (long long)verts_per_mesh * N == P) {
    hipLaunchKernelGGL(k_surface_bwd_lds, dim3(N), dim3(SSB_TPB), sizeof(float) * 3 * (size_t)verts_per_mesh, st,
                       grad_points, face_idx, uv, faces, S, P, F, verts_per_mesh, grad_verts);
    ACFM_CHECK_LAUNCH();
    return ACFM_OK;
  }
  if (zero_async(grad_verts, sizeof(float) * 3 * (size_t)P, st) != ACFM_OK) return ACFM_E_LAUNCH;
  const size_t NS = (size_t)N * S;
  hipLaunchKernelGGL(k_surface_bwd_scatter, dim3((unsigned)((NS + SS_TPB - 1) / SS_TPB)), dim3(SS_TPB), 0, st,
                     grad_points, face_idx, uv, faces, NS, P, F, grad_verts);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
