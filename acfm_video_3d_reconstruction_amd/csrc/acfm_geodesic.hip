// Surface distances between the vertices of a template mesh, for the handle weights `lbs` of MeshNet
// (multiframe/nnutils/mesh_net.py:69-85, 523-544, where gdist.local_gdist_matrix supplies them): shortest paths on the
// edge-Steiner graph of the mesh (DESIGN.md "Geodesic handles").
//   nodes   the V vertices, then m points per edge: node V + e m + (j - 1), j = 1..m, at a + (j / (m + 1)) (b - a),
//           a, b = the positions of edges[e] = (lo, hi)
//   arcs    inside every face all pairs of the 3 + 3 m nodes on its boundary, length = their Euclidean distance
//   D[s,v]  the shortest path from vertex s to vertex v; +inf where there is none
// One workgroup per (source, mesh) keeps the distances of ALL nodes in LDS and relaxes the faces until a whole sweep
// lowers nothing.  A wave takes one face at a time, lane l owning boundary node l: it loads the node's position and
// distance once, then reads every node of the face out of the other lanes' registers (v_readlane, no LDS traffic) and
// takes the minimum of d_src + |p - p_src|.  Only a lane that found something shorter touches LDS again, with one
// atomicMin on the value's bits (distances are >= 0 or +inf: their order is the order of the unsigned bits).
// A face whose distances have not changed since a visit that lowered nothing is skipped (a signature kept in registers).
// fl(d + w) is monotone in d, so the least fixed point -- which is what the sweeps converge to from above -- does not
// depend on the order in which waves relax: the same bits on every run.  No global atomics, nothing shared between
// workgroups, no scratch.
//
// k_geodesic_dev is the same relaxation for a graph that does not fit LDS (the 2562-vertex template at m >= 5): the
// distances of a workgroup's current (source, mesh) item live in ITS row of a device workspace, LDS keeps the sweep
// flags and the clean-face signatures (two words per face, all F faces).  A persistent grid of G workgroups; workgroup
// g takes items g, g + G, ... and fills its row with +inf for each.  No row is shared, there are no global tickets.
// Visibility: a distance is lowered with an agent-scope atomicMin, which executes at L2; a plain load could be served
// from a stale line of this CU's vector L1 -- still an upper bound, but a sweep could then "lower nothing" with an
// improvement pending and stop on a non-fixed point.  So EVERY access to a distance is an agent-scope relaxed atomic:
// geo_ld (global_load_dword sc1, which bypasses L1) for every read, geo_st for the fill, geo_min for the update.  No
// plain load or store touches the workspace, so there is nothing an acquire would have to invalidate.  The workgroup
// barrier behind each sweep orders them: an atomicMin whose result a lane has tested has executed at L2, and an sc1
// load issued after the barrier reads L2.
#include "acfm_common.h"

#include <math.h>

namespace acfm {

constexpr int GEO_TPB = 1024;                 // 16 waves: the LDS request allows one workgroup per CU anyway
constexpr int GEO_WAVES = GEO_TPB / ACFM_WAVE;
constexpr int GEO_HEAD = 16;                  // bytes in front of the distances: three sweep flags (and alignment)
constexpr size_t GEO_LDS_MAX = ACFM_GEODESIC_LDS_MAX;

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += (unsigned)__shfl_xor((int)v, o, 64);
  return v;
}

__global__ __launch_bounds__(GEO_TPB) void k_geodesic(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                      const int32_t* __restrict__ edges,
                                                      const int32_t* __restrict__ face_edges, int V, int F, int E, int m,
                                                      const int32_t* __restrict__ sources, int S,
                                                      float* __restrict__ out, int32_t* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_geo[];
  int* s_flag = (int*)s_geo;                             // [3]: sweep i raises s_flag[i % 3]
  float* s_d = (float*)(s_geo + GEO_HEAD);               // [V + m E]
  unsigned* s_bits = (unsigned*)(s_geo + GEO_HEAD);

  const int tid = threadIdx.x, lane = tid & (ACFM_WAVE - 1), wave = tid / ACFM_WAVE;
  const int n = blockIdx.y;
  const int nodes = V + m * E, nb = 3 + 3 * m;           // nb <= 63
  const int src = sources ? sources[blockIdx.x] : (int)blockIdx.x;
  float* row = out + ((size_t)n * S + blockIdx.x) * V;
  const float* vn = verts + (size_t)n * V * 3;

  if (src < 0 || src >= V) {                             // the Python layer refuses these; never index LDS with one
    for (int v = tid; v < V; v += GEO_TPB) row[v] = __builtin_nanf("");
    if (tid == 0) *status = 2;
    return;
  }
  for (int i = tid; i < nodes; i += GEO_TPB) s_d[i] = INFINITY;
  if (tid < 3) s_flag[tid] = 0;
  __syncthreads();
  if (tid == 0) s_d[src] = 0.0f;
  __syncthreads();

  // what lane l is in a face: vertex l, or point j of the face's edge (l - 3) / m
  const int k = lane - 3;
  const int slot = m > 0 && k >= 0 ? k / m : 0;
  const int j = m > 0 && k >= 0 ? k - slot * m + 1 : 0;
  const float t = (float)j / (float)(m + 1);
  const bool mine = lane < nb;

  // Skipping clean faces.  A wave meets the same faces in every sweep.  When a visit lowered nothing, lane (i mod 64)
  // keeps the signature of the distances that visit read, for the wave's first 128 faces (F <= 2048: beyond that a face
  // is simply relaxed every time).  Distances only fall, so an equal signature means equal values, and relaxing them
  // again would lower nothing again: the skip is exactly a relaxation without effect, and the fixed point keeps its bits.
  unsigned clean_lo0 = ~0u, clean_hi0 = ~0u, clean_lo1 = ~0u, clean_hi1 = ~0u;   // ~0: no clean visit yet (sums are < 2^22)

  bool converged = false;
  for (int sweep = 0; sweep < nodes; ++sweep) {
    if (tid == 0) s_flag[(sweep + 1) % 3] = 0;           // last read before the previous barrier, next raised after this one
    bool lowered = false;
    int i = 0;                                           // this wave's i-th face
    for (int f = wave; f < F; f += GEO_WAVES, ++i) {
      int node = -1, e = -1;
      if (mine) {
        if (lane < 3) {
          const int v = faces[3 * (size_t)f + lane];
          if (v >= 0 && v < V) node = v;
        } else {
          e = face_edges[3 * (size_t)f + slot];
          if (e >= 0 && e < E) node = V + e * m + (j - 1);
        }
      }
      if (__any(mine && node < 0)) continue;             // a table entry out of range: the face is left out (wave-uniform)
      const float d = mine ? s_d[node] : INFINITY;
      if (!__any(d < INFINITY)) continue;                // the front has not reached this face yet
      // the face's signature: the sum of its distances' bits, as two 16-bit column sums (each < 2^22)
      const unsigned bits = mine ? __builtin_bit_cast(unsigned, d) : 0u;
      const unsigned s_lo = wave_sum_u32(bits & 0xffffu), s_hi = wave_sum_u32(bits >> 16);
      const bool tracked = i < 2 * ACFM_WAVE;
      const int keeper = i & (ACFM_WAVE - 1);
      if (tracked) {
        const unsigned c_lo = (unsigned)__builtin_amdgcn_readlane((int)(i < ACFM_WAVE ? clean_lo0 : clean_lo1), keeper);
        const unsigned c_hi = (unsigned)__builtin_amdgcn_readlane((int)(i < ACFM_WAVE ? clean_hi0 : clean_hi1), keeper);
        if (c_lo == s_lo && c_hi == s_hi) continue;      // the very values that lowered nothing last time
      }
      float px = 0.f, py = 0.f, pz = 0.f;
      bool ok = true;
      if (mine) {
        if (lane < 3) {
          px = vn[3 * (size_t)node]; py = vn[3 * (size_t)node + 1]; pz = vn[3 * (size_t)node + 2];
        } else {
          const int lo = edges[2 * (size_t)e], hi = edges[2 * (size_t)e + 1];
          ok = lo >= 0 && lo < V && hi >= 0 && hi < V;
          if (ok) {
            const float ax = vn[3 * (size_t)lo], ay = vn[3 * (size_t)lo + 1], az = vn[3 * (size_t)lo + 2];
            px = ax + t * (vn[3 * (size_t)hi] - ax);
            py = ay + t * (vn[3 * (size_t)hi + 1] - ay);
            pz = az + t * (vn[3 * (size_t)hi + 2] - az);
          }
        }
      }
      if (__any(!ok)) continue;
      float best = d;
      for (int q = 0; q < nb; ++q) {
        const float sd = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), q));
        const float dx = px - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, px), q));
        const float dy = py - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, py), q));
        const float dz = pz - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pz), q));
        best = fminf(best, sd + sqrtf(dx * dx + dy * dy + dz * dz));
      }
      const bool shorter = mine && best < d;
      if (shorter) {
        const unsigned b = __builtin_bit_cast(unsigned, best);
        if (atomicMin(&s_bits[node], b) > b) lowered = true;
      }
      const bool clean = !__any(shorter);                // (a ballot of the whole wave: taken before the lanes part)
      if (tracked && lane == keeper) {
        const unsigned k_lo = clean ? s_lo : ~0u, k_hi = clean ? s_hi : ~0u;
        if (i < ACFM_WAVE) { clean_lo0 = k_lo; clean_hi0 = k_hi; } else { clean_lo1 = k_lo; clean_hi1 = k_hi; }
      }
    }
    if (lowered) s_flag[sweep % 3] = 1;
    __syncthreads();
    if (!s_flag[sweep % 3]) { converged = true; break; }
  }
  // (the break is workgroup-uniform: every thread read the same flag after the same barrier)
  if (!converged) {
    // more sweeps than nodes: impossible for shortest paths with arcs >= 0; say so instead of returning upper bounds
    for (int v = tid; v < V; v += GEO_TPB) row[v] = __builtin_nanf("");
    if (tid == 0) *status = 1;
    return;
  }
  for (int v = tid; v < V; v += GEO_TPB) row[v] = s_d[v];
}

// ---- the same relaxation with the distances in a workspace row (header comment) ----
constexpr int GEOD_PER_CU = 2;                // default grid: workgroups per CU (2 x 16 waves fill a CU's wave slots)
constexpr int GEOD_SIG_FACES = (int)((GEO_LDS_MAX / GEOD_PER_CU - GEO_HEAD) / 8);   // faces with a signature in LDS: 9598

__device__ __forceinline__ float geo_ld(const unsigned* p) {
  return __builtin_bit_cast(float, __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}
__device__ __forceinline__ void geo_st(unsigned* p, unsigned bits) {
  __hip_atomic_store(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned geo_min(unsigned* p, unsigned bits) {
  return __hip_atomic_fetch_min(p, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(GEO_TPB) __attribute__((amdgpu_waves_per_eu(GEOD_PER_CU * GEO_WAVES / 4))) void k_geodesic_dev(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                          const int32_t* __restrict__ edges,
                                                          const int32_t* __restrict__ face_edges, int V, int F, int E,
                                                          int m, const int32_t* __restrict__ sources, int S,
                                                          long long items, float* __restrict__ out,
                                                          int32_t* __restrict__ status, unsigned* ws, size_t row_words,
                                                          int sig_faces) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s_geo[];
  int* s_flag = (int*)s_geo;                             // [3]: sweep i raises s_flag[i % 3]
  unsigned* s_sig = (unsigned*)(s_geo + GEO_HEAD);       // [sig_faces][2]: only the wave that owns the face touches its pair

  const int tid = threadIdx.x, lane = tid & (ACFM_WAVE - 1), wave = tid / ACFM_WAVE;
  const int nodes = V + m * E, nb = 3 + 3 * m;           // nodes <= row_words; nb <= 63
  unsigned* w_bits = ws + (size_t)blockIdx.x * row_words;   // this workgroup's row, [nodes]

  // what lane l is in a face: vertex l, or point j of the face's edge (l - 3) / m
  const int k = lane - 3;
  const int slot = m > 0 && k >= 0 ? k / m : 0;
  const int j = m > 0 && k >= 0 ? k - slot * m + 1 : 0;
  const float t = (float)j / (float)(m + 1);
  const bool mine = lane < nb;

  for (long long item = blockIdx.x; item < items; item += gridDim.x) {   // item = n S + s, as out is laid out
    const int s = (int)(item % S);
    const float* vn = verts + (size_t)(item / S) * V * 3;
    const int src = sources ? sources[s] : s;
    float* row = out + (size_t)item * V;
    if (src < 0 || src >= V) {                           // the Python layer refuses these; never index the row with one
      for (int v = tid; v < V; v += GEO_TPB) row[v] = __builtin_nanf("");
      if (tid == 0) *status = 2;
      continue;                                          // (workgroup-uniform; nothing below has started)
    }
    for (int i = tid; i < nodes; i += GEO_TPB) geo_st(&w_bits[i], __builtin_bit_cast(unsigned, INFINITY));
    for (int i = tid; i < 2 * sig_faces; i += GEO_TPB) s_sig[i] = ~0u;   // ~0: no clean visit yet (sums are < 2^22)
    if (tid < 3) s_flag[tid] = 0;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the fill has left this wave before any other wave goes on
    __syncthreads();
    if (tid == 0) geo_st(&w_bits[src], 0u);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    bool converged = false;
    for (int sweep = 0; sweep < nodes; ++sweep) {
      if (tid == 0) s_flag[(sweep + 1) % 3] = 0;         // last read before the previous barrier, next raised after this one
      bool lowered = false;
      for (int f = wave; f < F; f += GEO_WAVES) {
        int node = -1, e = -1;
        if (mine) {
          if (lane < 3) {
            const int v = faces[3 * (size_t)f + lane];
            if (v >= 0 && v < V) node = v;
          } else {
            e = face_edges[3 * (size_t)f + slot];
            if (e >= 0 && e < E) node = V + e * m + (j - 1);
          }
        }
        if (__any(mine && node < 0)) continue;           // a table entry out of range: the face is left out (wave-uniform)
        const float d = mine ? geo_ld(&w_bits[node]) : INFINITY;
        if (!__any(d < INFINITY)) continue;              // the front has not reached this face yet
        // the face's signature, as in k_geodesic; kept in LDS for every face below sig_faces.  Distances only fall, so
        // an equal signature means the very values of a visit that lowered nothing: the skip is a relaxation without effect.
        const unsigned bits = mine ? __builtin_bit_cast(unsigned, d) : 0u;
        const unsigned s_lo = wave_sum_u32(bits & 0xffffu), s_hi = wave_sum_u32(bits >> 16);
        const bool tracked = f < sig_faces;
        if (tracked && s_sig[2 * f] == s_lo && s_sig[2 * f + 1] == s_hi) continue;
        float px = 0.f, py = 0.f, pz = 0.f;
        bool ok = true;
        if (mine) {
          if (lane < 3) {
            px = vn[3 * (size_t)node]; py = vn[3 * (size_t)node + 1]; pz = vn[3 * (size_t)node + 2];
          } else {
            const int lo = edges[2 * (size_t)e], hi = edges[2 * (size_t)e + 1];
            ok = lo >= 0 && lo < V && hi >= 0 && hi < V;
            if (ok) {
              const float ax = vn[3 * (size_t)lo], ay = vn[3 * (size_t)lo + 1], az = vn[3 * (size_t)lo + 2];
              px = ax + t * (vn[3 * (size_t)hi] - ax);
              py = ay + t * (vn[3 * (size_t)hi + 1] - ay);
              pz = az + t * (vn[3 * (size_t)hi + 2] - az);
            }
          }
        }
        if (__any(!ok)) continue;
        float best = d;
        for (int q = 0; q < nb; ++q) {
          const float sd = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, d), q));
          const float dx = px - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, px), q));
          const float dy = py - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, py), q));
          const float dz = pz - __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, pz), q));
          best = fminf(best, sd + sqrtf(dx * dx + dy * dy + dz * dz));
        }
        const bool shorter = mine && best < d;
        if (shorter) {
          const unsigned b = __builtin_bit_cast(unsigned, best);
          if (geo_min(&w_bits[node], b) > b) lowered = true;
        }
        const bool clean = !__any(shorter);              // (a ballot of the whole wave: taken before the lanes part)
        if (tracked && lane == 0) {
          s_sig[2 * f] = clean ? s_lo : ~0u;
          s_sig[2 * f + 1] = clean ? s_hi : ~0u;
        }
      }
      if (lowered) s_flag[sweep % 3] = 1;
      __syncthreads();
      if (!s_flag[sweep % 3]) { converged = true; break; }
    }
    // (the break is workgroup-uniform: every thread read the same flag after the same barrier)
    if (!converged) {
      for (int v = tid; v < V; v += GEO_TPB) row[v] = __builtin_nanf("");
      if (tid == 0) *status = 1;
    } else {
      for (int v = tid; v < V; v += GEO_TPB) row[v] = geo_ld(&w_bits[v]);
    }
    __syncthreads();                                     // the next item refills the row and the flags
  }
}

}  // namespace acfm

using namespace acfm;

// the grid of k_geodesic_dev: min(S N, max_workgroups), max_workgroups = 0 -> GEOD_PER_CU per CU of the current device
static long long geo_dev_grid(int N, int S, int max_workgroups) {
  long long cap = max_workgroups;
  if (cap == 0) {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return 0;
    cap = (long long)GEOD_PER_CU * cus;
  }
  const long long items = (long long)N * S;
  return items < cap ? items : cap;
}
// a row: the distances of all nodes, padded to whole 128-byte lines so that no two workgroups share one
static size_t geo_dev_row_bytes(int V, int E, int m) {
  return (sizeof(unsigned) * ((size_t)V + (size_t)m * (size_t)E) + 127) & ~(size_t)127;
}

extern "C" {

size_t acfm_geodesic_lds_bytes(int V, int E, int m) {
  if (V <= 0 || E < 0 || m < 0 || m > ACFM_GEODESIC_MAX_STEINER) return 0;
  return (size_t)GEO_HEAD + sizeof(float) * ((size_t)V + (size_t)m * (size_t)E);
}

int acfm_geodesic_distances(const float* verts, const int32_t* faces, const int32_t* edges, const int32_t* face_edges,
                            int N, int V, int F, int E, int m, const int32_t* sources, int S, float* out,
                            int32_t* status, void* stream) {
  if (!verts || !faces || !edges || !face_edges || !out || !status || N <= 0 || N > 65535 || V <= 0 || F <= 0 || E <= 0 ||
      m < 0 || m > ACFM_GEODESIC_MAX_STEINER || S <= 0 || (!sources && S != V))
    return ACFM_E_BADARG;
  const size_t lds = acfm_geodesic_lds_bytes(V, E, m);
  if (lds == 0 || lds > GEO_LDS_MAX) return ACFM_E_BADARG;   // the graph has to fit one workgroup's LDS
  hipLaunchKernelGGL(k_geodesic, dim3((unsigned)S, (unsigned)N), dim3(GEO_TPB), lds, (hipStream_t)stream, verts, faces,
                     edges, face_edges, V, F, E, m, sources, S, out, status);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

size_t acfm_geodesic_workspace_bytes(int N, int V, int E, int m, int S, int max_workgroups) {
  if (N <= 0 || N > 65535 || V <= 0 || E < 0 || m < 0 || m > ACFM_GEODESIC_MAX_STEINER || S <= 0 || max_workgroups < 0 ||
      (size_t)V + (size_t)m * (size_t)E > (size_t)INT32_MAX)
    return 0;
  return (size_t)geo_dev_grid(N, S, max_workgroups) * geo_dev_row_bytes(V, E, m);
}

int acfm_geodesic_distances_dev(const float* verts, const int32_t* faces, const int32_t* edges,
                                const int32_t* face_edges, int N, int V, int F, int E, int m, const int32_t* sources,
                                int S, float* out, int32_t* status, int max_workgroups, void* ws, size_t ws_bytes,
                                void* stream) {
  if (!verts || !faces || !edges || !face_edges || !out || !status || !ws || N <= 0 || N > 65535 || V <= 0 || F <= 0 ||
      E <= 0 || m < 0 || m > ACFM_GEODESIC_MAX_STEINER || S <= 0 || (!sources && S != V) || max_workgroups < 0 ||
      (size_t)V + (size_t)m * (size_t)E > (size_t)INT32_MAX)
    return ACFM_E_BADARG;
  const long long G = geo_dev_grid(N, S, max_workgroups);
  if (G <= 0 || G > INT32_MAX) return ACFM_E_BADARG;
  const size_t row = geo_dev_row_bytes(V, E, m);
  if (ws_bytes < (size_t)G * row) return ACFM_E_WORKSPACE;
  const int sig_faces = F < GEOD_SIG_FACES ? F : GEOD_SIG_FACES;   // a face beyond them is relaxed in every sweep
  const size_t lds = (size_t)GEO_HEAD + 2 * sizeof(unsigned) * (size_t)sig_faces;
  hipLaunchKernelGGL(k_geodesic_dev, dim3((unsigned)G), dim3(GEO_TPB), lds, (hipStream_t)stream, verts, faces, edges,
                     face_edges, V, F, E, m, sources, S, (long long)N * S, out, status, (unsigned*)ws,
                     row / sizeof(unsigned), sig_faces);
  ACFM_CHECK_LAUNCH();
  return ACFM_OK;
}

}  // extern "C"
