// Boundary-point sampling for gfx950: the random subset of loss_utils.bds_loss (:211,
// torch.randperm(P)[:n_samples]) drawn on the device, so that the step has no host round trip and
// can be captured into a hipGraph.
//
// Definition (boundary_sampling.subset_host restates it in numpy and is the specification):
//   slot i of row r in draw t has the key  key64 = x0 << 32 | x1,  (x0, x1, x2, x3) = Philox4x32-10 with
//   key (seed lo, seed hi) and counter (i, r, t lo, t hi);  the subset of a row of P_r slots is the
//   min(n, P_r) slots with the smallest (key64, i), written in ascending slot order, then -1.
// Keys are recomputed from the index wherever they are needed: nothing is stored per slot.
#include "acfm_common.h"

namespace acfm {

constexpr int STPB = 1024;          // one workgroup per row
constexpr int SWAVES = STPB / 64;

__device__ __forceinline__ unsigned long long philox_key64(unsigned i, unsigned r, unsigned t_lo, unsigned t_hi,
                                                           unsigned k0, unsigned k1) {
  unsigned c0 = i, c1 = r, c2 = t_lo, c3 = t_hi;
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return ((unsigned long long)c0 << 32) | c1;
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

}  // extern "C"
