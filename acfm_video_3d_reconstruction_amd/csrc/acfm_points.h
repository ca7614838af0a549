// What the point-cloud units share (acfm_fit.hip: chamfer; acfm_knn.hip: K nearest neighbours, gather).
#pragma once
#include "acfm_common.h"

namespace acfm {

// The backward kernels that keep one cloud's [P,3] gradient in LDS: 12 B per point, at most 150 KB.
constexpr int CH_BWD_LDS_MAX_P = 12800;

// a cloud's length, clamped to [0, P]; no lengths = every row counts
__device__ __forceinline__ int clamped_len(const int64_t* __restrict__ len, int n, int P) {
  if (!len) return P;
  const int64_t l = len[n];
  return l < 0 ? 0 : (l > (int64_t)P ? P : (int)l);
}
// orders a wave's own LDS writes and reads: a tile that only this wave touches needs no workgroup barrier
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace acfm
