// The ticket finish of the per-row sums (RowScratch / row_finish), shared by the loss kernels of acfm_loss.hip and
// the template-fit kernels of acfm_fit.hip.
#pragma once
#include "acfm_common.h"

namespace acfm {

// ---- per-mesh sums in one launch: no zero fill of the output, no float atomics (the *_ws entry points) -------------
// Every workgroup of mesh `row` hands its C partial sums over in `partials`, draws a ticket, and the workgroup that
// draws the mesh's last ticket adds the partials in workgroup order 0, 1, 2, ... and stores the result: the same
// inputs give the same bits, and the output needs no prior contents.  The ticket is a WRAPPING increment
// (limit nblk - 1): the word is 0 again when the launch ends, so the caller zeroes it once, at allocation.
//
// The hand-over does not use a device-scope fence.  Such a fence in front of the ticket is a write-back of the
// XCD's whole L2 (buffer_wbl2 sc1), once per workgroup: measured at 9x the kernel time (DESIGN.md section 5,
// tools/variants/loss_ticket_finish.patch).  Instead every word that crosses workgroups is itself a device-scope
// atomic, performed at the memory side like the float atomicAdd it replaces: the partials go out as RETURNING
// exchanges, the wave waits for the old values to come back -- the exchanges have been performed by then -- and
// only then draws its ticket; the last workgroup reads the partials with device-scope atomic loads, after its own
// ticket came back.  The wait for the exchanges is the use of their old values (the empty asm: s_waitcnt vmcnt(0));
// the workgroup-scope fences keep the compiler from moving the atomics across it and do no cache maintenance.
//
// THIS RESTS ON THE HARDWARE, NOT ON THE MEMORY MODEL: relaxed atomics with workgroup-scope fences give no formal
// happens-before between workgroups.  What it needs is (1) a returning device-scope read-modify-write comes back only
// after it was performed where every XCD sees it, and (2) a device-scope atomic load (sc1) does not answer from a stale
// line of the reader's own L2.  Both hold on gfx942 / gfx950; a compiler that drops the wait, or an architecture
// with another coherence point, breaks it SILENTLY (a stale partial in a sum).  After a change of either, read the ISA
// (global_atomic_swap sc0 / s_waitcnt vmcnt(0) / global_atomic_inc sc0 / global_load_dword sc1) and run
// tests/test_gpu_loss_reductions.py: the graph replayed on changed inputs and the two-stream test read partials
// that other XCDs wrote in the launch before with different values, so a stale read fails their bit comparison.
struct RowScratch {
  unsigned* tickets;   // [N], zero between launches; nullptr = the atomics form behind a zero fill (plain entry points)
  float* partials;     // [N][nblk][C], any contents
};
// Called by one whole wave (lanes 0..63 of it); lane c < C carries the workgroup's partial sum c in `mine`.
template <int C>
__device__ __forceinline__ void row_finish(const RowScratch& sc, int row, int nblk, int blk, float mine,
                                           float* __restrict__ out_row) {
  const int lane = threadIdx.x & 63;
  unsigned* slot = reinterpret_cast<unsigned*>(sc.partials) + ((size_t)row * nblk + blk) * C;
  unsigned old = 0u;
  if (lane < C)
    old = __hip_atomic_exchange(slot + lane, __float_as_uint(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(old));   // the old values are back: the exchanges were performed
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  unsigned ticket = 0u;
  if (lane == 0) ticket = atomicInc(&sc.tickets[row], (unsigned)(nblk - 1));
  ticket = __shfl(ticket, 0, 64);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (ticket != (unsigned)(nblk - 1)) return;
  const unsigned* rowp = reinterpret_cast<const unsigned*>(sc.partials) + (size_t)row * nblk * C;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int b0 = 0; b0 < nblk; b0 += 64) {    // lane l holds workgroup b0 + l; added one after the other, in order
    float x[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
      x[c] = (b0 + lane < nblk) ? __uint_as_float(__hip_atomic_load(rowp + (size_t)(b0 + lane) * C + c, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT))
                                : 0.f;
    const int cnt = min(64, nblk - b0);
    for (int l = 0; l < cnt; ++l) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[c]), l));
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (lane == c) out_row[c] = acc[c];
}

// row_finish for a launch whose workgroups go on to read the rows that OTHER workgroups finished (k_step_tail's
// total).  The hand-over, the ticket and the sum are row_finish line for line -- written out a second time, not shared:
// with the sum in a common function the compiler scheduled every kernel that calls row_finish differently, and their
// machine code is pinned (tools/isa_diff.py against the parent) -- so a row has the same bits.  The row then leaves
// as returning device-scope exchanges, like the partials, and has been performed where every XCD sees it when this
// returns true: in the wave that finished the row, and in no other.
template <int C>
__device__ __forceinline__ bool row_finish_published(const RowScratch& sc, int row, int nblk, int blk, float mine,
                                                     float* __restrict__ out_row) {
  const int lane = threadIdx.x & 63;
  unsigned* slot = reinterpret_cast<unsigned*>(sc.partials) + ((size_t)row * nblk + blk) * C;
  unsigned old = 0u;
  if (lane < C)
    old = __hip_atomic_exchange(slot + lane, __float_as_uint(mine), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(old));   // the old values are back: the exchanges were performed
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  unsigned ticket = 0u;
  if (lane == 0) ticket = atomicInc(&sc.tickets[row], (unsigned)(nblk - 1));
  ticket = __shfl(ticket, 0, 64);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  if (ticket != (unsigned)(nblk - 1)) return false;
  const unsigned* rowp = reinterpret_cast<const unsigned*>(sc.partials) + (size_t)row * nblk * C;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.f;
  for (int b0 = 0; b0 < nblk; b0 += 64) {    // lane l holds workgroup b0 + l; added one after the other, in order
    float x[C];
#pragma unroll
    for (int c = 0; c < C; ++c)
      x[c] = (b0 + lane < nblk) ? __uint_as_float(__hip_atomic_load(rowp + (size_t)(b0 + lane) * C + c, __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT))
                                : 0.f;
    const int cnt = min(64, nblk - b0);
    for (int l = 0; l < cnt; ++l) {
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[c]), l));
    }
  }
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (lane == c) v = acc[c];
  unsigned was = 0u;
  if (lane < C)
    was = __hip_atomic_exchange(reinterpret_cast<unsigned*>(out_row) + lane, __float_as_uint(v), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_AGENT);
  asm volatile("" ::"v"(was));   // the old values are back: the row is where every XCD sees it
  return true;
}

}  // namespace acfm
