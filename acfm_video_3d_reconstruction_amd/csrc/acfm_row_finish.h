// The ticket finish of the per-row sums (RowScratch / row_finish), shared by the loss kernels of acfm_loss.hip and
// the template-fit kernels of acfm_fit.hip.
#pragma once
#include "acfm_common.h"

namespace acfm {

// ---- per-mesh sums in one launch: no zero fill of the output, no float atomics (entry points given tickets) --------
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
// The hand-over with the ticket, and the in-order sum, are one text each for this function and row_finish_published:
// two fragments included in both (why not a common function: see the fragments).  What differs between the two stands
// here: the return behind the ticket and the way the row leaves.
template <int C>
__device__ __forceinline__ void row_finish(const RowScratch& sc, int row, int nblk, int blk, float mine,
                                           float* __restrict__ out_row) {
#include "acfm_row_finish_handover.inc"
  if (ticket != (unsigned)(nblk - 1)) return;
#include "acfm_row_finish_sum.inc"
#pragma unroll
  for (int c = 0; c < C; ++c)
    if (lane == c) out_row[c] = acc[c];
}

// row_finish for a launch whose workgroups go on to read the rows that OTHER workgroups finished (k_step_tail's
// total).  The hand-over, the ticket and the sum are row_finish's own text (the two fragments), so a row has the same
// bits.  The row then leaves as returning device-scope exchanges, like the partials, and has been performed where
// every XCD sees it when this returns true: in the wave that finished the row, and in no other.
template <int C>
__device__ __forceinline__ bool row_finish_published(const RowScratch& sc, int row, int nblk, int blk, float mine,
                                                     float* __restrict__ out_row) {
#include "acfm_row_finish_handover.inc"
  if (ticket != (unsigned)(nblk - 1)) return false;
#include "acfm_row_finish_sum.inc"
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
