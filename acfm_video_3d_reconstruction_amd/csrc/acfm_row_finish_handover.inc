// FRAGMENT, no include guard: the ticket finish's hand-over (the partials leave as returning exchanges, then the ticket
// is drawn), included in row_finish and in row_finish_published of acfm_row_finish.h, on purpose.  Shared as text and
// not as a function: with it in a common function the compiler scheduled every kernel that calls row_finish
// differently, and their machine code is pinned (DESIGN.md, "The step's tail in one launch", "One text per kernel body").
//   expects: sc, row, nblk, blk, mine, and C (a constant expression)
//   leaves:  lane; ticket, in every lane (nblk - 1: this wave drew the row's last ticket).  The including function's
//            own return for the other waves follows, then acfm_row_finish_sum.inc.
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
