// FRAGMENT, no include guard: the ticket finish's in-order sum in the wave that drew the row's last ticket, included
// in row_finish and in row_finish_published behind acfm_row_finish_handover.inc, on purpose.  Shared as text and not as
// a function for the reason given there (DESIGN.md, "The step's tail in one launch", "One text per kernel body").
//   expects: sc, row, nblk, lane, and C (a constant expression)
//   leaves:  acc[c], in every lane: the row's sum c, the workgroups' partials added in workgroup order
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
