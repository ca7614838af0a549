// FRAGMENT, no include guard: the body of the masked texture MSE for one workgroup, included once in k_tex_mse and
// once in tex_mse_block (k_step_tail's role) of acfm_loss.hip, on purpose.  The text is shared by inclusion and not
// through a function because, called as a function, the same body changed the scalar address code of the kernels
// whose machine code is pinned (DESIGN.md, "The step's tail in one launch", the bullet "One text per kernel body").
//   expects: tex, img, m (the mask), HW, RB, n (the mesh), blk (the workgroup's index within the mesh), s_red [4] in
//            LDS, and PIX_FWD (pixels per workgroup, a constant expression)
//   leaves:  tid; the four waves' sums of (tex m - img m)^2 in s_red[wave], behind a workgroup barrier
  const int tid = threadIdx.x;
  const size_t b3 = (size_t)n * 3 * HW, r3 = (size_t)(n % RB) * 3 * HW, b1 = (size_t)(n % RB) * HW;
  const int start = blk * PIX_FWD;
  const int end = min(start + PIX_FWD, HW);
  float acc = 0.f;
  if ((HW & 3) == 0) {   // 16-byte loads
    // The mask first: where a piece's four mask values are all zero, (t m - g m)^2 is +0 for finite t and g and
    // acc + (+0) == acc, so the piece's six colour loads fetch nothing (the reference mask covers about a sixth of
    // a frame).  No branch does that: the colours come through buffer loads over the workgroup's pixel range, and a
    // lane whose piece is not wanted (or lies past the end) presents an offset outside the range, for which the
    // hardware returns zeros without a memory access.  Every piece then goes through the same expression in the
    // same order as before; an unread piece contributes (0 * 0 - 0 * 0)^2 = +0.
    constexpr int U = PIX_FWD / (LTPB * 4);
    constexpr int UB = U < 4 ? U : 4;   // pieces whose colour loads are in flight together (24 VGPRs each)
    static_assert(PIX_FWD % (LTPB * 4) == 0 && U % UB == 0, "a workgroup's pixels are whole rounds of one 16-byte piece per thread");
    const unsigned range_bytes = (unsigned)(end - start) * 4u;   // <= PIX_FWD * 4
    const __amdgpu_buffer_rsrc_t rm = pixel_range(m + b1 + start, range_bytes);
    float4 mk[U];   // (the same way: a piece past the end reads as zeros, and no branch splits the loads up)
#pragma unroll
    for (int u = 0; u < U; ++u) mk[u] = load16_in_range(rm, (u * LTPB + tid) * 16);
    __amdgpu_buffer_rsrc_t rt[3], rg[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      rt[c] = pixel_range(tex + b3 + (size_t)c * HW + start, range_bytes);
      rg[c] = pixel_range(img + r3 + (size_t)c * HW + start, range_bytes);
    }
#pragma unroll
    for (int u0 = 0; u0 < U; u0 += UB) {
      float4 t[UB][3], g[UB][3];
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const float4 k = mk[u0 + u];
        const bool want = k.x != 0.f || k.y != 0.f || k.z != 0.f || k.w != 0.f;
        const int off = want ? ((u0 + u) * LTPB + tid) * 16 : OUT_OF_RANGE;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          t[u][c] = load16_in_range(rt[c], off);
          g[u][c] = load16_in_range(rg[c], off);
        }
      }
#pragma unroll
      for (int u = 0; u < UB; ++u) {
        const float4 k = mk[u0 + u];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const float d0 = t[u][c].x * k.x - g[u][c].x * k.x, d1 = t[u][c].y * k.y - g[u][c].y * k.y;
          const float d2 = t[u][c].z * k.z - g[u][c].z * k.z, d3 = t[u][c].w * k.w - g[u][c].w * k.w;
          acc += d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
        }
      }
    }
  } else
  for (int i = start + tid; i < end; i += LTPB) {
    const float mk = m[b1 + i];
    if (mk == 0.f) continue;   // adds +0 for finite colours: not read
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float d = tex[b3 + (size_t)c * HW + i] * mk - img[r3 + (size_t)c * HW + i] * mk;
      acc += d * d;
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) s_red[tid >> 6] = acc;
  __syncthreads();
