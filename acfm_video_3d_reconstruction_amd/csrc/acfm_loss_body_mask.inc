// FRAGMENT, no include guard: the body of the fused silhouette losses for one workgroup, included once in
// k_mask_losses and once in mask_losses_block (k_step_tail's role) of acfm_loss.hip, on purpose.  The text is shared
// by inclusion and not through a function because, called as a function, the same body changed the register
// allocation and schedule of the kernels whose machine code is pinned (DESIGN.md, "The step's tail in one launch",
// the bullet "One text per kernel body").
//   expects: mask, gt, edt, HW, RB, n (the mesh), blk (the workgroup's index within the mesh), s_red [4][4] in LDS,
//            and PIX_FWD (pixels per workgroup, a constant expression)
//   leaves:  tid; the four waves' sums (sum|m-gt|, sum m*gt, sum(m+gt-m*gt), sum edt*m) in s_red[wave][0..3], behind a
//            workgroup barrier
  const int tid = threadIdx.x;
  const size_t base = (size_t)n * HW, rbase = (size_t)(n % RB) * HW;
  const int start = blk * PIX_FWD;
  const int end = min(start + PIX_FWD, HW);
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  const bool vec = ((HW & 3) == 0);
  if (vec) {
    // the block's two 16-byte pieces per thread and array are loaded before any of them is used
    constexpr int U = PIX_FWD / (LTPB * 4);
    static_assert(PIX_FWD % (LTPB * 4) == 0, "whole rounds of one 16-byte piece per thread");
    float4 m[U], g[U], e[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int i = start + (u * LTPB + tid) * 4;
      const bool in = i < end;
      m[u] = in ? *reinterpret_cast<const float4*>(mask + base + i) : make_float4(0, 0, 0, 0);
      g[u] = (in && gt) ? *reinterpret_cast<const float4*>(gt + rbase + i) : make_float4(0, 0, 0, 0);
    }
    // edt m is +0 wherever the rendered mask is 0 (most of a frame): edt is fetched only for the pieces whose four mask
    // values are not all zero -- the other lanes present an offset outside the workgroup's range and get zeros back
    // without a memory access (load16_in_range), and a3 + (+0) == a3
    if (edt) {
      const __amdgpu_buffer_rsrc_t re = pixel_range(edt + rbase + start, (unsigned)(end - start) * 4u);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const bool want = m[u].x != 0.f || m[u].y != 0.f || m[u].z != 0.f || m[u].w != 0.f;
        e[u] = load16_in_range(re, want ? (u * LTPB + tid) * 16 : OUT_OF_RANGE);
      }
    } else {
#pragma unroll
      for (int u = 0; u < U; ++u) e[u] = make_float4(0, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      a0 += fabsf(m[u].x - g[u].x) + fabsf(m[u].y - g[u].y) + fabsf(m[u].z - g[u].z) + fabsf(m[u].w - g[u].w);
      a1 += m[u].x * g[u].x + m[u].y * g[u].y + m[u].z * g[u].z + m[u].w * g[u].w;
      a2 += (m[u].x + g[u].x - m[u].x * g[u].x) + (m[u].y + g[u].y - m[u].y * g[u].y) +
            (m[u].z + g[u].z - m[u].z * g[u].z) + (m[u].w + g[u].w - m[u].w * g[u].w);
      a3 += e[u].x * m[u].x + e[u].y * m[u].y + e[u].z * m[u].z + e[u].w * m[u].w;
    }
  } else {
    for (int i = start + tid; i < end; i += LTPB) {
      const float m = mask[base + i], g = gt ? gt[rbase + i] : 0.f, e = edt ? edt[rbase + i] : 0.f;
      a0 += fabsf(m - g); a1 += m * g; a2 += m + g - m * g; a3 += e * m;
    }
  }
  a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a3 = wave_sum(a3);
  const int w = tid >> 6;
  if ((tid & 63) == 0) { s_red[w][0] = a0; s_red[w][1] = a1; s_red[w][2] = a2; s_red[w][3] = a3; }
  __syncthreads();
