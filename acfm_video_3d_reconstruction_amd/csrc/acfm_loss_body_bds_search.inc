// FRAGMENT, no include guard: the boundary loss's search for one workgroup -- the lane's point, the staging of the
// visible vertices and the four waves' arg-min -- included once in k_bds_loss, k_bds_loss_sel and bds_block
// (k_step_tail's role) of acfm_loss.hip, on purpose.  The text is shared by inclusion and not through a function or a
// kernel template because, with the body in a common function, the compiler allocated the registers of the kernels
// whose machine code is pinned differently (DESIGN.md, "The step's tail in one launch", the bullet "One text per
// kernel body").  acfm_loss_body_bds_merge.inc continues it in wave 0; what stands between the two is the including
// function's own return.
//   expects: verts_xy, bds, vis, V, P, RB, n (the mesh), blk (the workgroup's index within the mesh),
//            s_best [4][64] and s_bi [4][64] in LDS, SEL (a constant expression) and sel, rows, S (read only under SEL)
//   leaves:  tid, wv, lane, p, bm, empty; best, bi: the wave's own minimum for the lane's point; every wave's minimum in
//            s_best[wave][lane] / s_bi[wave][lane], behind a workgroup barrier
  extern __shared__ float s_xy[];  // [V][2]: per quarter, its visible vertices packed to the front; then int s_idx[V]
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
  // the lane's boundary point first: its load is in flight while the vertices are staged
  const int p = blk * 64 + lane;
  float bx = 0.f, by = 0.f, bm = 0.f;
  bool empty = false;
  if constexpr (SEL) {
    int s = -1;
    if (p < S) s = sel[(size_t)((n % RB) % rows) * S + p];
    empty = s < 0 || s >= P;
    if (!empty) {
      const float* b = bds + ((size_t)(n % RB) * P + s) * 3;
      bx = b[0]; by = b[1]; bm = b[2];
    }
  } else {
    if (p < P) {
      const float* b = bds + ((size_t)(n % RB) * P + p) * 3;
      bx = b[0]; by = b[1]; bm = b[2];
    }
  }
  const int chunk = (V + 3) / 4, v0 = wv * chunk, v1 = min(V, v0 + chunk);
  int* s_idx = reinterpret_cast<int*>(s_xy + 2 * (size_t)V);
  int nvis = 0;
  {
    const unsigned long long lt = (1ull << lane) - 1ull;
    // (unconditional loads, four rounds in flight: with the loads behind the visibility test the staging was a
    // chain of memory latencies)
    for (int base = v0; base < v1; base += 4 * 64) {
      uint8_t vz[4];
      float2 xy[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int v = min(base + u * 64 + lane, v1 - 1);
        vz[u] = vis[(size_t)n * V + v];
        xy[u] = *reinterpret_cast<const float2*>(verts_xy + ((size_t)n * V + v) * 2);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int v = base + u * 64 + lane;
        const bool keep = (v < v1) && vz[u] != 0;
        const unsigned long long m = __ballot(keep);
        if (keep) {
          const int pos = v0 + nvis + __popcll(m & lt);
          *reinterpret_cast<float2*>(s_xy + 2 * pos) = xy[u];
          s_idx[pos] = v;
        }
        nvis += __popcll(m);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  float best = 1000.0f;  // loss_utils.py:228: invisible vertices sit at distance 1000
  int bi = -1;
#pragma unroll 8
  for (int v = v0; v < v0 + nvis; ++v) {
    const float2 q = *reinterpret_cast<const float2*>(s_xy + 2 * v);
    const float dx = bx - q.x, dy = by - q.y;
    const float d = dx * dx + dy * dy;
    if (d < best) { best = d; bi = v; }
  }
  if (bi >= 0) bi = s_idx[bi];
  s_best[wv][lane] = best; s_bi[wv][lane] = bi;
  __syncthreads();
