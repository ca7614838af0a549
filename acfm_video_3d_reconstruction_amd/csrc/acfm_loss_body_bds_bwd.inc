// FRAGMENT, no include guard: the boundary loss's backward for one mesh, included once in k_bds_loss_bwd and once in
// k_bds_loss_sel_bwd of acfm_loss.hip, on purpose: the two kernels differ only in how an entry's point is found, and
// the text is shared by inclusion like the forward's (acfm_loss_body_bds_search.inc; DESIGN.md, "The step's tail in
// one launch", the bullet "One text per kernel body").
//   expects: verts_xy, bds, argmin, gl, V, P, RB, gv, SEL (a constant expression) and sel, rows, S (read only under SEL)
//   leaves:  the mesh's gradient row gv[n][V][2] written, zeros included
  extern __shared__ float s_g[];  // [V][2]
  const int n = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < 2 * V; i += 256) s_g[i] = 0.f;
  __syncthreads();
  const float go = gl[n];
  const int E = SEL ? S : P;   // entries of a mesh in argmin
  for (int p0 = tid; p0 < E; p0 += 4 * 256) {      // four points per thread in flight
    int v[4];
    float bx[4], by[4], bm[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = min(p0 + u * 256, E - 1);
      v[u] = (p0 + u * 256 < E) ? argmin[(size_t)n * E + p] : -1;
      int s = p;
      if constexpr (SEL) {
        s = sel[(size_t)((n % RB) % rows) * S + p];
        if (s < 0 || s >= P) { s = 0; v[u] = -1; }   // an empty entry (its argmin is -1 already)
      }
      const float* b = bds + ((size_t)(n % RB) * P + s) * 3;
      bx[u] = b[0]; by[u] = b[1]; bm[u] = b[2];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float g = go * bm[u];
      if (v[u] < 0 || g == 0.f) continue;
      const float* x = verts_xy + ((size_t)n * V + v[u]) * 2;
      atomicAdd(&s_g[2 * v[u]], 2.0f * (x[0] - bx[u]) * g);
      atomicAdd(&s_g[2 * v[u] + 1], 2.0f * (x[1] - by[u]) * g);
    }
  }
  __syncthreads();
  float* o = gv + (size_t)n * V * 2;
  for (int i = tid; i < 2 * V; i += 256) o[i] = s_g[i];
