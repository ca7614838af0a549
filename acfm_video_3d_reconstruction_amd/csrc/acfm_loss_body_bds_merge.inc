// FRAGMENT, no include guard: the boundary loss's merge in wave 0, behind acfm_loss_body_bds_search.inc and the
// including function's return for the other waves; included once in k_bds_loss, k_bds_loss_sel and bds_block of
// acfm_loss.hip, on purpose, and shared by inclusion for the reason given in the search fragment (DESIGN.md, "The
// step's tail in one launch", the bullet "One text per kernel body").
//   expects: what the search fragment leaves, argmin, and contrib: a float the including function declares (a local of
//            the kernels, bds_block's reference parameter)
//   leaves:  argmin written for the lane's point; in contrib, in every lane of the wave, the workgroup's sum
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float d = s_best[w][lane];
    if (d < best) { best = d; bi = s_bi[w][lane]; }
  }
  contrib = 0.f;
  if constexpr (SEL) {
    if (p < S) {
      contrib = empty ? 0.f : best * bm;
      argmin[(size_t)n * S + p] = empty ? -1 : bi;
    }
  } else {
    if (p < P) {
      contrib = best * bm;
      argmin[(size_t)n * P + p] = bi;
    }
  }
  contrib = wave_sum(contrib);
