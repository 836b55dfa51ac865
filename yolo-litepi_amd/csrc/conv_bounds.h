// Address choices of the conv kernels that a host program can replay (tests/native/conv_epilogue_bounds.cpp).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_HD __host__ __device__
#else
#define LP_HD
#endif

namespace lp {

// conv3x3_mfma_kernel, epilogue_tile: the column of the pixel the residual prefetch of a strip is based on.  A strip's five
// patches start at columns oxb, oxb + 4, .., oxb + 16; a patch right of the image reads the base pixel instead (its quads are
// discarded).  A strip that starts right of the image itself (a 40-column tile on a map narrower than 20 columns puts the
// second wave's strip at columns 20..23) has no patch inside: its base is the row's first pixel, which always exists.
LP_HD inline int residual_base_col(int oxb, int Wout) { return oxb < Wout ? oxb : 0; }

// the column patch p (0..4) of that strip reads its residual from
LP_HD inline int residual_patch_col(int oxb, int p, int Wout) {
  return residual_base_col(oxb, Wout) + (oxb + p * 4 < Wout ? p * 4 : 0);
}

}  // namespace lp
