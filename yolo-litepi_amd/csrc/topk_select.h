// The top-k selection rule (include/litepi.h, lp_topk): classes ordered by probability descending, ties by class ascending.
// One definition of the order for the host (lp_topk_select) and the device (topk_select_kernel), in the manner of
// evidence_window.h: a 64-bit key per (probability, class) whose unsigned order IS the rule, and the round structure both
// sides run -- round j takes the largest key below round j - 1's winner.  Integer operations only: a probability's bits are
// moved, never computed with, so a denormal comes out as it went in.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_TK_HD __host__ __device__
#else
#define LP_TK_HD
#endif

namespace lp {

#define LP_TOPK_K_MAX 8   // LP_TOPK_MAX of include/litepi.h

// Value high, inverted class low.  The fp32 bit patterns are ordered as signed magnitudes (a softmax value is non-negative:
// its bits order as unsigned already, and the sign bit set on top keeps that order); 0 <= c < 2^31, so a key is never 0 and
// 0 can stand for "no class left".
LP_TK_HD inline uint64_t topk_key(uint32_t bits, int c) {
  const uint32_t v = (bits >> 31) ? ~bits : (bits | 0x80000000u);
  return ((uint64_t)v << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)c);
}
LP_TK_HD inline int topk_key_class(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }
LP_TK_HD inline uint32_t topk_key_bits(uint64_t key) {
  const uint32_t v = (uint32_t)(key >> 32);
  return (v >> 31) ? (v & 0x7FFFFFFFu) : ~v;
}
// the larger of two keys that lie below `below`; 0 when neither does
LP_TK_HD inline uint64_t topk_better(uint64_t best, uint64_t key, uint64_t below) { return (key < below && key > best) ? key : best; }

struct TopkRec { int32_t cls[LP_TOPK_K_MAX]; uint32_t prob_bits[LP_TOPK_K_MAX]; };   // lp_topk with the floats as their bits

// the rule on one distribution given as bit patterns: k rounds over the nc classes
LP_TK_HD inline void topk_select_bits(const uint32_t* bits, int nc, int k, TopkRec* out) {
  uint64_t below = ~0ull;
  for (int j = 0; j < LP_TOPK_K_MAX; ++j) {
    uint64_t best = 0;
    if (j < k && below != 0)
      for (int c = 0; c < nc; ++c) best = topk_better(best, topk_key(bits[c], c), below);
    if (best) {
      out->cls[j] = topk_key_class(best); out->prob_bits[j] = topk_key_bits(best);
    } else {
      out->cls[j] = -1; out->prob_bits[j] = 0u;
    }
    below = best;
  }
}

}  // namespace lp
