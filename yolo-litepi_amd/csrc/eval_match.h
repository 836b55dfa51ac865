// The evaluator's matching rule (include/litepi.h, lp_eval_*): integer boxes, the IoU expression, the order
// among equal IoUs and the candidate test.  One definition for the host (lp_eval_match, eval_match_frame below) and the
// device (eval_kernel), in the manner of quality_measure.h and topk_select.h.  Host-pure: no HIP headers.
#pragma once
#include <limits.h>
#include <stdint.h>

#include <vector>

#include "../../include/litepi.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_EV_HD __host__ __device__
#else
#define LP_EV_HD
#endif

namespace lp {

#define LP_EVAL_COORD_MAX 536870912   // 2^29: differences stay within 2^30, areas within 2^60, their sum within 2^61

struct EvalBox { int32_t x1, y1, x2, y2; };

LP_EV_HD inline int32_t eval_clamp(int32_t v) { return v < -LP_EVAL_COORD_MAX ? -LP_EVAL_COORD_MAX : (v > LP_EVAL_COORD_MAX ? LP_EVAL_COORD_MAX : v); }
// truncation toward zero, as numpy's astype(int) of a coordinate that fits; a NaN gives 0
LP_EV_HD inline int32_t eval_trunc(float f) {
  if (!(f == f)) return 0;
  if (f <= (float)-LP_EVAL_COORD_MAX) return -LP_EVAL_COORD_MAX;
  if (f >= (float)LP_EVAL_COORD_MAX) return LP_EVAL_COORD_MAX;
  return (int32_t)f;
}
LP_EV_HD inline EvalBox eval_det_box(const lp_det& d) { return EvalBox{eval_trunc(d.x1), eval_trunc(d.y1), eval_trunc(d.x2), eval_trunc(d.y2)}; }
LP_EV_HD inline EvalBox eval_gt_box(const lp_gt& g) { return EvalBox{eval_clamp(g.x1), eval_clamp(g.y1), eval_clamp(g.x2), eval_clamp(g.y2)}; }

// _pairwise_iou on int64 arrays: one fp64 add, one correctly rounded fp64 division
LP_EV_HD inline double eval_iou(const EvalBox& p, const EvalBox& g) {
  const int64_t lx = p.x1 > g.x1 ? p.x1 : g.x1, ly = p.y1 > g.y1 ? p.y1 : g.y1;
  const int64_t rx = p.x2 < g.x2 ? p.x2 : g.x2, ry = p.y2 < g.y2 ? p.y2 : g.y2;
  const int64_t iw = rx - lx > 0 ? rx - lx : 0, ih = ry - ly > 0 ? ry - ly : 0;
  const int64_t inter = iw * ih;
  const int64_t area_p = ((int64_t)p.x2 - p.x1) * ((int64_t)p.y2 - p.y1), area_g = ((int64_t)g.x2 - g.x1) * ((int64_t)g.y2 - g.y1);
  return (double)inter / ((double)(area_p + area_g - inter) + 1e-7);
}

// the best ground truth of a record while walking g = 0, 1, ...: start with {-1, -inf}; `>=` lets the higher g win a tie
struct EvalBest { int gt; double iou; };
LP_EV_HD inline EvalBest eval_best_start() { return EvalBest{-1, -__builtin_huge_val()}; }
LP_EV_HD inline void eval_best_step(EvalBest& s, int g, double iou) {
  if (iou >= s.iou) { s.gt = g; s.iou = iou; }
}
// after the walk: no ground truth at all, or a best IoU of exactly 0, is "none" ({-1, 0})
LP_EV_HD inline EvalBest eval_best_end(const EvalBest& s) { return (s.gt < 0 || s.iou == 0.0) ? EvalBest{-1, 0.0} : s; }
LP_EV_HD inline bool eval_candidate(const EvalBest& s, double thr) { return s.gt >= 0 && s.iou >= thr; }

// the rule on one frame, the way the kernel runs it: pass 1 fills winner[g][j] with the lowest candidate, pass 2 forms the bits
inline void eval_match_frame(const lp_det* dets, int P, const lp_gt* gts, int G, const double* thr, int n_thr, lp_match_rec* out) {
  std::vector<int> winner((size_t)(G > 0 ? G : 0) * n_thr, INT_MAX);
  std::vector<EvalBest> best((size_t)(P > 0 ? P : 0));
  for (int p = 0; p < P; ++p) {
    const EvalBox pb = eval_det_box(dets[p]);
    EvalBest s = eval_best_start();
    for (int g = 0; g < G; ++g) eval_best_step(s, g, eval_iou(pb, eval_gt_box(gts[g])));
    s = best[p] = eval_best_end(s);
    for (int j = 0; j < n_thr; ++j)
      if (eval_candidate(s, thr[j]) && p < winner[(size_t)s.gt * n_thr + j]) winner[(size_t)s.gt * n_thr + j] = p;
  }
  for (int p = 0; p < P; ++p) {
    const EvalBest s = best[p];
    uint32_t correct = 0;
    if (s.gt >= 0 && dets[p].cls_class == gts[s.gt].cls)
      for (int j = 0; j < n_thr; ++j)
        if (winner[(size_t)s.gt * n_thr + j] == p) correct |= 1u << j;
    out[p].correct = correct; out[p].gt = s.gt; out[p].iou = s.iou;
  }
}

}  // namespace lp
