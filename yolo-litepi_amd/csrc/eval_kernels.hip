// Device-side evaluation (include/litepi.h, lp_eval_*): the records of a call against its ground truth.
// ONE WORKGROUP per frame.  The frame's ground truth (boxes as int4, classes) and the table winner[g][j] (int32, INT_MAX =
// nobody yet) live in LDS.  Pass 1: the lanes walk the frame's records in strides of the workgroup size; a record walks the
// ground truth in LDS (every lane reads the same word: a broadcast), keeps its best ground truth in registers and issues one
// LDS atomicMin(winner[best][j], p) per threshold it passes -- the minimum does not depend on the order of the atomics.
// Pass 2 behind a barrier: a record forms its best ground truth again (the same operations on the same words: the same
// bits; nothing per record is kept across the barrier, so max_det is bounded by nothing but the loop), reads its winners,
// and stores its lp_match_rec and its row, one 16-byte vector store each.
// Row order needs no atomics: a frame's first row is the log head at the start of the call plus the kept counts of the call's
// earlier frames (a wave-wide sum, B <= max_batch), and a one-thread launch behind the kernel advances head, dropped and the
// frame counter by the call's totals.  The class counters take global integer atomicAdd: integer adds commute.
#include <limits.h>

#include "common.h"
#include "eval_match.h"
#include "kernels.h"

namespace lp {

#define EVAL_THREADS 256

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int eval_kept(const EvalArgs& a, int b) { return min(max(a.counts[b], 0), a.max_det); }

__device__ __forceinline__ EvalBest eval_walk(const EvalBox& pb, const i32x4* s_box, int G) {
  EvalBest s = eval_best_start();
  for (int g = 0; g < G; ++g) {
    const i32x4 q = s_box[g];
    eval_best_step(s, g, eval_iou(pb, EvalBox{q.x, q.y, q.z, q.w}));
  }
  return eval_best_end(s);
}

__global__ __launch_bounds__(EVAL_THREADS) void eval_kernel(const EvalArgs a) {
  __shared__ i32x4 s_box[LP_EVAL_MAX_GT];
  __shared__ int s_cls[LP_EVAL_MAX_GT];
  __shared__ int s_winner[LP_EVAL_MAX_GT * LP_EVAL_MAX_THR];
  __shared__ double s_thr[LP_EVAL_MAX_THR];
  __shared__ long long s_first;
  const int b = blockIdx.x, t = threadIdx.x;
  const int n_thr = min(max(a.n_thr, 1), LP_EVAL_MAX_THR);
  const int G = min(max(a.frames[b].count, 0), LP_EVAL_MAX_GT);
  const int P = eval_kept(a, b);
  const lp_gt* gts = a.gts + a.frames[b].first;
  for (int g = t; g < G; g += EVAL_THREADS) {
    const lp_gt q = gts[g];
    const EvalBox gb = eval_gt_box(q);
    s_box[g] = i32x4{gb.x1, gb.y1, gb.x2, gb.y2};
    s_cls[g] = q.cls;
    if ((unsigned)q.cls < (unsigned)a.nc) atomicAdd(&a.gt_per_class[q.cls], 1);   // always true: lp_eval_device checked the class
  }
  for (int i = t; i < G * n_thr; i += EVAL_THREADS) s_winner[i] = INT_MAX;
  if (t < n_thr) s_thr[t] = a.thr[t];
  if (t < 64) {   // wave 0: the kept counts of the call's earlier frames
    long long sum = 0;
    for (int e = t; e < b; e += 64) sum += eval_kept(a, e);
#pragma unroll
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (t == 0) s_first = a.state->head + sum;
  }
  __syncthreads();

  const lp_det* dets = a.dets + (size_t)b * a.max_det;
  for (int p = t; p < P; p += EVAL_THREADS) {
    const EvalBest s = eval_walk(eval_det_box(dets[p]), s_box, G);
    if (s.gt >= 0)
      for (int j = 0; j < n_thr; ++j)
        if (eval_candidate(s, s_thr[j])) atomicMin(&s_winner[s.gt * n_thr + j], p);
  }
  __syncthreads();

  const long long first = s_first;
  const int frame = a.state->frames + b;
  for (int p = t; p < P; p += EVAL_THREADS) {
    const lp_det d = dets[p];
    const EvalBest s = eval_walk(eval_det_box(d), s_box, G);
    unsigned correct = 0;
    if (s.gt >= 0 && d.cls_class == s_cls[s.gt])
      for (int j = 0; j < n_thr; ++j)
        if (s_winner[s.gt * n_thr + j] == p) correct |= 1u << j;
    if (a.matches) {
      const unsigned long long iou_bits = (unsigned long long)__double_as_longlong(s.iou);
      reinterpret_cast<i32x4*>(a.matches + (size_t)b * a.max_det)[p] =
          i32x4{(int)correct, s.gt, (int)(unsigned)(iou_bits & 0xFFFFFFFFull), (int)(unsigned)(iou_bits >> 32)};
    }
    const long long pos = first + p;
    if (pos < (long long)a.max_rows)
      reinterpret_cast<i32x4*>(a.log)[pos] = i32x4{__float_as_int(d.det_conf), d.cls_class, (int)correct, frame};
  }
}

// behind eval_kernel in stream order: the next call's kernel reads what this leaves
__global__ void eval_advance_kernel(const EvalArgs a) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  long long total = 0;
  for (int b = 0; b < a.B; ++b) total += eval_kept(a, b);
  EvalState s = *a.state;
  const long long cap = a.max_rows, head = s.head + total;
  const long long over_old = s.head > cap ? s.head - cap : 0, over_new = head > cap ? head - cap : 0;
  s.head = head;
  s.dropped += over_new - over_old;
  s.frames += a.B;
  *a.state = s;
}

void launch_eval(const EvalArgs& a, hipStream_t st) {
  LP_CHECK(a.B >= 1 && a.max_det >= 1 && a.n_thr >= 1 && a.n_thr <= LP_EVAL_MAX_THR && a.max_rows >= 1, LP_ERR_ARG, "bad evaluator shape");
  LP_LAUNCH(eval_kernel, dim3(a.B), dim3(EVAL_THREADS), 0, st, a);
  LP_HIP(hipGetLastError());
  LP_LAUNCH(eval_advance_kernel, dim3(1), dim3(64), 0, st, a);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
