// Device-side pieces of the detector post-processing shared by post_kernels.hip (stand-alone decode) and
// head_kernels.hip (decode fused into the Detect-head kernel).
#pragma once
#include "common.h"
#include "kernels.h"

namespace lp {

// ------------------------------------------------------------------------------------
// conf filter + xywh->xyxy + un-letterbox + clip for one anchor (e2e.py:255-278)
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void emit_candidate(float cx, float cy, float w, float h, float score, int cls, int anchor,
                                               const ImgGeom& gm, float conf, Cand* cand, int* count) {
  if (!(score > conf)) return;
  const float hw = __fmul_rn(w, 0.5f), hh = __fmul_rn(h, 0.5f);  // w / 2 (exact either way)
  float x1 = __fsub_rn(cx, hw), y1 = __fsub_rn(cy, hh);
  float x2 = __fadd_rn(cx, hw), y2 = __fadd_rn(cy, hh);
  x1 = __fdiv_rn(__fsub_rn(x1, gm.pad_w), gm.ratio);
  x2 = __fdiv_rn(__fsub_rn(x2, gm.pad_w), gm.ratio);
  y1 = __fdiv_rn(__fsub_rn(y1, gm.pad_h), gm.ratio);
  y2 = __fdiv_rn(__fsub_rn(y2, gm.pad_h), gm.ratio);
  const float W = (float)gm.w, H = (float)gm.h;
  x1 = fminf(fmaxf(x1, 0.f), W); x2 = fminf(fmaxf(x2, 0.f), W);
  y1 = fminf(fmaxf(y1, 0.f), H); y2 = fminf(fmaxf(y2, 0.f), H);
  const int slot = atomicAdd(count, 1);
  Cand c;
  c.x1 = x1; c.y1 = y1; c.x2 = x2; c.y2 = y2; c.score = score; c.cls = cls; c.anchor = anchor; c.pad = 0;
  cand[slot] = c;
}

// ------------------------------------------------------------------------------------
// One axis of cv2.resize(INTER_LINEAR) on uint8: source index and the 11-bit coefficient pair of destination index d
// (OpenCV's published fixed-point algorithm: half-pixel centres, cvRound(f * 2048)).  Used by the letterbox kernel
// (e2e.py:80) and by the ROI resize of the e2e_optimize numerics (e2e_optimize.py:388-390).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void lin_coeff(int d, int dst, int src, int& s0, int& a0, int& a1) {
  const double inv_scale = (double)dst / (double)src;
  const double scale = 1.0 / inv_scale;
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  s0 = s;
  a1 = __float2int_rn(f * 2048.f);
  a0 = __float2int_rn((1.f - f) * 2048.f);
}

// ------------------------------------------------------------------------------------
// Pieces of the per-class greedy NMS shared by nms_kernel (post_kernels.hip) and the frame NMS of tiled
// inference (tile_kernels.hip)
// ------------------------------------------------------------------------------------
#define NMS_THREADS 1024

__device__ __forceinline__ unsigned long long nms_key(const Cand& c) {
  return ((unsigned long long)(0xFFFFu - (unsigned)c.cls) << 46) | ((unsigned long long)__float_as_uint(c.score) << 14) |
         (unsigned long long)(c.anchor & 0x3FFF);
}
// score-major key of a kept box (global top-max_det selection): unique per image
__device__ __forceinline__ unsigned long long nms_score_key(const Cand& c) {
  return ((unsigned long long)__float_as_uint(c.score) << 14) | (unsigned long long)(c.anchor & 0x3FFF);
}
// true when box j (area aj) is suppressed by kept box i (area ai): NOT (iou <= thr), e2e.py:116
__device__ __forceinline__ bool nms_suppressed(float ix1, float iy1, float ix2, float iy2, float ai, float jx1, float jy1, float jx2,
                                               float jy2, float thr) {
  const float aj = __fmul_rn(__fsub_rn(jx2, jx1), __fsub_rn(jy2, jy1));
  const float w = fmaxf(0.f, __fsub_rn(fminf(ix2, jx2), fmaxf(ix1, jx1)));
  const float h = fmaxf(0.f, __fsub_rn(fminf(iy2, jy2), fmaxf(iy1, jy1)));
  const float inter = __fmul_rn(w, h);
  const float iou = __fdiv_rn(inter, __fadd_rn(__fsub_rn(__fadd_rn(ai, aj), inter), 1e-6f));
  return !(iou <= thr);
}
// the match of the frame NMS of views (lp_set_view_merge): IOS = false is nms_suppressed itself; IOS = true divides by the
// smaller of the two areas, so a box cut by a view border matches the whole box it lies in
template <bool IOS>
__device__ __forceinline__ bool view_matched(float ix1, float iy1, float ix2, float iy2, float ai, float jx1, float jy1, float jx2,
                                             float jy2, float thr) {
  if (!IOS) return nms_suppressed(ix1, iy1, ix2, iy2, ai, jx1, jy1, jx2, jy2, thr);
  const float aj = __fmul_rn(__fsub_rn(jx2, jx1), __fsub_rn(jy2, jy1));
  const float w = fmaxf(0.f, __fsub_rn(fminf(ix2, jx2), fmaxf(ix1, jx1)));
  const float h = fmaxf(0.f, __fsub_rn(fminf(iy2, jy2), fmaxf(iy1, jy1)));
  const float inter = __fmul_rn(w, h);
  const float ios = __fdiv_rn(inter, __fadd_rn(fminf(ai, aj), 1e-6f));
  return !(ios <= thr);
}
// min / max of the 64 lanes' values, in every lane (float min and max commute: the order of the steps does not show)
__device__ __forceinline__ float wave_min(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// LDS atomic min / max of floats through their bit patterns: a non-negative float orders like its int pattern, a negative
// one like its unsigned pattern reversed, so either sign is exact (no NaN: candidates are clipped coordinates)
__device__ __forceinline__ void lds_min_f32(float* p, float v) {
  if (v >= 0.f) atomicMin(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void lds_max_f32(float* p, float v) {
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}

// exclusive prefix sum of one int per thread over the workgroup (NMS_THREADS = 16 waves); returns the total via *total
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_wave /*[17]*/, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  if (wave == 0) {
    int w = lane < NMS_THREADS / 64 ? s_wave[lane] : 0;
    int winc = w;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const int t = __shfl_up(winc, o);
      if (lane >= o) winc += t;
    }
    if (lane < NMS_THREADS / 64) s_wave[lane] = winc - w;
    if (lane == NMS_THREADS / 64 - 1) s_wave[NMS_THREADS / 64] = winc;
  }
  __syncthreads();
  const int r = s_wave[wave] + inc - v;
  *total = s_wave[NMS_THREADS / 64];
  __syncthreads();  // s_wave may be reused
  return r;
}

// ROI rectangle of a kept box (int truncation + clip) and the area filter.  rule 0 = HybridPipeline.run, e2e.py:465-473:
// x1 in [0, w-1], y1 in [0, h-1], x2 in [x1+1, w], y2 in [y1+1, h]; rule 1 = HybridPipelineOptimized.run,
// e2e_optimize.py:480-497: all four clipped to [0, w] / [0, h], empty rectangles dropped.  min_area < 0: no filter.
__device__ __forceinline__ bool roi_rect(const Cand& c, const ImgGeom& gm, int rule, int min_area, int& x1, int& y1, int& x2, int& y2) {
  x1 = (int)c.x1; y1 = (int)c.y1; x2 = (int)c.x2; y2 = (int)c.y2;
  if (rule == 0) {
    x1 = min(max(x1, 0), gm.w - 1); y1 = min(max(y1, 0), gm.h - 1);
    x2 = min(max(x2, x1 + 1), gm.w); y2 = min(max(y2, y1 + 1), gm.h);
  } else {
    x1 = min(max(x1, 0), gm.w); x2 = min(max(x2, 0), gm.w);
    y1 = min(max(y1, 0), gm.h); y2 = min(max(y2, 0), gm.h);
  }
  return min_area < 0 || (((x2 - x1) * (y2 - y1) >= min_area) && x2 > x1 && y2 > y1);
}

}  // namespace lp
