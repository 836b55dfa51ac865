// Device core of the ShuffleNetV2 classifier kernels, defined once: the vector types, the pointwise-GEMM helpers over A fragments
// from L2 and NHWC images in LDS, the conv5 epilogue, the fc tile and the softmax / arg-max / scatter tail.  Included by
// cls_net.hip (cls_front, cls_back), cls_fused.hip (shuffle_stage_fused, cls_head_fused) and cls_kernels.hip (softmax_argmax).
// A record's cls_conf is bit-equal to classify() of the same crop on every path because all of them end in cls_tail_row below.
#pragma once
#include "cls_fused.h"
#include "cls_plan.h"

namespace lp {

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ---- pointwise GEMM: D[out-channel][pixel] = W . X -------------------------------------------------------------------
// fragments of tile t (S K steps of pack_fused_pw's [tile][step][lane][16 B]) -> registers; steps past S read as zero
template <int SMAX>
__device__ __forceinline__ void wload(u32x4 (&af)[SMAX], const u32x4_t* __restrict__ w, int t, int S, int lane) {
#pragma unroll
  for (int s = 0; s < SMAX; ++s) {
    af[s] = u32x4{0u, 0u, 0u, 0u};
    if (s < S) af[s] = w[((size_t)t * S + s) * 64 + lane];
  }
}

// acc[p] (+)= W(tile) . X[pixels p0 + 16p .. +15]: K steps s0 .. s0+SMAX-1 of the fragments in af; Kp = physical
// channels of the LDS rows (K groups past it are row padding / the next row: never read)
template <int SMAX, int PT>
__device__ __forceinline__ void gemm_acc(const u32x4 (&af)[SMAX], int S, int s0, const char* bsrc, int brow, int Kp, int p0, int lane,
                                         floatx4 (&acc)[PT]) {
  const int g = lane >> 4, col = lane & 15;
#pragma unroll
  for (int s = 0; s < SMAX; ++s) {
    if (s < S) {
      const half8 a = __builtin_bit_cast(half8, af[s]);
      const int kg = 4 * (s0 + s) + g;
#pragma unroll
      for (int p = 0; p < PT; ++p) {
        u32x4 v = u32x4{0u, 0u, 0u, 0u};
        if (kg * 8 < Kp) v = *reinterpret_cast<const u32x4*>(bsrc + (p0 + p * 16 + col) * brow + kg * 16);
        acc[p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(half8, v), acc[p], 0, 0, 0);
      }
    }
  }
}

template <int PT> __device__ __forceinline__ void zero_acc(floatx4 (&acc)[PT]) {
#pragma unroll
  for (int p = 0; p < PT; ++p) acc[p] = floatx4{0.f, 0.f, 0.f, 0.f};
}

// relu(acc + bias) of tile t -> fp16 LDS image dst[pixel][channel]
template <int PT>
__device__ __forceinline__ void store_relu(char* dst, int drow, int p0, int t, const float* __restrict__ bias, const floatx4 (&acc)[PT],
                                           int lane) {
  const int g = lane >> 4, col = lane & 15;
  const int ch0 = t * 16 + 4 * g;
  const floatx4 b = *reinterpret_cast<const floatx4*>(bias + ch0);
#pragma unroll
  for (int p = 0; p < PT; ++p) {
    half4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = (half_t)fmaxf(acc[p][i] + b[i], 0.f);
    *reinterpret_cast<half4*>(dst + (p0 + p * 16 + col) * drow + ch0 * 2) = q;
  }
}

// channel_shuffle(cat(a, b), 2): logical channel 2c = a[c], 2c+1 = b[c]; each half of the stage tensor is padded to bfp
__device__ __forceinline__ int shuffle_phys(int l, int bf, int bfp) { return l < bf ? l : bfp + (l - bf); }

// ---- conv5's epilogue: relu(acc + bias) of output tile t, mean over the 2x2 map, fp16 -> Mn[roi][1024] -----------------
// ROIS ROIs per pass = ROIS / 4 pixel tiles; pixels 4r..4r+3 of ROI r sit on 4 adjacent lanes
template <int ROIS>
__device__ __forceinline__ void conv5_mean_store(char* Mn, int t, const float* b5, const floatx4 (&acc)[ROIS / 4], int lane) {
  const int g = lane >> 4, col = lane & 15;
  const int ch0 = t * 16 + 4 * g;
  const floatx4 bias = *reinterpret_cast<const floatx4*>(b5 + ch0);
#pragma unroll
  for (int p = 0; p < ROIS / 4; ++p) {
    half4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float v = fmaxf(acc[p][i] + bias[i], 0.f);
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      q[i] = (half_t)(v * 0.25f);
    }
    if ((col & 3) == 0) *reinterpret_cast<half4*>(Mn + (p * 4 + (col >> 2)) * clsplan::kMeanRow + ch0 * 2) = q;
  }
}

// ---- fc: logits[roi][16 classes of tile t] = Wfc . mean + b -> LG[roi][nc_p]; 32 K steps in four chunks of 8 fragments ------
template <int ROIS>
__device__ __forceinline__ void fc_tile(float* LG, const char* Mn, const u32x4_t* wfc, const float* bfc, int nc_p,
                                        int t, int lane) {
  const int g = lane >> 4, col = lane & 15;
  floatx4 acc = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int s0 = 0; s0 < 32; s0 += 8) {
    u32x4 af[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) af[u] = wfc[((size_t)t * 32 + s0 + u) * 64 + lane];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (ROIS >= 16 || col < ROIS) v = *reinterpret_cast<const u32x4*>(Mn + col * clsplan::kMeanRow + (4 * (s0 + u) + g) * 16);
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8, af[u]), __builtin_bit_cast(half8, v), acc, 0, 0, 0);
    }
  }
  const int c0 = t * 16 + 4 * g;
  if (ROIS >= 16 || col < ROIS) {
#pragma unroll
    for (int i = 0; i < 4; ++i) LG[col * nc_p + c0 + i] = acc[i] + bfc[c0 + i];
  }
}

// ---- softmax(dim=1) + arg-max (e2e.py:394-396) of ROI r's logits row l, by one wave (classes strided over lanes); lane 0
// writes the id, the confidence and the detection record (e2e.py:525-526).  Every output is optional.
__device__ __forceinline__ void cls_tail_row(const float* l, int nc, int r, int lane, float* probs, int* ids, float* conf, lp_det* dets,
                                             int max_det, const int* roi_img, const int* roi_slot) {
  float mx = -INFINITY;
  for (int c = lane; c < nc; c += 64) mx = fmaxf(mx, l[c]);
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.f;
  for (int c = lane; c < nc; c += 64) sum += expf(l[c] - mx);
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  float best = -1.f;
  int best_c = 0x7fffffff;
  for (int c = lane; c < nc; c += 64) {
    const float pr = expf(l[c] - mx) / sum;
    if (probs) probs[(long)r * nc + c] = pr;
    if (pr > best) { best = pr; best_c = c; }  // first maximum within the lane (ascending c)
  }
  for (int o = 32; o > 0; o >>= 1) {  // first maximum across lanes: larger p, then smaller class index
    const float ob = __shfl_xor(best, o);
    const int oc = __shfl_xor(best_c, o);
    if (ob > best || (ob == best && oc < best_c)) { best = ob; best_c = oc; }
  }
  if (lane == 0) {
    if (ids) ids[r] = best_c;
    if (conf) conf[r] = best;
    if (dets) {
      lp_det* d = dets + (long)roi_img[r] * max_det + roi_slot[r];
      d->cls_class = best_c;
      d->cls_conf = best;
    }
  }
}

// the tail of the fused kernels: ROI r's row of the logits image in LDS -> the output block, and the logits themselves
__device__ __forceinline__ void cls_tail(const float* l, int r, int lane, const ClsOut& o) {
  cls_tail_row(l, o.nc, r, lane, o.probs, o.ids, nullptr, o.dets, o.max_det, o.roi_img, o.roi_slot);
  if (o.logits)
    for (int c = lane; c < o.nc; c += 64) o.logits[(long)r * o.logits_pitch + c] = l[c];
}

}  // namespace lp
