// Mapped views (include/litepi.h "mapped views"): a view whose pixels come through a per-pixel remap table and whose boxes go
// back to the frame through the same table.  Three rules, one definition for the host (lp_map_fixed, lp_map_render, lp_map_box),
// the device (map_views_kernel, map_candidates_kernel; map_kernels.hip) and tests/native/map_rule_check.cpp, in the manner of
// evidence_window.h, topk_select.h and quality_measure.h.
//   Table: the caller's float positions, fixed once in doubles to int32 with 5 fractional bits (round half to even).
//   Pixel: a bilinear blend of four taps in int32 with 5-bit weights, 114 outside the frame.  This is the project's OWN rule:
//          it is not cv2.remap's weight table (cv2 also keeps 5 fractional bits, but blends with a table of 15-bit weights and
//          treats the border its own way), just as the P010 path truncates where a converter would round.  A table built for
//          cv2.remap shows the same picture, not the same bytes.
//   Box:   fp32, every operation rounded on its own, nothing contracted: eight points of the view box go through the bilinear
//          interpolation of the table (linear extrapolation beyond the border pixels' centres); their bounding box, clipped to
//          the frame, is the frame box.
// No function here reads a byte outside [frame, frame + H * W * 3) or an entry outside the table's S * S * 2.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_VM_HD __host__ __device__
#else
#define LP_VM_HD
#endif

namespace lp {

#define LP_MAP_FRAC_BITS 5
#define LP_MAP_ONE 32          // 1 << LP_MAP_FRAC_BITS
#define LP_MAP_SIDE_MAX 16384  // frame sides: a fixed coordinate then has at most 20 significant bits
#define LP_MAP_BORDER 114

// ---- table ---------------------------------------------------------------------------------------------------------------------
// one coordinate along an axis of L pixels: (int32)rint(min(max((double)v, -2), L + 1) * 32); false for a NaN
LP_VM_HD inline bool vm_fix(float v, int L, int32_t* out) {
  if (v != v) return false;
  double d = (double)v;
  d = d > -2.0 ? d : -2.0;
  d = d < (double)L + 1.0 ? d : (double)L + 1.0;
  *out = (int32_t)rint(d * 32.0);
  return true;
}

// ---- pixel ---------------------------------------------------------------------------------------------------------------------
// channel ch of P(r, c): the frame's pixel, 114 outside; a tap outside is not fetched
LP_VM_HD inline int vm_tap(const uint8_t* frame, int H, int W, int r, int c, int ch) {
  return (r >= 0 && r < H && c >= 0 && c < W) ? (int)frame[((long)r * W + c) * 3 + ch] : LP_MAP_BORDER;
}

// the view pixel whose table entry is (fx, fy), BGR into out[0..2]
LP_VM_HD inline void vm_pixel(const uint8_t* frame, int H, int W, int32_t fx, int32_t fy, uint8_t* out) {
  const int ix = fx >> LP_MAP_FRAC_BITS, ax = fx & (LP_MAP_ONE - 1);
  const int iy = fy >> LP_MAP_FRAC_BITS, ay = fy & (LP_MAP_ONE - 1);
  const int w00 = (LP_MAP_ONE - ax) * (LP_MAP_ONE - ay), w01 = ax * (LP_MAP_ONE - ay), w10 = (LP_MAP_ONE - ax) * ay, w11 = ax * ay;
  for (int ch = 0; ch < 3; ++ch) {
    const int v = vm_tap(frame, H, W, iy, ix, ch) * w00 + vm_tap(frame, H, W, iy, ix + 1, ch) * w01 +
                  vm_tap(frame, H, W, iy + 1, ix, ch) * w10 + vm_tap(frame, H, W, iy + 1, ix + 1, ch) * w11 + 512;
    out[ch] = (uint8_t)(v >> 10);
  }
}

// ---- box -----------------------------------------------------------------------------------------------------------------------
// fminf / fmaxf return the non-NaN operand: written out, so that host and device agree whatever the library does
LP_VM_HD inline float vm_max(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
LP_VM_HD inline float vm_min(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }

// one axis of a sample point: t = u - 0.5, cell i = min(max((int)floorf(t), 0), S - 2), fraction f = t - i (outside [0, 1]
// beyond the border pixels' centres: the extrapolation)
LP_VM_HD inline void vm_cell(float u, int S, int* i, float* f) {
#pragma clang fp contract(off)
  const float t = u - 0.5f;
  const float fl = floorf(t);
  const float hi = (float)(S - 2);
  *i = !(fl >= 0.f) ? 0 : (fl > hi ? S - 2 : (int)fl);   // the clamp in front of the conversion: the same value, defined for any t
  *f = t - (float)*i;
}

// component comp (0: x, 1: y) of the frame position of view point (u, v)
LP_VM_HD inline float vm_point(const int32_t* fixed, int S, int comp, float u, float v) {
#pragma clang fp contract(off)
  int i, j;
  float fu, fv;
  vm_cell(u, S, &i, &fu);
  vm_cell(v, S, &j, &fv);
  const int32_t* p = fixed + ((long)j * S + i) * 2 + comp;
  const float x00 = (float)p[0] * 0.03125f, x01 = (float)p[2] * 0.03125f;
  const float x10 = (float)p[2 * S] * 0.03125f, x11 = (float)p[2 * S + 2] * 0.03125f;
  const float d0 = x01 - x00;
  const float m0 = fu * d0;
  const float top = x00 + m0;
  const float d1 = x11 - x10;
  const float m1 = fu * d1;
  const float bot = x10 + m1;
  const float d2 = bot - top;
  const float m2 = fv * d2;
  const float s = top + m2;
  return s + 0.5f;
}

// the frame box of view box {x1, y1, x2, y2}: the bounding box of the four corners and the four edge midpoints, clipped to
// [0, W] x [0, H]
LP_VM_HD inline void vm_box(const int32_t* fixed, int S, int H, int W, const float* box, float* out) {
#pragma clang fp contract(off)
  const float x1 = box[0], y1 = box[1], x2 = box[2], y2 = box[3];
  const float sx = x1 + x2, sy = y1 + y2;
  const float xm = sx * 0.5f, ym = sy * 0.5f;
  const float us[8] = {x1, xm, x2, x1, x2, x1, xm, x2};
  const float vs[8] = {y1, y1, y1, ym, ym, y2, y2, y2};
  float lox = 0.f, loy = 0.f, hix = 0.f, hiy = 0.f;
  for (int k = 0; k < 8; ++k) {
    const float px = vm_point(fixed, S, 0, us[k], vs[k]), py = vm_point(fixed, S, 1, us[k], vs[k]);
    lox = k == 0 ? px : vm_min(lox, px);
    loy = k == 0 ? py : vm_min(loy, py);
    hix = k == 0 ? px : vm_max(hix, px);
    hiy = k == 0 ? py : vm_max(hiy, py);
  }
  out[0] = vm_min(vm_max(lox, 0.f), (float)W);
  out[1] = vm_min(vm_max(loy, 0.f), (float)H);
  out[2] = vm_min(vm_max(hix, 0.f), (float)W);
  out[3] = vm_min(vm_max(hiy, 0.f), (float)H);
}

}  // namespace lp
