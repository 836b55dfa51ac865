// The evidence store's arithmetic (include/litepi.h, lp_evidence_config): the window of a best sighting and the letterbox
// geometry of that window inside the E x E picture.  One definition for the host (lp_evidence_window, lp_view_geometry's
// numbers) and the device (inventory_evidence_kernel decides the window, evidence_pictures_kernel resamples it), in the
// manner of conv_bounds.h and surface_plan.h.  Window: fp32, every operation rounded on its own, nothing contracted; the
// geometry: doubles, as make_geom computes it (pipeline.cpp).
#pragma once
#include <math.h>

#include "letterbox_core.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_EW_HD __host__ __device__
#else
#define LP_EW_HD
#endif

namespace lp {

#define LP_EVIDENCE_SIDE_MIN 16
#define LP_EVIDENCE_SIDE_MAX 16384

struct EvWindow { int x, y, w, h; };

// fmaxf / fminf return the non-NaN operand: written out, so that host and device agree whatever the library does
LP_EW_HD inline float ew_max(float a, float b) { return a != a ? b : (b != b ? a : (a > b ? a : b)); }
LP_EW_HD inline float ew_min(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? a : b)); }
LP_EW_HD inline int ew_imin(int a, int b) { return a < b ? a : b; }
LP_EW_HD inline int ew_imax(int a, int b) { return a > b ? a : b; }

// the centre of one axis: (int)fminf(fmaxf(floorf((a + b) * 0.5f), 0), L)
LP_EW_HD inline int ew_centre(float a, float b, int L) {
#pragma clang fp contract(off)
  const float s = a + b;
  const float m = s * 0.5f;
  return (int)ew_min(ew_max(floorf(m), 0.f), (float)L);
}

// the window of box {x1, y1, x2, y2} on an H x W frame; false (and a zero window) when the sighting gets no picture
LP_EW_HD inline bool evidence_window(float scale, int H, int W, float x1, float y1, float x2, float y2, EvWindow* win) {
#pragma clang fp contract(off)
  win->x = win->y = win->w = win->h = 0;
  const float bw = x2 - x1, bh = y2 - y1;
  if (!(H >= 16 && W >= 16 && bw > 0.f && bh > 0.f)) return false;   // false for a NaN
  const float m = ew_max(bw, bh);
  const float want = scale * m;
  const int side = (int)ew_min(ew_max(ceilf(want), (float)LP_EVIDENCE_SIDE_MIN), (float)LP_EVIDENCE_SIDE_MAX);
  const int w = ew_imin(side, W), h = ew_imin(side, H);
  const int cx = ew_centre(x1, x2, W), cy = ew_centre(y1, y2, H);
  win->x = ew_imin(ew_imax(cx - w / 2, 0), W - w);
  win->y = ew_imin(ew_imax(cy - h / 2, 0), H - h);
  win->w = w; win->h = h;
  return true;
}

// letterbox of a h x w window into E x E: make_geom(h, w, E, E)'s new size and integer borders (round half to even), as
// the placement the letterbox core resamples into
LP_EW_HD inline LbPlace evidence_geom(int h, int w, int E) {
  const double rh = (double)E / h, rw = (double)E / w;
  const double r = rh < rw ? rh : rw;
  LbPlace g;
  g.new_w = (int)rint(w * r); g.new_h = (int)rint(h * r);
  const double dw = (E - g.new_w) / 2.0, dh = (E - g.new_h) / 2.0;
  g.top = (int)rint(dh - 0.1); g.left = (int)rint(dw - 0.1);
  return g;
}

}  // namespace lp
