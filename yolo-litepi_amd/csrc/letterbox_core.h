// The letterbox resample: cv2's INTER_LINEAR letterbox of a window of a BGR frame, 114 in the bars (DESIGN.md "Letterbox
// core").  One statement for the device -- letterbox_kernel / letterbox_tiled_kernel (misc_kernels.hip), window_views_kernel /
// window_views_pixel_kernel (tile_kernels.hip), evidence_pictures_kernel (evidence_kernels.hip), and the blend of
// rr_strip_linear (post_kernels.hip) -- and for the host, where tests/native/letterbox_core_check.cpp plays a workgroup
// through it under sanitizers; in the manner of topk_select.h and evidence_window.h.
//
// Staged form: a workgroup owns LB_TH output rows; for each of them the TWO window rows the vertical interpolation reads are
// staged in LDS with aligned 16-byte loads over the byte span [b0, b1) the workgroup's columns read, then a thread resamples
// four adjacent output pixels into three dwords.  Per-pixel form: the same resample with the rows read where they lie.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define LP_LB_HD __host__ __device__ __forceinline__
#else
#define LP_LB_HD inline
#endif
#if defined(__clang__)
#define LP_LB_UNROLL _Pragma("unroll")
#else
#define LP_LB_UNROLL
#endif

namespace lp {

#define LB_TH 8            // output rows of a workgroup (tile or band)
#define LB_TW 128          // output columns of a tile
#define EV_ROW_CAP 2048    // bytes of a staged row of the evidence pictures: 2 * LB_TH rows = 32 KB of static LDS

typedef uint32_t lb_u32x4 __attribute__((vector_size(16)));

struct LbSource {          // one window of one frame
  const uint8_t* im;       // the frame's first byte
  long frame_bytes;        // rows * pitch
  int pitch, x, y, w, h;   // frame row bytes; the window in frame pixels
};
struct LbPlace { int new_w, new_h, top, left; };   // the resized window inside the output picture

LP_LB_HD int lb_min(int a, int b) { return a < b ? a : b; }
LP_LB_HD int lb_max(int a, int b) { return a > b ? a : b; }
LP_LB_HD int lb_rint(float f) {   // round to nearest even
#if defined(__HIP_DEVICE_COMPILE__)
  return __float2int_rn(f);
#else
  return (int)lrintf(f);
#endif
}

// One axis of cv2.resize(INTER_LINEAR) on uint8: source index and the 11-bit coefficient pair of destination index d
// (OpenCV's published fixed-point algorithm: half-pixel centres, cvRound(f * 2048)).  e2e.py:80, e2e_optimize.py:388-390.
// The axis' scale apart (two double divisions): the four pixels of a thread share their x axis' scale.
LP_LB_HD double lin_scale(int dst, int src) {
  const double inv_scale = (double)dst / (double)src;
  return 1.0 / inv_scale;
}
LP_LB_HD void lin_coeff(int d, double scale, int src, int& s0, int& a0, int& a1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; }
  s0 = s;
  a1 = lb_rint(f * 2048.f);
  a0 = lb_rint((1.f - f) * 2048.f);
}
LP_LB_HD void lin_coeff(int d, int dst, int src, int& s0, int& a0, int& a1) { lin_coeff(d, lin_scale(dst, src), src, s0, a0, a1); }

// the four-tap blend: taps t<row><column>, int horizontal pass, cv2's vertical pass, clamped to a byte
LP_LB_HD int lin_blend(int t00, int t01, int t10, int t11, int ax0, int ax1, int ay0, int ay1) {
  const int h0 = t00 * ax0 + t01 * ax1;
  const int h1 = t10 * ax0 + t11 * ax1;
  const int v = (((ay0 * (h0 >> 4)) >> 16) + ((ay1 * (h1 >> 4)) >> 16) + 2) >> 2;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

LP_LB_HD bool lb_resizes(const LbSource& s, const LbPlace& g) { return !(g.new_w == s.w && g.new_h == s.h); }

// the byte span [b0, b1) of a WINDOW row that columns [dxa, dxb) of the resized window read (dxa < dxb)
struct LbSpan { int b0, b1; };
LP_LB_HD LbSpan lb_span(const LbSource& s, const LbPlace& g, bool resize, int dxa, int dxb) {
  int sa = dxa, sb = dxb - 1, t0, t1;
  if (resize) { lin_coeff(dxa, g.new_w, s.w, sa, t0, t1); lin_coeff(dxb - 1, g.new_w, s.w, sb, t0, t1); }
  return LbSpan{3 * sa, 3 * (lb_min(sb + 1, s.w - 1) + 1)};
}

// output row oy: whether it lies in the resized window, the two window rows it reads and their weights
struct LbRowCoef { bool in; int sy, sy1, ay0, ay1; };
LP_LB_HD LbRowCoef lb_row_coef(const LbSource& s, const LbPlace& g, bool resize, int oy) {
  const int dy = oy - g.top;
  LbRowCoef rc{dy >= 0 && dy < g.new_h, 0, 0, 2048, 0};
  if (rc.in) { if (resize) lin_coeff(dy, g.new_h, s.h, rc.sy, rc.ay0, rc.ay1); else rc.sy = dy; }
  rc.sy1 = lb_min(rc.sy + 1, s.h - 1);
  return rc;
}

// The frame's bytes, by offset from its first byte.  The check substitutes a frame that counts what is asked of it.
struct LbFrame {
  const uint8_t* im;
  LP_LB_HD lb_u32x4 load16(long o) const { return *reinterpret_cast<const lb_u32x4*>(im + o); }
  LP_LB_HD uint32_t operator[](long o) const { return im[o]; }
};

// Staging of LDS row r (2j / 2j+1 = the window rows sy / sy1 of output row oy0 + j), the part of one of the 16 threads
// (lane16) of that row; `row` is the row's first byte, row_cap its bytes.  Returns the byte index of window byte b0 inside the
// row, or -1 for a row outside the resized window (nothing is staged).  The aligned start is taken from the address itself; a
// chunk that lies wholly inside [im, im + frame_bytes) is one aligned 16-byte load, any other is assembled byte by byte into
// four dwords (no local byte array), and no byte outside the frame is read.  The chunk index is bounded by the row capacity
// (the launcher sized row_cap for the span: the bound never cuts).
template <class Frame>
LP_LB_HD int lb_stage_row(const Frame& fr, const LbSource& s, const LbPlace& g, bool resize, LbSpan sp, int oy0, int r, uint8_t* row,
                          int row_cap, int lane16) {
  const LbRowCoef rc = lb_row_coef(s, g, resize, oy0 + (r >> 1));
  if (!rc.in) return -1;
  const long goff = (long)(s.y + ((r & 1) ? rc.sy1 : rc.sy)) * s.pitch + 3L * s.x + sp.b0;   // byte offset of the span inside the frame
  const int shift = (int)(reinterpret_cast<uintptr_t>(s.im + goff) & 15);
  const long gal = goff - shift;                                                              // 16-byte aligned start, relative to the frame
  const int nchunk = lb_min((shift + (sp.b1 - sp.b0) + 15) >> 4, row_cap >> 4);
  for (int c = lane16; c < nchunk; c += 16) {
    const long o = gal + 16L * c;
    lb_u32x4 v;
    if (o >= 0 && o + 16 <= s.frame_bytes) {
      v = fr.load16(o);
    } else {   // the chunk passes the frame's first or last byte
      v = lb_u32x4{0u, 0u, 0u, 0u};
LP_LB_UNROLL
      for (int k = 0; k < 16; ++k)
        if (o + k >= 0 && o + k < s.frame_bytes) v[k >> 2] |= fr[o + k] << (8 * (k & 3));
    }
    *reinterpret_cast<lb_u32x4*>(row + 16 * c) = v;
  }
  return shift;
}

// A window row behind a byte accessor: window byte b is p[off + b].  Staged: p is the LDS row and off = shift - b0 -- added to
// the byte index, never to the address: b0 passes the shift once the down-scale passes 3x, and an LDS address that goes below
// its base and is widened to a generic pointer afterwards leaves the LDS aperture.  Per-pixel: p is the window row in the
// frame, off = 0.  The two are instantiated apart (every caller is inlined), so LDS rows are read with LDS loads.
struct LbRow {
  const uint8_t* p;
  int off;
  LP_LB_HD int operator[](int b) const { return p[off + b]; }
};
LP_LB_HD LbRow lb_global_row(const LbSource& s, int sy) { return LbRow{s.im + (long)(s.y + sy) * s.pitch + 3L * s.x, 0}; }

// output pixel (row of rc, column ox) from window rows r0 = sy, r1 = sy1: B, G, R into px; xscale = lin_scale(g.new_w, s.w)
template <class Row>
LP_LB_HD void lb_pixel(const LbSource& s, const LbPlace& g, bool resize, const LbRowCoef& rc, double xscale, int ox, const Row& r0,
                       const Row& r1, uint32_t px[3]) {
  const int dx = ox - g.left;
  px[0] = px[1] = px[2] = 114u;
  if (rc.in && dx >= 0 && dx < g.new_w) {
    if (resize) {
      int sx, ax0, ax1;
      lin_coeff(dx, xscale, s.w, sx, ax0, ax1);
      const int sx1 = lb_min(sx + 1, s.w - 1);
LP_LB_UNROLL
      for (int c = 0; c < 3; ++c) px[c] = (uint32_t)lin_blend(r0[sx * 3 + c], r0[sx1 * 3 + c], r1[sx * 3 + c], r1[sx1 * 3 + c], ax0, ax1, rc.ay0, rc.ay1);
    } else {   // new == window size: plain copy
LP_LB_UNROLL
      for (int c = 0; c < 3; ++c) px[c] = (uint32_t)r0[dx * 3 + c];
    }
  }
}

// four adjacent output pixels ox .. ox + 3 of one row as the three dwords of their 12 bytes
template <class Row>
LP_LB_HD void lb_resample4(const LbSource& s, const LbPlace& g, bool resize, const LbRowCoef& rc, int ox, const Row& r0, const Row& r1,
                           uint32_t out[3]) {
  out[0] = out[1] = out[2] = 0u;
  const double xscale = lin_scale(g.new_w, s.w);
LP_LB_UNROLL
  for (int q = 0; q < 4; ++q) {
    uint32_t px[3];
    lb_pixel(s, g, resize, rc, xscale, ox + q, r0, r1, px);
LP_LB_UNROLL
    for (int c = 0; c < 3; ++c) {
      const int b = 3 * q + c;
      out[b >> 2] |= px[c] << (8 * (b & 3));
    }
  }
}

// The launchers' rule: the LDS row of a tile of tile_w output columns of a w-wide window resized to new_w -- the source
// bytes of a tile row plus alignment slack, in whole 16-byte chunks -- and whether the 2 * LB_TH rows of a workgroup fit 64 KiB
// (otherwise the per-pixel form runs: down-scales beyond ~10x).
inline int lb_row_cap(int w, int new_w, int tile_w) {
  const double scale = (double)w / (double)(new_w > 1 ? new_w : 1);
  const int span = (int)(((double)tile_w * scale + 4.0) * 3.0) + 32;
  return (span + 15) & ~15;
}
inline bool lb_rows_fit(int row_cap) { return (size_t)row_cap * 2 * LB_TH <= 64 * 1024; }

#if defined(__HIPCC__)
// ---- the workgroup's steps (256 threads) ---------------------------------------------------------------------------
// stage the 2 * LB_TH rows of output rows oy0 .. oy0 + LB_TH - 1 into band[2 * LB_TH][row_cap], 16 threads per row
__device__ __forceinline__ void lb_stage_band(const LbSource& s, const LbPlace& g, bool resize, LbSpan sp, int oy0, uint8_t* band,
                                              int row_cap, int* s_shift) {
  const int tid = threadIdx.x;
  for (int r = tid >> 4; r < 2 * LB_TH; r += 16) {
    const int shift = lb_stage_row(LbFrame{s.im}, s, g, resize, sp, oy0, r, band + (size_t)r * row_cap, row_cap, tid & 15);
    if ((tid & 15) == 0 && shift >= 0) s_shift[r] = shift;
  }
}

// LDS row r of the band as a window row (`in`: the row was staged, s_shift[r] is set)
__device__ __forceinline__ LbRow lb_staged_row(const uint8_t* band, int row_cap, const int* s_shift, int r, bool in, int b0) {
  return LbRow{band + (size_t)r * row_cap, in ? s_shift[r] - b0 : 0};
}

// four pixels at (oy, ox) of the W-wide picture `pic` (W % 4 == 0, ox % 4 == 0: the 12-byte group is 4-byte aligned)
__device__ __forceinline__ void lb_store4(const LbSource& s, const LbPlace& g, bool resize, const LbRowCoef& rc, uint8_t* __restrict__ pic,
                                          int W, int oy, int ox, const LbRow& r0, const LbRow& r1) {
  uint32_t out[3];
  lb_resample4(s, g, resize, rc, ox, r0, r1, out);
  uint32_t* o = reinterpret_cast<uint32_t*>(pic + ((long)oy * W + ox) * 3);
  o[0] = out[0]; o[1] = out[1]; o[2] = out[2];
}

// the tiled kernels' body: the LB_TH x LB_TW tile (blockIdx.y, blockIdx.x) of the SH x SW picture `pic`
__device__ __forceinline__ void lb_tile(const LbSource& s, const LbPlace& g, uint8_t* __restrict__ pic, int SH, int SW, uint8_t* band,
                                        int row_cap, int* s_shift) {
  const int tid = threadIdx.x, ox0 = blockIdx.x * LB_TW, oy0 = blockIdx.y * LB_TH;
  const bool resize = lb_resizes(s, g);
  const int dxa = lb_max(ox0 - g.left, 0), dxb = lb_min(lb_min(ox0 + LB_TW, SW) - g.left, g.new_w);   // the tile's columns of the resized window
  LbSpan sp{0, 0};
  if (dxa < dxb) {
    sp = lb_span(s, g, resize, dxa, dxb);
    lb_stage_band(s, g, resize, sp, oy0, band, row_cap, s_shift);
  }
  __syncthreads();
  const int j = tid >> 5, ox = ox0 + 4 * (tid & 31);   // thread = (row j, four adjacent columns)
  if (oy0 + j >= SH || ox >= SW) return;
  const LbRowCoef rc = lb_row_coef(s, g, resize, oy0 + j);
  lb_store4(s, g, resize, rc, pic, SW, oy0 + j, ox, lb_staged_row(band, row_cap, s_shift, 2 * j, rc.in, sp.b0),
            lb_staged_row(band, row_cap, s_shift, 2 * j + 1, rc.in, sp.b0));
}

// the per-pixel kernels' body: pixel idx of the SH x SW picture `pic`, rows straight from global memory
__device__ __forceinline__ void lb_pixel_thread(const LbSource& s, const LbPlace& g, uint8_t* __restrict__ pic, int SW, int idx) {
  const int oy = idx / SW, ox = idx - oy * SW;
  const bool resize = lb_resizes(s, g);
  const LbRowCoef rc = lb_row_coef(s, g, resize, oy);
  uint32_t px[3];
  lb_pixel(s, g, resize, rc, lin_scale(g.new_w, s.w), ox, lb_global_row(s, rc.sy), lb_global_row(s, rc.sy1), px);
  uint8_t* o = pic + (long)idx * 3;
  o[0] = (uint8_t)px[0]; o[1] = (uint8_t)px[1]; o[2] = (uint8_t)px[2];
}
#endif

}  // namespace lp
