// The crop quality rule (include/litepi.h, lp_quality): sharpness as the variance of the Laplacian of the crop's luma, and the
// exposure figures.  One definition for the host (lp_quality_measure) and the device (quality_measure_kernel), in the manner
// of topk_select.h and evidence_window.h: the luma, the Laplacian tap, and the step from the integer sums to the record.
// Everything up to the sums is integer arithmetic, so the order of summation does not matter; the record is computed in fp64,
// every operation rounded on its own, and converted to fp32 once.  Pure: no HIP, no handle.
// Exactness: with S <= 1024, n <= N = S^2 <= 2^20, |s1| <= 1020 n < 2^30, s2 <= 1020^2 n < 2^40, t1 <= 255 N < 2^28,
// t2 <= 255^2 N < 2^36.  So n * s2 < 2^60, s1 * s1 < 2^60, N * t2 < 2^56 and t1 * t1 < 2^56: every integer product and
// difference is exact in int64, and n * n, N * N <= 2^40 are exact in fp64.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LP_QM_HD __host__ __device__
#else
#define LP_QM_HD
#endif

namespace lp {

#define LP_QM_S_MIN 3       // the smallest crop with an interior pixel
#define LP_QM_S_MAX 1024    // the largest crop whose int64 products are exact (above)
#define LP_QM_CLIP_LO 4     // Y <= 4 counts as clipped dark
#define LP_QM_CLIP_HI 251   // Y >= 251 counts as clipped bright
#define LP_QM_VALID 1       // LP_QUALITY_VALID of include/litepi.h

// integer luma in 0..255 of one R, G, B pixel
LP_QM_HD inline int qm_luma(int r, int g, int b) { return (77 * r + 150 * g + 29 * b + 128) >> 8; }
// the 4-neighbour Laplacian of an interior pixel, in -1020..1020
LP_QM_HD inline int qm_laplacian(int up, int down, int left, int right, int centre) { return up + down + left + right - 4 * centre; }

struct QualitySums {
  int64_t n, s1, s2;          // interior pixels, sum of L, sum of L^2
  int64_t N, t1, t2, lo, hi;  // pixels, sum of Y, sum of Y^2, #{Y <= 4}, #{Y >= 251}
};

struct QualityRec { float sharpness, luma_mean, luma_var, clip_lo, clip_hi; int32_t flags; int32_t reserved[2]; };   // lp_quality

// one correctly rounded fp64 division on either side
LP_QM_HD inline double qm_div(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __ddiv_rn(a, b);
#else
  return a / b;
#endif
}
LP_QM_HD inline double qm_sq(double a) {   // exact for the a used here (<= 2^20)
#if defined(__HIP_DEVICE_COMPILE__)
  return __dmul_rn(a, a);
#else
  return a * a;
#endif
}

// sums -> record (LP_QM_VALID)
LP_QM_HD inline void qm_record(const QualitySums& s, QualityRec* out) {
  const double n = (double)s.n, N = (double)s.N;
  out->sharpness = (float)qm_div((double)(s.n * s.s2 - s.s1 * s.s1), qm_sq(n));
  out->luma_mean = (float)qm_div((double)s.t1, N);
  out->luma_var = (float)qm_div((double)(s.N * s.t2 - s.t1 * s.t1), qm_sq(N));
  out->clip_lo = (float)qm_div((double)s.lo, N);
  out->clip_hi = (float)qm_div((double)s.hi, N);
  out->flags = LP_QM_VALID;
  out->reserved[0] = 0; out->reserved[1] = 0;
}

// the empty record: no crop was measured
LP_QM_HD inline void qm_empty(QualityRec* out) {
  out->sharpness = -1.0f; out->luma_mean = 0.0f; out->luma_var = 0.0f; out->clip_lo = 0.0f; out->clip_hi = 0.0f;
  out->flags = 0; out->reserved[0] = 0; out->reserved[1] = 0;
}

// ---- the strip plan of the device kernel (quality_kernels.hip), here so that tests/native/quality_measure_check.cpp can walk it
// on the host for every crop size.  The kernel holds the luma plane linearly (byte p = y * S + x) in LDS, lds_bytes at a
// time, and loads it in units of 16 pixels (48 RGB bytes); S % 4 == 0 makes S * S a whole number of units.
#define LP_QM_LDS_BYTES 32768   // luma bytes of a strip; a multiple of 16
// Laplacian rows per strip: a multiple of 4 (so H * S is a whole number of units), two halo rows fit beside them
LP_QM_HD inline int qm_strip_rows(int S, int lds_bytes) {
  const int h = ((lds_bytes / S) - 2) & ~3;
  return h < S ? h : S;
}
struct QmStrip { int p0, p1, y_end; };   // pixels [p0, p1) are loaded, both unit boundaries; Laplacian rows [y0, y_end)
// the strip whose first Laplacian row is y0 = 1 + k * H
LP_QM_HD inline QmStrip qm_strip(int S, int H, int y0) {
  QmStrip s;
  s.p0 = (y0 - 1) * S;                 // k * H * S: a unit boundary
  const int end = (y0 + H + 1) * S;    // the end of the lower halo row: 2 S past a unit boundary, i.e. one only when S % 8 == 0
  // rounded up to whole units: up to 8 pixels of the row behind the halo come along.  They fit: (H + 2) * S <= lds_bytes, a
  // multiple of 16; and end < S * S, a multiple of 16, keeps the rounded end inside the crop
  s.p1 = end >= S * S ? S * S : (end + 15) & ~15;
  s.y_end = y0 + H < S - 1 ? y0 + H : S - 1;
  return s;
}

// the rule on one S x S x 3 uint8 RGB crop, S in LP_QM_S_MIN..LP_QM_S_MAX: three luma rows at a time, row by row (host side)
inline void qm_measure_crop(const uint8_t* rgb, int S, QualityRec* out) {
  QualitySums s = {};
  s.n = (int64_t)(S - 2) * (S - 2); s.N = (int64_t)S * S;
  uint8_t rows[3][LP_QM_S_MAX];   // luma of rows y - 1, y, y + 1, rotating
  for (int y = 0; y < S; ++y) {
    uint8_t* cur = rows[y % 3];
    for (int x = 0; x < S; ++x) {
      const uint8_t* p = rgb + ((size_t)y * S + x) * 3;
      const int Y = qm_luma(p[0], p[1], p[2]);
      cur[x] = (uint8_t)Y;
      s.t1 += Y; s.t2 += Y * Y; s.lo += Y <= LP_QM_CLIP_LO; s.hi += Y >= LP_QM_CLIP_HI;
    }
    if (y >= 2) {   // row y - 1 is an interior row with both neighbours known
      const uint8_t *up = rows[(y - 2) % 3], *mid = rows[(y - 1) % 3], *down = cur;
      for (int x = 1; x < S - 1; ++x) {
        const int L = qm_laplacian(up[x], down[x], mid[x - 1], mid[x + 1], mid[x]);
        s.s1 += L; s.s2 += (int64_t)L * L;
      }
    }
  }
  qm_record(s, out);
}

}  // namespace lp
