// Stand-alone check of csrc/quality_measure.h (the crop quality rule shared by lp_quality_measure and the device kernel), built
// with -fsanitize=address,undefined by tests/test_quality_cpu.py.  It walks the crop sizes the tests use, random and extreme
// crops, and compares qm_measure_crop with a naive second implementation: the whole luma plane first, then plain double loops
// with 64-bit sums (128-bit products), so an overflow or an off-by-one row in the rotating three-row form would show.
// It also walks the device kernel's strip plan (qm_strip_rows, qm_strip) on the host for EVERY crop size S % 4 == 0 in 4..1024
// and a few LDS sizes: the same unit loads, the same `counted` rule and the same word indices as quality_measure_kernel, on
// an LDS image that keeps the stale bytes of the strip before, every index checked against what the strip loaded.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "quality_measure.h"

using namespace lp;

static uint32_t rng_state = 12345u;
static uint32_t rng() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static void naive(const std::vector<uint8_t>& rgb, int S, QualityRec* out) {
  std::vector<int> Y((size_t)S * S);
  for (int p = 0; p < S * S; ++p) Y[p] = (77 * rgb[3 * p] + 150 * rgb[3 * p + 1] + 29 * rgb[3 * p + 2] + 128) / 256;
  long long s1 = 0, s2 = 0, t1 = 0, t2 = 0, lo = 0, hi = 0;
  for (int y = 0; y < S; ++y)
    for (int x = 0; x < S; ++x) {
      const int v = Y[(size_t)y * S + x];
      t1 += v; t2 += (long long)v * v; lo += v <= 4; hi += v >= 251;
      if (y >= 1 && y <= S - 2 && x >= 1 && x <= S - 2) {
        const int L = Y[(size_t)(y - 1) * S + x] + Y[(size_t)(y + 1) * S + x] + Y[(size_t)y * S + x - 1] + Y[(size_t)y * S + x + 1] - 4 * v;
        s1 += L; s2 += (long long)L * L;
      }
    }
  const long long n = (long long)(S - 2) * (S - 2), N = (long long)S * S;
  const __int128 num_s = (__int128)n * s2 - (__int128)s1 * s1, num_t = (__int128)N * t2 - (__int128)t1 * t1;
  if (num_s < 0 || num_s >= ((__int128)1 << 62) || num_t < 0 || num_t >= ((__int128)1 << 62)) { printf("FAIL: a product leaves int64 at S = %d\n", S); out->flags = -1; return; }
  out->sharpness = (float)((double)(long long)num_s / ((double)n * (double)n));
  out->luma_mean = (float)((double)t1 / (double)N);
  out->luma_var = (float)((double)(long long)num_t / ((double)N * (double)N));
  out->clip_lo = (float)((double)lo / (double)N);
  out->clip_hi = (float)((double)hi / (double)N);
  out->flags = 1; out->reserved[0] = out->reserved[1] = 0;
}

// quality_measure_kernel's walk of one crop with lds_bytes of luma at a time, threads played one after the other
static bool strips(const std::vector<uint8_t>& rgb, int S, int lds_bytes, QualityRec* out, int* n_strips) {
  std::vector<uint8_t> lds((size_t)lds_bytes, 0xEE);   // persists across strips: what is not loaded is stale
  const int SW = S / 4, H = qm_strip_rows(S, lds_bytes);
  if (H < 4 || H % 4) { printf("FAIL plan S = %d lds %d: H = %d\n", S, lds_bytes, H); return false; }
  long long s1 = 0, s2 = 0, t1 = 0, t2 = 0, lo = 0, hi = 0, n_counted = 0;
  int counted = 0;
  *n_strips = 0;
  for (int y0 = 1; y0 <= S - 2; y0 += H) {
    const QmStrip st = qm_strip(S, H, y0);
    ++*n_strips;
    if (st.p0 % 16 || st.p1 % 16 || st.p0 < 0 || st.p1 > S * S || st.p1 - st.p0 > lds_bytes || st.p0 > counted) {
      printf("FAIL plan S = %d lds %d y0 %d: pixels [%d, %d), counted %d\n", S, lds_bytes, y0, st.p0, st.p1, counted);
      return false;
    }
    for (int u = st.p0 / 16; u < st.p1 / 16; ++u) {   // load: one unit of 16 pixels
      const bool count = u * 16 >= counted;
      for (int i = 0; i < 16; ++i) {
        const uint8_t* px = &rgb[((size_t)u * 16 + i) * 3];
        const int Y = qm_luma(px[0], px[1], px[2]);
        lds[(size_t)u * 16 - st.p0 + i] = (uint8_t)Y;
        if (count) { t1 += Y; t2 += Y * Y; lo += Y <= LP_QM_CLIP_LO; hi += Y >= LP_QM_CLIP_HI; ++n_counted; }
      }
    }
    counted = st.p1;
    const int n_words = (st.y_end - y0) * SW, loaded_words = (st.p1 - st.p0) / 4;
    for (int j = 0; j < n_words; ++j) {   // tap: one packed word
      const int row = j / SW, xw = j - row * SW, k = (row + 1) * SW + xw;
      if (k - SW < 0 || k - 1 < 0 || k + SW >= loaded_words || k + 1 >= loaded_words) {
        printf("FAIL tap S = %d lds %d y0 %d: word %d of %d loaded\n", S, lds_bytes, y0, k, loaded_words);
        return false;
      }
      for (int i = 0; i < 4; ++i) {
        const int x = 4 * xw + i;
        if (x < 1 || x > S - 2) continue;
        const int L = qm_laplacian(lds[4 * (k - SW) + i], lds[4 * (k + SW) + i], lds[4 * k + i - 1], lds[4 * k + i + 1], lds[4 * k + i]);
        s1 += L; s2 += (long long)L * L;
      }
    }
  }
  if (n_counted != (long long)S * S) { printf("FAIL S = %d lds %d: %lld of %d pixels counted\n", S, lds_bytes, n_counted, S * S); return false; }
  QualitySums q;
  q.n = (int64_t)(S - 2) * (S - 2); q.s1 = s1; q.s2 = s2; q.N = (int64_t)S * S; q.t1 = t1; q.t2 = t2; q.lo = lo; q.hi = hi;
  qm_record(q, out);
  return true;
}

static int check(const char* what, const std::vector<uint8_t>& rgb, int S, int* n_checked) {
  QualityRec a, b;
  memset(&a, 0xAB, sizeof(a)); memset(&b, 0xCD, sizeof(b));
  qm_measure_crop(rgb.data(), S, &a);
  naive(rgb, S, &b);
  ++*n_checked;
  if (memcmp(&a, &b, sizeof(a)) != 0) {
    printf("FAIL %s S = %d: header %.9g %.9g %.9g %.9g %.9g %d, naive %.9g %.9g %.9g %.9g %.9g %d\n", what, S, a.sharpness, a.luma_mean, a.luma_var,
           a.clip_lo, a.clip_hi, a.flags, b.sharpness, b.luma_mean, b.luma_var, b.clip_lo, b.clip_hi, b.flags);
    return 1;
  }
  return 0;
}

int main() {
  static_assert(sizeof(QualityRec) == 32, "lp_quality is 32 bytes");
  const int sizes[] = {3, 4, 5, 8, 36, 64, 188, 224, 372, 1024};
  int bad = 0, n_checked = 0;
  float top = 0.0f;
  for (int S : sizes) {
    std::vector<uint8_t> c((size_t)S * S * 3);
    for (int k = 0; k < (S <= 64 ? 4 : 1); ++k) {
      for (auto& v : c) v = (uint8_t)rng();
      bad += check("random", c, S, &n_checked);
    }
    std::fill(c.begin(), c.end(), (uint8_t)0);
    bad += check("zeros", c, S, &n_checked);
    std::fill(c.begin(), c.end(), (uint8_t)255);
    bad += check("ones", c, S, &n_checked);
    for (int y = 0; y < S; ++y)
      for (int x = 0; x < S; ++x) memset(&c[((size_t)y * S + x) * 3], ((x + y) & 1) ? 255 : 0, 3);
    bad += check("checkerboard", c, S, &n_checked);
    QualityRec r;
    qm_measure_crop(c.data(), S, &r);
    if (S % 2 == 0 && r.sharpness != 1040400.0f) { printf("FAIL checkerboard S = %d: sharpness %.9g\n", S, r.sharpness); ++bad; }
    if (r.sharpness > top) top = r.sharpness;
    for (int x = 0; x < S * S; ++x) memset(&c[(size_t)x * 3], (x % S) < S / 2 ? 3 : 252, 3);   // both clip counters
    bad += check("halves", c, S, &n_checked);
  }
  // the kernel's strip plan on every size it accepts; small LDS sizes make small crops take many strips
  int n_walked = 0, most_strips = 0, multi_odd = 0;
  for (int S = 4; S <= 1024; S += 4) {
    std::vector<uint8_t> c((size_t)S * S * 3);
    for (auto& v : c) v = (uint8_t)rng();
    QualityRec want;
    qm_measure_crop(c.data(), S, &want);
    for (int lds : {LP_QM_LDS_BYTES, 8192, 1024}) {
      if (lds / S - 2 < 4) continue;   // no room for four rows and the halo
      QualityRec got;
      int n_strips = 0;
      memset(&got, 0x5A, sizeof(got));
      if (!strips(c, S, lds, &got, &n_strips) || memcmp(&got, &want, sizeof(got)) != 0) {
        printf("FAIL strips S = %d lds %d (%d strips): %.9g %.9g %.9g, want %.9g %.9g %.9g\n", S, lds, n_strips, got.sharpness, got.luma_mean,
               got.luma_var, want.sharpness, want.luma_mean, want.luma_var);
        ++bad;
      }
      ++n_walked;
      if (n_strips > most_strips) most_strips = n_strips;
      if (lds == LP_QM_LDS_BYTES && n_strips > 1 && S % 8 == 4) ++multi_odd;
    }
  }
  if (multi_odd < 100) { printf("FAIL: only %d multi-strip sizes with S %% 8 == 4 walked\n", multi_odd); ++bad; }
  printf("strip walks %d, most strips %d, multi-strip sizes with S %% 8 == 4: %d\n", n_walked, most_strips, multi_odd);
  QualityRec e;
  qm_empty(&e);
  if (e.sharpness != -1.0f || e.luma_mean != 0 || e.luma_var != 0 || e.clip_lo != 0 || e.clip_hi != 0 || e.flags != 0 || e.reserved[0] || e.reserved[1]) {
    printf("FAIL empty record\n"); ++bad;
  }
  if (qm_luma(255, 255, 255) != 255 || qm_luma(0, 0, 0) != 0 || qm_laplacian(255, 255, 255, 255, 0) != 1020 || qm_laplacian(0, 0, 0, 0, 255) != -1020) {
    printf("FAIL luma / laplacian range\n"); ++bad;
  }
  printf("crops %d, largest sharpness %.1f\n", n_checked, top);
  if (bad) { printf("FAILED %d\n", bad); return 1; }
  printf("OK\n");
  return 0;
}
