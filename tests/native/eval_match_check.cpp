// Stand-alone check of csrc/eval_match.h (the evaluator's matching rule of include/litepi.h, lp_eval_*), built by
// tests/test_eval_cpu.py with a plain g++ under -fsanitize=address,undefined.  Records, ground truth and results live in heap
// arrays of exactly P, G and P elements, so an access past a frame is reported; coordinates at and beyond the limits of int32
// and float show that nothing in the IoU leaves int64.  The result is compared with a straightforward O(P * G * T)
// restatement of the rule: per threshold, the winner of a ground truth is found by a scan over all records.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <vector>

#include "eval_match.h"

using namespace lp;

static int failures = 0;
#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      ++failures;                                \
      std::printf("FAIL %s: ", #cond);           \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
    }                                            \
  } while (0)

static lp_det det(float x1, float y1, float x2, float y2, int cls, float conf = 0.5f) { return lp_det{x1, y1, x2, y2, conf, 0, cls, 0.5f}; }
static lp_gt gt(int cls, int x1, int y1, int x2, int y2) { return lp_gt{cls, x1, y1, x2, y2, {0, 0, 0}}; }

// the rule, stated apart from the header's functions
static long long coord(double v) {
  if (v != v) return 0;
  if (v < -536870912.0) return -536870912;
  if (v > 536870912.0) return 536870912;
  return (long long)std::trunc(v);
}
static double iou_of(const lp_det& d, const lp_gt& g) {
  const long long p[4] = {coord(d.x1), coord(d.y1), coord(d.x2), coord(d.y2)}, q[4] = {coord(g.x1), coord(g.y1), coord(g.x2), coord(g.y2)};
  const long long iw = std::max(0LL, std::min(p[2], q[2]) - std::max(p[0], q[0])), ih = std::max(0LL, std::min(p[3], q[3]) - std::max(p[1], q[1]));
  const long long inter = iw * ih, uni = (p[2] - p[0]) * (p[3] - p[1]) + (q[2] - q[0]) * (q[3] - q[1]) - inter;
  return (double)inter / ((double)uni + 1e-7);
}
static void rule(const std::vector<lp_det>& d, const std::vector<lp_gt>& g, const std::vector<double>& thr, std::vector<lp_match_rec>& out) {
  const int P = (int)d.size(), G = (int)g.size();
  std::vector<int> best(P, -1);
  std::vector<double> b(P, 0.0);
  for (int p = 0; p < P; ++p) {
    double m = -std::numeric_limits<double>::infinity();
    for (int k = 0; k < G; ++k) m = std::max(m, iou_of(d[p], g[k]));
    if (G == 0 || m == 0.0) continue;
    for (int k = G - 1; k >= 0; --k)
      if (iou_of(d[p], g[k]) == m) { best[p] = k; break; }
    b[p] = m;
  }
  for (int p = 0; p < P; ++p) {
    out[p].correct = 0; out[p].gt = best[p]; out[p].iou = b[p];
    if (best[p] < 0 || d[p].cls_class != g[best[p]].cls) continue;
    for (size_t j = 0; j < thr.size(); ++j) {
      if (!(b[p] >= thr[j])) continue;
      bool earlier = false;   // an earlier record that is a candidate of the same ground truth wins it
      for (int q = 0; q < p; ++q) earlier = earlier || (best[q] == best[p] && b[q] >= thr[j]);
      if (!earlier) out[p].correct |= 1u << j;
    }
  }
}

static int check(const char* name, const std::vector<lp_det>& d, const std::vector<lp_gt>& g, const std::vector<double>& thr,
                 const unsigned* want_bits = nullptr, const int* want_gt = nullptr) {
  const int P = (int)d.size(), G = (int)g.size();
  std::unique_ptr<lp_det[]> dets(new lp_det[P]);   // exactly P, G and P elements
  std::unique_ptr<lp_gt[]> gts(new lp_gt[G]);
  std::unique_ptr<lp_match_rec[]> got(new lp_match_rec[P]);
  for (int p = 0; p < P; ++p) dets[p] = d[p];
  for (int k = 0; k < G; ++k) gts[k] = g[k];
  std::memset(got.get(), 0xAB, sizeof(lp_match_rec) * P);
  eval_match_frame(dets.get(), P, gts.get(), G, thr.data(), (int)thr.size(), got.get());
  std::vector<lp_match_rec> want(P);
  rule(d, g, thr, want);
  for (int p = 0; p < P; ++p) {
    EXPECT(got[p].correct == want[p].correct && got[p].gt == want[p].gt && std::memcmp(&got[p].iou, &want[p].iou, 8) == 0,
           "%s record %d: correct %x / %x gt %d / %d iou %.17g / %.17g", name, p, got[p].correct, want[p].correct, got[p].gt, want[p].gt,
           got[p].iou, want[p].iou);
    if (want_bits) EXPECT(got[p].correct == want_bits[p] && got[p].gt == want_gt[p], "%s record %d: correct %x gt %d", name, p, got[p].correct, got[p].gt);
  }
  return 1;
}

int main() {
  static_assert(sizeof(lp_match_rec) == 16 && sizeof(lp_eval_row) == 16 && sizeof(lp_gt) == 32, "record sizes");
  std::vector<double> thr10;
  for (int j = 0; j < 10; ++j) thr10.push_back(0.5 + j * 0.05);
  int cases = 0;
  {   // the hand-built frames
    const unsigned b0[] = {0x3F}; const int g0[] = {1};
    cases += check("gt_tie_higher_g", {det(0, 0, 10, 10, 1)}, {gt(0, 0, 0, 10, 8), gt(1, 0, 2, 10, 10)}, thr10, b0, g0);
    const unsigned b1[] = {0x0FF, 0x300}; const int g1[] = {0, 0};
    cases += check("two_records_lower_p", {det(0, 0, 10, 9, 3), det(0, 0, 10, 10, 3)}, {gt(3, 0, 0, 10, 10)}, thr10, b1, g1);
    const unsigned b2[] = {0, 0}; const int g2[] = {0, 0};
    cases += check("wrong_class_blocks", {det(0, 0, 10, 10, 2), det(0, 0, 10, 10, 3)}, {gt(3, 0, 0, 10, 10)}, thr10, b2, g2);
    const unsigned b3[] = {0}; const int g3[] = {0};
    cases += check("unclassified", {det(0, 0, 10, 10, -1)}, {gt(0, 0, 0, 10, 10)}, thr10, b3, g3);
    const unsigned b4[] = {0, 0x3FF}; const int g4[] = {-1, 0};
    cases += check("zero_area", {det(5, 5, 5, 9, 0), det(0, 0, 10, 10, 0)}, {gt(0, 0, 0, 10, 10), gt(0, 20, 20, 20, 20)}, thr10, b4, g4);
    const unsigned b5[] = {0x3FF}; const int g5[] = {0};
    cases += check("truncation", {det(-0.9f, 2.99f, 12.99f, 14.5f, 0)}, {gt(0, 0, 2, 12, 14)}, thr10, b5, g5);
    const unsigned b6[] = {0x2}; const int g6[] = {0};
    cases += check("on_threshold", {det(0, 0, 10, 5, 0)}, {gt(0, 0, 0, 10, 10)}, {0.5, 0.45, 0.55}, b6, g6);
    const unsigned b7[] = {0, 0}; const int g7[] = {-1, -1};
    cases += check("no_ground_truth", {det(0, 0, 10, 10, 0), det(1, 1, 5, 5, 0)}, {}, thr10, b7, g7);
    cases += check("no_records", {}, {gt(0, 0, 0, 10, 10)}, thr10);
  }
  {   // the limits of the number formats: nothing leaves int64, no float-to-int conversion is out of range
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const int lo = std::numeric_limits<int>::min(), hi = std::numeric_limits<int>::max();
    cases += check("limits", {det(-inf, -inf, inf, inf, 0), det(nan, nan, nan, nan, 0), det(-3e9f, -3e9f, 3e9f, 3e9f, 0), det(3e38f, 0, -3e38f, 10, 0),
                              det(0, 0, 10, 10, 0)},
                   {gt(0, lo, lo, hi, hi), gt(0, hi, hi, lo, lo), gt(0, 0, 0, 10, 10), gt(0, lo, 0, hi, 1)}, thr10);
  }
  std::mt19937 rng(4321);
  int sweep = 0;
  for (int P : {0, 1, 7, 64, 65, 300})
    for (int G : {0, 1, 4, 64, 256})
      for (int n_thr : {1, 10, 16}) {
        std::vector<lp_gt> g;
        for (int k = 0; k < G; ++k) {
          const int x = rng() % 400, y = rng() % 400, w = 4 + rng() % 40, h = 4 + rng() % 40;
          g.push_back(gt(rng() % 5, x, y, x + w, y + h));
        }
        std::vector<lp_det> d;
        for (int p = 0; p < P; ++p) {
          if (G && rng() % 4) {   // around a ground truth, on a coarse grid: exact IoU ties between records and between boxes occur
            const lp_gt& s = g[rng() % G];
            const int j = 3;
            d.push_back(det((float)(s.x1 + (int)(rng() % j) - 1) + 0.25f * (rng() % 4), (float)(s.y1 + (int)(rng() % j) - 1), (float)(s.x2 + (int)(rng() % j) - 1),
                            (float)(s.y2 + (int)(rng() % j) - 1) + 0.5f, rng() % 3 ? s.cls : (int)(rng() % 5) - 1));
          } else {
            const int x = rng() % 400, y = rng() % 400;
            d.push_back(det((float)x, (float)y, (float)(x + 4 + rng() % 40), (float)(y + 4 + rng() % 40), (int)(rng() % 5)));
          }
        }
        std::vector<double> thr;
        for (int j = 0; j < n_thr; ++j) thr.push_back(n_thr == 16 ? 0.2 + 0.05 * ((j * 7) % 16) : 0.5 + j * 0.05);   // 16: unsorted
        sweep += check("sweep", d, g, thr);
      }
  std::printf("frames %d hand-built, %d swept\n", cases, sweep);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
