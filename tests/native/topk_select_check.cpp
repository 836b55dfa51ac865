// Stand-alone check of csrc/topk_select.h (the top-k selection rule of include/litepi.h, lp_topk), built by
// tests/test_topk_cpu.py with a plain g++ under -fsanitize=address,undefined.  Every distribution lives in a heap array of
// exactly nc words, so a read past the row is reported; the result is compared with an independent statement of the rule
// (a stable sort by value descending), the key helpers are checked to be inverses, and the order of the keys is checked
// against the order of the floats.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "topk_select.h"

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

static uint32_t bits_of(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

// the rule, stated apart from the header: classes by value descending, ties by class ascending
static void rule(const std::vector<float>& p, int k, TopkRec* out) {
  std::vector<int> order(p.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return p[a] > p[b]; });
  const int m = std::min<int>(k, (int)p.size());
  for (int j = 0; j < LP_TOPK_K_MAX; ++j) {
    out->cls[j] = j < m ? order[j] : -1;
    out->prob_bits[j] = j < m ? bits_of(p[order[j]]) : 0u;
  }
}

static int check(const char* name, const std::vector<float>& p, int k) {
  const int nc = (int)p.size();
  std::unique_ptr<uint32_t[]> row(new uint32_t[nc]);   // exactly nc words
  for (int c = 0; c < nc; ++c) row[c] = bits_of(p[c]);
  TopkRec got, want;
  std::memset(&got, 0xAB, sizeof(got));
  topk_select_bits(row.get(), nc, k, &got);
  rule(p, k, &want);
  const bool same = std::memcmp(&got, &want, sizeof(got)) == 0;
  EXPECT(same, "%s nc %d k %d: cls[0] %d / %d", name, nc, k, got.cls[0], want.cls[0]);
  return 1;
}

int main() {
  static_assert(sizeof(TopkRec) == 64, "a record is 64 bytes");
  std::mt19937 rng(1234);
  std::normal_distribution<float> normal(0.f, 3.f);
  int cases = 0;
  for (int nc : {1, 2, 3, 58, 63, 64, 65, 130, 1000})
    for (int k : {1, 3, 8}) {
      std::vector<float> z(nc), p(nc);
      for (auto& v : z) v = normal(rng);
      const float mx = *std::max_element(z.begin(), z.end());
      float sum = 0.f;
      for (int c = 0; c < nc; ++c) sum += (p[c] = std::exp(z[c] - mx));
      for (auto& v : p) v /= sum;
      cases += check("softmax", p, k);
      cases += check("equal", std::vector<float>(nc, 1.f / nc), k);
      std::vector<float> hot(nc, 0.f);
      hot[rng() % nc] = 1.f;
      cases += check("one_hot", hot, k);
      std::vector<float> ramp(nc);
      for (int c = 0; c < nc; ++c) ramp[c] = (float)(c + 1) / ((float)nc * (nc + 1) / 2);
      cases += check("ascending", ramp, k);
      std::reverse(ramp.begin(), ramp.end());
      cases += check("descending", ramp, k);
      std::vector<float> tiny(nc, 0.f);   // denormals and the smallest normal keep their bits and their order
      for (int c = 0; c < nc; ++c) tiny[c] = std::ldexp(1.f, -149 + (c * 7) % 24);
      cases += check("denormal", tiny, k);
      std::vector<float> pairs(nc);       // every value twice: ties inside the winners
      for (int c = 0; c < nc; ++c) pairs[c] = (float)((c / 2) % 5) * 0.125f;
      cases += check("pairs", pairs, k);
    }
  std::printf("rule %d cases\n", cases);

  // the key: its order is the rule's order, and class / bits come back out of it
  int keys = 0;
  const float vals[] = {0.f, std::ldexp(1.f, -149), std::ldexp(1.f, -126), 1e-6f, 0.25f, 0.5f, 0.99999994f, 1.f};
  const int classes[] = {0, 1, 63, 64, 65, 129, 1 << 20, 0x7FFFFFFF};
  for (float a : vals)
    for (int ca : classes) {
      const uint64_t ka = topk_key(bits_of(a), ca);
      EXPECT(ka != 0 && ka != ~0ull, "key of (%g, %d)", a, ca);
      EXPECT(topk_key_class(ka) == ca && topk_key_bits(ka) == bits_of(a), "round trip of (%g, %d)", a, ca);
      for (float b : vals)
        for (int cb : classes) {
          const uint64_t kb = topk_key(bits_of(b), cb);
          const bool first = a > b || (a == b && ca < cb);   // (a, ca) comes before (b, cb) under the rule
          EXPECT((ka > kb) == first, "order of (%g, %d) and (%g, %d)", a, ca, b, cb);
          EXPECT(topk_better(kb, ka, ~0ull) == (ka > kb ? ka : kb), "topk_better without a bound");
          EXPECT(topk_better(0, ka, kb) == (ka < kb ? ka : 0), "topk_better below a bound");
          ++keys;
        }
    }
  std::printf("keys %d pairs\n", keys);
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("OK\n");
  return 0;
}
