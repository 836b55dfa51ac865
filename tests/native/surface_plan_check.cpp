// Host-only check of csrc/surface_plan.h and csrc/ring_slots.h, built with a plain g++ under -fsanitize=address,undefined (tests/test_surface_plan_cpu.py):
// the argument rules of include/litepi.h on exact-sized arrays, the table records of seeded random surface sets, and the pinned
// rings' slot policy (RingSlots, behind every PlanRing) against a model of the copies in flight.  Prints one line per section and "OK"; any failure is a message on
// stderr and a non-zero exit.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "ring_slots.h"
#include "surface_plan.h"

namespace lp {
void set_last_error(const std::string&) {}
}  // namespace lp

using namespace lp;

static int failures = 0;
#define EXPECT(cond, ...)                     \
  do {                                        \
    if (!(cond)) {                            \
      fprintf(stderr, "line %d: ", __LINE__); \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
      ++failures;                             \
    }                                         \
  } while (0)

static int status(const lp_surface_format* f, const lp_surface* s, int B, bool same) {
  try {
    check_surfaces(f, s, B, same);
  } catch (const Error& e) {
    if (std::string(e.what()).empty()) return -100;   // every refusal says why
    return e.code;
  }
  return LP_OK;
}

static lp_surface surf(uintptr_t y, uintptr_t uv, int h, int w, int py = 0, int puv = 0) {
  lp_surface s;
  memset(&s, 0, sizeof(s));
  s.plane[0] = reinterpret_cast<const void*>(y); s.plane[1] = reinterpret_cast<const void*>(uv);
  s.pitch[0] = py; s.pitch[1] = puv; s.height = h; s.width = w;
  return s;
}

int main() {
  static_assert(sizeof(lp_surface) == 48 && sizeof(lp_surface_format) == 32, "the header's records");
  const uintptr_t A = 0x7f0000001000ull;
  lp_surface_format nv, p010;
  memset(&nv, 0, sizeof(nv)); memset(&p010, 0, sizeof(p010));
  nv.pixfmt = LP_SURF_NV12; p010.pixfmt = LP_SURF_P010;

  // ---- the rules, each on a heap array of exactly B records (a read past it is the sanitizer's finding)
  {
    std::vector<lp_surface> one(1, surf(A, A + 4096, 4, 6));
    EXPECT(status(&nv, one.data(), 1, false) == LP_OK && status(&p010, one.data(), 1, true) == LP_OK, "tight surfaces are accepted");
    EXPECT(status(nullptr, one.data(), 1, false) == LP_ERR_ARG && status(&nv, nullptr, 1, false) == LP_ERR_ARG, "null arguments");
    EXPECT(status(&nv, one.data(), 0, false) == LP_ERR_ARG && status(&nv, one.data(), -3, false) == LP_ERR_ARG, "B < 1 reads nothing");
    for (int pf : {0, 3, -1}) { lp_surface_format f = nv; f.pixfmt = pf; EXPECT(status(&f, one.data(), 1, false) == LP_ERR_ARG, "pixfmt %d", pf); }
    for (int m : {2, -1}) { lp_surface_format f = nv; f.matrix = m; EXPECT(status(&f, one.data(), 1, false) == LP_ERR_ARG, "matrix %d", m); }
    for (int k = 0; k < 6; ++k) { lp_surface_format f = nv; f.reserved[k] = 1; EXPECT(status(&f, one.data(), 1, false) == LP_ERR_ARG, "format reserved %d", k); }
    for (int k = 0; k < 4; ++k) { std::vector<lp_surface> s = one; s[0].reserved[k] = -1; EXPECT(status(&nv, s.data(), 1, false) == LP_ERR_ARG, "surface reserved %d", k); }
    struct Case { const char* name; lp_surface s; bool nv_ok, p010_ok; };
    const Case cases[] = {
        {"null luma", surf(0, A, 4, 6), false, false}, {"null chroma", surf(A, 0, 4, 6), false, false},
        {"odd height", surf(A, A, 5, 6), false, false}, {"odd width", surf(A, A, 4, 7), false, false},
        {"zero height", surf(A, A, 0, 6), false, false}, {"negative width", surf(A, A, 4, -6), false, false},
        {"luma pitch W - 1", surf(A, A, 4, 6, 5, 0), false, false}, {"chroma pitch W - 2", surf(A, A, 4, 6, 0, 4), false, false},
        {"pitch W", surf(A, A, 4, 6, 6, 6), true, false}, {"pitch 2 W - 2", surf(A, A, 4, 6, 10, 10), true, false},
        {"pitch 2 W", surf(A, A, 4, 6, 12, 12), true, true}, {"negative luma pitch", surf(A, A, 4, 6, -8, 0), false, false},
        {"negative chroma pitch", surf(A, A, 4, 6, 0, -256), false, false}, {"odd luma address", surf(A + 1, A, 4, 6), true, false},
        {"odd chroma address", surf(A, A + 3, 4, 6), true, false}, {"odd luma pitch", surf(A, A, 4, 6, 13, 0), true, false},
        {"odd chroma pitch", surf(A, A, 4, 6, 0, 257), true, false}, {"unequal pitches", surf(A + 8, A + 16, 4, 6, 14, 2048), true, true},
        {"the widest row", surf(A, A, 2, 0x7ffffffe), true, false},   // 2 W bytes do not fit an int: refused, not wrapped
    };
    for (const Case& c : cases)
      for (int pos = 0; pos < 3; ++pos) {   // the bad record first, in the middle, last
        std::vector<lp_surface> s(3, surf(A, A + 4096, 4, 6));
        s[pos] = c.s;
        EXPECT((status(&nv, s.data(), 3, false) == LP_OK) == c.nv_ok, "%s as NV12 at %d", c.name, pos);
        EXPECT((status(&p010, s.data(), 3, false) == LP_OK) == c.p010_ok, "%s as P010 at %d", c.name, pos);
      }
    std::vector<lp_surface> mixed = {surf(A, A, 4, 6), surf(A, A, 4, 8), surf(A, A, 6, 6)};
    EXPECT(status(&nv, mixed.data(), 3, false) == LP_OK && status(&nv, mixed.data(), 3, true) == LP_ERR_ARG, "sizes may differ only without same_size");
    EXPECT(status(&nv, mixed.data(), 1, true) == LP_OK, "one surface is of one size");
    printf("rules %zu cases\n", sizeof(cases) / sizeof(cases[0]));
  }

  // ---- the table: seeded random sets into an exact-sized array
  {
    std::mt19937 rng(5);
    int n_aligned = 0, n = 0;
    for (int round = 0; round < 2000; ++round) {
      const bool wide = rng() % 2;
      lp_surface_format f = wide ? p010 : nv;
      const int bps = wide ? 2 : 1, B = 1 + rng() % 9;
      std::vector<lp_surface> s(B);
      std::vector<long> off(B);
      const uintptr_t dst = A + 16 * (rng() % 4) + (rng() % 3 == 0 ? 8 : 0);
      long total = 0;
      for (int i = 0; i < B; ++i) {
        const int h = 2 * (1 + rng() % 600), w = rng() % 3 ? 16 * (1 + rng() % 130) : 2 * (1 + rng() % 1000);
        const int py = rng() % 2 ? 0 : bps * w + 2 * (int)(rng() % 3 ? 0 : rng() % 64), puv = rng() % 2 ? 0 : (bps * w + 255) / 256 * 256;
        s[i] = surf(A + 4096 * i + (rng() % 4 ? 0 : 2 * (rng() % 9)), A + (1 << 24) + 4096 * i + (rng() % 4 ? 0 : 2 * (rng() % 9)), h, w, py, puv);
        off[i] = total;
        total = (total + (long)h * w * 3 + 15) & ~15L;
      }
      if (status(&f, s.data(), B, false) != LP_OK) { EXPECT(false, "round %d: a generated set was refused", round); continue; }
      std::vector<SurfFrame> tab(B);
      const int mb = fill_surface_table(f, s.data(), B, reinterpret_cast<const void*>(dst), off.data(), tab.data());
      int want_mb = 0;
      for (int i = 0; i < B; ++i) {
        const SurfFrame& t = tab[i];
        const int py = s[i].pitch[0] ? s[i].pitch[0] : bps * s[i].width, puv = s[i].pitch[1] ? s[i].pitch[1] : bps * s[i].width;
        EXPECT(t.y == s[i].plane[0] && t.uv == s[i].plane[1] && t.h == s[i].height && t.w == s[i].width && t.dst_off == off[i] && t.pad == 0,
               "round %d record %d: fields", round, i);
        EXPECT(t.pitch_y == py && t.pitch_uv == puv && py >= bps * t.w && puv >= bps * t.w, "round %d record %d: pitches", round, i);
        // aligned <=> every 16-byte access of a full block is aligned: both bases, both pitches, the BGR row (3 W) and base
        bool al = true;
        for (uintptr_t v : {reinterpret_cast<uintptr_t>(t.y), reinterpret_cast<uintptr_t>(t.uv), (uintptr_t)py, (uintptr_t)puv,
                            (uintptr_t)(3 * (long)t.w), dst + (uintptr_t)off[i]})
          al = al && v % 16 == 0;
        EXPECT((t.aligned == 1) == al && (t.aligned == 0 || t.aligned == 1), "round %d record %d: aligned flag", round, i);
        // the last full block's reads end inside the row, the last row pair inside the plane
        const int cpr = (t.w + 15) / 16, full = t.w / 16;
        EXPECT(16 * bps * full <= py && 16 * bps * full <= puv && cpr >= 1, "round %d record %d: a full block passes the row", round, i);
        want_mb = std::max(want_mb, (t.h / 2) * cpr);
        n_aligned += t.aligned;
        ++n;
      }
      EXPECT(mb == want_mb && mb >= 1, "round %d: max_blocks %d, expected %d", round, mb, want_mb);
    }
    EXPECT(n_aligned > n / 50 && n_aligned < n, "both access paths occur (%d of %d aligned)", n_aligned, n);
    printf("tables %d records, %d aligned\n", n, n_aligned);
  }

  // ---- the ring: a slot is never written while its copy may be in flight, and nothing waits before the ring wraps
  {
    constexpr int RING = 8;
    RingSlots<RING> slots;
    int in_flight[RING];   // the call whose copy last read the slot, -1: none or waited for
    for (int& v : in_flight) v = -1;
    int waits = 0;
    for (int call = 0; call < 1000; ++call) {
      bool wait = false;
      const int slot = slots.take(&wait);
      EXPECT(slot == call % RING, "call %d took slot %d", call, slot);
      EXPECT(wait == (in_flight[slot] >= 0), "call %d: wait %d with copy of call %d in the slot", call, (int)wait, in_flight[slot]);
      EXPECT(wait == (call >= RING), "call %d: only a wrapped ring waits", call);
      if (wait) { EXPECT(in_flight[slot] == call - RING, "call %d waits for call %d", call, in_flight[slot]); ++waits; }
      in_flight[slot] = call;
      slots.mark(slot);
    }
    // a call that fails between take() and mark() (an error thrown by the copy) leaves the slot free, not busy for ever
    bool wait = false;
    const int s0 = slots.take(&wait);
    EXPECT(wait, "the slot was busy");
    for (int k = 1; k < RING; ++k) { const int s = slots.take(&wait); slots.mark(s); }
    EXPECT(slots.take(&wait) == s0 && !wait, "an unmarked slot is not waited for");
    printf("ring %d waits in 1000 calls\n", waits);
  }
  if (failures) { fprintf(stderr, "%d failures\n", failures); return 1; }
  printf("OK\n");
  return 0;
}
