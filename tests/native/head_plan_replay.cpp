// Host replay of csrc/head_plan.h, the planner and weight-stream packer of the fused Detect head (tests/test_head_plan_cpu.py).
// stdin: one request per line; stdout: one line per request.
//   head cin c2 c3 nc reg_max switches     (switches: bit 0 merged_a, 1 a32, 2 two_wg, 3 one_wg)
//        -> "0 <why>", or
//           1 variant name C3T KPT TH TW PA PB NPC KSA SLOTF OVL A16 SPLIT_A KSAC NCAC KSAB NCAB lds_bytes nchunks | coff.. | csz.. | cks.. |
//             stream_bytes fnv(stream) fnv(biasA) fnv(biasB) fnv(biasC)
//        with the source tensors of the recording: element i of tensor t is ((i * 7919 + 131 * t) mod 509 - 254) / 128
//   table -> one line per row of kHeadVariants: name and the kernel's 14 template arguments, then "end"
#include <cstdio>
#include <cstring>

#include "head_plan.h"

using namespace lp::hplan;

static unsigned long long fnv1a(const void* p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  const unsigned char* b = static_cast<const unsigned char*>(p);
  for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
  return h;
}
static std::vector<float> fill(size_t n, int t) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = (float)((int)((i * 7919ull + 131ull * t) % 509ull) - 254) / 128.0f;
  return v;
}

int main() {
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    int cin, c2, c3, nc, reg_max, m;
    if (sscanf(line, "head %d %d %d %d %d %d", &cin, &c2, &c3, &nc, &reg_max, &m) == 6) {
      HeadSwitches sw;
      sw.merged_a = m & 1; sw.a32 = m & 2; sw.two_wg = m & 4; sw.one_wg = m & 8;
      const HeadPlan p = plan_head(cin, c2, c3, nc, reg_max, sw);
      if (!p.ok) { printf("0 %s\n", p.plan_err); continue; }
      const std::vector<float> wa = fill((size_t)(64 + c3) * 9 * cin, 1), ba = fill(64 + c3, 2), wbb = fill(64 * 9 * 64, 3), bbb = fill(64, 4),
                               wpb = fill(64 * 64, 5), bpb = fill(64, 6), wbc = fill((size_t)c3 * 9 * c3, 7), bbc = fill(c3, 8),
                               wpc = fill((size_t)nc * c3, 9), bpc = fill(nc, 10);
      const Src s{&wa, &ba, &wbb, &bbb, &wpb, &bpb, &wbc, &bbc, &wpc, &bpc, nc};
      const HeadPack k = pack_head(p, s);
      if (k.pack_err) { printf("0 pack: %s\n", k.pack_err); continue; }
      printf("1 %d %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %zu %d |", p.variant, kernel_name(kHeadVariants[p.variant]).c_str(), p.C3T, p.KPT, p.TH,
             p.TW, p.PA, p.PB, p.NPC, p.KSA, p.SLOTF, p.OVL, p.A16, p.SPLIT_A, p.KSAC, p.NCAC, p.KSAB, p.NCAB, p.lds_bytes, p.nchunks);
      for (auto v : k.coff) printf(" %d", (int)v);
      printf(" |");
      for (auto v : k.csz) printf(" %d", (int)v);
      printf(" |");
      for (auto v : k.cks) printf(" %d", (int)v);
      printf(" | %zu %016llx %016llx %016llx %016llx\n", k.stream.size() * 2, fnv1a(k.stream.data(), k.stream.size() * 2),
             fnv1a(k.biasA.data(), k.biasA.size() * 4), fnv1a(k.biasB.data(), k.biasB.size() * 4), fnv1a(k.biasC.data(), k.biasC.size() * 4));
    } else if (strncmp(line, "table", 5) == 0) {
      for (const HeadVariant& v : kHeadVariants)
        printf("%s %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", kernel_name(v).c_str(), v.c3t, v.pa, v.pb, v.npc(), v.ksa, v.slotf, v.nrw, (int)v.ov, (int)v.a16,
               v.nca(), v.ksac(), v.ncac(), v.ksab(), v.ncab());
      printf("end\n");
    } else {
      fprintf(stderr, "bad request: %s", line);
      return 2;
    }
  }
  return 0;
}
