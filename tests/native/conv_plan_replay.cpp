// Host replay of csrc/conv_plan.h, the tile and split planner of the convolution kernels (tests/test_conv_plan_cpu.py).
// stdin: one request per line; stdout: one line of integers per request.
//   conv  prec k stride cin cout hout wout batch_hint full_n single_chunk
//         -> direct NT nsplits CK CGc nchunks steps LW PS bwh bww lds_bytes rcp_cg rcp_ps rcp_pcs      (or "err <message>")
//   bneck prec c h w batch_hint has_cv2 cat_global c3 in_is_last_stored cl
//         -> ok TH TW LW lds_bytes cl PSA T2 kg sg
//   tables -> the tables of instantiated variants, one per line, as plain numbers
#include <cstdio>
#include <cstring>

#include "conv_plan.h"

using namespace lp::cplan;

template <size_t N> static void print_variants(const char* name, const Variant (&t)[N]) {
  printf("%s", name);
  for (const Variant& v : t) printf(" %d,%d", v.nt, v.t2);
  printf("\n");
}
template <size_t N> static void print_ints(const char* name, const int (&t)[N]) {
  printf("%s", name);
  for (int v : t) printf(" %d", v);
  printf("\n");
}

int main() {
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    int v[10];
    if (sscanf(line, "conv %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9) == 10) {
      const ConvTiling p = plan_conv(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8] != 0, v[9] != 0);
      if (p.plan_err) { printf("err %s\n", p.plan_err); continue; }
      printf("%d %d %d %d %d %d %d %d %d %d %d %zu %u %u %u\n", (int)p.direct, p.NT, p.nsplits, p.CK, p.CGc, p.nchunks, p.steps, p.LW, p.PS, p.bwh, p.bww,
             p.lds_bytes, p.rcp_cg, p.rcp_ps, p.rcp_pcs);
    } else if (sscanf(line, "bneck %d %d %d %d %d %d %d %d %d %d", v, v + 1, v + 2, v + 3, v + 4, v + 5, v + 6, v + 7, v + 8, v + 9) == 10) {
      BneckTail t;
      t.cat_global = v[6]; t.c3 = v[7]; t.in_is_last_stored = v[8] != 0; t.cl = v[9] != 0;
      const BneckTiling p = plan_bneck(v[0], v[1], v[2], v[3], v[4], v[5] ? &t : nullptr);
      printf("%d %d %d %d %zu %d %d %d %d %d\n", (int)p.ok, p.TH, p.TW, p.LW, p.lds_bytes, (int)p.cl, p.PSA, p.T2, p.kg, p.sg);
    } else if (strncmp(line, "tables", 6) == 0) {
      print_variants("conv3x3", kConv3x3);
      print_variants("convs2", kConvS2);
      print_ints("conv1x1", kConv1x1);
      print_ints("stem_co", kStemCO);
      print_ints("bneck_nt", kBneckNT);
      print_variants("bneck_tails", kBneckTails);
      printf("bneck_max_sg %d %d\n", kBneckMaxSgF16, kBneckMaxSgF32);
      for (const BneckTile& b : kBneckTiles) printf("bneck_tile %d %d %d %d %d %d %d\n", b.th, b.tw, b.p1, b.p2, b.max_nt, (int)b.tail, (int)b.cl);
      printf("end\n");
    } else {
      fprintf(stderr, "bad request: %s", line);
      return 2;
    }
  }
  return 0;
}
