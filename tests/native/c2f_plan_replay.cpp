// Host replay of csrc/c2f_plan.h, the configurations, predicates and weight packers of c2f_kernels.hip (tests/test_c2f_plan_cpu.py).
// stdin: one request per line; stdout: one line per request.
//   c2f C NB KA KB UP COUT MODE KS2 h w      -> supported  kernel_name | "-"  cv2_from_lds
//   c2fpack C NB KA KB UP COUT MODE KS2 h w  -> "0", or 1 <the row, as "rows" prints it> | macs_per_image | bytes fnv(w) bytes fnv(b) per C2F_W_* slot
//   s2 cin cout cout2 tail h w               -> supported (tail 0) or tail_supported (tail 1)  lds_staged(cin, cout)
//   s2pack cin cout tail h w                 -> "0", or 1 <the row> | bytes fnv of w, b, w2, b2
//   sppf cin c cout h w                      -> "0", or 1 <the row> | macs_per_image | bytes fnv of w1, b1, w2, b2
//        with the source tensors of the recording: element i of tensor t is ((i * 7919 + 131 * t) mod 509 - 254) / 128; t counts the
//        members of C2fSrc from 1 in declaration order (cv1, cv1_b, a[0], a_b[0], bb[0], bb_b[0], a[1], .., sp2_b), the arguments of
//        pack_s2 and pack_sppf behind the shape likewise
//   rows  -> one line per row of the three tables, then "end":
//            c2f name C NB KA KB UP COUT MODE KS2 th tw waves lds wg_per_tile nt1 ntm nt2 nt_s2 perimg gk cv2_lds
//            s2 name cin cout tail th tw waves lds wg_per_tile nt ksplit S lds_staged
//            sppf name cin c cout th tw waves lds wg_per_tile nt1 nt2
//   table -> one line per type of the for_each_* lists and SppfCfg: kernel, profile name, the type's template arguments; then "end"
#include <cstdio>
#include <cstring>

#include "c2f_plan.h"

using namespace lp;
using namespace lp::c2fplan;

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
template <class T> static void print_hash(const std::vector<T>& v) { printf(" %zu %016llx", v.size() * sizeof(T), fnv1a(v.data(), v.size() * sizeof(T))); }

static void print_row(const C2fRow& r) {
  const C2fShape& k = r.key;
  printf("c2f %s %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", r.name.c_str(), k.C, k.NB, k.KA, k.KB, k.UP, k.COUT, k.MODE, k.KS2, r.th, r.tw, r.waves,
         r.lds_bytes, r.wg_per_tile, r.nt1, r.ntm, r.nt2, r.nt_s2, (int)r.perimg, (int)r.gk, (int)r.cv2_lds);
}
static void print_row(const S2Row& r) {
  printf("s2 %s %d %d %d %d %d %d %d %d %d %d %d %d", r.name.c_str(), r.cin, r.cout, (int)r.tail, r.th, r.tw, r.waves, r.lds_bytes, r.wg_per_tile, r.nt, r.ksplit, r.S,
         (int)r.lds_staged);
}
static void print_row(const SppfRow& r) {
  printf("sppf %s %d %d %d %d %d %d %d %d %d %d", r.name.c_str(), r.cin, r.c, r.cout, r.th, r.tw, r.waves, r.lds_bytes, r.wg_per_tile, r.nt1, r.nt2);
}

// the template arguments of a configuration type, as the object's symbols spell them
template <class T> struct Args;
template <int C, int NB, int KA, int KB, bool UP, int COUT, int MODE, int KS2, int TH, bool AW, int NWT>
struct Args<C2fCfg<C, NB, KA, KB, UP, COUT, MODE, KS2, TH, AW, NWT>> {
  static void print() { printf("c2f_kernel %s %d %d %d %d %d %d %d %d %d %d %d\n", c2f_name(C2fCfg<C, NB, KA, KB, UP, COUT, MODE, KS2, TH, AW, NWT>::shape()).c_str(), C, NB, KA, KB, (int)UP, COUT, MODE, KS2, TH, (int)AW, NWT); }
};
template <int CIN, int COUT, int TH> struct Args<S2Cfg<CIN, COUT, TH>> {
  static void print() { printf("s2conv_kernel %s %d %d %d\n", s2_name(CIN, COUT, false).c_str(), CIN, COUT, TH); }
};
template <int CIN, int COUT, int TH, int OS, int KS, bool TAIL> struct Args<S2LCfg<CIN, COUT, TH, OS, KS, TAIL>> {
  static void print() { printf("s2lds_kernel %s %d %d %d %d %d %d\n", s2_name(CIN, COUT, TAIL).c_str(), CIN, COUT, TH, OS, KS, (int)TAIL); }
};
template <int C, int CIN, int COUT, int OS> struct Args<SpCfg<C, CIN, COUT, OS>> {
  static void print() { printf("sppf_kernel %s %d %d %d %d\n", sppf_name(CIN, C, COUT).c_str(), C, CIN, COUT, OS); }
};
struct PrintArgs {
  template <class CFG> bool operator()() const { Args<CFG>::print(); return false; }
};

int main() {
  char line[512];
  while (fgets(line, sizeof(line), stdin)) {
    C2fShape s;
    int h, w, cin, c, cout, cout2, tail;
    if (sscanf(line, "c2f %d %d %d %d %d %d %d %d %d %d", &s.C, &s.NB, &s.KA, &s.KB, &s.UP, &s.COUT, &s.MODE, &s.KS2, &h, &w) == 10) {
      const std::string name = c2f_kernel_name(s);
      printf("%d %s %d\n", (int)c2f_supported(s, h, w), name.empty() ? "-" : name.c_str(), (int)c2f_cv2_from_lds(s));
    } else if (sscanf(line, "c2fpack %d %d %d %d %d %d %d %d %d %d", &s.C, &s.NB, &s.KA, &s.KB, &s.UP, &s.COUT, &s.MODE, &s.KS2, &h, &w) == 10) {
      if (!c2f_supported(s, h, w)) { printf("0\n"); continue; }
      const int C = s.C, K1 = s.KA + s.KB;
      std::vector<float> t[18];
      const size_t n[18] = {(size_t)2 * C * K1, (size_t)2 * C, (size_t)C * 9 * C, (size_t)C, (size_t)C * 9 * C, (size_t)C, (size_t)C * 9 * C, (size_t)C, (size_t)C * 9 * C, (size_t)C,
                            (size_t)s.COUT * (2 + s.NB) * C, (size_t)s.COUT, (size_t)2 * C * 9 * s.KS2, (size_t)2 * C, (size_t)C * s.COUT, (size_t)C, (size_t)s.COUT * 4 * C, (size_t)s.COUT};
      for (int i = 0; i < 18; ++i) t[i] = fill(n[i], i + 1);
      C2fSrc src;
      src.cv1 = &t[0]; src.cv1_b = &t[1];
      for (int k = 0; k < 2; ++k) { src.a[k] = &t[2 + 4 * k]; src.a_b[k] = &t[3 + 4 * k]; src.bb[k] = &t[4 + 4 * k]; src.bb_b[k] = &t[5 + 4 * k]; }
      src.cv2 = &t[10]; src.cv2_b = &t[11]; src.s2 = &t[12]; src.s2_b = &t[13]; src.sp1 = &t[14]; src.sp1_b = &t[15]; src.sp2 = &t[16]; src.sp2_b = &t[17];
      const C2fPack p = pack_c2f(s, h, w, src);
      printf("1 ");
      print_row(*find_c2f(s));
      printf(" | %.0f |", p.macs_per_image);
      for (int i = 0; i < C2F_NW; ++i) { print_hash(p.w[i]); print_hash(p.b[i]); }
      printf("\n");
    } else if (sscanf(line, "s2 %d %d %d %d %d %d", &cin, &cout, &cout2, &tail, &h, &w) == 6) {
      printf("%d %d\n", (int)(tail ? s2_tail_supported(cin, cout, cout2, h, w) : s2_supported(cin, cout, h, w)), (int)s2_lds_staged(cin, cout));
    } else if (sscanf(line, "s2pack %d %d %d %d %d", &cin, &cout, &tail, &h, &w) == 5) {
      if (!(tail ? s2_tail_supported(cin, cout, cout, h, w) : s2_supported(cin, cout, h, w))) { printf("0\n"); continue; }
      const std::vector<float> wt = fill((size_t)cout * 9 * cin, 1), b = fill(cout, 2), w2 = fill((size_t)cout * cout, 3), b2 = fill(cout, 4);
      const S2Pack p = pack_s2(cin, cout, wt, b, tail ? &w2 : nullptr, tail ? &b2 : nullptr);
      printf("1 ");
      print_row(*find_s2(cin, cout, tail != 0));
      printf(" |");
      print_hash(p.w); print_hash(p.b); print_hash(p.w2); print_hash(p.b2);
      printf("\n");
    } else if (sscanf(line, "sppf %d %d %d %d %d", &cin, &c, &cout, &h, &w) == 5) {
      if (!sppf_supported(cin, c, cout, h, w)) { printf("0\n"); continue; }
      const std::vector<float> w1 = fill((size_t)c * cin, 1), b1 = fill(c, 2), w2 = fill((size_t)cout * 4 * c, 3), b2 = fill(cout, 4);
      const SppfPack p = pack_sppf(cin, c, cout, h, w, w1, b1, w2, b2);
      printf("1 ");
      print_row(sppf_row());
      printf(" | %.0f |", p.macs_per_image);
      print_hash(p.w1); print_hash(p.b1); print_hash(p.w2); print_hash(p.b2);
      printf("\n");
    } else if (strncmp(line, "rows", 4) == 0) {
      for (const C2fRow& r : c2f_rows()) { print_row(r); printf("\n"); }
      for (const S2Row& r : s2_rows()) { print_row(r); printf("\n"); }
      print_row(sppf_row());
      printf("\nend\n");
    } else if (strncmp(line, "table", 5) == 0) {
      for_each_cfg(PrintArgs{});
      for_each_s2cfg(PrintArgs{});
      Args<SppfCfg>::print();
      printf("end\n");
    } else {
      fprintf(stderr, "bad request: %s", line);
      return 2;
    }
  }
  return 0;
}
