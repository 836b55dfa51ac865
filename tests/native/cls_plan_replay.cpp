// Host replay of csrc/cls_plan.h, the geometry, limits, plan choice and weight preparation of the ShuffleNetV2 classifier
// (tests/test_cls_plan_cpu.py).  No input; stdout: one line "<case> = <values>" per case, in a fixed order:
//   geometry                       -> repeats, logical / half / padded-half widths and map side of each stage
//   pack_fused_pw COUT_P CIN_P NC  -> bytes fnv of the fragments.  NC = 0: a full [COUT_P][CIN_P] matrix; NC > 0: fc as load() pads
//                                     it, NC filled rows of COUT_P = class_pad(NC)
//   pack_cls_stem                  -> bytes fnv of the fragments, bytes fnv of the four bias cases
//   fold KIND                      -> co ci k, bytes fnv of w, bytes fnv of b; the BatchNorm has one zero-variance channel
//   expand_pw / expand_dw LAYOUT   -> bytes fnv of w, bytes fnv of b; LAYOUT = single (24 channels) or stageN as load() uses it:
//                                     s1 = a stride-1 block's view of the second half, in = the whole tensor as the next layer's input
//   lds_stage BFP / lds_head CIN_P NC_P, back_supports NC / head_supports CIN_P NC, plan PRECISION IMPL SWITCH
// Tensors: element i of tensor t is ((i * 7919 + 131 * t) mod 509 - 254) / 128; a variance is that value squared.
#include <cstdio>
#include <cstring>

#include "cls_plan.h"

using namespace lp;
using namespace lp::clsplan;

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

static Folded folded(int co, int ci, int k, int t) {
  Folded f;
  f.co = co; f.ci = ci; f.k = k;
  f.w = fill((size_t)co * ci * k * k, t);
  f.b = fill(co, t + 1);
  return f;
}
static Layout layout(int C, int half, int halfp) { Layout l; l.C = C; l.half = half; l.halfp = halfp; return l; }

static void fold_case(const char* kind, int co, int ci, int k) {
  std::vector<float> w = fill((size_t)co * ci * k * k, 1), g = fill(co, 2), be = fill(co, 3), mu = fill(co, 4), var = fill(co, 5);
  for (float& v : var) v = v * v;
  var[3] = 0.f;
  std::map<std::string, NamedTensor> sd;
  sd["c.weight"].data = w.data(); sd["c.weight"].shape = {co, ci, k, k};
  const char* names[4] = {"n.weight", "n.bias", "n.running_mean", "n.running_var"};
  const std::vector<float>* src[4] = {&g, &be, &mu, &var};
  for (int i = 0; i < 4; ++i) { sd[names[i]].data = src[i]->data(); sd[names[i]].shape = {co}; }
  const Folded f = fold(sd, "c", "n");
  printf("fold %s = %d %d %d", kind, f.co, f.ci, f.k);
  print_hash(f.w); print_hash(f.b);
  printf("\n");
}

static void expand_pw_case(const char* name, const Folded& f, const Layout& in, int in_first, int cout_p, int cin_p, int off) {
  std::vector<float> w, b;
  expand_pw(f, in, in_first, cout_p, w, b, cin_p, off);
  printf("expand_pw %s =", name);
  print_hash(w); print_hash(b);
  printf("\n");
}
static void expand_dw_case(const char* name, const Folded& f, const Layout& in, int cp) {
  std::vector<float> w, b;
  expand_dw(f, in, 0, cp, 0, w, b);
  printf("expand_dw %s =", name);
  print_hash(w); print_hash(b);
  printf("\n");
}

int main() {
  printf("geometry =");
  for (int s = 0; s < 3; ++s) printf(" %d %d %d %d %d", kStageRepeats[s], kStageOut[s], half_c(s), half_cp(s), stage_side(s));
  printf("\n");

  const int pairs[6][2] = {{64, 24}, {64, 64}, {128, 128}, {240, 256}, {240, 240}, {1024, 480}};
  for (const auto& p : pairs) {
    printf("pack_fused_pw %d %d 0 =", p[0], p[1]);
    print_hash(pack_fused_pw(fill((size_t)p[0] * p[1], 1), p[0], p[1]));
    printf("\n");
  }
  const int ncs[6] = {1, 2, 58, 91, 256, 560};
  for (int nc : ncs) {
    const int rows = (nc + 15) / 16 * 16;
    std::vector<float> w((size_t)rows * 1024, 0.f);
    const std::vector<float> src = fill((size_t)nc * 1024, 2);
    memcpy(w.data(), src.data(), src.size() * 4);
    printf("pack_fused_pw %d 1024 %d =", rows, nc);
    print_hash(pack_fused_pw(w, rows, 1024));
    printf("\n");
  }
  {
    std::vector<uint16_t> fr;
    std::vector<float> bc;
    pack_cls_stem(fill((size_t)24 * 27, 1), fill(24, 2), fr, bc);
    printf("pack_cls_stem =");
    print_hash(fr); print_hash(bc);
    printf("\n");
  }
  fold_case("3x3", 8, 4, 3);
  fold_case("1x1", 16, 24, 1);
  fold_case("depthwise", 24, 1, 3);

  const Layout single = layout(24, 0, 0);
  expand_pw_case("single", folded(58, 24, 1, 1), single, 0, 64, single.Cp(), 0);
  expand_dw_case("single", folded(24, 1, 3, 3), single, single.Cp());
  for (int s = 0; s < 3; ++s) {
    const int bf = half_c(s), bfp = half_cp(s), next = s < 2 ? half_cp(s + 1) : 1024, next_c = s < 2 ? half_c(s + 1) : 1024;
    const Layout l = layout(kStageOut[s], bf, bfp);
    char name[32];
    snprintf(name, sizeof(name), "stage%d.s1", s + 2);
    expand_pw_case(name, folded(bf, bf, 1, 5 + s), l, bf, bfp, bfp, bfp);
    snprintf(name, sizeof(name), "stage%d.in", s + 2);
    expand_pw_case(name, folded(next_c, kStageOut[s], 1, 8 + s), l, 0, next, l.Cp(), 0);
    expand_dw_case(name, folded(kStageOut[s], 1, 3, 11 + s), l, l.Cp());
  }

  for (int bfp : {64, 128, 240}) printf("lds_stage %d = %zu\n", bfp, fused_stage_lds_bytes(bfp));
  for (int ncp : {16, 64, 96, 256, 272}) printf("lds_head 480 %d = %zu\n", ncp, fused_head_lds_bytes(480, ncp));
  for (int nc : {1, 91, 559, 560, 561, 576, 1024, 1025}) printf("back_supports %d = %d\n", nc, (int)cls_back_supports(nc));
  for (int nc : {1, 91, 255, 256, 257, 272}) printf("head_supports 480 %d = %d\n", nc, (int)cls_head_supports(480, nc));
  printf("head_supports 484 91 = %d\n", (int)cls_head_supports(484, 91));
  const char* plans[3] = {"TWO_LAUNCH", "STAGE_FUSED", "LAYERWISE"};
  for (int prec : {(int)LP_FP32, (int)LP_FP16})
    for (int impl = 0; impl < 2; ++impl)
      for (int sw = 0; sw < 2; ++sw)
        printf("plan %s %d %d = %s\n", prec == LP_FP16 ? "fp16" : "fp32", impl, sw, plans[choose_plan(prec, impl, 64, sw != 0)]);
  return 0;
}
