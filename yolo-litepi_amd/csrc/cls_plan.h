// ShuffleNetV2 x1.0 classifier: geometry, limits, plan choice and weight preparation (classifier.cpp, cls_net.hip,
// cls_fused.hip).  Host-only and pure: no HIP, no allocation on a device, no environment -- a plain C++ compiler builds it,
// and tests/native/cls_plan_replay.cpp replays it against a recording (tests/golden/cls_plans.json).  This header is the only
// place that knows the network's widths, the A-fragment format of the fused kernels and how many classes each of them takes.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "error.h"
#include "f16.h"

namespace lp {

struct NamedTensor {
  const float* data = nullptr;
  std::vector<int64_t> shape;
  size_t numel() const { size_t n = 1; for (auto d : shape) n *= (size_t)d; return n; }
};

namespace clsplan {

constexpr int rup(int x, int m) { return (x + m - 1) / m * m; }

// ---- geometry (torchvision shufflenet_v2_x1_0) --------------------------------------------------
// 64x64 crop -> conv1 3x3/s2 (24 ch, 32x32) -> maxpool 3x3/s2 (16x16) -> stages 2..4 -> conv5 1x1 (1024) -> mean -> fc.
// A stage tensor is two channel halves, each padded to a multiple of 16: [x_lo | pad | x_hi | pad].
constexpr int kInput = 64, kStemC = 24, kConv5C = 1024, kStages = 3;
constexpr int kStageRepeats[kStages] = {4, 8, 4};     // blocks per stage; the first has stride 2
constexpr int kStageOut[kStages] = {116, 232, 464};   // logical channels
constexpr int stage_in(int s) { return s == 0 ? kStemC : kStageOut[s - 1]; }
constexpr int half_c(int s) { return kStageOut[s] / 2; }
constexpr int half_cp(int s) { return rup(half_c(s), 16); }
constexpr int stage_cp(int s) { return 2 * half_cp(s); }                          // physical channels of the stage tensor
constexpr int stage_in_cp(int s) { return s == 0 ? rup(kStemC, 8) : stage_cp(s - 1); }
constexpr int kStemSide = kInput / 2, kPoolSide = kInput / 4;
constexpr int stage_side(int s) { return kPoolSide >> (s + 1); }                  // 8, 4, 2
static_assert(half_c(0) == 58 && half_cp(0) == 64 && half_c(1) == 116 && half_cp(1) == 128 && half_c(2) == 232 && half_cp(2) == 240,
              "the fused classifier kernels are built for ShuffleNetV2 x1.0 widths");
static_assert(stage_side(0) == 8 && stage_side(2) == 2 && stage_cp(2) == 480, "ShuffleNetV2 x1.0 at 64x64");

// ---- limits ---------------------------------------------------------------------------------------------------------
constexpr size_t kLdsMax = 160 * 1024;
constexpr int kFusedPix = 64;              // pixels per workgroup of shuffle_stage_kernel and cls_head_kernel
constexpr int kBackRois = 4, kHeadRois = 16;   // ROIs per workgroup pass of cls_back / cls_head_fused
constexpr int kMeanRow = kConv5C * 2 + 16; // bytes per ROI of the fp16 mean image (the fc operand), padded like every LDS row
constexpr int kBackRC = 17408;             // cls_back's LDS region that ends as [4 ROIs] mean | [4][nc_p] fp32 logits
constexpr int class_pad(int nc) { return rup(nc, 16); }   // fc rows of the fused kernels = pitch of the logits
constexpr size_t fused_stage_lds_bytes(int bfp) { return (size_t)kFusedPix * ((2 * bfp * 2 + 16) + 2 * (bfp * 2 + 16)); }
constexpr size_t fused_head_lds_bytes(int cin_p, int nc_p) {
  return (size_t)kFusedPix * (cin_p * 2 + 16) + (size_t)kHeadRois * kMeanRow + (size_t)kHeadRois * nc_p * 4;
}
// cls_back keeps 4 ROIs' logits behind their means in kBackRC: up to 560 classes
constexpr bool cls_back_supports(int nc) {
  return nc >= 1 && class_pad(nc) <= 1024 && (size_t)kBackRois * kMeanRow + (size_t)kBackRois * class_pad(nc) * 4 <= (size_t)kBackRC;
}
// cls_head_fused gives each of its 16 waves one 16-class fc tile: up to 256 classes
constexpr bool cls_head_supports(int cin_p, int nc) {
  return nc >= 1 && class_pad(nc) <= 16 * 16 && cin_p % 8 == 0 && fused_head_lds_bytes(cin_p, class_pad(nc)) <= kLdsMax;
}
constexpr bool fused_stage_supports(int bfp, int HW, int group) {
  return fused_stage_lds_bytes(bfp) <= kLdsMax && bfp % 16 == 0 && HW > 0 && kFusedPix % HW == 0 && group * HW == kFusedPix;
}

// ---- plan -----------------------------------------------------------------------------------------------------------
enum Plan {
  TWO_LAUNCH,    // cls_front + cls_back (cls_net.hip)
  STAGE_FUSED,   // stem, maxpool and stride-2 blocks one kernel per layer; stride-1 blocks of a stage and the head fused (cls_fused.hip)
  LAYERWISE,     // one kernel per layer, softmax by the caller
};
// layerwise_switch: LITEPI_CLS_LAYERWISE is set (read by Classifier::load, once per load)
constexpr Plan choose_plan(int precision, int conv_impl, int input, bool layerwise_switch) {
  return precision == LP_FP16 && conv_impl == 0 /* IMPL_MFMA */ && input == kInput ? (layerwise_switch ? STAGE_FUSED : TWO_LAUNCH) : LAYERWISE;
}

// ---- weight preparation ---------------------------------------------------------------------------------------------
struct Folded { std::vector<float> w, b; int co = 0, ci = 0, k = 1; };  // w [co][ci][k*k]

inline const NamedTensor& need(const std::map<std::string, NamedTensor>& sd, const std::string& key) {
  auto it = sd.find(key);
  LP_CHECK(it != sd.end() && it->second.data, LP_ERR_ARG, "classifier state_dict lacks %s", key.c_str());
  return it->second;
}

// conv (no bias) + BatchNorm(eval, eps 1e-5) -> conv with bias
inline Folded fold(const std::map<std::string, NamedTensor>& sd, const std::string& conv, const std::string& bn) {
  const NamedTensor& W = need(sd, conv + ".weight");
  LP_CHECK(W.shape.size() == 4, LP_ERR_ARG, "%s.weight must be 4-D", conv.c_str());
  Folded f;
  f.co = (int)W.shape[0]; f.ci = (int)W.shape[1]; f.k = (int)W.shape[2];
  const int kk = f.k * f.k;
  const NamedTensor& g = need(sd, bn + ".weight");
  const NamedTensor& be = need(sd, bn + ".bias");
  const NamedTensor& mu = need(sd, bn + ".running_mean");
  const NamedTensor& var = need(sd, bn + ".running_var");
  LP_CHECK((int)g.numel() == f.co && (int)be.numel() == f.co && (int)mu.numel() == f.co && (int)var.numel() == f.co, LP_ERR_ARG,
           "%s: BatchNorm size mismatch", bn.c_str());
  f.w.resize((size_t)f.co * f.ci * kk);
  f.b.resize(f.co);
  for (int o = 0; o < f.co; ++o) {
    const double s = (double)g.data[o] / std::sqrt((double)var.data[o] + 1e-5);
    for (int i = 0; i < f.ci * kk; ++i) f.w[(size_t)o * f.ci * kk + i] = (float)(W.data[(size_t)o * f.ci * kk + i] * s);
    f.b[o] = (float)((double)be.data[o] - (double)mu.data[o] * s);
  }
  return f;
}

// channel layout of a stage tensor: logical c -> physical
struct Layout {
  int C = 0, half = 0, halfp = 0;  // half == 0: single contiguous segment
  int Cp() const { return half ? 2 * halfp : rup(C, 8); }
  int phys(int c) const { return (!half || c < half) ? c : halfp + (c - half); }
};
inline Layout single_layout(int C) { Layout l; l.C = C; return l; }
inline Layout stage_layout(int s) { Layout l; l.C = kStageOut[s]; l.half = half_c(s); l.halfp = half_cp(s); return l; }

// pointwise weights over physical channels: rows = out layout (single segment, padded), cols = in layout
inline void expand_pw(const Folded& f, const Layout& in, int in_first, int cout_p, std::vector<float>& w, std::vector<float>& b,
                      int cin_p, int in_view_off) {
  w.assign((size_t)cout_p * cin_p, 0.f);
  b.assign(cout_p, 0.f);
  for (int o = 0; o < f.co; ++o) {
    for (int i = 0; i < f.ci; ++i) w[(size_t)o * cin_p + (in.phys(in_first + i) - in_view_off)] = f.w[(size_t)o * f.ci + i];
    b[o] = f.b[o];
  }
}

inline void expand_dw(const Folded& f, const Layout& in, int in_first, int cp, int in_view_off, std::vector<float>& w, std::vector<float>& b) {
  w.assign((size_t)9 * cp, 0.f);
  b.assign(cp, 0.f);
  for (int c = 0; c < f.co; ++c) {
    const int pc = in.phys(in_first + c) - in_view_off;
    for (int t = 0; t < 9; ++t) w[(size_t)t * cp + pc] = f.w[(size_t)c * 9 + t];
    b[pc] = f.b[c];
  }
}

// A fragments of a pointwise conv over PHYSICAL channels: [tile][step][lane][8 halfs];
// tile t row m = output channel 16t+m, K group q = 4s+g = input channels [8q, 8q+8).
inline std::vector<uint16_t> pack_fused_pw(const std::vector<float>& w_phys, int cout_p, int cin_p) {
  const int Tt = cout_p / 16, S = (cin_p + 31) / 32;
  std::vector<uint16_t> buf((size_t)Tt * S * 64 * 8, 0);
  for (int t = 0; t < Tt; ++t)
    for (int s = 0; s < S; ++s)
      for (int lane = 0; lane < 64; ++lane) {
        const int g = lane >> 4, m = lane & 15;
        const int oc = t * 16 + m;
        for (int j = 0; j < 8; ++j) {
          const int ci = (4 * s + g) * 8 + j;
          if (ci < cin_p) buf[(((size_t)t * S + s) * 64 + lane) * 8 + j] = f32_to_f16(w_phys[(size_t)oc * cin_p + ci]);
        }
      }
  return buf;
}

// conv1 (+BN) for cls_front's MFMA stem: w [24][3][3][3] (torch layout, BN folded), bias [24] -> A fragments [2 tiles][64 lanes]
// [8 halfs] + four bias cases [4][32].  K index of lane group g, element j: g < 3: window row ky = g, byte j = kx*3 + c (j < 8);
// g = 3: j < 3: the 9th byte (kx = 2, c = 2) of window row ky = j; rest zero.
inline void pack_cls_stem(const std::vector<float>& w, const std::vector<float>& bias, std::vector<uint16_t>& frags, std::vector<float>& bias_cases) {
  const double scale = 1.0 / 255.0 / 0.34, shift = 0.18 / 0.34;
  frags.assign((size_t)2 * 64 * 8, 0);
  for (int t = 0; t < 2; ++t)
    for (int lane = 0; lane < 64; ++lane) {
      const int gq = lane >> 4, m = lane & 15, co = t * 16 + m;
      if (co >= 24) continue;
      for (int j = 0; j < 8; ++j) {
        int ky, kb;
        if (gq < 3) { ky = gq; kb = j; }
        else if (j < 3) { ky = j; kb = 8; }
        else continue;
        const int kx = kb / 3, c = kb % 3;
        frags[((size_t)t * 64 + lane) * 8 + j] = f32_to_f16((float)((double)w[(((size_t)co * 3 + c) * 3 + ky) * 3 + kx] * scale));
      }
    }
  bias_cases.assign((size_t)4 * 32, 0.f);
  for (int ci = 0; ci < 4; ++ci)
    for (int co = 0; co < 24; ++co) {
      double s = 0.0;
      for (int ky = 0; ky < 3; ++ky)
        for (int kx = 0; kx < 3; ++kx) {
          if ((ci & 1) && ky == 0) continue;  // top row of the window is above the image
          if ((ci & 2) && kx == 0) continue;  // left column is left of the image
          for (int c = 0; c < 3; ++c) s += (double)w[(((size_t)co * 3 + c) * 3 + ky) * 3 + kx];
        }
      bias_cases[(size_t)ci * 32 + co] = (float)((double)bias[co] - shift * s);
    }
}

}  // namespace clsplan
}  // namespace lp
