// Host-side handles of the convolution kernels (conv_kernels.hip).
#pragma once
#include "common.h"
#include "conv_plan.h"

namespace lp {

struct ConvIO {
  View in, out, res, x1;
  View up;                     // 1x1 only: half-resolution source of the leading up.C input channels (fused Interp x2 + Concat)
  int N = 0;
  const int* m_dyn = nullptr;  // device scalar item count (classifier); M = *m_dyn * out.H * out.W
  int half_c = 0, half_cp = 0; // shuffle epilogue geometry (x1.base != nullptr)
  int out_f32 = 0;
  int res_first = 0;           // residual added BEFORE the activation (ResNet) instead of after it (C2f)
  unsigned long long* stamps = nullptr;  // diagnostic (see ConvArgs::stamps)
};

// One Convolution(+bias)(+activation)(+residual) layer with its device weights, packed for
// the kernel family chosen at build time.  The MFMA tiling (NT, nsplits, CK, .., direct) is cplan::plan_conv's result.
struct ConvLayer : cplan::ConvTiling {
  int prec = LP_FP16, impl = IMPL_MFMA;
  int k = 1, stride = 1, Cin = 0, Cout = 0, act = ACT_NONE;
  DevBuf d_w, d_bias;
  // fused 1x1 tail conv (second GEMM in the epilogue): 0 = none, else its 16-channel output tiles
  int T2 = 0, Cout2 = 0, act2 = ACT_NONE;
  DevBuf d_w2, d_bias2;
  std::string name;
  // host copies of the physical fp32 weights (build / attach_tail arguments): the Detect-head fusion re-packs them into
  // one weight stream (HeadLayer); a few MB per model
  std::vector<float> w_host, b_host, w2_host, b2_host;
  double macs_per_pixel() const { return (double)k * k * Cin * Cout; }

  // w_phys: fp32 [Cout][k*k][Cin] over PHYSICAL channels (zeros at padding channels);
  // bias_phys: fp32 [Cout] or empty.  hout/wout: output map size and batch_hint: images (or ROIs)
  // per call at capacity -- together they pick the tile shape and the channel split.
  void build(int prec, int impl, int k, int stride, int cin, int cout, int act,
             const std::vector<float>& w_phys, const std::vector<float>& bias_phys, int hout, int wout, int batch_hint,
             bool full_n = false, bool single_chunk = false);
  // Fuse a following 1x1 conv (weights w2_phys [cout2][Cout] over physical channels) into this 3x3 layer.
  // Requires build(..., full_n = true) (one workgroup holds every intermediate channel).  The fused layer's
  // output view then has cout2 channels.
  static bool tail_supported(int k, int stride, int cmid_phys, int cout2_phys) { return cplan::conv_tail_supported(k, stride, cmid_phys, cout2_phys); }
  void attach_tail(int cout2_phys, int act2, const std::vector<float>& w2_phys, const std::vector<float>& bias2_phys);
  void launch(const ConvIO& io, hipStream_t st) const;
  // profile names: the kernel family, and one name per instantiation (channel tiles NT, tail tiles T2, fused-upsample variant,
  // as rocprofv3 lists them), both without the precision suffix
  const char* family_name() const { return impl == IMPL_NAIVE ? "conv_naive" : direct ? "conv3x3s2_direct" : k == 3 ? "conv3x3_mfma" : "conv1x1_mfma"; }
  std::string kernel_name(bool up = false) const;
};

// C2f bottleneck x + silu(conv3x3(silu(conv3x3(x)))) as ONE launch (bottleneck_mfma_kernel): the
// intermediate lives in LDS.  The two ConvLayers only carry the packed weights (all of K in one chunk).
// The tile, its LDS size and the cv2 tail's shape (TH, TW, LW, lds_bytes, T2, kg, sg, cl, PSA) are cplan::plan_bneck's result.
struct BottleneckPair : cplan::BneckTiling {
  ConvLayer a, b;
  int prec = LP_FP16, C = 0, NT = 1, PS = 0, CG = 0, steps = 0;
  unsigned rcp_cg = 0, rcp_ps = 0, rcp_pcs = 0, rcp_w1 = 0, rcp_tw = 0;
  std::string name;
  // optional fused C2f.cv2 (1x1 over concat[stored segments .., y_last]); y_last = this bottleneck's output.  The base holds
  // what the plan depends on: cat_global = physical channels of the concat that precede y_last (read from the concat buffer),
  // c3 = cv2's physical output channels, in_is_last_stored (same buffer and pitch; C2f: y_n), and the planner's cl switch
  struct Cv2 : cplan::BneckTail {
    int act = ACT_NONE;
    const std::vector<float>* w = nullptr;  // fp32 [c3][cat_global + C] over physical concat channels
    const std::vector<float>* bias = nullptr;
  };
  int C3 = 0, act3 = ACT_NONE;
  DevBuf d_w3, d_b3;
  // can a C->C bottleneck on an h x w map (batch_hint images) run fused?  (LDS capacity, tile limits); cv2 = nullptr: without tail
  static bool supported(int prec, int impl, int c_phys, int h, int w, int batch_hint, const Cv2* cv2 = nullptr) {
    return impl == IMPL_MFMA && cplan::plan_bneck(prec, c_phys, h, w, batch_hint, cv2).ok;
  }
  // weights as for ConvLayer::build: fp32 [C][9][C] over physical channels, bias [C]
  void build(int prec, int c_phys, const std::vector<float>& wa, const std::vector<float>& ba, const std::vector<float>& wb,
             const std::vector<float>& bb, int h, int w, int batch_hint, const Cv2* cv2 = nullptr);
  // without cv2: out = bottleneck output.  With cv2: cat = the concat buffer view (its leading cat_global channels are read),
  // out = cv2's output view; the bottleneck output itself is not stored.
  void launch(const View& in, const View& out, int N, hipStream_t st, const View* cat = nullptr) const;
  // one name per kernel instantiation <NT, P1, P2, T2, SG> (what rocprofv3 lists as separate kernels), without the precision suffix
  std::string kernel_name() const;
};

// First layer: 3x3 stride-2 conv reading the uint8 BGR image directly.
struct StemLayer {
  int prec = LP_FP16, CO = 8, act = ACT_SILU;
  int k = 3, stride = 2, pad = 1;  // YOLOv8 family: 3x3/s2/p1 (fast kernels); anything else runs the generic kernel
  DevBuf d_w, d_bias;
  DevBuf d_afrag;  // fp16, 8 channels: MFMA A fragments (stem_mfma_kernel)
  DevBuf d_afrag_blk;  // the same weights in stem_block_kernel's K-group order
  // w_bgr: fp32 [k*k*3][CO], row = (ky*k+kx)*3 + c with c in BGR order
  void build(int prec, int cout_phys, int act, const std::vector<float>& w_bgr, const std::vector<float>& bias, int k = 3, int stride = 2,
             int pad = 1);
  void launch(const uint8_t* img, int N, int Hin, int Win, const View& out, hipStream_t st) const;
  // stem + the following stride-2 3x3 conv (+ its fused 1x1 tail) in one launch (stem_block_kernel); out = the tail's output
  bool block_supported(const ConvLayer& c1) const;
  const char* kernel_name(bool block) const { return !block ? "stem_conv" : CO == 16 ? "stem_block16" : "stem_block"; }
  void launch_block(const uint8_t* img, int N, int Hin, int Win, const ConvLayer& c1, const View& out, hipStream_t st) const;
};

}  // namespace lp
