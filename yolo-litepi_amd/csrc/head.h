// Fused Detect head of one pyramid level (head_kernels.hip): host-side declarations.
// Replaces, per level, the six convolutions of Ultralytics' Detect (box tower cv2[i] = 3x3 -> 3x3 -> 1x1 (4*reg_max),
// class tower cv3[i] = 3x3 -> 3x3 -> 1x1 (nc); reference graph model.ncnn.param:151-182) AND the decode tail
// (Reshape/Permute/Softmax/DFL conv/dist2bbox/Sigmoid, :184-208) + conf filter of postprocess (e2e.py:255-278).
#pragma once
#include "common.h"
#include "head_plan.h"
#include "kernels.h"

namespace lp {

struct HeadArgs {
  const void* in;          // neck feature map F [N][H][W][in_pitch] fp16
  const void* wstream;     // 1 KiB MFMA A fragments in consumption order (hplan::pack_head)
  const float* biasA;      // [32 * RT]  first 3x3 convs: box tower 64 | class tower 32*C3T (zero padded)
  const float* biasB;      // [32 * RT]  second 3x3 convs
  const float* biasC;      // [64 + 32]  projections: 4 x 16 DFL logits | class logits (zero padded to 32)
  const void* zeros;       // >= 16 zero bytes
  const float* anchors;    // [2][A] grid units
  const float* strides;    // [A]
  const float* dfl_w;      // [16]
  float* out0;             // optional [N][4+nc][A]
  const ImgGeom* geom;     // [N]
  Cand* cand;              // [N][A]
  int* cand_count;         // [N]
  float conf;
  int N, H, W, in_pitch, Cin;
  int TH, TW, tiles_x, ntiles;
  int KPT;                 // K steps (of 16 channels) per 3x3 tap of the first convs = Cin / 16
  int nchunks;             // weight-stream chunks
  int A, nc, anchor_off;
  int flags;               // experiment switches (HeadSwitches::flags, LITEPI_HEAD_FLAGS): 1 = s_setprio 1 in the K loops, 2 = s_setprio 1 in the epilogues
  unsigned long long* stamps;  // diagnostic only (LITEPI_HEAD_STAMPS=<file>): 16 clock stamps per workgroup
};

// One level's plan (head_plan.h) and its weights re-packed for head_fused_kernel.
struct HeadLayer : hplan::HeadPlan {
  using Src = hplan::Src;
  int H = 0, W = 0;        // the level's map: launch() checks the view against it
  int flags = 0;           // HeadSwitches::flags of the load that built the layer
  DevBuf d_stream, d_biasA, d_biasB, d_biasC;
  std::string name;
  double macs_per_image = 0;
  static bool supported(int cin_phys, int c2, int c3, int nc, int reg_max, const hplan::HeadSwitches& sw) {
    return hplan::plan_head(cin_phys, c2, c3, nc, reg_max, sw).ok;
  }
  void build(int cin_phys, int c3, int nc, int h, int w, const hplan::HeadSwitches& sw, const Src& s);   // plan, pack, upload
  std::string kernel_name() const { return hplan::kernel_name(hplan::kHeadVariants[variant]); }
  // anchor_off: index of the level's first anchor; out0 may be null
  void launch(const View& in, int N, int anchor_off, int A, const float* anchors, const float* strides, const float* dfl_w, float* out0,
              const ImgGeom* geom, Cand* cand, int* cand_count, float conf, hipStream_t st) const;
};

}  // namespace lp
