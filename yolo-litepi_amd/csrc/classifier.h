// ShuffleNetV2 x1.0 classifier plan (host side).  Replaces build_classifier('shufflenetv2')
// + self.model(batch) of the reference (e2e.py:331-333,393).
#pragma once
#include "common.h"
#include "conv.h"
#include "detector.h"
#include "cls_fused.h"
#include "cls_net.h"
#include "cls_plan.h"   // NamedTensor, the network's geometry, the plan kinds
#include "kernels.h"

namespace lp {

// where a classifier that finishes with softmax / arg-max itself (fused head) puts the results
struct ClsPost { float* probs = nullptr; int* ids = nullptr; lp_det* dets = nullptr; int max_det = 0; const int* roi_img = nullptr; const int* roi_slot = nullptr; };

// What the pipeline needs from a classifier architecture (build_classifier(arch, ..), e2e.py:320-333)
class ClassifierBase {
 public:
  typedef ClsPost Post;
  virtual ~ClassifierBase() {}
  virtual void load(const std::map<std::string, NamedTensor>& sd) = 0;   // torchvision state_dict of the architecture
  virtual bool loaded() const = 0;
  virtual int num_classes() const = 0;
  virtual int logits_pitch() const = 0;
  virtual const float* logits() const = 0;
  // rgb: device uint8 [R,S,S,3]; d_R: device ROI count.  Leaves fp32 logits [R, logits_pitch()].
  // With a fused head softmax/arg-max/scatter happen inside forward(); post describes where the results go.
  // fused_head() tells the caller whether it still has to run softmax itself.
  virtual bool fused_head() const = 0;
  virtual void forward(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post = nullptr) = 0;
};

// load() chooses ONE plan (clsplan::choose_plan; LITEPI_CLS_LAYERWISE is read there, once per load) and builds that plan's
// weights, buffers and kernel argument blocks and nothing else; forward() fills in the crop, the ROI count and the output block.
class Classifier : public ClassifierBase {
 public:
  Classifier(int prec, int impl, int max_rois, int num_classes, int input_size);
  // torchvision shufflenet_v2_x1_0 state_dict (fc replaced by Linear(1024, num_classes))
  void load(const std::map<std::string, NamedTensor>& sd) override;
  bool loaded() const override { return loaded_; }
  int num_classes() const override { return ncls_; }
  int logits_pitch() const override { return lpitch_; }
  const float* logits() const override { return d_logits_.as<float>(); }
  bool fused_head() const override { return plan_ != clsplan::LAYERWISE; }
  void forward(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post = nullptr) override;

 private:
  struct DwLayer { DevBuf w, b; int C = 0, stride = 1; std::string name; };
  struct Block {
    int b1_dw = -1, b1_pw = -1;          // stride 2 only
    int b2_pw1 = -1, b2_dw = -1, b2_pw2 = -1;
  };
  struct Act { DevBuf mem; int C = 0, H = 0, W = 0; };   // [max_rois,H,W,C]
  struct FusedW { DevBuf w1, b1, dw, dwb, w2, b2; };                                    // a stride-1 block of the fused kernels
  struct FusedS2 { DevBuf dw1, dw1b, pwb1, pwb1b, pw1, pw1b, dw2, dw2b, pw2, pw2b; };   // a stride-2 block of cls_front / cls_back
  // everything load() builds: the chosen plan's members are filled, the others stay empty
  struct Built {
    // layer at a time (LAYERWISE: every layer; STAGE_FUSED: stem, maxpool and the stride-2 blocks)
    std::vector<std::unique_ptr<ConvLayer>> pws;
    std::vector<DwLayer> dws;
    Block s2[clsplan::kStages];                // the stage's stride-2 block
    std::vector<Block> s1[clsplan::kStages];   // its stride-1 blocks (LAYERWISE)
    DevBuf stem_w, stem_b;
    int conv5 = -1, fc = -1;
    Act a_stem, a_pool, a_t1, a_t2, a_b1dw, a_b1, a_stage[clsplan::kStages][2], a_conv5, a_mean;
    // fused kernels (TWO_LAUNCH, STAGE_FUSED)
    std::vector<FusedW> fused[clsplan::kStages];
    DevBuf head_w5, head_b5, head_wfc, head_bfc;
    FusedStageArgs stage[clsplan::kStages];
    FusedHeadArgs head;
    // cls_front / cls_back (TWO_LAUNCH)
    FusedS2 fused_s2[clsplan::kStages];
    DevBuf stem_frag, stem_bias4, a_x3;
    ClsFrontArgs front;
    ClsBackArgs back;
  };
  View act_view(const Act& a) const;
  void alloc_act(Act& a, int C, int H, int W);
  int add_pw(const std::string& name, const std::vector<float>& w_phys, const std::vector<float>& b_phys, int cin, int cout, int act, int hw);
  int add_dw(const std::string& name, const std::vector<float>& w_phys, const std::vector<float>& b_phys, int C, int stride);
  ClsOut out_block(const Post* post) const;
  void forward_two_launch(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post);
  void forward_layers(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post);

  int prec_, impl_, maxR_, ncls_, S_, lpitch_ = 0;
  bool loaded_ = false;
  clsplan::Plan plan_ = clsplan::LAYERWISE;
  Built b_;
  DevBuf d_logits_;
};

}  // namespace lp
