// ShuffleNetV2 x1.0 on the GPU.  BatchNorm (eval mode, eps 1e-5) is folded into the preceding
// convolution at load time.  Every stage tensor is stored as two channel halves, each padded to
// a multiple of 16 channels: [x_lo | pad | x_hi | pad]; x.chunk(2) is then two aligned channel
// views, and channel_shuffle(cat(x1, branch2(x2)), 2) is fused into the epilogue of branch2's
// last pointwise conv (conv_kernels.hip, EPI_SHUFFLE), which also copies the pass-through half.
// The network's widths, the weight preparation and the choice of plan are cls_plan.h's.
#include "classifier.h"

#include <algorithm>
#include <cstdlib>

namespace lp {

using namespace clsplan;

Classifier::Classifier(int prec, int impl, int max_rois, int num_classes, int input_size)
    : prec_(prec), impl_(impl), maxR_(max_rois), ncls_(num_classes), S_(input_size) {}

static View make_view(const DevBuf& buf, size_t es, int coff, int C, int pitch, int H, int W) {
  View v;
  v.base = static_cast<char*>(buf.p) + (size_t)coff * es;
  v.C = C; v.pitch = pitch; v.H = H; v.W = W;
  return v;
}

View Classifier::act_view(const Act& a) const { return make_view(a.mem, prec_ == LP_FP16 ? 2 : 4, 0, a.C, a.C, a.H, a.W); }

void Classifier::alloc_act(Act& a, int C, int H, int W) {
  a.C = C; a.H = H; a.W = W;
  a.mem.alloc((size_t)maxR_ * H * W * C * (prec_ == LP_FP16 ? 2 : 4));
}

int Classifier::add_pw(const std::string& name, const std::vector<float>& w, const std::vector<float>& b, int cin,
                       int cout, int act, int hw) {
  b_.pws.emplace_back(new ConvLayer());
  b_.pws.back()->name = name;
  b_.pws.back()->build(prec_, impl_, 1, 1, cin, cout, act, w, b, hw, hw, std::min(maxR_, 512));
  return (int)b_.pws.size() - 1;
}

static void upload_f32(DevBuf& d, const std::vector<float>& v) {
  d.alloc((v.size() + 16) * 4);
  LP_HIP(hipMemcpy(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
}
static void upload_u16(DevBuf& d, const std::vector<uint16_t>& v) {
  d.alloc(v.size() * 2);
  LP_HIP(hipMemcpy(d.p, v.data(), v.size() * 2, hipMemcpyHostToDevice));
}

int Classifier::add_dw(const std::string& name, const std::vector<float>& w, const std::vector<float>& b, int C, int stride) {
  b_.dws.emplace_back();
  DwLayer& d = b_.dws.back();
  d.name = name; d.C = C; d.stride = stride;
  d.w.alloc(w.size() * 4);
  LP_HIP(hipMemcpy(d.w.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
  d.b.alloc(b.size() * 4);
  LP_HIP(hipMemcpy(d.b.p, b.data(), b.size() * 4, hipMemcpyHostToDevice));
  return (int)b_.dws.size() - 1;
}

void Classifier::load(const std::map<std::string, NamedTensor>& sd) {
  loaded_ = false;
  b_ = Built();
  // the reference resizes every ROI to 64x64 whatever --cls_input_size says (transforms.Resize((64, 64)), e2e.py:367)
  LP_CHECK(S_ == kInput, LP_ERR_ARG, "classifier input size must be 64 (the reference's transform is fixed at 64x64)");
  // A/B switch, read once per load: the stage-fused plan of round 2 in place of the two launches
  plan_ = choose_plan(prec_, impl_, S_, getenv("LITEPI_CLS_LAYERWISE") != nullptr);
  const bool two = plan_ == TWO_LAUNCH;       // cls_front + cls_back
  const bool fusedk = plan_ != LAYERWISE;     // stride-1 blocks and the head run in fused kernels
  const bool layers = plan_ != TWO_LAUNCH;    // stem, maxpool and the stride-2 blocks run one kernel per layer
  const bool s1layers = plan_ == LAYERWISE;   // and so do the stride-1 blocks, conv5, the mean and fc
  auto s1w = [](const FusedW& f) {
    return FusedBlockW{f.w1.as<u32x4_t>(), f.b1.as<float>(), f.dw.as<float>(), f.dwb.as<float>(), f.w2.as<u32x4_t>(), f.b2.as<float>()};
  };
  auto s2w = [](const FusedS2& f) {
    return FusedS2W{f.dw1.as<float>(), f.dw1b.as<float>(), f.pwb1.as<u32x4_t>(), f.pwb1b.as<float>(), f.pw1.as<u32x4_t>(),
                    f.pw1b.as<float>(), f.dw2.as<float>(), f.dw2b.as<float>(), f.pw2.as<u32x4_t>(), f.pw2b.as<float>()};
  };

  // conv1 + BN -> fp32 [27][24], RGB order (cls_stem) / MFMA fragments (cls_front)
  {
    Folded f = fold(sd, "conv1.0", "conv1.1");
    LP_CHECK(f.co == kStemC && f.ci == 3 && f.k == 3, LP_ERR_ARG, "conv1 must be 3->24 3x3");
    if (layers) {
      std::vector<float> w((size_t)27 * 24);
      for (int o = 0; o < 24; ++o)
        for (int c = 0; c < 3; ++c)
          for (int t = 0; t < 9; ++t) w[(size_t)(t * 3 + c) * 24 + o] = f.w[((size_t)o * 3 + c) * 9 + t];
      b_.stem_w.alloc(w.size() * 4);
      LP_HIP(hipMemcpy(b_.stem_w.p, w.data(), w.size() * 4, hipMemcpyHostToDevice));
      b_.stem_b.alloc(24 * 4);
      LP_HIP(hipMemcpy(b_.stem_b.p, f.b.data(), 24 * 4, hipMemcpyHostToDevice));
      alloc_act(b_.a_stem, kStemC, kStemSide, kStemSide);
      alloc_act(b_.a_pool, kStemC, kPoolSide, kPoolSide);
    }
    if (two) {
      std::vector<uint16_t> fr;
      std::vector<float> bc;
      pack_cls_stem(f.w, f.b, fr, bc);
      upload_u16(b_.stem_frag, fr);
      upload_f32(b_.stem_bias4, bc);
    }
  }

  Layout lin = single_layout(kStemC);
  size_t t1_elems = 0, t2_elems = 0, b1dw_elems = 0, b1_elems = 0;
  int inp = kStemC;
  for (int s = 0; s < kStages; ++s) {
    const int bf = half_c(s), bfp = half_cp(s);
    const Layout lout = stage_layout(s), lmid = single_layout(bf);
    const int Ho = stage_side(s), Hin = 2 * Ho;
    for (int r = 0; r < kStageRepeats[s]; ++r) {
      const int stride = r == 0 ? 2 : 1;
      const bool as_layers = stride == 2 ? layers : s1layers;
      const std::string p = fmt("stage%d.%d.", s + 2, r);
      Block B;
      FusedS2& f2 = b_.fused_s2[s];
      std::vector<float> w, b;
      if (stride == 2) {
        // branch1: dw(s2) on all input channels -> pw inp->bf + ReLU
        Folded d = fold(sd, p + "branch1.0", p + "branch1.1");
        LP_CHECK(d.co == inp && d.ci == 1 && d.k == 3, LP_ERR_ARG, "%sbranch1.0 shape", p.c_str());
        expand_dw(d, lin, 0, lin.Cp(), 0, w, b);
        if (layers) B.b1_dw = add_dw(p + "branch1.0", w, b, lin.Cp(), 2);
        if (two) { upload_f32(f2.dw1, w); upload_f32(f2.dw1b, b); }
        Folded q = fold(sd, p + "branch1.2", p + "branch1.3");
        LP_CHECK(q.co == bf && q.ci == inp && q.k == 1, LP_ERR_ARG, "%sbranch1.2 shape", p.c_str());
        expand_pw(q, lin, 0, bfp, w, b, lin.Cp(), 0);
        if (layers) B.b1_pw = add_pw(p + "branch1.2", w, b, lin.Cp(), bfp, ACT_RELU, Ho);
        if (two) { upload_u16(f2.pwb1, pack_fused_pw(w, bfp, lin.Cp())); upload_f32(f2.pwb1b, b); }
        // branch2: pw1 inp->bf + ReLU (full resolution), dw s2, pw2 + ReLU (+shuffle with branch1)
        Folded a1 = fold(sd, p + "branch2.0", p + "branch2.1");
        LP_CHECK(a1.co == bf && a1.ci == inp, LP_ERR_ARG, "%sbranch2.0 shape", p.c_str());
        expand_pw(a1, lin, 0, bfp, w, b, lin.Cp(), 0);
        if (layers) B.b2_pw1 = add_pw(p + "branch2.0", w, b, lin.Cp(), bfp, ACT_RELU, Hin);
        if (two) { upload_u16(f2.pw1, pack_fused_pw(w, bfp, lin.Cp())); upload_f32(f2.pw1b, b); }
        b1dw_elems = std::max(b1dw_elems, (size_t)Ho * Ho * lin.Cp());
        b1_elems = std::max(b1_elems, (size_t)Ho * Ho * bfp);
        t1_elems = std::max(t1_elems, (size_t)Hin * Hin * bfp);
      } else {
        // x1 = first half (pass-through), x2 = second half -> branch2
        Folded a1 = fold(sd, p + "branch2.0", p + "branch2.1");
        LP_CHECK(a1.co == bf && a1.ci == bf, LP_ERR_ARG, "%sbranch2.0 shape", p.c_str());
        expand_pw(a1, lout, bf, bfp, w, b, bfp, bfp);
        if (s1layers) B.b2_pw1 = add_pw(p + "branch2.0", w, b, bfp, bfp, ACT_RELU, Ho);
        t1_elems = std::max(t1_elems, (size_t)Ho * Ho * bfp);
        if (fusedk) {
          b_.fused[s].emplace_back();
          upload_u16(b_.fused[s].back().w1, pack_fused_pw(w, bfp, bfp));
          upload_f32(b_.fused[s].back().b1, b);
        }
      }
      Folded d2 = fold(sd, p + "branch2.3", p + "branch2.4");
      LP_CHECK(d2.co == bf && d2.ci == 1 && d2.k == 3, LP_ERR_ARG, "%sbranch2.3 shape", p.c_str());
      expand_dw(d2, lmid, 0, bfp, 0, w, b);
      if (as_layers) B.b2_dw = add_dw(p + "branch2.3", w, b, bfp, stride);
      if (fusedk && stride == 1) { upload_f32(b_.fused[s].back().dw, w); upload_f32(b_.fused[s].back().dwb, b); }
      if (two && stride == 2) { upload_f32(f2.dw2, w); upload_f32(f2.dw2b, b); }
      Folded a2 = fold(sd, p + "branch2.5", p + "branch2.6");
      LP_CHECK(a2.co == bf && a2.ci == bf, LP_ERR_ARG, "%sbranch2.5 shape", p.c_str());
      expand_pw(a2, lmid, 0, bfp, w, b, bfp, 0);
      if (as_layers) B.b2_pw2 = add_pw(p + "branch2.5", w, b, bfp, bfp, ACT_RELU, Ho);
      if (fusedk && stride == 1) { upload_u16(b_.fused[s].back().w2, pack_fused_pw(w, bfp, bfp)); upload_f32(b_.fused[s].back().b2, b); }
      if (two && stride == 2) { upload_u16(f2.pw2, pack_fused_pw(w, bfp, bfp)); upload_f32(f2.pw2b, b); }
      t2_elems = std::max(t2_elems, (size_t)Ho * Ho * bfp);
      if (stride == 2) b_.s2[s] = B; else if (s1layers) b_.s1[s].push_back(B);
      inp = kStageOut[s];
      lin = lout;
    }
    if (layers) {
      alloc_act(b_.a_stage[s][0], 2 * bfp, Ho, Ho);
      alloc_act(b_.a_stage[s][1], 2 * bfp, Ho, Ho);
    }
    if (plan_ == STAGE_FUSED) {
      // blocks 1..n-1 of the stage in one launch, X resident in LDS: the stride-2 block's output -> the stage's other buffer
      FusedStageArgs& fa = b_.stage[s];
      fa.in = b_.a_stage[s][0].mem.p; fa.out = b_.a_stage[s][1].mem.p;
      fa.nblk = kStageRepeats[s] - 1;
      for (int q = 0; q < fa.nblk; ++q) fa.blk[q] = s1w(b_.fused[s][q]);
      fa.HW = Ho * Ho; fa.W = Ho; fa.bf = bf; fa.bfp = bfp; fa.group = kFusedPix / fa.HW;
      fa.in_pitch = 2 * bfp; fa.out_pitch = 2 * bfp;
    }
  }
  if (layers) {
    const size_t es = prec_ == LP_FP16 ? 2 : 4;
    b_.a_t1.mem.alloc((size_t)maxR_ * t1_elems * es);
    b_.a_t2.mem.alloc((size_t)maxR_ * t2_elems * es);
    b_.a_b1dw.mem.alloc((size_t)maxR_ * b1dw_elems * es);
    b_.a_b1.mem.alloc((size_t)maxR_ * b1_elems * es);
  }

  // conv5 + BN + ReLU, mean, fc
  const int H = stage_side(kStages - 1), cin_p = lin.Cp();
  lpitch_ = class_pad(ncls_);
  d_logits_.alloc((size_t)maxR_ * lpitch_ * 4);
  {
    Folded f = fold(sd, "conv5.0", "conv5.1");
    LP_CHECK(f.co == kConv5C && f.ci == kStageOut[kStages - 1] && f.k == 1, LP_ERR_ARG, "conv5 must be 464->1024 1x1");
    std::vector<float> w, b;
    expand_pw(f, lin, 0, kConv5C, w, b, cin_p, 0);
    if (s1layers) {
      b_.conv5 = add_pw("conv5.0", w, b, cin_p, kConv5C, ACT_RELU, H);
      alloc_act(b_.a_conv5, kConv5C, H, H);
      alloc_act(b_.a_mean, kConv5C, 1, 1);
    }
    if (fusedk) {
      upload_u16(b_.head_w5, pack_fused_pw(w, kConv5C, cin_p));
      upload_f32(b_.head_b5, b);
    }
    const NamedTensor& fw = need(sd, "fc.weight");
    const NamedTensor& fb = need(sd, "fc.bias");
    LP_CHECK(fw.shape.size() == 2 && fw.shape[0] == ncls_ && fw.shape[1] == kConv5C && (int)fb.numel() == ncls_, LP_ERR_ARG,
             "fc must be Linear(1024, %d), got [%lld,%lld]", ncls_, (long long)(fw.shape.size() ? fw.shape[0] : 0),
             (long long)(fw.shape.size() > 1 ? fw.shape[1] : 0));
    // fc rows padded to 8 (ConvLayer) or to the logits pitch (fused kernels)
    const int rows = s1layers ? rup(ncls_, 8) : lpitch_;
    std::vector<float> w2((size_t)rows * kConv5C, 0.f), b2(rows, 0.f);
    memcpy(w2.data(), fw.data, (size_t)ncls_ * kConv5C * 4);
    memcpy(b2.data(), fb.data, (size_t)ncls_ * 4);
    if (s1layers) b_.fc = add_pw("fc", w2, b2, kConv5C, rows, ACT_NONE, 1);
    if (fusedk) {
      upload_u16(b_.head_wfc, pack_fused_pw(w2, rows, kConv5C));
      upload_f32(b_.head_bfc, b2);
    }
  }
  if (plan_ == STAGE_FUSED) {
    FusedHeadArgs& ha = b_.head;
    ha.in = b_.a_stage[kStages - 1][1].mem.p; ha.in_pitch = cin_p; ha.cin_p = cin_p;
    ha.w5 = b_.head_w5.as<u32x4_t>(); ha.b5 = b_.head_b5.as<float>();
    ha.wfc = b_.head_wfc.as<u32x4_t>(); ha.bfc = b_.head_bfc.as<float>();
  }
  if (two) {
    b_.a_x3.alloc((size_t)maxR_ * stage_side(1) * stage_side(1) * stage_cp(1) * 2);
    ClsFrontArgs& fa = b_.front;
    fa.out = b_.a_x3.p;
    fa.stem_w = b_.stem_frag.as<u32x4_t>(); fa.stem_b = b_.stem_bias4.as<float>();
    fa.s20 = s2w(b_.fused_s2[0]);
    for (int q = 0; q < 3; ++q) fa.s2[q] = s1w(b_.fused[0][q]);
    fa.s30 = s2w(b_.fused_s2[1]);
    ClsBackArgs& ba = b_.back;
    ba.in = b_.a_x3.p;
    for (int q = 0; q < 7; ++q) ba.s3[q] = s1w(b_.fused[1][q]);
    ba.s40 = s2w(b_.fused_s2[2]);
    for (int q = 0; q < 3; ++q) ba.s4[q] = s1w(b_.fused[2][q]);
    ba.w5 = b_.head_w5.as<u32x4_t>(); ba.b5 = b_.head_b5.as<float>();
    ba.wfc = b_.head_wfc.as<u32x4_t>(); ba.bfc = b_.head_bfc.as<float>();
  }
  loaded_ = true;
}

// the output block of cls_back / cls_head_fused: the logits and class counts are the handle's, the rest is the caller's
ClsOut Classifier::out_block(const Post* post) const {
  ClsOut o;
  memset(&o, 0, sizeof(o));
  o.nc = ncls_; o.nc_p = lpitch_;
  o.logits = d_logits_.as<float>(); o.logits_pitch = lpitch_;
  if (post) {
    o.probs = post->probs; o.ids = post->ids; o.dets = post->dets; o.max_det = post->max_det;
    o.roi_img = post->roi_img; o.roi_slot = post->roi_slot;
  }
  return o;
}

namespace {
// a profiler bracket around one launch; the kernel name carries the precision
struct Bracket {
  Profiler* prof; hipStream_t st; const char* sfx;
  void begin() const { if (prof) prof->begin(st); }
  void end(const char* kname, const std::string& layer, double flops, double bytes) const {
    if (prof) prof->end(st, std::string(kname) + sfx, layer, flops, bytes, true);
  }
};
}  // namespace

void Classifier::forward(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post) {
  LP_CHECK(loaded_, LP_ERR_STATE, "classifier not loaded");
  if (plan_ == TWO_LAUNCH) forward_two_launch(rgb, d_R, st, prof, post);
  else forward_layers(rgb, d_R, st, prof, post);
}

void Classifier::forward_two_launch(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post) {
  const Bracket P{prof, st, "_f16"};
  ClsFrontArgs fa = b_.front;
  fa.rgb = rgb; fa.m_dyn = d_R;
  P.begin();
  launch_cls_front(fa, maxR_, st);
  // conv1 0.66 + stage2 2.10 + stage3.0 0.6 MMAC per ROI; bytes: the uint8 crop in, stage 3.0's two depthwise sets
  // (staged per ROI, from L2), 8 KB out
  P.end("cls_front", "conv1..stage3.0", 2.0 * (0.66e6 + 2.10e6 + 0.60e6), 12288.0 + 10240.0 + 8192.0);
  ClsBackArgs ba = b_.back;
  ba.m_dyn = d_R; ba.out = out_block(post);
  P.begin();
  launch_cls_back(ba, maxR_, st);
  P.end("cls_back", "stage3.1..softmax", 2.0 * (3.86e6 + 2.63e6 + 1.90e6 + 1024.0 * ncls_), 8192.0 + ncls_ * 4.0);
}

// STAGE_FUSED and LAYERWISE: stem, maxpool and each stage's stride-2 block one kernel per layer; then the stage's stride-1
// blocks and the head either fused (one launch per stage, cls_head_fused) or layer by layer as well
void Classifier::forward_layers(const uint8_t* rgb, const int* d_R, hipStream_t st, Profiler* prof, const Post* post) {
  const size_t es = prec_ == LP_FP16 ? 2 : 4;
  const double esd = (double)es;
  const Bracket P{prof, st, prec_ == LP_FP16 ? "_f16" : "_f32"};
  auto run_pw = [&](int idx, const View& in, const View& out, const View* x1, int half_c, int half_cp, int out_f32) {
    const ConvLayer& c = *b_.pws[idx];
    ConvIO io;
    io.in = in; io.out = out; io.N = maxR_; io.m_dyn = d_R; io.out_f32 = out_f32;
    if (x1) { io.x1 = *x1; io.half_c = half_c; io.half_cp = half_cp; }
    P.begin();
    c.launch(io, st);
    const double px = (double)out.H * out.W;
    P.end(c.family_name(), c.name, 2.0 * c.Cin * c.Cout * px,
          px * (c.Cin + c.Cout * (x1 ? 2.0 : 1.0)) * esd);
  };
  auto run_dw = [&](int idx, const View& in, const View& out) {
    const DwLayer& d = b_.dws[idx];
    P.begin();
    launch_dwconv3x3(prec_, in, out, d.w.as<float>(), d.b.as<float>(), d.stride, d_R, maxR_, st);
    P.end("dwconv3x3", d.name, 2.0 * 9 * d.C * out.H * out.W, ((double)in.H * in.W + (double)out.H * out.W) * d.C * esd);
  };

  P.begin();
  launch_cls_stem(prec_, rgb, b_.stem_w.as<float>(), b_.stem_b.as<float>(), 24, act_view(b_.a_stem), S_, d_R, maxR_, st);
  P.end("cls_stem", "conv1", 2.0 * 27 * 24 * b_.a_stem.H * b_.a_stem.W, (double)S_ * S_ * 3 + (double)b_.a_stem.H * b_.a_stem.W * 24 * esd);
  P.begin();
  launch_maxpool3x3s2(prec_, act_view(b_.a_stem), act_view(b_.a_pool), d_R, maxR_, st);
  P.end("maxpool3x3s2", "maxpool", 0.0, ((double)b_.a_stem.H * b_.a_stem.W + (double)b_.a_pool.H * b_.a_pool.W) * 24 * esd);

  View x = act_view(b_.a_pool);
  for (int s = 0; s < kStages; ++s) {
    const int bf = half_c(s), bfp = half_cp(s), Ho = stage_side(s);
    const View t2 = make_view(b_.a_t2.mem, es, 0, bfp, bfp, Ho, Ho);
    {
      const Block& B = b_.s2[s];
      const View out = act_view(b_.a_stage[s][0]);
      const View b1dw = make_view(b_.a_b1dw.mem, es, 0, x.C, x.C, Ho, Ho);
      const View b1 = make_view(b_.a_b1.mem, es, 0, bfp, bfp, Ho, Ho);
      const View t1 = make_view(b_.a_t1.mem, es, 0, bfp, bfp, x.H, x.W);
      run_dw(B.b1_dw, x, b1dw);
      run_pw(B.b1_pw, b1dw, b1, nullptr, 0, 0, 0);
      run_pw(B.b2_pw1, x, t1, nullptr, 0, 0, 0);
      run_dw(B.b2_dw, t1, t2);
      run_pw(B.b2_pw2, t2, out, &b1, bf, bfp, 0);
      x = out;
    }
    if (plan_ == STAGE_FUSED) {
      FusedStageArgs fa = b_.stage[s];
      fa.m_dyn = d_R;
      P.begin();
      launch_fused_stage(fa, maxR_, st);
      const double px = (double)fa.HW;
      P.end("shuffle_stage_fused", fmt("stage%d.1-%d", s + 2, kStageRepeats[s] - 1),
            fa.nblk * (2.0 * 2.0 * bfp * bfp + 2.0 * 9 * bfp) * px, 2.0 * px * 2 * bfp * esd);
      x = act_view(b_.a_stage[s][1]);
      continue;
    }
    for (int r = 1; r < kStageRepeats[s]; ++r) {
      const Block& B = b_.s1[s][r - 1];
      const View out = act_view(b_.a_stage[s][r & 1]);
      const View x1 = View{x.base, bfp, x.pitch, x.H, x.W};
      const View x2 = View{static_cast<char*>(x.base) + (size_t)bfp * es, bfp, x.pitch, x.H, x.W};
      const View t1 = make_view(b_.a_t1.mem, es, 0, bfp, bfp, Ho, Ho);
      run_pw(B.b2_pw1, x2, t1, nullptr, 0, 0, 0);
      run_dw(B.b2_dw, t1, t2);
      run_pw(B.b2_pw2, t2, out, &x1, bf, bfp, 0);
      x = out;
    }
  }
  if (plan_ == STAGE_FUSED) {
    FusedHeadArgs ha = b_.head;
    ha.m_dyn = d_R; ha.out = out_block(post);
    P.begin();
    launch_fused_head(ha, maxR_, st);
    P.end("cls_head_fused", "conv5+mean+fc+softmax", 4.0 * 2.0 * ha.cin_p * 1024 + 2.0 * 1024 * lpitch_, 4.0 * ha.cin_p * esd + ncls_ * 4.0);
    return;
  }
  run_pw(b_.conv5, x, act_view(b_.a_conv5), nullptr, 0, 0, 0);
  P.begin();
  launch_spatial_mean(prec_, act_view(b_.a_conv5), act_view(b_.a_mean), d_R, maxR_, st);
  P.end("spatial_mean", "mean", 0.0, (double)(b_.a_conv5.H * b_.a_conv5.W + 1) * 1024 * esd);
  View lg;
  lg.base = d_logits_.p; lg.C = lpitch_; lg.pitch = lpitch_; lg.H = 1; lg.W = 1;
  run_pw(b_.fc, act_view(b_.a_mean), lg, nullptr, 0, 0, 1);
}

}  // namespace lp
