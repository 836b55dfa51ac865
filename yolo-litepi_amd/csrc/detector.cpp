// Detector at run time: the per-launch profiler, tensor views, the forward pass over the planned ops and the blob
// test aid.  The plan itself (Detector::load) is built in detector_plan.cpp.
#include "detector.h"
#include <cstring>

namespace lp {

// ---- profiler -------------------------------------------------------------------------
thread_local LaunchTimer* g_launch_timer = nullptr;
bool print_launches() {
  static const bool on = getenv("LITEPI_PRINT_LAUNCH") != nullptr;
  return on;
}

void Profiler::begin(hipStream_t st) {
  if (!enabled) return;
  LP_HIP(hipEventCreate(&cur));
  LP_HIP(hipEventRecord(cur, st));
  timer = LaunchTimer();
  LP_HIP(hipEventCreate(&timer.e0));
  LP_HIP(hipEventCreate(&timer.e1));
  g_launch_timer = &timer;
}
void Profiler::end(hipStream_t st, const std::string& name, const std::string& layer, double flops, double bytes, bool per_roi) {
  if (!enabled) return;
  g_launch_timer = nullptr;
  Rec r{name, layer, flops, bytes, cur, nullptr, per_roi, timer.e0, timer.e1, timer.launches};
  LP_HIP(hipEventCreate(&r.e1));
  LP_HIP(hipEventRecord(r.e1, st));
  recs.push_back(r);
  cur = nullptr;
}
void Profiler::collect(int roi_count) {
  results.clear();
  for (auto& r : recs) {
    lp_kernel_time k;
    memset(&k, 0, sizeof(k));
    snprintf(k.name, sizeof(k.name), "%s", r.name.c_str());
    snprintf(k.layer, sizeof(k.layer), "%s", r.layer.c_str());
    float ms = 0.f, kms = 0.f;
    if (hipEventElapsedTime(&ms, r.e0, r.e1) != hipSuccess) ms = -1.f;
    // one launch inside the bracket: its own start -> stop events (the kernel without the dispatch around it)
    if (r.launches == 1 && hipEventElapsedTime(&kms, r.k0, r.k1) == hipSuccess && kms > 0.f) ms = kms;
    k.ms = ms;
    k.flops = r.flops * (r.per_roi ? roi_count : 1);
    k.bytes = r.bytes * (r.per_roi ? roi_count : 1);
    results.push_back(k);
    (void)hipEventDestroy(r.e0);
    (void)hipEventDestroy(r.e1);
    (void)hipEventDestroy(r.k0);
    (void)hipEventDestroy(r.k1);
  }
  recs.clear();
}
Profiler::~Profiler() {
  for (auto& r : recs) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); (void)hipEventDestroy(r.k0); (void)hipEventDestroy(r.k1); }
  if (g_launch_timer == &timer) g_launch_timer = nullptr;
}

// ---- tensors ---------------------------------------------------------------------------
int Tensor::phys(int c) const {
  int lo = 0, po = 0;
  for (int s : segs) {
    if (c < lo + s) return po + (c - lo);
    lo += s;
    po += round_up(s, 8);
  }
  return -1;
}

Detector::Detector(int prec, int impl, int max_batch, int input_h, int input_w)
    : prec_(prec), impl_(impl), maxB_(max_batch), SH_(input_h), SW_(input_w) {}

View Detector::view(int t) const {
  const Tensor* T = &tensors_[t];
  int off = 0;
  if (T->parent >= 0) {
    const Tensor& P = tensors_[T->parent];
    for (int k = 0; k < T->parent_seg; ++k) off += round_up(P.segs[k], 8);
    off += P.off;
    LP_CHECK(P.buf >= 0, LP_ERR_STATE, "blob %s: parent has no storage", T->name.c_str());
    const Buffer& b = buffers_[P.buf];
    View v;
    v.base = static_cast<char*>(b.mem.p) + (size_t)off * (prec_ == LP_FP16 ? 2 : 4);
    v.C = T->Cp; v.pitch = b.Cp; v.H = T->H; v.W = T->W;
    return v;
  }
  LP_CHECK(T->buf >= 0, LP_ERR_STATE, "blob %s has no storage", T->name.c_str());
  const Buffer& b = buffers_[T->buf];
  View v;
  v.base = static_cast<char*>(b.mem.p) + (size_t)T->off * (prec_ == LP_FP16 ? 2 : 4);
  v.C = T->Cp; v.pitch = b.Cp; v.H = T->H; v.W = T->W;
  return v;
}

void Detector::forward(const uint8_t* imgs, int B, const ImgGeom* geom, float conf, float* out0, Cand* cand,
                       int* cand_count, hipStream_t st, Profiler* prof) {
  LP_CHECK(loaded_, LP_ERR_STATE, "detector not loaded");
  LP_CHECK(B >= 1 && B <= maxB_, LP_ERR_ARG, "batch %d outside 1..%d", B, maxB_);
  const char* sfx = prec_ == LP_FP16 ? "_f16" : "_f32";
  // Diagnostic only (tools/marginal_cost.sh): LITEPI_SKIP_OP=<i> leaves launch i out of every pass after this handle's first,
  // whose outputs stay in its (never re-used) buffers -- the marginal cost of one launch in a pipelined step.  Results are stale.
  static const int skip_op = getenv("LITEPI_SKIP_OP") ? atoi(getenv("LITEPI_SKIP_OP")) : -1;
  const bool skipping = skip_op >= 0 && fwd_calls_++ > 0 && !prof;
  int op_index = -1;
  for (const DetOp& op : ops_) {
    if (++op_index == skip_op && skipping) continue;
    if (prof) prof->begin(st);
    std::string kname;
    switch (op.kind) {
      case DetOp::STEM:
        stem_.launch(imgs, B, SH_, SW_, view(op.out), st);
        kname = std::string(stem_.kernel_name(false)) + sfx;
        break;
      case DetOp::STEMBLOCK:
        stem_.launch_block(imgs, B, SH_, SW_, *convs_[op.conv], view(op.out), st);
        kname = std::string(stem_.kernel_name(true)) + sfx;
        break;
      case DetOp::CONV: {
        const ConvLayer& c = *convs_[op.conv];
        ConvIO io;
        io.in = view(op.in); io.out = view(op.out); io.N = B;
        if (op.res >= 0) io.res = view(op.res);
        if (op.in2 >= 0) {  // fused upsample: leading channels from the half-resolution tensor, the rest from the concat buffer
          io.up = view(op.in2);
          io.in.base = static_cast<char*>(io.in.base) + (size_t)io.up.C * (prec_ == LP_FP16 ? 2 : 4);
          io.in.C -= io.up.C;
        }
        c.launch(io, st);
        kname = c.kernel_name(op.in2 >= 0) + sfx;
        break;
      }
      case DetOp::BNECK:
        if (op.in2 >= 0) {
          const View catv = view(op.in2);
          bnecks_[op.conv]->launch(view(op.in), view(op.out), B, st, &catv);
        } else {
          bnecks_[op.conv]->launch(view(op.in), view(op.out), B, st);
        }
        kname = bnecks_[op.conv]->kernel_name() + sfx;
        break;
      case DetOp::DWCONV:
        launch_dwconv3x3_act(prec_, view(op.in), view(op.out), dws_[op.conv].w.as<float>(), dws_[op.conv].b.as<float>(), dws_[op.conv].act, B, st);
        kname = std::string("dwconv3x3_det") + sfx;
        break;
      case DetOp::ATTN: {
        const AttnLayer& A = attns_[op.conv];
        launch_psa_attention(prec_, view(op.in), view(op.out), A.pe_w.as<float>(), A.pe_b.as<float>(), A.heads, A.dk, A.dv, A.scale, B, st);
        kname = std::string("psa_attention") + sfx;
        break;
      }
      case DetOp::UPSAMPLE:
        launch_upsample2x(prec_, view(op.in), view(op.out), B, st);
        kname = std::string("upsample2x") + sfx;
        break;
      case DetOp::SPPF:
        launch_sppf_pool(prec_, view(op.in), view(op.out), view(op.out2), view(op.out3), B, st);
        kname = std::string("sppf_pool") + sfx;
        break;
      case DetOp::ADD:
        launch_add(prec_, view(op.in), view(op.in2), view(op.out), B, st);
        kname = std::string("add") + sfx;
        break;
      case DetOp::COPY:
        launch_copy(prec_, view(op.in), view(op.out), B, st);
        kname = std::string("copy") + sfx;
        break;
      case DetOp::C2F: {
        const C2fLayer& cl = *c2fs_[op.conv];
        const C2fIO& ci = c2f_io_[op.conv];
        C2fLayer::IO io;
        io.src1 = view(ci.src1);
        if (ci.src0 >= 0) {  // fused upsample: leading channels from the half-resolution tensor, the rest from the concat buffer
          io.src0 = view(ci.src0);
          io.src1.base = static_cast<char*>(io.src1.base) + (size_t)ci.up_c * 2;
          io.src1.C -= ci.up_c;
        }
        io.cat = view(ci.cat);
        io.out = view(ci.out);
        if (ci.s2_in >= 0) { io.s2_in = view(ci.s2_in); io.x = view(ci.x); }
        if (ci.cat2 >= 0) { io.cat2 = view(ci.cat2); io.out2 = view(ci.out2); }
        cl.launch(io, B, st);
        kname = cl.kernel_name() + sfx;
        break;
      }
      case DetOp::SPPFUSED:
        sppfs_[op.conv]->launch(view(op.in), view(op.out), B, st);
        kname = sppfs_[op.conv]->kernel_name() + sfx;
        break;
      case DetOp::S2C:
        s2cs_[op.conv]->launch(view(op.in), view(op.out), B, st);
        kname = s2cs_[op.conv]->kernel_name() + sfx;
        break;
      case DetOp::HEAD:
        heads_[op.conv]->launch(view(op.in), B, levels_[op.in2].off, A_, d_anchors_.as<float>(), d_strides_.as<float>(), d_dfl_.as<float>(), out0,
                                geom, cand, cand_count, conf, st);
        kname = heads_[op.conv]->kernel_name() + sfx;
        break;
    }
    if (prof) prof->end(st, kname, op.layer, op.flops * B, op.bytes * B);
  }
  if (fused_head_) return;  // every level decoded and filtered inside its head kernel
  DecodeArgs a;
  memset(&a, 0, sizeof(a));
  a.nlevels = (int)levels_.size();
  for (int i = 0; i < a.nlevels; ++i) {
    const View b = view(levels_[i].box), c = view(levels_[i].cls);
    a.lv[i].box = b.base; a.lv[i].cls = c.base; a.lv[i].box_pitch = b.pitch; a.lv[i].cls_pitch = c.pitch;
    a.lv[i].H = levels_[i].H; a.lv[i].W = levels_[i].W; a.lv[i].anchor_off = levels_[i].off;
  }
  a.A = A_; a.nc = nc_; a.reg_max = reg_max_;
  a.anchors = d_anchors_.as<float>(); a.strides = d_strides_.as<float>(); a.dfl_w = d_dfl_.as<float>();
  a.out0 = out0; a.geom = geom; a.cand = cand; a.cand_count = cand_count; a.conf = conf;
  if (prof) prof->begin(st);
  launch_decode(prec_, a, B, st);
  if (prof)
    prof->end(st, std::string("decode") + sfx, "detect_decode", 0.0,
              (double)B * A_ * ((4.0 * reg_max_ + nc_) * (prec_ == LP_FP16 ? 2 : 4) + (out0 ? (4.0 + nc_) * 4 : 0.0)));
}

void Detector::fetch_blob(const std::string& name, int B, std::vector<float>& out, int& C, int& H, int& W) const {
  auto it = blob2tensor_.find(name);
  LP_CHECK(it != blob2tensor_.end(), LP_ERR_ARG, "unknown blob %s", name.c_str());
  const Tensor& T = tensors_[it->second];
  // a blob that a fused kernel keeps in registers / LDS has storage reserved (e.g. its concat slot) but is never written
  LP_CHECK(T.materialised || T.parent >= 0 || T.segs.size() > 1, LP_ERR_ARG, "blob %s is fused away (never stored)", name.c_str());
  LP_CHECK(!T.in_c2f && !(T.parent >= 0 && tensors_[T.parent].in_c2f), LP_ERR_ARG,
           "blob %s is fused away: it lives inside a whole-C2f launch (set LITEPI_C2F_STORE_ALL=1 before loading the model to have the "
           "module store its intermediates)", name.c_str());
  const View v = view(it->second);
  C = T.C; H = T.H; W = T.W;
  const size_t es = prec_ == LP_FP16 ? 2 : 4;
  const size_t npix = (size_t)B * H * W;
  // copy the pitch-wide rows of the underlying buffer and pick the view's channels out of them
  const Tensor& ST = T.parent >= 0 ? tensors_[T.parent] : T;
  const Buffer& buf = buffers_[ST.buf];
  const size_t voff = (size_t)(static_cast<const char*>(v.base) - static_cast<const char*>(buf.mem.p)) / es;
  std::vector<uint8_t> raw(npix * v.pitch * es);
  LP_HIP(hipMemcpy(raw.data(), buf.mem.p, raw.size(), hipMemcpyDeviceToHost));
  out.assign((size_t)B * C * H * W, 0.f);
  for (size_t p = 0; p < npix; ++p) {
    const size_t b = p / ((size_t)H * W), yx = p % ((size_t)H * W);
    for (int c = 0; c < C; ++c) {
      const int pc = T.phys(c);
      float f;
      if (prec_ == LP_FP16) {
        uint16_t h;
        memcpy(&h, &raw[(p * v.pitch + voff + pc) * 2], 2);
        f = f16_to_f32(h);
      } else {
        memcpy(&f, &raw[(p * v.pitch + voff + pc) * 4], 4);
      }
      out[(b * C + c) * H * W + yx] = f;
    }
  }
}

}  // namespace lp
