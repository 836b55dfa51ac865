// Detector planner: turns the NCNN graph of a YOLOv8-family detector (reference
// model.ncnn.param:3-208; YOLO-LitePi v1/v2 and the YOLOv8n baseline share this topology) into
// a list of fused NHWC kernel launches:
//   * Convolution+Swish(+BinaryOp add) -> one conv kernel with bias/SiLU/residual epilogue
//   * Split -> alias, Slice -> channel-slice view, Concat -> producers write straight into
//     channel slices of one buffer (C2f, SPPF, FPN/PAN concats are never materialised)
//   * three chained 5x5 max pools -> one SPPF kernel
//   * the Reshape/Permute/Softmax/DFL/BinaryOp/Sigmoid tail -> one decode kernel
// Channel counts that are not multiples of 8 (v2: 12-channel C2f halves) are padded per
// segment; padding channels carry zero weights on both sides and stay zero.
//
// Detector::load_graph (at the end of the file; Detector::load reads an NCNN pair and calls it, the ONNX loaders hand it
// onnx_graph.cpp's lowering) runs the Planner's phases in order; emit_ops visits the layers in file order and
// tries the fusion rules of a Convolution in the fixed order of emit_convolution.
#include "detector.h"
#include <cstring>

#include <algorithm>
#include <optional>
#include <set>

namespace lp {

// Every LITEPI_* switch the planner reads, read once at the top of a load: a process may set one between two loads.  Every plan-time
// switch of c2f_kernels.hip is here -- that file's supported() functions are pure functions of the shape, and the Planner's
// c2f_ok / s2c_ok / s2c_tail_ok / sppf_ok combine them with these -- and so is conv_kernels.hip's one (bneck_cl): its planner
// (conv_plan.h) reads no environment -- and head_kernels.hip's five (head): its planner (head_plan.h) reads none either, and a
// HeadLayer keeps the shape and the flags of the load that built it.  (What a launch reads stays in the kernels' files: the
// diagnostics LITEPI_C2F_STAMPS, LITEPI_C2F_DEBUG, LITEPI_BNECK_STAMPS, LITEPI_HEAD_STAMPS, and the kernel argument LITEPI_TILE_MAJOR.)
struct PlanSwitches {
  static bool on(const char* name) { return getenv(name) != nullptr; }
  bool no_c2f = on("LITEPI_NO_C2F");             // whole-C2f / SPPF / stride-2 launches of c2f_kernels.hip off
  // c2f<16,2,32>, the n = 2 module on the 80x80 map, is opt-in: its halo-4 recompute of 16-channel layers is VALU work the two-launch
  // bottleneck plan does not have -- 65-75 us against 59; LITEPI_C2F_BB80=1 enables it for A/B runs
  bool c2f_bb80 = on("LITEPI_C2F_BB80");
  // LITEPI_C2F_SKIP=<configuration names separated by ';'> keeps those modules on the layer plan (A/B); held as ";name;name;"
  std::string c2f_skip = getenv("LITEPI_C2F_SKIP") ? std::string(";") + getenv("LITEPI_C2F_SKIP") + ";" : std::string();
  // handles built for fewer than 4 images keep the layer plan: a whole-C2f launch is one long workgroup chain per tile, and with
  // a handful of tiles that chain is the latency -- batch-1 detect 0.475 ms against 0.43 ms
  int c2f_min_batch = getenv("LITEPI_C2F_MIN_BATCH") ? atoi(getenv("LITEPI_C2F_MIN_BATCH")) : 4;
  bool c2f_store_all = on("LITEPI_C2F_STORE_ALL");   // bisect mode: the modules store the intermediates they keep in LDS
  bool c2f_xcv1 = on("LITEPI_C2F_XCV1");         // cv1-less C2f behind a stride-2 conv + cv1 launch also where it is opt-in (v1)
  bool no_c2f_xcv1 = on("LITEPI_NO_C2F_XCV1");   // ... and off where it is the default (v2's 48-channel module)
  bool no_s2c = on("LITEPI_NO_S2C");             // stride-2 launches of c2f_kernels.hip off (with and without a tail)
  bool no_s2lds = on("LITEPI_NO_S2LDS");         // ... only those on the LDS-staged kernel (A/B: they stay on conv3x3s2_direct)
  bool no_s2tail = on("LITEPI_NO_S2TAIL");       // ... only those that carry a 1x1 tail
  bool no_sppf_fused = on("LITEPI_NO_SPPF_FUSED");   // one-launch SPPF off
  bool no_sibling = on("LITEPI_NO_SIBLING");
  bool no_bneck = on("LITEPI_NO_BNECK");         // keeps the layer-at-a-time plan (A/B measurements)
  bool no_cv2fuse = on("LITEPI_NO_CV2FUSE");
  // LITEPI_BNECK_CL=1: a bottleneck + cv2 launch whose input is the concat's last stored segment stages the whole stored concat
  // pixel and gathers cv2's K from LDS (opt-in: fewer HBM bytes, but slower; handed on in BottleneckPair::Cv2::cl)
  bool bneck_cl = getenv("LITEPI_BNECK_CL") && atoi(getenv("LITEPI_BNECK_CL")) == 1;
  bool no_upfuse = on("LITEPI_NO_UPFUSE");
  bool no_stemblock = on("LITEPI_NO_STEMBLOCK");
  bool no_headfuse = on("LITEPI_NO_HEADFUSE");
  bool headfuse_narrow = getenv("LITEPI_HEADFUSE") && strcmp(getenv("LITEPI_HEADFUSE"), "narrow") == 0;   // three-launch head for wide class towers (A/B)
  // the fused head's kernel shapes: the merged stage A everywhere, round 3's stage A (32-pixel slots), round 2's two-workgroup
  // shapes, the one-workgroup shapes; LITEPI_HEAD_FLAGS=<bits> is the kernel argument HeadArgs::flags
  hplan::HeadSwitches head = {on("LITEPI_HEAD_MERGED_A"), on("LITEPI_HEAD_A32"), on("LITEPI_HEAD_2WG"), on("LITEPI_HEAD_1WG"),
                              getenv("LITEPI_HEAD_FLAGS") ? atoi(getenv("LITEPI_HEAD_FLAGS")) : 0};
};

struct Planner {
  using C2fIO = Detector::C2fIO;
  using Level = Detector::Level;

  // ---- the detector being planned
  Detector& d;
  const int prec_, impl_, maxB_, SH_, SW_;
  std::vector<Tensor>& tensors_ = d.tensors_;
  std::map<std::string, int>& blob2tensor_ = d.blob2tensor_;
  std::vector<Buffer>& buffers_ = d.buffers_;
  std::vector<std::unique_ptr<ConvLayer>>& convs_ = d.convs_;
  std::vector<DetOp>& ops_ = d.ops_;
  std::vector<Level>& levels_ = d.levels_;
  double& macs_ = d.macs_;

  // ---- the graph
  const PlanSwitches sw;
  const std::string param_path;
  NcnnGraph g;
  std::vector<NcnnLayer>& L = g.layers;
  int n = 0;
  const size_t es;
  const double esd;
  std::map<std::string, int> producer;
  std::map<std::string, std::vector<int>> consumers;

  // ---- find_detect_tail
  std::vector<int> head_cats;
  int first_tail = 0;
  std::set<int> head_cat_set;
  // ---- find_attention_blocks
  struct AttnBlock { int heads, dk, dv, hw; float scale; int dw; std::string in_blob, out_blob; };
  std::map<int, AttnBlock> attn_at;
  std::vector<char> in_attn;
  // ---- resolve_aliases_and_swish
  std::map<std::string, std::string> alias;
  std::vector<int> fused_act;
  std::vector<std::string> conv_out;
  std::vector<char> skip;
  std::map<std::string, std::vector<int>> canon_consumers;
  std::map<std::string, std::vector<int>> slice_sizes;   // keyed by the canonical input blob (needed before the parent's layout is fixed)
  // ---- make_tensors
  struct ConvInfo { int tin = -1, tout = -1; };
  std::vector<ConvInfo> cinfo;
  int input_tensor = -1;
  // ---- place_concats
  struct CopyJob { int layer, src, dst_buf, dst_off; };
  std::vector<CopyJob> copies;
  // ---- emit_ops
  std::vector<char> done;
  std::map<int, int> fuse_up;  // 1x1 conv layer -> half-resolution tensor it upsamples on the fly (filled by emit_interp, layers in file order)
  bool c2f_on = false;
  std::vector<float> dfl;      // build_detect_tail

  Planner(Detector& det, NcnnGraph&& graph, const std::string& source_name);

  // phases, in the order Detector::load_graph runs them
  void find_detect_tail();
  void find_attention_blocks();
  void resolve_aliases_and_swish();
  void make_tensors();     // pass A
  void place_concats();    // pass B
  void emit_ops();         // pass D
  void fuse_stem_block();
  void build_detect_tail();
  void fuse_heads();

  // ---- graph helpers
  std::string prod_type(const std::string& b) const {
    auto it = producer.find(b);
    return it == producer.end() ? std::string() : L[it->second].type;
  }
  bool is_tail(int i) const { return i >= first_tail || head_cat_set.count(i) || L[i].type == "MemoryData"; }
  std::string canon(const std::string& b) const {
    std::string c = b;
    for (auto it = alias.find(c); it != alias.end(); it = alias.find(c)) c = it->second;
    return c;
  }
  int get(const std::string& blob) const {
    auto it = blob2tensor_.find(canon(blob));
    LP_CHECK(it != blob2tensor_.end(), LP_ERR_GRAPH, "blob %s used before it is produced", blob.c_str());
    return it->second;
  }
  int new_tensor(const std::string& name, int C, int H, int W);
  int alloc_buffer(int Cp, int H, int W);
  void ensure_buffer(int t);
  bool is_silu_conv(int j, int k, int s) {
    return j >= 0 && L[j].type == "Convolution" && !is_tail(j) && !done[j] && L[j].ipar(1, 1) == k && L[j].ipar(3, 1) == s &&
           fused_act[j] == ACT_SILU && !L[j].bias.empty() && cinfo[j].tin >= 0 && cinfo[j].tin != input_tensor;
  }
  int sole_consumer(int t) {
    auto& cs = canon_consumers[tensors_[t].name];
    return cs.size() == 1 ? cs[0] : -1;
  }
  bool feeds_add(int t) {   // a consumer of tensor t is a BinaryOp
    for (int c : canon_consumers[tensors_[t].name])
      if (L[c].type == "BinaryOp") return true;
    return false;
  }
  bool zero_copy_concat(int cc) const {
    for (auto& cj : copies)
      if (cj.layer == cc) return false;
    return true;
  }

  // ---- weights
  std::vector<float> conv_w(int j) const;
  void repack(const NcnnLayer& lc, const Tensor& I, const Tensor& O, int out_base, int cout_phys, std::vector<float>& w, std::vector<float>& b) const;
  static void upload(DevBuf& dst, const std::vector<float>& v) {
    dst.alloc(v.size() * 4);
    LP_HIP(hipMemcpy(dst.p, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  }

  // ---- whole-C2f launches (c2f_kernels.hip; fp16 MFMA plan)
  struct C2fMatch {
    int cv1 = -1, slice = -1, a[2] = {-1, -1}, b[2] = {-1, -1}, add[2] = {-1, -1}, cat = -1, cv2 = -1, nb = 0, c = 0;
    int t_cat = -1;
    std::vector<int> ys;
  };
  // cv1 (1x1) -> three chained 5x5 pools -> zero-copy Concat(s, p1, p2, p3) -> cv2 (1x1)
  struct SppfChain { int cv1 = -1, pools[3] = {-1, -1, -1}, chain[4] = {-1, -1, -1, -1}, cat = -1, t_cat = -1, cv2 = -1; };
  bool match_c2f(int i1, C2fMatch& m);
  bool match_c2f_bottleneck(C2fMatch& m, int cur, int ja, int jadd);
  bool match_sppf_chain(int j1, SppfChain& s);
  bool match_s2_front(int i, C2fMatch& m, int& xcat);
  C2fShape c2f_shape(const C2fMatch& m, int mode, int ks2);
  // One predicate per kernel family of c2f_kernels.hip -- may THIS load emit the launch: the family's pure shape rule (c2f.h) and
  // this load's switches.  Every rule that claims layers for such a launch asks one of these, and no rule asks c2f.h directly.
  bool c2f_ok(const C2fShape& s, int h, int w) const {
    if (!c2f_on || !C2fLayer::supported(s, h, w)) return false;
    const std::string name = C2fLayer::kernel_name(s);
    if (name == "c2f<16,2,32>" && !sw.c2f_bb80) return false;
    return sw.c2f_skip.find(";" + name + ";") == std::string::npos;
  }
  bool s2c_ok(int cin, int cout, int hout, int wout) const {
    return c2f_on && !sw.no_s2c && S2ConvLayer::supported(cin, cout, hout, wout) && !(sw.no_s2lds && S2ConvLayer::lds_staged(cin, cout));
  }
  bool sppf_ok(int cin, int c, int cout, int h, int w) const { return c2f_on && !sw.no_sppf_fused && SppfLayer::supported(cin, c, cout, h, w); }
  bool c2f_plain_ok(int i1);
  void emit_c2f(const C2fMatch& m, int mode, const C2fShape& sh, int i0, int xcat, const SppfChain* sp);
  void mark_inside_c2f(const C2fMatch& m, int mode, const C2fIO& io, const SppfChain* sp);

  // ---- one Convolution: the state the rules hand on, and the rules in the order emit_convolution tries them
  struct ConvSite {
    int i, tin, tout, k, s, Cout, Cin;
    int res = -1;              // take_residual: the tensor added behind the activation (tout is then the add's output)
    int tail = -1, tmid = -1;  // pick_1x1_tail: the folded 1x1 conv and this conv's own output (tout is then the tail's output)
  };
  struct Cv2Match { BottleneckPair::Cv2 cv2; int conv = -1, t_cat = -1; std::vector<float> w, b; };
  void emit_convolution(int i);
  bool try_c2f(int i);
  bool try_sppf(int i);
  void take_residual(ConvSite& c);
  int find_sibling(const ConvSite& c);
  bool try_sibling_merge(const ConvSite& c);
  bool try_bottleneck(const ConvSite& c);
  std::optional<Cv2Match> match_bneck_cv2(int tin, int tfinal);
  void pick_1x1_tail(ConvSite& c);
  bool s2c_tail_ok(const ConvSite& c, int tail, int tmid, int tout) const;   // (the stride-2 family's predicate for a conv WITH a tail)
  bool try_s2c_with_tail(const ConvSite& c);
  void emit_c2f_behind_tail(const ConvSite& c);
  bool try_s2c(const ConvSite& c);
  void emit_s2c(const ConvSite& c);
  void emit_stem_or_conv(const ConvSite& c);
  void emit_stem(const ConvSite& c, DetOp& op);
  void emit_conv(const ConvSite& c, DetOp& op);

  // ---- the other layer kinds
  void emit_attention(int i);
  void emit_dwconv(int i);
  void emit_add(int i);
  void emit_pool_chain(int i);
  void emit_interp(int i);
  void emit_concat_copies(int i);

  // ---- Detect-head fusion
  struct Trip { int a, b, c, c3, proj; };   // proj: the class tower's 1x1 projection when it is a launch of its own (else -1)
  int conv_producer_of(int tensor) const {
    for (size_t q = 0; q < ops_.size(); ++q)
      if (ops_[q].kind == DetOp::CONV && ops_[q].out == tensor) return (int)q;
    return -1;
  }
  bool match_head_level(const Level& lv, Trip& t);
};

Planner::Planner(Detector& det, NcnnGraph&& graph, const std::string& source_name)
    : d(det), prec_(det.prec_), impl_(det.impl_), maxB_(det.maxB_), SH_(det.SH_), SW_(det.SW_), param_path(source_name), g(std::move(graph)),
      es(det.prec_ == LP_FP16 ? 2 : 4), esd((double)es) {
  n = (int)L.size();
  d.tensors_.clear(); d.blob2tensor_.clear(); d.buffers_.clear(); d.convs_.clear(); d.ops_.clear(); d.levels_.clear();
  d.bnecks_.clear(); d.dws_.clear(); d.attns_.clear(); d.heads_.clear(); d.c2fs_.clear(); d.c2f_io_.clear(); d.s2cs_.clear(); d.sppfs_.clear();
  d.fused_head_ = false;
  d.loaded_ = false;
  for (int i = 0; i < n; ++i) {
    for (auto& o : L[i].outputs) producer[o] = i;
    for (auto& in : L[i].inputs) consumers[in].push_back(i);
  }
  c2f_on = !sw.no_c2f && prec_ == LP_FP16 && impl_ == IMPL_MFMA && maxB_ >= sw.c2f_min_batch;
}

// ---- find the Detect tail ---------------------------------------------------------------
void Planner::find_detect_tail() {
  first_tail = n;
  for (int i = 0; i < n; ++i) {
    if (L[i].type != "Reshape" || L[i].inputs.empty()) continue;
    auto it = producer.find(L[i].inputs[0]);
    if (it == producer.end()) continue;
    const NcnnLayer& c = L[it->second];
    if (c.type == "Concat" && c.inputs.size() == 2 && prod_type(c.inputs[0]) == "Convolution" &&
        prod_type(c.inputs[1]) == "Convolution") {
      head_cats.push_back(it->second);
      first_tail = std::min(first_tail, i);
    }
  }
  LP_CHECK(!head_cats.empty() && head_cats.size() <= 4, LP_ERR_GRAPH, "no YOLOv8-style Detect head found in %s", param_path.c_str());
  head_cat_set.insert(head_cats.begin(), head_cats.end());
}

// ---- YOLO11 C2PSA attention blocks: a fixed 12-layer sequence becomes one ATTN op (launch_psa_attention) --------
void Planner::find_attention_blocks() {
  in_attn.assign(n, 0);
  const char* seq[12] = {"Reshape", "Slice", "Split", "Permute", "MatMul", "BinaryOp", "Softmax", "MatMul", "Reshape", "Reshape",
                         "ConvolutionDepthWise", "BinaryOp"};
  for (int i = 0; i + 12 <= n; ++i) {
    if (is_tail(i) || L[i].type != "Reshape" || L[i].ipar(2, 0) <= 0 || prod_type(L[i].inputs[0]) != "Convolution") continue;
    bool ok = true;
    for (int q = 0; q < 12 && ok; ++q) ok = L[i + q].type == seq[q];
    if (!ok) continue;
    AttnBlock a;
    a.heads = L[i].ipar(2); a.hw = L[i].ipar(0);
    auto it = L[i + 1].arrays.find(0);
    ok = it != L[i + 1].arrays.end() && it->second.size() == 3 && L[i + 1].ipar(1, 0) == 1 && it->second[0] == it->second[1];
    if (ok) { a.dk = (int)it->second[0]; a.dv = (int)it->second[2]; }
    ok = ok && L[i].ipar(1) == 2 * a.dk + a.dv && L[i + 3].ipar(0, 0) == 1 && L[i + 5].ipar(0, 0) == 2 && L[i + 5].ipar(1, 0) == 1 &&
         L[i + 7].ipar(0, 0) == 1 && L[i + 10].ipar(1, 1) == 3 && L[i + 10].ipar(3, 1) == 1 && L[i + 10].ipar(4, 0) == 1 &&
         L[i + 10].ipar(7, 1) == a.heads * a.dv && L[i + 10].ipar(0) == a.heads * a.dv && L[i + 11].ipar(0, 0) == 0 &&
         L[i + 11].inputs.size() == 2;
    LP_CHECK(ok, LP_ERR_GRAPH, "attention block at %s has an unexpected shape", L[i].name.c_str());
    a.scale = (float)L[i + 5].fpar(2, 1.0);
    a.dw = i + 10;
    a.in_blob = L[i].inputs[0];
    a.out_blob = L[i + 11].outputs[0];
    attn_at[i] = a;
    for (int q = 0; q < 12; ++q) in_attn[i + q] = 1;
  }
}

// ---- aliases (Split) and Swish fusion; consumers per canonical blob; Slice sizes --------------------
void Planner::resolve_aliases_and_swish() {
  fused_act.assign(n, ACT_NONE);
  conv_out.assign(n, std::string());
  skip.assign(n, 0);
  for (int i = 0; i < n; ++i) {
    if (is_tail(i) || in_attn[i]) continue;
    if (L[i].type == "Split")
      for (auto& o : L[i].outputs) alias[o] = L[i].inputs[0];
    if (L[i].type == "Convolution" || L[i].type == "ConvolutionDepthWise") {
      const std::string& x = L[i].outputs[0];
      conv_out[i] = x;
      auto& cs = consumers[x];
      if (cs.size() == 1 && L[cs[0]].type == "Swish" && !is_tail(cs[0])) {
        fused_act[i] = ACT_SILU;
        conv_out[i] = L[cs[0]].outputs[0];
        skip[cs[0]] = 1;
      }
    }
  }
  for (int i = 0; i < n; ++i) {
    if (L[i].type == "Split" || skip[i]) continue;
    if (in_attn[i]) {  // the block as a whole consumes its input blob
      if (attn_at.count(i)) canon_consumers[canon(attn_at[i].in_blob)].push_back(i);
      continue;
    }
    for (auto& in : L[i].inputs) canon_consumers[canon(in)].push_back(i);
  }
  for (int i = 0; i < n; ++i) {
    if (is_tail(i) || in_attn[i] || L[i].type != "Slice") continue;
    LP_CHECK(L[i].ipar(1, 0) == 0, LP_ERR_GRAPH, "Slice %s: only channel slices supported", L[i].name.c_str());
    auto it = L[i].arrays.find(0);
    LP_CHECK(it != L[i].arrays.end() && it->second.size() == L[i].outputs.size(), LP_ERR_GRAPH, "Slice %s: bad size list", L[i].name.c_str());
    std::vector<int> sz;
    for (double v : it->second) sz.push_back((int)v);
    slice_sizes[canon(L[i].inputs[0])] = sz;
  }
}

// ---- pass A: shapes and tensors ---------------------------------------------------------
int Planner::new_tensor(const std::string& name, int C, int H, int W) {
  Tensor t;
  t.name = name; t.C = C; t.H = H; t.W = W;
  auto it = slice_sizes.find(name);
  if (it != slice_sizes.end()) {
    std::vector<int> sz = it->second;
    int known = 0, autos = 0;
    for (int s : sz) { if (s == -233) ++autos; else known += s; }
    for (int& s : sz) if (s == -233) s = (C - known) / autos;
    int sum = 0;
    for (int s : sz) sum += s;
    LP_CHECK(sum == C, LP_ERR_GRAPH, "Slice sizes of blob %s do not add up to %d", name.c_str(), C);
    t.segs = sz;
  } else {
    t.segs = {C};
  }
  tensors_.push_back(t);
  blob2tensor_[name] = (int)tensors_.size() - 1;
  return (int)tensors_.size() - 1;
}

void Planner::make_tensors() {
  cinfo.assign(n, ConvInfo());
  for (int i = 0; i < n; ++i) {
    if (is_tail(i) && L[i].type != "Convolution") continue;
    if (i >= first_tail) continue;  // DFL conv etc.
    const NcnnLayer& l = L[i];
    if (skip[i]) continue;
    if (in_attn[i]) {
      if (attn_at.count(i)) {
        const AttnBlock& a = attn_at[i];
        const Tensor tin = tensors_[get(a.in_blob)];
        LP_CHECK(tin.C == a.heads * (2 * a.dk + a.dv) && tin.H * tin.W == a.hw && tin.segs.size() == 1, LP_ERR_GRAPH,
                 "attention block at %s: qkv blob is %dx%dx%d", l.name.c_str(), tin.C, tin.H, tin.W);
        new_tensor(a.out_blob, a.heads * a.dv, tin.H, tin.W);
      }
      continue;
    }
    if (l.type == "ConvolutionDepthWise") {
      const int tin = get(l.inputs[0]);
      LP_CHECK(l.ipar(1, 1) == 3 && l.ipar(3, 1) == 1 && l.ipar(4, 0) == 1 && l.ipar(2, 1) == 1 && l.ipar(7, 1) == l.ipar(0) &&
                   l.ipar(0) == tensors_[tin].C && l.ipar(9, 0) == 0 && l.ipar(8, 0) == 0, LP_ERR_GRAPH,
               "ConvolutionDepthWise %s: only depthwise 3x3/s1/p1 without fused activation supported", l.name.c_str());
      cinfo[i].tin = tin;
      cinfo[i].tout = new_tensor(conv_out[i], l.ipar(0), tensors_[tin].H, tensors_[tin].W);
      continue;
    }
    if (l.type == "Input") {
      input_tensor = new_tensor(l.outputs[0], 3, SH_, SW_);
    } else if (l.type == "Convolution") {
      const int tin = get(l.inputs[0]);
      const int k = l.ipar(1, 1), s = l.ipar(3, 1), pad = l.ipar(4, 0), dil = l.ipar(2, 1);
      // pad k/2 everywhere; the image conv may also be YOLOv5's 6x6/s2/p2 stem (any k, s, p: generic stem kernel)
      LP_CHECK(l.ipar(11, k) == k && l.ipar(13, s) == s && l.ipar(14, pad) == pad && dil == 1 && (pad == k / 2 || tin == input_tensor), LP_ERR_GRAPH,
               "Convolution %s: only square k with pad k/2, dilation 1 supported", l.name.c_str());
      LP_CHECK(l.in_ch == tensors_[tin].C, LP_ERR_GRAPH, "Convolution %s: weight expects %d input channels, blob has %d",
               l.name.c_str(), l.in_ch, tensors_[tin].C);
      // fused activation (9 != 0, e.g. after ncnnoptimize), int8 weights (8), asymmetric / valued padding (15, 16, 18): the
      // kernels implement none of them, and ignoring the parameter would silently compute a different network
      LP_CHECK(l.ipar(9, 0) == 0 && l.ipar(8, 0) == 0 && l.ipar(15, pad) == pad && l.ipar(16, pad) == pad && l.fpar(18, 0.0) == 0.0,
               LP_ERR_GRAPH, "Convolution %s: fused activation_type / int8 / asymmetric padding parameters are unsupported", l.name.c_str());
      const int Ho = (tensors_[tin].H + 2 * pad - k) / s + 1, Wo = (tensors_[tin].W + 2 * pad - k) / s + 1;
      cinfo[i].tin = tin;
      cinfo[i].tout = new_tensor(conv_out[i], l.ipar(0), Ho, Wo);
    } else if (l.type == "Swish") {
      throw Error(LP_ERR_GRAPH, fmt("stand-alone Swish %s unsupported", l.name.c_str()));
    } else if (l.type == "Split") {
      const int t = get(l.inputs[0]);
      for (auto& o : l.outputs) blob2tensor_[o] = t;
    } else if (l.type == "Slice") {
      const int tin = get(l.inputs[0]);
      const std::vector<int> sz = tensors_[tin].segs;
      LP_CHECK(sz.size() == l.outputs.size(), LP_ERR_GRAPH, "Slice %s: layout mismatch", l.name.c_str());
      for (size_t j = 0; j < l.outputs.size(); ++j) {
        const int t = new_tensor(l.outputs[j], sz[j], tensors_[tin].H, tensors_[tin].W);
        tensors_[t].parent = tin;
        tensors_[t].parent_seg = (int)j;
      }
    } else if (l.type == "Concat") {
      LP_CHECK(l.ipar(0, 0) == 0, LP_ERR_GRAPH, "Concat %s: only channel concat supported", l.name.c_str());
      int C = 0;
      std::vector<int> segs;
      const int t0 = get(l.inputs[0]);
      for (auto& in : l.inputs) {
        const Tensor& t = tensors_[get(in)];
        LP_CHECK(t.H == tensors_[t0].H && t.W == tensors_[t0].W, LP_ERR_GRAPH, "Concat %s: spatial mismatch", l.name.c_str());
        C += t.C;
        segs.insert(segs.end(), t.segs.begin(), t.segs.end());
      }
      const int t = new_tensor(l.outputs[0], C, tensors_[t0].H, tensors_[t0].W);
      if (tensors_[t].segs.size() == 1) tensors_[t].segs = segs;
    } else if (l.type == "BinaryOp") {
      LP_CHECK(l.ipar(0, 0) == 0 && l.inputs.size() == 2 && l.ipar(1, 0) == 0, LP_ERR_GRAPH, "BinaryOp %s: only tensor add supported", l.name.c_str());
      const Tensor a = tensors_[get(l.inputs[0])], b = tensors_[get(l.inputs[1])];
      LP_CHECK(a.C == b.C && a.H == b.H && a.W == b.W, LP_ERR_GRAPH, "BinaryOp %s: shape mismatch", l.name.c_str());
      new_tensor(l.outputs[0], a.C, a.H, a.W);
    } else if (l.type == "Pooling") {
      LP_CHECK(l.ipar(0, 0) == 0 && l.ipar(1) == 5 && l.ipar(2, 1) == 1 && l.ipar(3, 0) == 2, LP_ERR_GRAPH,
               "Pooling %s: only the SPPF 5x5/s1/p2 max pool is supported", l.name.c_str());
      const Tensor a = tensors_[get(l.inputs[0])];
      new_tensor(l.outputs[0], a.C, a.H, a.W);
    } else if (l.type == "Interp") {
      LP_CHECK(l.ipar(0, 0) == 1 && l.fpar(1, 1.0) == 2.0 && l.fpar(2, 1.0) == 2.0, LP_ERR_GRAPH, "Interp %s: only nearest x2 supported", l.name.c_str());
      const Tensor a = tensors_[get(l.inputs[0])];
      new_tensor(l.outputs[0], a.C, 2 * a.H, 2 * a.W);
    } else {
      throw Error(LP_ERR_GRAPH, fmt("unsupported NCNN layer type %s (%s)", l.type.c_str(), l.name.c_str()));
    }
  }
  LP_CHECK(input_tensor >= 0, LP_ERR_GRAPH, "graph has no Input layer");
  for (auto& t : tensors_) {
    t.Cp = 0;
    for (int s : t.segs) t.Cp += round_up(s, 8);
  }
}

int Planner::alloc_buffer(int Cp, int H, int W) {
  buffers_.emplace_back();
  Buffer& b = buffers_.back();
  b.Cp = Cp; b.H = H; b.W = W;
  b.mem.alloc((size_t)maxB_ * H * W * Cp * es);
  return (int)buffers_.size() - 1;
}

void Planner::ensure_buffer(int t) {
  Tensor& T = tensors_[t];
  LP_CHECK(T.parent < 0, LP_ERR_GRAPH, "blob %s is a slice and cannot be produced directly", T.name.c_str());
  if (T.buf < 0) { T.buf = alloc_buffer(T.Cp, T.H, T.W); T.off = 0; }
  T.materialised = true;
}

// ---- pass B: place concat inputs inside the concat buffer -----------------------------------
void Planner::place_concats() {
  for (int i = 0; i < n; ++i) {
    if (is_tail(i) || L[i].type != "Concat") continue;
    const int tout = get(L[i].outputs[0]);
    Tensor& O = tensors_[tout];
    if (O.buf < 0) { O.buf = alloc_buffer(O.Cp, O.H, O.W); O.off = 0; }
    int o = O.off;
    size_t j = 0;
    while (j < L[i].inputs.size()) {
      const int t = get(L[i].inputs[j]);
      Tensor& T = tensors_[t];
      if (T.parent >= 0) {
        Tensor& P = tensors_[T.parent];
        const size_t m = P.segs.size();
        bool whole = T.parent_seg == 0 && j + m <= L[i].inputs.size() && P.buf < 0;
        for (size_t q = 0; whole && q < m; ++q) {
          const Tensor& Q = tensors_[get(L[i].inputs[j + q])];
          whole = Q.parent == T.parent && Q.parent_seg == (int)q;
        }
        if (whole) {
          P.buf = O.buf; P.off = o;
          o += P.Cp;
          j += m;
          continue;
        }
        copies.push_back({i, t, O.buf, o});
      } else if (T.buf < 0) {
        T.buf = O.buf; T.off = o;
      } else {
        copies.push_back({i, t, O.buf, o});
      }
      o += T.Cp;
      ++j;
    }
    LP_CHECK(o - O.off == O.Cp, LP_ERR_GRAPH, "Concat %s: layout bookkeeping error", L[i].name.c_str());
  }
}

// ---- weights -------------------------------------------------------------------------------
// NCNN [out][in][kh][kw] -> [out][tap][in] (3x3) / [out][in] (1x1) for layers without padded channel segments
std::vector<float> Planner::conv_w(int j) const {
  const NcnnLayer& lc = L[j];
  const int k = lc.ipar(1, 1), co = lc.ipar(0), ci = lc.in_ch, taps = k * k;
  std::vector<float> w((size_t)co * taps * ci);
  for (int o = 0; o < co; ++o)
    for (int c = 0; c < ci; ++c)
      for (int t = 0; t < taps; ++t) w[((size_t)o * taps + t) * ci + c] = lc.weight[((size_t)o * ci + c) * taps + t];
  return w;
}

// The same over PHYSICAL channels (zeros at padding channels): layer lc reads tensor I and writes tensor O, whose channels start
// at row out_base of a weight block of cout_phys rows [row][tap][I.Cp] (a block that several layers fill is sized by the first).
void Planner::repack(const NcnnLayer& lc, const Tensor& I, const Tensor& O, int out_base, int cout_phys, std::vector<float>& w,
                     std::vector<float>& b) const {
  const int k = lc.ipar(1, 1), taps = k * k, co_n = lc.ipar(0), ci_n = lc.in_ch;
  w.resize((size_t)cout_phys * taps * I.Cp, 0.f);
  b.resize(cout_phys, 0.f);
  for (int co = 0; co < co_n; ++co) {
    const int pc = out_base + O.phys(co);
    for (int ci = 0; ci < ci_n; ++ci) {
      const int pi = I.phys(ci);
      for (int t = 0; t < taps; ++t) w[((size_t)pc * taps + t) * I.Cp + pi] = lc.weight[((size_t)co * ci_n + ci) * taps + t];
    }
    if (!lc.bias.empty()) b[pc] = lc.bias[co];
  }
}

// ---- whole-C2f launches (LITEPI_NO_C2F=1: off).  match_c2f recognises, from its cv1, a complete C2f module:
//      Convolution 1x1 + Swish -> Slice (c | c) -> n x [3x3 + Swish -> 3x3 + Swish -> BinaryOp add] ->
//      Concat(y0 .. y_{n+1}) (zero-copy, pass B) -> Convolution 1x1 + Swish.  It has no side effects on `done`.
bool Planner::match_c2f(int i1, C2fMatch& m) {
  if (!is_silu_conv(i1, 1, 1)) return false;
  const int t1 = cinfo[i1].tout;
  const Tensor& T1 = tensors_[t1];
  if (T1.segs.size() != 2 || T1.segs[0] != T1.segs[1] || T1.parent >= 0) return false;
  const int c = T1.segs[0];
  if (c % 8 != 0 || tensors_[cinfo[i1].tin].Cp != L[i1].in_ch) return false;
  const int sl = sole_consumer(t1);
  if (sl < 0 || L[sl].type != "Slice" || L[sl].outputs.size() != 2) return false;
  const int ty0 = get(L[sl].outputs[0]), ty1 = get(L[sl].outputs[1]);
  const int cc = sole_consumer(ty0);
  if (cc < 0 || L[cc].type != "Concat" || is_tail(cc) || !zero_copy_concat(cc)) return false;
  m = C2fMatch();
  m.cv1 = i1; m.slice = sl; m.cat = cc; m.c = c;
  m.ys = {ty0, ty1};
  int cur = ty1;
  for (;;) {
    int ja = -1, jadd = -1;
    bool has_cat = false;
    for (int q : canon_consumers[tensors_[cur].name]) {
      if (q == cc) has_cat = true;
      else if (L[q].type == "Convolution" && ja == -1) ja = q;
      else if (L[q].type == "BinaryOp" && jadd == -1) jadd = q;
      else return false;
    }
    if (!has_cat) return false;
    if (ja == -1 && jadd == -1) break;
    if (!match_c2f_bottleneck(m, cur, ja, jadd)) return false;
    cur = m.ys.back();
  }
  if (m.nb < 1 || L[cc].inputs.size() != m.ys.size()) return false;
  for (size_t q = 0; q < m.ys.size(); ++q)
    if (get(L[cc].inputs[q]) != m.ys[q]) return false;
  m.t_cat = get(L[cc].outputs[0]);
  const Tensor& TC = tensors_[m.t_cat];
  if (TC.parent >= 0 || TC.buf < 0 || TC.Cp != (2 + m.nb) * c || T1.buf != TC.buf || T1.off != TC.off) return false;
  for (size_t q = 2; q < m.ys.size(); ++q) {
    const Tensor& Y = tensors_[m.ys[q]];
    if (Y.buf != TC.buf || Y.off != TC.off + (int)q * c || Y.Cp != c) return false;
  }
  m.cv2 = sole_consumer(m.t_cat);
  if (!is_silu_conv(m.cv2, 1, 1)) return false;
  const Tensor& TO = tensors_[cinfo[m.cv2].tout];
  if (TO.Cp != L[m.cv2].ipar(0) || TO.parent >= 0) return false;
  return !feeds_add(cinfo[m.cv2].tout);
}

// one bottleneck of the module: y = cur + silu(conv3x3(silu(conv3x3(cur)))) through layers ja -> jb -> jadd; appends y to m.ys
bool Planner::match_c2f_bottleneck(C2fMatch& m, int cur, int ja, int jadd) {
  const int c = m.c;
  if (ja < 0 || jadd < 0 || m.nb >= 2) return false;
  if (!is_silu_conv(ja, 3, 1) || L[ja].ipar(0) != c || L[ja].in_ch != c) return false;
  const int jb = sole_consumer(cinfo[ja].tout);
  if (!is_silu_conv(jb, 3, 1) || L[jb].ipar(0) != c || L[jb].in_ch != c) return false;
  if (sole_consumer(cinfo[jb].tout) != jadd || is_tail(jadd) || done[jadd]) return false;
  const NcnnLayer& add = L[jadd];
  if (add.ipar(0, 0) != 0 || add.inputs.size() != 2 || add.ipar(1, 0) != 0) return false;
  const int ta = get(add.inputs[0]), tb = get(add.inputs[1]);
  if (!((ta == cinfo[jb].tout && tb == cur) || (tb == cinfo[jb].tout && ta == cur))) return false;
  m.a[m.nb] = ja; m.b[m.nb] = jb; m.add[m.nb] = jadd;
  ++m.nb;
  m.ys.push_back(get(add.outputs[0]));
  return true;
}

C2fShape Planner::c2f_shape(const C2fMatch& m, int mode, int ks2) {
  C2fShape s;
  s.C = m.c; s.NB = m.nb; s.COUT = L[m.cv2].ipar(0); s.MODE = mode; s.KS2 = ks2;
  const int tin = cinfo[m.cv1].tin;
  if (fuse_up.count(m.cv1)) {
    s.UP = 1;
    s.KA = tensors_[fuse_up[m.cv1]].Cp;
    s.KB = tensors_[tin].Cp - s.KA;
  } else {
    s.KB = tensors_[tin].Cp;
  }
  return s;
}

bool Planner::c2f_plain_ok(int i1) {   // a stand-alone C2f launch exists for the module whose cv1 is layer i1
  C2fMatch m;
  if (!c2f_on || !match_c2f(i1, m)) return false;
  const Tensor& T = tensors_[cinfo[i1].tout];
  return c2f_ok(c2f_shape(m, 0, 0), T.H, T.W);
}

// The SPPF chain from its cv1 (layer j1, a 1x1 SiLU conv the caller has checked): three chained pools that nothing else reads,
// the zero-copy Concat of cv1's output and the pooled maps in that order, and the 1x1 SiLU conv that is its only consumer.
bool Planner::match_sppf_chain(int j1, SppfChain& s) {
  s = SppfChain();
  s.cv1 = j1;
  int cur = cinfo[j1].tout, cc = -1;
  s.chain[0] = cur;
  for (int q = 0; q < 3; ++q) {
    int jp = -1;
    for (int cq : canon_consumers[tensors_[cur].name]) {
      if (L[cq].type == "Pooling" && jp < 0) jp = cq;
      else if (L[cq].type == "Concat" && (cc < 0 || cc == cq)) cc = cq;
      else return false;
    }
    if (jp < 0 || done[jp]) return false;
    s.pools[q] = jp;
    cur = get(L[jp].outputs[0]);
    s.chain[q + 1] = cur;
  }
  for (int cq : canon_consumers[tensors_[cur].name])
    if (cq != cc) return false;
  if (cc < 0 || is_tail(cc) || !zero_copy_concat(cc) || L[cc].inputs.size() != 4) return false;
  for (int q = 0; q < 4; ++q)
    if (get(L[cc].inputs[q]) != s.chain[q]) return false;
  s.cat = cc;
  s.t_cat = get(L[cc].outputs[0]);
  if (tensors_[s.t_cat].parent >= 0) return false;
  s.cv2 = sole_consumer(s.t_cat);
  if (!is_silu_conv(s.cv2, 1, 1)) return false;
  const Tensor& TO = tensors_[cinfo[s.cv2].tout];
  return TO.Cp == L[s.cv2].ipar(0) && TO.parent < 0;
}

// stride-2 conv i -> [Concat(x, other) ->] cv1 of a C2f module: whole-image configurations only
bool Planner::match_s2_front(int i, C2fMatch& m, int& xcat) {
  const int tx = cinfo[i].tout;
  if (tensors_[tx].segs.size() != 1 || tensors_[tx].Cp != L[i].ipar(0) || tensors_[cinfo[i].tin].Cp != L[i].in_ch) return false;
  int jn = sole_consumer(tx);
  if (jn >= 0 && L[jn].type == "Concat" && !is_tail(jn)) {
    const int tcat_in = get(L[jn].outputs[0]);
    if (L[jn].inputs.size() != 2 || get(L[jn].inputs[0]) != tx || !zero_copy_concat(jn) || tensors_[tx].buf != tensors_[tcat_in].buf ||
        tensors_[tx].off != tensors_[tcat_in].off || tensors_[tcat_in].parent >= 0)
      return false;
    // the launch is emitted at the stride-2 conv's position, and cv1 reads the whole Concat(x, other): `other` must
    // have been produced by then.  Layers are emitted in file order, so its producer has to precede this conv (true for
    // the reference's graphs: P5 / F4 come earlier); otherwise the module is retried at its cv1, behind the Concat.
    auto po = producer.find(L[jn].inputs[1]);
    if (po != producer.end() && po->second >= i) return false;
    xcat = jn;
    jn = sole_consumer(tcat_in);
  }
  return jn >= 0 && match_c2f(jn, m) && !fuse_up.count(jn) && L[i].ipar(0) == 2 * m.c;
}

// try_c2f also folds in the stride-2 3x3 conv in front of the module and the SPPF behind it when a whole-image
// configuration exists for the level.
bool Planner::try_c2f(int i) {
  if (!c2f_on) return false;
  C2fMatch m;
  int i0 = -1, xcat = -1, mode = 0;
  if (is_silu_conv(i, 3, 2)) {
    if (!match_s2_front(i, m, xcat)) return false;
    i0 = i;
    mode = 1;
  } else if (!match_c2f(i, m)) {
    return false;
  }
  const int tout = cinfo[m.cv2].tout;
  const int Hh = tensors_[tout].H, Ww = tensors_[tout].W;
  // SPPF behind the module, its widths those of the module and its concat laid out segment by segment
  SppfChain sp;
  if (mode == 1) {
    const int j = sole_consumer(tout);
    bool ok = is_silu_conv(j, 1, 1) && L[j].ipar(0) == m.c && tensors_[cinfo[j].tout].segs.size() == 1 && match_sppf_chain(j, sp);
    if (ok) {
      const Tensor& TC2 = tensors_[sp.t_cat];
      ok = TC2.buf >= 0 && TC2.Cp == 4 * m.c && L[sp.cv2].ipar(0) == L[m.cv2].ipar(0);
      for (int q = 0; q < 4 && ok; ++q)
        ok = tensors_[sp.chain[q]].buf == TC2.buf && tensors_[sp.chain[q]].off == TC2.off + q * m.c && tensors_[sp.chain[q]].Cp == m.c;
    }
    if (ok) mode = 2;
  }
  C2fShape sh = c2f_shape(m, mode, i0 >= 0 ? L[i0].in_ch : 0);
  if (!c2f_ok(sh, Hh, Ww)) {
    if (mode == 2) { mode = 1; sh = c2f_shape(m, 1, L[i0].in_ch); }
    if (!c2f_ok(sh, Hh, Ww)) return false;   // (a stride-2 conv falls through to its own kernel; the module is tried again at its cv1)
  }
  emit_c2f(m, mode, sh, i0, xcat, mode == 2 ? &sp : nullptr);
  return true;
}

// Build the C2fLayer of a match and emit its op.  mode as C2fShape::MODE: -1 without cv1 (behind a stride-2 conv + cv1 launch),
// 0 the module, 1 with the stride-2 conv i0 in front (xcat: the Concat between them, or -1), 2 also with the SPPF sp behind.
void Planner::emit_c2f(const C2fMatch& m, int mode, const C2fShape& sh, int i0, int xcat, const SppfChain* sp) {
  const int tout = cinfo[m.cv2].tout;
  const int Hh = tensors_[tout].H, Ww = tensors_[tout].W;
  std::vector<float> w_cv1, w_cv2 = conv_w(m.cv2), w_a[2], w_b[2], w_s2, w_sp1, w_sp2;
  C2fLayer::Src src;
  if (mode >= 0) { w_cv1 = conv_w(m.cv1); src.cv1 = &w_cv1; src.cv1_b = &L[m.cv1].bias; }
  src.cv2 = &w_cv2; src.cv2_b = &L[m.cv2].bias;
  for (int k = 0; k < m.nb; ++k) {
    w_a[k] = conv_w(m.a[k]); w_b[k] = conv_w(m.b[k]);
    src.a[k] = &w_a[k]; src.a_b[k] = &L[m.a[k]].bias;
    src.bb[k] = &w_b[k]; src.bb_b[k] = &L[m.b[k]].bias;
  }
  if (mode >= 1) { w_s2 = conv_w(i0); src.s2 = &w_s2; src.s2_b = &L[i0].bias; }
  if (mode == 2) {
    w_sp1 = conv_w(sp->cv1); w_sp2 = conv_w(sp->cv2);
    src.sp1 = &w_sp1; src.sp1_b = &L[sp->cv1].bias;
    src.sp2 = &w_sp2; src.sp2_b = &L[sp->cv2].bias;
  }
  d.c2fs_.emplace_back(new C2fLayer());
  C2fLayer& cl = *d.c2fs_.back();
  cl.name = (i0 >= 0 ? L[i0].name + "+" : std::string()) + L[mode < 0 ? m.a[0] : m.cv1].name + ".." + L[m.cv2].name + (mode == 2 ? "+sppf" : "");
  cl.build(sh, Hh, Ww, src);
  cl.store_all = sw.c2f_store_all;
  C2fIO io;
  io.src1 = mode < 0 ? m.t_cat : cinfo[m.cv1].tin;   // (unused by MODE -1: the module reads the concat buffer)
  if (mode >= 0 && sh.UP) { io.src0 = fuse_up[m.cv1]; io.up_c = sh.KA; }
  io.cat = m.t_cat;
  io.out = tout;
  ensure_buffer(tout);
  // (the y segments cv2 takes from LDS are only stored in the bisect mode, LITEPI_C2F_STORE_ALL=1)
  for (size_t q = 2; q < m.ys.size(); ++q) tensors_[m.ys[q]].materialised = sw.c2f_store_all || !cl.cv2_from_lds();
  if (mode >= 1) {
    io.s2_in = cinfo[i0].tin;
    io.x = cinfo[i0].tout;
    if (xcat < 0) ensure_buffer(io.x);
    else tensors_[io.x].materialised = true;
  }
  double bytes = ((double)tensors_[io.src1].C * Hh * Ww + (double)tensors_[tout].C * Hh * Ww) * esd;
  if (mode < 0) bytes = ((double)tensors_[m.t_cat].C * 0.5 + (double)tensors_[tout].C) * Hh * Ww * esd;
  if (mode >= 0 && sh.UP) bytes -= 0.75 * sh.KA * Hh * Ww * esd;   // the upsampled segment is read at half resolution
  if (mode >= 1) bytes += ((double)sh.KS2 * 4 - (xcat < 0 ? (double)tensors_[io.src1].C : (double)tensors_[io.x].C)) * Hh * Ww * esd;
  if (mode == 2) {
    io.cat2 = sp->t_cat;
    io.out2 = cinfo[sp->cv2].tout;
    ensure_buffer(io.out2);
    if (sw.c2f_store_all) {   // (s and the pooled maps stay in LDS otherwise: sppf_tail)
      for (int q = 0; q < 3; ++q) tensors_[sp->chain[q + 1]].materialised = true;
      tensors_[sp->chain[0]].materialised = true;
    }
    bytes += ((double)tensors_[io.out2].C - (double)tensors_[tout].C) * Hh * Ww * esd;
  }
  if (!sw.c2f_store_all) mark_inside_c2f(m, mode, io, sp);
  d.c2f_io_.push_back(io);
  macs_ += cl.macs_per_image;
  DetOp op;
  op.kind = DetOp::C2F; op.conv = (int)d.c2fs_.size() - 1; op.layer = cl.name;
  op.in = io.src1; op.out = mode == 2 ? io.out2 : tout;
  op.flops = 2.0 * cl.macs_per_image;
  op.bytes = bytes;
  ops_.push_back(op);
  done[m.cv1] = done[m.cv2] = 1;   // (MODE -1: cv1 is already claimed as the tail of the conv in front)
  for (int k = 0; k < m.nb; ++k) done[m.a[k]] = done[m.b[k]] = done[m.add[k]] = 1;
  if (i0 >= 0) done[i0] = 1;
  if (mode == 2) { done[sp->cv1] = done[sp->cv2] = 1; done[sp->pools[0]] = done[sp->pools[1]] = done[sp->pools[2]] = 1; }
}

// every tensor between the launch's input and its output: lp_debug_blob must not hand out their (possibly never
// written) storage -- which of them a configuration stores is the kernel's business (c2f_kernels.hip)
void Planner::mark_inside_c2f(const C2fMatch& m, int mode, const C2fIO& io, const SppfChain* sp) {
  auto inside = [&](int t) { if (t >= 0 && t != io.out && (mode != 2 || t != io.out2)) tensors_[t].in_c2f = true; };
  if (mode >= 0) { inside(cinfo[m.cv1].tout); inside(m.t_cat); }   // (MODE -1: cv1's output y0 | y1 is the launch's input)
  for (size_t q = mode < 0 ? 2 : 0; q < m.ys.size(); ++q) inside(m.ys[q]);
  for (int k = 0; k < m.nb; ++k) {
    inside(cinfo[m.a[k]].tout); inside(cinfo[m.b[k]].tout);
    for (auto& o : L[m.add[k]].outputs) inside(get(o));
  }
  if (mode >= 1) inside(io.x);
  if (mode == 2) {
    tensors_[io.out].in_c2f = true;   // the C2f's own output: SPPF.cv1 reads it from LDS
    for (int q = 0; q < 4; ++q) inside(sp->chain[q]);
    inside(io.cat2);
  }
}

// ---- SPPF in one launch (sppf_kernel; the widths the whole-image C2f kernel does not take along: v2's 192 -> 96 -> 192 @20x20);
//      s and the pooled maps stay in LDS, the concat buffer is never written
bool Planner::try_sppf(int i) {
  if (!c2f_on || !is_silu_conv(i, 1, 1)) return false;
  const int tin = cinfo[i].tin, ts = cinfo[i].tout;
  if (tensors_[ts].segs.size() != 1 || tensors_[tin].Cp != L[i].in_ch || tensors_[ts].Cp != L[i].ipar(0)) return false;
  SppfChain sp;
  const int c = L[i].ipar(0);
  if (!match_sppf_chain(i, sp) || tensors_[sp.t_cat].Cp != 4 * c) return false;
  const int j2 = sp.cv2, tc2 = sp.t_cat, tout = cinfo[j2].tout;
  if (tensors_[tout].segs.size() != 1 || feeds_add(tout)) return false;
  const int Hh = tensors_[ts].H, Ww = tensors_[ts].W;
  if (!sppf_ok(L[i].in_ch, c, L[j2].ipar(0), Hh, Ww)) return false;
  d.sppfs_.emplace_back(new SppfLayer());
  SppfLayer& sl = *d.sppfs_.back();
  sl.name = L[i].name + "+pools+" + L[j2].name;
  sl.build(L[i].in_ch, c, L[j2].ipar(0), Hh, Ww, conv_w(i), L[i].bias, conv_w(j2), L[j2].bias);
  ensure_buffer(tout);
  for (int q = 0; q < 4; ++q) tensors_[sp.chain[q]].in_c2f = true;   // never written: lp_debug_blob must not hand them out
  tensors_[tc2].in_c2f = true;
  macs_ += sl.macs_per_image;
  DetOp op;
  op.kind = DetOp::SPPFUSED; op.conv = (int)d.sppfs_.size() - 1; op.layer = sl.name; op.in = tin; op.out = tout;
  op.flops = 2.0 * sl.macs_per_image;
  op.bytes = ((double)tensors_[tin].C + (double)tensors_[tout].C) * Hh * Ww * esd + (double)(L[i].weight.size() + L[j2].weight.size()) * esd;
  ops_.push_back(op);
  done[i] = done[j2] = done[sp.pools[0]] = done[sp.pools[1]] = done[sp.pools[2]] = 1;
  return true;
}

// ---- pass D: emit ops, layers in file order ----------------------------------------------------
void Planner::emit_ops() {
  done.assign(n, 0);
  macs_ = 0;
  for (int i = 0; i < first_tail; ++i) {
    if ((is_tail(i) && L[i].type != "Convolution") || skip[i] || done[i]) continue;
    const std::string& type = L[i].type;
    if (in_attn[i]) {
      if (attn_at.count(i)) emit_attention(i);
    } else if (type == "ConvolutionDepthWise") emit_dwconv(i);
    else if (type == "Convolution") emit_convolution(i);
    else if (type == "BinaryOp") emit_add(i);
    else if (type == "Pooling") emit_pool_chain(i);
    else if (type == "Interp") emit_interp(i);
    else if (type == "Concat") emit_concat_copies(i);
  }
}

// The fusion rules of one Convolution, in the order that is the planner's contract: the first rule that claims the layer emits it.
void Planner::emit_convolution(int i) {
  if (try_c2f(i) || try_sppf(i)) return;
  const NcnnLayer& l = L[i];
  ConvSite c{i, cinfo[i].tin, cinfo[i].tout, l.ipar(1, 1), l.ipar(3, 1), l.ipar(0), l.in_ch};
  take_residual(c);   // moves c.tout to the add's output and claims the add before the later rules look
  if (try_sibling_merge(c) || try_bottleneck(c)) return;
  pick_1x1_tail(c);
  ensure_buffer(c.tout);
  if (try_s2c_with_tail(c) || try_s2c(c)) return;
  emit_stem_or_conv(c);
}

// residual fusion: the activation output feeds exactly one BinaryOp add
void Planner::take_residual(ConvSite& c) {
  auto& cs = canon_consumers[tensors_[c.tout].name];
  if (cs.size() != 1 || L[cs[0]].type != "BinaryOp" || is_tail(cs[0])) return;
  const NcnnLayer& add = L[cs[0]];
  const int ta = get(add.inputs[0]), tb = get(add.inputs[1]);
  const int other = ta == c.tout ? tb : ta;
  if (other != c.tout && tensors_[other].Cp == tensors_[c.tout].Cp) {
    c.res = other;
    c.tout = get(add.outputs[0]);
    done[cs[0]] = 1;
  }
}

// sibling merge: another plain 3x3 conv reads the same input (Detect head: the box and class branches of a
// level both start with a 3x3 conv on the neck output): one launch computes both, output channels side by
// side in one buffer -- the input is read once and a launch disappears.  LITEPI_NO_SIBLING=1 disables it.
int Planner::find_sibling(const ConvSite& c) {
  const int i = c.i, tin = c.tin, tout = c.tout;
  if (sw.no_sibling || c.res >= 0 || c.k != 3 || c.s != 1 || tin == input_tensor || impl_ != IMPL_MFMA || tensors_[tout].buf >= 0 ||
      tensors_[tout].parent >= 0 || tensors_[tout].segs.size() != 1)
    return -1;
  for (int j = i + 1; j < first_tail; ++j) {
    if (L[j].type != "Convolution" || done[j] || skip[j] || is_tail(j) || cinfo[j].tin != tin) continue;
    const int tj = cinfo[j].tout;
    // (the outputs must stay plain tensors: no fused add on them)
    if (L[j].ipar(1, 1) == 3 && L[j].ipar(3, 1) == 1 && fused_act[j] == fused_act[i] && tensors_[tj].buf < 0 &&
        tensors_[tj].parent < 0 && tensors_[tj].segs.size() == 1 && !feeds_add(tj) && !feeds_add(tout) &&
        L[j].bias.empty() == L[i].bias.empty())
      return j;
  }
  return -1;
}

bool Planner::try_sibling_merge(const ConvSite& c) {
  const int sib = find_sibling(c);
  if (sib < 0) return false;
  const int i = c.i, tin = c.tin, tout = c.tout;
  const NcnnLayer &l = L[i], &l2 = L[sib];
  const int t2 = cinfo[sib].tout;
  const int cpa = tensors_[tout].Cp, cpb = tensors_[t2].Cp, Ho = tensors_[tout].H, Wo = tensors_[tout].W;
  const int CpO = cpa + cpb;
  const int nb = alloc_buffer(CpO, Ho, Wo);
  tensors_[tout].buf = nb; tensors_[tout].off = 0; tensors_[tout].materialised = true;
  tensors_[t2].buf = nb; tensors_[t2].off = cpa; tensors_[t2].materialised = true;
  const Tensor& TI = tensors_[tin];
  std::vector<float> w, b;
  repack(l, TI, tensors_[tout], 0, CpO, w, b);
  repack(l2, TI, tensors_[t2], cpa, CpO, w, b);
  convs_.emplace_back(new ConvLayer());
  convs_.back()->name = l.name + "|" + l2.name;
  convs_.back()->build(prec_, impl_, 3, 1, TI.Cp, CpO, fused_act[i], w, b, Ho, Wo, maxB_);
  const double macs = 9.0 * c.Cin * (c.Cout + l2.ipar(0)) * Ho * Wo;
  macs_ += macs;
  DetOp op;
  op.kind = DetOp::CONV; op.layer = convs_.back()->name; op.conv = (int)convs_.size() - 1;
  op.flops = 2.0 * macs;
  op.bytes = ((double)TI.C * TI.H * TI.W + (double)(c.Cout + l2.ipar(0)) * Ho * Wo) * esd + (double)(l.weight.size() + l2.weight.size()) * esd;
  // a tensor that stands for the merged buffer (the conv's output view); pushed last: it invalidates references
  Tensor M = tensors_[tout];
  M.name = tensors_[tout].name + "|" + tensors_[t2].name; M.C = tensors_[tout].C + tensors_[t2].C; M.Cp = CpO;
  M.segs = {cpa, cpb}; M.buf = nb; M.off = 0;
  tensors_.push_back(M);
  op.in = tin; op.out = (int)tensors_.size() - 1;
  ops_.push_back(op);
  done[sib] = 1;
  return true;
}

// bottleneck fusion: this 3x3 conv feeds exactly one 3x3 conv whose activation is added to THIS conv's
// input (C2f.m[i] with shortcut): both convs, the SiLUs and the add become one launch, the intermediate
// stays in LDS (BottleneckPair).  LITEPI_NO_BNECK=1 keeps the layer-at-a-time plan (A/B measurements).
bool Planner::try_bottleneck(const ConvSite& c) {
  const int i = c.i, tin = c.tin, tout = c.tout, Cin = c.Cin, Cout = c.Cout;
  const NcnnLayer& l = L[i];
  if (sw.no_bneck || c.res >= 0 || c.k != 3 || c.s != 1 || Cin != Cout || tin == input_tensor || impl_ != IMPL_MFMA ||
      fused_act[i] != ACT_SILU || tensors_[tout].segs.size() != 1 || tensors_[tin].segs.size() != 1)
    return false;
  const int j = sole_consumer(tout);
  if (j < 0 || L[j].type != "Convolution" || is_tail(j) || done[j]) return false;
  const NcnnLayer& lb = L[j];
  const int tb = cinfo[j].tout;
  const int jadd = sole_consumer(tb);
  if (lb.ipar(1, 1) != 3 || lb.ipar(3, 1) != 1 || lb.ipar(0) != Cout || lb.in_ch != Cout || fused_act[j] != ACT_SILU || jadd < 0 ||
      L[jadd].type != "BinaryOp" || is_tail(jadd))
    return false;
  const NcnnLayer& add = L[jadd];
  const int ta = get(add.inputs[0]), tb2 = get(add.inputs[1]);
  const int other = ta == tb ? tb2 : ta;
  const int tfinal = get(add.outputs[0]);
  const Tensor& TI = tensors_[tin];
  if (other != tin || TI.Cp != tensors_[tfinal].Cp || TI.Cp != tensors_[tout].Cp || !BottleneckPair::supported(prec_, impl_, TI.Cp, TI.H, TI.W, maxB_))
    return false;
  std::optional<Cv2Match> f = match_bneck_cv2(tin, tfinal);
  if (f) { f->cv2.w = &f->w; f->cv2.bias = &f->b; }
  const int jc = f ? f->conv : -1, tcat = f ? f->t_cat : -1;
  const int tdst = jc >= 0 ? cinfo[jc].tout : tfinal;
  ensure_buffer(tdst);
  // the kernel's 32-bit byte offsets: every buffer it indexes must stay below 2^31 bytes at the handle's capacity, else the layer plan
  auto span_ok = [&](int t) {
    if (t < 0) return true;
    const Tensor& X = tensors_[t];
    const int bi = X.parent >= 0 ? tensors_[X.parent].buf : X.buf;
    return bi < 0 || cplan::bneck_span_ok(maxB_, X.H, X.W, buffers_[bi].Cp, (int)esd);
  };
  if (!span_ok(tin) || !span_ok(tdst) || !span_ok(tcat)) return false;
  std::vector<float> wa, ba, wb, bb;
  repack(l, TI, tensors_[tout], 0, tensors_[tout].Cp, wa, ba);
  repack(lb, tensors_[tout], tensors_[tfinal], 0, tensors_[tfinal].Cp, wb, bb);
  d.bnecks_.emplace_back(new BottleneckPair());
  d.bnecks_.back()->name = l.name + "+" + lb.name + (jc >= 0 ? "+" + L[jc].name : std::string());
  d.bnecks_.back()->build(prec_, TI.Cp, wa, ba, wb, bb, TI.H, TI.W, maxB_, jc >= 0 ? &f->cv2 : nullptr);
  double macs = 2.0 * 9.0 * Cin * Cout * TI.H * TI.W;
  if (jc >= 0) macs += (double)L[jc].in_ch * L[jc].ipar(0) * TI.H * TI.W;
  macs_ += macs;
  DetOp op;
  op.kind = DetOp::BNECK; op.layer = d.bnecks_.back()->name; op.conv = (int)d.bnecks_.size() - 1;
  op.flops = 2.0 * macs;
  op.bytes = 2.0 * TI.C * TI.H * TI.W * esd + (double)(l.weight.size() + lb.weight.size()) * esd;
  if (jc >= 0)
    op.bytes = ((double)(tensors_[tcat].C - TI.C) + TI.C + tensors_[tdst].C) * TI.H * TI.W * esd +
               (double)(l.weight.size() + lb.weight.size() + L[jc].weight.size()) * esd;
  op.in = tin; op.out = tdst; op.in2 = tcat;
  ops_.push_back(op);
  if (jc >= 0) done[jc] = 1;
  done[j] = 1; done[jadd] = 1;
  return true;
}

// cv2 fusion: the bottleneck's output y_last (tfinal) is the last segment of a zero-copy Concat whose only consumer is a 1x1
// conv (C2f.cv2): that conv runs in the same launch, y_last stays in registers (LITEPI_NO_CV2FUSE=1: off).  The caller points
// cv2.w / cv2.bias at the returned weights.
std::optional<Planner::Cv2Match> Planner::match_bneck_cv2(int tin, int tfinal) {
  const int cc = sole_consumer(tfinal);
  if (sw.no_cv2fuse || cc < 0 || L[cc].type != "Concat" || canon(L[cc].inputs.back()) != tensors_[tfinal].name) return std::nullopt;
  const int tO = get(L[cc].outputs[0]);
  const int j3 = sole_consumer(tO);
  if (!zero_copy_concat(cc) || j3 < 0 || L[j3].type != "Convolution" || is_tail(j3) || done[j3] || L[j3].ipar(1, 1) != 1 ||
      L[j3].ipar(3, 1) != 1 || fuse_up.count(j3) || tensors_[tfinal].buf != tensors_[tO].buf || tensors_[tO].parent >= 0)
    return std::nullopt;
  const int t3 = cinfo[j3].tout;
  const Tensor &TI = tensors_[tin], &TO = tensors_[tO];
  const int glob = tensors_[tfinal].off - TO.off;
  if (feeds_add(t3) || glob <= 0 || glob + TI.Cp != TO.Cp || tensors_[t3].segs.size() != 1) return std::nullopt;
  Cv2Match f;
  f.cv2.cat_global = glob; f.cv2.c3 = tensors_[t3].Cp; f.cv2.act = fused_act[j3];
  // (C2f: the bottleneck's input y_n sits right in front of y_last in the concat buffer)
  int bi = TI.buf, oi = TI.off;   // storage of the input: a Slice output is a view of its parent's segment (view())
  if (TI.parent >= 0) {
    const Tensor& P = tensors_[TI.parent];
    oi = P.off; bi = P.buf;
    for (int k2 = 0; k2 < TI.parent_seg; ++k2) oi += round_up(P.segs[k2], 8);
  }
  f.cv2.in_is_last_stored = bi >= 0 && bi == TO.buf && oi == TO.off + glob - TI.Cp;
  f.cv2.cl = sw.bneck_cl;
  if (!BottleneckPair::supported(prec_, impl_, TI.Cp, TI.H, TI.W, maxB_, &f.cv2)) return std::nullopt;
  f.conv = j3; f.t_cat = tO;
  repack(L[j3], TO, tensors_[t3], 0, f.cv2.c3, f.w, f.b);
  return f;
}

// 1x1 tail fusion: this 3x3 conv's activation output feeds exactly one 1x1 conv (Detect-head
// projections, C2f cv1 after a stride-2 conv): the second GEMM runs on the accumulator tile
void Planner::pick_1x1_tail(ConvSite& c) {
  if (c.res >= 0 || c.k != 3 || c.tin == input_tensor || impl_ != IMPL_MFMA) return;
  const int tout = c.tout;
  const int j = sole_consumer(tout);
  if (j < 0 || L[j].type != "Convolution" || is_tail(j) || done[j]) return;
  const NcnnLayer& lb = L[j];
  const int tb = cinfo[j].tout;
  const bool plain1x1 = lb.ipar(1, 1) == 1 && lb.ipar(3, 1) == 1 && tensors_[tout].segs.size() == 1;
  // B must not itself be the producer of a fused residual add
  const bool b_feeds_add = feeds_add(tb);
  // (a C2f.cv1 that the whole-C2f launch computes itself is not folded into this conv)
  // (a stride-2 conv whose 1x1 consumer is the cv1 of a C2f module that can run WITHOUT its cv1 -- C2fShape::MODE -1 -- keeps
  //  that cv1 as its tail on the LDS-staged kernel even though a whole-module launch exists: v2's 80x80 backbone module.  Claimed
  //  only when try_s2c_with_tail will emit that launch, hence the same predicate: ConvLayer has no 48 -> 48 tail to fall back on)
  bool s2tail = false;
  if (plain1x1 && !sw.no_c2f_xcv1 && tensors_[tout].Cp == 48 && s2c_tail_ok(c, j, tout, tb)) {
    C2fMatch mx;
    s2tail = match_c2f(j, mx) && c2f_ok(c2f_shape(mx, -1, 0), tensors_[tb].H, tensors_[tb].W);
  }
  if (plain1x1 && !b_feeds_add && (s2tail || (!c2f_plain_ok(j) && ConvLayer::tail_supported(c.k, c.s, tensors_[tout].Cp, tensors_[tb].Cp)))) {
    c.tail = j;
    c.tmid = tout;
    c.tout = tb;
    done[j] = 1;
  }
}

// May this load run stride-2 conv c with the 1x1 conv `tail` folded in as ONE launch of the LDS-staged kernel?  tmid: the conv's own
// output, tout: the tail's.  Asked by pick_1x1_tail before it claims v2's cv1 as a tail, and by try_s2c_with_tail before it emits.
bool Planner::s2c_tail_ok(const ConvSite& c, int tail, int tmid, int tout) const {
  const int i = c.i, tin = c.tin, Cin = c.Cin, Cout = c.Cout;
  return c2f_on && !sw.no_s2c && !sw.no_s2lds && !sw.no_s2tail && c.res < 0 && c.k == 3 && c.s == 2 && fused_act[i] == ACT_SILU &&
         fused_act[tail] == ACT_SILU && !L[i].bias.empty() && !L[tail].bias.empty() && tin != input_tensor && tensors_[tin].Cp == Cin &&
         tensors_[tmid].Cp == Cout && tensors_[tout].Cp == L[tail].ipar(0) && tensors_[tout].parent < 0 &&
         S2ConvLayer::tail_supported(Cin, Cout, L[tail].ipar(0), tensors_[tout].H, tensors_[tout].W);
}

// a stride-2 conv WITH its folded 1x1 tail on the LDS-staged kernel (v1's conv_6 + conv_7: s2lds_kernel<S2L16x32t>)
bool Planner::try_s2c_with_tail(const ConvSite& c) {
  if (c.tail < 0 || !s2c_tail_ok(c, c.tail, c.tmid, c.tout)) return false;
  emit_s2c(c);
  emit_c2f_behind_tail(c);
  return true;
}

// The C2f module the folded cv1 (c.tail) belongs to, WITHOUT its cv1 (C2fShape::MODE -1: y0 | y1 come from the concat buffer the
// launch in front fills; for n = 2 modules cv1 on the halo-4 region was twice its work): both bottlenecks + cv2 in one launch.
// On for v2's module, whose alternative is the whole-module launch with cv1 recomputed on the halo-4 region.  Opt-in for v1's
// (LITEPI_C2F_XCV1=1), the 80x80 backbone module: 56.0 us against 25.0 + 33.1 for the two bottleneck launches, 19 launches,
// +0.1 to +0.5 % end to end: inside the noise, so the two-launch plan stays the default.
void Planner::emit_c2f_behind_tail(const ConvSite& c) {
  C2fMatch m;
  done[c.tail] = 0;   // (match_c2f wants its cv1 unclaimed)
  const bool ok = (sw.c2f_xcv1 || (c.Cout == 48 && !sw.no_c2f_xcv1)) && match_c2f(c.tail, m);
  done[c.tail] = 1;
  if (!ok) return;
  const C2fShape sh = c2f_shape(m, -1, 0);
  const Tensor& T2 = tensors_[cinfo[m.cv2].tout];
  if (c2f_ok(sh, T2.H, T2.W)) emit_c2f(m, -1, sh, -1, -1, nullptr);
}

// a stride-2 conv without a folded tail whose shape the c2f machinery covers: s2conv_kernel (LITEPI_NO_S2C=1: off)
bool Planner::try_s2c(const ConvSite& c) {
  const int i = c.i, tin = c.tin, tout = c.tout, Cin = c.Cin, Cout = c.Cout;
  const NcnnLayer& l = L[i];
  if (c.tail >= 0 || c.res >= 0 || c.k != 3 || c.s != 2 || fused_act[i] != ACT_SILU || l.bias.empty() ||
      tin == input_tensor || tensors_[tin].Cp != Cin || tensors_[tout].Cp != Cout || tensors_[tout].segs.size() != 1 ||
      !s2c_ok(Cin, Cout, tensors_[tout].H, tensors_[tout].W))
    return false;
  emit_s2c(c);
  return true;
}

// the S2ConvLayer of a stride-2 conv (with c.tail, its folded 1x1, when it has one) and its op
void Planner::emit_s2c(const ConvSite& c) {
  const NcnnLayer& l = L[c.i];
  const NcnnLayer* lt = c.tail >= 0 ? &L[c.tail] : nullptr;
  const Tensor& TI = tensors_[c.tin];
  const Tensor& TO = tensors_[c.tout];
  d.s2cs_.emplace_back(new S2ConvLayer());
  S2ConvLayer& sc = *d.s2cs_.back();
  sc.name = lt ? l.name + "+" + lt->name : l.name;
  const std::vector<float> w2 = lt ? conv_w(c.tail) : std::vector<float>();
  sc.build(c.Cin, c.Cout, TO.H, TO.W, conv_w(c.i), l.bias, lt ? &w2 : nullptr, lt ? &lt->bias : nullptr);
  const double macs = (9.0 * c.Cin * c.Cout + (lt ? (double)c.Cout * lt->ipar(0) : 0.0)) * TO.H * TO.W;
  macs_ += macs;
  DetOp op;
  op.kind = DetOp::S2C; op.conv = (int)d.s2cs_.size() - 1; op.layer = sc.name; op.in = c.tin; op.out = c.tout;
  op.flops = 2.0 * macs;
  op.bytes = ((double)TI.C * TI.H * TI.W + (double)TO.C * TO.H * TO.W) * esd + (double)(l.weight.size() + (lt ? lt->weight.size() : 0)) * esd;
  ops_.push_back(op);
}

// the conv kernels proper: what no fusion rule claimed (with its residual and its 1x1 tail, when it has them)
void Planner::emit_stem_or_conv(const ConvSite& c) {
  const NcnnLayer& l = L[c.i];
  const Tensor& TI = tensors_[c.tin];
  const Tensor& TO = tensors_[c.tail >= 0 ? c.tmid : c.tout];
  double macs = (double)c.k * c.k * c.Cin * c.Cout * TO.H * TO.W;
  if (c.tail >= 0) macs += (double)L[c.tail].in_ch * L[c.tail].ipar(0) * TO.H * TO.W;
  macs_ += macs;
  DetOp op;
  op.layer = l.name;
  op.flops = 2.0 * macs;
  op.bytes = ((double)TI.C * TI.H * TI.W + (double)TO.C * TO.H * TO.W * (c.res >= 0 ? 2 : 1)) * esd + (double)l.weight.size() * esd;
  op.in = c.tin; op.out = c.tout; op.res = c.res;
  if (c.tin == input_tensor) emit_stem(c, op);
  else emit_conv(c, op);
  ops_.push_back(op);
}

void Planner::emit_stem(const ConvSite& c, DetOp& op) {
  const NcnnLayer& l = L[c.i];
  const Tensor& TI = tensors_[c.tin];
  const Tensor& TO = tensors_[c.tail >= 0 ? c.tmid : c.tout];
  const int k = c.k;
  LP_CHECK(c.Cin == 3 && k >= 1 && k <= 7, LP_ERR_GRAPH, "first convolution must read the 3-channel image with k <= 7");
  // weights in BGR order, [k*k*3][CO]
  const int CO = TO.Cp;
  std::vector<float> w((size_t)k * k * 3 * CO, 0.f), b(CO, 0.f);
  for (int co = 0; co < c.Cout; ++co) {
    const int pc = TO.phys(co);
    for (int ch = 0; ch < 3; ++ch)
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
          w[(size_t)((ky * k + kx) * 3 + (2 - ch)) * CO + pc] = l.weight[(((size_t)co * 3 + ch) * k + ky) * k + kx];
    if (!l.bias.empty()) b[pc] = l.bias[co];
  }
  d.stem_.build(prec_, CO, fused_act[c.i], w, b, k, c.s, l.ipar(4, 0));
  op.kind = DetOp::STEM;
  op.bytes = (double)3 * TI.H * TI.W + (double)TO.C * TO.H * TO.W * esd;
}

void Planner::emit_conv(const ConvSite& c, DetOp& op) {
  const int i = c.i, tail = c.tail;
  const NcnnLayer& l = L[i];
  const Tensor& TI = tensors_[c.tin];
  const Tensor& TO = tensors_[tail >= 0 ? c.tmid : c.tout];
  std::vector<float> w, b;
  repack(l, TI, TO, 0, TO.Cp, w, b);
  convs_.emplace_back(new ConvLayer());
  convs_.back()->name = l.name;
  convs_.back()->build(prec_, impl_, c.k, c.s, TI.Cp, TO.Cp, fused_act[i], w, b, TO.H, TO.W, maxB_, tail >= 0);
  if (tail >= 0) {
    const NcnnLayer& lb = L[tail];
    const Tensor& TB = tensors_[c.tout];
    std::vector<float> w2, b2;
    repack(lb, TO, TB, 0, TB.Cp, w2, b2);
    convs_.back()->attach_tail(TB.Cp, fused_act[tail], w2, b2);
    convs_.back()->name = l.name + "+" + lb.name;
    op.layer = convs_.back()->name;
    op.bytes = ((double)TI.C * TI.H * TI.W + (double)TB.C * TB.H * TB.W) * esd + (double)(l.weight.size() + lb.weight.size()) * esd;
  }
  op.kind = DetOp::CONV;
  op.conv = (int)convs_.size() - 1;
  if (fuse_up.count(i)) {
    op.in2 = fuse_up[i];
    op.layer = l.name + "(up)";
    op.bytes -= 0.75 * tensors_[op.in2].C * 4.0 * tensors_[op.in2].H * tensors_[op.in2].W * esd;  // u is read once, not its x4 copy
  }
}

// ---- the other layer kinds ---------------------------------------------------------------------
void Planner::emit_attention(int i) {
  const AttnBlock& a = attn_at[i];
  const int tin = get(a.in_blob), tout = get(a.out_blob);
  ensure_buffer(tout);
  const NcnnLayer& dw = L[a.dw];
  const int Cv = a.heads * a.dv;
  d.attns_.emplace_back();
  Detector::AttnLayer& A = d.attns_.back();
  A.heads = a.heads; A.dk = a.dk; A.dv = a.dv; A.scale = a.scale;
  std::vector<float> w((size_t)9 * Cv, 0.f), b(Cv, 0.f);
  for (int c = 0; c < Cv; ++c) {
    for (int t = 0; t < 9; ++t) w[(size_t)t * Cv + c] = dw.weight[(size_t)c * 9 + t];
    if (!dw.bias.empty()) b[c] = dw.bias[c];
  }
  upload(A.pe_w, w);
  upload(A.pe_b, b);
  const Tensor& TI = tensors_[tin];
  DetOp op;
  op.kind = DetOp::ATTN; op.layer = L[i].name; op.conv = (int)d.attns_.size() - 1; op.in = tin; op.out = tout;
  op.flops = 2.0 * a.heads * (double)a.hw * a.hw * (a.dk + a.dv);
  op.bytes = ((double)TI.C + Cv) * TI.H * TI.W * esd;
  ops_.push_back(op);
}

void Planner::emit_dwconv(int i) {
  const NcnnLayer& l = L[i];
  const int tin = cinfo[i].tin, tout = cinfo[i].tout;
  const Tensor& TI = tensors_[tin];
  LP_CHECK(TI.segs.size() == 1 && tensors_[tout].segs.size() == 1 && TI.Cp == tensors_[tout].Cp, LP_ERR_GRAPH,
           "ConvolutionDepthWise %s: input and output must be plain tensors", l.name.c_str());
  ensure_buffer(tout);
  const int C = l.ipar(0), Cp = TI.Cp;
  d.dws_.emplace_back();
  Detector::DwLayer& D = d.dws_.back();
  D.act = fused_act[i];
  std::vector<float> w((size_t)9 * Cp, 0.f), b(Cp, 0.f);
  for (int c = 0; c < C; ++c) {
    for (int t = 0; t < 9; ++t) w[(size_t)t * Cp + TI.phys(c)] = l.weight[(size_t)c * 9 + t];
    if (!l.bias.empty()) b[TI.phys(c)] = l.bias[c];
  }
  upload(D.w, w);
  upload(D.b, b);
  DetOp op;
  op.kind = DetOp::DWCONV; op.layer = l.name; op.conv = (int)d.dws_.size() - 1; op.in = tin; op.out = tout;
  op.flops = 2.0 * 9.0 * C * TI.H * TI.W;
  op.bytes = 2.0 * C * TI.H * TI.W * esd;
  macs_ += 9.0 * C * TI.H * TI.W;
  ops_.push_back(op);
}

void Planner::emit_add(int i) {
  const NcnnLayer& l = L[i];
  DetOp op;
  op.kind = DetOp::ADD; op.layer = l.name;
  op.in = get(l.inputs[0]); op.in2 = get(l.inputs[1]); op.out = get(l.outputs[0]);
  ensure_buffer(op.out);
  const Tensor& T = tensors_[op.out];
  op.bytes = 3.0 * T.C * T.H * T.W * esd;
  ops_.push_back(op);
}

// SPPF on the layer plan: this pool and the two that consume it in a chain
void Planner::emit_pool_chain(int i) {
  const NcnnLayer& l = L[i];
  int chain[3] = {i, -1, -1};
  for (int q = 1; q < 3; ++q) {
    auto& cs = canon_consumers[canon(L[chain[q - 1]].outputs[0])];
    for (int c : cs)
      if (L[c].type == "Pooling") chain[q] = c;
    LP_CHECK(chain[q] >= 0, LP_ERR_GRAPH, "Pooling %s is not part of an SPPF chain of three", l.name.c_str());
  }
  DetOp op;
  op.kind = DetOp::SPPF; op.layer = l.name;
  op.in = get(l.inputs[0]);
  op.out = get(L[chain[0]].outputs[0]); op.out2 = get(L[chain[1]].outputs[0]); op.out3 = get(L[chain[2]].outputs[0]);
  ensure_buffer(op.out); ensure_buffer(op.out2); ensure_buffer(op.out3);
  done[chain[1]] = done[chain[2]] = 1;
  const Tensor& T = tensors_[op.in];
  op.bytes = 4.0 * T.C * T.H * T.W * esd;
  ops_.push_back(op);
}

// upsample fusion: Interp x2 -> first input of a Concat -> exactly one 1x1 conv (FPN top-down: C2f.cv1).  The conv
// gathers those channels from the half-resolution tensor itself; the upsampled copy is never materialised (LITEPI_NO_UPFUSE=1: off).
void Planner::emit_interp(int i) {
  const NcnnLayer& l = L[i];
  const int tsrc = get(l.inputs[0]), tup = get(l.outputs[0]);
  auto& c1 = canon_consumers[canon(l.outputs[0])];
  if (!sw.no_upfuse && impl_ == IMPL_MFMA && c1.size() == 1 && L[c1[0]].type == "Concat" && canon(L[c1[0]].inputs[0]) == canon(l.outputs[0])) {
    auto& c2 = canon_consumers[canon(L[c1[0]].outputs[0])];
    if (c2.size() == 1 && L[c2[0]].type == "Convolution" && L[c2[0]].ipar(1, 1) == 1 && L[c2[0]].ipar(3, 1) == 1 &&
        !is_tail(c2[0]) && tensors_[tup].off == 0 && tensors_[tsrc].Cp % 8 == 0 &&
        tensors_[tup].buf >= 0 && tensors_[tup].buf == tensors_[get(L[c1[0]].outputs[0])].buf &&  // zero-copy segment 0
        tensors_[tsrc].Cp == tensors_[tup].Cp) {
      fuse_up[c2[0]] = tsrc;
      return;
    }
  }
  DetOp op;
  op.kind = DetOp::UPSAMPLE; op.layer = l.name;
  op.in = tsrc; op.out = tup;
  ensure_buffer(op.out);
  const Tensor& T = tensors_[op.out];
  op.bytes = 1.25 * T.C * T.H * T.W * esd;
  ops_.push_back(op);
}

// the Concat inputs that pass B could not place inside the concat buffer
void Planner::emit_concat_copies(int i) {
  for (auto& cj : copies) {
    if (cj.layer != i) continue;
    // destination view = slice of the concat buffer
    Tensor dst = tensors_[cj.src];
    dst.name += "@cat"; dst.parent = -1; dst.buf = cj.dst_buf; dst.off = cj.dst_off;
    tensors_.push_back(dst);
    DetOp op;
    op.kind = DetOp::COPY; op.layer = L[i].name; op.in = cj.src; op.out = (int)tensors_.size() - 1;
    op.bytes = 2.0 * dst.C * dst.H * dst.W * esd;
    ops_.push_back(op);
  }
}

// ---- stem block: stem + the stride-2 conv that is its only consumer (+ that conv's fused 1x1 tail) in one launch;
//      the 320x320 stem map is never stored (StemLayer::launch_block; LITEPI_NO_STEMBLOCK=1: off)
void Planner::fuse_stem_block() {
  if (sw.no_stemblock || ops_.size() < 2 || ops_[0].kind != DetOp::STEM || ops_[1].kind != DetOp::CONV || ops_[1].in != ops_[0].out ||
      ops_[1].res >= 0 || SW_ % 4 != 0 || canon_consumers[tensors_[ops_[0].out].name].size() != 1 ||
      !d.stem_.block_supported(*convs_[ops_[1].conv]))
    return;
  const Tensor& TI = tensors_[ops_[0].in >= 0 ? ops_[0].in : input_tensor];
  const Tensor& TO = tensors_[ops_[1].out];
  ops_[0].kind = DetOp::STEMBLOCK;
  ops_[0].conv = ops_[1].conv;
  ops_[0].out = ops_[1].out;
  ops_[0].layer += "+" + ops_[1].layer;
  ops_[0].flops += ops_[1].flops;
  ops_[0].bytes = 3.0 * TI.H * TI.W + (double)TO.C * TO.H * TO.W * esd;
  ops_.erase(ops_.begin() + 1);
}

// ---- Detect tail ---------------------------------------------------------------------------
void Planner::build_detect_tail() {
  int& reg_max_ = d.reg_max_;
  int &A_ = d.A_, &nc_ = d.nc_;
  reg_max_ = 0;
  const NcnnLayer* anchors = nullptr;
  const NcnnLayer* strides = nullptr;
  for (int i = 0; i < n; ++i) {
    if (L[i].type == "Convolution" && i >= first_tail) {
      LP_CHECK(L[i].bias.empty() && L[i].ipar(0) == 1, LP_ERR_GRAPH, "unexpected convolution %s in the Detect tail", L[i].name.c_str());
      dfl = L[i].weight;
      reg_max_ = (int)dfl.size();
    }
    if (L[i].type == "MemoryData") {
      if (L[i].ipar(1, 0) == 2 && !anchors) anchors = &L[i];
      if (L[i].ipar(1, 0) == 0 && L[i].ipar(2, 0) == 0 && !strides) strides = &L[i];
    }
  }
  LP_CHECK(reg_max_ > 0 && reg_max_ <= 32, LP_ERR_GRAPH, "no DFL convolution found in the Detect tail");
  LP_CHECK(anchors && strides, LP_ERR_GRAPH, "anchor / stride constants missing from the Detect tail");
  A_ = 0;
  nc_ = -1;
  for (int hc : head_cats) {
    Level lv;
    lv.box = get(L[hc].inputs[0]);
    lv.cls = get(L[hc].inputs[1]);
    const Tensor& B = tensors_[lv.box];
    const Tensor& C = tensors_[lv.cls];
    LP_CHECK(B.C == 4 * reg_max_ && B.segs.size() == 1 && C.segs.size() == 1 && B.H == C.H && B.W == C.W, LP_ERR_GRAPH,
             "Detect head %s: box branch must have 4*reg_max channels", L[hc].name.c_str());
    LP_CHECK(nc_ < 0 || nc_ == C.C, LP_ERR_GRAPH, "Detect head: class count differs between levels");
    nc_ = C.C;
    lv.H = B.H; lv.W = B.W; lv.off = A_;
    A_ += B.H * B.W;
    levels_.push_back(lv);
  }
  // the NMS kernel packs the anchor index into 14 bits of its sort key and keeps every candidate of an image in one
  // workgroup's LDS: reject larger heads here, at load time, not on every call (a 1024x1024 input has 21504 anchors)
  LP_CHECK(A_ <= 16384, LP_ERR_GRAPH, "Detect head with %d anchors: at most 16384 are supported (input size %dx%d is too large)", A_, SH_, SW_);
  LP_CHECK((int)anchors->data.size() == 2 * A_ && (int)strides->data.size() == A_, LP_ERR_GRAPH,
           "anchor tables (%zu, %zu) do not match %d anchors", anchors->data.size(), strides->data.size(), A_);
  for (auto& lv : levels_) {
    const float st = strides->data[lv.off];
    LP_CHECK(st * lv.H == (float)SH_ && st * lv.W == (float)SW_, LP_ERR_GRAPH, "stride table does not match level %dx%d of a %dx%d input", lv.H, lv.W,
             SH_, SW_);
  }
  upload(d.d_anchors_, anchors->data);
  upload(d.d_strides_, strides->data);
  upload(d.d_dfl_, dfl);
}

// ---- Detect-head fusion (fp16 MFMA plan; LITEPI_NO_HEADFUSE=1: off).  Per level the planner has emitted three ops:
//      A = the two first 3x3 convs merged (sibling merge: box tower 64 | class tower c3 channels in one buffer),
//      B = box tower's second 3x3 + its 1x1 projection (fused tail), C = the same for the class tower.  When every level
//      has exactly this shape, each (A, B, C) triple becomes one HEAD op (head_fused_kernel) that also decodes and filters,
//      and the stand-alone decode launch disappears.
bool Planner::match_head_level(const Level& lv, Trip& t) {
  const int ob = conv_producer_of(lv.box);
  int oc = conv_producer_of(lv.cls), oproj = -1;
  if (ob < 0 || oc < 0) return false;
  // class tower: second 3x3 with the projection as its fused tail, or (48-channel towers: no tail kernel for three
  // channel tiles) the 3x3 and the 1x1 as two launches
  if (convs_[ops_[oc].conv]->k == 1) {
    const ConvLayer& cp = *convs_[ops_[oc].conv];
    oproj = oc;
    oc = conv_producer_of(ops_[oproj].in);
    if (oc < 0 || cp.T2 != 0 || cp.act != ACT_NONE || ops_[oproj].res >= 0 || ops_[oproj].in2 >= 0 || cp.Cin != convs_[ops_[oc].conv]->Cout ||
        convs_[ops_[oc].conv]->T2 != 0 || cp.b_host.empty())
      return false;
  }
  const ConvLayer& cb = *convs_[ops_[ob].conv];
  const ConvLayer& cc = *convs_[ops_[oc].conv];
  const Tensor& tb = tensors_[ops_[ob].in];
  const Tensor& tc = tensors_[ops_[oc].in];
  bool ok = cb.k == 3 && cb.stride == 1 && cb.T2 > 0 && cb.act == ACT_SILU && cb.act2 == ACT_NONE && cb.Cin == 64 && cb.Cout == 64 &&
            cb.Cout2 == 64 && cc.k == 3 && cc.stride == 1 && (oproj >= 0 || (cc.T2 > 0 && cc.act2 == ACT_NONE)) && cc.act == ACT_SILU && cc.Cin == cc.Cout &&
            ops_[ob].res < 0 && ops_[oc].res < 0 && tb.buf >= 0 && tb.buf == tc.buf && tb.parent < 0 && tc.parent < 0 && tb.off == 0 &&
            tc.off == tb.Cp && tb.Cp == 64 && tc.Cp == cc.Cin && buffers_[tb.buf].Cp == 64 + cc.Cin;
  int oa = -1;
  for (size_t q = 0; ok && q < ops_.size(); ++q)
    if (ops_[q].kind == DetOp::CONV && ops_[q].out >= 0 && tensors_[ops_[q].out].buf == tb.buf && (int)q != ob && (int)q != oc && (int)q != oproj) oa = (int)q;
  ok = ok && oa >= 0 && oa < ob && oa < oc;
  if (ok) {
    const ConvLayer& ca = *convs_[ops_[oa].conv];
    const Tensor& ti = tensors_[ops_[oa].in];
    ok = ca.k == 3 && ca.stride == 1 && ca.T2 == 0 && ca.act == ACT_SILU && ca.Cout == 64 + cc.Cin && ops_[oa].res < 0 && ops_[oa].in2 < 0 &&
         ca.Cin == ti.Cp && !ca.b_host.empty() && tensors_[lv.cls].C == d.nc_ &&
         HeadLayer::supported(ca.Cin, 64, cc.Cin, d.nc_, d.reg_max_, sw.head);
  }
  if (ok) t = {oa, ob, oc, cc.Cin, oproj};
  return ok;
}

void Planner::fuse_heads() {
  if (sw.no_headfuse || prec_ != LP_FP16 || impl_ != IMPL_MFMA || d.reg_max_ != 16) return;
  std::vector<Trip> trips;
  for (auto& lv : levels_) {
    Trip t;
    if (!match_head_level(lv, t)) return;
    trips.push_back(t);
  }
  // Two class row tiles (48-channel class towers, v2): stage A on 16-pixel tiles, P3 and P4 at two workgroups per CU and a
  // one-round P5 shape make it the faster plan (same-box A/B 53.4 k -> 54.2 k images/s, 53 -> 43 launches), so it is the
  // default; LITEPI_HEADFUSE=narrow restores the three-launch plan for A/B
  if (trips.empty() || (trips[0].c3 > 32 && sw.headfuse_narrow)) return;
  std::vector<char> dead(ops_.size(), 0);
  for (size_t q = 0; q < trips.size(); ++q) {
    const Trip& t = trips[q];
    const ConvLayer& ca = *convs_[ops_[t.a].conv];
    const ConvLayer& cb = *convs_[ops_[t.b].conv];
    const ConvLayer& cc = *convs_[ops_[t.c].conv];
    HeadLayer::Src src;
    src.wa = &ca.w_host; src.ba = &ca.b_host;
    src.wbb = &cb.w_host; src.bbb = &cb.b_host; src.wpb = &cb.w2_host; src.bpb = &cb.b2_host;
    src.wbc = &cc.w_host; src.bbc = &cc.b_host; src.wpc = &cc.w2_host; src.bpc = &cc.b2_host;
    src.ncp = cc.Cout2;
    if (t.proj >= 0) {
      const ConvLayer& cp = *convs_[ops_[t.proj].conv];
      src.wpc = &cp.w_host; src.bpc = &cp.b_host; src.ncp = cp.Cout;
    }
    d.heads_.emplace_back(new HeadLayer());
    d.heads_.back()->name = ops_[t.a].layer + "+" + ops_[t.b].layer + "+" + ops_[t.c].layer + "+decode";
    d.heads_.back()->build(ca.Cin, t.c3, d.nc_, levels_[q].H, levels_[q].W, sw.head, src);
    DetOp& op = ops_[t.a];
    op.kind = DetOp::HEAD; op.conv = (int)d.heads_.size() - 1; op.in2 = (int)q; op.out = -1;
    op.layer = d.heads_.back()->name;
    op.flops = ops_[t.a].flops + ops_[t.b].flops + ops_[t.c].flops + (t.proj >= 0 ? ops_[t.proj].flops : 0.0);
    op.bytes = (double)tensors_[op.in].C * levels_[q].H * levels_[q].W * esd;
    dead[t.b] = dead[t.c] = 1;
    if (t.proj >= 0) dead[t.proj] = 1;
  }
  std::vector<DetOp> kept;
  for (size_t q = 0; q < ops_.size(); ++q)
    if (!dead[q]) kept.push_back(ops_[q]);
  ops_.swap(kept);
  d.fused_head_ = true;
}

void Detector::load(const std::string& param_path, const std::string& bin_path) {
  NcnnGraph g;
  g.load(param_path, bin_path);
  load_graph(std::move(g), param_path);
}

// The plan of a graph a reader has produced (ncnn_graph.cpp, onnx_graph.cpp); `name` stands for the model file in messages.
void Detector::load_graph(NcnnGraph&& graph, const std::string& name) {
  Planner p(*this, std::move(graph), name);   // clears the previous plan
  p.find_detect_tail();
  p.find_attention_blocks();
  p.resolve_aliases_and_swish();
  p.make_tensors();
  p.place_concats();
  p.emit_ops();
  p.fuse_stem_block();
  p.build_detect_tail();
  p.fuse_heads();
  loaded_ = true;
}

}  // namespace lp
