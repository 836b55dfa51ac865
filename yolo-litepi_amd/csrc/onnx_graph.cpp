// ONNX detector export -> NcnnGraph.  Two halves: a protobuf wire-format walker for the messages of onnx.proto3 a detector
// export uses, and the lowering of its nodes to the NCNN layers ncnn_graph.cpp reads and the planner recognises.
//
// Field numbers (onnx.proto3): ModelProto.opset_import = 8, .graph = 7; OperatorSetIdProto.domain = 1, .version = 2;
// GraphProto.node = 1, .initializer = 5, .input = 11, .output = 12; ValueInfoProto.name = 1;
// NodeProto.input = 1, .output = 2, .name = 3, .op_type = 4, .attribute = 5;
// AttributeProto.name = 1, .f = 2, .i = 3, .s = 4, .t = 5, .floats = 7, .ints = 8;
// TensorProto.dims = 1, .data_type = 2, .float_data = 4, .int32_data = 5, .int64_data = 7, .name = 8, .raw_data = 9,
// .data_location = 14; data types FLOAT = 1, INT32 = 6, INT64 = 7.
#include "onnx_graph.h"

#include <algorithm>
#include <fstream>
#include <set>

namespace lp {
namespace {

// ---- wire format ----------------------------------------------------------------------------------------------------------------
struct Rd {
  const uint8_t* p;
  const uint8_t* e;
  struct Field { int no, wt; uint64_t v; const uint8_t* b; size_t len; };   // v: varint / fixed bits; [b, b + len): bytes

  bool more() const { return p < e; }
  uint64_t varint() {
    uint64_t v = 0;
    for (int shift = 0; shift < 64; shift += 7) {
      LP_CHECK(p < e, LP_ERR_GRAPH, "ONNX file is truncated (inside a varint)");
      const uint8_t b = *p++;
      v |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) return v;
    }
    throw Error(LP_ERR_GRAPH, "ONNX file is malformed (varint longer than 10 bytes)");
  }
  Field field() {
    const uint64_t key = varint();
    Field f{(int)std::min<uint64_t>(key >> 3, 1u << 30), (int)(key & 7), 0, nullptr, 0};
    LP_CHECK(f.no > 0, LP_ERR_GRAPH, "ONNX file is malformed (field number 0)");
    if (f.wt == 0) {
      f.v = varint();
    } else if (f.wt == 1 || f.wt == 5) {
      const size_t n = f.wt == 1 ? 8 : 4;
      LP_CHECK((size_t)(e - p) >= n, LP_ERR_GRAPH, "ONNX file is truncated (inside a fixed-width field)");
      memcpy(&f.v, p, n);
      f.b = p; f.len = n;
      p += n;
    } else if (f.wt == 2) {
      const uint64_t n = varint();
      LP_CHECK(n <= (uint64_t)(e - p), LP_ERR_GRAPH, "ONNX file is truncated (a field of %llu bytes, %zu left)", (unsigned long long)n, (size_t)(e - p));
      f.b = p; f.len = (size_t)n;
      p += n;
    } else {
      throw Error(LP_ERR_GRAPH, fmt("ONNX file is malformed (wire type %d)", f.wt));
    }
    return f;
  }
};

Rd sub(const Rd::Field& f) {
  LP_CHECK(f.wt == 2, LP_ERR_GRAPH, "ONNX file is malformed (field %d is not a message)", f.no);
  return Rd{f.b, f.b + f.len};
}
std::string str(const Rd::Field& f) {
  LP_CHECK(f.wt == 2, LP_ERR_GRAPH, "ONNX file is malformed (field %d is not a string)", f.no);
  return std::string(reinterpret_cast<const char*>(f.b), f.len);
}
void add_ints(const Rd::Field& f, std::vector<int64_t>& out) {   // a repeated integer field, packed or not
  if (f.wt == 0) { out.push_back((int64_t)f.v); return; }
  Rd r = sub(f);
  while (r.more()) out.push_back((int64_t)r.varint());
}
void add_floats(const Rd::Field& f, std::vector<float>& out) {
  LP_CHECK(f.wt == 5 || (f.wt == 2 && f.len % 4 == 0), LP_ERR_GRAPH, "ONNX file is malformed (field %d is not a float list)", f.no);
  for (size_t o = 0; o < f.len; o += 4) {
    float v;
    memcpy(&v, f.b + o, 4);
    out.push_back(v);
  }
}

// ---- the messages -----------------------------------------------------------------------------------------------------------------
enum { DT_FLOAT = 1, DT_INT32 = 6, DT_INT64 = 7 };

struct OTensor {
  std::string name;
  std::vector<int64_t> dims;
  int dtype = 0;
  std::vector<float> f;     // FLOAT
  std::vector<int64_t> i;   // INT64 / INT32
  size_t numel() const { return dtype == DT_FLOAT ? f.size() : i.size(); }
};

OTensor parse_tensor(Rd r) {
  OTensor t;
  const uint8_t* raw = nullptr;
  size_t raw_len = 0;
  std::vector<int64_t> i32;
  bool external = false;
  while (r.more()) {
    const Rd::Field f = r.field();
    if (f.no == 1) add_ints(f, t.dims);
    else if (f.no == 2 && f.wt == 0) t.dtype = (int)std::min<uint64_t>(f.v, 1000);
    else if (f.no == 4) add_floats(f, t.f);
    else if (f.no == 5) add_ints(f, i32);
    else if (f.no == 7) add_ints(f, t.i);
    else if (f.no == 8) t.name = str(f);
    else if (f.no == 9 && f.wt == 2) { raw = f.b; raw_len = f.len; }
    else if (f.no == 14 && f.wt == 0) external = f.v != 0;
  }
  LP_CHECK(!external, LP_ERR_GRAPH, "initializer %s keeps its data in an external file: unsupported", t.name.c_str());
  uint64_t n = 1;
  for (int64_t d : t.dims) {
    LP_CHECK(d >= 0 && d <= (int64_t)1 << 31, LP_ERR_GRAPH, "initializer %s: bad dimension %lld", t.name.c_str(), (long long)d);
    n *= (uint64_t)d;
    LP_CHECK(n <= (uint64_t)1 << 31, LP_ERR_GRAPH, "initializer %s: too many elements", t.name.c_str());
  }
  if (t.dtype == DT_FLOAT) {
    if (raw) {
      LP_CHECK(raw_len % 4 == 0, LP_ERR_GRAPH, "initializer %s: raw_data is not a whole number of floats", t.name.c_str());
      t.f.resize(raw_len / 4);
      if (raw_len) memcpy(t.f.data(), raw, raw_len);
    }
    t.i.clear();
  } else if (t.dtype == DT_INT64 || t.dtype == DT_INT32) {
    const size_t w = t.dtype == DT_INT64 ? 8 : 4;
    if (t.dtype == DT_INT32) t.i = i32;
    if (raw) {
      LP_CHECK(raw_len % w == 0, LP_ERR_GRAPH, "initializer %s: raw_data is not a whole number of integers", t.name.c_str());
      t.i.resize(raw_len / w);
      for (size_t k = 0; k < t.i.size(); ++k) {
        if (w == 8) { memcpy(&t.i[k], raw + 8 * k, 8); }
        else { int32_t v; memcpy(&v, raw + 4 * k, 4); t.i[k] = v; }
      }
    }
    t.f.clear();
  } else {
    t.f.clear();
    t.i.clear();
    return t;   // (another element type: refused where a node uses it, with the node's name)
  }
  LP_CHECK(t.numel() == n, LP_ERR_GRAPH, "initializer %s: %zu values for a shape of %llu elements", t.name.c_str(), t.numel(), (unsigned long long)n);
  return t;
}

struct OAttr {
  std::string name, s;
  bool has_f = false, has_i = false, has_s = false, has_t = false;
  float f = 0.f;
  int64_t i = 0;
  OTensor t;
  std::vector<float> floats;
  std::vector<int64_t> ints;
};

struct ONode {
  int index = 0;   // position in the file's node list
  std::string op, name;
  std::vector<std::string> in, out;
  std::vector<OAttr> attrs;
  const OAttr* attr(const char* n) const {
    for (auto& a : attrs)
      if (a.name == n) return &a;
    return nullptr;
  }
  std::string label() const { return name.empty() ? op + "_" + std::to_string(index) : name; }   // a nameless node: <op>_<index>
};

ONode parse_node(Rd r) {
  ONode n;
  while (r.more()) {
    const Rd::Field f = r.field();
    if (f.no == 1) n.in.push_back(str(f));
    else if (f.no == 2) n.out.push_back(str(f));
    else if (f.no == 3) n.name = str(f);
    else if (f.no == 4) n.op = str(f);
    else if (f.no == 5) {
      OAttr a;
      Rd ar = sub(f);
      while (ar.more()) {
        const Rd::Field g = ar.field();
        if (g.no == 1) a.name = str(g);
        else if (g.no == 2 && g.wt == 5) { memcpy(&a.f, g.b, 4); a.has_f = true; }
        else if (g.no == 3 && g.wt == 0) { a.i = (int64_t)g.v; a.has_i = true; }
        else if (g.no == 4) { a.s = str(g); a.has_s = true; }
        else if (g.no == 5) { a.t = parse_tensor(sub(g)); a.has_t = true; }
        else if (g.no == 7) add_floats(g, a.floats);
        else if (g.no == 8) add_ints(g, a.ints);
      }
      n.attrs.push_back(std::move(a));
    }
  }
  return n;
}

struct OModel {
  int64_t opset = 0;
  std::vector<ONode> nodes;
  std::map<std::string, OTensor> init;
  std::vector<std::string> inputs, outputs;
};

std::string value_name(Rd r) {
  std::string name;
  while (r.more()) {
    const Rd::Field f = r.field();
    if (f.no == 1) name = str(f);
  }
  return name;
}

OModel parse_model(const uint8_t* data, size_t bytes, const std::string& src) {
  OModel m;
  Rd r{data, data + bytes};
  bool have_graph = false;
  while (r.more()) {
    const Rd::Field f = r.field();
    if (f.no == 8 && f.wt == 2) {
      Rd o = sub(f);
      std::string domain;
      int64_t version = 0;
      while (o.more()) {
        const Rd::Field g = o.field();
        if (g.no == 1) domain = str(g);
        else if (g.no == 2 && g.wt == 0) version = (int64_t)g.v;
      }
      if (domain.empty() || domain == "ai.onnx") m.opset = version;
    } else if (f.no == 7 && f.wt == 2) {
      have_graph = true;
      Rd g = sub(f);
      while (g.more()) {
        const Rd::Field h = g.field();
        if (h.no == 1) {
          m.nodes.push_back(parse_node(sub(h)));
          m.nodes.back().index = (int)m.nodes.size() - 1;
        }
        else if (h.no == 5) {
          OTensor t = parse_tensor(sub(h));
          std::string name = t.name;
          m.init[name] = std::move(t);
        } else if (h.no == 11) m.inputs.push_back(value_name(sub(h)));
        else if (h.no == 12) m.outputs.push_back(value_name(sub(h)));
      }
    }
  }
  LP_CHECK(have_graph && !m.nodes.empty(), LP_ERR_GRAPH, "%s: not an ONNX model (no graph with nodes)", src.c_str());
  return m;
}

// ---- lowering ---------------------------------------------------------------------------------------------------------------------
struct Op {
  NcnnLayer l;
  int group = 0;   // 0 backbone and neck, 1 Detect towers and their Concat, 2 Detect tail
};

struct Lowerer {
  const std::string& src;
  OModel m;
  std::vector<char> tail, absorbed;
  std::map<int, std::string> swish_in;            // Mul node -> x of x * sigmoid(x)
  std::map<std::string, std::vector<int>> cons;   // tensor -> consuming nodes
  std::map<std::string, int> made_by;             // tensor -> producing node
  std::vector<Op> ops;
  std::map<std::string, int> n_memdata;           // constant -> MemoryData layers made of it

  [[noreturn]] void bad(const ONode& n, const std::string& why) const {
    throw Error(LP_ERR_GRAPH, fmt("%s: node %s (op %s): %s", src.c_str(), n.label().c_str(), n.op.c_str(), why.c_str()));
  }
  const OTensor* init(const std::string& name) const {
    auto it = m.init.find(name);
    return it == m.init.end() ? nullptr : &it->second;
  }
  std::vector<int64_t> ints_attr(const ONode& n, const char* name, std::vector<int64_t> dflt) const {
    const OAttr* a = n.attr(name);
    return a ? a->ints : dflt;
  }
  int64_t int_attr(const ONode& n, const char* name, int64_t dflt) const {
    const OAttr* a = n.attr(name);
    return a && a->has_i ? a->i : dflt;
  }
  // the integer list a node takes as an input (Reshape's shape, Split's sizes, Slice's bounds): an INT64 / INT32 initializer
  std::vector<int64_t> ints_input(const ONode& n, size_t k, const char* what) const {
    const OTensor* t = k < n.in.size() && !n.in[k].empty() ? init(n.in[k]) : nullptr;
    if (!t) bad(n, std::string(what) + " is not a constant: dynamic shapes are not supported");
    if (t->dtype != DT_INT64 && t->dtype != DT_INT32) bad(n, std::string(what) + " is not an integer tensor");
    return t->i;
  }
  const std::string& data_in(const ONode& n, size_t k) const {
    if (k >= n.in.size() || n.in[k].empty()) bad(n, fmt("input %zu is missing", k));
    if (init(n.in[k])) bad(n, fmt("input %zu (%s) is a constant: unsupported here", k, n.in[k].c_str()));
    return n.in[k];
  }
  static int axis_of(int64_t a) { return (int)(a > 0 ? a - 1 : a); }   // NCNN axes do not count the batch dimension
  void check_small(const ONode& n, const std::vector<int64_t>& v, const char* what) const {   // values that become int parameters
    for (int64_t x : v)
      if (x < -(1 << 30) || x > (1 << 30)) bad(n, fmt("%s value %lld is out of range", what, (long long)x));
  }

  Lowerer(const std::string& s, OModel&& model) : src(s), m(std::move(model)) {}

  void fold_constants();
  void index();
  void find_tail();
  void find_swish();
  NcnnLayer& emit(const ONode& n, int idx, const char* type, std::vector<std::string> ins, std::vector<std::string> outs);
  void lower_node(int idx);
  void lower_conv(const ONode& n, int idx);
  void lower_binary(const ONode& n, int idx);
  std::string memory_data(const ONode& n, const OTensor& t);
  NcnnGraph finish();
};

// Constant nodes an exporter did not fold are initializers
void Lowerer::fold_constants() {
  std::vector<ONode> kept;
  for (auto& n : m.nodes) {
    if (n.op != "Constant") { kept.push_back(std::move(n)); continue; }
    if (n.out.size() != 1) bad(n, "a Constant has one output");
    OTensor t;
    if (const OAttr* a = n.attr("value")) {
      if (!a->has_t) bad(n, "attribute value holds no tensor");
      t = a->t;
    } else if (const OAttr* a = n.attr("value_float")) { t.dtype = DT_FLOAT; t.f = {a->f}; }
    else if (const OAttr* a = n.attr("value_floats")) { t.dtype = DT_FLOAT; t.f = a->floats; t.dims = {(int64_t)t.f.size()}; }
    else if (const OAttr* a = n.attr("value_int")) { t.dtype = DT_INT64; t.i = {a->i}; }
    else if (const OAttr* a = n.attr("value_ints")) { t.dtype = DT_INT64; t.i = a->ints; t.dims = {(int64_t)t.i.size()}; }
    else bad(n, "only tensor, float and integer constants are supported");
    t.name = n.out[0];
    m.init[n.out[0]] = std::move(t);
  }
  m.nodes.swap(kept);
}

void Lowerer::index() {
  std::vector<std::string> real_inputs;
  for (auto& i : m.inputs)
    if (!init(i)) real_inputs.push_back(i);
  LP_CHECK(real_inputs.size() == 1, LP_ERR_GRAPH, "%s: a detector takes one input, this graph has %zu", src.c_str(), real_inputs.size());
  m.inputs = real_inputs;
  LP_CHECK(m.outputs.size() == 1, LP_ERR_GRAPH, "%s: one output (out0) expected, this graph has %zu: exports with NMS inside are not supported",
           src.c_str(), m.outputs.size());
  for (int i = 0; i < (int)m.nodes.size(); ++i) {
    const ONode& n = m.nodes[i];
    for (auto& o : n.out) {
      if (o.empty()) continue;
      if (made_by.count(o) || init(o) || o == m.inputs[0]) bad(n, "output " + o + " is defined twice");
      made_by[o] = i;
    }
    for (auto& in : n.in)
      if (!in.empty()) cons[in].push_back(i);
  }
  for (auto& n : m.nodes)
    for (auto& in : n.in)
      if (!in.empty() && !made_by.count(in) && !init(in) && in != m.inputs[0]) bad(n, "input " + in + " is produced by nothing");
}

// the Detect tail: the Reshape nodes (the backbone, the neck and the towers have none) and everything behind them
void Lowerer::find_tail() {
  tail.assign(m.nodes.size(), 0);
  std::vector<int> todo;
  for (int i = 0; i < (int)m.nodes.size(); ++i)
    if (m.nodes[i].op == "Reshape") { tail[i] = 1; todo.push_back(i); }
  while (!todo.empty()) {
    const int i = todo.back();
    todo.pop_back();
    for (auto& o : m.nodes[i].out) {
      auto it = cons.find(o);
      if (it == cons.end()) continue;
      for (int c : it->second)
        if (!tail[c]) { tail[c] = 1; todo.push_back(c); }
    }
  }
}

// x -> Sigmoid -> Mul(x, .) with nothing else reading the Sigmoid: one Swish at the Mul
void Lowerer::find_swish() {
  absorbed.assign(m.nodes.size(), 0);
  for (int i = 0; i < (int)m.nodes.size(); ++i) {
    const ONode& n = m.nodes[i];
    if (n.op != "Sigmoid" || tail[i] || n.in.size() != 1 || n.out.size() != 1) continue;
    auto it = cons.find(n.out[0]);
    if (it == cons.end() || it->second.size() != 1) continue;
    const int c = it->second[0];
    const ONode& mul = m.nodes[c];
    if (mul.op != "Mul" || tail[c] || mul.in.size() != 2) continue;
    if ((mul.in[0] == n.in[0] && mul.in[1] == n.out[0]) || (mul.in[1] == n.in[0] && mul.in[0] == n.out[0])) {
      absorbed[i] = 1;
      swish_in[c] = n.in[0];
    }
  }
}

NcnnLayer& Lowerer::emit(const ONode& n, int idx, const char* type, std::vector<std::string> ins, std::vector<std::string> outs) {
  ops.emplace_back();
  Op& op = ops.back();
  op.group = tail[idx] ? 2 : 0;
  op.l.type = type;
  op.l.name = n.label();
  op.l.inputs = std::move(ins);
  op.l.outputs = std::move(outs);
  for (auto& o : op.l.outputs)
    if (o.empty()) bad(n, "an output has no name");
  return op.l;
}

void Lowerer::lower_conv(const ONode& n, int idx) {
  if (n.in.size() < 2 || n.in.size() > 3 || n.out.size() != 1) bad(n, "Conv takes X, W and an optional B");
  const OTensor* w = init(n.in[1]);
  if (!w) bad(n, "the weight is not an initializer");
  if (w->dtype != DT_FLOAT) bad(n, fmt("the weight has element type %d: only fp32 weights are supported (no fp16 or quantised initializers)", w->dtype));
  if (w->dims.size() != 4 || w->f.empty()) bad(n, "the weight is not a 4-D tensor");
  const int64_t O = w->dims[0], Ig = w->dims[1], kh = w->dims[2], kw = w->dims[3];
  if (O > 65536 || Ig > 65536 || kh > 64 || kw > 64) bad(n, "the weight is too large");
  const std::vector<int64_t> ks = ints_attr(n, "kernel_shape", {kh, kw}), st = ints_attr(n, "strides", {1, 1}),
                             pd = ints_attr(n, "pads", {0, 0, 0, 0}), dl = ints_attr(n, "dilations", {1, 1});
  if (ks.size() != 2 || ks[0] != kh || ks[1] != kw) bad(n, "kernel_shape does not match the weight");
  if (st.size() != 2 || pd.size() != 4 || dl.size() != 2) bad(n, "only 2-D convolutions are supported");
  check_small(n, st, "strides");
  check_small(n, pd, "pads");
  if (dl[0] != 1 || dl[1] != 1) bad(n, fmt("dilation %lldx%lld: only dilation 1 is supported", (long long)dl[0], (long long)dl[1]));
  if (pd[0] != pd[2] || pd[1] != pd[3])
    bad(n, fmt("asymmetric pads [%lld, %lld, %lld, %lld] are not supported", (long long)pd[0], (long long)pd[1], (long long)pd[2], (long long)pd[3]));
  if (const OAttr* ap = n.attr("auto_pad"))
    if (ap->has_s && ap->s != "NOTSET") bad(n, "auto_pad " + ap->s + " is not supported: export with explicit pads");
  const int64_t group = int_attr(n, "group", 1);
  if (group != 1 && !(group == O && Ig == 1)) bad(n, fmt("group %lld: only group 1 and depthwise convolutions are supported", (long long)group));
  NcnnLayer& l = emit(n, idx, group == 1 ? "Convolution" : "ConvolutionDepthWise", {data_in(n, 0)}, {n.out[0]});
  l.weight = w->f;
  l.in_ch = (int)Ig;
  if (n.in.size() == 3 && !n.in[2].empty()) {
    const OTensor* b = init(n.in[2]);
    if (!b) bad(n, "the bias is not an initializer");
    if (b->dtype != DT_FLOAT) bad(n, fmt("the bias has element type %d: only fp32 is supported", b->dtype));
    if ((int64_t)b->f.size() != O) bad(n, "the bias does not have one value per output channel");
    l.bias = b->f;
  }
  // the parameter set pnnx writes: 0 num_output, 1 / 11 kernel w / h, 2 / 12 dilation, 3 / 13 stride, 4 / 14 pad, 5 bias_term, 6 weight count
  l.params = {{0, (double)O}, {1, (double)kw}, {11, (double)kh}, {2, 1.0}, {12, 1.0}, {3, (double)st[1]}, {13, (double)st[0]},
              {4, (double)pd[1]}, {14, (double)pd[0]}, {5, l.bias.empty() ? 0.0 : 1.0}, {6, (double)w->f.size()}};
  if (group != 1) l.params[7] = (double)group;
}

// a float constant a tail node reads as a tensor: the anchor table (1, 2, A), the stride table (1, A)
std::string Lowerer::memory_data(const ONode& n, const OTensor& t) {
  if (t.dtype != DT_FLOAT) bad(n, fmt("constant %s has element type %d: only fp32 is supported", t.name.c_str(), t.dtype));
  std::vector<int64_t> d = t.dims;
  if (!d.empty() && d[0] == 1) d.erase(d.begin());   // the batch dimension
  if (d.empty() || d.size() > 3) bad(n, fmt("constant %s has %zu dimensions", t.name.c_str(), t.dims.size()));
  ops.emplace_back();
  Op& op = ops.back();
  op.group = 2;
  op.l.type = "MemoryData";
  op.l.name = t.name;
  const int copy = n_memdata[t.name]++;   // (one layer per reader, as pnnx writes them)
  const std::string blob = copy ? t.name + "_" + std::to_string(copy) : t.name;
  op.l.outputs = {blob};
  op.l.data = t.f;
  static const int key[3] = {0, 1, 2};   // w, h, c
  for (size_t k = 0; k < d.size(); ++k) op.l.params[key[k]] = (double)d[d.size() - 1 - k];
  return blob;
}

// tail arithmetic (Sub / Add / Div / Mul) and the residual Add of a bottleneck
void Lowerer::lower_binary(const ONode& n, int idx) {
  if (n.in.size() != 2 || n.out.size() != 1) bad(n, "two inputs and one output expected");
  static const std::map<std::string, int> code = {{"Add", 0}, {"Sub", 1}, {"Mul", 2}, {"Div", 3}};
  int opc = code.at(n.op);
  const OTensor* c0 = init(n.in[0]);
  const OTensor* c1 = init(n.in[1]);
  if (c0 && c1) bad(n, "both inputs are constants");
  if (!tail[idx]) {
    if (n.op != "Add" || c0 || c1) bad(n, "outside the Detect tail only the sum of two tensors is supported");
    emit(n, idx, "BinaryOp", {n.in[0], n.in[1]}, {n.out[0]}).params = {{0, 0.0}};
    return;
  }
  const OTensor* c = c0 ? c0 : c1;
  if (c && c->dtype == DT_FLOAT && c->f.size() == 1) {   // x op scalar; scalar - x and scalar / x are NCNN's reversed forms
    if (c0 && opc == 1) opc = 7;
    if (c0 && opc == 3) opc = 8;
    emit(n, idx, "BinaryOp", {c0 ? n.in[1] : n.in[0]}, {n.out[0]}).params = {{0, (double)opc}, {1, 1.0}, {2, (double)c->f[0]}};
    return;
  }
  std::vector<std::string> ins = {n.in[0], n.in[1]};
  if (c) ins[c0 ? 0 : 1] = memory_data(n, *c);
  emit(n, idx, "BinaryOp", ins, {n.out[0]}).params = {{0, (double)opc}};
}

void Lowerer::lower_node(int idx) {
  const ONode& n = m.nodes[idx];
  const bool in_tail = tail[idx] != 0;
  auto one_out = [&] { if (n.out.size() != 1) bad(n, "one output expected"); };
  auto tail_only = [&] { if (!in_tail) bad(n, "is supported in the Detect tail only (behind the head's Reshape)"); };
  if (n.op == "Conv") {
    lower_conv(n, idx);
  } else if (n.op == "Sigmoid") {
    one_out();
    emit(n, idx, "Sigmoid", {data_in(n, 0)}, {n.out[0]});
  } else if (n.op == "Mul" && swish_in.count(idx)) {
    one_out();
    emit(n, idx, "Swish", {swish_in[idx]}, {n.out[0]});
  } else if (n.op == "Add" || n.op == "Sub" || n.op == "Mul" || n.op == "Div") {
    lower_binary(n, idx);
  } else if (n.op == "Split") {
    std::vector<int64_t> sizes = ints_attr(n, "split", {});
    if (sizes.empty() && n.in.size() > 1 && !n.in[1].empty()) sizes = ints_input(n, 1, "the split input");
    if (sizes.empty()) sizes.assign(n.out.size(), -233);   // equal parts
    if (sizes.size() != n.out.size() || n.out.empty()) bad(n, "the split sizes do not match the outputs");
    check_small(n, sizes, "split");
    const int64_t axis = int_attr(n, "axis", 0);
    if (axis == 0) bad(n, "a split along the batch axis is batch-dependent control flow: unsupported");
    NcnnLayer& l = emit(n, idx, "Slice", {data_in(n, 0)}, n.out);
    l.arrays[0] = std::vector<double>(sizes.begin(), sizes.end());
    l.params = {{1, (double)axis_of(axis)}};
  } else if (n.op == "Concat") {
    one_out();
    if (n.in.empty()) bad(n, "no inputs");
    const OAttr* a = n.attr("axis");
    if (!a || !a->has_i) bad(n, "axis is missing");
    if (a->i == 0) bad(n, "a concat along the batch axis is unsupported");
    std::vector<std::string> ins;
    for (size_t k = 0; k < n.in.size(); ++k) ins.push_back(data_in(n, k));
    emit(n, idx, "Concat", ins, {n.out[0]}).params = {{0, (double)axis_of(a->i)}};
  } else if (n.op == "MaxPool") {
    if (n.out.empty() || (n.out.size() > 1 && !n.out[1].empty())) bad(n, "the Indices output is not supported");
    const std::vector<int64_t> ks = ints_attr(n, "kernel_shape", {}), st = ints_attr(n, "strides", {1, 1}), pd = ints_attr(n, "pads", {0, 0, 0, 0}),
                               dl = ints_attr(n, "dilations", {1, 1});
    if (ks.size() != 2 || st.size() != 2 || pd.size() != 4 || dl.size() != 2) bad(n, "only 2-D pooling is supported");
    check_small(n, ks, "kernel_shape");
    check_small(n, st, "strides");
    check_small(n, pd, "pads");
    if (dl[0] != 1 || dl[1] != 1) bad(n, "dilated pooling is not supported");
    if (pd[0] != pd[2] || pd[1] != pd[3]) bad(n, "asymmetric pads are not supported");
    if (const OAttr* ap = n.attr("auto_pad"))
      if (ap->has_s && ap->s != "NOTSET") bad(n, "auto_pad " + ap->s + " is not supported");
    const int64_t ceil_mode = int_attr(n, "ceil_mode", 0);
    // pnnx's set: 0 = max, 1 / 11 kernel, 2 / 12 stride, 3 / 13 pad, 5 pad_mode (1 = floor, the mode the SPPF pools have)
    emit(n, idx, "Pooling", {data_in(n, 0)}, {n.out[0]}).params = {{0, 0.0}, {1, (double)ks[1]}, {11, (double)ks[0]}, {2, (double)st[1]},
                                                                 {12, (double)st[0]}, {3, (double)pd[1]}, {13, (double)pd[0]},
                                                                 {5, ceil_mode ? 0.0 : 1.0}};
  } else if (n.op == "Resize") {
    one_out();
    const OAttr* mode = n.attr("mode");
    if (mode && mode->has_s && mode->s != "nearest") bad(n, "mode " + mode->s + ": only nearest is supported");
    const OAttr* ctm = n.attr("coordinate_transformation_mode");
    const OAttr* nm = n.attr("nearest_mode");
    if (!ctm || ctm->s != "asymmetric" || !nm || nm->s != "floor")
      bad(n, "only coordinate_transformation_mode asymmetric with nearest_mode floor is supported (out[y][x] = in[y / s][x / s])");
    if (n.in.size() > 3 && !n.in[3].empty()) bad(n, "Resize to sizes needs the tensor's shape: export with a scale factor");
    const OTensor* sc = n.in.size() > 2 && !n.in[2].empty() ? init(n.in[2]) : nullptr;
    if (!sc || sc->dtype != DT_FLOAT) bad(n, "scales is not a constant fp32 tensor: dynamic shapes are not supported");
    if (sc->f.size() != 4 || sc->f[0] != 1.f || sc->f[1] != 1.f || !(sc->f[2] >= 1.f && sc->f[2] <= 64.f) || !(sc->f[3] >= 1.f && sc->f[3] <= 64.f) ||
        sc->f[2] != (float)(int)sc->f[2] || sc->f[3] != (float)(int)sc->f[3])
      bad(n, "scales must be [1, 1, sy, sx] with integral sy, sx");
    emit(n, idx, "Interp", {data_in(n, 0)}, {n.out[0]}).params = {{0, 1.0}, {1, (double)sc->f[2]}, {2, (double)sc->f[3]}, {6, 0.0}};
  } else if (n.op == "Reshape") {
    one_out();
    const std::vector<int64_t> shape = ints_input(n, 1, "the shape input");
    if (shape.size() < 2 || shape.size() > 4) bad(n, fmt("a shape of %zu dimensions", shape.size()));
    if (shape[0] != 1) bad(n, "the target shape's batch dimension is not 1: batch-dependent reshapes are not supported");
    check_small(n, shape, "shape");
    NcnnLayer& l = emit(n, idx, "Reshape", {data_in(n, 0)}, {n.out[0]});
    for (size_t k = 1; k < shape.size(); ++k) l.params[(int)(shape.size() - 1 - k)] = (double)shape[k];   // 0 = w, 1 = h, 2 = c
  } else if (n.op == "Transpose") {
    tail_only();
    one_out();
    const std::vector<int64_t> perm = ints_attr(n, "perm", {});
    if ((perm.size() != 3 && perm.size() != 4) || perm[0] != 0) bad(n, "only a permutation of 3 or 4 dimensions that keeps the batch axis is supported");
    std::vector<int> p;
    std::set<int> seen;
    for (size_t k = 1; k < perm.size(); ++k) {
      if (perm[k] < 1 || perm[k] >= (int64_t)perm.size() || !seen.insert((int)perm[k]).second) bad(n, "perm is not a permutation");
      p.push_back((int)perm[k] - 1);
    }
    // NCNN Permute order_type of the dimensions behind the batch
    int order = 0;
    if (p.size() == 2) order = p[0] == 0 ? 0 : 1;
    else {
      static const int table[6][4] = {{0, 1, 2, 0}, {0, 2, 1, 1}, {1, 0, 2, 2}, {1, 2, 0, 3}, {2, 0, 1, 4}, {2, 1, 0, 5}};
      for (auto& row : table)
        if (row[0] == p[0] && row[1] == p[1] && row[2] == p[2]) order = row[3];
    }
    emit(n, idx, "Permute", {data_in(n, 0)}, {n.out[0]}).params = {{0, (double)order}};
  } else if (n.op == "Softmax") {
    tail_only();
    one_out();
    const int64_t axis = int_attr(n, "axis", m.opset >= 13 ? -1 : 1);   // the default changed with opset 13
    if (axis == 0 || axis < -8 || axis > 8) bad(n, "a softmax along the batch axis is unsupported");
    emit(n, idx, "Softmax", {data_in(n, 0)}, {n.out[0]}).params = {{0, (double)axis_of(axis)}, {1, 1.0}};
  } else if (n.op == "Slice") {
    tail_only();
    one_out();
    if (n.in.size() < 3) bad(n, "starts and ends as inputs expected (opset 10 and later)");
    const std::vector<int64_t> starts = ints_input(n, 1, "starts"), ends = ints_input(n, 2, "ends");
    std::vector<int64_t> axes, steps;
    if (n.in.size() > 3 && !n.in[3].empty()) axes = ints_input(n, 3, "axes");
    if (n.in.size() > 4 && !n.in[4].empty()) steps = ints_input(n, 4, "steps");
    if (axes.empty())
      for (size_t k = 0; k < starts.size(); ++k) axes.push_back((int64_t)k);
    if (starts.empty() || starts.size() != ends.size() || axes.size() != starts.size()) bad(n, "starts, ends and axes differ in length");
    for (int64_t s : steps)
      if (s != 1) bad(n, "only step 1 is supported");
    // NCNN's Slice cuts a blob into consecutive parts; one [start, end) window is its Crop (-23309 starts, -23310 ends, -23311 axes)
    NcnnLayer& l = emit(n, idx, "Crop", {data_in(n, 0)}, {n.out[0]});
    for (size_t k = 0; k < axes.size(); ++k) {
      if (axes[k] == 0) bad(n, "a slice along the batch axis is unsupported");
      const double big = 2147483647.0;   // INT64_MAX as "to the end" is NCNN's -233
      l.arrays[9].push_back((double)std::max<int64_t>(std::min<int64_t>(starts[k], 1 << 30), -(1 << 30)));
      l.arrays[10].push_back(ends[k] >= (int64_t)big ? -233.0 : (double)std::max<int64_t>(ends[k], -(1 << 30)));
      l.arrays[11].push_back((double)axis_of(std::max<int64_t>(std::min<int64_t>(axes[k], 8), -8)));
    }
  } else if (n.op == "MatMul") {
    bad(n, "attention blocks (YOLO11's C2PSA) are not supported from ONNX: convert this model to NCNN");
  } else if (n.op == "Shape" || n.op == "Gather" || n.op == "Unsqueeze" || n.op == "Squeeze" || n.op == "Cast" || n.op == "Range" ||
             n.op == "ConstantOfShape" || n.op == "Expand") {
    bad(n, "shape arithmetic inside the graph (dynamic axes): export with a static input shape");
  } else if (n.op == "If" || n.op == "Loop" || n.op == "NonMaxSuppression" || n.op == "TopK") {
    bad(n, "control flow and NMS inside the graph are not supported: export the raw Detect output");
  } else {
    bad(n, "unsupported operator");
  }
}

NcnnGraph Lowerer::finish() {
  // ---- the Input layer, then every node in file order
  {
    ops.emplace_back();
    ops.back().l.type = "Input";
    ops.back().l.name = m.inputs[0];
    ops.back().l.outputs = {m.inputs[0]};
  }
  for (int i = 0; i < (int)m.nodes.size(); ++i)
    if (!absorbed[i]) lower_node(i);

  // ---- layer order.  The planner emits launches in file order and takes everything from the first head Reshape on as the
  // Detect tail, but an ONNX file is only topologically sorted (the reference's export interleaves the towers of one level
  // with the next level's neck).  So: depth-first from the output, inputs in order -- the order the modules ran in when
  // the model was traced -- then the towers behind the neck and the tail behind the towers, as pnnx writes them.
  const int N = (int)ops.size();
  std::map<std::string, int> prod;
  for (int k = 0; k < N; ++k)
    for (auto& o : ops[k].l.outputs) {
      LP_CHECK(!prod.count(o), LP_ERR_GRAPH, "%s: tensor %s is defined twice", src.c_str(), o.c_str());
      prod[o] = k;
    }
  auto producer_of = [&](const std::string& t, const NcnnLayer& who) {
    auto it = prod.find(t);
    LP_CHECK(it != prod.end(), LP_ERR_GRAPH, "%s: layer %s reads %s, which no supported node produces", src.c_str(), who.name.c_str(), t.c_str());
    return it->second;
  };
  std::vector<int> order;
  {
    std::vector<char> state(N, 0);
    std::vector<std::pair<int, size_t>> stack;
    auto out_it = prod.find(m.outputs[0]);
    LP_CHECK(out_it != prod.end(), LP_ERR_GRAPH, "%s: graph output %s is produced by nothing", src.c_str(), m.outputs[0].c_str());
    stack.push_back({out_it->second, 0});
    state[out_it->second] = 1;
    while (!stack.empty()) {
      const int k = stack.back().first;
      if (stack.back().second < ops[k].l.inputs.size()) {
        const int p = producer_of(ops[k].l.inputs[stack.back().second++], ops[k].l);
        LP_CHECK(state[p] != 1, LP_ERR_GRAPH, "%s: the graph has a cycle through %s", src.c_str(), ops[p].l.name.c_str());
        if (state[p] == 0) { state[p] = 1; stack.push_back({p, 0}); }
      } else {
        state[k] = 2;
        order.push_back(k);
        stack.pop_back();
      }
    }
  }
  std::map<std::string, int> uses;
  for (int k : order)
    for (auto& in : ops[k].l.inputs) ++uses[in];
  // the towers: from each input of a head Concat back through layers with one input whose output nothing else reads
  for (int k : order) {
    if (ops[k].group != 2 || ops[k].l.type != "Reshape") continue;
    const int cat = producer_of(ops[k].l.inputs[0], ops[k].l);
    if (ops[cat].group != 0 || ops[cat].l.type != "Concat") continue;
    ops[cat].group = 1;
    for (auto& t : ops[cat].l.inputs) {
      int p = producer_of(t, ops[cat].l);
      while (ops[p].group == 0 && ops[p].l.inputs.size() == 1 && ops[p].l.outputs.size() == 1 && uses[ops[p].l.outputs[0]] == 1) {
        ops[p].group = 1;
        p = producer_of(ops[p].l.inputs[0], ops[p].l);
      }
    }
  }
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return ops[a].group < ops[b].group; });

  // ---- a tensor with several consumers goes through a Split (the planner resolves those as aliases)
  NcnnGraph g;
  std::map<std::string, std::vector<std::string>> copies;   // tensor -> the Split outputs not handed out yet, last first
  int n_split = 0;
  for (int k : order) {
    NcnnLayer l = std::move(ops[k].l);
    for (auto& in : l.inputs) {
      auto it = copies.find(in);
      if (it != copies.end()) {
        LP_CHECK(!it->second.empty(), LP_ERR_GRAPH, "%s: internal error: consumers of %s miscounted", src.c_str(), in.c_str());
        const std::string c = it->second.back();
        it->second.pop_back();
        in = c;
      }
    }
    const std::vector<std::string> outs = l.outputs;
    g.layers.push_back(std::move(l));
    for (auto& o : outs) {
      const int u = uses.count(o) ? uses[o] : 0;
      if (u < 2) continue;
      NcnnLayer s;
      s.type = "Split";
      s.name = "splitncnn_" + std::to_string(n_split++);
      s.inputs = {o};
      for (int q = 0; q < u; ++q) s.outputs.push_back(o + "_splitncnn_" + std::to_string(q));
      copies[o] = std::vector<std::string>(s.outputs.rbegin(), s.outputs.rend());
      g.layers.push_back(std::move(s));
    }
  }
  return g;
}

}  // namespace

NcnnGraph onnx_to_graph(const void* data, size_t bytes, const std::string& name) {
  LP_CHECK(data && bytes > 0, LP_ERR_GRAPH, "%s: empty ONNX model", name.c_str());
  OModel m = parse_model(static_cast<const uint8_t*>(data), bytes, name);
  // Split sizes, Resize scales and Slice bounds moved from attributes to inputs between opsets 10 and 13; both forms are read.
  // Below 11 Resize has another input list.
  LP_CHECK(m.opset >= 11 && m.opset <= 64, LP_ERR_GRAPH, "%s: ONNX opset %lld is not supported (11 and later)", name.c_str(), (long long)m.opset);
  Lowerer lw(name, std::move(m));
  lw.fold_constants();
  lw.index();
  lw.find_tail();
  lw.find_swish();
  return lw.finish();
}

NcnnGraph onnx_file_to_graph(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  LP_CHECK(f.good(), LP_ERR_IO, "Failed to load ONNX model: %s", path.c_str());
  std::vector<char> buf((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
  LP_CHECK(!f.bad(), LP_ERR_IO, "read error on %s", path.c_str());
  return onnx_to_graph(buf.data(), buf.size(), path);
}

}  // namespace lp
