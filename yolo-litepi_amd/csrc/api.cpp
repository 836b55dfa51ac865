// C-ABI of liblitepi_hip.so (see include/litepi.h for the reference call sites each entry
// point replaces).  The handle (handle.h) owns the device, the stream, all activation/result buffers and the two
// model plans; every pipeline stage runs on the GPU -- there is no CPU fallback anywhere.
// This file: errors and small host helpers, the handle's lifecycle, and the RCCL binding.  The pipeline entry points are in
// pipeline.cpp, pixfmt.cpp, views.cpp, tracking.cpp, inventory.cpp, topk.cpp and quality.cpp, the test hooks in test_hooks.cpp.
#include <cstdlib>
#include <dlfcn.h>
#include <mutex>
#include <set>

#include "handle.h"
#include "mbnet.h"
#include "onnx_graph.h"
#include "resnet.h"

namespace lp {

static thread_local std::string g_last_error;
void set_last_error(const std::string& s) { g_last_error = s; }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-device attribute: set it once per (device, kernel) and
// check the result (a kernel that needs more than 64 KB of LDS fails to launch without it)
void set_max_dynamic_lds(const void* fn, int bytes) {
  static std::mutex mu;
  static std::set<std::pair<int, const void*>> done;
  int dev = 0;
  LP_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu);
  if (done.count({dev, fn})) return;
  LP_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
  done.insert({dev, fn});
}

}  // namespace lp

using namespace lp;

// RCCL, bound at run time (lp_comm_* / lp_gather): the library links nothing but the HIP runtime
struct NcclId { char internal[128]; };
struct Rccl {
  void* lib = nullptr;
  int (*GetUniqueId)(NcclId*) = nullptr;
  int (*CommInitRank)(void**, int, NcclId, int) = nullptr;
  int (*Gather)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*CommDestroy)(void*) = nullptr;
  const char* (*GetErrorString)(int) = nullptr;
};
Rccl& rccl() {
  static Rccl r;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (r.lib) break;
    }
    if (!r.lib) return;
    r.GetUniqueId = reinterpret_cast<int (*)(NcclId*)>(dlsym(r.lib, "ncclGetUniqueId"));
    r.CommInitRank = reinterpret_cast<int (*)(void**, int, NcclId, int)>(dlsym(r.lib, "ncclCommInitRank"));
    r.Gather = reinterpret_cast<int (*)(const void*, void*, size_t, int, int, void*, hipStream_t)>(dlsym(r.lib, "ncclGather"));
    r.CommDestroy = reinterpret_cast<int (*)(void*)>(dlsym(r.lib, "ncclCommDestroy"));
    r.GetErrorString = reinterpret_cast<const char* (*)(int)>(dlsym(r.lib, "ncclGetErrorString"));
  });
  LP_CHECK(r.lib && r.GetUniqueId && r.CommInitRank && r.Gather && r.CommDestroy, LP_ERR_STATE,
           "RCCL is not available (dlopen librccl.so.1: %s)", r.lib ? "a symbol is missing" : dlerror());
  return r;
}
#define LP_RCCL(expr)                                                                                                           \
  do {                                                                                                                          \
    const int rc_ = (expr);                                                                                                     \
    if (rc_ != 0) throw Error(LP_ERR_HIP, fmt("%s: RCCL error %d (%s)", #expr, rc_, rccl().GetErrorString ? rccl().GetErrorString(rc_) : "?")); \
  } while (0)

extern "C" {

const char* lp_last_error(void) { return lp::g_last_error.c_str(); }
int lp_version(void) { return LP_ABI_VERSION; }

void lp_default_config(lp_config* c) {
  memset(c, 0, sizeof(*c));
  c->device = 0; c->precision = LP_FP16; c->max_batch = 1; c->max_det = 300; c->num_classes = 58;
  c->det_input = 640; c->cls_input = 64; c->max_rois = 0; c->conv_impl = 0;
}

int lp_create(const lp_config* cfg, lp_handle** out) {
  LP_API_BEGIN
  LP_CHECK(cfg && out, LP_ERR_ARG, "null argument");
  LP_CHECK(cfg->max_batch >= 1 && cfg->max_batch <= 1024 && cfg->max_det >= 1 && cfg->det_input % 32 == 0 && cfg->det_input >= 64,
           LP_ERR_ARG, "bad config (max_batch %d, max_det %d, det_input %d)", cfg->max_batch, cfg->max_det, cfg->det_input);
  LP_CHECK(cfg->det_input_h == 0 || (cfg->det_input_h % 32 == 0 && cfg->det_input_h >= 64), LP_ERR_ARG,
           "bad config (det_input_h %d: 0 for a square input, else a multiple of 32 and at least 64)", cfg->det_input_h);
  LP_CHECK((cfg->numerics == 0 || cfg->numerics == 1) && cfg->cls_arch >= 0 && cfg->cls_arch <= LP_CLS_EFFICIENTNET_B0, LP_ERR_ARG,
           "bad config (numerics %d, cls_arch %d)", cfg->numerics, cfg->cls_arch);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= cfg->device)
    throw Error(LP_ERR_NODEVICE, fmt("HIP device %d not available (%d visible): liblitepi_hip has no CPU path", cfg->device, ndev));
  LP_HIP(hipSetDevice(cfg->device));
  hipDeviceProp_t prop;
  LP_HIP(hipGetDeviceProperties(&prop, cfg->device));
  if (std::string(prop.gcnArchName).find("gfx950") == std::string::npos)
    throw Error(LP_ERR_NODEVICE, fmt("device %d is %s; this library is built for gfx950 only", cfg->device, prop.gcnArchName));
  std::unique_ptr<lp_handle> h(new lp_handle());
  h->cfg = *cfg;
  // the run path's switches, as this handle's environment has them (RunOptions).  The two measurement diagnostics make every
  // pass after a handle's first return STALE results with LP_OK: never silently
  {
    static bool warned = false;
    const char *ss = getenv("LITEPI_SKIP_STAGE"), *so = getenv("LITEPI_SKIP_OP");
    if ((ss || so) && !warned) {
      warned = true;
      fprintf(stderr, "[litepi] WARNING: LITEPI_SKIP_STAGE=%s LITEPI_SKIP_OP=%s -- diagnostic mode (tools/marginal_cost.sh): a pipeline stage / "
                      "detector launch is LEFT OUT of every pass after a handle's first; results are stale and must not be used\n",
              ss ? ss : "", so ? so : "");
    }
    const char *ut = getenv("LITEPI_UPLOAD_THREADS"), *ug = getenv("LITEPI_UPLOAD_GROUP_MB");
    h->opt.no_graph = getenv("LITEPI_NO_GRAPH") != nullptr;
    if (ss) h->opt.skip_stage = ss;
    if (ut) h->opt.upload_threads = atoi(ut);
    if (ug) h->opt.upload_group_mb = (size_t)atol(ug);
  }
  // every kept box is a ROI (the reference classifies all of them, e2e.py:493-497): the default capacity can not overflow
  h->max_rois = cfg->max_rois > 0 ? cfg->max_rois : cfg->max_batch * cfg->max_det;
  // the classifier's widest per-ROI tensor must stay below 2^31 elements (32-bit element offsets in the conv kernels): say so
  // here, not at the first launch.  ShuffleNetV2 / ResNet18 at cls_input S: conv1 output 24 (64) channels at (S/2)^2.
  {
    const double per_roi = cfg->cls_arch >= LP_CLS_MOBILENETV2 ? MBNetClassifier::widest_per_roi(cfg->cls_input)
                                                               : (double)(cfg->cls_arch == LP_CLS_RESNET18 ? 64 : 24) * (cfg->cls_input / 2.0) * (cfg->cls_input / 2.0);
    LP_CHECK(per_roi * h->max_rois < 2147483648.0, LP_ERR_ARG,
             "max_rois = %d (max_batch %d x max_det %d when left 0) makes the classifier's activations exceed 2^31 elements; lower "
             "max_det or set max_rois (at most %d for this classifier)", h->max_rois, cfg->max_batch, cfg->max_det, (int)(2147483647.0 / per_roi));
  }
  LP_HIP(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  for (auto& e : h->ev) LP_HIP(hipEventCreate(&e));
  h->d_geom.alloc((size_t)std::max(cfg->max_batch, h->max_rois) * sizeof(ImgGeom));
  h->d_lb.alloc((size_t)cfg->max_batch * h->det_h() * h->det_w() * 3, false);
  h->d_roi_base.alloc((size_t)(cfg->max_batch + 1) * 4);
  h->d_roi_total.alloc(32);  // total, unclamped total | accumulator, ticket (kernels.h RoiTable)
  h->d_roi_img.alloc((size_t)h->max_rois * 4);
  h->d_roi_slot.alloc((size_t)h->max_rois * 4);
  const int cs = cfg->cls_input;
  h->d_roi_rgb.alloc((size_t)h->max_rois * cs * cs * 3, false);
  h->d_probs.alloc((size_t)h->max_rois * std::max(cfg->num_classes, 1) * 4);
  h->d_ids.alloc((size_t)h->max_rois * 4);
  h->d_conf.alloc((size_t)h->max_rois * 4);
  *out = h.release();
  LP_API_END
}

void lp_destroy(lp_handle* h) {
  if (!h) return;
  (void)hipSetDevice(h->cfg.device);
  (void)hipDeviceSynchronize();
  h->drop_graphs();
  h->trk.reset();
  h->evl.reset();
  for (auto& e : h->ev)
    if (e) (void)hipEventDestroy(e);
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  h->pool.reset();
  if (h->h_stage) (void)hipHostFree(h->h_stage);
  if (h->comm) { try { (void)rccl().CommDestroy(h->comm); } catch (...) {} }
  delete h;
}

// Every detector loader ends here: the plan is built on a fresh Detector, so a graph the planner refuses leaves the handle's
// model (and its captured graphs) as they were.
static void install_detector(lp_handle* h, NcnnGraph&& g, const std::string& name) {
  LP_HIP(hipSetDevice(h->cfg.device));
  std::unique_ptr<Detector> d(new Detector(h->cfg.precision, h->cfg.conv_impl, h->cfg.max_batch, h->det_h(), h->det_w()));
  d->load_graph(std::move(g), name);
  h->drop_graphs();
  h->det = std::move(d);
  h->alloc_post_buffers();
  LP_HIP(hipDeviceSynchronize());
}

int lp_load_detector_ncnn(lp_handle* h, const char* param_path, const char* bin_path) {
  LP_API_BEGIN
  LP_CHECK(h && param_path && bin_path, LP_ERR_ARG, "null argument");
  NcnnGraph g;
  g.load(param_path, bin_path);
  install_detector(h, std::move(g), param_path);
  LP_API_END
}

int lp_load_detector_onnx(lp_handle* h, const char* onnx_path) {
  LP_API_BEGIN
  LP_CHECK(h && onnx_path, LP_ERR_ARG, "null argument");
  install_detector(h, onnx_file_to_graph(onnx_path), onnx_path);
  LP_API_END
}

int lp_load_detector_onnx_memory(lp_handle* h, const void* data, size_t bytes, const char* name) {
  LP_API_BEGIN
  LP_CHECK(h && data && bytes > 0, LP_ERR_ARG, "null argument");
  const std::string src = name && *name ? name : "<memory>";
  install_detector(h, onnx_to_graph(data, bytes, src), src);
  LP_API_END
}

int lp_detector_graph_describe(const char* model_path, const char* bin_path, char* out, size_t cap, size_t* needed) {
  LP_API_BEGIN
  LP_CHECK(model_path && needed, LP_ERR_ARG, "null argument");
  NcnnGraph g;
  if (bin_path) g.load(model_path, bin_path);
  else g = onnx_file_to_graph(model_path);
  const std::string text = g.describe();
  *needed = text.size() + 1;
  if (out) {
    LP_CHECK(cap >= *needed, LP_ERR_ARG, "buffer of %zu bytes, %zu needed", cap, *needed);
    memcpy(out, text.c_str(), *needed);
  }
  LP_API_END
}

int lp_load_classifier_tensors(lp_handle* h, int n, const char* const* names, const float* const* data,
                               const int64_t* const* shapes, const int* ndims) {
  LP_API_BEGIN
  LP_CHECK(h && names && data && shapes && ndims && n > 0, LP_ERR_ARG, "null argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  std::map<std::string, NamedTensor> sd;
  for (int i = 0; i < n; ++i) {
    NamedTensor t;
    t.data = data[i];
    t.shape.assign(shapes[i], shapes[i] + ndims[i]);
    sd[names[i]] = t;
  }
  std::unique_ptr<ClassifierBase> c;
  if (h->cfg.cls_arch == LP_CLS_RESNET18) c.reset(new ResNet18Classifier(h->cfg.precision, h->cfg.conv_impl, h->max_rois, h->cfg.num_classes, h->cfg.cls_input));
  else if (h->cfg.cls_arch == LP_CLS_MOBILENETV2 || h->cfg.cls_arch == LP_CLS_EFFICIENTNET_B0)
    c.reset(new MBNetClassifier(h->cfg.cls_arch == LP_CLS_MOBILENETV2 ? MBNetClassifier::MOBILENET_V2 : MBNetClassifier::EFFICIENTNET_B0, h->cfg.precision,
                                h->cfg.conv_impl, h->max_rois, h->cfg.num_classes, h->cfg.cls_input));
  else c.reset(new Classifier(h->cfg.precision, h->cfg.conv_impl, h->max_rois, h->cfg.num_classes, h->cfg.cls_input));
  c->load(sd);
  h->drop_graphs();
  h->cls = std::move(c);
  LP_HIP(hipDeviceSynchronize());
  LP_API_END
}

int lp_set_stream(lp_handle* h, void* s) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  h->stream = s ? reinterpret_cast<hipStream_t>(s) : h->own_stream;
  LP_API_END
}

int lp_synchronize(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

int lp_profile_next(lp_handle* h, int enable) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  h->prof_next = enable != 0;
  LP_API_END
}

int lp_profile_read(lp_handle* h, lp_kernel_time* out, int cap, int* n) {
  LP_API_BEGIN
  LP_CHECK(h && n, LP_ERR_ARG, "null argument");
  if (!h->prof.recs.empty()) {
    LP_HIP(hipStreamSynchronize(h->stream));
    int R = 0;
    LP_HIP(hipMemcpy(&R, h->d_roi_total.p, 4, hipMemcpyDeviceToHost));
    h->prof.collect(R);
  }
  const int m = std::min<int>(cap, (int)h->prof.results.size());
  for (int i = 0; i < m && out; ++i) out[i] = h->prof.results[i];
  *n = (int)h->prof.results.size();
  LP_API_END
}

int lp_detector_info(lp_handle* h, int* num_anchors, int* nc, int* reg_max, double* macs) {
  LP_API_BEGIN
  LP_CHECK(h && h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  if (num_anchors) *num_anchors = h->det->num_anchors();
  if (nc) *nc = h->det->num_classes();
  if (reg_max) *reg_max = h->det->reg_max();
  if (macs) *macs = h->det->macs_per_image();
  LP_API_END
}


int lp_comm_unique_id(void* id_out) {
  LP_API_BEGIN
  LP_CHECK(id_out, LP_ERR_ARG, "null argument");
  NcclId id;
  LP_RCCL(rccl().GetUniqueId(&id));
  memcpy(id_out, &id, sizeof(id));
  LP_API_END
}

int lp_comm_init(lp_handle* h, const void* id, int rank, int world) {
  LP_API_BEGIN
  LP_CHECK(h && id && world >= 1 && rank >= 0 && rank < world, LP_ERR_ARG, "bad argument (rank %d of %d)", rank, world);
  LP_CHECK(!h->comm, LP_ERR_STATE, "the handle already has a communicator");
  LP_HIP(hipSetDevice(h->cfg.device));
  NcclId nid;
  memcpy(&nid, id, sizeof(nid));
  void* comm = nullptr;
  LP_RCCL(rccl().CommInitRank(&comm, world, nid, rank));
  h->comm = comm; h->comm_rank = rank; h->comm_world = world;
  LP_API_END
}

int lp_gather(lp_handle* h, const void* dev_send, size_t bytes, void* dev_recv, int root) {
  LP_API_BEGIN
  LP_CHECK(h && dev_send && bytes > 0, LP_ERR_ARG, "bad argument");
  LP_CHECK(h->comm, LP_ERR_STATE, "lp_comm_init has not been called on this handle");
  LP_CHECK(root >= 0 && root < h->comm_world && (h->comm_rank != root || dev_recv), LP_ERR_ARG, "bad root %d / receive buffer", root);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_RCCL(rccl().Gather(dev_send, dev_recv, bytes, 1 /* ncclUint8 */, root, h->comm, h->stream));
  LP_API_END
}

int lp_comm_destroy(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null argument");
  if (h->comm) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));
    LP_RCCL(rccl().CommDestroy(h->comm));
    h->comm = nullptr; h->comm_world = 1; h->comm_rank = 0;
  }
  LP_API_END
}

int lp_roi_overflow(lp_handle* h, int* classified, int* kept) {
  LP_API_BEGIN
  LP_CHECK(h && classified && kept, LP_ERR_ARG, "null argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  int R[2] = {0, 0};
  LP_HIP(hipMemcpy(R, h->d_roi_total.p, sizeof(R), hipMemcpyDeviceToHost));
  *classified = R[0];
  *kept = R[1];
  LP_API_END
}

}  // extern "C"
