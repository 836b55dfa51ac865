// Internal to the C-ABI translation units (api.cpp, pipeline.cpp, pixfmt.cpp, views.cpp, maps.cpp, tracking.cpp, inventory.cpp, focus.cpp,
// topk.cpp, quality.cpp, eval.cpp, test_hooks.cpp): the handle behind include/litepi.h's lp_handle, the captured-step cache, and the pipeline pieces the entry points share.
#pragma once
#include <algorithm>
#include <array>
#include <functional>
#include <map>
#include <vector>

#include "classifier.h"
#include "common.h"
#include "copy_pool.h"
#include "detector.h"
#include "kernels.h"
#include "ring_slots.h"

namespace lp {

// The call plan the tracker's, the inventory's and the focus plan's rings carry (one slot: up to max_batch TrackJobs, then the
// max_batch frame indices): one job per stream present in the call, in order of first appearance; its frames in batch order.
// Returns the number of jobs.
inline int plan_stream_jobs(int* slot, int max_batch, int B, const int* stream_ids) {
  TrackJob* jobs = reinterpret_cast<TrackJob*>(slot);
  int* frames = slot + (size_t)max_batch * (sizeof(TrackJob) / sizeof(int));
  std::map<int, int> job_of;
  std::vector<int> sid(B, 0), per_job;
  for (int b = 0; b < B; ++b) {
    const int s = stream_ids ? stream_ids[b] : 0;
    auto it = job_of.find(s);
    if (it == job_of.end()) {
      it = job_of.emplace(s, (int)per_job.size()).first;
      jobs[per_job.size()] = TrackJob{s, 0, 0, 0};
      per_job.push_back(0);
    }
    sid[b] = it->second;
    ++per_job[it->second];
  }
  const int n_jobs = (int)per_job.size();
  for (int j = 0, off = 0; j < n_jobs; ++j) { jobs[j].first = off; off += per_job[j]; }
  for (int b = 0; b < B; ++b) frames[jobs[sid[b]].first + jobs[sid[b]].nframes++] = b;
  return n_jobs;
}

// The one pinned -> device plan ring.  A call's plan (the tracker's, the inventory's and the focus plan's stream jobs and frame
// lists, a surfaces call's table records) is written into a slot of a pinned block and copied from there to the device on the
// handle's stream (a pageable source would synchronise it).  dev_slots = RING: every pinned slot has a device slot of its
// own, and the event is recorded behind the launch that read it (tracker, inventory, focus).  dev_slots = 1: every captured
// step reads ONE device table at a fixed address, rewritten in stream order in front of the step, and the event is recorded
// behind the copy (surfaces).  Which slot comes next and whether its event has to be waited for is RingSlots' policy
// (ring_slots.h): only a slot still marked busy waits, i.e. once the ring has wrapped.
struct PlanRing {
  static constexpr int RING = 8;
  struct Slot { int index; void* host; void* dev; };
  DevBuf dev;             // dev_slots slots of slot_bytes
  char* host = nullptr;   // pinned, RING slots of slot_bytes
  size_t slot_bytes = 0;
  int dev_slots = RING;
  hipEvent_t ev[RING] = {};
  RingSlots<RING> slots;
  void create(size_t bytes, int n_dev = RING) {
    slot_bytes = bytes; dev_slots = n_dev;
    dev.alloc((size_t)n_dev * bytes);
    LP_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), RING * bytes, hipHostMallocDefault));
    for (auto& e : ev) LP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  // the next slot, free to be written (independent of any stream: it waits on the host, and only where the policy says so)
  Slot acquire() {
    bool wait = false;
    const int k = slots.take(&wait);
    if (wait) LP_HIP(hipEventSynchronize(ev[k]));
    return Slot{k, host + (size_t)k * slot_bytes, dev.as<char>() + (size_t)(dev_slots == RING ? k : 0) * slot_bytes};
  }
  void upload(const Slot& s, size_t bytes, hipStream_t st) { LP_HIP(hipMemcpyAsync(s.dev, s.host, bytes, hipMemcpyHostToDevice, st)); }
  // behind whatever read the slot last on st: the slot is re-used only after this point of the stream
  void release(const Slot& s, hipStream_t st) {
    LP_HIP(hipEventRecord(ev[s.index], st));
    slots.mark(s.index);
  }
  ~PlanRing() {
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
    if (host) (void)hipHostFree(host);
  }
};

// Sign inventory of a tracker (lp_inventory_*; include/litepi.h): entries, frame counters, the gallery of best crops and the
// log of finished signs stay in HBM between calls.  Its call plans go through a plan ring of its own: the tracker's ring keeps
// its re-use timing.
// Evidence store of an inventory (lp_evidence_*; include/litepi.h): per entry the E x E BGR picture of its best sighting's
// surroundings and that picture's window; the same per logged sign; and the job list the deciding kernel leaves for the
// picture launch (kernels.h, EvJob).
struct Evidence {
  lp_evidence_config cfg;
  size_t pic_bytes = 0;
  DevBuf gallery, log_pics, win, log_win, jobs, n_jobs;
};

struct Inventory {
  std::unique_ptr<Evidence> evid;   // null until lp_evidence_create: no other path looks at it
  lp_inventory_config cfg;
  int min_hits = 0, crop_bytes = 0;
  int rank = LP_RANK_CONFIG;        // lp_inventory_set_rank: LP_RANK_SHARPNESS reads the handle's lp_quality records in step 4
  DevBuf entries, frame_no, head, log, log_crops, gallery, roi_of;
  DevBuf d_dets, d_counts, d_tracks;   // lp_inventory (host records): allocated on first use
  PlanRing ring;                       // a slot: the tracker's plan (plan_stream_jobs)
};

// Focus plan of a tracker (lp_focus_*; include/litepi.h): the per-stream sweep cursor and unserved counter stay in HBM between
// calls.  Its call plans (the tracker's jobs and frame lists, then every frame's height, width and letterbox ratio) go through
// a plan ring of its own.  blob / vgeom remember the placeholder layout whose device tables the plan kernel rewrites in place
// (focus.cpp: upload_focus_tables).
struct FocusPlan {
  lp_focus_config cfg;   // the zeros resolved
  DevBuf state, d_views, d_dead;
  PlanRing ring;
  std::vector<char> blob;
  std::vector<ImgGeom> vgeom;
};

// Sign tracker of a handle (lp_tracker_*, lp_track*; include/litepi.h): the track table, the stream heads and the vote accumulators
// stay in HBM between calls.  A call's per-stream frame lists go through its plan ring.
struct Tracker {
  std::unique_ptr<Inventory> inv;   // null until lp_inventory_create: no other path looks at it
  std::unique_ptr<FocusPlan> focus; // null until lp_focus_create: no other path looks at it
  lp_track_config cfg;
  int nc = 1, max_det = 0, max_batch = 0;
  DevBuf table, heads, acc, scratch;
  DevBuf d_dets, d_counts, d_tracks;   // lp_track (host records): allocated on first use
  DevBuf d_topk;                       // lp_track_topk (host records): allocated on first use
  PlanRing ring;                       // a slot: up to max_batch jobs, then the max_batch frame indices (plan_stream_jobs)
};

// Evaluator of a handle (lp_eval_*; include/litepi.h): the counters with the class counts behind them, the thresholds and the
// row log stay in HBM between calls.  A call's ground truth goes through a plan ring of its own (a slot: max_batch EvalFrame,
// then up to max_batch * max_gt lp_gt packed in frame order).
struct Evaluator {
  lp_eval_config cfg;
  int nc = 1, max_det = 0, max_batch = 0;
  size_t gts_off = 0;                  // of the packed boxes in a slot
  DevBuf state, thr, log;              // EvalState + nc int32; n_thr doubles; max_rows lp_eval_row
  DevBuf d_dets, d_counts, d_matches;  // lp_eval (host records): allocated on first use
  PlanRing ring;
};

// a call's stream ids against the tracker's streams (tracker, inventory and focus calls)
inline void check_stream_ids(const Tracker& t, int B, const int* stream_ids) {
  if (stream_ids)
    for (int b = 0; b < B; ++b)
      LP_CHECK(stream_ids[b] >= 0 && stream_ids[b] < t.cfg.n_streams, LP_ERR_ARG, "stream_ids[%d] = %d outside 0..%d", b, stream_ids[b],
               t.cfg.n_streams - 1);
}

// ---- captured steps: the launch sequence of a call is a pure function of (entry point, buffers, batch, geometry,
//      thresholds), so the second call with the same key is captured into a hipGraph and later calls replay it
//      (one hipGraphLaunch instead of ~40 kernel launches on the host).  LITEPI_NO_GRAPH=1 keeps every call of a handle
//      created under it eager (RunOptions).
// One enumerator per captured piece: a key of another piece never compares equal, so no entry point replays another's step.
// A host entry point's three pieces are consecutive: run_host_pass takes the front's and counts on.
enum GraphKind {
  GK_BATCH_DEVICE,                                // lp_run_batch_device
  GK_DETECT,                                      // lp_detect
  GK_BATCH_FRONT, GK_BATCH_ROI, GK_BATCH_CLS,     // lp_run_batch: detect + NMS, ROI resize, classifier
  GK_TILED_FRONT, GK_TILED_ROI, GK_TILED_CLS,     // lp_run_tiled: tiled detect + frame NMS, ROI resize, classifier
  GK_TILED_DEVICE,                                // lp_run_tiled_device
  GK_VIEWS_FRONT, GK_VIEWS_ROI, GK_VIEWS_CLS,     // lp_run_views: view gather + detect + frame NMS, ROI resize, classifier
  GK_VIEWS_DEVICE,                                // lp_run_views_device
  GK_FOCUS_FRONT, GK_FOCUS_ROI, GK_FOCUS_CLS,     // lp_run_focus: view gather + detect + mask + frame NMS, ROI resize, classifier
  GK_FOCUS_DEVICE,                                // lp_run_focus_device
  GK_SURFACES_DEVICE,                             // lp_run_surfaces_device
  GK_VIEWS_SURFACES_DEVICE,                       // lp_run_views_surfaces_device
};
struct GraphKey {
  GraphKind kind;
  int B, geom_ver, min_area;
  const void* p0; void* p1; void* p2;
  float conf, iou;
  // the frame format the step was captured with (key_format; all zero for packed BGR) and the identity of its conversion table
  int pixfmt = 0, matrix = 0, pitch = 0, csc_gen = 0;
  int64_t uv_offset = 0, frame_stride = 0;
  bool operator==(const GraphKey& o) const {
    return kind == o.kind && B == o.B && geom_ver == o.geom_ver && min_area == o.min_area && p0 == o.p0 && p1 == o.p1 && p2 == o.p2 &&
           conf == o.conf && iou == o.iou && pixfmt == o.pixfmt && matrix == o.matrix && pitch == o.pitch && csc_gen == o.csc_gen &&
           uv_offset == o.uv_offset && frame_stride == o.frame_stride;
  }
};
struct GraphEntry { GraphKey key; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; bool failed = false; unsigned long stamp = 0; };

// The run path's environment switches, read once per handle in lp_create: LITEPI_NO_GRAPH (every call eager),
// LITEPI_SKIP_STAGE=nms|roi|cls (diagnostic, pipeline.cpp: skip_stage), LITEPI_UPLOAD_THREADS (copy workers of the host upload,
// <= 0: none) and LITEPI_UPLOAD_GROUP_MB (its group size).
struct RunOptions {
  bool no_graph = false;
  std::string skip_stage;
  int upload_threads = 8;
  size_t upload_group_mb = 10;
};

}  // namespace lp

struct lp_handle {
  lp_config cfg;
  lp::RunOptions opt;
  // the detector input, rows x columns (lp_config::det_input_h: 0 = square)
  int det_h() const { return cfg.det_input_h ? cfg.det_input_h : cfg.det_input; }
  int det_w() const { return cfg.det_input; }
  std::unique_ptr<lp::Tracker> trk;   // null until lp_tracker_create: no other path looks at it
  std::unique_ptr<lp::Evaluator> evl; // null until lp_eval_create: no other path looks at it
  void* comm = nullptr;        // ncclComm_t of lp_comm_init
  int comm_rank = 0, comm_world = 1;
  // pinned staging of the host entry points + the copy workers (created on first use)
  uint8_t* h_stage = nullptr;
  size_t h_stage_bytes = 0;
  std::unique_ptr<lp::CopyPool> pool;
  hipStream_t own_stream = nullptr, stream = nullptr;
  std::unique_ptr<lp::Detector> det;
  std::unique_ptr<lp::ClassifierBase> cls;
  lp::Profiler prof;
  bool prof_next = false;
  int max_rois = 0;
  // device buffers
  lp::DevBuf d_src, d_lb, d_geom, d_cand, d_cand_count, d_sorted, d_dets, d_counts, d_rects, d_out0;
  lp::DevBuf d_roi_base, d_roi_total, d_roi_img, d_roi_slot, d_roi_rgb, d_probs, d_ids, d_conf;
  std::vector<lp::ImgGeom> geom_cache;
  // frame views (lp_run_tiled*, lp_run_views*): frame geometry, frame table + view slots, per-view counts; allocated on first use
  lp::DevBuf d_fgeom, d_ftab, d_vcnt;
  lp::DevBuf d_vwin;   // scaled views (lp_run_views*): the window table, [max_batch] ViewWin; allocated on first use
  // mapped views (lp_map_add, lp_run_mapped*): the handle's maps as device tables fixed[S][S][2] (view_map.h) with the frame
  // size they belong to, and the per-slot map table of a call, [max_batch] MapSlot; both allocated on first use
  struct MapEntry { lp::DevBuf fixed; int H = 0, W = 0; double foot_bytes = 0.0; };   // foot_bytes: the frame bytes its positions span
  std::vector<std::unique_ptr<MapEntry>> maps;
  lp::DevBuf d_vmap;
  std::vector<char> tile_cache;
  lp_view_merge vmerge = {};   // lp_set_view_merge: how the frame NMS merges a frame's views (zeros: the reference's rule)
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // staged host pass: start, after the ROI resize, after the front, end
  int last_roi_count = 0;
  // top-k of the class distribution per detection (lp_topk_enable): k (0 = off) and the [max_batch * max_det] lp_topk records,
  // allocated at the first enable and kept until lp_destroy.  While k == 0 no path looks at either.
  int topk_k = 0;
  lp::DevBuf d_topk;
  // crop quality per detection (lp_quality_enable): on / off and the [max_batch * max_det] lp_quality records, allocated at the
  // first enable and kept until lp_destroy.  While off no path looks at either.
  bool quality_on = false;
  lp::DevBuf d_quality;
  // where the last pipeline call's BGR frames and their geometry are (host bookkeeping; the evidence store reads them behind
  // lp_inventory*(crops = 1)).  Whatever rewrites or reallocates d_src or d_geom (ensure_src, upload_geom: every entry point
  // that does so, lp_detect* and lp_classify included) forgets them first; the pipeline entry points remember their own
  // frames afterwards, so a store never reads a table or a buffer that a later call of another kind has replaced
  // (lp_inventory*(crops = 1) is then LP_ERR_STATE).  d_tframes / d_tgeom: the frames of lp_test_set_frames, allocated on first use
  const uint8_t* last_frames = nullptr;
  const lp::ImgGeom* last_fgeom = nullptr;
  int last_nframes = 0;
  lp::DevBuf d_tframes, d_tgeom;
  void remember_frames(const uint8_t* src, const lp::ImgGeom* geom, int B) { last_frames = src; last_fgeom = geom; last_nframes = B; }
  // ---- input pixel format (lp_set_input_format).  NV12 frames are converted into d_src, which then holds exactly the packed
  //      BGR frames a BGR call would have put there; host NV12 frames are uploaded into d_raw first.  The converter reads its
  //      per-frame geometry from one of four table slots in d_csc: a slot's content never changes while a captured step may
  //      still point at it (a re-used slot gets a new generation number, which is part of the graph key), so alternating
  //      layouts keep their captured steps.
  lp_frame_format fmt = {};
  lp::DevBuf d_raw, d_csc;
  struct CscSlot { std::vector<char> tab; int gen = 0; };
  CscSlot csc_slots[4];
  int csc_gen = 0, csc_next = 0;
  bool nv12() const { return fmt.pixfmt == LP_PIX_NV12; }
  void ensure_raw(size_t bytes) {
    if (d_raw.bytes < bytes) {
      d_raw.alloc(bytes + bytes / 4, false);
      ++geom_ver;
    }
  }
  // Decoder surfaces (lp_run_surfaces_device, lp_run_views_surfaces_device; surfaces.cpp): a plan ring with one device table,
  // [max_batch] SurfFrame.  A surface's address and pitches are data in that table and not part of a step's identity.
  std::unique_ptr<lp::PlanRing> surf;   // null until the first surfaces call: no other path looks at it
  std::vector<lp::GraphEntry> graphs;   // captured steps (run_or_capture)
  int64_t n_eager = 0, n_captures = 0, n_replays = 0;   // lp_graph_stats: calls of run_or_capture by what they did
  int geom_ver = 0;
  unsigned long graph_clock = 0;
  void drop_graphs() {
    for (auto& g : graphs) {
      if (g.exec) (void)hipGraphExecDestroy(g.exec);
      if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    graphs.clear();
  }

  lp::RoiTable roi_table() {
    lp::RoiTable t;
    t.base = d_roi_base.as<int>(); t.total = d_roi_total.as<int>(); t.work = d_roi_total.as<int>() + 4;
    t.img = d_roi_img.as<int>(); t.slot = d_roi_slot.as<int>();
    return t;
  }
  void ensure_src(size_t bytes) {
    remember_frames(nullptr, nullptr, 0);   // d_src is about to be rewritten
    if (d_src.bytes < bytes) {
      d_src.alloc(bytes + bytes / 4, false);
      ++geom_ver;  // captured steps hold the old address
    }
  }
  void alloc_post_buffers() {
    const int B = cfg.max_batch, A = det->num_anchors(), nc = det->num_classes();
    d_cand.alloc((size_t)B * A * sizeof(lp::Cand), false);
    d_sorted.alloc((size_t)B * A * sizeof(lp::Cand), false);
    d_cand_count.alloc((size_t)B * 4);
    d_dets.alloc((size_t)B * cfg.max_det * sizeof(lp_det));
    d_counts.alloc((size_t)3 * B * 4);
    d_rects.alloc((size_t)B * cfg.max_det * 16);
    d_out0.alloc((size_t)B * (4 + nc) * A * 4, false);
  }
  void upload_geom(const std::vector<lp::ImgGeom>& g) {
    remember_frames(nullptr, nullptr, 0);   // d_geom now describes this call's images
    bool same = g.size() == geom_cache.size() && (g.empty() || memcmp(g.data(), geom_cache.data(), g.size() * sizeof(lp::ImgGeom)) == 0);
    if (same) return;
    LP_HIP(hipMemcpyAsync(d_geom.p, g.data(), g.size() * sizeof(lp::ImgGeom), hipMemcpyHostToDevice, stream));
    LP_HIP(hipStreamSynchronize(stream));  // g may be a temporary; uploads are rare (shape changes only)
    geom_cache = g;
    ++geom_ver;
  }
};

#define LP_API_BEGIN try {
#define LP_API_END                                   \
  }                                                  \
  catch (const lp::Error& e) {                       \
    lp::set_last_error(e.what());                    \
    return e.code;                                   \
  }                                                  \
  catch (const std::exception& e) {                  \
    lp::set_last_error(e.what());                    \
    return LP_ERR_STATE;                             \
  }                                                  \
  return LP_OK;

namespace lp {

// ---- pipeline pieces shared by the entry points (pipeline.cpp) -----------------------------------------------------------------
// letterbox geometry exactly as the reference computes it in Python doubles (e2e.py:72-83)
// with one side per axis, (SH, SW) = (rows, columns); lp_letterbox_geometry returns its fields
ImgGeom make_geom(int h, int w, int SH, int SW, long src_off);
// the frame-view families (tiled, views, focus) take a square detector input: LP_ERR_STATE on a rectangular handle
void check_square(const lp_handle* h, const char* what);
Profiler* begin_profile(lp_handle* h);
// the argument checks of lp_run_batch*, lp_run_tiled* and lp_run_views*: pointers, loaded models (host calls need the classifier),
// batch size, and for host calls min_area
void check_run_args(const lp_handle* h, bool pointers, int B, bool host, int min_area);
// the letterbox of n images (geometry geoms on the host, d_geom on the device) into dst [n,SH,SW,3], booked as every source byte
// once + every output byte once
void enqueue_letterbox(const uint8_t* src, const ImgGeom* d_geom, uint8_t* dst, const ImgGeom* geoms, int n, int SH, int SW, hipStream_t st,
                       Profiler* prof);
// detector (+ optional letterbox) on images resident at src with geometry already uploaded
void enqueue_detect(lp_handle* h, const uint8_t* src, const std::vector<ImgGeom>& geoms, int B, float conf, float* out0, Profiler* prof);
// the arguments the image NMS and the frame NMS share: results into dets / counts / rects, A anchors of nc classes; the ROI
// rule, the ROI list (with_rois) and its capacity are the handle's
NmsCommon nms_common(lp_handle* h, lp_det* dets, int* counts, int* rects, int A, int nc, int max_det, float iou, int min_area,
                     bool with_rois);
// NMS + ROI rectangles; with_rois: also the batch-wide ROI list the classifier stage consumes
void enqueue_nms(lp_handle* h, int B, float iou, int min_area, lp_det* dets, int* counts, bool with_rois, Profiler* prof);
// PIL resize + classifier + softmax over the ROI list; stage 0 = both halves, 1 = only the ROI resize, 2 = only the classifier;
// geom: the images' geometry (default d_geom; the tiled path passes its frame geometry)
void enqueue_classify(lp_handle* h, const uint8_t* src, int B, lp_det* dets, float* probs, int* ids, float* conf, Profiler* prof, int stage = 0,
                      const ImgGeom* geom = nullptr);
// top-k on: clear the B * max_det records of the call's frames, then (classify: a classifier ran and left its probabilities in
// d_probs) the select over the classified ROIs; two plain launches.  Never called while top-k is off.
void enqueue_topk(lp_handle* h, int B, bool classify, Profiler* prof);
// quality on: clear the B * max_det records of the call's frames, then (classify: a classifier is loaded, so the ROI stage
// left its crops in d_roi_rgb) the measure over the classified ROIs; two plain launches.  Never called while quality is off.
void enqueue_quality(lp_handle* h, int B, bool classify, Profiler* prof);
// the measure launch's arguments for B frames on the handle's ROI list and crops (pipeline.cpp; lp_test_quality shares them)
QualityArgs quality_args(lp_handle* h, int B);
// eager the first time a key is seen, captured into a hipGraph the second time, replayed from then on
void run_or_capture(lp_handle* h, const GraphKey& key, bool allow, const std::function<void()>& enqueue);

// ---- the two passes every lp_run_* entry point ends in (pipeline.cpp) -------------------------------------------------------------
// Where a call's packed BGR frames are once `convert` has run (empty: they are there already), and the graph key fields the
// source owns: p0 and the format fields.  device_frames (pixfmt.cpp) and surface_frames (surfaces.cpp) make them.
struct FrameSource {
  const uint8_t* src = nullptr;
  std::function<void(Profiler*)> convert;
  GraphKey key = {};
};
// What runs on those frames: detect + NMS (plain_front) or view gather + detect + frame NMS (view_front), writing records and
// counts; with_rois: also the ROI list the classifier stage consumes.  roi_geom: the geometry the ROI stage reads the frames
// with (nullptr: d_geom).  A front refers to the geometry or layout it was made from: it lives no longer than they do.
struct Front {
  std::function<void(Profiler*, lp_det* dets, int* counts, int min_area, bool with_rois)> run;
  const ImgGeom* roi_geom = nullptr;
};
Front plain_front(lp_handle* h, const uint8_t* src, const std::vector<ImgGeom>& geoms, int B, float conf, float iou);
// The device pass of every lp_run_*_device entry point, called behind the entry point's last check and upload: one captured
// step (conversion, front, and ROI resize + classifier when one is loaded) under the key {kind, the call, the source's
// fields}.  before: enqueued in front of the step, outside the capture, inside the profile (the focus plan launch).
void run_device_pass(lp_handle* h, GraphKind kind, int B, float conf, float iou, int min_area, void* dev_dets, void* dev_counts,
                     const FrameSource& frames, const Front& front, const std::function<void(Profiler*)>& before = nullptr);

// ---- input pixel format (pixfmt.cpp) -------------------------------------------------------------------------------------------
// the layout of one H x W frame with the zeros resolved
struct FrameLayout { int pitch; int64_t uv_off, frame_bytes, stride; };
// one conversion launch: table in a slot of d_csc, grid extent, matrix, identity for the graph key, pixels for the profile
struct CscPlan {
  const CscFrame* dev = nullptr;
  int B = 0, max_blocks = 0, matrix = 0, gen = 0;
  double pixels = 0.0;
};
inline size_t align16(size_t n) { return (n + 15) & ~(size_t)15; }
void check_format(const lp_frame_format* f);
FrameLayout frame_layout(const lp_frame_format& f, int H, int W);
void finish_csc_table(std::vector<CscFrame>& tab, const void* src, const void* dst);
CscPlan plan_csc(lp_handle* h, std::vector<CscFrame>& tab, const void* src);
void enqueue_csc(lp_handle* h, const uint8_t* src, const CscPlan& p, Profiler* prof);
void key_format(const lp_handle* h, const CscPlan& p, GraphKey& k);
CscPlan device_csc(lp_handle* h, const void* dev_imgs, int B, int H, int W, std::vector<ImgGeom>& g);
// the frames of a lp_*_device call as a frame source: packed BGR in place, NV12 converted into d_src under csc
FrameSource device_frames(lp_handle* h, const void* dev_imgs, const CscPlan& csc);

// ---- host frames (pipeline.cpp) ------------------------------------------------------------------------------------------------
// upload B host images of individual sizes into d_src (NV12 frames: into d_raw, with the plan of their conversion into d_src
// in *csc); returns their geometry
std::vector<ImgGeom> upload_images(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, CscPlan* csc = nullptr);
// The staged host pass of lp_run_batch, lp_run_tiled, lp_run_views and lp_run_focus on the frames upload_images left: the colour
// conversion under csc + `front`, the ROI resize and the classifier as three captured pieces (front_kind and the two
// enumerators behind it) with the stage events between them, then records, counts and timing back on the host.  An overflow
// of max_rois is reported last: the records are delivered.
void run_host_pass(lp_handle* h, int B, float conf, float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg,
                   lp_timing* timing, const CscPlan& csc, GraphKind front_kind, const Front& front);
// R crops as R "images" whose single ROI is the whole crop (lp_classify, lp_test_roi_resize): geometry at 16-byte aligned
// offsets, one rectangle each, img[i] = i, slot 0; total = bytes of the packed crops
struct CropRois {
  std::vector<ImgGeom> g;
  std::vector<int> rects, img, slot;
  size_t total = 0;
};
CropRois whole_crop_rois(const uint8_t* const* rois, const int* hs, const int* ws, int R);

// ---- frame views: tiled inference and scaled views (views.cpp) ------------------------------------------------------------------
// One view of a frame: the letterboxed whole frame, a native S x S crop at (x, y) -- it may pass the frame's edge where the
// frame is shorter than S --, or the window {x, y, w, h} letterboxed at its own scale.
// A mapped view (lp_run_mapped*) shows the frame through map x of the handle (lp_map_add); y, w and h are unused.
enum ViewKind { VIEW_FULL, VIEW_CROP, VIEW_WINDOW, VIEW_MAPPED };
struct FrameView { ViewKind kind; int x, y, w, h; };
using FrameViews = std::vector<std::vector<FrameView>>;   // every frame's views, in the frame's view order
// The call's view layout.  Batch slots: first the L letterboxed views (one launch of the letterbox kernel, so they are exactly
// lp_run_batch's input), then the C crops, then the windows, whose table entries wins[i] fill slot L + C + i (no windows: an
// empty table), then the mapped views, whose table entries maps[i] fill slot L + C + wins.size() + i (likewise).  frames[f] /
// vslot list each frame's slots in the frame's view order.
struct ViewLayout {
  std::vector<ImgGeom> vgeom;     // [V] by slot
  std::vector<TileFrame> frames;  // [F]
  std::vector<int> vslot;         // [V] frame-major
  std::vector<ViewWin> wins;      // the windows
  std::vector<MapSlot> maps;      // the mapped views: V = L + C + wins.size() + maps.size()
  double map_src_bytes = 0.0;     // the frame bytes the mapped views' tables span (the profiler's booking)
  int L = 0, C = 0, V = 0, max_views = 0;
};
void check_tiling(const lp_tiling* t, int S);
void check_view_merge(const lp_view_merge* m);
void apply_view_merge(const lp_handle* h, float iou, FrameNmsArgs& a);
// the frames' views under tiling (lp_tile_grid of every frame) / through one list of {x, y, w, h} views, validated against every frame
FrameViews tiled_views(int S, const lp_tiling& t, const std::vector<ImgGeom>& fg);
FrameViews listed_views(const lp_handle* h, const int* views, int n_views, const std::vector<ImgGeom>& fg);
// the list (n_views may be 0), then the handle's maps of the given ids; every frame must have every listed map's size
FrameViews mapped_views(const lp_handle* h, const int* views, int n_views, const int* maps, int n_maps, const std::vector<ImgGeom>& fg);
// the one builder; LP_ERR_ARG for more views than max_batch or than the frame NMS holds per frame
ViewLayout view_layout(const lp_handle* h, const std::vector<ImgGeom>& fg, const FrameViews& per);
// upload the frame geometry, the frame table, the view slots, the view geometry, the window table and the map table when any of
// them changed; a change invalidates captured graphs (geom_ver)
void upload_tiles(lp_handle* h, const std::vector<ImgGeom>& fg, const ViewLayout& lay);
// letterboxed views through launch_letterbox, crops through launch_crop_views, windows through launch_window_views, mapped views
// through launch_map_views (d_maps: their device table), into dst [V,S,S,3]; what the layout does not contain is not launched
void enqueue_view_gather(const uint8_t* src, const ImgGeom* d_geom, const ViewWin* d_wins, uint8_t* dst, const ViewLayout& lay, int S,
                         hipStream_t st, Profiler* prof, const MapSlot* d_maps = nullptr);
// view gather + detector on the views + frame NMS (+ the ROI list when with_rois); dead (focus views only): view slots whose
// candidates are dropped between the detector and the view sort
void enqueue_view_front(lp_handle* h, const uint8_t* src, const ViewLayout& lay, int F, float conf, float iou, int min_area, lp_det* dets,
                        int* counts, bool with_rois, Profiler* prof, const int* dead = nullptr);
Front view_front(lp_handle* h, const uint8_t* src, const ViewLayout& lay, int F, float conf, float iou, const int* dead = nullptr);
// What a view entry point brings along: its frames' geometry -> the call's layout (its own argument checks included).
// Everything is validated in one order: the shared arguments, the layout against every frame, the NV12 format; only then is
// anything uploaded or allocated.
using LayoutFn = std::function<ViewLayout(const std::vector<ImgGeom>&)>;
// Host frames of a view call: the layout dry-run on geometry without offsets (upload_images assigns them), the NV12 format
// check, the upload into d_src (fg, csc), and the layout of the uploaded frames.
ViewLayout upload_view_frames(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const LayoutFn& layout_of,
                              std::vector<ImgGeom>& fg, CscPlan& csc);
// Device frames of a view call: B packed H x W frames; NV12 frames get their conversion plan (device_csc checks the format
// before it sizes d_src) and the layout is built again on the converted frames' 16-byte aligned offsets.
ViewLayout device_view_frames(lp_handle* h, const void* dev_imgs, int B, int H, int W, const LayoutFn& layout_of, std::vector<ImgGeom>& fg,
                              CscPlan& csc);

}  // namespace lp
