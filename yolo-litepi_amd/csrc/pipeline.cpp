// The pipeline pieces the entry points share, the host upload path, the staged host pass, and the untiled entry points.
#include <cmath>

#include "handle.h"

namespace lp {

// letterbox geometry exactly as the reference computes it in Python doubles (e2e.py:72-83);
// Python's round() is round-half-to-even == nearbyint in the default rounding mode.
// One side per axis (the reference's new_shape = (rows, columns)); lp_letterbox_geometry returns this function's fields.
ImgGeom make_geom(int h, int w, int SH, int SW, long src_off) {
  ImgGeom g;
  memset(&g, 0, sizeof(g));  // padding bytes too: geometry is compared with memcmp
  const double r = std::min((double)SH / h, (double)SW / w);
  const int nw = (int)std::nearbyint(w * r), nh = (int)std::nearbyint(h * r);
  const double dw = (SW - nw) / 2.0, dh = (SH - nh) / 2.0;
  g.src_off = src_off; g.h = h; g.w = w; g.new_w = nw; g.new_h = nh;
  g.top = (int)std::nearbyint(dh - 0.1);
  g.left = (int)std::nearbyint(dw - 0.1);
  g.ratio = (float)r; g.pad_w = (float)dw; g.pad_h = (float)dh;
  return g;
}

void check_square(const lp_handle* h, const char* what) {
  LP_CHECK(h, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det_h() == h->det_w(), LP_ERR_STATE, "%s needs a square detector input; this handle's is %dx%d (rows x columns, lp_config::det_input_h)",
           what, h->det_h(), h->det_w());
}

Profiler* begin_profile(lp_handle* h) {
  if (!h->prof_next) return nullptr;
  h->prof_next = false;
  h->prof.enabled = true;
  h->prof.results.clear();
  return &h->prof;
}

void check_run_args(const lp_handle* h, bool pointers, int B, bool host, int min_area) {
  LP_CHECK(h && pointers, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(!host || (h->cls && h->cls->loaded()), LP_ERR_STATE, "classifier not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_CHECK(!host || min_area >= 0, LP_ERR_ARG, "min_area must be >= 0");
}

void enqueue_letterbox(const uint8_t* src, const ImgGeom* d_geom, uint8_t* dst, const ImgGeom* geoms, int n, int SH, int SW, hipStream_t st,
                       Profiler* prof) {
  if (prof) prof->begin(st);
  launch_letterbox(src, d_geom, dst, n, SH, SW, st, geoms);
  if (prof) {
    double bytes = (double)n * SH * SW * 3;
    for (int i = 0; i < n; ++i) bytes += (double)geoms[i].h * geoms[i].w * 3;
    prof->end(st, "letterbox_u8", "letterbox", 0.0, bytes);
  }
}

// detector (+ optional letterbox) on images resident at src with geometry already uploaded
void enqueue_detect(lp_handle* h, const uint8_t* src, const std::vector<ImgGeom>& geoms, int B, float conf, float* out0,
                    Profiler* prof) {
  const int SH = h->det_h(), SW = h->det_w();
  bool identity = true;
  for (int i = 0; i < B; ++i)
    identity = identity && geoms[i].h == SH && geoms[i].w == SW && geoms[i].src_off == (long)i * SH * SW * 3;
  const uint8_t* img = src;
  if (!identity) {
    enqueue_letterbox(src, h->d_geom.as<ImgGeom>(), h->d_lb.as<uint8_t>(), geoms.data(), B, SH, SW, h->stream, prof);
    img = h->d_lb.as<uint8_t>();
  }
  h->det->forward(img, B, h->d_geom.as<ImgGeom>(), conf, out0, h->d_cand.as<Cand>(), h->d_cand_count.as<int>(), h->stream, prof);
}

// Diagnostic only (tools/marginal_cost.sh): LITEPI_SKIP_STAGE=nms|roi|cls leaves that stage out of every pass after the handle's
// first (its outputs stay in the handle's buffers): the marginal cost of the stage in a pipelined step.  Results are stale.
static bool skip_stage(const lp_handle* h, const char* name, const Profiler* prof) {
  return !prof && h->graph_clock > 1 && h->opt.skip_stage == name;
}

NmsCommon nms_common(lp_handle* h, lp_det* dets, int* counts, int* rects, int A, int nc, int max_det, float iou, int min_area,
                     bool with_rois) {
  NmsCommon c;
  memset(&c, 0, sizeof(c));
  c.dets = dets; c.counts = counts; c.rects = rects;
  c.A = A; c.max_det = max_det; c.nc = nc; c.iou = iou; c.min_area = min_area;
  if (with_rois) c.tab = h->roi_table();
  c.max_rois = h->max_rois;
  c.roi_rule = h->cfg.numerics;
  return c;
}

// NMS + ROI rectangles; with_rois: also the batch-wide ROI list the classifier stage consumes
void enqueue_nms(lp_handle* h, int B, float iou, int min_area, lp_det* dets, int* counts, bool with_rois, Profiler* prof) {
  NmsArgs a;
  memset(&a, 0, sizeof(a));
  a.cand = h->d_cand.as<Cand>(); a.cand_count = h->d_cand_count.as<int>(); a.sorted = h->d_sorted.as<Cand>();
  a.geom = h->d_geom.as<ImgGeom>();
  a.c = nms_common(h, dets, counts, h->d_rects.as<int>(), h->det->num_anchors(), h->det->num_classes(), h->cfg.max_det, iou, min_area, with_rois);
  if (skip_stage(h, "nms", prof)) return;
  if (prof) prof->begin(h->stream);
  launch_nms(a, B, h->stream);
  if (prof) prof->end(h->stream, "nms", "nms", 0.0, 0.0);
}

// PIL resize + ShuffleNetV2 + softmax over the ROI list; scatters (cls, conf) into dets when given
// stage: 0 = both halves, 1 = only the ROI crop + resize (the device's share of the reference's ROI loop, e2e.py:460-475),
// 2 = only the classifier (lp_run_batch times the two separately: PipelineMetrics.t_roi_extract / t_classification)
// geom: the images' geometry (default d_geom; the tiled path passes its frame geometry)
void enqueue_classify(lp_handle* h, const uint8_t* src, int B, lp_det* dets, float* probs, int* ids, float* conf, Profiler* prof, int stage,
                      const ImgGeom* geom) {
  RoiTable tab = h->roi_table();
  if (stage != 2 && !skip_stage(h, "roi", prof)) {
    RoiResizeArgs r;
    r.src = src; r.geom = geom ? geom : h->d_geom.as<ImgGeom>(); r.rects = h->d_rects.as<int>(); r.tab = tab;
    r.out = h->d_roi_rgb.as<uint8_t>(); r.max_det = h->cfg.max_det; r.S = h->cfg.cls_input; r.linear = h->cfg.numerics;
    if (prof) prof->begin(h->stream);
    launch_roi_resize(r, std::min(h->max_rois, B * h->cfg.max_det), h->stream);
    if (prof) prof->end(h->stream, "roi_resize_pil", "roi_resize", 0.0, (double)r.S * r.S * 3 * 2, true);
  }
  if (stage == 1 || skip_stage(h, "cls", prof)) return;
  ClsPost post;
  post.probs = probs; post.ids = ids; post.dets = dets; post.max_det = h->cfg.max_det; post.roi_img = tab.img; post.roi_slot = tab.slot;
  h->cls->forward(h->d_roi_rgb.as<uint8_t>(), tab.total, h->stream, prof, &post);
  if (!h->cls->fused_head()) {
    if (prof) prof->begin(h->stream);
    launch_softmax_argmax(h->cls->logits(), h->cls->logits_pitch(), h->cls->num_classes(), probs, ids, conf, dets, h->cfg.max_det,
                          &tab, tab.total, h->max_rois, h->stream);
    if (prof) prof->end(h->stream, "softmax_argmax", "softmax", 0.0, (double)h->cls->num_classes() * 8, true);
  }
}

void enqueue_topk(lp_handle* h, int B, bool classify, Profiler* prof) {
  lp_topk* out = h->d_topk.as<lp_topk>();
  if (prof) prof->begin(h->stream);
  launch_topk_clear(out, B * h->cfg.max_det, h->stream);
  if (prof) prof->end(h->stream, "topk_clear", "topk", 0.0, (double)B * h->cfg.max_det * sizeof(lp_topk));
  if (!classify) return;
  RoiTable tab = h->roi_table();
  TopkArgs a;
  a.probs = h->d_probs.as<float>(); a.total = tab.total; a.roi_img = tab.img; a.roi_slot = tab.slot; a.out = out;
  a.nc = h->cls->num_classes(); a.k = h->topk_k; a.B = B; a.max_det = h->cfg.max_det;
  a.cap = std::min(h->max_rois, B * h->cfg.max_det);
  if (prof) prof->begin(h->stream);
  launch_topk_select(a, h->stream);
  if (prof) prof->end(h->stream, "topk_select", "topk", 0.0, (double)a.nc * 4 + sizeof(lp_topk), true);
}

QualityArgs quality_args(lp_handle* h, int B) {
  RoiTable tab = h->roi_table();
  QualityArgs a;
  a.roi_rgb = h->d_roi_rgb.as<uint8_t>(); a.total = tab.total; a.roi_img = tab.img; a.roi_slot = tab.slot; a.out = h->d_quality.as<lp_quality>();
  a.S = h->cfg.cls_input; a.B = B; a.max_det = h->cfg.max_det;
  a.cap = std::min(h->max_rois, B * h->cfg.max_det);
  return a;
}

void enqueue_quality(lp_handle* h, int B, bool classify, Profiler* prof) {
  if (prof) prof->begin(h->stream);
  launch_quality_clear(h->d_quality.as<lp_quality>(), B * h->cfg.max_det, h->stream);
  if (prof) prof->end(h->stream, "quality_clear", "quality", 0.0, (double)B * h->cfg.max_det * sizeof(lp_quality));
  if (!classify) return;
  const QualityArgs a = quality_args(h, B);
  if (prof) prof->begin(h->stream);
  launch_quality_measure(a, h->stream);
  if (prof) prof->end(h->stream, "quality_measure", "quality", 0.0, 3.0 * a.S * a.S + sizeof(lp_quality), true);
}

// Run `enqueue` (kernel launches on h->stream only: no allocation, no synchronisation) eagerly the first time a key is
// seen -- that call also performs every one-time set-up (LDS attributes, lazy packing) --, capture it into a hipGraph the
// second time, replay the graph from then on.
void run_or_capture(lp_handle* h, const GraphKey& key, bool allow, const std::function<void()>& enqueue) {
  if (h->opt.no_graph || !allow) { ++h->n_eager; enqueue(); return; }
  GraphEntry* e = nullptr;
  for (auto& g : h->graphs)
    if (g.key == key) { e = &g; break; }
  if (!e) {  // first sight: eager, remember the key
    if (h->graphs.size() >= 32) {  // evict the least recently used entry
      size_t lru = 0;
      for (size_t i = 1; i < h->graphs.size(); ++i)
        if (h->graphs[i].stamp < h->graphs[lru].stamp) lru = i;
      if (h->graphs[lru].exec) (void)hipGraphExecDestroy(h->graphs[lru].exec);
      if (h->graphs[lru].graph) (void)hipGraphDestroy(h->graphs[lru].graph);
      h->graphs.erase(h->graphs.begin() + lru);
    }
    GraphEntry ne;
    ne.key = key;
    ne.stamp = ++h->graph_clock;
    h->graphs.push_back(ne);
    ++h->n_eager;
    enqueue();
    return;
  }
  e->stamp = ++h->graph_clock;
  if (e->failed) { ++h->n_eager; enqueue(); return; }
  const bool replay = e->exec != nullptr;
  if (!e->exec) {
    if (hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) { e->failed = true; ++h->n_eager; enqueue(); return; }
    bool ok = true;
    std::string err;
    try { enqueue(); } catch (const lp::Error& ex) { ok = false; err = ex.what(); }
    hipGraph_t graph = nullptr;
    if (hipStreamEndCapture(h->stream, &graph) != hipSuccess || !graph) ok = false;
    if (ok && hipGraphInstantiate(&e->exec, graph, nullptr, nullptr, 0) != hipSuccess) { ok = false; e->exec = nullptr; }
    if (!ok) {
      if (graph) (void)hipGraphDestroy(graph);
      (void)hipGetLastError();
      e->failed = true;
      LP_CHECK(err.empty(), LP_ERR_STATE, "%s", err.c_str());
      ++h->n_eager;
      enqueue();
      return;
    }
    e->graph = graph;
  }
  LP_HIP(hipGraphLaunch(e->exec, h->stream));
  ++(replay ? h->n_replays : h->n_captures);   // lp_graph_stats: the call that captured a step also launched it once
}

// upload B host images of individual sizes into d_src (NV12 frames: into d_raw, with the plan of their conversion into d_src
// in *csc); returns their geometry
std::vector<ImgGeom> upload_images(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, CscPlan* csc) {
  const bool nv = h->nv12();
  lp_frame_format hf = h->fmt;
  hf.frame_stride = 0;   // host frames come one pointer each: frame_bytes apiece, the stride of device batches does not apply
  std::vector<ImgGeom> g(B);
  std::vector<size_t> nb(B), off(B);   // bytes of every frame as it is uploaded, and its offset in the upload buffer
  std::vector<CscFrame> tab;
  size_t bgr_total = 0, total = 0;
  for (int i = 0; i < B; ++i) {
    LP_CHECK(imgs[i] && hs[i] > 0 && ws[i] > 0, LP_ERR_ARG, "image %d is empty", i);
    g[i] = make_geom(hs[i], ws[i], h->det_h(), h->det_w(), (long)bgr_total);
    bgr_total = align16(bgr_total + (size_t)hs[i] * ws[i] * 3);
    if (nv) {
      const FrameLayout L = frame_layout(hf, hs[i], ws[i]);
      nb[i] = (size_t)L.frame_bytes; off[i] = total;
      tab.push_back(CscFrame{(long)total, (long)L.uv_off, g[i].src_off, hs[i], ws[i], L.pitch, 0});
      total = align16(total + nb[i]);
    } else {
      nb[i] = (size_t)hs[i] * ws[i] * 3; off[i] = (size_t)g[i].src_off;
      total = bgr_total;
    }
  }
  h->ensure_src(bgr_total);
  uint8_t* dst = h->d_src.as<uint8_t>();
  if (nv) {
    LP_CHECK(csc, LP_ERR_STATE, "this entry point takes packed BGR frames only");
    h->ensure_raw(total);
    dst = h->d_raw.as<uint8_t>();
    *csc = plan_csc(h, tab, dst);
  }
  // small uploads (a single frame: the batch-1 latency path) go straight from the caller's memory
  const int n_threads = h->opt.upload_threads;
  if (n_threads <= 0 || B < 4 || total < ((size_t)4 << 20)) {
    for (int i = 0; i < B; ++i)
      LP_HIP(hipMemcpyAsync(dst + off[i], imgs[i], nb[i], hipMemcpyHostToDevice, h->stream));
    return g;
  }
  if (h->h_stage_bytes < total) {
    if (h->h_stage) { LP_HIP(hipStreamSynchronize(h->stream)); (void)hipHostFree(h->h_stage); h->h_stage = nullptr; h->h_stage_bytes = 0; }
    LP_HIP(hipHostMalloc(reinterpret_cast<void**>(&h->h_stage), total + total / 4, hipHostMallocDefault));
    h->h_stage_bytes = total + total / 4;
  }
  if (!h->pool) h->pool.reset(new CopyPool(n_threads - 1));
  // (the previous call synchronised the stream before it returned: the staging buffer is free)
  // groups of about 10 MB: the workers fill group k+1 while the DMA engine moves group k; an image larger than that is split
  // into slices so that every worker has a share
  std::vector<CopyPool::Job> jobs;
  // (the first groups are small: nothing overlaps the first group's copy, the link idles until it is staged)
  const size_t group_mb = h->opt.upload_group_mb;
  const size_t slice = (size_t)1 << 20;
  int i0 = 0, ngroup = 0;
  while (i0 < B) {
    int i1 = i0;
    size_t gb = 0;
    const size_t group_bytes = ngroup == 0 ? (size_t)2 << 20 : (ngroup == 1 ? (size_t)5 << 20 : group_mb << 20);
    ++ngroup;
    jobs.clear();
    while (i1 < B && (i1 == i0 || gb + nb[i1] <= group_bytes)) {
      for (size_t o = 0; o < nb[i1]; o += slice) jobs.push_back({imgs[i1] + o, h->h_stage + off[i1] + o, std::min(slice, nb[i1] - o)});
      gb += nb[i1];
      ++i1;
    }
    h->pool->run(jobs.data(), (int)jobs.size());
    const size_t lo = off[i0], hi = off[i1 - 1] + nb[i1 - 1];
    LP_HIP(hipMemcpyAsync(dst + lo, h->h_stage + lo, hi - lo, hipMemcpyHostToDevice, h->stream));
    i0 = i1;
  }
  return g;
}

Front plain_front(lp_handle* h, const uint8_t* src, const std::vector<ImgGeom>& geoms, int B, float conf, float iou) {
  Front f;
  f.run = [=, &geoms](Profiler* prof, lp_det* dets, int* counts, int min_area, bool with_rois) {
    enqueue_detect(h, src, geoms, B, conf, nullptr, prof);
    enqueue_nms(h, B, iou, min_area, dets, counts, with_rois, prof);
  };
  return f;
}

void run_device_pass(lp_handle* h, GraphKind kind, int B, float conf, float iou, int min_area, void* dev_dets, void* dev_counts,
                     const FrameSource& frames, const Front& front, const std::function<void(Profiler*)>& before) {
  Profiler* prof = begin_profile(h);
  if (before) before(prof);
  const bool classify = h->cls && h->cls->loaded();
  const bool topk = h->topk_k > 0;   // lp_topk_enable: the step also fills the handle's lp_topk records
  const bool quality = h->quality_on;   // lp_quality_enable: and its lp_quality records
  lp_det* dets = static_cast<lp_det*>(dev_dets);
  h->remember_frames(frames.src, front.roi_geom ? front.roi_geom : h->d_geom.as<ImgGeom>(), B);
  GraphKey key = frames.key;
  key.kind = kind; key.B = B; key.geom_ver = h->geom_ver; key.min_area = min_area; key.p1 = dev_dets; key.p2 = dev_counts;
  key.conf = conf; key.iou = iou;
  run_or_capture(h, key, prof == nullptr, [&]() {
    if (frames.convert) frames.convert(prof);
    front.run(prof, dets, static_cast<int*>(dev_counts), classify ? min_area : -1, classify);
    if (classify) enqueue_classify(h, frames.src, B, dets, topk ? h->d_probs.as<float>() : nullptr, nullptr, nullptr, prof, 0, front.roi_geom);
    if (topk) enqueue_topk(h, B, classify, prof);
    if (quality) enqueue_quality(h, B, classify, prof);
  });
  if (prof) prof->enabled = false;  // records are collected by lp_profile_read after the caller synchronises
}

void run_host_pass(lp_handle* h, int B, float conf, float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg,
                   lp_timing* timing, const CscPlan& csc, GraphKind front_kind, const Front& front) {
  Profiler* prof = begin_profile(h);
  const uint8_t* src = h->d_src.as<uint8_t>();
  lp_det* d_dets = h->d_dets.as<lp_det>();
  const ImgGeom* roi_geom = front.roi_geom;
  h->remember_frames(src, roi_geom ? roi_geom : h->d_geom.as<ImgGeom>(), B);
  // three captured pieces with the stage-boundary events between them (PipelineMetrics wants detection, ROI extraction and
  // classification times separately, e2e.py:452-499); the colour conversion of NV12 frames is booked under detection
  GraphKey k1{front_kind, B, h->geom_ver, min_area, h->d_src.p, h->d_dets.p, h->d_counts.p, conf, iou}, k2 = k1, k3 = k1;
  k2.kind = GraphKind(front_kind + 1); k3.kind = GraphKind(front_kind + 2);
  key_format(h, csc, k1);   // the conversion is part of the front only
  LP_HIP(hipEventRecord(h->ev[0], h->stream));
  run_or_capture(h, k1, prof == nullptr, [&]() {
    if (h->nv12()) enqueue_csc(h, h->d_raw.as<uint8_t>(), csc, prof);
    front.run(prof, d_dets, h->d_counts.as<int>(), min_area, true);
  });
  LP_HIP(hipEventRecord(h->ev[2], h->stream));
  run_or_capture(h, k2, prof == nullptr, [&]() { enqueue_classify(h, src, B, d_dets, nullptr, nullptr, nullptr, prof, 1, roi_geom); });
  LP_HIP(hipEventRecord(h->ev[1], h->stream));
  const bool topk = h->topk_k > 0;   // lp_topk_enable: part of the classification piece
  run_or_capture(h, k3, prof == nullptr, [&]() {
    enqueue_classify(h, src, B, d_dets, topk ? h->d_probs.as<float>() : nullptr, nullptr, nullptr, prof, 2, roi_geom);
    if (topk) enqueue_topk(h, B, true, prof);
    if (h->quality_on) enqueue_quality(h, B, true, prof);   // lp_quality_enable: part of the classification piece too
  });
  LP_HIP(hipEventRecord(h->ev[3], h->stream));
  LP_HIP(hipMemcpyAsync(dets, h->d_dets.p, (size_t)B * h->cfg.max_det * sizeof(lp_det), hipMemcpyDeviceToHost, h->stream));
  std::vector<int> cnt(3 * B);
  LP_HIP(hipMemcpyAsync(cnt.data(), h->d_counts.p, (size_t)3 * B * 4, hipMemcpyDeviceToHost, h->stream));
  int R[2] = {0, 0};
  LP_HIP(hipMemcpyAsync(R, h->d_roi_total.p, 8, hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  for (int i = 0; i < B; ++i) {
    counts[i] = cnt[i];
    if (num_det) num_det[i] = cnt[B + i];
    if (det_conf_avg) memcpy(&det_conf_avg[i], &cnt[2 * B + i], 4);
  }
  h->last_roi_count = R[0];
  if (timing) {
    // the front (view gather, detector, decode + NMS) is booked under detection like the reference's detect() (e2e.py:452-453);
    // the ROI rectangles come out of the NMS kernel, the crop + PIL resize is the device's share of the ROI loop (e2e.py:460-475)
    (void)hipEventElapsedTime(&timing->t_detection, h->ev[0], h->ev[2]);
    (void)hipEventElapsedTime(&timing->t_roi_extract, h->ev[2], h->ev[1]);
    (void)hipEventElapsedTime(&timing->t_classification, h->ev[1], h->ev[3]);
    (void)hipEventElapsedTime(&timing->t_total, h->ev[0], h->ev[3]);
  }
  if (prof) { prof->collect(R[0]); prof->enabled = false; }
  // every kept ROI must have been classified (the reference classifies all of them): a user-set max_rois that was too
  // small is an error, not a silent cls_class = -1
  LP_CHECK(R[1] <= h->max_rois, LP_ERR_STATE, "%d ROIs in this batch exceed max_rois = %d: %d detections were left unclassified", R[1],
           h->max_rois, R[1] - h->max_rois);
}

CropRois whole_crop_rois(const uint8_t* const* rois, const int* hs, const int* ws, int R) {
  CropRois c;
  c.g.resize(R); c.rects.resize((size_t)R * 4); c.img.resize(R); c.slot.assign(R, 0);
  for (int i = 0; i < R; ++i) {
    LP_CHECK(rois[i] && hs[i] > 0 && ws[i] > 0 && hs[i] <= 4096 && ws[i] <= 4096, LP_ERR_ARG, "ROI %d has a bad size", i);
    memset(&c.g[i], 0, sizeof(ImgGeom));
    c.g[i].src_off = (long)c.total; c.g[i].h = hs[i]; c.g[i].w = ws[i];
    c.total += align16((size_t)hs[i] * ws[i] * 3);
    c.img[i] = i;
    int* rc = &c.rects[(size_t)i * 4];
    rc[0] = 0; rc[1] = 0; rc[2] = ws[i]; rc[3] = hs[i];
  }
  return c;
}
}  // namespace lp

using namespace lp;

extern "C" {

int lp_detect_raw(lp_handle* h, const uint8_t* bgr, int B, float* out0) {
  LP_API_BEGIN
  LP_CHECK(h && bgr && out0, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_HIP(hipSetDevice(h->cfg.device));
  const int SH = h->det_h(), SW = h->det_w();
  const size_t bytes = (size_t)B * SH * SW * 3;
  h->ensure_src(bytes);
  LP_HIP(hipMemcpyAsync(h->d_src.p, bgr, bytes, hipMemcpyHostToDevice, h->stream));
  std::vector<ImgGeom> g(B);
  for (int i = 0; i < B; ++i) g[i] = make_geom(SH, SW, SH, SW, (long)i * SH * SW * 3);
  h->upload_geom(g);
  Profiler* prof = begin_profile(h);
  LP_HIP(hipMemsetAsync(h->d_cand_count.p, 0, (size_t)h->cfg.max_batch * 4, h->stream));
  enqueue_detect(h, h->d_src.as<uint8_t>(), g, B, 2.0f /* nothing passes: raw output only */, h->d_out0.as<float>(), prof);
  const size_t obytes = (size_t)B * (4 + h->det->num_classes()) * h->det->num_anchors() * 4;
  LP_HIP(hipMemcpyAsync(out0, h->d_out0.p, obytes, hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  if (prof) { prof->collect(0); prof->enabled = false; }
  LP_API_END
}

int lp_detect(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, float conf, float iou,
              lp_det* dets, int* counts) {
  LP_API_BEGIN
  LP_CHECK(h && imgs && hs && ws && dets && counts, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_HIP(hipSetDevice(h->cfg.device));
  const bool nv = h->nv12();
  CscPlan csc;
  std::vector<ImgGeom> g = upload_images(h, imgs, hs, ws, B, &csc);
  h->upload_geom(g);
  Profiler* prof = begin_profile(h);
  GraphKey key{GK_DETECT, B, h->geom_ver, -1, h->d_src.p, h->d_dets.p, h->d_counts.p, conf, iou};
  key_format(h, csc, key);
  run_or_capture(h, key, prof == nullptr, [&]() {
    if (nv) enqueue_csc(h, h->d_raw.as<uint8_t>(), csc, prof);
    enqueue_detect(h, h->d_src.as<uint8_t>(), g, B, conf, nullptr, prof);
    enqueue_nms(h, B, iou, -1, h->d_dets.as<lp_det>(), h->d_counts.as<int>(), false, prof);
  });
  LP_HIP(hipMemcpyAsync(dets, h->d_dets.p, (size_t)B * h->cfg.max_det * sizeof(lp_det), hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipMemcpyAsync(counts, h->d_counts.p, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  if (prof) { prof->collect(0); prof->enabled = false; }
  LP_API_END
}

int lp_run_batch(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, float conf, float iou,
                 int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing) {
  LP_API_BEGIN
  check_run_args(h, imgs && hs && ws && dets && counts, B, true, min_area);
  LP_HIP(hipSetDevice(h->cfg.device));
  CscPlan csc;
  std::vector<ImgGeom> g = upload_images(h, imgs, hs, ws, B, &csc);
  h->upload_geom(g);
  run_host_pass(h, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, csc, GK_BATCH_FRONT,
                plain_front(h, h->d_src.as<uint8_t>(), g, B, conf, iou));
  LP_API_END
}

int lp_run_batch_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, float conf, float iou, int min_area,
                        void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  check_run_args(h, dev_imgs && dev_dets && dev_counts, B, false, min_area);
  LP_CHECK(H > 0 && W > 0, LP_ERR_ARG, "frames of %dx%d", W, H);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> g(B);
  CscPlan csc;
  if (h->nv12()) csc = device_csc(h, dev_imgs, B, H, W, g);
  else
    for (int i = 0; i < B; ++i) g[i] = make_geom(H, W, h->det_h(), h->det_w(), (long)i * H * W * 3);
  h->upload_geom(g);
  const FrameSource frames = device_frames(h, dev_imgs, csc);
  run_device_pass(h, GK_BATCH_DEVICE, B, conf, iou, min_area, dev_dets, dev_counts, frames, plain_front(h, frames.src, g, B, conf, iou));
  LP_API_END
}

int lp_classify(lp_handle* h, const uint8_t* const* rois, const int* hs, const int* ws, int R, int* ids, float* probs) {
  LP_API_BEGIN
  LP_CHECK(h && ids && probs, LP_ERR_ARG, "null argument");
  LP_CHECK(h->cls && h->cls->loaded(), LP_ERR_STATE, "classifier not loaded");
  LP_CHECK(R >= 0 && R <= h->max_rois && R <= h->cfg.max_batch * h->cfg.max_det, LP_ERR_ARG,
           "%d ROIs exceed the capacity (%d)", R, std::min(h->max_rois, h->cfg.max_batch * h->cfg.max_det));
  if (R == 0) return LP_OK;
  LP_CHECK(rois && hs && ws, LP_ERR_ARG, "null argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  const CropRois c = whole_crop_rois(rois, hs, ws, R);
  LP_CHECK(R <= (int)(h->d_geom.bytes / sizeof(ImgGeom)), LP_ERR_ARG, "too many ROIs");
  h->ensure_src(c.total);
  for (int i = 0; i < R; ++i)
    LP_HIP(hipMemcpyAsync(h->d_src.as<uint8_t>() + c.g[i].src_off, rois[i], (size_t)hs[i] * ws[i] * 3, hipMemcpyHostToDevice, h->stream));
  h->geom_cache.clear();
  LP_HIP(hipMemcpyAsync(h->d_geom.p, c.g.data(), (size_t)R * sizeof(ImgGeom), hipMemcpyHostToDevice, h->stream));
  DevBuf d_rects_tmp;  // [R][1][4]: one whole-crop rectangle per "image"
  d_rects_tmp.alloc((size_t)R * 16);
  LP_HIP(hipMemcpyAsync(d_rects_tmp.p, c.rects.data(), c.rects.size() * 4, hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_roi_img.p, c.img.data(), (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_roi_slot.p, c.slot.data(), (size_t)R * 4, hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_roi_total.p, &R, 4, hipMemcpyHostToDevice, h->stream));
  Profiler* prof = begin_profile(h);
  RoiTable tab = h->roi_table();
  RoiResizeArgs r;
  r.src = h->d_src.as<uint8_t>(); r.geom = h->d_geom.as<ImgGeom>(); r.rects = d_rects_tmp.as<int>(); r.tab = tab;
  r.out = h->d_roi_rgb.as<uint8_t>(); r.max_det = 1; r.S = h->cfg.cls_input; r.linear = h->cfg.numerics;
  launch_roi_resize(r, R, h->stream);
  ClsPost post;
  post.probs = h->d_probs.as<float>(); post.ids = h->d_ids.as<int>();
  h->cls->forward(h->d_roi_rgb.as<uint8_t>(), tab.total, h->stream, prof, &post);
  if (!h->cls->fused_head())
    launch_softmax_argmax(h->cls->logits(), h->cls->logits_pitch(), h->cls->num_classes(), h->d_probs.as<float>(), h->d_ids.as<int>(),
                          nullptr, nullptr, h->cfg.max_det, nullptr, tab.total, h->max_rois, h->stream);
  LP_HIP(hipMemcpyAsync(ids, h->d_ids.p, (size_t)R * 4, hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipMemcpyAsync(probs, h->d_probs.p, (size_t)R * h->cls->num_classes() * 4, hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  if (prof) { prof->collect(R); prof->enabled = false; }
  LP_API_END
}

}  // extern "C"
