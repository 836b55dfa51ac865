// Tiled inference (lp_tile_grid, lp_run_tiled*): the view grid of a frame, the call's view layout and the tiled front.
#include "handle.h"

namespace lp {

// one axis of the view grid (include/litepi.h lp_tile_grid)
static int tile_axis(int L, int S, int overlap, std::vector<int>& xs) {
  xs.clear();
  if (L <= S) { xs.push_back(0); return 1; }
  const int step = S - overlap, n = 1 + (L - S + step - 1) / step;
  for (int k = 0; k < n; ++k) xs.push_back(std::min(k * step, L - S));
  return n;
}

void check_tiling(const lp_tiling* t, int S) {
  LP_CHECK(t, LP_ERR_ARG, "null tiling");
  LP_CHECK(t->overlap >= 0 && t->overlap < S, LP_ERR_ARG, "tiling overlap %d outside 0..%d", t->overlap, S - 1);
  LP_CHECK(t->full_frame == 0 || t->full_frame == 1, LP_ERR_ARG, "tiling full_frame must be 0 or 1 (got %d)", t->full_frame);
}

// views of one H x W frame as {x, y, w, h} windows; x = -1 marks the letterboxed whole frame
static std::vector<std::array<int, 4>> tile_views(int S, const lp_tiling& t, int H, int W) {
  std::vector<int> xs, ys;
  const int nx = tile_axis(W, S, t.overlap, xs), ny = tile_axis(H, S, t.overlap, ys);
  std::vector<std::array<int, 4>> v;
  if (nx * ny == 1 || t.full_frame) v.push_back({-1, -1, W, H});
  if (nx * ny > 1)
    for (int y : ys)
      for (int x : xs) v.push_back({x, y, S, S});
  return v;
}

TileLayout tile_layout(const lp_handle* h, const std::vector<ImgGeom>& fg, const lp_tiling& t) {
  const int S = h->cfg.det_input, F = (int)fg.size();
  std::vector<std::vector<std::array<int, 4>>> per(F);
  TileLayout lay;
  int ncrop = 0;
  for (int f = 0; f < F; ++f) {
    per[f] = tile_views(S, t, fg[f].h, fg[f].w);
    for (auto& w : per[f]) (w[0] < 0 ? lay.L : ncrop) += 1;
    lay.max_views = std::max(lay.max_views, (int)per[f].size());
  }
  lay.V = lay.L + ncrop;
  LP_CHECK(lay.V <= h->cfg.max_batch, LP_ERR_ARG, "%d frames need %d views, more than max_batch = %d: split the call", F, lay.V,
           h->cfg.max_batch);
  if (h->det && h->det->loaded()) {   // the frame NMS's LDS flag masks: checked here, before anything is enqueued
    const int A = h->det->num_anchors();
    LP_CHECK(lay.max_views <= 1024 && frame_nms_lds_bytes(lay.max_views * A) <= FRAME_NMS_LDS_CAP, LP_ERR_ARG,
             "a frame of %d views x %d anchors exceeds the frame NMS capacity (%d candidate slots per frame): raise the overlap "
             "or lower the frame size", lay.max_views, A, (int)((FRAME_NMS_LDS_CAP - 16) / 8 * 32));
  }
  lay.vgeom.resize(lay.V);
  int next_lb = 0, next_crop = lay.L;
  for (int f = 0; f < F; ++f) {
    lay.frames.push_back(TileFrame{(int)lay.vslot.size(), (int)per[f].size()});
    for (auto& w : per[f]) {
      const int slot = w[0] < 0 ? next_lb++ : next_crop++;
      ImgGeom g = fg[f];   // letterbox geometry of the whole frame (make_geom)
      if (w[0] >= 0) {
        g.new_w = S; g.new_h = S; g.top = -w[1]; g.left = -w[0];
        g.ratio = 1.0f; g.pad_w = -(float)w[0]; g.pad_h = -(float)w[1];
      }
      lay.vgeom[slot] = g;
      lay.vslot.push_back(slot);
    }
  }
  return lay;
}

// upload the frame geometry + frame table + view slots (+ the window table of scaled views) when they changed; a change
// invalidates captured graphs (geom_ver)
void upload_tiles(lp_handle* h, const std::vector<ImgGeom>& fg, const TileLayout& lay, const std::vector<ViewWin>* wins) {
  const int B = h->cfg.max_batch;
  if (!h->d_fgeom.p) {
    h->d_fgeom.alloc((size_t)B * sizeof(ImgGeom));
    h->d_ftab.alloc((size_t)B * (sizeof(TileFrame) + sizeof(int)));
    h->d_vcnt.alloc((size_t)B * 4);
  }
  const size_t nw = wins ? wins->size() : 0;
  if (nw && !h->d_vwin.p) h->d_vwin.alloc((size_t)B * sizeof(ViewWin));
  h->upload_geom(lay.vgeom);
  const size_t nf = fg.size();
  std::vector<char> blob(nf * sizeof(ImgGeom) + nf * sizeof(TileFrame) + lay.vslot.size() * sizeof(int) + nw * sizeof(ViewWin));
  memcpy(blob.data(), fg.data(), nf * sizeof(ImgGeom));
  memcpy(blob.data() + nf * sizeof(ImgGeom), lay.frames.data(), nf * sizeof(TileFrame));
  memcpy(blob.data() + nf * (sizeof(ImgGeom) + sizeof(TileFrame)), lay.vslot.data(), lay.vslot.size() * sizeof(int));
  if (nw) memcpy(blob.data() + blob.size() - nw * sizeof(ViewWin), wins->data(), nw * sizeof(ViewWin));
  if (blob == h->tile_cache) return;
  LP_HIP(hipMemcpyAsync(h->d_fgeom.p, fg.data(), nf * sizeof(ImgGeom), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_ftab.p, lay.frames.data(), nf * sizeof(TileFrame), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_ftab.as<char>() + (size_t)B * sizeof(TileFrame), lay.vslot.data(), lay.vslot.size() * sizeof(int),
                        hipMemcpyHostToDevice, h->stream));
  if (nw) LP_HIP(hipMemcpyAsync(h->d_vwin.p, wins->data(), nw * sizeof(ViewWin), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  h->tile_cache.swap(blob);
  ++h->geom_ver;
}

// the detector on the gathered views + view sort + frame NMS (+ the ROI list when with_rois)
void enqueue_view_detect(lp_handle* h, const TileLayout& lay, int F, float conf, float iou, int min_area, lp_det* dets, int* counts,
                         bool with_rois, Profiler* prof) {
  h->det->forward(h->d_lb.as<uint8_t>(), lay.V, h->d_geom.as<ImgGeom>(), conf, nullptr, h->d_cand.as<Cand>(), h->d_cand_count.as<int>(),
                  h->stream, prof);
  FrameNmsArgs a;
  memset(&a, 0, sizeof(a));
  a.cand = h->d_cand.as<Cand>(); a.cand_count = h->d_cand_count.as<int>(); a.vcnt = h->d_vcnt.as<int>(); a.sorted = h->d_sorted.as<Cand>();
  a.frames = h->d_ftab.as<TileFrame>();
  a.vslot = reinterpret_cast<const int*>(h->d_ftab.as<char>() + (size_t)h->cfg.max_batch * sizeof(TileFrame));
  a.dets = dets; a.counts = counts; a.rects = h->d_rects.as<int>(); a.fgeom = h->d_fgeom.as<ImgGeom>();
  a.A = h->det->num_anchors(); a.max_det = h->cfg.max_det; a.nc = h->det->num_classes(); a.iou = iou; a.min_area = min_area;
  if (with_rois) a.tab = h->roi_table();
  a.max_rois = h->max_rois;
  a.roi_rule = h->cfg.numerics;
  if (prof) prof->begin(h->stream);
  launch_view_sort(a, lay.V, h->stream);
  if (prof) prof->end(h->stream, "view_sort", "nms", 0.0, 0.0);
  if (prof) prof->begin(h->stream);
  launch_frame_nms(a, F, lay.max_views, h->stream);
  if (prof) prof->end(h->stream, "frame_nms", "nms", 0.0, 0.0);
}

// view gather + detector on the views + frame NMS (+ the ROI list when with_rois)
static void enqueue_tiled_detect(lp_handle* h, const uint8_t* src, const TileLayout& lay, int F, float conf, float iou, int min_area, lp_det* dets,
                          int* counts, bool with_rois, Profiler* prof) {
  const int S = h->cfg.det_input;
  if (lay.L > 0) {
    if (prof) prof->begin(h->stream);
    launch_letterbox(src, h->d_geom.as<ImgGeom>(), h->d_lb.as<uint8_t>(), lay.L, S, h->stream, lay.vgeom.data());
    if (prof) {
      double bytes = (double)lay.L * S * S * 3;
      for (int i = 0; i < lay.L; ++i) bytes += (double)lay.vgeom[i].h * lay.vgeom[i].w * 3;
      prof->end(h->stream, "letterbox_u8", "letterbox", 0.0, bytes);
    }
  }
  if (lay.V > lay.L) {
    if (prof) prof->begin(h->stream);
    launch_crop_views(src, h->d_geom.as<ImgGeom>(), h->d_lb.as<uint8_t>(), lay.L, lay.V - lay.L, S, h->stream);
    if (prof) prof->end(h->stream, "tile_crop_u8", "tile_crop", 0.0, 2.0 * (lay.V - lay.L) * S * S * 3);
  }
  enqueue_view_detect(h, lay, F, conf, iou, min_area, dets, counts, with_rois, prof);
}

}  // namespace lp

using namespace lp;

extern "C" {

int lp_tile_grid(int det_input, const lp_tiling* tiling, int H, int W, int* n_views, int* views, int cap) {
  LP_API_BEGIN
  LP_CHECK(n_views && det_input >= 1 && H > 0 && W > 0, LP_ERR_ARG, "bad argument (det_input %d, frame %dx%d)", det_input, H, W);
  check_tiling(tiling, det_input);
  const auto v = tile_views(det_input, *tiling, H, W);
  *n_views = (int)v.size();
  if (views) {
    LP_CHECK(cap >= (int)v.size(), LP_ERR_ARG, "%zu views, room for %d", v.size(), cap);
    for (size_t i = 0; i < v.size(); ++i)
      for (int k = 0; k < 4; ++k) views[4 * i + k] = v[i][k];
  }
  LP_API_END
}

int lp_run_tiled(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const lp_tiling* tiling, float conf,
                 float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing) {
  LP_API_BEGIN
  LP_CHECK(h && imgs && hs && ws && dets && counts, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(h->cls && h->cls->loaded(), LP_ERR_STATE, "classifier not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_CHECK(min_area >= 0, LP_ERR_ARG, "min_area must be >= 0");
  check_tiling(tiling, h->cfg.det_input);
  for (int i = 0; i < B; ++i) LP_CHECK(hs[i] > 0 && ws[i] > 0, LP_ERR_ARG, "frame %d is empty", i);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg(B);
  for (int i = 0; i < B; ++i) fg[i] = make_geom(hs[i], ws[i], h->cfg.det_input, 0);
  (void)tile_layout(h, fg, *tiling);   // view count checked before anything is uploaded
  const bool nv = h->nv12();
  if (nv) {   // and the format, likewise (host frames: frame_stride does not apply)
    lp_frame_format hf = h->fmt;
    hf.frame_stride = 0;
    for (int i = 0; i < B; ++i) (void)frame_layout(hf, hs[i], ws[i]);
  }
  CscPlan csc;
  fg = upload_images(h, imgs, hs, ws, B, &csc);
  const TileLayout lay = tile_layout(h, fg, *tiling);
  upload_tiles(h, fg, lay);
  run_host_pass(h, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, csc, GK_TILED_FRONT, GK_TILED_ROI, GK_TILED_CLS,
                [&](Profiler* prof) {
                  if (nv) enqueue_csc(h, h->d_raw.as<uint8_t>(), csc, prof);
                  enqueue_tiled_detect(h, h->d_src.as<uint8_t>(), lay, B, conf, iou, min_area, h->d_dets.as<lp_det>(), h->d_counts.as<int>(),
                                       true, prof);
                }, h->d_fgeom.as<ImgGeom>());
  LP_API_END
}

int lp_run_tiled_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const lp_tiling* tiling, float conf, float iou,
                        int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  LP_CHECK(h && dev_imgs && dev_dets && dev_counts, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch && H > 0 && W > 0, LP_ERR_ARG, "bad batch/shape");
  check_tiling(tiling, h->cfg.det_input);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg(B);
  const bool nv = h->nv12();
  CscPlan csc;
  for (int i = 0; i < B; ++i) fg[i] = make_geom(H, W, h->cfg.det_input, (long)i * H * W * 3);
  if (nv) {
    (void)frame_layout(h->fmt, H, W);
    (void)tile_layout(h, fg, *tiling);   // format and view count checked before any buffer is sized
    csc = device_csc(h, dev_imgs, B, H, W, fg);
  }
  const TileLayout lay = tile_layout(h, fg, *tiling);
  upload_tiles(h, fg, lay);
  Profiler* prof = begin_profile(h);
  const uint8_t* src = nv ? h->d_src.as<uint8_t>() : static_cast<const uint8_t*>(dev_imgs);
  const bool classify = h->cls && h->cls->loaded();
  GraphKey key{GK_TILED_DEVICE, B, h->geom_ver, min_area, dev_imgs, dev_dets, dev_counts, conf, iou};
  key_format(h, csc, key);
  run_or_capture(h, key, prof == nullptr, [&]() {
    if (nv) enqueue_csc(h, static_cast<const uint8_t*>(dev_imgs), csc, prof);
    enqueue_tiled_detect(h, src, lay, B, conf, iou, classify ? min_area : -1, static_cast<lp_det*>(dev_dets), static_cast<int*>(dev_counts),
                         classify, prof);
    if (classify) enqueue_classify(h, src, B, static_cast<lp_det*>(dev_dets), nullptr, nullptr, nullptr, prof, 0, h->d_fgeom.as<ImgGeom>());
  });
  if (prof) prof->enabled = false;  // records are collected by lp_profile_read after the caller synchronises
  LP_API_END
}

}  // extern "C"
