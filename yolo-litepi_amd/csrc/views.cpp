// Scaled views (lp_view_grid, lp_view_geometry, lp_run_views*, lp_test_view_windows; include/litepi.h "scaled views"): any
// window of a frame, letterboxed into the detector batch at its own scale.  The view's ImgGeom carries the window as
// ratio / pad, so decode, frame NMS, ROI stage, tracker and inventory run as in tiled inference (tiling.cpp).
#include <cmath>

#include "handle.h"

namespace lp {

// one axis of the window grid (include/litepi.h lp_view_grid): origins and the common side
static int view_axis(int L, int tile, int overlap, std::vector<int>& xs) {
  xs.clear();
  if (L <= tile) { xs.push_back(0); return L; }
  const int step = tile - overlap, n = 1 + (L - tile + step - 1) / step;
  for (int k = 0; k < n; ++k) xs.push_back(std::min(k * step, L - tile));
  return tile;
}

// a view of an H x W frame as the window it covers; LP_ERR_ARG for a window the frame does not hold
static std::array<int, 4> view_window(const int* v, int H, int W, int index) {
  if (v[0] == -1) return {0, 0, W, H};
  LP_CHECK(v[0] >= 0 && v[1] >= 0 && v[2] >= 16 && v[3] >= 16, LP_ERR_ARG,
           "view %d: window {%d, %d, %d, %d} needs x, y >= 0 (x = -1: the whole frame) and w, h >= 16", index, v[0], v[1], v[2], v[3]);
  LP_CHECK((long)v[0] + v[2] <= W && (long)v[1] + v[3] <= H, LP_ERR_ARG, "view %d: window {%d, %d, %d, %d} passes the edge of a %dx%d frame",
           index, v[0], v[1], v[2], v[3], W, H);
  return {v[0], v[1], v[2], v[3]};
}

// geometry of the window {x, y, w, h} of a frame: make_geom of a h x w image, the pads moved by the window's origin
static ImgGeom window_geom(const ImgGeom& frame, const std::array<int, 4>& win, int S) {
  ImgGeom g = make_geom(win[3], win[2], S, frame.src_off);
  const double r = std::min((double)S / win[3], (double)S / win[2]);
  const double dw = (S - g.new_w) / 2.0, dh = (S - g.new_h) / 2.0;
  g.h = frame.h; g.w = frame.w;   // boxes are clipped to the frame, ROIs are cut from it
  g.pad_w = (float)(dw - r * win[0]);
  g.pad_h = (float)(dh - r * win[1]);
  return g;
}

ViewLayout view_layout(const lp_handle* h, const std::vector<ImgGeom>& fg, const int* views, int n_views) {
  const int S = h->cfg.det_input, F = (int)fg.size();
  LP_CHECK(views && n_views >= 1, LP_ERR_ARG, "a call needs at least one view (n_views = %d)", n_views);
  LP_CHECK((long)F * n_views <= h->cfg.max_batch, LP_ERR_ARG, "%d frames x %d views are more than max_batch = %d: split the call", F, n_views,
           h->cfg.max_batch);
  if (h->det && h->det->loaded()) {   // the frame NMS's LDS flag masks: checked here, before anything is enqueued
    const int A = h->det->num_anchors();
    LP_CHECK(n_views <= 1024 && frame_nms_lds_bytes(n_views * A) <= FRAME_NMS_LDS_CAP, LP_ERR_ARG,
             "a frame of %d views x %d anchors exceeds the frame NMS capacity (%d candidate slots per frame)", n_views, A,
             (int)((FRAME_NMS_LDS_CAP - 16) / 8 * 32));
  }
  int n_full = 0;
  for (int k = 0; k < n_views; ++k) n_full += views[4 * k] == -1;
  ViewLayout vl;
  TileLayout& lay = vl.lay;
  lay.L = F * n_full; lay.V = F * n_views; lay.max_views = n_views;
  lay.vgeom.resize(lay.V);
  vl.wins.resize(lay.V - lay.L);
  int next_lb = 0, next_win = lay.L;
  for (int f = 0; f < F; ++f) {
    lay.frames.push_back(TileFrame{(int)lay.vslot.size(), n_views});
    for (int k = 0; k < n_views; ++k) {
      const std::array<int, 4> win = view_window(views + 4 * k, fg[f].h, fg[f].w, k);
      const bool full = views[4 * k] == -1;
      const int slot = full ? next_lb++ : next_win++;
      lay.vgeom[slot] = full ? fg[f] : window_geom(fg[f], win, S);
      lay.vslot.push_back(slot);
      if (!full) {
        const ImgGeom& g = lay.vgeom[slot];
        ViewWin w;
        memset(&w, 0, sizeof(w));   // padding bytes too: the table is compared with memcmp
        w.src_off = fg[f].src_off; w.pitch = 3 * fg[f].w; w.frame_bytes = (long)fg[f].h * w.pitch;
        w.x = win[0]; w.y = win[1]; w.w = win[2]; w.h = win[3];
        w.new_w = g.new_w; w.new_h = g.new_h; w.top = g.top; w.left = g.left;
        vl.wins[slot - lay.L] = w;
      }
    }
  }
  return vl;
}

void enqueue_view_gather(const uint8_t* src, const ImgGeom* d_geom, const ViewWin* d_wins, uint8_t* dst, const ViewLayout& vl, int S,
                         hipStream_t st, Profiler* prof) {
  const TileLayout& lay = vl.lay;
  if (lay.L > 0) {
    if (prof) prof->begin(st);
    launch_letterbox(src, d_geom, dst, lay.L, S, st, lay.vgeom.data());
    if (prof) {
      double bytes = (double)lay.L * S * S * 3;
      for (int i = 0; i < lay.L; ++i) bytes += (double)lay.vgeom[i].h * lay.vgeom[i].w * 3;
      prof->end(st, "letterbox_u8", "letterbox", 0.0, bytes);
    }
  }
  if (lay.V > lay.L) {
    if (prof) prof->begin(st);
    launch_window_views(src, d_wins, dst, lay.L, lay.V - lay.L, S, st, vl.wins.data());
    if (prof) {   // booked like the letterbox: every window byte once, every view byte once
      double bytes = (double)(lay.V - lay.L) * S * S * 3;
      for (const ViewWin& w : vl.wins) bytes += (double)w.h * w.w * 3;
      prof->end(st, "window_views_u8", "view_gather", 0.0, bytes);
    }
  }
}

}  // namespace lp

using namespace lp;

extern "C" {

int lp_view_grid(int tile, int overlap, int full_frame, int H, int W, int* n_views, int* views, int cap) {
  LP_API_BEGIN
  LP_CHECK(n_views && H > 0 && W > 0, LP_ERR_ARG, "bad argument (frame %dx%d)", H, W);
  LP_CHECK(tile >= 16 && overlap >= 0 && overlap < tile, LP_ERR_ARG, "view grid needs tile >= 16 and 0 <= overlap < tile (tile %d, overlap %d)",
           tile, overlap);
  LP_CHECK(full_frame == 0 || full_frame == 1, LP_ERR_ARG, "full_frame must be 0 or 1 (got %d)", full_frame);
  std::vector<int> xs, ys;
  const int sw = view_axis(W, tile, overlap, xs), sh = view_axis(H, tile, overlap, ys);
  std::vector<std::array<int, 4>> v;
  if (xs.size() * ys.size() == 1 || full_frame) v.push_back({-1, -1, W, H});
  if (xs.size() * ys.size() > 1)
    for (int y : ys)
      for (int x : xs) v.push_back({x, y, sw, sh});
  *n_views = (int)v.size();
  if (views) {
    LP_CHECK(cap >= (int)v.size(), LP_ERR_ARG, "%zu views, room for %d", v.size(), cap);
    for (size_t i = 0; i < v.size(); ++i)
      for (int k = 0; k < 4; ++k) views[4 * i + k] = v[i][k];
  }
  LP_API_END
}

int lp_view_geometry(int det_input, int H, int W, const int* view, float* ratio, float* pad_w, float* pad_h, int* new_w, int* new_h,
                     int* top, int* left) {
  LP_API_BEGIN
  LP_CHECK(view && det_input >= 1 && H > 0 && W > 0, LP_ERR_ARG, "bad argument (det_input %d, frame %dx%d)", det_input, H, W);
  const ImgGeom frame = make_geom(H, W, det_input, 0);
  const ImgGeom g = window_geom(frame, view_window(view, H, W, 0), det_input);
  if (ratio) *ratio = g.ratio;
  if (pad_w) *pad_w = g.pad_w;
  if (pad_h) *pad_h = g.pad_h;
  if (new_w) *new_w = g.new_w;
  if (new_h) *new_h = g.new_h;
  if (top) *top = g.top;
  if (left) *left = g.left;
  LP_API_END
}

int lp_run_views(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const int* views, int n_views, float conf,
                 float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing) {
  LP_API_BEGIN
  LP_CHECK(h && imgs && hs && ws && dets && counts, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(h->cls && h->cls->loaded(), LP_ERR_STATE, "classifier not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_CHECK(min_area >= 0, LP_ERR_ARG, "min_area must be >= 0");
  for (int i = 0; i < B; ++i) LP_CHECK(hs[i] > 0 && ws[i] > 0, LP_ERR_ARG, "frame %d is empty", i);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg(B);
  for (int i = 0; i < B; ++i) fg[i] = make_geom(hs[i], ws[i], h->cfg.det_input, 0);
  (void)view_layout(h, fg, views, n_views);   // the list checked against every frame before anything is uploaded
  const bool nv = h->nv12();
  if (nv) {   // and the format, likewise (host frames: frame_stride does not apply)
    lp_frame_format hf = h->fmt;
    hf.frame_stride = 0;
    for (int i = 0; i < B; ++i) (void)frame_layout(hf, hs[i], ws[i]);
  }
  CscPlan csc;
  fg = upload_images(h, imgs, hs, ws, B, &csc);
  const ViewLayout vl = view_layout(h, fg, views, n_views);
  upload_tiles(h, fg, vl.lay, &vl.wins);
  run_host_pass(h, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, csc, GK_VIEWS_FRONT, GK_VIEWS_ROI, GK_VIEWS_CLS,
                [&](Profiler* prof) {
                  if (nv) enqueue_csc(h, h->d_raw.as<uint8_t>(), csc, prof);
                  enqueue_view_gather(h->d_src.as<uint8_t>(), h->d_geom.as<ImgGeom>(), h->d_vwin.as<ViewWin>(), h->d_lb.as<uint8_t>(), vl,
                                      h->cfg.det_input, h->stream, prof);
                  enqueue_view_detect(h, vl.lay, B, conf, iou, min_area, h->d_dets.as<lp_det>(), h->d_counts.as<int>(), true, prof);
                }, h->d_fgeom.as<ImgGeom>());
  LP_API_END
}

int lp_run_views_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* views, int n_views, float conf, float iou,
                        int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  LP_CHECK(h && dev_imgs && dev_dets && dev_counts, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch && H > 0 && W > 0, LP_ERR_ARG, "bad batch/shape");
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg(B);
  const bool nv = h->nv12();
  CscPlan csc;
  for (int i = 0; i < B; ++i) fg[i] = make_geom(H, W, h->cfg.det_input, (long)i * H * W * 3);
  (void)view_layout(h, fg, views, n_views);   // the list and the format checked before any buffer is sized
  if (nv) {
    (void)frame_layout(h->fmt, H, W);
    csc = device_csc(h, dev_imgs, B, H, W, fg);
  }
  const ViewLayout vl = view_layout(h, fg, views, n_views);
  upload_tiles(h, fg, vl.lay, &vl.wins);
  Profiler* prof = begin_profile(h);
  const uint8_t* src = nv ? h->d_src.as<uint8_t>() : static_cast<const uint8_t*>(dev_imgs);
  const bool classify = h->cls && h->cls->loaded();
  GraphKey key{GK_VIEWS_DEVICE, B, h->geom_ver, min_area, dev_imgs, dev_dets, dev_counts, conf, iou};
  key_format(h, csc, key);
  run_or_capture(h, key, prof == nullptr, [&]() {
    if (nv) enqueue_csc(h, static_cast<const uint8_t*>(dev_imgs), csc, prof);
    enqueue_view_gather(src, h->d_geom.as<ImgGeom>(), h->d_vwin.as<ViewWin>(), h->d_lb.as<uint8_t>(), vl, h->cfg.det_input, h->stream, prof);
    enqueue_view_detect(h, vl.lay, B, conf, iou, classify ? min_area : -1, static_cast<lp_det*>(dev_dets), static_cast<int*>(dev_counts),
                        classify, prof);
    if (classify) enqueue_classify(h, src, B, static_cast<lp_det*>(dev_dets), nullptr, nullptr, nullptr, prof, 0, h->d_fgeom.as<ImgGeom>());
  });
  if (prof) prof->enabled = false;  // records are collected by lp_profile_read after the caller synchronises
  LP_API_END
}

int lp_test_view_windows(lp_handle* h, const uint8_t* img, int H, int W, const int* views, int n_views, int byte_offset, uint8_t* out,
                         int cap) {
  LP_API_BEGIN
  LP_CHECK(h && img && out && H > 0 && W > 0 && byte_offset >= 0 && byte_offset < 64, LP_ERR_ARG, "bad argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  const int S = h->cfg.det_input;
  const size_t bytes = (size_t)H * W * 3;
  std::vector<ImgGeom> fg(1, make_geom(H, W, S, byte_offset));
  const ViewLayout vl = view_layout(h, fg, views, n_views);
  const TileLayout& lay = vl.lay;
  LP_CHECK(cap >= lay.V, LP_ERR_ARG, "%d views, room for %d", lay.V, cap);
  // the frame is the whole allocation but for the offset in front: nothing the gather may read lies beyond it
  DevBuf d_src, d_geom, d_wins, d_out;
  d_src.alloc(bytes + byte_offset);
  LP_HIP(hipMemcpy(d_src.as<uint8_t>() + byte_offset, img, bytes, hipMemcpyHostToDevice));
  d_geom.alloc((size_t)lay.V * sizeof(ImgGeom));
  LP_HIP(hipMemcpy(d_geom.p, lay.vgeom.data(), (size_t)lay.V * sizeof(ImgGeom), hipMemcpyHostToDevice));
  if (!vl.wins.empty()) {
    d_wins.alloc(vl.wins.size() * sizeof(ViewWin));
    LP_HIP(hipMemcpy(d_wins.p, vl.wins.data(), vl.wins.size() * sizeof(ViewWin), hipMemcpyHostToDevice));
  }
  d_out.alloc((size_t)lay.V * S * S * 3);
  enqueue_view_gather(d_src.as<uint8_t>(), d_geom.as<ImgGeom>(), d_wins.as<ViewWin>(), d_out.as<uint8_t>(), vl, S, h->stream, nullptr);
  LP_HIP(hipStreamSynchronize(h->stream));
  const size_t vb = (size_t)S * S * 3;
  for (int k = 0; k < lay.V; ++k)   // in the list's order
    LP_HIP(hipMemcpy(out + (size_t)k * vb, d_out.as<uint8_t>() + (size_t)lay.vslot[k] * vb, vb, hipMemcpyDeviceToHost));
  LP_API_END
}

}  // extern "C"
