// Frame views: tiled inference (lp_tile_grid, lp_run_tiled*), scaled views (lp_view_grid, lp_view_geometry, lp_run_views*) and
// mapped views (lp_run_mapped*; include/litepi.h "tiled inference", "scaled views", "mapped views").  A frame is seen through a
// list of views -- the letterboxed whole frame, native crops, windows letterboxed at their own scale, views through a remap
// table --; every view's ImgGeom carries its place in the frame as ratio / pad (a mapped view's candidates are carried to the
// frame by map_candidates in front of the view sort), so decode, frame NMS, ROI stage, tracker and inventory do not know which
// kind a view is.  One grid, one layout, one gather and one host / one device front serve the families: they differ in how a
// call's frames become view lists.
#include <cmath>

#include "handle.h"

namespace lp {

// ---- the view grid -------------------------------------------------------------------------------------------------------------
// one axis of a view grid: the origins of windows of side `tile` overlapping by `overlap` ({0} where one window covers the axis)
static std::vector<int> grid_axis(int L, int tile, int overlap) {
  if (L <= tile) return {0};
  const int step = tile - overlap, n = 1 + (L - tile + step - 1) / step;
  std::vector<int> xs(n);
  for (int k = 0; k < n; ++k) xs[k] = std::min(k * step, L - tile);
  return xs;
}

// The views of an H x W frame as {x, y, w, h}: {-1, -1, W, H}, the letterboxed whole frame, when full_frame or when one window
// covers the frame, then the ys x xs windows row-major.  clip: a window's side is the frame's where that is shorter than `tile`
// (lp_view_grid); otherwise every window is tile x tile and may pass the frame's edge (lp_tile_grid's crops).
static std::vector<std::array<int, 4>> grid_views(int H, int W, int tile, int overlap, int full_frame, bool clip) {
  const std::vector<int> xs = grid_axis(W, tile, overlap), ys = grid_axis(H, tile, overlap);
  const int sw = clip ? std::min(W, tile) : tile, sh = clip ? std::min(H, tile) : tile;
  std::vector<std::array<int, 4>> v;
  if (xs.size() * ys.size() == 1 || full_frame) v.push_back({-1, -1, W, H});
  if (xs.size() * ys.size() > 1)
    for (int y : ys)
      for (int x : xs) v.push_back({x, y, sw, sh});
  return v;
}

static void write_views(const std::vector<std::array<int, 4>>& v, int* n_views, int* views, int cap) {
  *n_views = (int)v.size();
  if (!views) return;
  LP_CHECK(cap >= (int)v.size(), LP_ERR_ARG, "%zu views, room for %d", v.size(), cap);
  for (size_t i = 0; i < v.size(); ++i)
    for (int k = 0; k < 4; ++k) views[4 * i + k] = v[i][k];
}

// the optional outputs of lp_view_geometry and lp_letterbox_geometry
static void write_geometry(const ImgGeom& g, float* ratio, float* pad_w, float* pad_h, int* new_w, int* new_h, int* top, int* left) {
  if (ratio) *ratio = g.ratio;
  if (pad_w) *pad_w = g.pad_w;
  if (pad_h) *pad_h = g.pad_h;
  if (new_w) *new_w = g.new_w;
  if (new_h) *new_h = g.new_h;
  if (top) *top = g.top;
  if (left) *left = g.left;
}

void check_tiling(const lp_tiling* t, int S) {
  LP_CHECK(t, LP_ERR_ARG, "null tiling");
  LP_CHECK(t->overlap >= 0 && t->overlap < S, LP_ERR_ARG, "tiling overlap %d outside 0..%d", t->overlap, S - 1);
  LP_CHECK(t->full_frame == 0 || t->full_frame == 1, LP_ERR_ARG, "tiling full_frame must be 0 or 1 (got %d)", t->full_frame);
}

// lp_view_merge_check's rule; NULL is an error here (lp_set_view_merge resolves it to the default first)
void check_view_merge(const lp_view_merge* m) {
  LP_CHECK(m, LP_ERR_ARG, "null view merge");
  LP_CHECK(m->metric == LP_MATCH_IOU || m->metric == LP_MATCH_IOS, LP_ERR_ARG, "view merge: unknown metric %d", m->metric);
  LP_CHECK(m->mode == LP_MERGE_SUPPRESS || m->mode == LP_MERGE_UNION, LP_ERR_ARG, "view merge: unknown mode %d", m->mode);
  LP_CHECK(m->threshold >= 0.f && m->threshold < 1.f, LP_ERR_ARG, "view merge: threshold %g outside [0, 1) (0 = the call's iou)",
           (double)m->threshold);   // NaN fails both comparisons
  for (int r : m->reserved) LP_CHECK(r == 0, LP_ERR_ARG, "view merge: non-zero reserved word");
}

// the handle's merge setting in a frame NMS launch: metric, mode and the threshold in place of the call's iou
void apply_view_merge(const lp_handle* h, float iou, FrameNmsArgs& a) {
  a.metric = h->vmerge.metric;
  a.mode = h->vmerge.mode;
  a.c.iou = h->vmerge.threshold > 0.f ? h->vmerge.threshold : iou;
}

// ---- a call's frames as view lists ---------------------------------------------------------------------------------------------
FrameViews tiled_views(int S, const lp_tiling& t, const std::vector<ImgGeom>& fg) {
  FrameViews per(fg.size());
  for (size_t f = 0; f < fg.size(); ++f)
    for (const auto& w : grid_views(fg[f].h, fg[f].w, S, t.overlap, t.full_frame, false))
      per[f].push_back(FrameView{w[0] < 0 ? VIEW_FULL : VIEW_CROP, w[0], w[1], w[2], w[3]});
  return per;
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

static void check_view_count(const lp_handle* h, int F, long V) {
  LP_CHECK(V <= h->cfg.max_batch, LP_ERR_ARG, "%d frames need %ld views, more than max_batch = %d: split the call", F, V, h->cfg.max_batch);
}

FrameViews listed_views(const lp_handle* h, const int* views, int n_views, const std::vector<ImgGeom>& fg) {
  LP_CHECK(views && n_views >= 1, LP_ERR_ARG, "a call needs at least one view (n_views = %d)", n_views);
  check_view_count(h, (int)fg.size(), (long)fg.size() * n_views);   // before a list of any length is copied once per frame
  FrameViews per(fg.size());
  for (size_t f = 0; f < fg.size(); ++f)
    for (int k = 0; k < n_views; ++k) {
      const std::array<int, 4> w = view_window(views + 4 * k, fg[f].h, fg[f].w, k);
      per[f].push_back(FrameView{views[4 * k] == -1 ? VIEW_FULL : VIEW_WINDOW, w[0], w[1], w[2], w[3]});
    }
  return per;
}

FrameViews mapped_views(const lp_handle* h, const int* views, int n_views, const int* maps, int n_maps, const std::vector<ImgGeom>& fg) {
  LP_CHECK(n_views >= 0 && n_maps >= 0 && (views || n_views == 0) && (maps || n_maps == 0) && n_views + (long)n_maps >= 1, LP_ERR_ARG,
           "a call needs at least one view or map (n_views = %d, n_maps = %d)", n_views, n_maps);
  check_view_count(h, (int)fg.size(), (long)fg.size() * ((long)n_views + n_maps));
  for (int k = 0; k < n_maps; ++k) {
    LP_CHECK(maps[k] >= 0 && maps[k] < (int)h->maps.size(), LP_ERR_ARG, "map %d: id %d is not a map of the handle (it holds %zu)", k, maps[k],
             h->maps.size());
    const lp_handle::MapEntry& m = *h->maps[maps[k]];
    for (size_t f = 0; f < fg.size(); ++f)
      LP_CHECK(fg[f].h == m.H && fg[f].w == m.W, LP_ERR_ARG, "map %d (id %d) belongs to %dx%d frames, frame %zu is %dx%d", k, maps[k], m.W, m.H,
               f, fg[f].w, fg[f].h);
  }
  FrameViews per = n_views ? listed_views(h, views, n_views, fg) : FrameViews(fg.size());
  for (auto& list : per)
    for (int k = 0; k < n_maps; ++k) list.push_back(FrameView{VIEW_MAPPED, maps[k], 0, 0, 0});
  return per;
}

// ---- the layout ----------------------------------------------------------------------------------------------------------------
// geometry of the window {x, y, w, h} of a frame: make_geom of a h x w image, the pads moved by the window's origin
static ImgGeom window_geom(const ImgGeom& frame, const std::array<int, 4>& win, int S) {
  ImgGeom g = make_geom(win[3], win[2], S, S, frame.src_off);
  const double r = std::min((double)S / win[3], (double)S / win[2]);
  const double dw = (S - g.new_w) / 2.0, dh = (S - g.new_h) / 2.0;
  g.h = frame.h; g.w = frame.w;   // boxes are clipped to the frame, ROIs are cut from it
  g.pad_w = (float)(dw - r * win[0]);
  g.pad_h = (float)(dh - r * win[1]);
  return g;
}

ViewLayout view_layout(const lp_handle* h, const std::vector<ImgGeom>& fg, const FrameViews& per) {
  const int S = h->cfg.det_input, F = (int)fg.size();
  ViewLayout lay;
  int count[4] = {0, 0, 0, 0};   // by ViewKind
  for (const auto& views : per) {
    for (const FrameView& v : views) ++count[v.kind];
    lay.max_views = std::max(lay.max_views, (int)views.size());
  }
  lay.L = count[VIEW_FULL]; lay.C = count[VIEW_CROP];
  lay.V = lay.L + lay.C + count[VIEW_WINDOW] + count[VIEW_MAPPED];
  check_view_count(h, F, lay.V);
  if (h->det && h->det->loaded()) {   // the frame NMS's LDS flag masks: checked here, before anything is enqueued
    const int A = h->det->num_anchors();
    LP_CHECK(lay.max_views <= 1024 && frame_nms_lds_bytes(lay.max_views * A) <= FRAME_NMS_LDS_CAP, LP_ERR_ARG,
             "a frame of %d views x %d anchors exceeds the frame NMS capacity (%d candidate slots per frame): use fewer views per "
             "frame (tiled: raise the overlap or lower the frame size)", lay.max_views, A, (int)((FRAME_NMS_LDS_CAP - 16) / 8 * 32));
  }
  lay.vgeom.resize(lay.V);
  lay.wins.resize(count[VIEW_WINDOW]);
  lay.maps.resize(count[VIEW_MAPPED]);
  const int first_map = lay.L + lay.C + count[VIEW_WINDOW];
  int next[4] = {0, lay.L, lay.L + lay.C, first_map};   // the first slot of every kind
  for (int f = 0; f < F; ++f) {
    lay.frames.push_back(TileFrame{(int)lay.vslot.size(), (int)per[f].size()});
    for (const FrameView& v : per[f]) {
      const int slot = next[v.kind]++;
      ImgGeom g = fg[f];   // letterbox geometry of the whole frame (make_geom)
      if (v.kind == VIEW_CROP) {
        g.new_w = S; g.new_h = S; g.top = -v.y; g.left = -v.x;
        g.ratio = 1.0f; g.pad_w = -(float)v.x; g.pad_h = -(float)v.y;
      } else if (v.kind == VIEW_WINDOW) {
        g = window_geom(fg[f], {v.x, v.y, v.w, v.h}, S);
        ViewWin w;
        memset(&w, 0, sizeof(w));   // padding bytes too: the table is compared with memcmp
        w.src_off = fg[f].src_off; w.pitch = 3 * fg[f].w; w.frame_bytes = (long)fg[f].h * w.pitch;
        w.x = v.x; w.y = v.y; w.w = v.w; w.h = v.h;
        w.new_w = g.new_w; w.new_h = g.new_h; w.top = g.top; w.left = g.left;
        lay.wins[slot - lay.L - lay.C] = w;
      } else if (v.kind == VIEW_MAPPED) {   // decoded as a crop of an S x S image; map_candidates carries the boxes to the frame
        g.h = S; g.w = S; g.new_w = S; g.new_h = S; g.top = 0; g.left = 0;
        g.ratio = 1.0f; g.pad_w = 0.f; g.pad_h = 0.f;
        MapSlot m;
        memset(&m, 0, sizeof(m));   // padding bytes too: the table is compared with memcmp
        m.fixed = h->maps[v.x]->fixed.as<int32_t>(); m.frame_off = fg[f].src_off; m.H = fg[f].h; m.W = fg[f].w;
        lay.maps[slot - first_map] = m;
        lay.map_src_bytes += h->maps[v.x]->foot_bytes;
      }
      lay.vgeom[slot] = g;
      lay.vslot.push_back(slot);
    }
  }
  return lay;
}

// upload the frame geometry, the frame table, the view slots, the view geometry, the window table and the map table when any of
// them changed; a change invalidates captured graphs (geom_ver)
void upload_tiles(lp_handle* h, const std::vector<ImgGeom>& fg, const ViewLayout& lay) {
  const int B = h->cfg.max_batch;
  if (!h->d_fgeom.p) {
    h->d_fgeom.alloc((size_t)B * sizeof(ImgGeom));
    h->d_ftab.alloc((size_t)B * (sizeof(TileFrame) + sizeof(int)));
    h->d_vcnt.alloc((size_t)B * 4);
  }
  const size_t nw = lay.wins.size();
  if (nw && !h->d_vwin.p) h->d_vwin.alloc((size_t)B * sizeof(ViewWin));
  const size_t nm = lay.maps.size();
  if (nm && !h->d_vmap.p) h->d_vmap.alloc((size_t)B * sizeof(MapSlot));
  h->upload_geom(lay.vgeom);
  const size_t nf = fg.size();
  std::vector<char> blob(nf * sizeof(ImgGeom) + nf * sizeof(TileFrame) + lay.vslot.size() * sizeof(int) + nw * sizeof(ViewWin) +
                         nm * sizeof(MapSlot));
  memcpy(blob.data(), fg.data(), nf * sizeof(ImgGeom));
  memcpy(blob.data() + nf * sizeof(ImgGeom), lay.frames.data(), nf * sizeof(TileFrame));
  memcpy(blob.data() + nf * (sizeof(ImgGeom) + sizeof(TileFrame)), lay.vslot.data(), lay.vslot.size() * sizeof(int));
  if (nw) memcpy(blob.data() + blob.size() - nm * sizeof(MapSlot) - nw * sizeof(ViewWin), lay.wins.data(), nw * sizeof(ViewWin));
  if (nm) memcpy(blob.data() + blob.size() - nm * sizeof(MapSlot), lay.maps.data(), nm * sizeof(MapSlot));
  if (blob == h->tile_cache) return;
  LP_HIP(hipMemcpyAsync(h->d_fgeom.p, fg.data(), nf * sizeof(ImgGeom), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_ftab.p, lay.frames.data(), nf * sizeof(TileFrame), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(h->d_ftab.as<char>() + (size_t)B * sizeof(TileFrame), lay.vslot.data(), lay.vslot.size() * sizeof(int),
                        hipMemcpyHostToDevice, h->stream));
  if (nw) LP_HIP(hipMemcpyAsync(h->d_vwin.p, lay.wins.data(), nw * sizeof(ViewWin), hipMemcpyHostToDevice, h->stream));
  if (nm) LP_HIP(hipMemcpyAsync(h->d_vmap.p, lay.maps.data(), nm * sizeof(MapSlot), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  h->tile_cache.swap(blob);
  ++h->geom_ver;
}

// ---- gather and detect ---------------------------------------------------------------------------------------------------------
void enqueue_view_gather(const uint8_t* src, const ImgGeom* d_geom, const ViewWin* d_wins, uint8_t* dst, const ViewLayout& lay, int S,
                         hipStream_t st, Profiler* prof, const MapSlot* d_maps) {
  const int nwin = (int)lay.wins.size(), nmap = (int)lay.maps.size();
  if (lay.L > 0) enqueue_letterbox(src, d_geom, dst, lay.vgeom.data(), lay.L, S, S, st, prof);
  if (lay.C > 0) {
    if (prof) prof->begin(st);
    launch_crop_views(src, d_geom, dst, lay.L, lay.C, S, st);
    if (prof) prof->end(st, "tile_crop_u8", "tile_crop", 0.0, 2.0 * lay.C * S * S * 3);
  }
  if (nwin > 0) {
    if (prof) prof->begin(st);
    launch_window_views(src, d_wins, dst, lay.L + lay.C, nwin, S, st, lay.wins.data());
    if (prof) {   // booked like the letterbox: every window byte once, every view byte once
      double bytes = (double)nwin * S * S * 3;
      for (const ViewWin& w : lay.wins) bytes += (double)w.h * w.w * 3;
      prof->end(st, "window_views_u8", "view_gather", 0.0, bytes);
    }
  }
  if (nmap > 0) {
    LP_CHECK(d_maps, LP_ERR_STATE, "mapped views without their table");
    if (prof) prof->begin(st);
    launch_map_views(src, d_maps, dst, lay.L + lay.C + nwin, nmap, S, st);
    // booked as the table once (8 bytes per view pixel), every view byte once, and the frame bytes the tables' positions span
    if (prof) prof->end(st, "map_views_u8", "view_gather", 0.0, (double)nmap * S * S * (8 + 3) + lay.map_src_bytes);
  }
}

// the detector on the gathered views + view sort + frame NMS (+ the ROI list when with_rois)
static void enqueue_view_detect(lp_handle* h, const ViewLayout& lay, int F, float conf, float iou, int min_area, lp_det* dets, int* counts,
                                bool with_rois, Profiler* prof, const int* dead) {
  h->det->forward(h->d_lb.as<uint8_t>(), lay.V, h->d_geom.as<ImgGeom>(), conf, nullptr, h->d_cand.as<Cand>(), h->d_cand_count.as<int>(),
                  h->stream, prof);
  if (dead) {   // focus views: an empty slot's view is all bars; whatever the detector made of it does not count
    if (prof) prof->begin(h->stream);
    launch_focus_mask(dead, h->d_cand_count.as<int>(), lay.V, h->stream);
    if (prof) prof->end(h->stream, "focus_mask", "nms", 0.0, 0.0);
  }
  if (!lay.maps.empty()) {   // mapped views: their candidates' boxes from view to frame coordinates, in front of the view sort
    if (prof) prof->begin(h->stream);
    launch_map_candidates(h->d_vmap.as<MapSlot>(), h->d_cand.as<Cand>(), h->d_cand_count.as<int>(), lay.V - (int)lay.maps.size(),
                          (int)lay.maps.size(), h->det->num_anchors(), h->cfg.det_input, h->stream);
    if (prof) prof->end(h->stream, "map_candidates", "nms", 0.0, 0.0);
  }
  FrameNmsArgs a;
  memset(&a, 0, sizeof(a));
  a.cand = h->d_cand.as<Cand>(); a.cand_count = h->d_cand_count.as<int>(); a.vcnt = h->d_vcnt.as<int>(); a.sorted = h->d_sorted.as<Cand>();
  a.frames = h->d_ftab.as<TileFrame>();
  a.vslot = reinterpret_cast<const int*>(h->d_ftab.as<char>() + (size_t)h->cfg.max_batch * sizeof(TileFrame));
  a.fgeom = h->d_fgeom.as<ImgGeom>();
  a.c = nms_common(h, dets, counts, h->d_rects.as<int>(), h->det->num_anchors(), h->det->num_classes(), h->cfg.max_det, iou, min_area, with_rois);
  apply_view_merge(h, iou, a);
  if (prof) prof->begin(h->stream);
  launch_view_sort(a, lay.V, h->stream);
  if (prof) prof->end(h->stream, "view_sort", "nms", 0.0, 0.0);
  if (prof) prof->begin(h->stream);
  launch_frame_nms(a, F, lay.max_views, h->stream);
  if (prof) prof->end(h->stream, "frame_nms", "nms", 0.0, 0.0);
}

// view gather + detector on the views + frame NMS (+ the ROI list when with_rois)
void enqueue_view_front(lp_handle* h, const uint8_t* src, const ViewLayout& lay, int F, float conf, float iou, int min_area, lp_det* dets,
                        int* counts, bool with_rois, Profiler* prof, const int* dead) {
  enqueue_view_gather(src, h->d_geom.as<ImgGeom>(), h->d_vwin.as<ViewWin>(), h->d_lb.as<uint8_t>(), lay, h->cfg.det_input, h->stream, prof,
                      h->d_vmap.as<MapSlot>());
  enqueue_view_detect(h, lay, F, conf, iou, min_area, dets, counts, with_rois, prof, dead);
}

Front view_front(lp_handle* h, const uint8_t* src, const ViewLayout& lay, int F, float conf, float iou, const int* dead) {
  Front f;
  f.run = [=, &lay](Profiler* prof, lp_det* dets, int* counts, int min_area, bool with_rois) {
    enqueue_view_front(h, src, lay, F, conf, iou, min_area, dets, counts, with_rois, prof, dead);
  };
  f.roi_geom = h->d_fgeom.as<ImgGeom>();
  return f;
}

// ---- a view call's frames ------------------------------------------------------------------------------------------------------
ViewLayout upload_view_frames(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const LayoutFn& layout_of,
                              std::vector<ImgGeom>& fg, CscPlan& csc) {
  fg.resize(B);
  for (int i = 0; i < B; ++i) fg[i] = make_geom(hs[i], ws[i], h->det_h(), h->det_w(), 0);
  (void)layout_of(fg);   // validates the call before anything is uploaded
  if (h->nv12()) {   // host frames: frame_stride does not apply
    lp_frame_format hf = h->fmt;
    hf.frame_stride = 0;
    for (int i = 0; i < B; ++i) (void)frame_layout(hf, hs[i], ws[i]);
  }
  fg = upload_images(h, imgs, hs, ws, B, &csc);
  return layout_of(fg);
}

ViewLayout device_view_frames(lp_handle* h, const void* dev_imgs, int B, int H, int W, const LayoutFn& layout_of, std::vector<ImgGeom>& fg,
                              CscPlan& csc) {
  fg.resize(B);
  for (int i = 0; i < B; ++i) fg[i] = make_geom(H, W, h->det_h(), h->det_w(), (long)i * H * W * 3);
  ViewLayout lay = layout_of(fg);
  if (h->nv12()) {
    csc = device_csc(h, dev_imgs, B, H, W, fg);
    lay = layout_of(fg);
  }
  return lay;
}

// ---- the two entries of lp_run_tiled* and lp_run_views* -------------------------------------------------------------------------
static void run_views_host(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, float conf, float iou, int min_area,
                           lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing, GraphKind front_kind,
                           const LayoutFn& layout_of) {
  check_run_args(h, imgs && hs && ws && dets && counts, B, true, min_area);
  for (int i = 0; i < B; ++i) LP_CHECK(hs[i] > 0 && ws[i] > 0, LP_ERR_ARG, "frame %d is empty", i);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg;
  CscPlan csc;
  const ViewLayout lay = upload_view_frames(h, imgs, hs, ws, B, layout_of, fg, csc);
  upload_tiles(h, fg, lay);
  run_host_pass(h, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, csc, front_kind,
                view_front(h, h->d_src.as<uint8_t>(), lay, B, conf, iou));
}

static void run_views_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, float conf, float iou, int min_area, void* dev_dets,
                             void* dev_counts, GraphKind kind, const LayoutFn& layout_of) {
  check_run_args(h, dev_imgs && dev_dets && dev_counts, B, false, min_area);
  LP_CHECK(H > 0 && W > 0, LP_ERR_ARG, "frames of %dx%d", W, H);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg;
  CscPlan csc;
  const ViewLayout lay = device_view_frames(h, dev_imgs, B, H, W, layout_of, fg, csc);
  upload_tiles(h, fg, lay);
  const FrameSource frames = device_frames(h, dev_imgs, csc);
  run_device_pass(h, kind, B, conf, iou, min_area, dev_dets, dev_counts, frames, view_front(h, frames.src, lay, B, conf, iou));
}

}  // namespace lp

using namespace lp;

extern "C" {

int lp_tile_grid(int det_input, const lp_tiling* tiling, int H, int W, int* n_views, int* views, int cap) {
  LP_API_BEGIN
  LP_CHECK(n_views && det_input >= 1 && H > 0 && W > 0, LP_ERR_ARG, "bad argument (det_input %d, frame %dx%d)", det_input, H, W);
  check_tiling(tiling, det_input);
  write_views(grid_views(H, W, det_input, tiling->overlap, tiling->full_frame, false), n_views, views, cap);
  LP_API_END
}

int lp_view_grid(int tile, int overlap, int full_frame, int H, int W, int* n_views, int* views, int cap) {
  LP_API_BEGIN
  LP_CHECK(n_views && H > 0 && W > 0, LP_ERR_ARG, "bad argument (frame %dx%d)", H, W);
  LP_CHECK(tile >= 16 && overlap >= 0 && overlap < tile, LP_ERR_ARG, "view grid needs tile >= 16 and 0 <= overlap < tile (tile %d, overlap %d)",
           tile, overlap);
  LP_CHECK(full_frame == 0 || full_frame == 1, LP_ERR_ARG, "full_frame must be 0 or 1 (got %d)", full_frame);
  write_views(grid_views(H, W, tile, overlap, full_frame, true), n_views, views, cap);
  LP_API_END
}

int lp_view_geometry(int det_input, int H, int W, const int* view, float* ratio, float* pad_w, float* pad_h, int* new_w, int* new_h,
                     int* top, int* left) {
  LP_API_BEGIN
  LP_CHECK(view && det_input >= 1 && H > 0 && W > 0, LP_ERR_ARG, "bad argument (det_input %d, frame %dx%d)", det_input, H, W);
  const ImgGeom frame = make_geom(H, W, det_input, det_input, 0);
  const ImgGeom g = window_geom(frame, view_window(view, H, W, 0), det_input);
  write_geometry(g, ratio, pad_w, pad_h, new_w, new_h, top, left);
  LP_API_END
}

// the reference's letterbox(img, (det_h, det_w)) in Python doubles (e2e.py:72-83): make_geom itself, what a handle of that input uses
int lp_letterbox_geometry(int det_h, int det_w, int H, int W, float* ratio, float* pad_w, float* pad_h, int* new_w, int* new_h, int* top,
                          int* left) {
  LP_API_BEGIN
  LP_CHECK(det_h > 0 && det_w > 0 && H > 0 && W > 0, LP_ERR_ARG, "bad argument (detector input %dx%d, image %dx%d; rows x columns)", det_h, det_w, H, W);
  const ImgGeom g = make_geom(H, W, det_h, det_w, 0);
  write_geometry(g, ratio, pad_w, pad_h, new_w, new_h, top, left);
  LP_API_END
}

void lp_view_merge_default(lp_view_merge* cfg) {
  if (cfg) memset(cfg, 0, sizeof(*cfg));   // LP_MATCH_IOU, LP_MERGE_SUPPRESS, the call's iou
}

int lp_run_mapped(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const int* views, int n_views, const int* maps,
                  int n_maps, float conf, float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg,
                  lp_timing* timing) {
  LP_API_BEGIN
  check_square(h, "lp_run_mapped");
  run_views_host(h, imgs, hs, ws, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, GK_VIEWS_FRONT,
                 [&](const std::vector<ImgGeom>& fg) { return view_layout(h, fg, mapped_views(h, views, n_views, maps, n_maps, fg)); });
  LP_API_END
}

int lp_run_mapped_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* views, int n_views, const int* maps, int n_maps,
                         float conf, float iou, int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  check_square(h, "lp_run_mapped_device");
  run_views_device(h, dev_imgs, B, H, W, conf, iou, min_area, dev_dets, dev_counts, GK_VIEWS_DEVICE,
                   [&](const std::vector<ImgGeom>& fg) { return view_layout(h, fg, mapped_views(h, views, n_views, maps, n_maps, fg)); });
  LP_API_END
}

int lp_view_merge_check(const lp_view_merge* cfg) {
  LP_API_BEGIN
  check_view_merge(cfg);
  LP_API_END
}

int lp_set_view_merge(lp_handle* h, const lp_view_merge* cfg) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (cfg) check_view_merge(cfg);
  const lp_view_merge def = {};
  const lp_view_merge next = cfg ? *cfg : def;
  if (memcmp(&next, &h->vmerge, sizeof(next)) != 0) {
    h->vmerge = next;
    ++h->geom_ver;   // captured steps of the view families hold the old instantiation and threshold
  }
  LP_API_END
}

int lp_run_tiled(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const lp_tiling* tiling, float conf,
                 float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing) {
  LP_API_BEGIN
  check_square(h, "lp_run_tiled");
  run_views_host(h, imgs, hs, ws, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, GK_TILED_FRONT,
                 [&](const std::vector<ImgGeom>& fg) {
                   check_tiling(tiling, h->cfg.det_input);
                   return view_layout(h, fg, tiled_views(h->cfg.det_input, *tiling, fg));
                 });
  LP_API_END
}

int lp_run_tiled_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const lp_tiling* tiling, float conf, float iou,
                        int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  check_square(h, "lp_run_tiled_device");
  run_views_device(h, dev_imgs, B, H, W, conf, iou, min_area, dev_dets, dev_counts, GK_TILED_DEVICE, [&](const std::vector<ImgGeom>& fg) {
    check_tiling(tiling, h->cfg.det_input);
    return view_layout(h, fg, tiled_views(h->cfg.det_input, *tiling, fg));
  });
  LP_API_END
}

int lp_run_views(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const int* views, int n_views, float conf,
                 float iou, int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing) {
  LP_API_BEGIN
  check_square(h, "lp_run_views");
  run_views_host(h, imgs, hs, ws, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, GK_VIEWS_FRONT,
                 [&](const std::vector<ImgGeom>& fg) { return view_layout(h, fg, listed_views(h, views, n_views, fg)); });
  LP_API_END
}

int lp_run_views_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* views, int n_views, float conf, float iou,
                        int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  check_square(h, "lp_run_views_device");
  run_views_device(h, dev_imgs, B, H, W, conf, iou, min_area, dev_dets, dev_counts, GK_VIEWS_DEVICE,
                   [&](const std::vector<ImgGeom>& fg) { return view_layout(h, fg, listed_views(h, views, n_views, fg)); });
  LP_API_END
}

}  // extern "C"
