// Focus views (lp_focus_*, lp_run_focus*; include/litepi.h "focus views"); the FocusPlan itself is in handle.h, owned by the
// handle's Tracker.  The host side of a call is constant per (B, frame sizes, slots): one whole-frame view and `slots` window
// placeholders per frame, laid out by the one view_layout, so the captured step replays; the plan kernel, enqueued in front of
// it outside the graph like the tracker's launch, rewrites the window table, the windows' view geometry and the empty-slot
// flags at their fixed device addresses.
#include <cmath>

#include "handle.h"

using namespace lp;

static lp_focus_config resolved(const lp_focus_config& c, int S) {
  lp_focus_config r = c;
  if (r.side_min == 0) r.side_min = S;
  if (r.side_max == 0) r.side_max = 2 * S;
  return r;
}

static void check_focus_config(const lp_focus_config* c, int S) {
  LP_CHECK(c, LP_ERR_ARG, "null focus configuration");
  LP_CHECK(S >= 16, LP_ERR_ARG, "det_input %d is below 16", S);
  const lp_focus_config r = resolved(*c, S);
  LP_CHECK(c->slots >= 1 && c->slots <= 16, LP_ERR_ARG, "slots %d outside 1..16", c->slots);
  LP_CHECK(c->side_min >= 0 && c->side_max >= 0 && r.side_min >= 16 && r.side_min <= r.side_max, LP_ERR_ARG,
           "side_min %d / side_max %d: need 16 <= side_min <= side_max", r.side_min, r.side_max);
  LP_CHECK(r.side_max <= 8 * S, LP_ERR_ARG, "side_max %d exceeds 8 x det_input = %d", r.side_max, 8 * S);
  LP_CHECK(c->margin >= 1.f && std::isfinite(c->margin), LP_ERR_ARG, "margin %g is below 1 or not finite", c->margin);
  LP_CHECK(c->small_px > 0.f, LP_ERR_ARG, "small_px %g is not positive", c->small_px);
  LP_CHECK(c->border >= 0, LP_ERR_ARG, "border %d is negative", c->border);
  LP_CHECK(c->sweep == 0 || c->sweep == 1, LP_ERR_ARG, "sweep %d is not 0 or 1", c->sweep);
  LP_CHECK(c->sweep_overlap >= 0 && c->sweep_overlap < r.side_min, LP_ERR_ARG, "sweep_overlap %d outside 0..%d", c->sweep_overlap,
           r.side_min - 1);
  for (int v : c->reserved) LP_CHECK(v == 0, LP_ERR_ARG, "a reserved word of lp_focus_config is not zero");
}

static FocusPlan& focus_of(lp_handle* h) {
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  LP_CHECK(h->trk->focus, LP_ERR_STATE, "no focus plan: call lp_focus_create first");
  return *h->trk->focus;
}

// ---- the device tables ---------------------------------------------------------------------------------------------------------
// While the plan kernel owns the window table and the windows' geometry, the handle's two host mirrors hold a mark no upload
// can equal: any other path re-uploads (and so invalidates the captured steps), and a focus call knows its tables are still
// in place when both marks stand and the placeholder layout is the one it uploaded.
static bool marked(const lp_handle* h) {
  return h->tile_cache.size() == 1 && h->tile_cache[0] == (char)0x7f && h->geom_cache.size() == 1 && h->geom_cache[0].h == -1;
}

static void mark(lp_handle* h) {
  h->tile_cache.assign(1, (char)0x7f);
  ImgGeom g;
  memset(&g, 0, sizeof(g));
  g.h = -1;
  h->geom_cache.assign(1, g);
}

// the call's layout: the whole frame, then `slots` windows of the largest down-scale (it sizes the gather's LDS rows)
static ViewLayout focus_layout(const lp_handle* h, const FocusPlan& p, const std::vector<ImgGeom>& fg) {
  FrameViews per(fg.size());
  for (size_t f = 0; f < fg.size(); ++f) {
    per[f].push_back(FrameView{VIEW_FULL, 0, 0, fg[f].w, fg[f].h});
    for (int k = 0; k < p.cfg.slots; ++k) per[f].push_back(FrameView{VIEW_WINDOW, 0, 0, p.cfg.side_max, p.cfg.side_max});
  }
  return view_layout(h, fg, per);
}

static void upload_focus_tables(lp_handle* h, FocusPlan& p, const std::vector<ImgGeom>& fg, const ViewLayout& lay) {
  const size_t nf = fg.size();
  std::vector<char> blob(nf * sizeof(ImgGeom) + lay.vslot.size() * sizeof(int));
  memcpy(blob.data(), fg.data(), nf * sizeof(ImgGeom));
  memcpy(blob.data() + nf * sizeof(ImgGeom), lay.vslot.data(), lay.vslot.size() * sizeof(int));
  const bool same_geom = p.vgeom.size() == lay.vgeom.size() && memcmp(p.vgeom.data(), lay.vgeom.data(), lay.vgeom.size() * sizeof(ImgGeom)) == 0;
  if (marked(h) && blob == p.blob && same_geom) return;
  h->tile_cache.clear();   // (a mark, or another call's blob that happens to equal this one's: upload in any case)
  h->geom_cache.clear();
  upload_tiles(h, fg, lay);   // synchronises and invalidates the captured steps
  p.blob.swap(blob);
  p.vgeom = lay.vgeom;
  mark(h);
}

// ---- the plan launch -----------------------------------------------------------------------------------------------------------
// ring slot: the tracker's plan (max_batch jobs, max_batch frame indices), then max_batch heights, widths and ratios
static void enqueue_focus_plan(lp_handle* h, int B, const int* hs, const int* ws, int H, int W, const int* stream_ids, int* dev_views,
                               bool tables, int advance, Profiler* prof) {
  Tracker& t = *h->trk;
  FocusPlan& p = *t.focus;
  const int mb = t.max_batch, S = h->cfg.det_input;
  const PlanRing::Slot rs = p.ring.acquire();
  int* slot = static_cast<int*>(rs.host);
  const int n_jobs = plan_stream_jobs(slot, mb, B, stream_ids);
  int* fh = slot + (size_t)mb * 5;
  int* fw = fh + mb;
  float* frf = reinterpret_cast<float*>(fw + mb);
  for (int b = 0; b < B; ++b) {
    fh[b] = hs ? hs[b] : H; fw[b] = ws ? ws[b] : W;
    frf[b] = make_geom(fh[b], fw[b], S, S, 0).ratio;
  }
  const int* dslot = static_cast<const int*>(rs.dev);
  p.ring.upload(rs, p.ring.slot_bytes, h->stream);
  FocusArgs a;
  memset(&a, 0, sizeof(a));
  a.jobs = reinterpret_cast<const TrackJob*>(dslot); a.frames = dslot + (size_t)mb * 4;
  a.fh = dslot + (size_t)mb * 5; a.fw = a.fh + mb; a.frf = reinterpret_cast<const float*>(a.fw + mb);
  a.table = t.table.as<TrackSlot>(); a.state = p.state.as<FocusState>(); a.views = dev_views;
  if (tables) {
    a.fgeom = h->d_fgeom.as<ImgGeom>(); a.vwin = h->d_vwin.as<ViewWin>(); a.geom = h->d_geom.as<ImgGeom>(); a.dead = p.d_dead.as<int>();
  }
  a.B = B; a.T = t.cfg.max_tracks; a.S = S; a.motion = t.cfg.motion; a.advance = advance;
  a.slots = p.cfg.slots; a.side_min = p.cfg.side_min; a.side_max = p.cfg.side_max; a.border = p.cfg.border; a.sweep = p.cfg.sweep;
  a.sweep_overlap = p.cfg.sweep_overlap; a.margin = p.cfg.margin; a.small_px = p.cfg.small_px;
  if (prof) prof->begin(h->stream);
  launch_focus_plan(a, n_jobs, h->stream);
  if (prof) prof->end(h->stream, "focus_plan", "focus_plan", 0.0, 0.0);
  p.ring.release(rs, h->stream);
}

// what both run calls check before anything is enqueued
static void check_focus_run(lp_handle* h, int B, const int* hs, const int* ws, int H, int W, const int* stream_ids) {
  const FocusPlan& p = focus_of(h);
  LP_CHECK((long)B * (1 + p.cfg.slots) <= h->cfg.max_batch, LP_ERR_ARG, "%d frames need %ld views (1 + %d slots each), more than max_batch = %d",
           B, (long)B * (1 + p.cfg.slots), p.cfg.slots, h->cfg.max_batch);
  check_stream_ids(*h->trk, B, stream_ids);
  for (int b = 0; b < B; ++b) {
    const int fh = hs ? hs[b] : H, fw = ws ? ws[b] : W;
    LP_CHECK(fh >= 16 && fw >= 16, LP_ERR_ARG, "frame %d is %dx%d: focus views need at least 16 pixels a side", b, fw, fh);
  }
}

extern "C" {

void lp_focus_default_config(lp_focus_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->slots = 3; c->side_min = 0; c->side_max = 0; c->margin = 2.f; c->small_px = 32.f; c->border = 16; c->sweep = 1; c->sweep_overlap = 0;
}

int lp_focus_config_check(const lp_focus_config* cfg, int det_input) {
  LP_API_BEGIN
  check_focus_config(cfg, det_input);
  LP_API_END
}

int lp_focus_destroy(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (h->trk && h->trk->focus) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));
    h->trk->focus.reset();
  }
  LP_API_END
}

int lp_focus_create(lp_handle* h, const lp_focus_config* cfg) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  check_square(h, "lp_focus_create");
  check_focus_config(cfg, h->cfg.det_input);
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  Tracker& t = *h->trk;
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));   // a replaced plan may still be in use
  std::unique_ptr<FocusPlan> p(new FocusPlan());
  p->cfg = resolved(*cfg, h->cfg.det_input);
  p->state.alloc((size_t)t.cfg.n_streams * sizeof(FocusState));
  p->d_views.alloc((size_t)t.max_batch * 16 * 4 * sizeof(int));
  p->d_dead.alloc((size_t)t.max_batch * sizeof(int));
  p->ring.create((size_t)t.max_batch * 8 * sizeof(int));
  t.focus = std::move(p);   // its first call uploads its tables: the steps captured under a replaced plan go with them
  LP_API_END
}

int lp_focus_plan(lp_handle* h, int B, const int* heights, const int* widths, const int* stream_ids, int* views, int advance) {
  LP_API_BEGIN
  check_square(h, "lp_focus_plan");
  FocusPlan& p = focus_of(h);
  const Tracker& t = *h->trk;
  LP_CHECK(heights && widths && views, LP_ERR_ARG, "null argument");
  LP_CHECK(B >= 1 && B <= t.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, t.max_batch);
  LP_CHECK(advance == 0 || advance == 1, LP_ERR_ARG, "advance %d is not 0 or 1", advance);
  check_stream_ids(t, B, stream_ids);
  for (int b = 0; b < B; ++b)
    LP_CHECK(heights[b] >= 16 && widths[b] >= 16, LP_ERR_ARG, "frame %d is %dx%d: focus views need at least 16 pixels a side", b, widths[b],
             heights[b]);
  LP_HIP(hipSetDevice(h->cfg.device));
  enqueue_focus_plan(h, B, heights, widths, 0, 0, stream_ids, p.d_views.as<int>(), false, advance, nullptr);
  LP_HIP(hipMemcpyAsync(views, p.d_views.p, (size_t)B * p.cfg.slots * 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

int lp_focus_state(lp_handle* h, int stream, int* cursor, int* unserved) {
  LP_API_BEGIN
  FocusPlan& p = focus_of(h);
  LP_CHECK(stream >= 0 && stream < h->trk->cfg.n_streams, LP_ERR_ARG, "stream %d outside 0..%d", stream, h->trk->cfg.n_streams - 1);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  FocusState s;
  LP_HIP(hipMemcpy(&s, p.state.as<FocusState>() + stream, sizeof(s), hipMemcpyDeviceToHost));
  if (cursor) *cursor = s.cursor;
  if (unserved) *unserved = s.unserved;
  LP_API_END
}

int lp_run_focus_device(lp_handle* h, const void* dev_imgs, int B, int H, int W, const int* stream_ids, float conf, float iou, int min_area,
                        void* dev_dets, void* dev_counts, void* dev_views) {
  LP_API_BEGIN
  check_square(h, "lp_run_focus_device");
  FocusPlan& p = focus_of(h);
  check_run_args(h, dev_imgs && dev_dets && dev_counts, B, false, min_area);
  check_focus_run(h, B, nullptr, nullptr, H, W, stream_ids);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg;
  CscPlan csc;
  const ViewLayout lay =
      device_view_frames(h, dev_imgs, B, H, W, [&](const std::vector<ImgGeom>& g) { return focus_layout(h, p, g); }, fg, csc);
  upload_focus_tables(h, p, fg, lay);
  const FrameSource frames = device_frames(h, dev_imgs, csc);
  run_device_pass(h, GK_FOCUS_DEVICE, B, conf, iou, min_area, dev_dets, dev_counts, frames,
                  view_front(h, frames.src, lay, B, conf, iou, p.d_dead.as<int>()), [&](Profiler* prof) {
                    enqueue_focus_plan(h, B, nullptr, nullptr, H, W, stream_ids, static_cast<int*>(dev_views), true, 1, prof);
                  });
  LP_API_END
}

int lp_run_focus(lp_handle* h, const uint8_t* const* imgs, const int* hs, const int* ws, int B, const int* stream_ids, float conf, float iou,
                 int min_area, lp_det* dets, int* counts, int* num_det, float* det_conf_avg, lp_timing* timing, int* views) {
  LP_API_BEGIN
  check_square(h, "lp_run_focus");
  FocusPlan& p = focus_of(h);
  check_run_args(h, imgs && hs && ws && dets && counts, B, true, min_area);
  check_focus_run(h, B, hs, ws, 0, 0, stream_ids);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg;
  CscPlan csc;
  const ViewLayout lay =
      upload_view_frames(h, imgs, hs, ws, B, [&](const std::vector<ImgGeom>& g) { return focus_layout(h, p, g); }, fg, csc);
  upload_focus_tables(h, p, fg, lay);
  // the plan launch stays outside the captured front (the staged pass's profile starts behind it: only lp_run_focus_device
  // books it); the windows are read back first, so that a ROI overflow reported by the pass still delivers them
  enqueue_focus_plan(h, B, hs, ws, 0, 0, stream_ids, p.d_views.as<int>(), true, 1, nullptr);
  if (views) {
    LP_HIP(hipMemcpyAsync(views, p.d_views.p, (size_t)B * p.cfg.slots * 4 * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    LP_HIP(hipStreamSynchronize(h->stream));   // the destination is the caller's pageable memory
  }
  run_host_pass(h, B, conf, iou, min_area, dets, counts, num_det, det_conf_avg, timing, csc, GK_FOCUS_FRONT,
                view_front(h, h->d_src.as<uint8_t>(), lay, B, conf, iou, p.d_dead.as<int>()));
  LP_API_END
}

}  // extern "C"
