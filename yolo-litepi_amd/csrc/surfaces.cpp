// Decoder surfaces in place (include/litepi.h lp_surface): the staging of a call's table through the handle's plan
// ring (handle.h: PlanRing, one device table), the two entry points and the converter's test hook.  The argument rules and the
// table's records are surface_plan.h.
// A surface's addresses and pitches reach the converter through one device table at a fixed address, rewritten in stream order
// in front of every step: they are data, not part of a captured step's identity, so surfaces that rotate through a decoder
// pool replay one step and never synchronise the host.
#include "handle.h"

namespace lp {

namespace {

// one call's conversion: what the step's first launch needs besides the table
struct SurfPlan {
  int B = 0, max_blocks = 0, matrix = 0;
  bool p010 = false;
  double bytes = 0.0;   // booked traffic: every sample byte once, every BGR byte once
};

// The call's records into the next pinned slot and from there to the device table, on the handle's stream in front of the
// step.  Called after every check and after ensure_src: the destination address is final.
SurfPlan stage_surfaces(lp_handle* h, const lp_surface_format& fmt, const lp_surface* s, int B, const std::vector<ImgGeom>& g) {
  if (!h->surf) {
    std::unique_ptr<PlanRing> ring(new PlanRing);
    ring->create((size_t)h->cfg.max_batch * sizeof(SurfFrame), 1);
    h->surf = std::move(ring);
  }
  PlanRing& r = *h->surf;
  const PlanRing::Slot slot = r.acquire();   // waits only once the ring has wrapped: the copy that read the slot has long gone
  SurfFrame* rec = static_cast<SurfFrame*>(slot.host);
  std::vector<long> off(B);
  SurfPlan p;
  p.B = B; p.matrix = fmt.matrix; p.p010 = fmt.pixfmt == LP_SURF_P010;
  for (int i = 0; i < B; ++i) {
    off[i] = g[i].src_off;
    p.bytes += (double)s[i].height * s[i].width * (1.5 * surface_sample_bytes(fmt.pixfmt) + 3.0);
  }
  p.max_blocks = fill_surface_table(fmt, s, B, h->d_src.p, off.data(), rec);
  r.upload(slot, (size_t)B * sizeof(SurfFrame), h->stream);
  r.release(slot, h->stream);
  return p;
}

void enqueue_surfaces(lp_handle* h, const SurfPlan& p, Profiler* prof) {
  if (prof) prof->begin(h->stream);
  launch_surfaces_to_bgr(h->surf->dev.as<SurfFrame>(), h->d_src.as<uint8_t>(), p.B, p.max_blocks, p.p010, p.matrix, h->stream);
  if (prof) prof->end(h->stream, p.p010 ? "surfaces_to_bgr_p010" : "surfaces_to_bgr", "csc", 0.0, p.bytes);
}

// the converted frames' geometry: make_geom offsets, 16-byte aligned like the host path's; returns the bytes of d_src they need
size_t surface_geometry(const lp_handle* h, const lp_surface* s, int B, std::vector<ImgGeom>& g) {
  size_t total = 0;
  for (int i = 0; i < B; ++i) {
    g[i] = make_geom(s[i].height, s[i].width, h->det_h(), h->det_w(), (long)total);
    total = align16(total + (size_t)s[i].height * s[i].width * 3);
  }
  return total;
}

// the staged surfaces as a frame source: converted into d_src by the step's first launch.  Its key fields hold no surface
// address, pitch or table generation (p0 stays null): the table's content is data.  Sizes are in geom_ver (upload_geom), the
// destination's address too (ensure_src).
FrameSource surface_frames(lp_handle* h, const lp_surface_format& fmt, const SurfPlan& plan) {
  FrameSource f;
  f.src = h->d_src.as<uint8_t>();
  f.convert = [=](Profiler* prof) { enqueue_surfaces(h, plan, prof); };
  f.key.pixfmt = fmt.pixfmt; f.key.matrix = fmt.matrix;
  return f;
}

}  // namespace
}  // namespace lp

using namespace lp;

extern "C" {

int lp_surfaces_check(const lp_surface_format* fmt, const lp_surface* s, int B) {
  LP_API_BEGIN
  check_surfaces(fmt, s, B, false);
  LP_API_END
}

int lp_run_surfaces_device(lp_handle* h, const lp_surface_format* fmt, const lp_surface* surfaces, int B, float conf, float iou,
                           int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  check_run_args(h, fmt && surfaces && dev_dets && dev_counts, B, false, min_area);
  check_surfaces(fmt, surfaces, B, false);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> g(B);
  h->ensure_src(surface_geometry(h, surfaces, B, g));
  h->upload_geom(g);
  const FrameSource frames = surface_frames(h, *fmt, stage_surfaces(h, *fmt, surfaces, B, g));
  run_device_pass(h, GK_SURFACES_DEVICE, B, conf, iou, min_area, dev_dets, dev_counts, frames, plain_front(h, frames.src, g, B, conf, iou));
  LP_API_END
}

int lp_run_views_surfaces_device(lp_handle* h, const lp_surface_format* fmt, const lp_surface* surfaces, int B, const int* views,
                                 int n_views, float conf, float iou, int min_area, void* dev_dets, void* dev_counts) {
  LP_API_BEGIN
  check_square(h, "lp_run_views_surfaces_device");
  check_run_args(h, fmt && surfaces && dev_dets && dev_counts, B, false, min_area);
  check_surfaces(fmt, surfaces, B, true);
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<ImgGeom> fg(B);
  const size_t total = surface_geometry(h, surfaces, B, fg);
  const ViewLayout lay = view_layout(h, fg, listed_views(h, views, n_views, fg));   // validated before anything is sized or enqueued
  h->ensure_src(total);
  upload_tiles(h, fg, lay);
  const FrameSource frames = surface_frames(h, *fmt, stage_surfaces(h, *fmt, surfaces, B, fg));
  run_device_pass(h, GK_VIEWS_SURFACES_DEVICE, B, conf, iou, min_area, dev_dets, dev_counts, frames,
                  view_front(h, frames.src, lay, B, conf, iou));
  LP_API_END
}

int lp_test_convert_surfaces(lp_handle* h, const lp_surface_format* fmt, const lp_surface* surfaces, int B, uint8_t* out_bgr) {
  LP_API_BEGIN
  LP_CHECK(h && out_bgr, LP_ERR_ARG, "null argument");
  check_surfaces(fmt, surfaces, B, false);
  LP_HIP(hipSetDevice(h->cfg.device));
  // the output sits between two guard zones, and its frames at 16-byte aligned offsets as in d_src; every byte the
  // converter does not own (guards, the gaps between frames) must still hold the fill pattern afterwards
  const size_t guard = 256;
  std::vector<long> off(B);
  std::vector<size_t> fb(B);
  size_t total = 0;
  for (int i = 0; i < B; ++i) {
    off[i] = (long)(guard + total);
    fb[i] = (size_t)surfaces[i].height * surfaces[i].width * 3;
    total = align16(total + fb[i]);
  }
  DevBuf d_tab, d_out;
  d_out.alloc(2 * guard + total, false);
  LP_HIP(hipMemset(d_out.p, 0xA5, d_out.bytes));
  LP_HIP(hipDeviceSynchronize());
  std::vector<SurfFrame> tab(B);
  const int max_blocks = fill_surface_table(*fmt, surfaces, B, d_out.p, off.data(), tab.data());
  d_tab.alloc(tab.size() * sizeof(SurfFrame));
  LP_HIP(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(SurfFrame), hipMemcpyHostToDevice));
  launch_surfaces_to_bgr(d_tab.as<SurfFrame>(), d_out.as<uint8_t>(), B, max_blocks, fmt->pixfmt == LP_SURF_P010, fmt->matrix, h->stream);
  LP_HIP(hipStreamSynchronize(h->stream));
  std::vector<uint8_t> all(d_out.bytes);
  LP_HIP(hipMemcpy(all.data(), d_out.p, all.size(), hipMemcpyDeviceToHost));
  std::vector<char> owned(all.size(), 0);
  size_t o = 0;
  for (int i = 0; i < B; ++i) {
    memcpy(out_bgr + o, all.data() + off[i], fb[i]);
    memset(owned.data() + off[i], 1, fb[i]);
    o += fb[i];
  }
  size_t touched = 0;
  for (size_t k = 0; k < all.size(); ++k) touched += !owned[k] && all[k] != 0xA5;
  LP_CHECK(touched == 0, LP_ERR_STATE, "the converter wrote %zu bytes outside its output frames", touched);
  LP_API_END
}

int lp_graph_stats(lp_handle* h, int* entries, int64_t* eager, int64_t* captures, int64_t* replays) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (entries) *entries = (int)h->graphs.size();
  if (eager) *eager = h->n_eager;
  if (captures) *captures = h->n_captures;
  if (replays) *replays = h->n_replays;
  LP_API_END
}

}  // extern "C"
