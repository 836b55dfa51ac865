// Decoder surfaces in place (include/litepi.h lp_surface): the pinned -> device table ring, the two entry points
// and the converter's test hook.  The argument rules, the table's records and the ring's slot policy are surface_plan.h.
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
    std::unique_ptr<SurfaceRing> ring(new SurfaceRing);
    ring->table.alloc((size_t)h->cfg.max_batch * sizeof(SurfFrame));
    LP_HIP(hipHostMalloc(reinterpret_cast<void**>(&ring->host), (size_t)SurfaceRing::RING * h->cfg.max_batch * sizeof(SurfFrame),
                         hipHostMallocDefault));
    for (auto& e : ring->ev) LP_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    h->surf = std::move(ring);
  }
  SurfaceRing& r = *h->surf;
  bool wait = false;
  const int slot = r.slots.take(&wait);
  if (wait) LP_HIP(hipEventSynchronize(r.ev[slot]));   // the ring wrapped: the copy that read this slot RING calls ago has long gone
  SurfFrame* rec = r.host + (size_t)slot * h->cfg.max_batch;
  std::vector<long> off(B);
  SurfPlan p;
  p.B = B; p.matrix = fmt.matrix; p.p010 = fmt.pixfmt == LP_SURF_P010;
  for (int i = 0; i < B; ++i) {
    off[i] = g[i].src_off;
    p.bytes += (double)s[i].height * s[i].width * (1.5 * surface_sample_bytes(fmt.pixfmt) + 3.0);
  }
  p.max_blocks = fill_surface_table(fmt, s, B, h->d_src.p, off.data(), rec);
  LP_HIP(hipMemcpyAsync(r.table.p, rec, (size_t)B * sizeof(SurfFrame), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipEventRecord(r.ev[slot], h->stream));
  r.slots.mark(slot);
  return p;
}

void enqueue_surfaces(lp_handle* h, const SurfPlan& p, Profiler* prof) {
  if (prof) prof->begin(h->stream);
  launch_surfaces_to_bgr(h->surf->table.as<SurfFrame>(), h->d_src.as<uint8_t>(), p.B, p.max_blocks, p.p010, p.matrix, h->stream);
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

GraphKey surface_key(const lp_handle* h, GraphKind kind, const lp_surface_format& fmt, int B, int min_area, void* dev_dets, void* dev_counts,
                     float conf, float iou) {
  // no surface address, pitch or table generation: the table's content is data.  Sizes are in geom_ver (upload_geom), the
  // destination's address too (ensure_src).
  GraphKey key{kind, B, h->geom_ver, min_area, nullptr, dev_dets, dev_counts, conf, iou};
  key.pixfmt = fmt.pixfmt; key.matrix = fmt.matrix;
  return key;
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
  const SurfPlan plan = stage_surfaces(h, *fmt, surfaces, B, g);
  Profiler* prof = begin_profile(h);
  const uint8_t* src = h->d_src.as<uint8_t>();
  const bool classify = h->cls && h->cls->loaded();
  h->remember_frames(src, h->d_geom.as<ImgGeom>(), B);
  const GraphKey key = surface_key(h, GK_SURFACES_DEVICE, *fmt, B, min_area, dev_dets, dev_counts, conf, iou);
  run_or_capture(h, key, prof == nullptr, [&]() {
    enqueue_surfaces(h, plan, prof);
    enqueue_detect(h, src, g, B, conf, nullptr, prof);
    enqueue_nms(h, B, iou, classify ? min_area : -1, static_cast<lp_det*>(dev_dets), static_cast<int*>(dev_counts), classify, prof);
    if (classify) enqueue_classify(h, src, B, static_cast<lp_det*>(dev_dets), nullptr, nullptr, nullptr, prof);
  });
  if (prof) prof->enabled = false;  // records are collected by lp_profile_read after the caller synchronises
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
  const SurfPlan plan = stage_surfaces(h, *fmt, surfaces, B, fg);
  Profiler* prof = begin_profile(h);
  const uint8_t* src = h->d_src.as<uint8_t>();
  const bool classify = h->cls && h->cls->loaded();
  h->remember_frames(src, h->d_fgeom.as<ImgGeom>(), B);
  const GraphKey key = surface_key(h, GK_VIEWS_SURFACES_DEVICE, *fmt, B, min_area, dev_dets, dev_counts, conf, iou);
  run_or_capture(h, key, prof == nullptr, [&]() {
    enqueue_surfaces(h, plan, prof);
    enqueue_view_front(h, src, lay, B, conf, iou, classify ? min_area : -1, static_cast<lp_det*>(dev_dets), static_cast<int*>(dev_counts),
                       classify, prof);
    if (classify) enqueue_classify(h, src, B, static_cast<lp_det*>(dev_dets), nullptr, nullptr, nullptr, prof, 0, h->d_fgeom.as<ImgGeom>());
  });
  if (prof) prof->enabled = false;  // records are collected by lp_profile_read after the caller synchronises
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
