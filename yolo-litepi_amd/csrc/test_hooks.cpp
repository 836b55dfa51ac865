// Test and debug hooks (lp_test_*, lp_debug_blob): single kernels and host rules on buffers of their own, for the test suite.
#include "handle.h"

using namespace lp;

namespace {

// counts, records and rectangles of one image (or frame) back on the host once the stream is idle
void read_one_image(lp_handle* h, const DevBuf& d_dets, const DevBuf& d_counts, const DevBuf& d_rects, lp_det* dets, int* rects, int* count,
                    int* num_det) {
  LP_HIP(hipStreamSynchronize(h->stream));
  int cnt[3];
  LP_HIP(hipMemcpy(cnt, d_counts.p, 12, hipMemcpyDeviceToHost));
  *count = cnt[0];
  if (num_det) *num_det = cnt[1];
  LP_HIP(hipMemcpy(dets, d_dets.p, (size_t)(*count) * sizeof(lp_det), hipMemcpyDeviceToHost));
  if (rects) LP_HIP(hipMemcpy(rects, d_rects.p, (size_t)(*count) * 16, hipMemcpyDeviceToHost));
}

// NMS of one image's candidates (A slots in d_cand, their number in d_cnt) on buffers of its own, and the results back
void nms_one_image(lp_handle* h, const DevBuf& d_geom, const DevBuf& d_cand, const DevBuf& d_cnt, int A, int nc, float iou, int min_area,
                   int max_det, lp_det* dets, int* rects, int* count, int* num_det) {
  if (max_det <= 0 || max_det > A) max_det = A;  // the reference keeps every survivor
  DevBuf d_sorted, d_dets, d_counts, d_rects;
  d_sorted.alloc((size_t)A * sizeof(Cand));
  d_dets.alloc((size_t)max_det * sizeof(lp_det)); d_counts.alloc(16); d_rects.alloc((size_t)max_det * 16);
  NmsArgs a;
  memset(&a, 0, sizeof(a));
  a.cand = d_cand.as<Cand>(); a.cand_count = d_cnt.as<int>(); a.sorted = d_sorted.as<Cand>(); a.geom = d_geom.as<ImgGeom>();
  a.c = nms_common(h, d_dets.as<lp_det>(), d_counts.as<int>(), d_rects.as<int>(), A, nc, max_det, iou, min_area, false);
  launch_nms(a, 1, h->stream);
  read_one_image(h, d_dets, d_counts, d_rects, dets, rects, count, num_det);
}

// The views of one frame through enqueue_view_gather on buffers of its own, back in the frame's view order.  The frame is
// uploaded frame.src_off bytes into an allocation of its size + slack bytes.
void gather_one_frame(lp_handle* h, const uint8_t* img, const ImgGeom& frame, size_t slack, const ViewLayout& lay, uint8_t* out) {
  const int S = h->cfg.det_input;
  const size_t bytes = (size_t)frame.h * frame.w * 3, vb = (size_t)S * S * 3;
  DevBuf d_src, d_geom, d_wins, d_out;
  d_src.alloc(bytes + slack);
  LP_HIP(hipMemcpy(d_src.as<uint8_t>() + frame.src_off, img, bytes, hipMemcpyHostToDevice));
  d_geom.alloc((size_t)lay.V * sizeof(ImgGeom));
  LP_HIP(hipMemcpy(d_geom.p, lay.vgeom.data(), (size_t)lay.V * sizeof(ImgGeom), hipMemcpyHostToDevice));
  if (!lay.wins.empty()) {
    d_wins.alloc(lay.wins.size() * sizeof(ViewWin));
    LP_HIP(hipMemcpy(d_wins.p, lay.wins.data(), lay.wins.size() * sizeof(ViewWin), hipMemcpyHostToDevice));
  }
  DevBuf d_maps;
  if (!lay.maps.empty()) {
    d_maps.alloc(lay.maps.size() * sizeof(MapSlot));
    LP_HIP(hipMemcpy(d_maps.p, lay.maps.data(), lay.maps.size() * sizeof(MapSlot), hipMemcpyHostToDevice));
  }
  d_out.alloc((size_t)lay.V * vb);
  enqueue_view_gather(d_src.as<uint8_t>(), d_geom.as<ImgGeom>(), d_wins.as<ViewWin>(), d_out.as<uint8_t>(), lay, S, h->stream, nullptr,
                      d_maps.as<MapSlot>());
  LP_HIP(hipStreamSynchronize(h->stream));
  for (int k = 0; k < lay.V; ++k)
    LP_HIP(hipMemcpy(out + (size_t)k * vb, d_out.as<uint8_t>() + (size_t)lay.vslot[k] * vb, vb, hipMemcpyDeviceToHost));
}

// the letterbox of one host image on buffers of its own; kernel: 0 = the launcher's choice (the tiled kernel where its LDS rows
// fit), 1 = the per-pixel kernel
void test_letterbox(lp_handle* h, const uint8_t* img, int H, int W, uint8_t* out, float* ratio, float* pad_w, float* pad_h, int kernel) {
  LP_CHECK(h && img && out && H > 0 && W > 0, LP_ERR_ARG, "bad argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  const int SH = h->det_h(), SW = h->det_w();
  ImgGeom g = make_geom(H, W, SH, SW, 0);
  DevBuf d_src, d_geom, d_out;
  d_src.alloc((size_t)H * W * 3);
  LP_HIP(hipMemcpy(d_src.p, img, (size_t)H * W * 3, hipMemcpyHostToDevice));
  d_geom.alloc(sizeof(g));
  LP_HIP(hipMemcpy(d_geom.p, &g, sizeof(g), hipMemcpyHostToDevice));
  d_out.alloc((size_t)SH * SW * 3);
  launch_letterbox(d_src.as<uint8_t>(), d_geom.as<ImgGeom>(), d_out.as<uint8_t>(), 1, SH, SW, h->stream, kernel == 1 ? nullptr : &g);
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_HIP(hipMemcpy(out, d_out.p, (size_t)SH * SW * 3, hipMemcpyDeviceToHost));
  if (ratio) *ratio = g.ratio;
  if (pad_w) *pad_w = g.pad_w;
  if (pad_h) *pad_h = g.pad_h;
}

}  // namespace

extern "C" {

int lp_test_nms_views(lp_handle* h, const float* boxes, const float* scores, const int* classes, const int* views, const int* anchors,
                      int n, int n_views, int orig_h, int orig_w, float iou, int min_area, int max_det, lp_det* dets, int* rects,
                      int* count, int* num_det) {
  LP_API_BEGIN
  LP_CHECK(h && dets && count && n >= 0 && n_views >= 1 && n_views <= 1024 && orig_h > 0 && orig_w > 0, LP_ERR_ARG, "bad argument");
  LP_CHECK(n == 0 || (boxes && scores && views && anchors), LP_ERR_ARG, "null argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  int A = 1, nc = 1;
  for (int i = 0; i < n; ++i) {
    LP_CHECK(views[i] >= 0 && views[i] < n_views && anchors[i] >= 0 && anchors[i] < 16384, LP_ERR_ARG,
             "candidate %d: view %d / anchor %d out of range", i, views[i], anchors[i]);
    A = std::max(A, anchors[i] + 1);
    nc = std::max(nc, (classes ? classes[i] : 0) + 1);
  }
  std::vector<Cand> cand((size_t)n_views * A);
  std::vector<int> cnt(n_views, 0);
  std::vector<char> seen((size_t)n_views * A, 0);
  for (int i = 0; i < n; ++i) {
    const int v = views[i];
    LP_CHECK(!seen[(size_t)v * A + anchors[i]], LP_ERR_ARG, "candidate %d: anchor %d appears twice in view %d", i, anchors[i], v);
    seen[(size_t)v * A + anchors[i]] = 1;
    Cand c;
    c.x1 = boxes[4 * i]; c.y1 = boxes[4 * i + 1]; c.x2 = boxes[4 * i + 2]; c.y2 = boxes[4 * i + 3];
    c.score = scores[i]; c.cls = classes ? classes[i] : 0; c.anchor = anchors[i]; c.pad = 0;
    cand[(size_t)v * A + cnt[v]++] = c;
  }
  ImgGeom g;
  memset(&g, 0, sizeof(g));
  g.h = orig_h; g.w = orig_w; g.ratio = 1.f;
  TileFrame fr{0, n_views};
  std::vector<int> vslot(n_views);
  for (int v = 0; v < n_views; ++v) vslot[v] = v;
  if (max_det <= 0 || max_det > n_views * A) max_det = n_views * A;  // the reference keeps every survivor
  DevBuf d_geom, d_cand, d_sorted, d_cnt, d_vcnt, d_fr, d_vslot, d_dets, d_counts, d_rects;
  d_geom.alloc(sizeof(g));
  LP_HIP(hipMemcpy(d_geom.p, &g, sizeof(g), hipMemcpyHostToDevice));
  d_cand.alloc(cand.size() * sizeof(Cand)); d_sorted.alloc(cand.size() * sizeof(Cand));
  LP_HIP(hipMemcpy(d_cand.p, cand.data(), cand.size() * sizeof(Cand), hipMemcpyHostToDevice));
  d_cnt.alloc((size_t)n_views * 4); d_vcnt.alloc((size_t)n_views * 4);
  LP_HIP(hipMemcpy(d_cnt.p, cnt.data(), (size_t)n_views * 4, hipMemcpyHostToDevice));
  d_fr.alloc(sizeof(fr)); LP_HIP(hipMemcpy(d_fr.p, &fr, sizeof(fr), hipMemcpyHostToDevice));
  d_vslot.alloc((size_t)n_views * 4); LP_HIP(hipMemcpy(d_vslot.p, vslot.data(), (size_t)n_views * 4, hipMemcpyHostToDevice));
  d_dets.alloc((size_t)max_det * sizeof(lp_det)); d_counts.alloc(16); d_rects.alloc((size_t)max_det * 16);
  FrameNmsArgs a;
  memset(&a, 0, sizeof(a));
  a.cand = d_cand.as<Cand>(); a.cand_count = d_cnt.as<int>(); a.vcnt = d_vcnt.as<int>(); a.sorted = d_sorted.as<Cand>();
  a.frames = d_fr.as<TileFrame>(); a.vslot = d_vslot.as<int>();
  a.fgeom = d_geom.as<ImgGeom>();
  a.c = nms_common(h, d_dets.as<lp_det>(), d_counts.as<int>(), d_rects.as<int>(), A, nc, max_det, iou, min_area, false);
  apply_view_merge(h, iou, a);
  launch_view_sort(a, n_views, h->stream);
  launch_frame_nms(a, 1, n_views, h->stream);
  read_one_image(h, d_dets, d_counts, d_rects, dets, rects, count, num_det);
  LP_API_END
}

int lp_test_tile_views(lp_handle* h, const uint8_t* img, int H, int W, const lp_tiling* tiling, int byte_offset, uint8_t* out, int cap,
                       int* n_views) {
  LP_API_BEGIN
  LP_CHECK(h && img && n_views && H > 0 && W > 0 && byte_offset >= 0 && byte_offset < 64, LP_ERR_ARG, "bad argument");
  check_square(h, "lp_test_tile_views");
  check_tiling(tiling, h->cfg.det_input);
  LP_HIP(hipSetDevice(h->cfg.device));
  const std::vector<ImgGeom> fg(1, make_geom(H, W, h->det_h(), h->det_w(), byte_offset));
  const ViewLayout lay = view_layout(h, fg, tiled_views(h->cfg.det_input, *tiling, fg));
  *n_views = lay.V;
  LP_CHECK(!out || cap >= lay.V, LP_ERR_ARG, "%d views, room for %d", lay.V, cap);
  if (out) gather_one_frame(h, img, fg[0], 64, lay, out);
  LP_API_END
}

int lp_test_view_windows(lp_handle* h, const uint8_t* img, int H, int W, const int* views, int n_views, int byte_offset, uint8_t* out,
                         int cap) {
  LP_API_BEGIN
  LP_CHECK(h && img && out && H > 0 && W > 0 && byte_offset >= 0 && byte_offset < 64, LP_ERR_ARG, "bad argument");
  check_square(h, "lp_test_view_windows");
  LP_HIP(hipSetDevice(h->cfg.device));
  const std::vector<ImgGeom> fg(1, make_geom(H, W, h->det_h(), h->det_w(), byte_offset));
  const ViewLayout lay = view_layout(h, fg, listed_views(h, views, n_views, fg));
  LP_CHECK(cap >= lay.V, LP_ERR_ARG, "%d views, room for %d", lay.V, cap);
  // the frame is the whole allocation but for the offset in front: nothing the gather may read lies beyond it
  gather_one_frame(h, img, fg[0], byte_offset, lay, out);
  LP_API_END
}

int lp_test_map_views(lp_handle* h, const uint8_t* img, int H, int W, const int* maps, int n_maps, int byte_offset, uint8_t* out, int cap) {
  LP_API_BEGIN
  LP_CHECK(h && img && out && H > 0 && W > 0 && byte_offset >= 0 && byte_offset < 64, LP_ERR_ARG, "bad argument");
  check_square(h, "lp_test_map_views");
  LP_HIP(hipSetDevice(h->cfg.device));
  const std::vector<ImgGeom> fg(1, make_geom(H, W, h->det_h(), h->det_w(), byte_offset));
  const ViewLayout lay = view_layout(h, fg, mapped_views(h, nullptr, 0, maps, n_maps, fg));
  LP_CHECK(cap >= lay.V, LP_ERR_ARG, "%d views, room for %d", lay.V, cap);
  // the frame is the whole allocation but for the offset in front: nothing the gather may read lies beyond it
  gather_one_frame(h, img, fg[0], byte_offset, lay, out);
  LP_API_END
}

int lp_test_map_boxes(lp_handle* h, int map, const float* boxes, int n, float* out) {
  LP_API_BEGIN
  LP_CHECK(h && n >= 0 && n <= 16384 && (n == 0 || (boxes && out)), LP_ERR_ARG, "bad argument");
  check_square(h, "lp_test_map_boxes");
  LP_CHECK(map >= 0 && map < (int)h->maps.size(), LP_ERR_ARG, "id %d is not a map of the handle (it holds %zu)", map, h->maps.size());
  if (n == 0) return LP_OK;
  LP_HIP(hipSetDevice(h->cfg.device));
  std::vector<Cand> cand(n);
  for (int i = 0; i < n; ++i) {
    Cand c;
    c.x1 = boxes[4 * i]; c.y1 = boxes[4 * i + 1]; c.x2 = boxes[4 * i + 2]; c.y2 = boxes[4 * i + 3];
    c.score = 1.f; c.cls = 0; c.anchor = i; c.pad = 0;
    cand[i] = c;
  }
  MapSlot m;
  memset(&m, 0, sizeof(m));
  m.fixed = h->maps[map]->fixed.as<int32_t>(); m.H = h->maps[map]->H; m.W = h->maps[map]->W;
  DevBuf d_map, d_cand, d_cnt;
  d_map.alloc(sizeof(m)); LP_HIP(hipMemcpy(d_map.p, &m, sizeof(m), hipMemcpyHostToDevice));
  d_cand.alloc((size_t)n * sizeof(Cand)); LP_HIP(hipMemcpy(d_cand.p, cand.data(), (size_t)n * sizeof(Cand), hipMemcpyHostToDevice));
  d_cnt.alloc(16); LP_HIP(hipMemcpy(d_cnt.p, &n, 4, hipMemcpyHostToDevice));
  launch_map_candidates(d_map.as<MapSlot>(), d_cand.as<Cand>(), d_cnt.as<int>(), 0, 1, n, h->cfg.det_input, h->stream);
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_HIP(hipMemcpy(cand.data(), d_cand.p, (size_t)n * sizeof(Cand), hipMemcpyDeviceToHost));
  for (int i = 0; i < n; ++i) {
    LP_CHECK(cand[i].score == 1.f && cand[i].cls == 0 && cand[i].anchor == i, LP_ERR_STATE, "candidate %d: score, class or anchor changed", i);
    out[4 * i] = cand[i].x1; out[4 * i + 1] = cand[i].y1; out[4 * i + 2] = cand[i].x2; out[4 * i + 3] = cand[i].y2;
  }
  LP_API_END
}

int lp_test_convert_frames(lp_handle* h, const uint8_t* frames, int B, int H, int W, const lp_frame_format* fmt, int byte_offset,
                           uint8_t* out_bgr) {
  LP_API_BEGIN
  LP_CHECK(h && frames && out_bgr && fmt && B >= 1 && byte_offset >= 0 && byte_offset < 64, LP_ERR_ARG, "bad argument");
  check_format(fmt);
  LP_CHECK(fmt->pixfmt == LP_PIX_NV12, LP_ERR_ARG, "lp_test_convert_frames converts NV12 frames");
  const FrameLayout L = frame_layout(*fmt, H, W);
  LP_HIP(hipSetDevice(h->cfg.device));
  // the output sits between two guard zones, and its frames at 16-byte aligned offsets as in d_src; every byte the
  // converter does not own (guards, the gaps between frames) must still hold the fill pattern afterwards
  const size_t guard = 256, fb = (size_t)H * W * 3, fs = align16(fb), in_bytes = (size_t)(B - 1) * L.stride + L.frame_bytes;
  DevBuf d_in, d_tab, d_out;
  d_in.alloc(in_bytes + 64);
  LP_HIP(hipMemcpy(d_in.as<uint8_t>() + byte_offset, frames, in_bytes, hipMemcpyHostToDevice));
  d_out.alloc(2 * guard + fs * B, false);
  LP_HIP(hipMemset(d_out.p, 0xA5, d_out.bytes));
  LP_HIP(hipDeviceSynchronize());
  std::vector<CscFrame> tab(B);
  int max_blocks = 0;
  for (int i = 0; i < B; ++i) {
    tab[i] = CscFrame{(long)(byte_offset + i * L.stride), (long)L.uv_off, (long)(guard + i * fs), H, W, L.pitch, 0};
    max_blocks = std::max(max_blocks, (H / 2) * ((W + 15) / 16));
  }
  finish_csc_table(tab, d_in.p, d_out.p);
  d_tab.alloc(tab.size() * sizeof(CscFrame));
  LP_HIP(hipMemcpy(d_tab.p, tab.data(), tab.size() * sizeof(CscFrame), hipMemcpyHostToDevice));
  launch_nv12_to_bgr(d_in.as<uint8_t>(), d_tab.as<CscFrame>(), d_out.as<uint8_t>(), B, max_blocks, fmt->matrix, h->stream);
  LP_HIP(hipStreamSynchronize(h->stream));
  std::vector<uint8_t> all(d_out.bytes);
  LP_HIP(hipMemcpy(all.data(), d_out.p, all.size(), hipMemcpyDeviceToHost));
  for (int i = 0; i < B; ++i) memcpy(out_bgr + i * fb, all.data() + guard + i * fs, fb);
  size_t touched = 0;
  for (size_t k = 0; k < all.size(); ++k) {
    const bool owned = k >= guard && k < guard + fs * B && (k - guard) % fs < fb;
    touched += !owned && all[k] != 0xA5;
  }
  LP_CHECK(touched == 0, LP_ERR_STATE, "the converter wrote %zu bytes outside its output frames", touched);
  LP_API_END
}

int lp_debug_blob(lp_handle* h, const char* blob, float* out, int64_t cap, int* C, int* H, int* W) {
  LP_API_BEGIN
  LP_CHECK(h && blob && C && H && W, LP_ERR_ARG, "null argument");
  LP_CHECK(h->det && h->det->loaded(), LP_ERR_STATE, "detector not loaded");
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  std::vector<float> v;
  h->det->fetch_blob(blob, 1, v, *C, *H, *W);
  // as many leading images of the last batch as the caller's buffer holds (at least one, at most the handle's capacity)
  const int64_t per_image = (int64_t)v.size();
  if (out && per_image > 0 && cap >= 2 * per_image) {
    LP_CHECK(cap / per_image <= h->cfg.max_batch, LP_ERR_ARG, "buffer for %lld images, the handle holds %d", (long long)(cap / per_image), h->cfg.max_batch);
    h->det->fetch_blob(blob, (int)(cap / per_image), v, *C, *H, *W);
  }
  if (out) {
    LP_CHECK((int64_t)v.size() <= cap, LP_ERR_ARG, "blob needs %zu floats, buffer has %lld", v.size(), (long long)cap);
    memcpy(out, v.data(), v.size() * 4);
  }
  LP_API_END
}

int lp_test_conv(lp_handle* h, int impl, const float* x, int N, int Cin, int H, int W, const float* w, const float* bias,
                 int Cout, int k, int stride, int act, const float* res, float* y) {
  LP_API_BEGIN
  LP_CHECK(h && x && w && y, LP_ERR_ARG, "null argument");
  LP_CHECK(Cin % 8 == 0 && Cout % 8 == 0, LP_ERR_ARG, "test conv needs channel counts that are multiples of 8");
  LP_HIP(hipSetDevice(h->cfg.device));
  const int prec = h->cfg.precision;
  const size_t es = prec == LP_FP16 ? 2 : 4;
  const int pad = k / 2, Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  const int taps = k * k;
  std::vector<float> wp((size_t)Cout * taps * Cin), bp(Cout, 0.f);
  for (int o = 0; o < Cout; ++o) {
    for (int i = 0; i < Cin; ++i)
      for (int t = 0; t < taps; ++t) wp[((size_t)o * taps + t) * Cin + i] = w[((size_t)o * Cin + i) * taps + t];
    if (bias) bp[o] = bias[o];
  }
  ConvLayer L;
  L.build(prec, impl, k, stride, Cin, Cout, act, wp, bp, Ho, Wo, N);
  auto to_dev = [&](const float* src, int C, int HH, int WW, DevBuf& d) {
    const size_t npix = (size_t)N * HH * WW;
    std::vector<uint8_t> buf(npix * C * es);
    for (size_t p = 0; p < npix; ++p) {
      const size_t b = p / ((size_t)HH * WW), yx = p % ((size_t)HH * WW);
      for (int c = 0; c < C; ++c) {
        const float v = src[(b * C + c) * HH * WW + yx];
        if (prec == LP_FP16) { uint16_t hv = f32_to_f16(v); memcpy(&buf[(p * C + c) * 2], &hv, 2); }
        else memcpy(&buf[(p * C + c) * 4], &v, 4);
      }
    }
    d.alloc(buf.size());
    LP_HIP(hipMemcpy(d.p, buf.data(), buf.size(), hipMemcpyHostToDevice));
  };
  DevBuf dx, dy, dr;
  to_dev(x, Cin, H, W, dx);
  dy.alloc((size_t)N * Ho * Wo * Cout * es);
  ConvIO io;
  io.N = N;
  io.in = View{dx.p, Cin, Cin, H, W};
  io.out = View{dy.p, Cout, Cout, Ho, Wo};
  if (res) { to_dev(res, Cout, Ho, Wo, dr); io.res = View{dr.p, Cout, Cout, Ho, Wo}; }
  // diagnostic: LITEPI_STAMPS=<file> dumps 16 clock stamps per workgroup of a (warm) second launch
  const char* stamp_path = getenv("LITEPI_STAMPS");
  L.launch(io, h->stream);
  LP_HIP(hipStreamSynchronize(h->stream));
  if (stamp_path && *stamp_path) {
    const size_t nst = (size_t)1 << 22;
    DevBuf ds;
    ds.alloc(nst * 8);
    io.stamps = ds.as<unsigned long long>();
    L.launch(io, h->stream);
    LP_HIP(hipStreamSynchronize(h->stream));
    std::vector<unsigned long long> hs(nst);
    LP_HIP(hipMemcpy(hs.data(), ds.p, nst * 8, hipMemcpyDeviceToHost));
    size_t used = nst;
    while (used > 16 && hs[used - 16] == 0 && hs[used - 4] == 0) used -= 16;
    FILE* f = fopen(stamp_path, "wb");
    if (f) { fwrite(hs.data(), 8, used, f); fclose(f); }
    io.stamps = nullptr;
  }
  std::vector<uint8_t> raw((size_t)N * Ho * Wo * Cout * es);
  LP_HIP(hipMemcpy(raw.data(), dy.p, raw.size(), hipMemcpyDeviceToHost));
  const size_t npix = (size_t)N * Ho * Wo;
  for (size_t p = 0; p < npix; ++p) {
    const size_t b = p / ((size_t)Ho * Wo), yx = p % ((size_t)Ho * Wo);
    for (int c = 0; c < Cout; ++c) {
      float f;
      if (prec == LP_FP16) { uint16_t hv; memcpy(&hv, &raw[(p * Cout + c) * 2], 2); f = f16_to_f32(hv); }
      else memcpy(&f, &raw[(p * Cout + c) * 4], 4);
      y[(b * Cout + c) * Ho * Wo + yx] = f;
    }
  }
  LP_API_END
}

int lp_test_postprocess(lp_handle* h, const float* out0, int nc, int A, int orig_h, int orig_w, float ratio, float pad_w,
                        float pad_h, float conf, float iou, int min_area, int max_det, lp_det* dets, int* rects, int* count,
                        int* num_det) {
  LP_API_BEGIN
  LP_CHECK(h && out0 && dets && count && nc >= 1 && A >= 1 && A <= 16384, LP_ERR_ARG, "bad argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  ImgGeom g;
  memset(&g, 0, sizeof(g));
  g.h = orig_h; g.w = orig_w; g.ratio = ratio; g.pad_w = pad_w; g.pad_h = pad_h;
  DevBuf d_out0, d_geom, d_cand, d_cnt;
  d_out0.alloc((size_t)(4 + nc) * A * 4);
  LP_HIP(hipMemcpy(d_out0.p, out0, (size_t)(4 + nc) * A * 4, hipMemcpyHostToDevice));
  d_geom.alloc(sizeof(g));
  LP_HIP(hipMemcpy(d_geom.p, &g, sizeof(g), hipMemcpyHostToDevice));
  d_cand.alloc((size_t)A * sizeof(Cand)); d_cnt.alloc(16);
  launch_filter_out0(d_out0.as<float>(), nc, A, d_geom.as<ImgGeom>(), d_cand.as<Cand>(), d_cnt.as<int>(), conf, 1, h->stream);
  nms_one_image(h, d_geom, d_cand, d_cnt, A, nc, iou, min_area, max_det, dets, rects, count, num_det);
  LP_API_END
}

int lp_test_nms_boxes(lp_handle* h, const float* boxes, const float* scores, const int* classes, int n, int orig_h, int orig_w,
                      float iou, int min_area, int max_det, lp_det* dets, int* rects, int* count, int* num_det) {
  LP_API_BEGIN
  LP_CHECK(h && boxes && scores && dets && count && n >= 0 && n <= 16384, LP_ERR_ARG, "bad argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  const int A = n > 0 ? n : 1;
  ImgGeom g;
  memset(&g, 0, sizeof(g));
  g.h = orig_h; g.w = orig_w; g.ratio = 1.f;
  std::vector<Cand> cand(A);
  int nc = 1;
  for (int i = 0; i < n; ++i) {
    Cand c;
    c.x1 = boxes[4 * i]; c.y1 = boxes[4 * i + 1]; c.x2 = boxes[4 * i + 2]; c.y2 = boxes[4 * i + 3];
    c.score = scores[i]; c.cls = classes ? classes[i] : 0; c.anchor = i; c.pad = 0;
    nc = std::max(nc, c.cls + 1);
    cand[i] = c;
  }
  DevBuf d_geom, d_cand, d_cnt;
  d_geom.alloc(sizeof(g));
  LP_HIP(hipMemcpy(d_geom.p, &g, sizeof(g), hipMemcpyHostToDevice));
  d_cand.alloc((size_t)A * sizeof(Cand)); d_cnt.alloc(16);
  LP_HIP(hipMemcpy(d_cand.p, cand.data(), (size_t)A * sizeof(Cand), hipMemcpyHostToDevice));
  LP_HIP(hipMemcpy(d_cnt.p, &n, 4, hipMemcpyHostToDevice));
  nms_one_image(h, d_geom, d_cand, d_cnt, A, nc, iou, min_area, max_det, dets, rects, count, num_det);
  LP_API_END
}

int lp_test_roi_resize(lp_handle* h, const uint8_t* const* rois, const int* hs, const int* ws, int R, uint8_t* out_rgb) {
  LP_API_BEGIN
  LP_CHECK(h && rois && hs && ws && out_rgb && R >= 1, LP_ERR_ARG, "bad argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  const int S = h->cfg.cls_input;
  const CropRois c = whole_crop_rois(rois, hs, ws, R);
  DevBuf d_src, d_geom, d_rects, d_img, d_slot, d_total, d_base, d_out;
  d_src.alloc(c.total);
  for (int i = 0; i < R; ++i) LP_HIP(hipMemcpy(d_src.as<uint8_t>() + c.g[i].src_off, rois[i], (size_t)hs[i] * ws[i] * 3, hipMemcpyHostToDevice));
  d_geom.alloc((size_t)R * sizeof(ImgGeom));
  LP_HIP(hipMemcpy(d_geom.p, c.g.data(), (size_t)R * sizeof(ImgGeom), hipMemcpyHostToDevice));
  d_rects.alloc((size_t)R * 16); LP_HIP(hipMemcpy(d_rects.p, c.rects.data(), (size_t)R * 16, hipMemcpyHostToDevice));
  d_img.alloc((size_t)R * 4); LP_HIP(hipMemcpy(d_img.p, c.img.data(), (size_t)R * 4, hipMemcpyHostToDevice));
  d_slot.alloc((size_t)R * 4);
  d_total.alloc(16); LP_HIP(hipMemcpy(d_total.p, &R, 4, hipMemcpyHostToDevice));
  d_base.alloc(16);
  d_out.alloc((size_t)R * S * S * 3);
  RoiResizeArgs r;
  r.src = d_src.as<uint8_t>(); r.geom = d_geom.as<ImgGeom>(); r.rects = d_rects.as<int>();
  r.tab.base = d_base.as<int>(); r.tab.total = d_total.as<int>(); r.tab.img = d_img.as<int>(); r.tab.slot = d_slot.as<int>();
  r.out = d_out.as<uint8_t>(); r.max_det = 1; r.S = S; r.linear = h->cfg.numerics;
  launch_roi_resize(r, R, h->stream);
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_HIP(hipMemcpy(out_rgb, d_out.p, (size_t)R * S * S * 3, hipMemcpyDeviceToHost));
  LP_API_END
}

// R rectangles of ONE frame: the frame's buffer is exactly H * W * 3 bytes, so a rectangle that touches a corner has the
// buffer's first or last byte inside it, and an odd W puts the rows on all four alignments
int lp_test_roi_resize_rects(lp_handle* h, const uint8_t* frame, int H, int W, const int* rects, int R, uint8_t* out_rgb) {
  LP_API_BEGIN
  LP_CHECK(h && frame && rects && out_rgb && H >= 1 && W >= 1 && R >= 1, LP_ERR_ARG, "bad argument");
  LP_CHECK((long)H * W * 3 <= 0x7fffffffL, LP_ERR_ARG, "frame %d x %d too large", H, W);
  for (int i = 0; i < R; ++i) {
    const int* rc = rects + 4 * i;
    LP_CHECK(rc[0] >= 0 && rc[0] < rc[2] && rc[2] <= W && rc[1] >= 0 && rc[1] < rc[3] && rc[3] <= H, LP_ERR_ARG,
             "rectangle %d (%d, %d, %d, %d) is empty or leaves the %d x %d frame", i, rc[0], rc[1], rc[2], rc[3], W, H);
  }
  LP_HIP(hipSetDevice(h->cfg.device));
  const int S = h->cfg.cls_input;
  ImgGeom g;
  memset(&g, 0, sizeof(g));
  g.h = H; g.w = W;
  std::vector<int> img(R, 0), slot(R);
  for (int i = 0; i < R; ++i) slot[i] = i;
  DevBuf d_src, d_geom, d_rects, d_img, d_slot, d_total, d_base, d_out;
  d_src.alloc((size_t)H * W * 3, false);
  LP_HIP(hipMemcpy(d_src.p, frame, (size_t)H * W * 3, hipMemcpyHostToDevice));
  d_geom.alloc(sizeof(g)); LP_HIP(hipMemcpy(d_geom.p, &g, sizeof(g), hipMemcpyHostToDevice));
  d_rects.alloc((size_t)R * 16); LP_HIP(hipMemcpy(d_rects.p, rects, (size_t)R * 16, hipMemcpyHostToDevice));
  d_img.alloc((size_t)R * 4);
  d_slot.alloc((size_t)R * 4); LP_HIP(hipMemcpy(d_slot.p, slot.data(), (size_t)R * 4, hipMemcpyHostToDevice));
  d_total.alloc(16); LP_HIP(hipMemcpy(d_total.p, &R, 4, hipMemcpyHostToDevice));
  d_base.alloc(16);
  d_out.alloc((size_t)R * S * S * 3);
  RoiResizeArgs r;
  r.src = d_src.as<uint8_t>(); r.geom = d_geom.as<ImgGeom>(); r.rects = d_rects.as<int>();
  r.tab.base = d_base.as<int>(); r.tab.total = d_total.as<int>(); r.tab.img = d_img.as<int>(); r.tab.slot = d_slot.as<int>();
  r.tab.work = nullptr;
  r.out = d_out.as<uint8_t>(); r.max_det = R; r.S = S; r.linear = h->cfg.numerics;
  launch_roi_resize(r, R, h->stream);
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_HIP(hipMemcpy(out_rgb, d_out.p, (size_t)R * S * S * 3, hipMemcpyDeviceToHost));
  LP_API_END
}

int lp_test_letterbox(lp_handle* h, const uint8_t* img, int H, int W, uint8_t* out, float* ratio, float* pad_w, float* pad_h) {
  LP_API_BEGIN
  test_letterbox(h, img, H, W, out, ratio, pad_w, pad_h, 0);
  LP_API_END
}

int lp_test_letterbox_kernel(lp_handle* h, const uint8_t* img, int H, int W, int kernel, uint8_t* out, float* ratio, float* pad_w, float* pad_h) {
  LP_API_BEGIN
  LP_CHECK(kernel == 0 || kernel == 1, LP_ERR_ARG, "kernel %d is not 0 (launcher's choice) or 1 (per pixel)", kernel);
  test_letterbox(h, img, H, W, out, ratio, pad_w, pad_h, kernel);
  LP_API_END
}

// the ROI list and the classifier input crops of a pipeline call (tests of the sign inventory's crops)
int lp_test_set_rois(lp_handle* h, const uint8_t* crops, const int* img, const int* slot, int R) {
  LP_API_BEGIN
  LP_CHECK(h && R >= 0 && (R == 0 || (crops && img && slot)), LP_ERR_ARG, "bad argument");
  LP_CHECK(R <= h->max_rois, LP_ERR_ARG, "%d ROIs exceed max_rois = %d", R, h->max_rois);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  const size_t crop = (size_t)h->cfg.cls_input * h->cfg.cls_input * 3;
  if (R > 0) {
    LP_HIP(hipMemcpy(h->d_roi_rgb.p, crops, (size_t)R * crop, hipMemcpyHostToDevice));
    LP_HIP(hipMemcpy(h->d_roi_img.p, img, (size_t)R * 4, hipMemcpyHostToDevice));
    LP_HIP(hipMemcpy(h->d_roi_slot.p, slot, (size_t)R * 4, hipMemcpyHostToDevice));
  }
  const int total[2] = {R, R};
  LP_HIP(hipMemcpy(h->d_roi_total.p, total, sizeof(total), hipMemcpyHostToDevice));
  LP_API_END
}

int lp_test_set_frames(lp_handle* h, const uint8_t* frames, int B, int H, int W) {
  LP_API_BEGIN
  LP_CHECK(h && frames, LP_ERR_ARG, "null argument");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch && H >= 1 && W >= 1 && H <= 16384 && W <= 16384, LP_ERR_ARG, "%d frames of %dx%d", B, W, H);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  const size_t fb = (size_t)H * W * 3;
  std::vector<ImgGeom> g(B);
  for (int i = 0; i < B; ++i) g[i] = make_geom(H, W, h->det_h(), h->det_w(), (long)(i * fb));
  h->remember_frames(nullptr, nullptr, 0);
  if (h->d_tframes.bytes < B * fb) h->d_tframes.alloc(B * fb, false);
  if (h->d_tgeom.bytes < B * sizeof(ImgGeom)) h->d_tgeom.alloc((size_t)h->cfg.max_batch * sizeof(ImgGeom));
  LP_HIP(hipMemcpy(h->d_tframes.p, frames, B * fb, hipMemcpyHostToDevice));
  LP_HIP(hipMemcpy(h->d_tgeom.p, g.data(), B * sizeof(ImgGeom), hipMemcpyHostToDevice));
  h->remember_frames(h->d_tframes.as<uint8_t>(), h->d_tgeom.as<ImgGeom>(), B);
  LP_API_END
}

int lp_debug_rois(lp_handle* h, uint8_t* crops, int* img, int* slot, int cap, int* n) {
  LP_API_BEGIN
  LP_CHECK(h && n, LP_ERR_ARG, "null argument");
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  int total = 0;
  LP_HIP(hipMemcpy(&total, h->d_roi_total.p, 4, hipMemcpyDeviceToHost));
  total = std::min(std::max(total, 0), h->max_rois);
  *n = total;
  if (!crops && !img && !slot) return LP_OK;
  LP_CHECK(cap >= total, LP_ERR_ARG, "%d ROIs do not fit cap = %d", total, cap);
  if (total == 0) return LP_OK;
  const size_t crop = (size_t)h->cfg.cls_input * h->cfg.cls_input * 3;
  if (crops) LP_HIP(hipMemcpy(crops, h->d_roi_rgb.p, (size_t)total * crop, hipMemcpyDeviceToHost));
  if (img) LP_HIP(hipMemcpy(img, h->d_roi_img.p, (size_t)total * 4, hipMemcpyDeviceToHost));
  if (slot) LP_HIP(hipMemcpy(slot, h->d_roi_slot.p, (size_t)total * 4, hipMemcpyDeviceToHost));
  LP_API_END
}

}  // extern "C"
