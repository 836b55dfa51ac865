// Input pixel format (include/litepi.h lp_frame_format): the layout rules, the conversion plan of a call and its place in the
// graph key.
#include "handle.h"

namespace lp {

// what can be said without a frame size: enum values, reserved words, signs, BGR8 without layout fields
void check_format(const lp_frame_format* f) {
  if (!f) return;   // packed BGR
  LP_CHECK(f->pixfmt == LP_PIX_BGR8 || f->pixfmt == LP_PIX_NV12, LP_ERR_ARG, "unknown pixel format %d", f->pixfmt);
  bool zero = f->reserved0 == 0;
  for (int r : f->reserved) zero = zero && r == 0;
  LP_CHECK(zero, LP_ERR_ARG, "lp_frame_format: reserved words must be zero");
  if (f->pixfmt == LP_PIX_BGR8) {
    LP_CHECK(f->pitch == 0 && f->uv_offset == 0 && f->frame_stride == 0, LP_ERR_ARG,
             "packed BGR frames are tight: pitch / uv_offset / frame_stride must be 0");
    return;
  }
  LP_CHECK(f->matrix == LP_CSC_BT601_LIMITED || f->matrix == LP_CSC_BT709_LIMITED, LP_ERR_ARG, "unknown colour matrix %d", f->matrix);
  LP_CHECK(f->pitch >= 0 && f->uv_offset >= 0 && f->frame_stride >= 0, LP_ERR_ARG, "lp_frame_format: negative pitch / uv_offset / frame_stride");
}

// the layout of one H x W frame with the zeros resolved; throws LP_ERR_ARG for what the size rules out
FrameLayout frame_layout(const lp_frame_format& f, int H, int W) {
  LP_CHECK(H > 0 && W > 0, LP_ERR_ARG, "frame of %dx%d is empty", W, H);
  FrameLayout L;
  if (f.pixfmt != LP_PIX_NV12) {
    L.pitch = W * 3; L.uv_off = 0; L.frame_bytes = (int64_t)H * W * 3; L.stride = L.frame_bytes;
    return L;
  }
  LP_CHECK(H % 2 == 0 && W % 2 == 0, LP_ERR_ARG, "NV12 frames need an even width and height (got %dx%d)", W, H);
  L.pitch = f.pitch ? f.pitch : W;
  LP_CHECK(L.pitch >= W, LP_ERR_ARG, "NV12 pitch %d is smaller than the frame width %d", L.pitch, W);
  L.uv_off = f.uv_offset ? f.uv_offset : (int64_t)L.pitch * H;
  LP_CHECK(L.uv_off >= (int64_t)L.pitch * H, LP_ERR_ARG, "NV12 uv_offset %lld lies inside the Y plane (pitch %d x height %d = %lld bytes)",
           (long long)L.uv_off, L.pitch, H, (long long)L.pitch * H);
  L.frame_bytes = L.uv_off + (int64_t)L.pitch * (H / 2);
  L.stride = f.frame_stride ? f.frame_stride : L.frame_bytes;
  LP_CHECK(L.stride >= L.frame_bytes, LP_ERR_ARG, "NV12 frame_stride %lld is smaller than one frame (%lld bytes)", (long long)L.stride,
           (long long)L.frame_bytes);
  return L;
}

void finish_csc_table(std::vector<CscFrame>& tab, const void* src, const void* dst) {
  for (auto& f : tab)
    f.aligned = (reinterpret_cast<uintptr_t>(src) + f.src_off) % 16 == 0 && f.pitch % 16 == 0 && f.uv_off % 16 == 0 && f.w % 16 == 0 &&
                (reinterpret_cast<uintptr_t>(dst) + f.dst_off) % 16 == 0;
}

// put the call's table into a slot of d_csc (found by content, else the next slot round-robin under a new generation)
CscPlan plan_csc(lp_handle* h, std::vector<CscFrame>& tab, const void* src) {
  const int cap = h->cfg.max_batch;
  LP_CHECK((int)tab.size() <= cap, LP_ERR_ARG, "%zu frames exceed max_batch = %d", tab.size(), cap);
  if (!h->d_csc.p) h->d_csc.alloc((size_t)4 * cap * sizeof(CscFrame));
  finish_csc_table(tab, src, h->d_src.p);
  CscPlan p;
  p.B = (int)tab.size(); p.matrix = h->fmt.matrix;
  for (const auto& f : tab) {
    p.max_blocks = std::max(p.max_blocks, (f.h / 2) * ((f.w + 15) / 16));
    p.pixels += (double)f.h * f.w;
  }
  const size_t nbytes = tab.size() * sizeof(CscFrame);
  std::vector<char> blob(nbytes);
  memcpy(blob.data(), tab.data(), nbytes);
  int slot = -1;
  for (int s = 0; s < 4; ++s)
    if (h->csc_slots[s].gen && h->csc_slots[s].tab == blob) slot = s;
  if (slot < 0) {
    slot = h->csc_next;
    h->csc_next = (h->csc_next + 1) % 4;
    LP_HIP(hipStreamSynchronize(h->stream));   // an earlier asynchronous call may still read the slot
    LP_HIP(hipMemcpyAsync(h->d_csc.as<CscFrame>() + (size_t)slot * cap, tab.data(), nbytes, hipMemcpyHostToDevice, h->stream));
    LP_HIP(hipStreamSynchronize(h->stream));   // tab is the caller's temporary; uploads are rare (layout changes only)
    h->csc_slots[slot].tab.swap(blob);
    h->csc_slots[slot].gen = ++h->csc_gen;
  }
  p.dev = h->d_csc.as<CscFrame>() + (size_t)slot * cap;
  p.gen = h->csc_slots[slot].gen;
  return p;
}

void enqueue_csc(lp_handle* h, const uint8_t* src, const CscPlan& p, Profiler* prof) {
  if (prof) prof->begin(h->stream);
  launch_nv12_to_bgr(src, p.dev, h->d_src.as<uint8_t>(), p.B, p.max_blocks, p.matrix, h->stream);
  if (prof) prof->end(h->stream, "nv12_to_bgr", "csc", 0.0, 4.5 * p.pixels);
}

// the handle's format as part of a graph key (nothing for packed BGR: those keys are what they were)
void key_format(const lp_handle* h, const CscPlan& p, GraphKey& k) {
  if (!h->nv12()) return;
  k.pixfmt = h->fmt.pixfmt; k.matrix = h->fmt.matrix; k.pitch = h->fmt.pitch; k.csc_gen = p.gen;
  k.uv_offset = h->fmt.uv_offset; k.frame_stride = h->fmt.frame_stride;
}

// B equally sized NV12 frames resident at dev_imgs (lp_*_device): validates the layout, sizes d_src for the converted frames,
// gives their geometry (make_geom offsets, 16-byte aligned like the host path's) and the conversion plan
CscPlan device_csc(lp_handle* h, const void* dev_imgs, int B, int H, int W, std::vector<ImgGeom>& g) {
  const FrameLayout L = frame_layout(h->fmt, H, W);
  const size_t fb = align16((size_t)H * W * 3);
  std::vector<CscFrame> tab(B);
  for (int i = 0; i < B; ++i) {
    g[i] = make_geom(H, W, h->det_h(), h->det_w(), (long)(i * fb));
    tab[i] = CscFrame{(long)(i * L.stride), (long)L.uv_off, (long)(i * fb), H, W, L.pitch, 0};
  }
  h->ensure_src(fb * B);
  return plan_csc(h, tab, dev_imgs);
}

FrameSource device_frames(lp_handle* h, const void* dev_imgs, const CscPlan& csc) {
  const uint8_t* imgs = static_cast<const uint8_t*>(dev_imgs);
  FrameSource f;
  f.src = h->nv12() ? h->d_src.as<uint8_t>() : imgs;
  if (h->nv12()) f.convert = [=](Profiler* prof) { enqueue_csc(h, imgs, csc, prof); };
  f.key.p0 = dev_imgs;
  key_format(h, csc, f.key);
  return f;
}

}  // namespace lp

using namespace lp;

extern "C" {

int lp_frame_layout(const lp_frame_format* fmt, int H, int W, int64_t* uv_offset, int64_t* frame_bytes) {
  LP_API_BEGIN
  check_format(fmt);
  const lp_frame_format bgr = {};
  const FrameLayout L = frame_layout(fmt ? *fmt : bgr, H, W);
  if (uv_offset) *uv_offset = L.uv_off;
  if (frame_bytes) *frame_bytes = L.frame_bytes;
  LP_API_END
}

int lp_set_input_format(lp_handle* h, const lp_frame_format* fmt) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  check_format(fmt);
  const lp_frame_format bgr = {};
  h->fmt = fmt ? *fmt : bgr;
  LP_API_END
}

}  // extern "C"
