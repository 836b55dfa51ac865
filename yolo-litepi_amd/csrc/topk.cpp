// Top-k of the class distribution per detection (lp_topk_*, lp_test_topk; include/litepi.h).  The handle state is in handle.h,
// the launches the run families add while top-k is on in pipeline.cpp (enqueue_topk), the distribution vote in tracking.cpp.
#include "handle.h"
#include "topk_select.h"

using namespace lp;

static_assert(sizeof(lp_topk) == 64 && sizeof(TopkRec) == sizeof(lp_topk), "lp_topk is 64 bytes");
static_assert(LP_TOPK_K_MAX == LP_TOPK_MAX, "topk_select.h and litepi.h disagree on k");

static void check_topk_on(const lp_handle* h) {
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->topk_k > 0, LP_ERR_STATE, "top-k is off: call lp_topk_enable first");
}

extern "C" {

int lp_topk_enable(lp_handle* h, int k) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(k >= 0 && k <= LP_TOPK_MAX, LP_ERR_ARG, "k = %d outside 0..%d", k, LP_TOPK_MAX);
  if (k == h->topk_k) return LP_OK;
  if (k > 0 && !h->d_topk.p) {
    LP_HIP(hipSetDevice(h->cfg.device));
    h->d_topk.alloc((size_t)h->cfg.max_batch * h->cfg.max_det * sizeof(lp_topk));
    launch_topk_clear(h->d_topk.as<lp_topk>(), h->cfg.max_batch * h->cfg.max_det, h->stream);   // empty until a call fills them
  }
  h->topk_k = k;
  ++h->geom_ver;   // captured steps hold the old k's launches
  LP_API_END
}

int lp_topk_buffer(lp_handle* h, const void** dev_topk, int* k) {
  LP_API_BEGIN
  check_topk_on(h);
  if (dev_topk) *dev_topk = h->d_topk.p;
  if (k) *k = h->topk_k;
  LP_API_END
}

int lp_topk_read(lp_handle* h, lp_topk* out, int B) {
  LP_API_BEGIN
  check_topk_on(h);
  LP_CHECK(out, LP_ERR_ARG, "null argument");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipMemcpyAsync(out, h->d_topk.p, (size_t)B * h->cfg.max_det * sizeof(lp_topk), hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

int lp_topk_select(const float* p, int nc, int k, lp_topk* out) {
  LP_API_BEGIN
  LP_CHECK(p && out, LP_ERR_ARG, "null argument");
  LP_CHECK(nc >= 1 && k >= 1 && k <= LP_TOPK_MAX, LP_ERR_ARG, "nc = %d, k = %d: nc >= 1 and k in 1..%d", nc, k, LP_TOPK_MAX);
  std::vector<uint32_t> bits(nc);
  memcpy(bits.data(), p, (size_t)nc * 4);
  TopkRec r;
  topk_select_bits(bits.data(), nc, k, &r);
  memcpy(out, &r, sizeof(r));
  LP_API_END
}

int lp_test_topk(lp_handle* h, const float* probs, int R, const int* img, const int* slot, int B, lp_topk* out) {
  LP_API_BEGIN
  check_topk_on(h);
  LP_CHECK(out && R >= 0 && (R == 0 || (probs && img && slot)), LP_ERR_ARG, "bad argument");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_CHECK(R <= h->max_rois, LP_ERR_ARG, "%d ROIs exceed max_rois = %d", R, h->max_rois);
  for (int r = 0; r < R; ++r)
    LP_CHECK(img[r] >= 0 && img[r] < B && slot[r] >= 0 && slot[r] < h->cfg.max_det, LP_ERR_ARG, "ROI %d names record (%d, %d) outside (%d, %d)", r,
             img[r], slot[r], B, h->cfg.max_det);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  const int nc = std::max(h->cfg.num_classes, 1);
  if (R > 0) {
    LP_HIP(hipMemcpy(h->d_probs.p, probs, (size_t)R * nc * 4, hipMemcpyHostToDevice));
    LP_HIP(hipMemcpy(h->d_roi_img.p, img, (size_t)R * 4, hipMemcpyHostToDevice));
    LP_HIP(hipMemcpy(h->d_roi_slot.p, slot, (size_t)R * 4, hipMemcpyHostToDevice));
  }
  const int total[2] = {R, R};
  LP_HIP(hipMemcpy(h->d_roi_total.p, total, sizeof(total), hipMemcpyHostToDevice));
  lp_topk* d_out = h->d_topk.as<lp_topk>();
  launch_topk_clear(d_out, B * h->cfg.max_det, h->stream);
  RoiTable tab = h->roi_table();
  TopkArgs a;
  a.probs = h->d_probs.as<float>(); a.total = tab.total; a.roi_img = tab.img; a.roi_slot = tab.slot; a.out = d_out;
  a.nc = nc; a.k = h->topk_k; a.B = B; a.max_det = h->cfg.max_det; a.cap = std::min(h->max_rois, B * h->cfg.max_det);
  launch_topk_select(a, h->stream);
  LP_HIP(hipMemcpyAsync(out, d_out, (size_t)B * h->cfg.max_det * sizeof(lp_topk), hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

}  // extern "C"
