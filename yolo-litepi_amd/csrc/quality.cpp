// Crop quality per detection (lp_quality_*, lp_inventory_set_rank, lp_test_quality; include/litepi.h).  The handle state is in
// handle.h, the launches the run families add while quality is on in pipeline.cpp (enqueue_quality), the rule in
// quality_measure.h, the inventory's use of the records in inventory.cpp / inventory_kernels.hip.
#include "handle.h"
#include "quality_measure.h"

using namespace lp;

static_assert(sizeof(lp_quality) == 32 && sizeof(QualityRec) == sizeof(lp_quality), "lp_quality is 32 bytes");
static_assert(LP_QM_VALID == LP_QUALITY_VALID, "quality_measure.h and litepi.h disagree on the valid flag");

static void check_quality_on(const lp_handle* h) {
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->quality_on, LP_ERR_STATE, "quality is off: call lp_quality_enable first");
}

static bool ranked_by_sharpness(const lp_handle* h) { return h->trk && h->trk->inv && h->trk->inv->rank == LP_RANK_SHARPNESS; }

extern "C" {

int lp_quality_enable(lp_handle* h, int on) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(on == 0 || on == 1, LP_ERR_ARG, "on = %d is not 0 or 1", on);
  if ((on != 0) == h->quality_on) return LP_OK;
  const int S = h->cfg.cls_input;
  LP_CHECK(!on || (S >= 4 && S <= LP_QM_S_MAX && S % 4 == 0), LP_ERR_STATE,
           "quality needs a cls_input that is a multiple of 4 in 4..%d (it is %d): the crops are read 16 bytes at a time", LP_QM_S_MAX, S);
  LP_CHECK(on || !ranked_by_sharpness(h), LP_ERR_STATE, "the inventory ranks by sharpness: set LP_RANK_CONFIG before switching quality off");
  if (on && !h->d_quality.p) {
    LP_HIP(hipSetDevice(h->cfg.device));
    h->d_quality.alloc((size_t)h->cfg.max_batch * h->cfg.max_det * sizeof(lp_quality));
    launch_quality_clear(h->d_quality.as<lp_quality>(), h->cfg.max_batch * h->cfg.max_det, h->stream);   // empty until a call fills them
  }
  h->quality_on = on != 0;
  ++h->geom_ver;   // captured steps hold the other state's launches
  LP_API_END
}

int lp_quality_buffer(lp_handle* h, const void** dev_quality) {
  LP_API_BEGIN
  check_quality_on(h);
  if (dev_quality) *dev_quality = h->d_quality.p;
  LP_API_END
}

int lp_quality_read(lp_handle* h, lp_quality* out, int B) {
  LP_API_BEGIN
  check_quality_on(h);
  LP_CHECK(out, LP_ERR_ARG, "null argument");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipMemcpyAsync(out, h->d_quality.p, (size_t)B * h->cfg.max_det * sizeof(lp_quality), hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

int lp_quality_measure(const uint8_t* rgb, int S, lp_quality* out) {
  LP_API_BEGIN
  LP_CHECK(rgb && out, LP_ERR_ARG, "null argument");
  LP_CHECK(S >= LP_QM_S_MIN && S <= LP_QM_S_MAX, LP_ERR_ARG, "S = %d outside %d..%d", S, LP_QM_S_MIN, LP_QM_S_MAX);
  QualityRec r;
  qm_measure_crop(rgb, S, &r);
  memcpy(out, &r, sizeof(r));
  LP_API_END
}

int lp_inventory_set_rank(lp_handle* h, int rank) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk && h->trk->inv, LP_ERR_STATE, "no inventory: call lp_inventory_create first");
  LP_CHECK(rank == LP_RANK_CONFIG || rank == LP_RANK_SHARPNESS, LP_ERR_ARG, "rank %d is no lp_rank", rank);
  LP_CHECK(rank != LP_RANK_SHARPNESS || h->quality_on, LP_ERR_STATE, "LP_RANK_SHARPNESS needs quality on: call lp_quality_enable first");
  h->trk->inv->rank = rank;   // host state read when the next inventory call is enqueued
  LP_API_END
}

int lp_test_quality(lp_handle* h, int B, lp_quality* out) {
  LP_API_BEGIN
  check_quality_on(h);
  LP_CHECK(out, LP_ERR_ARG, "null argument");
  LP_CHECK(B >= 1 && B <= h->cfg.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, h->cfg.max_batch);
  LP_HIP(hipSetDevice(h->cfg.device));
  launch_quality_clear(h->d_quality.as<lp_quality>(), B * h->cfg.max_det, h->stream);
  launch_quality_measure(quality_args(h, B), h->stream);
  LP_HIP(hipMemcpyAsync(out, h->d_quality.p, (size_t)B * h->cfg.max_det * sizeof(lp_quality), hipMemcpyDeviceToHost, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

}  // extern "C"
