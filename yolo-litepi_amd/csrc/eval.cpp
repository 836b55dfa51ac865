// Device-side evaluation (lp_eval_*; include/litepi.h); the Evaluator itself is in handle.h, the rule in eval_match.h.
#include "eval_match.h"
#include "handle.h"

using namespace lp;

extern "C" {

void lp_eval_default_config(lp_eval_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->max_gt = 64; c->max_rows = 1 << 20; c->n_thr = 10;
  // np.arange(0.5, 1.0, 0.05)'s bit patterns: numpy steps by (start + step) - start, which is not 0.05
  const double delta = (0.5 + 0.05) - 0.5;
  for (int j = 0; j < 10; ++j) c->thr[j] = 0.5 + j * delta;
}

static void check_eval_config(const lp_eval_config* c) {
  LP_CHECK(c, LP_ERR_ARG, "null evaluator configuration");
  LP_CHECK(c->max_gt >= 1 && c->max_gt <= LP_EVAL_MAX_GT, LP_ERR_ARG, "max_gt %d outside 1..%d", c->max_gt, LP_EVAL_MAX_GT);
  LP_CHECK(c->max_rows >= 1, LP_ERR_ARG, "max_rows %d is below 1", c->max_rows);
  LP_CHECK(c->n_thr >= 1 && c->n_thr <= LP_EVAL_MAX_THR, LP_ERR_ARG, "n_thr %d outside 1..%d", c->n_thr, LP_EVAL_MAX_THR);
  for (int j = 0; j < c->n_thr; ++j) LP_CHECK(c->thr[j] == c->thr[j], LP_ERR_ARG, "thr[%d] is not a number", j);
  LP_CHECK(c->reserved0 == 0, LP_ERR_ARG, "a reserved word of lp_eval_config is not zero");
  for (int r : c->reserved) LP_CHECK(r == 0, LP_ERR_ARG, "a reserved word of lp_eval_config is not zero");
}

int lp_eval_config_check(const lp_eval_config* cfg) {
  LP_API_BEGIN
  check_eval_config(cfg);
  LP_API_END
}

int lp_eval_match(const lp_det* dets, int P, const lp_gt* gts, int G, const double* thr, int n_thr, lp_match_rec* out) {
  LP_API_BEGIN
  LP_CHECK(P >= 0 && G >= 0, LP_ERR_ARG, "negative count (P %d, G %d)", P, G);
  LP_CHECK(n_thr >= 1 && n_thr <= LP_EVAL_MAX_THR && thr, LP_ERR_ARG, "n_thr %d outside 1..%d, or no thresholds", n_thr, LP_EVAL_MAX_THR);
  LP_CHECK((P == 0 || (dets && out)) && (G == 0 || gts), LP_ERR_ARG, "null argument");
  eval_match_frame(dets, P, gts, G, thr, n_thr, out);
  LP_API_END
}

int lp_eval_destroy(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (h->evl) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));
    h->evl.reset();
  }
  LP_API_END
}

int lp_eval_create(lp_handle* h, const lp_eval_config* cfg) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  check_eval_config(cfg);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));   // a replaced evaluator may still be in use
  std::unique_ptr<Evaluator> e(new Evaluator());
  e->cfg = *cfg;
  e->nc = std::max(h->cfg.num_classes, 1);
  e->max_det = h->cfg.max_det;
  e->max_batch = h->cfg.max_batch;
  e->state.alloc(sizeof(EvalState) + (size_t)e->nc * sizeof(int));
  e->thr.alloc(LP_EVAL_MAX_THR * sizeof(double));
  LP_HIP(hipMemcpy(e->thr.p, cfg->thr, LP_EVAL_MAX_THR * sizeof(double), hipMemcpyHostToDevice));
  e->log.alloc((size_t)cfg->max_rows * sizeof(lp_eval_row));
  e->gts_off = ((size_t)e->max_batch * sizeof(EvalFrame) + 31) & ~(size_t)31;
  e->ring.create(e->gts_off + (size_t)e->max_batch * cfg->max_gt * sizeof(lp_gt));
  h->evl = std::move(e);
  LP_API_END
}

int lp_eval_reset(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->evl, LP_ERR_STATE, "no evaluator: call lp_eval_create first");
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipMemsetAsync(h->evl->state.p, 0, h->evl->state.bytes, h->stream));
  LP_API_END
}

// every argument error before anything is enqueued
static void check_eval_call(lp_handle* h, int B, const lp_gt* gts, const int* gt_counts) {
  LP_CHECK(h->evl, LP_ERR_STATE, "no evaluator: call lp_eval_create first");
  const Evaluator& e = *h->evl;
  LP_CHECK(B >= 1 && B <= e.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, e.max_batch);
  LP_CHECK(gt_counts, LP_ERR_ARG, "null argument");
  for (int b = 0; b < B; ++b) {
    LP_CHECK(gt_counts[b] >= 0 && gt_counts[b] <= e.cfg.max_gt, LP_ERR_ARG, "gt_counts[%d] = %d outside 0..%d", b, gt_counts[b], e.cfg.max_gt);
    LP_CHECK(gt_counts[b] == 0 || gts, LP_ERR_ARG, "null argument");
    for (int g = 0; g < gt_counts[b]; ++g) {
      const int c = gts[(size_t)b * e.cfg.max_gt + g].cls;
      LP_CHECK(c >= 0 && c < e.nc, LP_ERR_ARG, "ground truth %d of frame %d has class %d outside 0..%d", g, b, c, e.nc - 1);
    }
  }
}

// behind check_eval_call: the alignment check, then the plan upload and the two launches on the handle's stream
static void enqueue_eval(lp_handle* h, const void* dev_dets, const void* dev_counts, int B, const lp_gt* gts, const int* gt_counts,
                         void* dev_matches) {
  Evaluator& e = *h->evl;
  LP_CHECK(((uintptr_t)dev_dets | (uintptr_t)dev_matches) % 16 == 0 && (uintptr_t)dev_counts % 4 == 0, LP_ERR_ARG,
           "the record buffers must be 16-byte aligned");
  LP_HIP(hipSetDevice(h->cfg.device));
  // a HIP error thrown between acquire and release leaves the slot unmarked, not un-advanced (ring_slots.h): nothing waits on it
  const PlanRing::Slot rs = e.ring.acquire();
  EvalFrame* frames = static_cast<EvalFrame*>(rs.host);
  lp_gt* packed = reinterpret_cast<lp_gt*>(static_cast<char*>(rs.host) + e.gts_off);
  int total = 0;
  for (int b = 0; b < B; ++b) {
    frames[b] = EvalFrame{total, gt_counts[b]};
    if (gt_counts[b] > 0) memcpy(packed + total, gts + (size_t)b * e.cfg.max_gt, (size_t)gt_counts[b] * sizeof(lp_gt));
    total += gt_counts[b];
  }
  e.ring.upload(rs, e.gts_off + (size_t)total * sizeof(lp_gt), h->stream);
  EvalArgs a;
  a.dets = static_cast<const lp_det*>(dev_dets); a.counts = static_cast<const int*>(dev_counts); a.matches = static_cast<lp_match_rec*>(dev_matches);
  a.frames = static_cast<const EvalFrame*>(rs.dev);
  a.gts = reinterpret_cast<const lp_gt*>(static_cast<const char*>(rs.dev) + e.gts_off);
  a.thr = e.thr.as<double>();
  a.state = e.state.as<EvalState>(); a.gt_per_class = reinterpret_cast<int*>(e.state.as<char>() + sizeof(EvalState));
  a.log = e.log.as<lp_eval_row>();
  a.B = B; a.max_det = e.max_det; a.n_thr = e.cfg.n_thr; a.max_rows = e.cfg.max_rows; a.nc = e.nc;
  launch_eval(a, h->stream);
  e.ring.release(rs, h->stream);
}

int lp_eval_device(lp_handle* h, const void* dev_dets, const void* dev_counts, int B, const lp_gt* gts, const int* gt_counts,
                   void* dev_matches) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->evl, LP_ERR_STATE, "no evaluator: call lp_eval_create first");
  LP_CHECK(dev_dets && dev_counts, LP_ERR_ARG, "null argument");
  check_eval_call(h, B, gts, gt_counts);
  enqueue_eval(h, dev_dets, dev_counts, B, gts, gt_counts, dev_matches);
  LP_API_END
}

int lp_eval(lp_handle* h, const lp_det* dets, const int* counts, int B, const lp_gt* gts, const int* gt_counts, lp_match_rec* matches) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->evl, LP_ERR_STATE, "no evaluator: call lp_eval_create first");
  LP_CHECK(dets && counts, LP_ERR_ARG, "null argument");
  check_eval_call(h, B, gts, gt_counts);   // every argument error before the first copy is enqueued
  Evaluator& e = *h->evl;
  LP_HIP(hipSetDevice(h->cfg.device));
  const size_t cap = (size_t)e.max_batch * e.max_det, used = (size_t)B * e.max_det;
  if (!e.d_dets.p) {
    e.d_dets.alloc(cap * sizeof(lp_det));
    e.d_counts.alloc((size_t)e.max_batch * sizeof(int));
    e.d_matches.alloc(cap * sizeof(lp_match_rec));
  }
  LP_HIP(hipMemcpyAsync(e.d_dets.p, dets, used * sizeof(lp_det), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(e.d_counts.p, counts, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));   // the sources are the caller's pageable memory
  enqueue_eval(h, e.d_dets.p, e.d_counts.p, B, gts, gt_counts, e.d_matches.p);
  for (int b = 0; matches && b < B; ++b) {   // only the first count[b] records of a frame are results: nothing else is copied or written
    const int n = std::min(std::max(counts[b], 0), e.max_det);
    if (n > 0)
      LP_HIP(hipMemcpyAsync(matches + (size_t)b * e.max_det, e.d_matches.as<lp_match_rec>() + (size_t)b * e.max_det, (size_t)n * sizeof(lp_match_rec),
                            hipMemcpyDeviceToHost, h->stream));
  }
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

int lp_eval_drain(lp_handle* h, lp_eval_row* rows, int cap, int* n, int* gt_per_class, int* frames, int* dropped) {
  LP_API_BEGIN
  LP_CHECK(h && n, LP_ERR_ARG, "null argument");
  LP_CHECK(h->evl, LP_ERR_STATE, "no evaluator: call lp_eval_create first");
  Evaluator& e = *h->evl;
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  std::vector<char> st(e.state.bytes);
  LP_HIP(hipMemcpy(st.data(), e.state.p, st.size(), hipMemcpyDeviceToHost));
  EvalState s;
  memcpy(&s, st.data(), sizeof(s));
  const long long in_log = std::min<long long>(std::max<long long>(s.head, 0), e.cfg.max_rows);
  *n = (int)in_log;
  if (frames) *frames = s.frames;
  if (dropped) *dropped = (int)std::min<long long>(s.dropped, INT32_MAX);
  if (gt_per_class) memcpy(gt_per_class, st.data() + sizeof(EvalState), (size_t)e.nc * sizeof(int));
  if (!rows) return LP_OK;
  LP_CHECK(cap >= *n, LP_ERR_ARG, "%d rows do not fit cap = %d", *n, cap);
  if (in_log > 0) LP_HIP(hipMemcpy(rows, e.log.p, (size_t)in_log * sizeof(lp_eval_row), hipMemcpyDeviceToHost));
  LP_API_END
}

}  // extern "C"
