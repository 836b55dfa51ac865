// Sign tracking (lp_tracker_*, lp_track*; include/litepi.h); the Tracker itself is in handle.h.
#include "handle.h"

using namespace lp;

extern "C" {

void lp_track_default_config(lp_track_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->n_streams = 1; c->max_tracks = 64; c->iou_match = 0.3f; c->max_age = 5; c->min_hits = 3; c->new_conf = 0.f;
  c->vote_decay = 1.f; c->class_gate = 1; c->motion = 1;
}

static void check_track_config(const lp_track_config* c) {
  LP_CHECK(c, LP_ERR_ARG, "null tracker configuration");
  LP_CHECK(c->n_streams >= 1 && c->n_streams <= 1024, LP_ERR_ARG, "n_streams %d outside 1..1024", c->n_streams);
  LP_CHECK(c->max_tracks >= 1 && c->max_tracks <= 256, LP_ERR_ARG, "max_tracks %d outside 1..256", c->max_tracks);
  LP_CHECK(c->iou_match >= 0.f && c->iou_match < 1.f, LP_ERR_ARG, "iou_match %g outside [0, 1)", c->iou_match);
  LP_CHECK(c->max_age >= 0, LP_ERR_ARG, "max_age %d is negative", c->max_age);
  LP_CHECK(c->min_hits >= 1, LP_ERR_ARG, "min_hits %d is below 1", c->min_hits);
  LP_CHECK(c->new_conf == c->new_conf, LP_ERR_ARG, "new_conf is not a number");
  LP_CHECK(c->vote_decay > 0.f && c->vote_decay <= 1.f, LP_ERR_ARG, "vote_decay %g outside (0, 1]", c->vote_decay);
  LP_CHECK(c->class_gate == 0 || c->class_gate == 1, LP_ERR_ARG, "class_gate %d is not 0 or 1", c->class_gate);
  LP_CHECK(c->motion == 0 || c->motion == 1, LP_ERR_ARG, "motion %d is not 0 or 1", c->motion);
  for (int r : c->reserved) LP_CHECK(r == 0, LP_ERR_ARG, "a reserved word of lp_track_config is not zero");
}

int lp_track_config_check(const lp_track_config* cfg) {
  LP_API_BEGIN
  check_track_config(cfg);
  LP_API_END
}

int lp_tracker_destroy(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (h->trk) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));
    h->trk.reset();
  }
  LP_API_END
}

int lp_tracker_create(lp_handle* h, const lp_track_config* cfg) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  check_track_config(cfg);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));   // a replaced tracker may still be in use
  std::unique_ptr<Tracker> t(new Tracker());
  t->cfg = *cfg;
  t->nc = std::max(h->cfg.num_classes, 1);
  t->max_det = h->cfg.max_det;
  t->max_batch = h->cfg.max_batch;
  const size_t S = cfg->n_streams, T = cfg->max_tracks;
  t->table.alloc(S * T * sizeof(TrackSlot));
  t->acc.alloc(S * T * t->nc * sizeof(float));
  std::vector<TrackHead> heads(S, TrackHead{1, 0, {0, 0}});
  t->heads.alloc(S * sizeof(TrackHead));
  LP_HIP(hipMemcpy(t->heads.p, heads.data(), S * sizeof(TrackHead), hipMemcpyHostToDevice));
  if (t->max_det > LP_TRACK_KEY_LDS) t->scratch.alloc((size_t)t->max_batch * 2 * t->max_det * sizeof(unsigned), false);
  t->ring.create((size_t)t->max_batch * (sizeof(TrackJob) + sizeof(int)));
  h->trk = std::move(t);
  LP_API_END
}

int lp_tracker_reset(lp_handle* h, int stream) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  Tracker& t = *h->trk;
  LP_CHECK(stream >= -1 && stream < t.cfg.n_streams, LP_ERR_ARG, "stream %d outside -1..%d", stream, t.cfg.n_streams - 1);
  LP_HIP(hipSetDevice(h->cfg.device));
  launch_track_reset(t.table.as<TrackSlot>(), t.cfg.max_tracks, stream < 0 ? 0 : stream, stream < 0 ? t.cfg.n_streams : 1, h->stream);
  LP_API_END
}

// validates everything, then enqueues the plan upload and the launch on the handle's stream
static void check_track_call(lp_handle* h, int B, const int* stream_ids) {
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  const Tracker& t = *h->trk;
  LP_CHECK(B >= 1 && B <= t.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, t.max_batch);
  check_stream_ids(t, B, stream_ids);
}

// dev_topk: null for the vote on (cls_class, cls_conf), else the [B * max_det] lp_topk records of the distribution vote
static void enqueue_track(lp_handle* h, const void* dev_dets, const void* dev_counts, int B, const int* stream_ids, void* dev_tracks,
                          const void* dev_topk = nullptr) {
  check_track_call(h, B, stream_ids);
  Tracker& t = *h->trk;
  LP_CHECK(((uintptr_t)dev_dets | (uintptr_t)dev_tracks | (uintptr_t)dev_topk) % 16 == 0 && (uintptr_t)dev_counts % 4 == 0, LP_ERR_ARG,
           "the record buffers must be 16-byte aligned");
  LP_HIP(hipSetDevice(h->cfg.device));
  const PlanRing::Slot rs = t.ring.acquire();
  const int n_jobs = plan_stream_jobs(static_cast<int*>(rs.host), t.max_batch, B, stream_ids);
  const int* dslot = static_cast<const int*>(rs.dev);
  t.ring.upload(rs, t.ring.slot_bytes, h->stream);
  TrackArgs a;
  a.dets = static_cast<const lp_det*>(dev_dets); a.counts = static_cast<const int*>(dev_counts); a.out = static_cast<TrackRec*>(dev_tracks);
  a.jobs = reinterpret_cast<const TrackJob*>(dslot); a.frames = dslot + (size_t)t.max_batch * (sizeof(TrackJob) / sizeof(int));
  a.table = t.table.as<TrackSlot>(); a.heads = t.heads.as<TrackHead>(); a.acc = t.acc.as<float>(); a.scratch = t.scratch.as<unsigned>();
  a.max_det = t.max_det; a.T = t.cfg.max_tracks; a.nc = t.nc; a.iou_match = t.cfg.iou_match; a.max_age = t.cfg.max_age;
  a.min_hits = t.cfg.min_hits; a.new_conf = t.cfg.new_conf; a.decay = t.cfg.vote_decay; a.class_gate = t.cfg.class_gate; a.motion = t.cfg.motion;
  a.topk = static_cast<const lp_topk*>(dev_topk);
  launch_track(a, n_jobs, h->stream);
  t.ring.release(rs, h->stream);
}

int lp_track_device(lp_handle* h, const void* dev_dets, const void* dev_counts, int B, const int* stream_ids, void* dev_tracks) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  LP_CHECK(dev_dets && dev_counts && dev_tracks, LP_ERR_ARG, "null argument");
  enqueue_track(h, dev_dets, dev_counts, B, stream_ids, dev_tracks);
  LP_API_END
}

int lp_track_topk_device(lp_handle* h, const void* dev_dets, const void* dev_counts, const void* dev_topk, int B, const int* stream_ids,
                         void* dev_tracks) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  LP_CHECK(dev_dets && dev_counts && dev_topk && dev_tracks, LP_ERR_ARG, "null argument");
  enqueue_track(h, dev_dets, dev_counts, B, stream_ids, dev_tracks, dev_topk);
  LP_API_END
}

// lp_track and lp_track_topk (topk != null): upload, the device call, download
static void track_host(lp_handle* h, const lp_det* dets, const int* counts, const lp_topk* topk, int B, const int* stream_ids,
                       struct lp_track* tracks) {
  check_track_call(h, B, stream_ids);   // every argument error before the first copy is enqueued
  Tracker& t = *h->trk;
  LP_HIP(hipSetDevice(h->cfg.device));
  const size_t cap = (size_t)t.max_batch * t.max_det, used = (size_t)B * t.max_det;
  if (!t.d_dets.p) {
    t.d_dets.alloc(cap * sizeof(lp_det));
    t.d_counts.alloc((size_t)t.max_batch * sizeof(int));
    t.d_tracks.alloc(cap * sizeof(TrackRec));
  }
  if (topk && !t.d_topk.p) t.d_topk.alloc(cap * sizeof(lp_topk));
  LP_HIP(hipMemcpyAsync(t.d_dets.p, dets, used * sizeof(lp_det), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(t.d_counts.p, counts, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (topk) LP_HIP(hipMemcpyAsync(t.d_topk.p, topk, used * sizeof(lp_topk), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));   // the sources are the caller's pageable memory
  enqueue_track(h, t.d_dets.p, t.d_counts.p, B, stream_ids, t.d_tracks.p, topk ? t.d_topk.p : nullptr);
  for (int b = 0; b < B; ++b) {   // only the first count[b] records of a frame are results: nothing else is copied or written
    const int n = std::min(std::max(counts[b], 0), t.max_det);
    if (n > 0)
      LP_HIP(hipMemcpyAsync(tracks + (size_t)b * t.max_det, t.d_tracks.as<TrackRec>() + (size_t)b * t.max_det, (size_t)n * sizeof(TrackRec),
                            hipMemcpyDeviceToHost, h->stream));
  }
  LP_HIP(hipStreamSynchronize(h->stream));
}

int lp_track(lp_handle* h, const lp_det* dets, const int* counts, int B, const int* stream_ids, struct lp_track* tracks) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  LP_CHECK(dets && counts && tracks, LP_ERR_ARG, "null argument");
  track_host(h, dets, counts, nullptr, B, stream_ids, tracks);
  LP_API_END
}

int lp_track_topk(lp_handle* h, const lp_det* dets, const int* counts, const lp_topk* topk, int B, const int* stream_ids,
                  struct lp_track* tracks) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  LP_CHECK(dets && counts && topk && tracks, LP_ERR_ARG, "null argument");
  track_host(h, dets, counts, topk, B, stream_ids, tracks);
  LP_API_END
}

int lp_tracker_snapshot(lp_handle* h, int stream, lp_track_state* out, int cap, int* n, float* acc, int* next_id, int* overflow) {
  LP_API_BEGIN
  LP_CHECK(h && n, LP_ERR_ARG, "null argument");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  Tracker& t = *h->trk;
  LP_CHECK(stream >= 0 && stream < t.cfg.n_streams, LP_ERR_ARG, "stream %d outside 0..%d", stream, t.cfg.n_streams - 1);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  const int T = t.cfg.max_tracks;
  std::vector<TrackSlot> tab(T);
  LP_HIP(hipMemcpy(tab.data(), t.table.as<TrackSlot>() + (size_t)stream * T, (size_t)T * sizeof(TrackSlot), hipMemcpyDeviceToHost));
  TrackHead head;
  LP_HIP(hipMemcpy(&head, t.heads.as<TrackHead>() + stream, sizeof(head), hipMemcpyDeviceToHost));
  if (next_id) *next_id = head.next_id;
  if (overflow) *overflow = head.overflow;
  int live = 0;
  for (const TrackSlot& s : tab) live += s.live != 0;
  *n = live;
  if (!out && !acc) return LP_OK;
  LP_CHECK(cap >= live, LP_ERR_ARG, "%d live tracks do not fit cap = %d", live, cap);
  std::vector<float> rows;
  if (acc) {
    rows.resize((size_t)T * t.nc);
    LP_HIP(hipMemcpy(rows.data(), t.acc.as<float>() + (size_t)stream * T * t.nc, rows.size() * sizeof(float), hipMemcpyDeviceToHost));
  }
  int k = 0;
  for (int s = 0; s < T; ++s) {
    const TrackSlot& q = tab[s];
    if (!q.live) continue;
    if (out) {
      lp_track_state& o = out[k];
      o.slot = s; o.track_id = q.id;
      o.x1 = q.box[0]; o.y1 = q.box[1]; o.x2 = q.box[2]; o.y2 = q.box[3];
      o.vx1 = q.vel[0]; o.vy1 = q.vel[1]; o.vx2 = q.vel[2]; o.vy2 = q.vel[3];
      o.hits = q.hits; o.missed = q.missed; o.age = q.age; o.det_class = q.det_class; o.wsum = q.wsum; o.has_vote = q.has_vote;
    }
    if (acc) memcpy(acc + (size_t)k * t.nc, rows.data() + (size_t)s * t.nc, (size_t)t.nc * sizeof(float));
    ++k;
  }
  LP_API_END
}

}  // extern "C"
