// Sign inventory (lp_inventory_*; include/litepi.h); the Inventory itself is in handle.h, owned by the handle's Tracker.
#include <cmath>

#include "evidence_window.h"
#include "handle.h"

using namespace lp;

static void check_inventory_config(const lp_inventory_config* c) {
  LP_CHECK(c, LP_ERR_ARG, "null inventory configuration");
  LP_CHECK(c->max_signs >= 1 && c->max_signs <= (1 << 20), LP_ERR_ARG, "max_signs %d outside 1..%d", c->max_signs, 1 << 20);
  LP_CHECK(c->keep_crops == 0 || c->keep_crops == 1, LP_ERR_ARG, "keep_crops %d is not 0 or 1", c->keep_crops);
  LP_CHECK(c->best >= LP_BEST_AREA && c->best <= LP_BEST_CLS_CONF, LP_ERR_ARG, "best %d is no lp_best", c->best);
  LP_CHECK(c->min_hits >= 0, LP_ERR_ARG, "min_hits %d is negative", c->min_hits);
  for (int r : c->reserved) LP_CHECK(r == 0, LP_ERR_ARG, "a reserved word of lp_inventory_config is not zero");
}

static Inventory& inventory_of(lp_handle* h) {
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  LP_CHECK(h->trk->inv, LP_ERR_STATE, "no inventory: call lp_inventory_create first");
  return *h->trk->inv;
}

// everything but the records, the plan and the crops of a call
static InvArgs base_args(const lp_handle* h) {
  const Tracker& t = *h->trk;
  const Inventory& v = *t.inv;
  InvArgs a;
  memset(&a, 0, sizeof(a));
  a.entries = v.entries.as<InvEntry>(); a.frame_no = v.frame_no.as<int>(); a.head = v.head.as<InvHead>(); a.log = v.log.as<lp_sign>();
  a.log_crops = v.log_crops.as<uint8_t>(); a.gallery = v.gallery.as<uint8_t>(); a.roi_of = v.roi_of.as<int>();
  a.max_rois = h->max_rois; a.max_det = t.max_det; a.T = t.cfg.max_tracks; a.max_age = t.cfg.max_age; a.min_hits = v.min_hits;
  a.best = v.cfg.best; a.max_signs = v.cfg.max_signs; a.crop_bytes = v.crop_bytes;
  a.quality = v.rank == LP_RANK_SHARPNESS ? h->d_quality.as<lp_quality>() : nullptr;   // lp_inventory_set_rank
  return a;
}

static void check_evidence_config(const lp_evidence_config* c) {
  LP_CHECK(c, LP_ERR_ARG, "null evidence configuration");
  LP_CHECK(c->size >= 32 && c->size <= 256 && c->size % 16 == 0, LP_ERR_ARG, "size %d is no multiple of 16 in 32..256", c->size);
  LP_CHECK(c->scale >= 1.0f && c->scale <= 16.0f, LP_ERR_ARG, "scale %g outside 1..16", (double)c->scale);   // false for a NaN
  for (int r : c->reserved) LP_CHECK(r == 0, LP_ERR_ARG, "a reserved word of lp_evidence_config is not zero");
}

static Evidence& evidence_of(lp_handle* h) {
  Inventory& v = inventory_of(h);
  LP_CHECK(v.evid, LP_ERR_STATE, "no evidence store: call lp_evidence_create first");
  return *v.evid;
}

// everything but the frames of a call
static EvArgs evidence_args(const lp_handle* h) {
  const Tracker& t = *h->trk;
  const Evidence& e = *t.inv->evid;
  EvArgs a;
  memset(&a, 0, sizeof(a));
  a.win = e.win.as<int>(); a.log_win = e.log_win.as<int>(); a.gallery = e.gallery.as<uint8_t>(); a.log_pics = e.log_pics.as<uint8_t>();
  a.jobs = e.jobs.as<EvJob>(); a.n_jobs = e.n_jobs.as<int>();
  a.cap_jobs = t.cfg.n_streams * t.cfg.max_tracks + t.max_batch * t.max_det; a.E = e.cfg.size; a.scale = e.cfg.scale;
  return a;
}

// no open entry keeps LP_SIGN_HAS_EVIDENCE (the store that held its picture is going or gone); the stream is idle
static void clear_evidence_flags(lp_handle* h, Inventory& v) {
  const size_t n = (size_t)h->trk->cfg.n_streams * h->trk->cfg.max_tracks;
  std::vector<InvEntry> ent(n);
  LP_HIP(hipMemcpy(ent.data(), v.entries.p, n * sizeof(InvEntry), hipMemcpyDeviceToHost));
  bool any = false;
  for (InvEntry& e : ent)
    if (e.sign.flags & LP_SIGN_HAS_EVIDENCE) { e.sign.flags &= ~LP_SIGN_HAS_EVIDENCE; any = true; }
  if (any) LP_HIP(hipMemcpy(v.entries.p, ent.data(), n * sizeof(InvEntry), hipMemcpyHostToDevice));
}

static void check_inventory_call(lp_handle* h, int B, const int* stream_ids, int crops) {
  const Inventory& v = inventory_of(h);
  const Tracker& t = *h->trk;
  LP_CHECK(B >= 1 && B <= t.max_batch, LP_ERR_ARG, "batch %d outside 1..%d", B, t.max_batch);
  check_stream_ids(t, B, stream_ids);
  LP_CHECK(crops == 0 || crops == 1, LP_ERR_ARG, "crops %d is not 0 or 1", crops);
  LP_CHECK(!crops || v.cfg.keep_crops, LP_ERR_ARG, "crops = 1 on an inventory created with keep_crops = 0");
  LP_CHECK(crops || v.rank != LP_RANK_SHARPNESS, LP_ERR_ARG,
           "crops = 0 under LP_RANK_SHARPNESS: the quality records describe the last pipeline call, which is what crops = 1 asserts");
  LP_CHECK(!crops || !v.evid || (h->last_frames && h->last_fgeom && h->last_nframes >= B), LP_ERR_STATE,
           "crops = 1 with an evidence store: the handle remembers %d frames of its last pipeline call, this call has %d", h->last_nframes, B);
}

// validates everything, then enqueues the plan upload and the launches on the handle's stream
static void enqueue_inventory(lp_handle* h, const void* dev_dets, const void* dev_counts, const void* dev_tracks, int B, const int* stream_ids,
                              int crops) {
  check_inventory_call(h, B, stream_ids, crops);
  Tracker& t = *h->trk;
  Inventory& v = *t.inv;
  LP_CHECK(((uintptr_t)dev_dets | (uintptr_t)dev_tracks) % 16 == 0 && (uintptr_t)dev_counts % 4 == 0, LP_ERR_ARG,
           "the record buffers must be 16-byte aligned");
  LP_HIP(hipSetDevice(h->cfg.device));
  const PlanRing::Slot rs = v.ring.acquire();
  const int n_jobs = plan_stream_jobs(static_cast<int*>(rs.host), t.max_batch, B, stream_ids);   // the tracker's plan
  const int* dslot = static_cast<const int*>(rs.dev);
  v.ring.upload(rs, v.ring.slot_bytes, h->stream);
  InvArgs a = base_args(h);
  a.dets = static_cast<const lp_det*>(dev_dets); a.counts = static_cast<const int*>(dev_counts); a.tracks = static_cast<const TrackRec*>(dev_tracks);
  a.jobs = reinterpret_cast<const TrackJob*>(dslot); a.frames = dslot + (size_t)t.max_batch * (sizeof(TrackJob) / sizeof(int));
  a.B = B;
  if (crops) {
    const RoiTable tab = h->roi_table();
    a.roi_rgb = h->d_roi_rgb.as<uint8_t>(); a.roi_total = tab.total; a.roi_img = tab.img; a.roi_slot = tab.slot;
  }
  if (v.evid) {
    EvArgs e = evidence_args(h);
    if (crops) { e.frames = h->last_frames; e.fgeom = h->last_fgeom; }
    launch_inventory_evidence(a, e, n_jobs, h->stream);
  } else {
    launch_inventory(a, n_jobs, h->stream);
  }
  v.ring.release(rs, h->stream);
}

// the first n entries of the log (signs, and their crops when wanted) after a synchronise
static void read_head(lp_handle* h, Inventory& v, int* n, int* dropped) {
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  InvHead head;
  LP_HIP(hipMemcpy(&head, v.head.p, sizeof(head), hipMemcpyDeviceToHost));
  *n = std::min(std::max(head.logged, 0), v.cfg.max_signs);
  if (dropped) *dropped = std::max(head.logged - v.cfg.max_signs, 0);
}

// lp_inventory_drain and lp_inventory_drain_evidence (evidence, windows: only with a store; either may be null)
static void drain(lp_handle* h, lp_sign* out, uint8_t* crops, uint8_t* evidence, int* windows, int cap, int* n, int* dropped) {
  Inventory& v = inventory_of(h);
  LP_CHECK(n, LP_ERR_ARG, "null argument");
  LP_CHECK(!crops || v.cfg.keep_crops, LP_ERR_ARG, "crops asked of an inventory created with keep_crops = 0");
  read_head(h, v, n, dropped);
  if (!out) return;
  LP_CHECK(cap >= *n, LP_ERR_ARG, "%d logged signs do not fit cap = %d", *n, cap);
  if (*n > 0) {
    LP_HIP(hipMemcpy(out, v.log.p, (size_t)*n * sizeof(lp_sign), hipMemcpyDeviceToHost));
    if (crops) {
      LP_HIP(hipMemcpy(crops, v.log_crops.p, (size_t)*n * v.crop_bytes, hipMemcpyDeviceToHost));
      for (int i = 0; i < *n; ++i)   // a sign without a crop left its place in the log's crop buffer unwritten
        if (!(out[i].flags & LP_SIGN_HAS_CROP)) memset(crops + (size_t)i * v.crop_bytes, 0, v.crop_bytes);
    }
    if (evidence) {
      const size_t pb = v.evid->pic_bytes;
      LP_HIP(hipMemcpy(evidence, v.evid->log_pics.p, (size_t)*n * pb, hipMemcpyDeviceToHost));
      for (int i = 0; i < *n; ++i)   // a sign without a picture left its place in the log's picture buffer unwritten
        if (!(out[i].flags & LP_SIGN_HAS_EVIDENCE)) memset(evidence + (size_t)i * pb, 0, pb);
    }
    if (windows) LP_HIP(hipMemcpy(windows, v.evid->log_win.p, (size_t)*n * 16, hipMemcpyDeviceToHost));   // zeros without a picture
  }
  LP_HIP(hipMemsetAsync(v.head.p, 0, sizeof(InvHead), h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));
}

extern "C" {

void lp_inventory_default_config(lp_inventory_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->max_signs = 4096; c->keep_crops = 1; c->best = LP_BEST_AREA; c->min_hits = 0;
}

int lp_inventory_config_check(const lp_inventory_config* cfg) {
  LP_API_BEGIN
  check_inventory_config(cfg);
  LP_API_END
}

int lp_inventory_destroy(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (h->trk && h->trk->inv) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));
    h->trk->inv.reset();
  }
  LP_API_END
}

int lp_inventory_create(lp_handle* h, const lp_inventory_config* cfg) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  check_inventory_config(cfg);
  LP_CHECK(h->trk, LP_ERR_STATE, "no tracker: call lp_tracker_create first");
  Tracker& t = *h->trk;
  const int S = h->cfg.cls_input;
  LP_CHECK(!cfg->keep_crops || (S > 0 && S % 4 == 0), LP_ERR_ARG, "keep_crops needs a cls_input that is a multiple of 4 (it is %d)", S);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));   // a replaced inventory may still be in use
  std::unique_ptr<Inventory> v(new Inventory());
  v->cfg = *cfg;
  v->min_hits = cfg->min_hits > 0 ? cfg->min_hits : t.cfg.min_hits;
  v->crop_bytes = 3 * S * S;
  const size_t NS = t.cfg.n_streams, T = t.cfg.max_tracks;
  v->entries.alloc(NS * T * sizeof(InvEntry));
  v->frame_no.alloc(NS * sizeof(int));
  v->head.alloc(sizeof(InvHead));
  v->log.alloc((size_t)cfg->max_signs * sizeof(lp_sign));
  if (cfg->keep_crops) {
    v->log_crops.alloc((size_t)cfg->max_signs * v->crop_bytes, false);
    v->gallery.alloc(NS * T * v->crop_bytes, false);
    v->roi_of.alloc((size_t)t.max_batch * t.max_det * sizeof(int));
  }
  v->ring.create((size_t)t.max_batch * (sizeof(TrackJob) + sizeof(int)));
  t.inv = std::move(v);
  LP_API_END
}

int lp_inventory_device(lp_handle* h, const void* dev_dets, const void* dev_counts, const void* dev_tracks, int B, const int* stream_ids,
                        int crops) {
  LP_API_BEGIN
  inventory_of(h);
  LP_CHECK(dev_dets && dev_counts && dev_tracks, LP_ERR_ARG, "null argument");
  enqueue_inventory(h, dev_dets, dev_counts, dev_tracks, B, stream_ids, crops);
  LP_API_END
}

int lp_inventory(lp_handle* h, const lp_det* dets, const int* counts, const struct lp_track* tracks, int B, const int* stream_ids, int crops) {
  LP_API_BEGIN
  Inventory& v = inventory_of(h);
  LP_CHECK(dets && counts && tracks, LP_ERR_ARG, "null argument");
  check_inventory_call(h, B, stream_ids, crops);   // every argument error before the first copy is enqueued
  const Tracker& t = *h->trk;
  LP_HIP(hipSetDevice(h->cfg.device));
  const size_t cap = (size_t)t.max_batch * t.max_det, used = (size_t)B * t.max_det;
  if (!v.d_dets.p) {
    v.d_dets.alloc(cap * sizeof(lp_det));
    v.d_counts.alloc((size_t)t.max_batch * sizeof(int));
    v.d_tracks.alloc(cap * sizeof(TrackRec));
  }
  LP_HIP(hipMemcpyAsync(v.d_dets.p, dets, used * sizeof(lp_det), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(v.d_counts.p, counts, (size_t)B * sizeof(int), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipMemcpyAsync(v.d_tracks.p, tracks, used * sizeof(TrackRec), hipMemcpyHostToDevice, h->stream));
  LP_HIP(hipStreamSynchronize(h->stream));   // the sources are the caller's pageable memory
  enqueue_inventory(h, v.d_dets.p, v.d_counts.p, v.d_tracks.p, B, stream_ids, crops);
  LP_HIP(hipStreamSynchronize(h->stream));
  LP_API_END
}

int lp_inventory_flush(lp_handle* h, int stream) {
  LP_API_BEGIN
  inventory_of(h);
  const Tracker& t = *h->trk;
  LP_CHECK(stream >= -1 && stream < t.cfg.n_streams, LP_ERR_ARG, "stream %d outside -1..%d", stream, t.cfg.n_streams - 1);
  LP_HIP(hipSetDevice(h->cfg.device));
  const int first = stream < 0 ? 0 : stream, n = stream < 0 ? t.cfg.n_streams : 1;
  if (t.inv->evid) launch_inventory_flush_evidence(base_args(h), evidence_args(h), first, n, h->stream);
  else launch_inventory_flush(base_args(h), first, n, h->stream);
  LP_API_END
}

int lp_inventory_drain(lp_handle* h, lp_sign* out, uint8_t* crops, int cap, int* n, int* dropped) {
  LP_API_BEGIN
  inventory_of(h);
  drain(h, out, crops, nullptr, nullptr, cap, n, dropped);
  LP_API_END
}

int lp_inventory_drain_evidence(lp_handle* h, lp_sign* out, uint8_t* crops, uint8_t* evidence, int* windows, int cap, int* n, int* dropped) {
  LP_API_BEGIN
  evidence_of(h);
  drain(h, out, crops, evidence, windows, cap, n, dropped);
  LP_API_END
}


int lp_inventory_open(lp_handle* h, int stream, lp_sign* out, int cap, int* n) {
  LP_API_BEGIN
  Inventory& v = inventory_of(h);
  LP_CHECK(n, LP_ERR_ARG, "null argument");
  const Tracker& t = *h->trk;
  LP_CHECK(stream >= 0 && stream < t.cfg.n_streams, LP_ERR_ARG, "stream %d outside 0..%d", stream, t.cfg.n_streams - 1);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  const int T = t.cfg.max_tracks;
  std::vector<InvEntry> ent(T);
  LP_HIP(hipMemcpy(ent.data(), v.entries.as<InvEntry>() + (size_t)stream * T, (size_t)T * sizeof(InvEntry), hipMemcpyDeviceToHost));
  int open = 0;
  for (const InvEntry& e : ent) open += e.open != 0;
  *n = open;
  if (!out) return LP_OK;
  LP_CHECK(cap >= open, LP_ERR_ARG, "%d open entries do not fit cap = %d", open, cap);
  int k = 0;
  for (const InvEntry& e : ent)
    if (e.open) out[k++] = e.sign;
  LP_API_END
}

void lp_evidence_default_config(lp_evidence_config* c) {
  if (!c) return;
  memset(c, 0, sizeof(*c));
  c->size = 128; c->scale = 2.0f;
}

int lp_evidence_config_check(const lp_evidence_config* cfg) {
  LP_API_BEGIN
  check_evidence_config(cfg);
  LP_API_END
}

int lp_evidence_window(const lp_evidence_config* cfg, int H, int W, const float* box, int* win, int* has) {
  LP_API_BEGIN
  check_evidence_config(cfg);
  LP_CHECK(box && win && has && H >= 1 && W >= 1, LP_ERR_ARG, "bad argument (frame %dx%d)", W, H);
  EvWindow w;
  *has = evidence_window(cfg->scale, H, W, box[0], box[1], box[2], box[3], &w) ? 1 : 0;
  win[0] = w.x; win[1] = w.y; win[2] = w.w; win[3] = w.h;
  LP_API_END
}

int lp_evidence_destroy(lp_handle* h) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  if (h->trk && h->trk->inv && h->trk->inv->evid) {
    LP_HIP(hipSetDevice(h->cfg.device));
    LP_HIP(hipStreamSynchronize(h->stream));
    clear_evidence_flags(h, *h->trk->inv);
    h->trk->inv->evid.reset();
  }
  LP_API_END
}

int lp_evidence_create(lp_handle* h, const lp_evidence_config* cfg) {
  LP_API_BEGIN
  LP_CHECK(h, LP_ERR_ARG, "null handle");
  check_evidence_config(cfg);
  Inventory& v = inventory_of(h);
  LP_CHECK(v.cfg.keep_crops, LP_ERR_ARG, "an evidence store needs an inventory created with keep_crops = 1");
  const Tracker& t = *h->trk;
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));   // a replaced store may still be in use
  std::unique_ptr<Evidence> e(new Evidence());
  e->cfg = *cfg;
  e->pic_bytes = (size_t)3 * cfg->size * cfg->size;
  const size_t slots = (size_t)t.cfg.n_streams * t.cfg.max_tracks;
  e->gallery.alloc(slots * e->pic_bytes, false);
  e->log_pics.alloc((size_t)v.cfg.max_signs * e->pic_bytes, false);
  e->win.alloc(slots * 16);
  e->log_win.alloc((size_t)v.cfg.max_signs * 16);
  e->jobs.alloc((slots + (size_t)t.max_batch * t.max_det) * sizeof(EvJob));
  e->n_jobs.alloc(sizeof(int));
  clear_evidence_flags(h, v);
  v.evid = std::move(e);
  LP_API_END
}

int lp_evidence_open(lp_handle* h, int stream, uint8_t* evidence, int* windows, int cap, int* n) {
  LP_API_BEGIN
  Evidence& e = evidence_of(h);
  Inventory& v = *h->trk->inv;
  LP_CHECK(n, LP_ERR_ARG, "null argument");
  const Tracker& t = *h->trk;
  LP_CHECK(stream >= 0 && stream < t.cfg.n_streams, LP_ERR_ARG, "stream %d outside 0..%d", stream, t.cfg.n_streams - 1);
  LP_HIP(hipSetDevice(h->cfg.device));
  LP_HIP(hipStreamSynchronize(h->stream));
  const int T = t.cfg.max_tracks;
  std::vector<InvEntry> ent(T);
  LP_HIP(hipMemcpy(ent.data(), v.entries.as<InvEntry>() + (size_t)stream * T, (size_t)T * sizeof(InvEntry), hipMemcpyDeviceToHost));
  int open = 0;
  for (const InvEntry& en : ent) open += en.open != 0;
  *n = open;
  if (!evidence && !windows) return LP_OK;
  LP_CHECK(cap >= open, LP_ERR_ARG, "%d open entries do not fit cap = %d", open, cap);
  int k = 0;
  for (int s = 0; s < T; ++s) {
    if (!ent[s].open) continue;
    const bool pic = (ent[s].sign.flags & LP_SIGN_HAS_EVIDENCE) != 0;
    const size_t slot = (size_t)stream * T + s;
    if (evidence) {
      if (pic) LP_HIP(hipMemcpy(evidence + (size_t)k * e.pic_bytes, e.gallery.as<uint8_t>() + slot * e.pic_bytes, e.pic_bytes, hipMemcpyDeviceToHost));
      else memset(evidence + (size_t)k * e.pic_bytes, 0, e.pic_bytes);
    }
    if (windows) {
      if (pic) LP_HIP(hipMemcpy(windows + 4 * k, e.win.as<int>() + slot * 4, 16, hipMemcpyDeviceToHost));
      else memset(windows + 4 * k, 0, 16);
    }
    ++k;
  }
  LP_API_END
}

}  // extern "C"
