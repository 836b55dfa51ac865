// Sign tracking across the frames of a sequence (the rule is stated in include/litepi.h, lp_track_config).
// The work is sequential over the frames of one stream and over the detections of one frame (each match removes a track
// from the candidates of the next), parallel over the tracks a detection is compared with and over the streams of a call.
// So: ONE WAVE per stream present in the call.  Lane l owns the table slots l, l + 64, l + 128, l + 192; the per-track
// scalars live in LDS for the duration of the call; every decision that needs all tracks (the best track of a detection, the
// next detection in score order, the free-slot list, the birth ranks) is a wave-wide reduction, ballot or prefix count in
// registers.  A single wave needs no barrier to agree on anything; __syncthreads() is used only as the LDS hand-over fence
// between a lane's write and another lane's read (it costs a waitcnt for a one-wave workgroup).
// The vote accumulators [max_tracks, num_classes] stay in HBM: only the rows of this frame's matched and born tracks are
// touched, lanes over classes.
#include "common.h"
#include "kernels.h"

namespace lp {

#define TRK_LANES 64
#define TRK_MAXT 256                  // lp_track_config::max_tracks <= 256
#define TRK_DET_LDS 256               // records of a frame cached in LDS (the rest is re-read from L2 when it is their turn)
#define TRK_KEYS LP_TRACK_KEY_LDS

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct Rec { float x1, y1, x2, y2, conf; int dcls, ccls; float cconf; };

__device__ __forceinline__ Rec unpack_rec(const i32x4 a, const i32x4 b) {
  Rec r;
  r.x1 = __int_as_float(a.x); r.y1 = __int_as_float(a.y); r.x2 = __int_as_float(a.z); r.y2 = __int_as_float(a.w);
  r.conf = __int_as_float(b.x); r.dcls = b.y; r.ccls = b.z; r.cconf = __int_as_float(b.w);
  return r;
}

// descending det_conf == descending key; never 0 (0 means "no detection left")
__device__ __forceinline__ unsigned conf_key(float conf) {
  const unsigned u = __float_as_uint(conf);
  const unsigned k = (u >> 31) ? ~u : (u | 0x80000000u);
  return k ? k : 1u;
}

// nms_suppressed's IoU (nms_dev.h) with the detection as i and the predicted box as j
__device__ __forceinline__ float track_iou(float ix1, float iy1, float ix2, float iy2, float ai, float jx1, float jy1, float jx2, float jy2) {
  const float aj = __fmul_rn(__fsub_rn(jx2, jx1), __fsub_rn(jy2, jy1));
  const float w = fmaxf(0.f, __fsub_rn(fminf(ix2, jx2), fmaxf(ix1, jx1)));
  const float h = fmaxf(0.f, __fsub_rn(fminf(iy2, jy2), fmaxf(iy1, jy1)));
  const float inter = __fmul_rn(w, h);
  return __fdiv_rn(inter, __fadd_rn(__fsub_rn(__fadd_rn(ai, aj), inter), 1e-6f));
}

__device__ __forceinline__ int lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// The distribution vote of lp_track_topk* (include/litepi.h): a detection's lp_topk record, always read from memory at the
// detection's own index (frames beyond TRK_DET_LDS included).
struct TopkVote { int cls[LP_TOPK_MAX]; float prob[LP_TOPK_MAX]; };

__device__ __forceinline__ TopkVote load_topk(const lp_topk* t) {
  const i32x4* p = reinterpret_cast<const i32x4*>(t);
  const i32x4 c0 = p[0], c1 = p[1], q0 = p[2], q1 = p[3];
  TopkVote v;
  v.cls[0] = c0.x; v.cls[1] = c0.y; v.cls[2] = c0.z; v.cls[3] = c0.w; v.cls[4] = c1.x; v.cls[5] = c1.y; v.cls[6] = c1.z; v.cls[7] = c1.w;
  v.prob[0] = __int_as_float(q0.x); v.prob[1] = __int_as_float(q0.y); v.prob[2] = __int_as_float(q0.z); v.prob[3] = __int_as_float(q0.w);
  v.prob[4] = __int_as_float(q1.x); v.prob[5] = __int_as_float(q1.y); v.prob[6] = __int_as_float(q1.z); v.prob[7] = __int_as_float(q1.w);
  return v;
}
__device__ __forceinline__ bool topk_votes(const TopkVote& v, int nc) { return v.cls[0] >= 0 && v.cls[0] < nc; }
// s = 0; for valid j in order: s = s + prob[j]
__device__ __forceinline__ float topk_weight(const TopkVote& v, int nc) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < LP_TOPK_MAX; ++j)
    if (v.cls[j] >= 0 && v.cls[j] < nc) s = __fadd_rn(s, v.prob[j]);
  return s;
}

// TOPK = false: the vote of lp_track* on (cls_class, cls_conf), a.topk is not looked at; TOPK = true: the distribution vote
template <bool TOPK>
__global__ __launch_bounds__(TRK_LANES) void track_kernel(const TrackArgs a) {
  // per-track state of the stream, structure of arrays
  __shared__ float s_box[4][TRK_MAXT], s_vel[4][TRK_MAXT], s_pred[4][TRK_MAXT], s_wsum[TRK_MAXT];
  __shared__ int s_id[TRK_MAXT], s_hits[TRK_MAXT], s_missed[TRK_MAXT], s_age[TRK_MAXT], s_cls[TRK_MAXT], s_vote[TRK_MAXT], s_live[TRK_MAXT];
  __shared__ int s_claimed[TRK_MAXT], s_born[TRK_MAXT], s_free[TRK_MAXT], s_list[TRK_MAXT];
  // per-frame: the cached records, and (frames of up to TRK_KEYS detections) sort key + assignment of every detection
  __shared__ i32x4 s_det[TRK_DET_LDS][2];
  __shared__ unsigned s_key[TRK_KEYS];
  __shared__ int s_asg[TRK_KEYS];

  const int lane = threadIdx.x;
  const TrackJob job = a.jobs[blockIdx.x];
  const int T = a.T, nc = a.nc, max_det = a.max_det;
  const int* frames = a.frames + job.first;
  TrackSlot* tab = a.table + (size_t)job.stream * T;
  float* accs = a.acc + (size_t)job.stream * T * nc;

  // records of the first frame (independent of its count: slot `lane` of a frame always exists in the buffer)
  int b_next = frames[0];
  const bool pf_lane = lane < max_det;
  i32x4 pf0 = {0, 0, 0, 0}, pf1 = {0, 0, 0, 0};
  int n_next = a.counts[b_next];
  if (pf_lane) {
    const i32x4* p = reinterpret_cast<const i32x4*>(a.dets + (size_t)b_next * max_det + lane);
    pf0 = p[0]; pf1 = p[1];
  }

  for (int s = lane; s < T; s += TRK_LANES) {
    const i32x4* p = reinterpret_cast<const i32x4*>(tab + s);
    const i32x4 q0 = p[0], q1 = p[1], q2 = p[2], q3 = p[3];
    s_box[0][s] = __int_as_float(q0.x); s_box[1][s] = __int_as_float(q0.y); s_box[2][s] = __int_as_float(q0.z); s_box[3][s] = __int_as_float(q0.w);
    s_vel[0][s] = __int_as_float(q1.x); s_vel[1][s] = __int_as_float(q1.y); s_vel[2][s] = __int_as_float(q1.z); s_vel[3][s] = __int_as_float(q1.w);
    s_id[s] = q2.x; s_hits[s] = q2.y; s_missed[s] = q2.z; s_age[s] = q2.w;
    s_cls[s] = q3.x; s_wsum[s] = __int_as_float(q3.y); s_vote[s] = q3.z; s_live[s] = q3.w;
  }
  int next_id = a.heads[job.stream].next_id, overflow = a.heads[job.stream].overflow;
  __syncthreads();

  for (int f = 0; f < job.nframes; ++f) {
    const int b = b_next;
    const int n = min(max(n_next, 0), max_det);
    const lp_det* fdets = a.dets + (size_t)b * max_det;
    TrackRec* fout = a.out + (size_t)b * max_det;
    const lp_topk* ftopk = TOPK ? a.topk + (size_t)b * max_det : nullptr;
    // sort key + assignment: LDS, or the job's slice of the scratch buffer for a frame of more than TRK_KEYS detections
    unsigned* keys = s_key;
    int* asg = s_asg;
    if (n > TRK_KEYS) {
      keys = a.scratch + (size_t)blockIdx.x * 2 * max_det;
      asg = reinterpret_cast<int*>(keys + max_det);
    }
    // ---- the frame's records: the prefetched first 64, then the rest
    if (lane < n) {
      s_det[lane][0] = pf0; s_det[lane][1] = pf1;
      keys[lane] = conf_key(__int_as_float(pf1.x));
      asg[lane] = -1;
    }
    for (int i = TRK_LANES + lane; i < n; i += TRK_LANES) {
      const i32x4* p = reinterpret_cast<const i32x4*>(fdets + i);
      const i32x4 r0 = p[0], r1 = p[1];
      if (i < TRK_DET_LDS) { s_det[i][0] = r0; s_det[i][1] = r1; }
      keys[i] = conf_key(__int_as_float(r1.x));
      asg[i] = -1;
    }
    // ---- the next frame's records travel while this frame is matched
    if (f + 1 < job.nframes) {
      b_next = frames[f + 1];
      n_next = a.counts[b_next];
      if (pf_lane) {
        const i32x4* p = reinterpret_cast<const i32x4*>(a.dets + (size_t)b_next * max_det + lane);
        pf0 = p[0]; pf1 = p[1];
      }
    }
    // ---- 1 predict, and the list of live slots in ascending order
    int n_live = 0;
    for (int base = 0; base < T; base += TRK_LANES) {
      const int s = base + lane;
      const bool live = s < T && s_live[s];
      if (s < T) { s_claimed[s] = 0; s_born[s] = 0; }
      if (live) {
        const float dt = (float)(s_missed[s] + 1);
#pragma unroll
        for (int k = 0; k < 4; ++k) s_pred[k][s] = a.motion ? __fadd_rn(s_box[k][s], __fmul_rn(s_vel[k][s], dt)) : s_box[k][s];
      }
      const unsigned long long m = __ballot(live);
      if (live) s_list[n_live + lanes_below(m, lane)] = s;
      n_live += __popcll(m);
    }
    __syncthreads();
    // ---- screen, lanes over detections: the predicted boxes are fixed for the frame and claims only remove candidates, so a
    // detection that passes iou_match with no live track of its class now can match nothing later either.  It leaves the
    // score-ordered walk below, which is sequential and rescans the keys per step: the walk visits only detections that
    // overlap a track, however many the frame has and however long a track stays unmatched.
    if (n_live > 0)
      for (int i = lane; i < n; i += TRK_LANES) {
        Rec r;
        if (i < TRK_DET_LDS) r = unpack_rec(s_det[i][0], s_det[i][1]);
        else {
          const i32x4* p = reinterpret_cast<const i32x4*>(fdets + i);
          r = unpack_rec(p[0], p[1]);
        }
        const float ai = __fmul_rn(__fsub_rn(r.x2, r.x1), __fsub_rn(r.y2, r.y1));
        bool possible = false;
        for (int j = 0; j < n_live && !possible; ++j) {
          const int s = s_list[j];
          if (!a.class_gate || s_cls[s] == r.dcls)
            possible = track_iou(r.x1, r.y1, r.x2, r.y2, ai, s_pred[0][s], s_pred[1][s], s_pred[2][s], s_pred[3][s]) > a.iou_match;
        }
        if (!possible) asg[i] = -2;
      }
    __syncthreads();

    // ---- 2 match + 3 update, the screened detections in descending det_conf; ends when every live track is claimed
    int unclaimed = n_live;
    while (unclaimed > 0) {
      unsigned long long best = 0;
      for (int i = lane; i < n; i += TRK_LANES)
        if (asg[i] == -1) {
          const unsigned long long K = ((unsigned long long)keys[i] << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
          best = K > best ? K : best;
        }
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other > best ? other : best;
      }
      if (best == 0) break;
      const int d = __builtin_amdgcn_readfirstlane((int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull)));
      Rec r;
      if (d < TRK_DET_LDS) r = unpack_rec(s_det[d][0], s_det[d][1]);
      else {
        const i32x4* p = reinterpret_cast<const i32x4*>(fdets + d);
        r = unpack_rec(p[0], p[1]);
      }
      const float ai = __fmul_rn(__fsub_rn(r.x2, r.x1), __fsub_rn(r.y2, r.y1));
      int bi = -1;
      float bv = 0.f;
      for (int s = lane; s < T; s += TRK_LANES)
        if (s_live[s] && !s_claimed[s] && (!a.class_gate || s_cls[s] == r.dcls)) {
          const float iou = track_iou(r.x1, r.y1, r.x2, r.y2, ai, s_pred[0][s], s_pred[1][s], s_pred[2][s], s_pred[3][s]);
          if (iou > a.iou_match && (bi < 0 || iou > bv)) { bi = s; bv = iou; }   // false for a NaN
        }
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
      }
      bi = __builtin_amdgcn_readfirstlane(bi);
      if (lane == (bi >= 0 ? (bi & (TRK_LANES - 1)) : 0)) {
        asg[d] = bi >= 0 ? bi : -2;
        if (bi >= 0) {
          const float dt = (float)(s_missed[bi] + 1);
          const float db[4] = {r.x1, r.y1, r.x2, r.y2};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (a.motion) s_vel[k][bi] = __fdiv_rn(__fsub_rn(db[k], s_box[k][bi]), dt);
            s_box[k][bi] = db[k];
          }
          s_hits[bi] += 1; s_missed[bi] = 0; s_claimed[bi] = 1;
          if (TOPK) {
            const TopkVote tv = load_topk(ftopk + d);
            if (topk_votes(tv, nc)) {
              s_wsum[bi] = __fadd_rn(__fmul_rn(s_wsum[bi], a.decay), topk_weight(tv, nc));
              s_vote[bi] = 1;
            }
          } else if (r.ccls >= 0 && r.ccls < nc) {
            s_wsum[bi] = __fadd_rn(__fmul_rn(s_wsum[bi], a.decay), r.cconf);
            s_vote[bi] = 1;
          }
        }
      }
      if (bi >= 0) --unclaimed;
      __syncthreads();
    }

    // ---- 4 age, and the free-slot list in ascending slot order
    int n_free = 0;
    for (int base = 0; base < T; base += TRK_LANES) {
      const int s = base + lane;
      bool is_free = false;
      if (s < T) {
        if (s_live[s]) {
          if (!s_claimed[s]) {
            const int m = s_missed[s] + 1;
            s_missed[s] = m;
            if (m > a.max_age) s_live[s] = 0;
          }
          if (s_live[s]) s_age[s] += 1;
        }
        is_free = !s_live[s];
      }
      const unsigned long long m = __ballot(is_free);
      if (is_free) s_free[n_free + lanes_below(m, lane)] = s;
      n_free += __popcll(m);
    }
    __syncthreads();

    // ---- 5 birth: the unmatched detections at or above new_conf, in record order, take the free slots in ascending order
    int births = 0;   // eligible detections so far, born or not
    for (int base = 0; base < n; base += TRK_LANES) {
      const int i = base + lane;
      bool elig = false;
      Rec r = {};
      if (i < n && asg[i] < 0) {
        if (i < TRK_DET_LDS) r = unpack_rec(s_det[i][0], s_det[i][1]);
        else {
          const i32x4* p = reinterpret_cast<const i32x4*>(fdets + i);
          r = unpack_rec(p[0], p[1]);
        }
        elig = r.conf >= a.new_conf;
      }
      const unsigned long long m = __ballot(elig);
      const int rank = births + lanes_below(m, lane);
      if (elig && rank < n_free) {
        const int s = s_free[rank];
        s_box[0][s] = r.x1; s_box[1][s] = r.y1; s_box[2][s] = r.x2; s_box[3][s] = r.y2;
#pragma unroll
        for (int k = 0; k < 4; ++k) s_vel[k][s] = 0.f;
        s_id[s] = next_id + rank; s_hits[s] = 1; s_missed[s] = 0; s_age[s] = 0; s_cls[s] = r.dcls;
        bool vote = r.ccls >= 0 && r.ccls < nc;
        float weight = r.cconf;
        if (TOPK) {
          const TopkVote tv = load_topk(ftopk + i);
          vote = topk_votes(tv, nc);
          weight = topk_weight(tv, nc);
        }
        s_wsum[s] = vote ? __fadd_rn(__fmul_rn(0.f, a.decay), weight) : 0.f;
        s_vote[s] = vote ? 1 : 0;
        s_live[s] = 1; s_claimed[s] = 1; s_born[s] = 1;
        asg[i] = s;
      }
      births += __popcll(m);
    }
    const int born = min(births, n_free);
    next_id += born;
    overflow += births - born;
    __syncthreads();

    // ---- 6 emit: untracked records, lanes over records ...
    for (int i = lane; i < n; i += TRK_LANES)
      if (asg[i] < 0) {
        i32x4* o = reinterpret_cast<i32x4*>(fout + i);
        o[0] = i32x4{0, -1, 0, 0};
        o[1] = i32x4{-1, 0, 0, 0};
      }
    // ... and the tracked ones one after the other, lanes over the classes of the track's accumulator row
    for (int base = 0; base < n; base += TRK_LANES) {
      const int i0 = base + lane;
      unsigned long long m = __ballot(i0 < n && asg[i0] >= 0);
      while (m) {
        const int i = base + (__ffsll((long long)m) - 1);
        m &= m - 1;
        const int s = asg[i];
        int ccls;
        float cconf;
        if (i < TRK_DET_LDS) { ccls = s_det[i][1].z; cconf = __int_as_float(s_det[i][1].w); }
        else { ccls = fdets[i].cls_class; cconf = fdets[i].cls_conf; }
        bool vote = ccls >= 0 && ccls < nc;
        const bool is_born = s_born[s] != 0;
        TopkVote tv = {};
        if (TOPK) {
          tv = load_topk(ftopk + i);
          vote = topk_votes(tv, nc);
        }
        float* row = accs + (size_t)s * nc;
        int bc = -1;
        float bvv = 0.f;
        for (int c = lane; c < nc; c += TRK_LANES) {
          float v = is_born ? 0.f : row[c];
          if (vote) {
            v = __fmul_rn(v, a.decay);
            if (TOPK) {
#pragma unroll
              for (int j = 0; j < LP_TOPK_MAX; ++j)
                if (tv.cls[j] == c) v = __fadd_rn(v, tv.prob[j]);   // c is in range: an invalid entry names no c
            } else if (c == ccls) v = __fadd_rn(v, cconf);
          }
          if (vote || is_born) row[c] = v;
          if (bc < 0 || v > bvv) { bc = c; bvv = v; }
        }
#pragma unroll
        for (int o = 32; o; o >>= 1) {
          const float ov = __shfl_xor(bvv, o);
          const int oc = __shfl_xor(bc, o);
          if (oc >= 0 && (bc < 0 || ov > bvv || (ov == bvv && oc < bc))) { bvv = ov; bc = oc; }
        }
        if (lane == 0) {
          const bool has = s_vote[s] != 0;
          const float ws = s_wsum[s];
          const float vconf = (has && ws > 0.f) ? __fdiv_rn(bvv, ws) : 0.f;
          const int flags = (s_hits[s] >= a.min_hits ? LP_TRACK_CONFIRMED : 0) | (is_born ? LP_TRACK_BORN : 0);
          i32x4* o = reinterpret_cast<i32x4*>(fout + i);
          o[0] = i32x4{s_id[s], s, s_hits[s], s_age[s]};
          o[1] = i32x4{has ? bc : -1, __float_as_int(vconf), __float_as_int(ws), flags};
        }
      }
    }
    __syncthreads();
  }

  for (int s = lane; s < T; s += TRK_LANES) {
    i32x4* p = reinterpret_cast<i32x4*>(tab + s);
    p[0] = i32x4{__float_as_int(s_box[0][s]), __float_as_int(s_box[1][s]), __float_as_int(s_box[2][s]), __float_as_int(s_box[3][s])};
    p[1] = i32x4{__float_as_int(s_vel[0][s]), __float_as_int(s_vel[1][s]), __float_as_int(s_vel[2][s]), __float_as_int(s_vel[3][s])};
    p[2] = i32x4{s_id[s], s_hits[s], s_missed[s], s_age[s]};
    p[3] = i32x4{s_cls[s], __float_as_int(s_wsum[s]), s_vote[s], s_live[s]};
  }
  if (lane == 0) *reinterpret_cast<i32x4*>(a.heads + job.stream) = i32x4{next_id, overflow, 0, 0};
}

__global__ __launch_bounds__(TRK_MAXT) void track_reset_kernel(TrackSlot* table, int T, int first) {
  if ((int)threadIdx.x >= T) return;
  i32x4* p = reinterpret_cast<i32x4*>(table + (size_t)(first + blockIdx.x) * T + threadIdx.x);
  const i32x4 z = {0, 0, 0, 0};
  p[0] = z; p[1] = z; p[2] = z; p[3] = z;
}

void launch_track(const TrackArgs& a, int n_jobs, hipStream_t st) {
  if (n_jobs <= 0) return;
  LP_CHECK(a.T >= 1 && a.T <= TRK_MAXT && a.nc >= 1 && a.max_det >= 1, LP_ERR_ARG, "bad tracker shape (max_tracks %d, classes %d)", a.T, a.nc);
  LP_CHECK(a.max_det <= LP_TRACK_KEY_LDS || a.scratch, LP_ERR_STATE, "the tracker has no scratch buffer for max_det %d", a.max_det);
  if (a.topk) LP_LAUNCH(track_kernel<true>, dim3(n_jobs), dim3(TRK_LANES), 0, st, a);
  else LP_LAUNCH(track_kernel<false>, dim3(n_jobs), dim3(TRK_LANES), 0, st, a);
  LP_HIP(hipGetLastError());
}

void launch_track_reset(TrackSlot* table, int T, int first, int n, hipStream_t st) {
  if (n <= 0) return;
  LP_LAUNCH(track_reset_kernel, dim3(n), dim3(TRK_MAXT), 0, st, table, T, first);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
