// Sign inventory: one record and best crop per finished track (the rule is stated in include/litepi.h,
// lp_inventory_config).  It runs behind the tracker's launch and sees only the two record streams, so track_kernel and its
// table are untouched.  Like the tracker the work is sequential over the frames of a stream and parallel over its slots and
// over the streams of a call: ONE WAVE per stream present in the call, lane l owns the entries l, l + 64, l + 128, l + 192,
// whose scalars live in LDS for the duration of the call.  Which entries close in a frame and where they land in the log come
// from ballots and prefix counts; the log head takes one atomicAdd per (stream, frame with closings).
// The crops are the only bandwidth, 16 bytes per lane, the whole wave on one crop at a time: classifier input buffer ->
// the slot's place in the gallery on a new best sighting, gallery -> log on a logged close.
#include <climits>

#include "common.h"
#include "evidence_window.h"
#include "kernels.h"

namespace lp {

#define INV_LANES 64
#define INV_MAXT 256                  // lp_track_config::max_tracks <= 256
#define INV_CHUNKS (INV_MAXT / INV_LANES)
#define EV_WORKERS 256                // list workers of the picture launch (x E / 8 bands)

typedef int i32x4 __attribute__((ext_vector_type(4)));

// words of an lp_sign
enum { W_STREAM, W_ID, W_FIRST, W_LAST, W_HITS, W_VCLS, W_VCONF, W_VW, W_BFRAME, W_BQ, W_X1, W_Y1, W_X2, W_Y2, W_DCLS, W_FLAGS, W_N };

__device__ __forceinline__ int inv_lanes_below(unsigned long long m, int lane) { return __popcll(m & ((1ull << lane) - 1ull)); }

// the whole wave copies one crop (bytes: a multiple of 16; both ends 16-byte aligned)
__device__ __forceinline__ void copy_crop(uint8_t* dst, const uint8_t* src, int bytes, int lane) {
  const i32x4* s = reinterpret_cast<const i32x4*>(src);
  i32x4* d = reinterpret_cast<i32x4*>(dst);
  for (int q = lane; q < bytes / 16; q += INV_LANES) d[q] = s[q];
}

// the evidence store's per-slot scalars in LDS (EV only): the window of the entry's best, the batch index of the frame that
// holds a best taken in this call (-1: the picture is in the gallery, or there is none), the log position the slot's
// gallery picture goes to (-1: none)
enum { EV_X, EV_Y, EV_W, EV_H, EV_B, EV_COPY, EV_N };

// frames == nullptr: flush the stream (every open entry closes, LP_SIGN_FLUSHED; the frame counter stays)
// EV: the deciding variant of a handle with an evidence store (kernels.h, EvArgs).
// With EV = false nothing of `e` is read and the code is the kernel's of before.
template <bool EV>
__device__ __forceinline__ void inventory_stream(const InvArgs& a, const EvArgs& e, int stream, const int* frames, int nframes) {
  __shared__ int s_ev[EV_N][EV ? INV_MAXT : 1];
  __shared__ int s_w[W_N][INV_MAXT];   // the entries' signs, structure of arrays
  __shared__ int s_open[INV_MAXT], s_missed[INV_MAXT];
  __shared__ int s_sight[INV_MAXT];    // per frame: the lowest record index that names the slot, INT_MAX = not sighted
  __shared__ int s_roi[INV_MAXT];      // per frame: ROI index of the crop the slot takes, -1 = none

  const int lane = threadIdx.x;
  const int T = a.T, max_det = a.max_det;
  const bool flush = frames == nullptr;
  InvEntry* ent = a.entries + (size_t)stream * T;
  uint8_t* gal = a.gallery ? a.gallery + (size_t)stream * T * a.crop_bytes : nullptr;

  for (int s = lane; s < T; s += INV_LANES) {
    const i32x4* p = reinterpret_cast<const i32x4*>(ent + s);
    const i32x4 q[5] = {p[0], p[1], p[2], p[3], p[4]};
#pragma unroll
    for (int k = 0; k < 4; ++k) { s_w[4 * k][s] = q[k].x; s_w[4 * k + 1][s] = q[k].y; s_w[4 * k + 2][s] = q[k].z; s_w[4 * k + 3][s] = q[k].w; }
    s_open[s] = q[4].x; s_missed[s] = q[4].y;
    if constexpr (EV) {
      const i32x4 w = *reinterpret_cast<const i32x4*>(e.win + ((size_t)stream * T + s) * 4);
      s_ev[EV_X][s] = w.x; s_ev[EV_Y][s] = w.y; s_ev[EV_W][s] = w.z; s_ev[EV_H][s] = w.w;
      s_ev[EV_B][s] = -1; s_ev[EV_COPY][s] = -1;
    }
  }
  const int t0 = a.frame_no[stream];
  int roi_total = 0;
  if (a.roi_rgb) roi_total = min(max(*a.roi_total, 0), a.max_rois);
  __syncthreads();

  const int steps = flush ? 1 : nframes;
  for (int f = 0; f < steps; ++f) {
    const int t = t0 + f;
    const int b = flush ? 0 : frames[f];
    const int n = flush ? 0 : min(max(a.counts[b], 0), max_det);
    const TrackRec* ftrk = a.tracks + (size_t)b * max_det;
    const lp_det* fdet = a.dets + (size_t)b * max_det;

    // ---- 1 sight, lanes over records
    if (!flush) {
      for (int s = lane; s < T; s += INV_LANES) s_sight[s] = INT_MAX;
      __syncthreads();
      for (int i = lane; i < n; i += INV_LANES) {
        const i32x4 r = *reinterpret_cast<const i32x4*>(ftrk + i);   // track_id, slot, hits, age
        if (r.x > 0 && r.y >= 0 && r.y < T) atomicMin(&s_sight[r.y], i);
      }
      __syncthreads();
    }

    // ---- 2 close, lanes over slots; the ballots of the entries that go to the log
    unsigned long long m[INV_CHUNKS];
    int n_log = 0;
#pragma unroll
    for (int c = 0; c < INV_CHUNKS; ++c) {
      const int s = c * INV_LANES + lane;
      bool log_it = false;
      if (s < T && s_open[s]) {
        bool closes = flush;
        if (!flush) {
          const int idx = s_sight[s];
          if (idx != INT_MAX) closes = ftrk[idx].track_id != s_w[W_ID][s];
          else {
            closes = s_missed[s] + 1 > a.max_age;
            if (!closes) s_missed[s] += 1;
          }
        }
        if (closes) {
          s_open[s] = 0;
          log_it = s_w[W_HITS][s] >= a.min_hits;
        }
      }
      m[c] = __ballot(log_it);
      n_log += __popcll(m[c]);
    }

    // ---- 3 log: one block per (stream, frame), ascending slots; what does not fit is counted by the head alone
    if (n_log > 0) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&a.head->logged, n_log);
      base = __builtin_amdgcn_readfirstlane(base);
      int before = 0;
#pragma unroll
      for (int c = 0; c < INV_CHUNKS; ++c) {
        const int s = c * INV_LANES + lane;
        if ((m[c] >> lane) & 1ull) {
          const int pos = base + before + inv_lanes_below(m[c], lane);
          if (pos >= 0 && pos < a.max_signs) {
            i32x4* o = reinterpret_cast<i32x4*>(a.log + pos);
#pragma unroll
            for (int k = 0; k < 4; ++k)
              o[k] = i32x4{s_w[4 * k][s], s_w[4 * k + 1][s], s_w[4 * k + 2][s], s_w[4 * k + 3][s] | (k == 3 && flush ? LP_SIGN_FLUSHED : 0)};
            if constexpr (EV) {   // the window goes with the sign; the pixels are the picture launch's
              const bool pic = (s_w[W_FLAGS][s] & LP_SIGN_HAS_EVIDENCE) != 0;
              const i32x4 w = pic ? i32x4{s_ev[EV_X][s], s_ev[EV_Y][s], s_ev[EV_W][s], s_ev[EV_H][s]} : i32x4{0, 0, 0, 0};
              *reinterpret_cast<i32x4*>(e.log_win + (size_t)pos * 4) = w;
              if (pic && s_ev[EV_B][s] >= 0) {   // the best lies in this call: frame -> log
                const int k = atomicAdd(e.n_jobs, 1);
                if (k >= 0 && k < e.cap_jobs) {
                  i32x4* j = reinterpret_cast<i32x4*>(e.jobs + k);
                  j[0] = i32x4{-1, s_ev[EV_B][s], w.x, w.y};
                  j[1] = i32x4{w.z, w.w, -1, pos};
                }
              } else if (pic) s_ev[EV_COPY][s] = pos;   // gallery -> log
            }
          }
        }
        if (gal && a.log_crops) {
          unsigned long long mm = m[c];
          for (int j = 0; mm; ++j) {
            const int sl = c * INV_LANES + (__ffsll((long long)mm) - 1);
            mm &= mm - 1;
            const int pos = base + before + j;
            if (pos >= 0 && pos < a.max_signs && (s_w[W_FLAGS][sl] & LP_SIGN_HAS_CROP))
              copy_crop(a.log_crops + (size_t)pos * a.crop_bytes, gal + (size_t)sl * a.crop_bytes, a.crop_bytes, lane);
          }
        }
        before += __popcll(m[c]);
      }
    }
    if (flush) break;
    __syncthreads();   // the gallery reads above are complete before a new best overwrites a slot's crop

    // ---- 4 open / update, lanes over slots
    for (int s = lane; s < T; s += INV_LANES) {
      const int idx = s_sight[s];
      int roi = -1;
      if (idx != INT_MAX) {
        const i32x4* tp = reinterpret_cast<const i32x4*>(ftrk + idx);
        const i32x4* dp = reinterpret_cast<const i32x4*>(fdet + idx);
        const i32x4 t0v = tp[0], t1v = tp[1], d0 = dp[0], d1 = dp[1];
        const bool opened = !s_open[s];
        if (opened) { s_open[s] = 1; s_w[W_STREAM][s] = stream; s_w[W_ID][s] = t0v.x; s_w[W_FIRST][s] = t; }
        s_w[W_LAST][s] = t; s_w[W_HITS][s] = t0v.z; s_w[W_VCLS][s] = t1v.x; s_w[W_VCONF][s] = t1v.y; s_w[W_VW][s] = t1v.z;
        s_missed[s] = 0;
        float q;
        if (a.quality) q = a.quality[(size_t)b * max_det + idx].sharpness;   // LP_RANK_SHARPNESS: the record as it is, -1 when empty
        else if (a.best == LP_BEST_AREA)
          q = __fmul_rn(__fsub_rn(__int_as_float(d0.z), __int_as_float(d0.x)), __fsub_rn(__int_as_float(d0.w), __int_as_float(d0.y)));
        else if (a.best == LP_BEST_DET_CONF) q = __int_as_float(d1.x);
        else q = d1.z >= 0 ? __int_as_float(d1.w) : -1.0f;
        if (opened || q > __int_as_float(s_w[W_BQ][s])) {   // false for a NaN
          s_w[W_BFRAME][s] = t; s_w[W_BQ][s] = __float_as_int(q);
          s_w[W_X1][s] = d0.x; s_w[W_Y1][s] = d0.y; s_w[W_X2][s] = d0.z; s_w[W_Y2][s] = d0.w; s_w[W_DCLS][s] = d1.y;
          if (a.roi_rgb) {
            const int r = a.roi_of[(size_t)b * max_det + idx];   // stale unless the list's entry r names this record
            if (r >= 0 && r < roi_total && a.roi_img[r] == b && a.roi_slot[r] == idx) roi = r;
          }
          s_w[W_FLAGS][s] = roi >= 0 ? LP_SIGN_HAS_CROP : 0;
          if constexpr (EV) {
            EvWindow wn = {0, 0, 0, 0};
            bool pic = false;
            if (e.frames) {
              const ImgGeom* g = e.fgeom + b;
              pic = evidence_window(e.scale, g->h, g->w, __int_as_float(d0.x), __int_as_float(d0.y), __int_as_float(d0.z), __int_as_float(d0.w), &wn);
            }
            s_ev[EV_X][s] = wn.x; s_ev[EV_Y][s] = wn.y; s_ev[EV_W][s] = wn.w; s_ev[EV_H][s] = wn.h;
            s_ev[EV_B][s] = pic ? b : -1;
            if (pic) s_w[W_FLAGS][s] |= LP_SIGN_HAS_EVIDENCE;
          }
        }
      }
      s_roi[s] = roi;
    }
    __syncthreads();
    if (gal && a.roi_rgb)
      for (int c = 0; c * INV_LANES < T; ++c) {
        const int s = c * INV_LANES + lane;
        unsigned long long mm = __ballot(s < T && s_roi[s] >= 0);
        while (mm) {
          const int sl = c * INV_LANES + (__ffsll((long long)mm) - 1);
          mm &= mm - 1;
          copy_crop(gal + (size_t)sl * a.crop_bytes, a.roi_rgb + (size_t)s_roi[sl] * a.crop_bytes, a.crop_bytes, lane);
        }
      }
    __syncthreads();   // the gallery writes are visible to the next frame's log copies
  }

  for (int s = lane; s < T; s += INV_LANES) {
    i32x4* p = reinterpret_cast<i32x4*>(ent + s);
#pragma unroll
    for (int k = 0; k < 4; ++k) p[k] = i32x4{s_w[4 * k][s], s_w[4 * k + 1][s], s_w[4 * k + 2][s], s_w[4 * k + 3][s]};
    p[4] = i32x4{s_open[s], s_missed[s], 0, 0};
    if constexpr (EV) {
      const i32x4 w = i32x4{s_ev[EV_X][s], s_ev[EV_Y][s], s_ev[EV_W][s], s_ev[EV_H][s]};
      *reinterpret_cast<i32x4*>(e.win + ((size_t)stream * T + s) * 4) = w;
      const int b = s_open[s] ? s_ev[EV_B][s] : -1;
      if (s_ev[EV_COPY][s] >= 0 || b >= 0) {
        const int k = atomicAdd(e.n_jobs, 1);
        if (k >= 0 && k < e.cap_jobs) {
          i32x4* j = reinterpret_cast<i32x4*>(e.jobs + k);
          j[0] = i32x4{s_ev[EV_COPY][s], b, w.x, w.y};
          j[1] = i32x4{w.z, w.w, stream * T + s, -1};
        }
      }
    }
  }
  if (!flush && lane == 0) a.frame_no[stream] = t0 + nframes;
}

__global__ __launch_bounds__(INV_LANES) void inventory_kernel(const InvArgs a) {
  const TrackJob job = a.jobs[blockIdx.x];
  inventory_stream<false>(a, EvArgs{}, job.stream, a.frames + job.first, job.nframes);
}

__global__ __launch_bounds__(INV_LANES) void inventory_flush_kernel(const InvArgs a, int first) {
  inventory_stream<false>(a, EvArgs{}, first + blockIdx.x, nullptr, 0);
}

// the deciding variants of a handle with an evidence store
__global__ __launch_bounds__(INV_LANES) void inventory_evidence_kernel(const InvArgs a, const EvArgs e) {
  const TrackJob job = a.jobs[blockIdx.x];
  inventory_stream<true>(a, e, job.stream, a.frames + job.first, job.nframes);
}

__global__ __launch_bounds__(INV_LANES) void inventory_flush_evidence_kernel(const InvArgs a, const EvArgs e, int first) {
  inventory_stream<true>(a, e, first + blockIdx.x, nullptr, 0);
}

// record -> ROI index of the call's ROI list; entries of earlier calls stay and are recognised as stale by the reader
__global__ __launch_bounds__(256) void inventory_roi_scatter_kernel(const InvArgs a) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  const int total = min(max(*a.roi_total, 0), a.max_rois);
  if (r >= total) return;
  const int img = a.roi_img[r], slot = a.roi_slot[r];
  if (img >= 0 && img < a.B && slot >= 0 && slot < a.max_det) a.roi_of[(size_t)img * a.max_det + slot] = r;
}

static void check_inventory_args(const InvArgs& a) {
  LP_CHECK(a.T >= 1 && a.T <= INV_MAXT && a.max_det >= 1 && a.max_signs >= 1, LP_ERR_ARG, "bad inventory shape (max_tracks %d, max_signs %d)", a.T,
           a.max_signs);
  LP_CHECK(!a.gallery || (a.crop_bytes > 0 && a.crop_bytes % 16 == 0), LP_ERR_ARG, "crops of %d bytes are not a multiple of 16", a.crop_bytes);
}

void launch_inventory(const InvArgs& a, int n_jobs, hipStream_t st) {
  if (n_jobs <= 0) return;
  check_inventory_args(a);
  if (a.roi_rgb) {
    LP_LAUNCH(inventory_roi_scatter_kernel, dim3(ceil_div(std::max(a.max_rois, 1), 256)), dim3(256), 0, st, a);
  }
  LP_LAUNCH(inventory_kernel, dim3(n_jobs), dim3(INV_LANES), 0, st, a);
  LP_HIP(hipGetLastError());
}

void launch_inventory_flush(const InvArgs& a, int first, int n, hipStream_t st) {
  if (n <= 0) return;
  check_inventory_args(a);
  LP_LAUNCH(inventory_flush_kernel, dim3(n), dim3(INV_LANES), 0, st, a, first);
  LP_HIP(hipGetLastError());
}

void launch_inventory_evidence(const InvArgs& a, const EvArgs& e, int n_jobs, hipStream_t st) {
  if (n_jobs <= 0) return;
  check_inventory_args(a);
  if (a.roi_rgb) {
    LP_LAUNCH(inventory_roi_scatter_kernel, dim3(ceil_div(std::max(a.max_rois, 1), 256)), dim3(256), 0, st, a);
  }
  LP_HIP(hipMemsetAsync(e.n_jobs, 0, sizeof(int), st));
  LP_LAUNCH(inventory_evidence_kernel, dim3(n_jobs), dim3(INV_LANES), 0, st, a, e);
  LP_HIP(hipGetLastError());
  launch_evidence_pictures(e, std::min(e.cap_jobs, EV_WORKERS), st);
}

void launch_inventory_flush_evidence(const InvArgs& a, const EvArgs& e, int first, int n, hipStream_t st) {
  if (n <= 0) return;
  check_inventory_args(a);
  LP_HIP(hipMemsetAsync(e.n_jobs, 0, sizeof(int), st));
  LP_LAUNCH(inventory_flush_evidence_kernel, dim3(n), dim3(INV_LANES), 0, st, a, e, first);
  LP_HIP(hipGetLastError());
  launch_evidence_pictures(e, std::min(n * a.T, EV_WORKERS), st);   // a flush only copies: the pictures are all in the gallery
}

}  // namespace lp
