// The per-class greedy NMS core (e2e.py:89-119, 280-296, 465-473), defined once.  Two front ends put a list of candidates in
// final order -- nms_kernel (post_kernels.hip) sorts one image's candidates, frame_nms_kernel (tile_kernels.hip) merges the
// sorted lists of a frame's views -- and everything from there on is here: the wave64 ballot sweep, the outer phase, the
// max_det cut, the ROI rule, the records, the counts and the batch's ROI list.  The image NMS is the one-view case of the frame
// NMS with the reference's match and no union: nms_finish<false, false>.
//
// Everything that decides WHICH boxes survive is explicit round-to-nearest fp32 in the reference's operation order.
#pragma once
#include "common.h"
#include "kernels.h"

namespace lp {

#define NMS_THREADS 1024

// (0xFFFF - class, score bits, anchor): descending order is class ascending, score descending, ties -> higher anchor first
// (the order a stable ascending argsort reversed gives; e2e.py:96)
__device__ __forceinline__ unsigned long long nms_key(const Cand& c) {
  return ((unsigned long long)(0xFFFFu - (unsigned)c.cls) << 46) | ((unsigned long long)__float_as_uint(c.score) << 14) |
         (unsigned long long)(c.anchor & 0x3FFF);
}
// score-major key of a kept box (global top-max_det selection): (score, view, anchor), unique inside a frame (views < 1024,
// anchors < 16384).  Cand::pad holds the view; emit_candidate sets it to 0 for every image candidate.
__device__ __forceinline__ unsigned long long frame_score_key(const Cand& c) {
  return ((unsigned long long)__float_as_uint(c.score) << 24) | ((unsigned long long)(c.pad & 0x3FF) << 14) |
         (unsigned long long)(c.anchor & 0x3FFF);
}
// true when box j (area aj) is suppressed by kept box i (area ai): NOT (iou <= thr), e2e.py:116
__device__ __forceinline__ bool nms_suppressed(float ix1, float iy1, float ix2, float iy2, float ai, float jx1, float jy1, float jx2,
                                               float jy2, float thr) {
  const float aj = __fmul_rn(__fsub_rn(jx2, jx1), __fsub_rn(jy2, jy1));
  const float w = fmaxf(0.f, __fsub_rn(fminf(ix2, jx2), fmaxf(ix1, jx1)));
  const float h = fmaxf(0.f, __fsub_rn(fminf(iy2, jy2), fmaxf(iy1, jy1)));
  const float inter = __fmul_rn(w, h);
  const float iou = __fdiv_rn(inter, __fadd_rn(__fsub_rn(__fadd_rn(ai, aj), inter), 1e-6f));
  return !(iou <= thr);
}
// the match of the frame NMS of views (lp_set_view_merge): IOS = false is nms_suppressed itself; IOS = true divides by the
// smaller of the two areas, so a box cut by a view border matches the whole box it lies in
template <bool IOS>
__device__ __forceinline__ bool view_matched(float ix1, float iy1, float ix2, float iy2, float ai, float jx1, float jy1, float jx2,
                                             float jy2, float thr) {
  if (!IOS) return nms_suppressed(ix1, iy1, ix2, iy2, ai, jx1, jy1, jx2, jy2, thr);
  const float aj = __fmul_rn(__fsub_rn(jx2, jx1), __fsub_rn(jy2, jy1));
  const float w = fmaxf(0.f, __fsub_rn(fminf(ix2, jx2), fmaxf(ix1, jx1)));
  const float h = fmaxf(0.f, __fsub_rn(fminf(iy2, jy2), fmaxf(iy1, jy1)));
  const float inter = __fmul_rn(w, h);
  const float ios = __fdiv_rn(inter, __fadd_rn(fminf(ai, aj), 1e-6f));
  return !(ios <= thr);
}
// min / max of the 64 lanes' values, in every lane (float min and max commute: the order of the steps does not show)
__device__ __forceinline__ float wave_min(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fminf(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
  return v;
}
// LDS atomic min / max of floats through their bit patterns: a non-negative float orders like its int pattern, a negative
// one like its unsigned pattern reversed, so either sign is exact (no NaN: candidates are clipped coordinates)
__device__ __forceinline__ void lds_min_f32(float* p, float v) {
  if (v >= 0.f) atomicMin(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMax(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}
__device__ __forceinline__ void lds_max_f32(float* p, float v) {
  if (v >= 0.f) atomicMax(reinterpret_cast<int*>(p), __float_as_int(v));
  else atomicMin(reinterpret_cast<unsigned*>(p), __float_as_uint(v));
}

// exclusive prefix sum of one int per thread over the workgroup (NMS_THREADS = 16 waves); returns the total via *total
__device__ __forceinline__ int block_exclusive_scan(int v, int* s_wave /*[17]*/, int* total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o);
    if (lane >= o) inc += t;
  }
  if (lane == 63) s_wave[wave] = inc;
  __syncthreads();
  if (wave == 0) {
    int w = lane < NMS_THREADS / 64 ? s_wave[lane] : 0;
    int winc = w;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const int t = __shfl_up(winc, o);
      if (lane >= o) winc += t;
    }
    if (lane < NMS_THREADS / 64) s_wave[lane] = winc - w;
    if (lane == NMS_THREADS / 64 - 1) s_wave[NMS_THREADS / 64] = winc;
  }
  __syncthreads();
  const int r = s_wave[wave] + inc - v;
  *total = s_wave[NMS_THREADS / 64];
  __syncthreads();  // s_wave may be reused
  return r;
}

// ROI rectangle of a kept box (int truncation + clip) and the area filter.  rule 0 = HybridPipeline.run, e2e.py:465-473:
// x1 in [0, w-1], y1 in [0, h-1], x2 in [x1+1, w], y2 in [y1+1, h]; rule 1 = HybridPipelineOptimized.run,
// e2e_optimize.py:480-497: all four clipped to [0, w] / [0, h], empty rectangles dropped.  min_area < 0: no filter.
__device__ __forceinline__ bool roi_rect(const Cand& c, const ImgGeom& gm, int rule, int min_area, int& x1, int& y1, int& x2, int& y2) {
  x1 = (int)c.x1; y1 = (int)c.y1; x2 = (int)c.x2; y2 = (int)c.y2;
  if (rule == 0) {
    x1 = min(max(x1, 0), gm.w - 1); y1 = min(max(y1, 0), gm.h - 1);
    x2 = min(max(x2, x1 + 1), gm.w); y2 = min(max(y2, y1 + 1), gm.h);
  } else {
    x1 = min(max(x1, 0), gm.w); x2 = min(max(x2, 0), gm.w);
    y1 = min(max(y1, 0), gm.h); y2 = min(max(y2, 0), gm.h);
  }
  return min_area < 0 || (((x2 - x1) * (y2 - y1) >= min_area) && x2 > x1 && y2 > y1);
}

// ------------------------------------------------------------------------------------
// Sort: keys[i] = nms_key(cand[i]) through a descending bitonic sort in LDS (keys: room for cnt rounded up to a power of two),
// then the records in that order to sorted[].  The slot of a key inside cand[] is not stored in it, so each candidate finds
// its own rank by binary search (keys are unique in one image / view).  Whole workgroup; ends without a barrier.
// ------------------------------------------------------------------------------------
__device__ __forceinline__ void nms_sort_to(unsigned long long* keys, const Cand* cand, Cand* sorted, int cnt) {
  const int tid = threadIdx.x;
  int nsort = 1;
  while (nsort < cnt) nsort <<= 1;
  for (int i = tid; i < nsort; i += NMS_THREADS) keys[i] = i < cnt ? nms_key(cand[i]) : 0ull;   // (a real key is never 0: that would take class 65535)
  __syncthreads();
  for (int k = 2; k <= nsort; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < nsort; i += NMS_THREADS) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long x = keys[i], y = keys[ixj];
          const bool desc = (i & k) == 0;
          if (desc ? (x < y) : (x > y)) { keys[i] = y; keys[ixj] = x; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < cnt; i += NMS_THREADS) {
    const Cand c = cand[i];
    const unsigned long long k = nms_key(c);
    int lo = 0, hi = cnt - 1;
    while (lo < hi) {  // descending order
      const int mid = (lo + hi) >> 1;
      if (keys[mid] > k) lo = mid + 1; else hi = mid;
    }
    sorted[lo] = c;
  }
}

// ------------------------------------------------------------------------------------
// Greedy sweep of one chunk of 64 boxes in final order, one box per lane of ONE wave (box bj, area aj; `alive`: the lanes that
// hold a box no earlier chunk removed): box i, still alive, is kept and suppresses every later lane of its class that matches
// it; the ballot of those lanes clears them from the alive mask, no barrier.  At most `room` boxes are kept.  Returns the kept
// mask.  UNI: un[] enters as the lane's own box and leaves, in a keeper's lane, grown by every box the keeper absorbed
// (reduced over the ballot); matching always uses the keeper's OWN box.  <false, false> is the reference's rule and carries
// none of the merge.
// ------------------------------------------------------------------------------------
template <bool IOS, bool UNI>
__device__ __forceinline__ unsigned long long nms_sweep_chunk(const Cand& bj, float aj, unsigned long long alive, int room, float thr,
                                                              float (&un)[4]) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = alive, kept = 0ull;
  while (todo && room > 0) {  // wave-uniform
    const int i = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    kept |= 1ull << i;
    --room;
    const float ix1 = __shfl(bj.x1, i), iy1 = __shfl(bj.y1, i), ix2 = __shfl(bj.x2, i), iy2 = __shfl(bj.y2, i);
    const float ai = __shfl(aj, i);
    const int ic = __shfl(bj.cls, i);
    const bool sup = lane > i && ((alive >> lane) & 1ull) && bj.cls == ic &&
                     view_matched<IOS>(ix1, iy1, ix2, iy2, ai, bj.x1, bj.y1, bj.x2, bj.y2, thr);
    const unsigned long long m = __ballot(sup);
    alive &= ~m;
    todo &= ~m;
    if (UNI && m) {   // wave-uniform
      const float mx1 = wave_min(sup ? bj.x1 : INFINITY), my1 = wave_min(sup ? bj.y1 : INFINITY);
      const float mx2 = wave_max(sup ? bj.x2 : -INFINITY), my2 = wave_max(sup ? bj.y2 : -INFINITY);
      if (lane == i) { un[0] = fminf(un[0], mx1); un[1] = fminf(un[1], my1); un[2] = fmaxf(un[2], mx2); un[3] = fmaxf(un[3], my2); }
    }
  }
  return kept;
}

// ------------------------------------------------------------------------------------
// The end of every path: counts, the batch-wide ROI list, one record.  n: the image / frame = the workgroup; nblocks: the grid.
// ------------------------------------------------------------------------------------
// counts[n] = kept after the area filter, counts[N + n] = kept before it, then the float bits of the mean detector confidence
// over ALL kept boxes, before the area filter (PipelineMetrics.det_confidence_avg, e2e.py:456-457)
__device__ __forceinline__ void nms_publish_counts(const NmsCommon& a, int n, int nblocks, int run, int nsel, double ssum) {
  a.counts[n] = run;
  a.counts[nblocks + n] = nsel;
  reinterpret_cast<float*>(a.counts)[2 * nblocks + n] = nsel > 0 ? (float)(ssum / (double)nsel) : 0.f;
}
// the workgroup's slice of the batch-wide ROI list: work[0] accumulates, the block that draws the last ticket (work[1])
// publishes the clamped total for the classifier kernels and re-arms both words for the next call.  The ticket is issued
// only after the slice's add has RETURNED, so the last ticket implies every add is done.  One thread per workgroup.
__device__ __forceinline__ int nms_roi_slice(const NmsCommon& a, int run, int nblocks) {
  int base = 0;
  if (a.tab.total) {
    base = atomicAdd(a.tab.work, run);
    int one = 1;
    asm volatile("" : "+v"(one) : "v"(base));
    const int ticket = atomicAdd(a.tab.work + 1, one);
    if (ticket == nblocks - 1) {
      const int raw = atomicExch(a.tab.work, 0);
      atomicExch(a.tab.work + 1, 0);
      a.tab.total[0] = raw < a.max_rois ? raw : a.max_rois;
      a.tab.total[1] = raw;  // unclamped: the host checks it against the capacity
    }
  }
  return base;
}
// kept box c of workgroup n as record o, its ROI rectangle, and its entry base + o of the ROI list
__device__ __forceinline__ void nms_emit(const NmsCommon& a, int n, int o, int base, const Cand& c, int x1, int y1, int x2, int y2) {
  lp_det d;
  d.x1 = c.x1; d.y1 = c.y1; d.x2 = c.x2; d.y2 = c.y2; d.det_conf = c.score; d.det_class = c.cls;
  d.cls_class = -1; d.cls_conf = 0.f;
  a.dets[(long)n * a.max_det + o] = d;
  int* rects = a.rects + ((long)n * a.max_det + o) * 4;
  rects[0] = x1; rects[1] = y1; rects[2] = x2; rects[3] = y2;
  if (a.tab.total && base + o < a.max_rois) { a.tab.img[base + o] = n; a.tab.slot[base + o] = o; }
}

// ------------------------------------------------------------------------------------
// One-wave path: at most 64 candidates, none of which max_det can cut (the usual image or frame at conf 0.25).  The front end
// has candidate `lane` of the final order in bj (lanes >= cnt: class -1, zero box); from here the sweep, the ROI rule, the
// compaction by ballot and the bookkeeping of the general path, with identical results (same arithmetic) and none of its
// sixteen-wave barriers, LDS passes and global round trips.  Wave 0 only.
// ------------------------------------------------------------------------------------
template <bool IOS, bool UNI>
__device__ __forceinline__ void nms_small_tail(const NmsCommon& a, const ImgGeom& geom, int n, int nblocks, Cand bj, int cnt) {
  const int lane = threadIdx.x & 63;
  const float aj = __fmul_rn(__fsub_rn(bj.x2, bj.x1), __fsub_rn(bj.y2, bj.y1));
  float un[4] = {bj.x1, bj.y1, bj.x2, bj.y2};
  const unsigned long long kept = nms_sweep_chunk<IOS, UNI>(bj, aj, __ballot(lane < cnt), 64, a.iou, un);
  if (UNI) { bj.x1 = un[0]; bj.y1 = un[1]; bj.x2 = un[2]; bj.y2 = un[3]; }   // only the keepers' boxes are read from here on
  const bool is_kept = (kept >> lane) & 1ull;
  const int nsel = __popcll(kept);   // <= cnt <= max_det: nothing to cut
  const ImgGeom gm = geom;
  int x1 = 0, y1 = 0, x2 = 0, y2 = 0;
  const bool ok = is_kept && roi_rect(bj, gm, a.roi_rule, a.min_area, x1, y1, x2, y2);
  const unsigned long long okm = __ballot(ok);
  const int o = __popcll(okm & ((1ull << lane) - 1ull)), run = __popcll(okm);
  double ssum = is_kept ? (double)bj.score : 0.0;
  for (int off = 32; off > 0; off >>= 1) ssum += __shfl_xor(ssum, off);
  int base = 0;
  if (lane == 0) {
    nms_publish_counts(a, n, nblocks, run, nsel, ssum);
    base = nms_roi_slice(a, run, nblocks);
  }
  base = __shfl(base, 0);
  if (ok) nms_emit(a, n, o, base, bj, x1, y1, x2, y2);
}

// ------------------------------------------------------------------------------------
// General path, from "list[0, cnt) is in final order" to the end.  Whole workgroup; masks: 2 * ceil(cnt / 32) words of LDS.
//   1. greedy sweep over the list in chunks of 64: wave 0 runs nms_sweep_chunk, the chunk's keepers (s_chunk) then suppress
//      all later boxes in parallel over the workgroup -- one barrier pair per 64 boxes instead of one per kept box.  Removed
//      and kept flags are bit masks in LDS.
//   2. max_det: the reference keeps every survivor.  When more than max_det survive, the max_det highest (score, view, anchor)
//      keys stay and are emitted in list order; that key is unique, so the threshold key T with exactly max_det keys >= T
//      exists and is found bit by bit.  With a single class the list order is score order: the sweep stops at max_det keepers.
//   3. ROI rectangle and area filter of the kept boxes, order-preserving compaction into the records, the counts and the
//      workgroup's slice of the ROI list.
// UNI: the union grows in s_union -- over the ballot in wave 0's sweep, by LDS atomics from the thread that owns j in the
// outer phase -- and is written over the keeper's record in list[] once the chunk's outer phase is done: no later chunk reads
// an earlier chunk's keepers, the final phases read the union.
// ------------------------------------------------------------------------------------
template <bool IOS, bool UNI>
__device__ __forceinline__ void nms_finish(const NmsCommon& a, const ImgGeom& geom, Cand* list, int cnt, int n, int nblocks, unsigned* masks) {
  __shared__ int s_wave[NMS_THREADS / 64 + 1];
  __shared__ float s_chunk[64 * 6];  // kept boxes of the current chunk: x1, y1, x2, y2, area, class bits
  __shared__ float s_union[UNI ? 64 * 4 : 1];
  __shared__ int s_nk, s_base;
  __shared__ double s_red[NMS_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nwords = (cnt + 31) >> 5;
  unsigned* removed = masks;
  unsigned* keptm = removed + nwords;
  for (int i = tid; i < 2 * nwords; i += NMS_THREADS) removed[i] = 0u;
  __threadfence_block();
  __syncthreads();   // the front end's list[] and the masks

  // ---- greedy sweep, 64 boxes per step
  int nkeep = 0;
  const float thr = a.iou;
  const bool single_class = a.nc <= 1;
  for (int c0 = 0; c0 < cnt; c0 += 64) {
    unsigned long long kept = 0ull;   // wave 0: the chunk's keepers
    if (wave == 0) {
      const int j = c0 + lane;
      const bool valid = j < cnt;
      Cand bj;
      bj.x1 = bj.y1 = bj.x2 = bj.y2 = 0.f; bj.cls = -1;
      if (valid) bj = list[j];
      const float aj = __fmul_rn(__fsub_rn(bj.x2, bj.x1), __fsub_rn(bj.y2, bj.y1));
      const unsigned long long alive = __ballot(valid && !((removed[valid ? (j >> 5) : 0] >> (j & 31)) & 1u));
      float un[4] = {bj.x1, bj.y1, bj.x2, bj.y2};
      kept = nms_sweep_chunk<IOS, UNI>(bj, aj, alive, single_class ? a.max_det - nkeep : 0x7fffffff, thr, un);
      if ((kept >> lane) & 1ull) {
        const int idx = __popcll(kept & ((1ull << lane) - 1ull));
        float* cb = s_chunk + idx * 6;
        cb[0] = bj.x1; cb[1] = bj.y1; cb[2] = bj.x2; cb[3] = bj.y2; cb[4] = aj; cb[5] = __int_as_float(bj.cls);
        if (UNI) {
          float* ub = s_union + idx * 4;
          ub[0] = un[0]; ub[1] = un[1]; ub[2] = un[2]; ub[3] = un[3];
        }
      }
      if (lane == 0) {   // c0 is a multiple of 64: the chunk owns two whole words of the kept mask
        keptm[c0 >> 5] = (unsigned)kept;
        if ((c0 >> 5) + 1 < nwords) keptm[(c0 >> 5) + 1] = (unsigned)(kept >> 32);
        s_nk = __popcll(kept);
      }
    }
    __syncthreads();
    const int nk = s_nk;
    nkeep += nk;
    // one class: max_det keepers are all there will be.  The union of this last chunk's keepers still needs its outer phase.
    const bool full = single_class && nkeep >= a.max_det;
    if (!UNI && full) break;
    for (int j = c0 + 64 + tid; j < cnt; j += NMS_THREADS) {
      if ((removed[j >> 5] >> (j & 31)) & 1u) continue;
      const Cand bj = list[j];
      for (int k = 0; k < nk; ++k) {
        const float* cb = s_chunk + k * 6;
        if (__float_as_int(cb[5]) != bj.cls) continue;
        if (view_matched<IOS>(cb[0], cb[1], cb[2], cb[3], cb[4], bj.x1, bj.y1, bj.x2, bj.y2, thr)) {
          atomicOr(&removed[j >> 5], 1u << (j & 31));
          if (UNI) {   // the FIRST matching keeper of the chunk takes j
            float* ub = s_union + k * 4;
            lds_min_f32(ub + 0, bj.x1); lds_min_f32(ub + 1, bj.y1); lds_max_f32(ub + 2, bj.x2); lds_max_f32(ub + 3, bj.y2);
          }
          break;
        }
      }
    }
    __syncthreads();
    if (UNI) {
      if ((kept >> lane) & 1ull) {   // wave 0 only: the other waves' kept is 0
        const float* ub = s_union + __popcll(kept & ((1ull << lane) - 1ull)) * 4;
        Cand* m = list + c0 + lane;
        m->x1 = ub[0]; m->y1 = ub[1]; m->x2 = ub[2]; m->y2 = ub[3];
      }
      __threadfence_block();
      if (full) break;
    }
  }
  __syncthreads();

  // ---- more survivors than max_det (several classes; one class never keeps more): the max_det best (score, view, anchor) keys
  unsigned long long T = 0ull;
  int nsel = nkeep;
  const bool by_key = nkeep > a.max_det;
  if (by_key) {
    for (int bit = 55; bit >= 0; --bit) {
      const unsigned long long candT = T | (1ull << bit);
      int c = 0;
      for (int j = tid; j < cnt; j += NMS_THREADS)
        if ((keptm[j >> 5] >> (j & 31)) & 1u) c += frame_score_key(list[j]) >= candT ? 1 : 0;
      int tot;
      (void)block_exclusive_scan(c, s_wave, &tot);
      if (tot >= a.max_det) T = candT;
    }
    nsel = a.max_det;
  }

  // ---- ROI rectangle + area filter, order-preserving compaction
  const ImgGeom gm = geom;
  const int per = (cnt + NMS_THREADS - 1) / NMS_THREADS;
  const int k0 = tid * per, k1 = (k0 + per < cnt) ? k0 + per : cnt;
  int nvalid = 0;
  double ssum = 0.0;
  for (int k = k0; k < k1; ++k) {
    if (!((keptm[k >> 5] >> (k & 31)) & 1u)) continue;
    const Cand c = list[k];
    if (by_key && frame_score_key(c) < T) continue;
    ssum += (double)c.score;
    int x1, y1, x2, y2;
    nvalid += roi_rect(c, gm, a.roi_rule, a.min_area, x1, y1, x2, y2) ? 1 : 0;
  }
  int run;
  int o = block_exclusive_scan(nvalid, s_wave, &run);
  for (int off = 32; off > 0; off >>= 1) ssum += __shfl_xor(ssum, off);
  if (lane == 0) s_red[wave] = ssum;
  __syncthreads();
  if (tid == 0) {
    double tot = 0.0;
    for (int w = 0; w < NMS_THREADS / 64; ++w) tot += s_red[w];
    nms_publish_counts(a, n, nblocks, run, nsel, tot);
    s_base = nms_roi_slice(a, run, nblocks);
  }
  __syncthreads();
  const int base = s_base;
  for (int k = k0; k < k1; ++k) {
    if (!((keptm[k >> 5] >> (k & 31)) & 1u)) continue;
    const Cand c = list[k];
    if (by_key && frame_score_key(c) < T) continue;
    int x1, y1, x2, y2;
    if (!roi_rect(c, gm, a.roi_rule, a.min_area, x1, y1, x2, y2)) continue;
    nms_emit(a, n, o, base, c, x1, y1, x2, y2);
    ++o;
  }
}

}  // namespace lp
