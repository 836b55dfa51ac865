// Tiled inference of large frames (DESIGN.md "Tiled inference"): the view gather that cuts native-resolution crops out of
// the frames, and the frame NMS that merges the candidates of all views of one frame into ONE per-class greedy NMS with the
// reference's arithmetic (e2e.py:89-119).  The letterboxed whole-frame views are made by the letterbox kernel itself
// (misc_kernels.hip), so they are bit-identical to lp_test_letterbox.  Scaled views add the window gather:
// the letterbox of any window of a frame, a front end of the same core (letterbox_core.h).
#include "common.h"
#include "kernels.h"
#include "nms_dev.h"
#include "post_dev.h"
#include <algorithm>

namespace lp {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------
// Crop views: dst[slot] = frame[y0:y0+S, x0:x0+S] (BGR uint8), 114 where the window passes the frame edge.  The view's
// geometry holds the window as top = -y0, left = -x0.  One thread per 16-byte chunk of an output row (3S % 16 == 0): aligned
// 16-byte loads (two, funnel-shifted, when the source run is not 16-byte aligned), one 16-byte store.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void crop_views_kernel(const uint8_t* __restrict__ src, const ImgGeom* __restrict__ geom,
                                                         uint8_t* __restrict__ dst, int slot0, int S) {
  const int slot = slot0 + blockIdx.y;
  const int cpr = 3 * S / 16;   // chunks per output row
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= cpr * S) return;
  const int row = idx / cpr, c = idx - row * cpr;
  const ImgGeom gm = geom[slot];
  const int fy = row - gm.top;
  const long rb = (long)gm.w * 3;                 // frame row bytes
  const long sx = (long)(-gm.left) * 3 + 16L * c;  // first source byte of the chunk inside the frame row
  const uint8_t* im = src + gm.src_off;
  const long img_bytes = rb * gm.h;
  u32x4 v;
  if (fy < 0 || fy >= gm.h || sx >= rb) {
    v = u32x4{0x72727272u, 0x72727272u, 0x72727272u, 0x72727272u};   // 114
  } else {
    const long off = (long)fy * rb + sx;
    const uintptr_t p = reinterpret_cast<uintptr_t>(im + off);
    const int sh = (int)(p & 15);
    const long al = off - sh;   // aligned start, relative to the frame
    if (sx + 16 <= rb && sh == 0) {
      v = *reinterpret_cast<const u32x4*>(im + off);
    } else if (sx + 16 <= rb && al >= 0 && al + 32 <= img_bytes) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(im + al), b = *reinterpret_cast<const u32x4*>(im + al + 16);
      const uint32_t w[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
      const int q = sh >> 2, r = sh & 3;
      uint32_t s[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) s[i] = q == 0 ? w[i] : (q == 1 ? w[i + 1] : (q == 2 ? w[i + 2] : w[i + 3]));
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = r == 0 ? s[k] : (uint32_t)((((unsigned long long)s[k + 1] << 32) | s[k]) >> (8 * r));
    } else {   // the chunk reaches the frame's right edge (or its first / last bytes): byte by byte, nothing outside is read
      uint8_t t[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) t[k] = sx + k < rb ? im[off + k] : (uint8_t)114;
      v = *reinterpret_cast<const u32x4*>(t);
    }
  }
  *reinterpret_cast<u32x4*>(dst + (long)slot * S * S * 3 + (long)row * S * 3 + 16L * c) = v;
}

void launch_crop_views(const uint8_t* src, const ImgGeom* geom, uint8_t* dst, int slot0, int nslots, int S, hipStream_t st) {
  if (nslots <= 0) return;
  LP_CHECK(S % 16 == 0, LP_ERR_ARG, "crop views need det_input %% 16 == 0");
  dim3 grid(ceil_div(3 * S / 16 * S, 256), nslots);
  LP_LAUNCH(crop_views_kernel, grid, dim3(256), 0, st, src, geom, dst, slot0, S);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Window views (lp_run_views*): dst[slot] = letterbox(frame[y:y+h, x:x+w]) at any scale, 114 in the bars.  Front ends of the
// letterbox core (letterbox_core.h) over the windows of the view table: the row pitch and the window width apart, a window
// starts at byte 3x of a frame row, so the staged runs are unaligned in general.  Bit for bit what letterbox_kernel computes
// on the window copied out contiguously.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void window_views_kernel(const uint8_t* __restrict__ src, const ViewWin* __restrict__ wins,
                                                           uint8_t* __restrict__ dst, int slot0, int S, int row_cap) {
  extern __shared__ __attribute__((aligned(16))) uint8_t band[];   // [2 * LB_TH][row_cap]
  __shared__ int s_shift[2 * LB_TH];                                // byte index of window byte b0 inside an LDS row
  const int n = blockIdx.z;
  const ViewWin vw = wins[n];
  lb_tile(lb_source(src, vw), lb_place(vw), dst + (long)(slot0 + n) * S * S * 3, S, S, band, row_cap, s_shift);
}

// per-pixel form, straight from global memory: the windows whose source row span exceeds the LDS rows
__global__ __launch_bounds__(256) void window_views_pixel_kernel(const uint8_t* __restrict__ src, const ViewWin* __restrict__ wins,
                                                                 uint8_t* __restrict__ dst, int slot0, int S) {
  const int n = blockIdx.y;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= S * S) return;
  const ViewWin vw = wins[n];
  lb_pixel_thread(lb_source(src, vw), lb_place(vw), dst + (long)(slot0 + n) * S * S * 3, S, idx);
}

void launch_window_views(const uint8_t* src, const ViewWin* wins, uint8_t* dst, int slot0, int n, int S, hipStream_t st,
                         const ViewWin* host_wins) {
  if (n <= 0) return;
  LP_CHECK(S % 4 == 0 && host_wins, LP_ERR_ARG, "window views need det_input %% 4 == 0");
  int cap = 0;
  for (int i = 0; i < n; ++i) cap = std::max(cap, lb_row_cap(host_wins[i].w, host_wins[i].new_w, LB_TW));
  if (lb_rows_fit(cap)) {
    dim3 grid(ceil_div(S, LB_TW), ceil_div(S, LB_TH), n);
    LP_LAUNCH(window_views_kernel, grid, dim3(256), (size_t)cap * 2 * LB_TH, st, src, wins, dst, slot0, S, cap);
  } else {
    dim3 grid(ceil_div(S * S, 256), n);
    LP_LAUNCH(window_views_pixel_kernel, grid, dim3(256), 0, st, src, wins, dst, slot0, S);
  }
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Frame NMS of views: the frame front end of the core in nms_dev.h.
// Step 1: one workgroup per view sorts the view's candidates with nms_kernel's sort (nms_sort_to) into the view's slice of
// `sorted`, records the view's count and re-arms cand_count for the next call.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(NMS_THREADS) void view_sort_kernel(const FrameNmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int v = blockIdx.x;
  int cnt = a.cand_count[v];
  cnt = cnt > a.c.A ? a.c.A : cnt;
  __syncthreads();
  if (threadIdx.x == 0) { a.vcnt[v] = cnt; a.cand_count[v] = 0; }
  if (cnt == 0) return;
  nms_sort_to(reinterpret_cast<unsigned long long*>(smem), a.cand + (long)v * a.c.A, a.sorted + (long)v * a.c.A, cnt);
}

// records of another view's descending list [0, n) that precede a candidate of (class, score) key k = nms_key >> 14: those
// with a larger key, and -- when that view's index is higher (inclusive) -- those with an equal one.  The anchor only orders
// records of ONE view: across views the view index decides.
__device__ __forceinline__ int count_before(const Cand* list, int n, unsigned long long k, bool inclusive) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const unsigned long long m = nms_key(list[mid]) >> 14;
    if (inclusive ? (m >= k) : (m > k)) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// candidate t of a frame's view-major concatenation: view k, position p inside the view's sorted list
__device__ __forceinline__ void frame_locate(const FrameNmsArgs& a, const TileFrame& fr, int t, int& k, int& p) {
  k = 0;
  p = t;
  while (k < fr.nviews - 1) {
    const int c = a.vcnt[a.vslot[fr.view0 + k]];
    if (p < c) break;
    p -= c;
    ++k;
  }
}

// One-wave path (nms_small_tail): lane t holds candidate t of the concatenation; its rank in the merged order is counted
// against the other 63 lanes with shuffles, the records are gathered by rank.
template <bool IOS, bool UNI>
__device__ __forceinline__ void frame_nms_small(const FrameNmsArgs& a, int f, const TileFrame& fr, int cnt, int nframes) {
  const int lane = threadIdx.x & 63;
  Cand c;
  c.x1 = c.y1 = c.x2 = c.y2 = c.score = 0.f; c.cls = -1; c.anchor = 0; c.pad = 0;
  int view = 0;
  if (lane < cnt) {
    int p;
    frame_locate(a, fr, lane, view, p);
    c = a.sorted[(long)a.vslot[fr.view0 + view] * a.c.A + p];
    c.pad = view;
  }
  const unsigned long long key = lane < cnt ? nms_key(c) : 0ull;
  int rank = 0;
  for (int j = 0; j < 64; ++j) {
    const unsigned lo = __shfl((unsigned)key, j), hi = __shfl((unsigned)(key >> 32), j);
    const unsigned long long ok = ((unsigned long long)hi << 32) | lo;
    const int ov = __shfl(view, j);
    const unsigned long long oh = ok >> 14, h = key >> 14;   // (class, score); then the view; inside one view the anchor
    rank += (j < cnt && (oh > h || (oh == h && (ov > view || (ov == view && ok > key))))) ? 1 : 0;
  }
  if (lane >= cnt) rank = lane;   // the empty lanes keep their places behind the real ones
  int src = lane;
  for (int j = 0; j < 64; ++j)
    if (__shfl(rank, j) == lane) src = j;
  Cand bj;
  bj.x1 = __shfl(c.x1, src); bj.y1 = __shfl(c.y1, src); bj.x2 = __shfl(c.x2, src); bj.y2 = __shfl(c.y2, src);
  bj.score = __shfl(c.score, src); bj.cls = __shfl(c.cls, src); bj.anchor = __shfl(c.anchor, src); bj.pad = __shfl(c.pad, src);
  nms_small_tail<IOS, UNI>(a.c, a.fgeom[f], f, nframes, bj, cnt);
}

// ------------------------------------------------------------------------------------
// Step 2: one workgroup per frame.  Merge: candidate p of view k finds its rank in the union by binary search in the frame's
// other sorted lists -- the order is (class asc, score desc, view desc, anchor desc): nms_kernel's order with the view above
// the anchor -- and is written to the frame's contiguous region of `cand` (free since step 1), its view index in Cand::pad.
// Then nms_finish.  IOS: the match is intersection over the smaller area.  UNI: a keeper's emitted box is the union of its own
// and of every box it absorbs.  <false, false> is the reference's rule (e2e.py:89-119).
// ------------------------------------------------------------------------------------
template <bool IOS, bool UNI>
__global__ __launch_bounds__(NMS_THREADS) void frame_nms_kernel(const FrameNmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int f = blockIdx.x;
  const TileFrame fr = a.frames[f];
  int cnt = 0;
  for (int k = 0; k < fr.nviews; ++k) cnt += a.vcnt[a.vslot[fr.view0 + k]];
  if (cnt <= 64 && cnt <= a.c.max_det && !a.c.no_small) {   // block-uniform
    if (threadIdx.x < 64) frame_nms_small<IOS, UNI>(a, f, fr, cnt, (int)gridDim.x);
    return;
  }
  Cand* merged = a.cand + (long)fr.view0 * a.c.A;
  for (int t = threadIdx.x; t < cnt; t += NMS_THREADS) {
    int k, p;
    frame_locate(a, fr, t, k, p);
    Cand c = a.sorted[(long)a.vslot[fr.view0 + k] * a.c.A + p];
    const unsigned long long key = nms_key(c);
    int rank = p;
    for (int u = 0; u < fr.nviews; ++u) {
      if (u == k) continue;
      const int su = a.vslot[fr.view0 + u];
      rank += count_before(a.sorted + (long)su * a.c.A, a.vcnt[su], key >> 14, u > k);
    }
    c.pad = k;
    merged[rank] = c;
  }
  nms_finish<IOS, UNI>(a.c, a.fgeom[f], merged, cnt, f, (int)gridDim.x, reinterpret_cast<unsigned*>(smem));
}

size_t frame_nms_lds_bytes(int max_union) { return (size_t)2 * 4 * ((max_union + 31) / 32) + 16; }

void launch_view_sort(const FrameNmsArgs& a, int V, hipStream_t st) {
  LP_CHECK(a.c.A <= 16384, LP_ERR_STATE, "frame NMS: anchor index needs more than 14 key bits");
  const size_t lds = nms_lds_bytes(a.c.A);
  LP_CHECK(lds <= 150 * 1024, LP_ERR_STATE, "frame NMS: %d anchors exceed the LDS sort capacity", a.c.A);
  set_max_dynamic_lds(reinterpret_cast<const void*>(view_sort_kernel), 150 * 1024);
  LP_LAUNCH(view_sort_kernel, dim3(V), dim3(NMS_THREADS), lds, st, a);
  LP_HIP(hipGetLastError());
}

template <bool IOS, bool UNI>
static void launch_frame_nms_as(const FrameNmsArgs& b, int F, size_t lds, hipStream_t st) {
  set_max_dynamic_lds(reinterpret_cast<const void*>(frame_nms_kernel<IOS, UNI>), FRAME_NMS_LDS_CAP);
  LP_LAUNCH((frame_nms_kernel<IOS, UNI>), dim3(F), dim3(NMS_THREADS), lds, st, b);
}

void launch_frame_nms(const FrameNmsArgs& a, int F, int max_views, hipStream_t st) {
  LP_CHECK(max_views >= 1 && max_views <= 1024, LP_ERR_ARG, "frame NMS: %d views in one frame (1..1024)", max_views);
  const size_t lds = frame_nms_lds_bytes(max_views * a.c.A);
  LP_CHECK(lds <= FRAME_NMS_LDS_CAP, LP_ERR_ARG, "frame NMS: a frame of %d views x %d anchors exceeds the LDS flag capacity", max_views, a.c.A);
  FrameNmsArgs b = a;
  b.c.no_small = nms_no_small(a.c.no_small);
  LP_CHECK((a.metric == 0 || a.metric == 1) && (a.mode == 0 || a.mode == 1), LP_ERR_ARG, "frame NMS: metric %d / mode %d", a.metric, a.mode);
  switch (a.metric * 2 + a.mode) {   // chosen on the host: the default instantiation carries none of the merge
    case 0: launch_frame_nms_as<false, false>(b, F, lds, st); break;
    case 1: launch_frame_nms_as<false, true>(b, F, lds, st); break;
    case 2: launch_frame_nms_as<true, false>(b, F, lds, st); break;
    default: launch_frame_nms_as<true, true>(b, F, lds, st); break;
  }
  LP_HIP(hipGetLastError());
}

}  // namespace lp
