// Detector post-processing and ROI extraction on the GPU.  Replaces the NumPy code of
// NCNNDetector.postprocess / nms_numpy (reference e2e.py:240-296, 89-119), the ROI loop of
// HybridPipeline.run (e2e.py:465-473) and the PIL resize of PyTorchClassifier.predict_batch
// (e2e.py:385-389).  Everything that decides WHICH boxes survive is computed with explicit
// round-to-nearest fp32 operations in the reference's operation order (no FMA contraction),
// so that for the same out0 tensor the kept set is identical to the NumPy result.
#include "common.h"
#include "kernels.h"
#include "nms_dev.h"
#include "post_dev.h"
#include <atomic>
#include <cstdlib>

namespace lp {

typedef _Float16 half_t;

// ------------------------------------------------------------------------------------
// Detect head decode (model.ncnn.param:184-208): per anchor, softmax over reg_max bins of
// each box side, expectation with the DFL weights, dist2bbox around the anchor point,
// x stride; class sigmoid.  One thread per (image, anchor).
// ------------------------------------------------------------------------------------
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));
template <typename T> struct DecVec;
template <> struct DecVec<half_t> { typedef half8_t type; static constexpr int G = 8; };
template <> struct DecVec<float> { typedef float4_t type; static constexpr int G = 4; };
template <typename T> __device__ __forceinline__ float dec_exp(float x);
template <> __device__ __forceinline__ float dec_exp<half_t>(float x) { return __expf(x); }
template <> __device__ __forceinline__ float dec_exp<float>(float x) { return expf(x); }

// Four adjacent lanes share one anchor, one box side each: a wave reads 16 anchors x 4*reg_max
// channels = fully coalesced 16-byte loads.  The side-0 lane then gathers the four distances
// with wave shuffles and finishes the anchor.
template <typename T, int RM>
__global__ __launch_bounds__(256) void decode_kernel(const DecodeArgs a) {
  typedef typename DecVec<T>::type vec;
  constexpr int G = DecVec<T>::G;
  const int n = blockIdx.y;
  const int gid = blockIdx.x * 256 + threadIdx.x;
  int anchor = gid >> 2;
  const int side = gid & 3;
  const bool live = anchor < a.A;
  anchor = live ? anchor : a.A - 1;
  int l = 0;
  for (int i = 1; i < a.nlevels; ++i)
    if (anchor >= a.lv[i].anchor_off) l = i;
  const DecodeLevel lv = a.lv[l];
  const long pix = (long)n * lv.H * lv.W + (anchor - lv.anchor_off);
  const T* b = reinterpret_cast<const T*>(lv.box) + pix * lv.box_pitch + side * RM;
  float v[RM];
#pragma unroll
  for (int q = 0; q < RM / G; ++q) {
    const vec x = *reinterpret_cast<const vec*>(b + q * G);
#pragma unroll
    for (int i = 0; i < G; ++i) v[q * G + i] = (float)x[i];
  }
  float mx = v[0];
#pragma unroll
  for (int i = 1; i < RM; ++i) mx = fmaxf(mx, v[i]);
  float sum = 0.f, ex = 0.f;
#pragma unroll
  for (int i = 0; i < RM; ++i) {
    const float e = dec_exp<T>(v[i] - mx);
    sum += e;
    ex += e * a.dfl_w[i];
  }
  const float dist = ex / sum;
  const int lane = threadIdx.x & 63, base = lane & ~3;
  const float d0 = __shfl(dist, base), d1 = __shfl(dist, base + 1), d2 = __shfl(dist, base + 2), d3 = __shfl(dist, base + 3);
  if (side != 0 || !live) return;
  const T* cls = reinterpret_cast<const T*>(lv.cls) + pix * lv.cls_pitch;
  const float ax = a.anchors[anchor], ay = a.anchors[a.A + anchor], s = a.strides[anchor];
  const float x1 = ax - d0, y1 = ay - d1, x2 = ax + d2, y2 = ay + d3;
  const float cx = (x1 + x2) * 0.5f * s, cy = (y1 + y2) * 0.5f * s;
  const float w = (x2 - x1) * s, h = (y2 - y1) * s;
  float best = -1.f;
  int best_c = 0;
  float* o = a.out0 ? a.out0 + (long)n * (4 + a.nc) * a.A + anchor : nullptr;
  for (int c = 0; c < a.nc; ++c) {
    const float sc = 1.f / (1.f + dec_exp<T>(-(float)cls[c]));
    if (o) o[(long)(4 + c) * a.A] = sc;
    if (sc > best) { best = sc; best_c = c; }
  }
  if (o) {
    o[0] = cx; o[(long)a.A] = cy; o[2L * a.A] = w; o[3L * a.A] = h;
  }
  emit_candidate(cx, cy, w, h, best, best_c, anchor, a.geom[n], a.conf, a.cand + (long)n * a.A, a.cand_count + n);
}

void launch_decode(int prec, const DecodeArgs& a, int N, hipStream_t st) {
  dim3 grid(ceil_div(a.A * 4, 256), N);
  LP_CHECK(a.reg_max == 16 || a.reg_max == 8 || a.reg_max == 32, LP_ERR_GRAPH, "reg_max %d unsupported (8, 16, 32)", a.reg_max);
#define LP_DEC(TT)                                                                           \
  if (a.reg_max == 16) LP_LAUNCH((decode_kernel<TT, 16>), grid, dim3(256), 0, st, a); \
  else if (a.reg_max == 8) LP_LAUNCH((decode_kernel<TT, 8>), grid, dim3(256), 0, st, a); \
  else LP_LAUNCH((decode_kernel<TT, 32>), grid, dim3(256), 0, st, a);
  if (prec == LP_FP16) { LP_DEC(half_t) } else { LP_DEC(float) }
#undef LP_DEC
  LP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void filter_out0_kernel(const float* __restrict__ out0, int nc, int A,
                                                          const ImgGeom* __restrict__ geom, Cand* cand, int* cand_count,
                                                          float conf) {
  const int n = blockIdx.y;
  const int anchor = blockIdx.x * 256 + threadIdx.x;
  if (anchor >= A) return;
  const float* o = out0 + (long)n * (4 + nc) * A + anchor;
  float best = -INFINITY;
  int best_c = 0;
  for (int c = 0; c < nc; ++c) {
    const float sc = o[(long)(4 + c) * A];
    if (sc > best) { best = sc; best_c = c; }
  }
  emit_candidate(o[0], o[(long)A], o[2L * A], o[3L * A], best, best_c, anchor, geom[n], conf, cand + (long)n * A,
                 cand_count + n);
}

void launch_filter_out0(const float* out0, int nc, int A, const ImgGeom* geom, Cand* cand, int* cand_count, float conf,
                        int N, hipStream_t st) {
  dim3 grid(ceil_div(A, 256), N);
  LP_LAUNCH(filter_out0_kernel, grid, dim3(256), 0, st, out0, nc, A, geom, cand, cand_count, conf);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Per-class greedy NMS, one workgroup per image: the image front end of the core in nms_dev.h.  The candidates are sorted by
// nms_key (class ascending, score descending, ties -> higher anchor first) and handed to nms_finish<false, false>: the
// reference's rule, the one-view case of the frame NMS (tile_kernels.hip).
// ------------------------------------------------------------------------------------
size_t nms_lds_bytes(int A) {   // the sort's keys; the general path's flag masks overlay them once the sort is done
  int npad = 1;
  while (npad < A) npad <<= 1;
  return (size_t)npad * 8 + 16;
}

// One-wave path (nms_small_tail): lane i loads candidate i, the 64 keys are bitonic-sorted with lane shuffles (21
// compare-exchange steps, the source lane travels with the key), the records are gathered from their source lanes.
// Same keys as the LDS sort, so the same order.  25 -> ~8 us per launch.
__device__ __forceinline__ void nms_small(const NmsArgs& a, int n, int cnt, int nimg) {
  const int lane = threadIdx.x & 63;
  const Cand* cand = a.cand + (long)n * a.c.A;
  Cand c;
  c.x1 = c.y1 = c.x2 = c.y2 = c.score = 0.f; c.cls = -1; c.anchor = 0; c.pad = 0;
  if (lane < cnt) c = cand[lane];
  unsigned long long key = lane < cnt ? nms_key(c) : 0ull;   // the zero keys of the empty lanes sort behind every real one
  int src = lane;
  // (rolled on purpose: one wave executes this once per image, from a cold instruction cache -- 21 unrolled stages were ~2.5 KB of
  //  straight-line code, each 64-byte line a fetch from L2 that nothing hides)
#pragma unroll 1
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll 1
    for (int j = k >> 1; j > 0; j >>= 1) {
      const unsigned lo = __shfl_xor((unsigned)key, j), hi = __shfl_xor((unsigned)(key >> 32), j);
      const unsigned long long okey = ((unsigned long long)hi << 32) | lo;
      const int osrc = __shfl_xor(src, j);
      const bool lower = (lane & j) == 0, desc = (lane & k) == 0;   // as the LDS sort: the lower index of a descending pair keeps the larger key
      const bool take = (lower == desc) ? (okey > key) : (okey < key);
      key = take ? okey : key;
      src = take ? osrc : src;
    }
  }
  Cand bj;
  bj.x1 = __shfl(c.x1, src); bj.y1 = __shfl(c.y1, src); bj.x2 = __shfl(c.x2, src); bj.y2 = __shfl(c.y2, src);
  bj.score = __shfl(c.score, src); bj.cls = __shfl(c.cls, src); bj.anchor = __shfl(c.anchor, src); bj.pad = 0;
  nms_small_tail<false, false>(a.c, a.geom[n], n, nimg, bj, cnt);
  if (lane == 0) a.cand_count[n] = 0;  // ready for the next call
}

__global__ __launch_bounds__(NMS_THREADS) void nms_kernel(const NmsArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int n = blockIdx.x;
  int cnt = a.cand_count[n];
  cnt = cnt > a.c.A ? a.c.A : cnt;
  if (cnt <= 64 && cnt <= a.c.max_det && !a.c.no_small) {   // block-uniform: the other 15 waves leave before any barrier
    if (threadIdx.x < 64) nms_small(a, n, cnt, (int)gridDim.x);
    return;
  }
  Cand* sorted = a.sorted + (long)n * a.c.A;
  nms_sort_to(reinterpret_cast<unsigned long long*>(smem), a.cand + (long)n * a.c.A, sorted, cnt);
  __syncthreads();   // the keys are dead from here on
  nms_finish<false, false>(a.c, a.geom[n], sorted, cnt, n, (int)gridDim.x, reinterpret_cast<unsigned*>(smem));
  if (threadIdx.x == 0) a.cand_count[n] = 0;  // ready for the next call
}

int nms_no_small(int no_small) {
  // A/B switch + the path-equivalence tests (read per enqueue: a captured graph keeps what it saw)
  return getenv("LITEPI_NMS_NO_SMALL") != nullptr ? 1 : no_small;
}

void launch_nms(const NmsArgs& a, int N, hipStream_t st) {
  set_max_dynamic_lds(reinterpret_cast<const void*>(nms_kernel), 150 * 1024);
  const size_t lds = nms_lds_bytes(a.c.A);
  LP_CHECK(lds <= 150 * 1024, LP_ERR_STATE, "NMS: %d anchors exceed the LDS sort capacity", a.c.A);
  LP_CHECK(a.c.A <= 16384, LP_ERR_STATE, "NMS: anchor index needs more than 14 key bits");
  NmsArgs b = a;
  b.c.no_small = nms_no_small(a.c.no_small);
  LP_LAUNCH(nms_kernel, dim3(N), dim3(NMS_THREADS), lds, st, b);
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// PIL Image.resize((S,S), BILINEAR) of every ROI (Pillow libImaging Resample.c): triangle filter scaled by the
// down-sampling factor, coefficients normalised in double and quantised to 22-bit fixed point, horizontal pass to
// uint8 then vertical pass to uint8.  Pinned against Pillow itself through oracle/pil_resize_ref.py.
//
// The work unit is (ROI, strip of 16 output rows): four units per ROI, dealt grid-stride over workgroups of four waves
// that need 39 KB of LDS, so four of them share a CU whatever the ROI's size.  A unit builds the x table for the 64 output
// columns and the y table of its own 16 rows, and touches only the input rows its strip reads
// (by[y0].ymin .. by[y0 + 15].ymin + ny: at most 102 rows for sides <= 384).  Both passes are integer sums, so the
// split changes no byte.
//   banded (sides <= 384 px: at most 13 taps): the strip's input rows are copied into LDS in bands with aligned
//          dword loads, each band is resampled horizontally into the strip's uint8 intermediate [rows][S][3] (Pillow's
//          intermediate image), then the vertical pass runs on dwords
//   large  (sides up to 4096 px, 129 taps): the strip's input rows stream through a 16-row chunk, taps gathered from
//          global memory; every output row of the strip accumulates its share of a chunk
// ------------------------------------------------------------------------------------
#define RR_THREADS 256
#define RR_WAVES (RR_THREADS / 64)
#define RR_WG_PER_CU 4
#define RR_LDS_BYTES (39 * 1024)  /* x 4 workgroups = 156 of the CU's 160 KB */
#define RR_PRECISION_BITS 22
#define RR_S 64       /* output side: one wave per row of the horizontal pass, lane = output column */
#define RR_STRIP 16   /* output rows per unit */
#define RR_SMALL_SIDE 384
#define RR_SMALL_K 13
#define RR_STRIP_ROWS 102  /* input rows one strip reads, in_h <= RR_SMALL_SIDE */
#define RR_LARGE_SIDE 4096
#define RR_LARGE_K 129
#define RR_LARGE_CHUNK 16
#define RR_COPY_ROWS 6
#define RR_ROWB (RR_S * 3)
#define RR_BANDED_TABLES ((RR_S + RR_STRIP) * (RR_SMALL_K + 2) * 4)
static_assert(RR_BANDED_TABLES % 16 == 0, "the intermediate image starts on a 16-byte boundary");
// the widest crop row (1156 bytes) still gets 13 rows per band beside a full intermediate image
#define RR_TAP_SLACK 64  /* >= 13 taps x 3 bytes behind a row's end */
static_assert(RR_LDS_BYTES - RR_BANDED_TABLES - RR_TAP_SLACK - RR_STRIP_ROWS * RR_ROWB >= 13 * ((RR_SMALL_SIDE * 3 + 6) & ~3), "band");

// tap x of output index xx (Pillow's precompute_coeffs + normalize_coeffs_8bpc, one tap per thread); the x == 0 thread also
// writes the window bounds {xmin, n}
__device__ void pil_coeff_tap(int in_size, int out_size, int xx, int x, int* k, int* bounds) {
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 1.0 * filterscale;
  const double ss = 1.0 / filterscale;
  const double center = (xx + 0.5) * scale;
  int xmin = (int)(center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  xmax -= xmin;
  if (x == 0) { bounds[0] = xmin; bounds[1] = xmax; }
  if (x >= xmax) return;
  double ww = 0.0;
  for (int t = 0; t < xmax; ++t) {
    double v = (t + xmin - center + 0.5) * ss;
    v = v < 0 ? -v : v;
    ww += v < 1.0 ? 1.0 - v : 0.0;
  }
  double v = (x + xmin - center + 0.5) * ss;
  v = v < 0 ? -v : v;
  double w = v < 1.0 ? 1.0 - v : 0.0;
  if (ww != 0.0) w /= ww;
  k[x] = w < 0 ? (int)(-0.5 + w * (double)(1 << RR_PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << RR_PRECISION_BITS));
}

// An upper bound of the window sizes of one axis: n < 2 * support + 1 with support = max(1, in / S), so
// n <= ceil(2 * in / S) <= 2 * in / S + 1 in integers; one more for good measure.  Taps beyond it are not visited.
__device__ __forceinline__ int rr_tap_bound(int in_size, int maxk) {
  const int b = in_size <= RR_S ? 3 : 2 * in_size / RR_S + 2;
  return b < maxk ? b : maxk;
}

__device__ __forceinline__ int clip8(int v) {
  v >>= RR_PRECISION_BITS;
  return v < 0 ? 0 : (v > 255 ? 255 : v);
}

struct RrUnit {
  const uint8_t* src;      // the image's first byte
  const uint8_t* img_end;  // one past its last
  uint8_t* out;            // the ROI's [S][S][3]
  int rx, ry, in_w, in_h;
  int w;                   // image width
  int y0;                  // first output row of the strip
};

// first byte of the ROI's row `row` (workgroup-uniform)
__device__ __forceinline__ const uint8_t* rr_row(const RrUnit& u, int row) { return u.src + ((long)(u.ry + row) * u.w + u.rx) * 3; }

// The aligned dwords that hold ROI row `row` (the row's bytes keep their global address modulo 4 in the LDS copy), all
// wave-uniform: dwords [0, nd) cover the row, of which [jlo, jhi) lie inside the image and are read whole.  Only the image's
// first and last dword can straddle its ends -- and with them the caller's buffer --, so jlo > 0 or jhi < nd happens on at most
// two rows of a frame: those dwords are read byte-wise (rr_edge_dword).
struct RrRow {
  const uint8_t* base;  // rp & ~3
  int al, nd, jlo, jhi;
};
__device__ __forceinline__ RrRow rr_row_dwords(const RrUnit& u, int row) {
  const uint8_t* rp = rr_row(u, row);
  RrRow r;
  r.al = (int)(reinterpret_cast<uintptr_t>(rp) & 3);
  r.base = rp - r.al;
  r.nd = (r.al + u.in_w * 3 + 3) >> 2;
  const long before = r.base - u.src, room = (u.img_end - r.base) >> 2;  // before >= -3; whole dwords up to the image's end
  r.jlo = before < 0 ? 1 : 0;
  r.jhi = room < r.nd ? (int)room : r.nd;
  return r;
}
__device__ __forceinline__ uint32_t rr_edge_dword(const RrUnit& u, const uint8_t* ap) {
  uint32_t x = 0;
  for (int b = 0; b < 4; ++b)
    if (ap + b >= u.src && ap + b < u.img_end) x |= (uint32_t)ap[b] << (8 * b);
  return x;
}

// horizontal pass of the band's rows `wave`, `wave` + 4, ...: lane = xx, NT taps from registers (zero beyond the lane's own
// window, so every lane runs the same straight line), three channels, BGR -> RGB
template <int NT>
__device__ __forceinline__ void rr_hpass(const RrUnit& u, const uint8_t* crop, uint8_t* tmp_band, int pitch, int row0, int nb, int wave,
                                         int lane, int xmin, const int (&kr)[RR_SMALL_K]) {
  const int half = 1 << (RR_PRECISION_BITS - 1);
  for (int row = wave; row < nb; row += RR_WAVES) {
    const int al = (int)(reinterpret_cast<uintptr_t>(rr_row(u, row0 + row)) & 3);
    const uint8_t* p = crop + row * pitch + al + xmin * 3;
    uint8_t* o = tmp_band + row * RR_ROWB + lane * 3;
    if (NT == 0) {  // Pillow skips the pass when the width already matches (identity either way)
      o[0] = p[2]; o[1] = p[1]; o[2] = p[0];
    } else {
      unsigned a0 = half, a1 = half, a2 = half;
#pragma unroll
      for (int x = 0; x < NT; ++x) {
        a0 += __umul24(p[x * 3 + 2], (unsigned)kr[x]);   // coefficients are in [0, 2^22]: the 24-bit product is the product
        a1 += __umul24(p[x * 3 + 1], (unsigned)kr[x]);
        a2 += __umul24(p[x * 3 + 0], (unsigned)kr[x]);
      }
      o[0] = (uint8_t)clip8((int)a0); o[1] = (uint8_t)clip8((int)a1); o[2] = (uint8_t)clip8((int)a2);
    }
  }
}

__device__ __forceinline__ void rr_strip_banded(const RrUnit& u, char* smem) {
  constexpr int K = RR_SMALL_K;
  int* kx = reinterpret_cast<int*>(smem);  // [S][K]
  int* ky = kx + RR_S * K;                 // [STRIP][K]
  int* bx = ky + RR_STRIP * K;             // [S][2]
  int* by = bx + 2 * RR_S;                 // [STRIP][2]
  uint8_t* tmp = reinterpret_cast<uint8_t*>(by + 2 * RR_STRIP);  // [rows][S][3]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: a wave's row address, alignment and dword count are too
  const int half = 1 << (RR_PRECISION_BITS - 1);
  // one thread per (output index, tap), tap-major so that whole waves share a tap: Pillow's double arithmetic in Pillow's
  // order (the weight sum is re-done by every tap's thread), so the table costs one division of latency instead of a serial loop
  const int kbx = rr_tap_bound(u.in_w, K), kby = rr_tap_bound(u.in_h, K);
  const int kb = kbx > kby ? kbx : kby;
  for (int i = tid; i < kb * (RR_S + RR_STRIP); i += RR_THREADS) {
    const int x = i / (RR_S + RR_STRIP), idx = i - x * (RR_S + RR_STRIP);
    if (idx < RR_S) {
      if (x < kbx) pil_coeff_tap(u.in_w, RR_S, idx, x, kx + idx * K, bx + 2 * idx);
    } else {
      const int yy = idx - RR_S;
      if (x < kby) pil_coeff_tap(u.in_h, RR_S, u.y0 + yy, x, ky + yy * K, by + 2 * yy);
    }
  }
  __syncthreads();
  const int ya = by[0];                                              // first input row of the strip
  const int nrows = by[2 * RR_STRIP - 2] + by[2 * RR_STRIP - 1] - ya;  // <= RR_STRIP_ROWS
  uint8_t* crop = tmp + nrows * RR_ROWB;
  const int pitch = (u.in_w * 3 + 3 + 3) & ~3;  // row pitch of the LDS copy
  // rows per band (>= 13); RR_TAP_SLACK bytes stay free behind the band: a lane reads the widest window of its wave
  const int rpb = (RR_LDS_BYTES - RR_BANDED_TABLES - RR_TAP_SLACK - nrows * RR_ROWB) / pitch;
  // the lane's column of the horizontal pass, in registers for the whole unit
  const int xmin = bx[2 * lane], nx = bx[2 * lane + 1];
  int kr[K];
#pragma unroll
  for (int x = 0; x < K; ++x) kr[x] = x < nx ? kx[lane * K + x] : 0;
  int nxmax = nx;
  for (int off = 32; off > 0; off >>= 1) nxmax = max(nxmax, __shfl_xor(nxmax, off));
  nxmax = __builtin_amdgcn_readfirstlane(nxmax);
  for (int r0 = 0; r0 < nrows; r0 += rpb) {
    const int nb = nrows - r0 < rpb ? nrows - r0 : rpb;
    // 1. band -> LDS: a wave takes a row, its lanes stride the row's dwords.  Twelve loads per thread (six rows, two
    //    dwords of each) are requested before the first store: the copy is a chain of memory round trips, and four waves
    //    hide none of them
    for (int rw = wave; rw < nb; rw += RR_WAVES * RR_COPY_ROWS) {
      for (int j0 = lane; j0 < (pitch >> 2); j0 += 128) {
        uint32_t v[RR_COPY_ROWS][2];
#pragma unroll
        for (int q = 0; q < RR_COPY_ROWS; ++q) {
          const int row = rw + q * RR_WAVES;
          const RrRow rr = rr_row_dwords(u, ya + r0 + (row < nb ? row : nb - 1));
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int j = j0 + 64 * t;
            v[q][t] = 0u;
            if (row < nb && j >= rr.jlo && j < rr.jhi) v[q][t] = *reinterpret_cast<const uint32_t*>(rr.base + 4 * j);
          }
        }
#pragma unroll
        for (int q = 0; q < RR_COPY_ROWS; ++q) {
          const int row = rw + q * RR_WAVES;
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            const int j = j0 + 64 * t;
            if (row < nb && j < (pitch >> 2)) *reinterpret_cast<uint32_t*>(crop + row * pitch + 4 * j) = v[q][t];
          }
        }
      }
    }
    // (the image's first and last dword, after the wave's own zero store to the same place)
    for (int row = wave; row < nb; row += RR_WAVES) {
      const RrRow rr = rr_row_dwords(u, ya + r0 + row);
      if (rr.jlo > 0 || rr.jhi < rr.nd) {  // wave-uniform, two rows of a frame at the most
        const int j = lane == 0 ? 0 : rr.nd - 1;
        if (lane < 2 && (j < rr.jlo || j >= rr.jhi))
          *reinterpret_cast<uint32_t*>(crop + row * pitch + 4 * j) = rr_edge_dword(u, rr.base + 4 * j);
      }
    }
    __syncthreads();
    // 2. horizontal pass of the band, unrolled for the widest window of the x table
    uint8_t* tb = tmp + r0 * RR_ROWB;
    if (u.in_w == RR_S) rr_hpass<0>(u, crop, tb, pitch, ya + r0, nb, wave, lane, xmin, kr);
    else if (nxmax <= 3) rr_hpass<3>(u, crop, tb, pitch, ya + r0, nb, wave, lane, xmin, kr);
    else if (nxmax <= 5) rr_hpass<5>(u, crop, tb, pitch, ya + r0, nb, wave, lane, xmin, kr);
    else if (nxmax <= 8) rr_hpass<8>(u, crop, tb, pitch, ya + r0, nb, wave, lane, xmin, kr);
    else rr_hpass<K>(u, crop, tb, pitch, ya + r0, nb, wave, lane, xmin, kr);
    __syncthreads();
  }
  // 3. vertical pass on dwords: four bytes of an output row per thread
  const uint32_t* tmp32 = reinterpret_cast<const uint32_t*>(tmp);
  uint32_t* out32 = reinterpret_cast<uint32_t*>(u.out + u.y0 * RR_ROWB);
  for (int i = tid; i < RR_STRIP * (RR_ROWB / 4); i += RR_THREADS) {
    const int yy = i / (RR_ROWB / 4), dj = i - yy * (RR_ROWB / 4);
    const int ymin = by[2 * yy] - ya, ny = by[2 * yy + 1];
    const uint32_t* col = tmp32 + ymin * (RR_ROWB / 4) + dj;
    uint32_t v;
    if (u.in_h == RR_S) {
      v = col[0];
    } else {
      const int* k = ky + yy * K;
      unsigned a0 = half, a1 = half, a2 = half, a3 = half;
      for (int y = 0; y < ny; ++y) {
        const uint32_t t = col[y * (RR_ROWB / 4)];
        const unsigned w = (unsigned)k[y];
        a0 += __umul24(t & 255u, w);
        a1 += __umul24((t >> 8) & 255u, w);
        a2 += __umul24((t >> 16) & 255u, w);
        a3 += __umul24(t >> 24, w);
      }
      v = (uint32_t)clip8((int)a0) | ((uint32_t)clip8((int)a1) << 8) | ((uint32_t)clip8((int)a2) << 16) | ((uint32_t)clip8((int)a3) << 24);
    }
    out32[i] = v;
  }
}

// LDS of the large variant: bounds, the strip's y table, the chunk of resampled rows, then the x table of `xw` output columns
__device__ __forceinline__ int rr_large_lds(int skx, int sky, int xw) {
  return (2 * RR_S + 2 * RR_STRIP + RR_STRIP * sky + xw * skx) * 4 + RR_LARGE_CHUNK * RR_ROWB;
}

__device__ __forceinline__ void rr_strip_large(const RrUnit& u, char* smem) {
  const int tid = threadIdx.x;
  const int half = 1 << (RR_PRECISION_BITS - 1);
  const int kbx = rr_tap_bound(u.in_w, RR_LARGE_K), kby = rr_tap_bound(u.in_h, RR_LARGE_K);
  const int skx = kbx | 1, sky = kby | 1;  // odd table pitches (<= 129): lanes on distinct banks
  // the x table is staged in two halves of 32 output columns when both tables at full size would pass the LDS request
  const int xw = rr_large_lds(skx, sky, RR_S) <= RR_LDS_BYTES ? RR_S : RR_S / 2;
  const int xsh = xw == RR_S ? 6 : 5;
  int* bx = reinterpret_cast<int*>(smem);  // [S][2]
  int* by = bx + 2 * RR_S;                 // [STRIP][2]
  int* ky = by + 2 * RR_STRIP;             // [STRIP][sky]
  uint8_t* hrow = reinterpret_cast<uint8_t*>(ky + RR_STRIP * sky);  // [CHUNK][xw][3]
  int* kx = reinterpret_cast<int*>(hrow + RR_LARGE_CHUNK * RR_ROWB);  // [xw][skx]
  for (int i = tid; i < kby * RR_STRIP; i += RR_THREADS) {
    const int x = i >> 4, yy = i & 15;
    pil_coeff_tap(u.in_h, RR_S, u.y0 + yy, x, ky + yy * sky, by + 2 * yy);
  }
  for (int xh = 0; xh < RR_S; xh += xw) {
    __syncthreads();  // (second half: the first half's x table is free)
    for (int i = tid; i < kbx * xw; i += RR_THREADS) {
      const int x = i >> xsh, xl = i & (xw - 1);
      pil_coeff_tap(u.in_w, RR_S, xh + xl, x, kx + xl * skx, bx + 2 * (xh + xl));
    }
    __syncthreads();
    int acc[RR_STRIP];
#pragma unroll
    for (int yy = 0; yy < RR_STRIP; ++yy) acc[yy] = half;
    const bool vcopy = u.in_h == RR_S;  // Pillow skips the vertical pass: output row yy is input row ymin = yy
    const int ya = by[0], yb = by[2 * RR_STRIP - 2] + (vcopy ? 1 : by[2 * RR_STRIP - 1]);
    const int rowb = xw * 3;  // bytes of a chunk row
    for (int c0 = ya; c0 < yb; c0 += RR_LARGE_CHUNK) {
      const int nc = yb - c0 < RR_LARGE_CHUNK ? yb - c0 : RR_LARGE_CHUNK;
      // horizontal pass of the chunk's rows: one thread per (row, column), three channels, BGR -> RGB
      for (int i = tid; i < nc * xw; i += RR_THREADS) {
        const int row = i >> xsh, xl = i & (xw - 1);
        const int xmin = bx[2 * (xh + xl)], nx = bx[2 * (xh + xl) + 1];
        const uint8_t* p = rr_row(u, c0 + row) + xmin * 3;
        uint8_t* o = hrow + row * rowb + xl * 3;
        if (u.in_w == RR_S) {
          o[0] = p[2]; o[1] = p[1]; o[2] = p[0];
        } else {
          const int* k = kx + xl * skx;
          int a0 = half, a1 = half, a2 = half;
#pragma unroll 4
          for (int x = 0; x < nx; ++x) {
            const int w = k[x];
            a0 += (int)p[x * 3 + 2] * w;
            a1 += (int)p[x * 3 + 1] * w;
            a2 += (int)p[x * 3 + 0] * w;
          }
          o[0] = (uint8_t)clip8(a0); o[1] = (uint8_t)clip8(a1); o[2] = (uint8_t)clip8(a2);
        }
      }
      __syncthreads();
      // vertical pass: a thread keeps its byte column; every output row of the strip takes the chunk rows of its window
      if (tid < rowb) {
        for (int row = 0; row < nc; ++row) {
          const int h = hrow[row * rowb + tid];
#pragma unroll
          for (int yy = 0; yy < RR_STRIP; ++yy) {
            const int t = c0 + row - by[2 * yy];
            if (t >= 0 && t < (vcopy ? 1 : by[2 * yy + 1])) {  // workgroup-uniform
              if (vcopy) acc[yy] = h;
              else acc[yy] += h * ky[yy * sky + t];
            }
          }
        }
      }
      __syncthreads();
    }
    if (tid < rowb) {
#pragma unroll
      for (int yy = 0; yy < RR_STRIP; ++yy)
        u.out[(u.y0 + yy) * RR_ROWB + xh * 3 + tid] = (uint8_t)(vcopy ? acc[yy] : clip8(acc[yy]));
    }
  }
}

// cv2.resize(roi_rgb, (S, S), interpolation=cv2.INTER_LINEAR) (e2e_optimize.py:386-390): no antialiasing, two source rows
// and columns per output pixel whatever the ROI's size; BGR -> RGB on the way.  The coefficient triples of the S columns and
// of the strip's rows go through LDS, the pixels are gathered from global memory (4 taps x 3 bytes per output pixel).
__device__ __forceinline__ void rr_strip_linear(const RrUnit& u, char* smem) {
  int* cx = reinterpret_cast<int*>(smem);  // [S][3]: source index, a0, a1
  int* cy = cx + 3 * RR_S;                 // [STRIP][3]
  const int tid = threadIdx.x;
  if (tid < RR_S + RR_STRIP) {
    const int axis = tid >= RR_S, d = tid - axis * RR_S;
    int s0, a0, a1;
    lin_coeff(axis ? u.y0 + d : d, RR_S, axis ? u.in_h : u.in_w, s0, a0, a1);
    int* c = (axis ? cy : cx) + 3 * d;
    c[0] = s0; c[1] = a0; c[2] = a1;
  }
  __syncthreads();
  for (int i = tid; i < RR_STRIP * RR_S; i += RR_THREADS) {
    const int oy = i >> 6, ox = i & 63;
    const int sx = cx[3 * ox], ax0 = cx[3 * ox + 1], ax1 = cx[3 * ox + 2];
    const int sy = cy[3 * oy], ay0 = cy[3 * oy + 1], ay1 = cy[3 * oy + 2];
    const int sx1 = sx + 1 < u.in_w ? sx + 1 : u.in_w - 1;
    const int sy1 = sy + 1 < u.in_h ? sy + 1 : u.in_h - 1;
    const uint8_t* r0 = rr_row(u, sy);
    const uint8_t* r1 = rr_row(u, sy1);
    uint8_t* o = u.out + ((u.y0 + oy) * RR_S + ox) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int v;
      if (u.in_w == RR_S && u.in_h == RR_S) {
        v = r0[sx * 3 + c];   // cv2.resize returns a copy when the size already matches
      } else {
        v = lin_blend(r0[sx * 3 + c], r0[sx1 * 3 + c], r1[sx * 3 + c], r1[sx1 * 3 + c], ax0, ax1, ay0, ay1);
      }
      o[2 - c] = (uint8_t)v;   // BGR -> RGB
    }
  }
}

// One launch for every ROI of the batch: a workgroup takes units u = 4 * ROI + strip round-robin and picks the variant by
// the ROI's size (a launch per variant, two of them usually empty, costs more than the resampling of a typical batch).
__global__ __launch_bounds__(RR_THREADS, RR_WG_PER_CU) void roi_resize_kernel(const RoiResizeArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int U = a.tab.total[0] * (RR_S / RR_STRIP);
  for (int unit = blockIdx.x; unit < U; unit += gridDim.x) {
    const int r = unit >> 2;
    const int img = a.tab.img[r], slot = a.tab.slot[r];
    const ImgGeom gm = a.geom[img];
    const int* rc = a.rects + ((long)img * a.max_det + slot) * 4;
    RrUnit u;
    u.rx = rc[0]; u.ry = rc[1];
    u.in_w = rc[2] - u.rx; u.in_h = rc[3] - u.ry;
    u.w = gm.w;
    u.src = a.src + gm.src_off;
    u.img_end = u.src + (long)gm.h * gm.w * 3;    u.out = a.out + (long)r * RR_S * RR_S * 3;
    u.y0 = (unit & 3) * RR_STRIP;
    if (a.linear) {
      rr_strip_linear(u, smem);
    } else if (u.in_w > RR_LARGE_SIDE || u.in_h > RR_LARGE_SIDE || u.in_w < 1 || u.in_h < 1) {
      // beyond the tap budget: defined (zero) output instead of garbage
      for (int i = threadIdx.x; i < RR_STRIP * RR_ROWB; i += RR_THREADS) u.out[u.y0 * RR_ROWB + i] = 0;
    } else if (u.in_w <= RR_SMALL_SIDE && u.in_h <= RR_SMALL_SIDE) {
      rr_strip_banded(u, smem);
    } else {
      rr_strip_large(u, smem);
    }
    __syncthreads();  // the next unit rewrites the tables
  }
}

// workgroups of the resize kernel that one device holds at a time: its CUs times what the occupancy query admits per CU
static int rr_resident_workgroups() {
  static std::atomic<int> cache[64];
  int dev = 0;
  LP_HIP(hipGetDevice(&dev));
  const int slot = dev & 63;
  int n = cache[slot].load(std::memory_order_relaxed);
  if (n == 0) {
    int cus = 0, per_cu = 0;
    LP_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    LP_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, roi_resize_kernel, RR_THREADS, RR_LDS_BYTES));
    per_cu = per_cu < 1 ? 1 : (per_cu > RR_WG_PER_CU ? RR_WG_PER_CU : per_cu);
    n = (cus < 1 ? 1 : cus) * per_cu;
    cache[slot].store(n, std::memory_order_relaxed);
  }
  return n;
}

void launch_roi_resize(const RoiResizeArgs& a, int max_items, hipStream_t st) {
  LP_CHECK(a.S == RR_S, LP_ERR_ARG, "the ROI resize kernel's tap tables are sized for a 64x64 classifier input (e2e.py:367 resizes to 64x64 whatever --cls_input_size says)");
  LP_CHECK((reinterpret_cast<uintptr_t>(a.out) & 3) == 0, LP_ERR_ARG, "the ROI resize writes dwords: the output must be 4-byte aligned");
  const int resident = rr_resident_workgroups();
  long grid = (long)(max_items < 1 ? 1 : max_items) * (RR_S / RR_STRIP);
  if (grid > resident) grid = resident;
  LP_LAUNCH(roi_resize_kernel, dim3((unsigned)grid), dim3(RR_THREADS), RR_LDS_BYTES, st, a);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
