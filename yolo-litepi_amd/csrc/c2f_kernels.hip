// Whole-C2f launches for gfx950 (fp16 storage, fp32 accumulate).  One workgroup (8 waves) owns a 20x20 tile of one image
// -- the whole image on the 20x20 level -- and runs every layer of a C2f module of the reference graph
// (model.ncnn.param: cv1 -> Slice -> n x [3x3 -> 3x3 -> add] -> Concat -> cv2) back to back:
//
//   [s2]   3x3 stride-2 conv + SiLU in front of the module            (whole-image configurations only)
//   cv1    1x1 + SiLU over concat(src0 [nearest-x2 upsampled], src1)  -> y0 | y1
//   a_k    3x3 + SiLU on y_{k+1}                                     -> mid          (LDS -> LDS)
//   b_k    3x3 + SiLU on mid, + y_{k+1}                              -> y_{k+2}      (LDS -> LDS, in place of y_{k+1})
//   cv2    1x1 + SiLU over concat(y0 .. y_{n+1})                     -> out
//   [sppf] cv1 -> 5x5 max pool x3 -> cv2                              (whole-image configuration of the backbone's last stage)
//
// Data movement rule: ONLY what a 3x3 stride-1 conv (or a pool) reads lives in LDS -- two planes of c channels over the
// tile + halo frame.  Every 1x1 conv takes its pixel operand straight from global memory / L2 (16 B per lane = the MFMA B
// fragment of one pixel's 8 channels), including tensors this workgroup stored a phase earlier (y0 .. y_{n+1} go through the
// module's concat buffer, which exists anyway): the concat is an address, never a copy, and the LDS budget does not depend
// on the module's width.  Weights never touch LDS either: each wave streams the A fragments of its channel block from L2
// one K step ahead of the MFMAs.
//
// MFMA: v_mfma_f32_16x16x32_f16, D[out-channel][pixel] = W . X, a wave owns NT channel tiles x PT pixel tiles.  A pixel tile
// is 16 consecutive pixels of the phase's (image-clipped) region, row-major.  LDS pixel pitch = 2c + 16 bytes (an odd number
// of 16-byte slots); column `col` of the tile holds pixel offset sig(col) with sig = even offsets for the lanes
// {0-3, 12-15} and odd offsets for {4-11}, and K group g reads channel group gam(g) = {0, 2, 1, 3}: inside every
// ds_read_b128 lane group ({0-3,12-15,20-27}, ..) the 16 lanes then hit 16 distinct 16-byte slots -- conflict-free
// fragment reads without padding rows (MI355X guide, LDS).
//
// Round 4 (v2, the paper's widths c = 24 / 48 / 96; yolo_plus_ncnn_model/model.ncnn.param): general K packing for the 3x3 convs
// whose taps are not whole K steps (C2fCfg::GK), channel tiles in threes, 10-row / half-image tiles and weights from L2 where two
// planes fill the LDS, cv2 with a per-lane source table (pw_gk_phase); and, on the same machinery, s2lds_kernel (stride-2 3x3 conv
// from an LDS-staged input tile, output-channel and input-channel splits) and sppf_kernel (SPPF in one plane, pools in place).
#include "c2f.h"

#include <cstdlib>

namespace lp {

typedef _Float16 half_t;
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

using namespace c2fplan;   // configurations, rows, predicates and packers: c2f_plan.h

namespace {

struct Ctx {
  int n, oy0, ox0, H, W;
  int lane, wave, g, sig, gam;
  int dbg;                  // diagnostic flags (C2fArgs::debug_store): bit 1 = the stride-2 gather reads one cache-hot KiB
  unsigned long long* st;   // diagnostic stamps of this workgroup (null on the product path)
};
// in-phase stamp (wave 0's first lane), pinned between the surrounding instructions
#define C2F_ISTAMP(k)                                          \
  if (cx.st && threadIdx.x == 0) {                             \
    __builtin_amdgcn_sched_barrier(0);                         \
    cx.st[(k)] = clock64();                                    \
    __builtin_amdgcn_sched_barrier(0);                         \
  }
struct Rg {
  int gy0, gx0, fy0, fx0, rh, rw, R;
  unsigned magic;
};

#define C2F_STAMP(k) \
  if (a.stamps && threadIdx.x == 0) a.stamps[(size_t)blockIdx.x * 16 + (k)] = ((k) == 0 || (k) == 15) ? wall_clock64() : clock64();

// 16-byte LDS-DMA: lane l's 16 bytes land at lds + 16*l (wave-uniform lds), no VGPR in between
#define C2F_GLDS16(gptr, lptr)                                                                        \
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)(gptr),          \
                                   (void __attribute__((address_space(3)))*)(lptr), 16, 0, 0)

// Phase boundary: every wave's global stores, LDS-DMA requests and LDS traffic are done, then the workgroup barrier.
// (NOT __syncthreads(): its workgroup-scope fence does not wait for vmcnt on this target, so staged weights could still
// be in flight when another wave reads the slot.)
__device__ __forceinline__ void wg_sync() {
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

__device__ __forceinline__ floatx4 mma16(half8 a, half8 b, floatx4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ half8 as_h8(u32x4 v) { return __builtin_bit_cast(half8, v); }

// x * sigmoid(x) of (v + b), the arithmetic of act4<T, ACT_SILU> in conv_kernels.hip (hardware exp2 / rcp, two-wide multiplies)
__device__ __forceinline__ floatx4 silu4(floatx4 v, floatx4 b) {
  v = v + b;
  float nl2e = -1.4426950408889634f;   // in an SGPR: two v_pk_mul_f32 instead of four v_mul_f32 with a literal (act4, conv_kernels.hip)
  asm("" : "+s"(nl2e));
  const floatx4 t = v * floatx4{nl2e, nl2e, nl2e, nl2e};
  floatx4 e;
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = __builtin_amdgcn_exp2f(t[i]);
  e = e + 1.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) e[i] = __builtin_amdgcn_rcpf(e[i]);
  return v * e;
}

template <class CFG> __device__ __forceinline__ Rg make_region(const Ctx& cx, int E) {
  Rg r;
  const int y0 = max(cx.oy0 - E, 0), y1 = min(cx.oy0 + CFG::TH + E, cx.H);
  const int x0 = max(cx.ox0 - E, 0), x1 = min(cx.ox0 + CFG::TW + E, cx.W);
  r.gy0 = y0; r.gx0 = x0;
  r.rh = y1 - y0; r.rw = x1 - x0;
  r.R = r.rh * r.rw;
  r.fy0 = y0 - (cx.oy0 - CFG::F);
  r.fx0 = x0 - (cx.ox0 - CFG::F);
  r.magic = 0xFFFFFFFFu / (unsigned)r.rw + 1u;   // rw >= 20 (host-checked): p / rw == umulhi(p, magic) for p < 2^16
  return r;
}
// linear region pixel -> (row, column); p is clamped into the region by the caller
__device__ __forceinline__ void pix_of(const Rg& r, int p, int& py, int& px) {
  py = (int)__umulhi((unsigned)p, r.magic);
  px = p - py * r.rw;
}

// 4*NT consecutive halfs (this lane's channels of one pixel) -> memory
template <int NT> __device__ __forceinline__ void store_h(char* dst, const half_t (&h)[4 * NT]) {
  if constexpr (NT == 1) {
    half4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = h[i];
    *reinterpret_cast<half4*>(dst) = q;
  } else if constexpr (NT % 2 == 1) {   // NT = 3: 24 bytes at a 24-byte stride -- 8-byte aligned pieces
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      half4 q;
#pragma unroll
      for (int i = 0; i < 4; ++i) q[i] = h[4 * j + i];
      *reinterpret_cast<half4*>(dst + 8 * j) = q;
    }
  } else {
#pragma unroll
    for (int j = 0; j < NT / 2; ++j) {
      half8 q;
#pragma unroll
      for (int i = 0; i < 8; ++i) q[i] = h[8 * j + i];
      *reinterpret_cast<half8*>(dst + 16 * j) = q;
    }
  }
}
template <int NT> __device__ __forceinline__ void load_h(const char* src, half_t (&h)[4 * NT]) {
  if constexpr (NT == 1) {
    const half4 q = *reinterpret_cast<const half4*>(src);
#pragma unroll
    for (int i = 0; i < 4; ++i) h[i] = q[i];
  } else if constexpr (NT % 2 == 1) {
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const half4 q = *reinterpret_cast<const half4*>(src + 8 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i) h[4 * j + i] = q[i];
    }
  } else {
#pragma unroll
    for (int j = 0; j < NT / 2; ++j) {
      const half8 q = *reinterpret_cast<const half8*>(src + 16 * j);
#pragma unroll
      for (int i = 0; i < 8; ++i) h[8 * j + i] = q[i];
    }
  }
}
template <int NT> __device__ __forceinline__ void to_half(const floatx4 (&v)[NT], half_t (&h)[4 * NT]) {
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) h[4 * t + r] = (half_t)v[t][r];
}

// Epilogue of a phase whose output goes to a global NHWC tensor and nowhere else: this lane's 4*NT activated channels of region
// pixel (py, px) -> base + pixel * pitch * 2 + channel * 2.  The stride-2 convs (c3s2_phase: the entry conv of the whole-image
// configurations, s2conv_kernel) use it; the other global-store epilogues of c2f_kernel keep their lambdas, since cv2, SPPF.cv1's
// debug store, sppf_tail and the concat stores of cv1 / epi_b through this form changed the register allocation of their kernels.
template <int NT> struct GlobalEpi {
  const Ctx& cx; const Rg& rg; char* const& base; const int& pitch;
  __device__ __forceinline__ void operator()(int cb, bool ok, int py, int px, const floatx4 (&v)[NT]) const {
    const int chb = cb * 16 * NT + 4 * NT * cx.g;
    half_t h[4 * NT];
    to_half<NT>(v, h);
    const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
    if (ok) store_h<NT>(base + (size_t)((unsigned)gpix * (unsigned)pitch) * 2 + chb * 2, h);
  }
};

// K loop of one block: acc[t][i] += A(step s, tile t) . B(step s, pixel tile i).  DA / DB register sets for the A / B
// fragments: step s + D - 1 is requested before the MFMAs of step s (static indices after unrolling); fix() runs on a
// step's B fragments right before they are consumed (border masks of the stride-2 gather: applied at the load they would
// make the wave wait for it at once).
template <int S, int DA, int DB, int NT, int PT, class LA, class LB, class FX>
__device__ __forceinline__ void kloop(floatx4 (&acc)[NT][PT], LA&& la, LB&& lb, FX&& fix) {
  half8 af[DA][NT], bf[DB][PT];
#pragma unroll
  for (int s = 0; s < DA - 1; ++s)
    if (s < S) la(s, af[s]);
#pragma unroll
  for (int s = 0; s < DB - 1; ++s)
    if (s < S) lb(s, bf[s]);
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (s + DA - 1 < S) la(s + DA - 1, af[(s + DA - 1) % DA]);
    if (s + DB - 1 < S) lb(s + DB - 1, bf[(s + DB - 1) % DB]);
    __builtin_amdgcn_sched_barrier(0);
    fix(s, bf[s % DB]);
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < PT; ++i) acc[t][i] = mma16(af[s % DA][t], bf[s % DB][i], acc[t][i]);
  }
}
struct NoFix {
  template <int PT> __device__ __forceinline__ void operator()(int, half8 (&)[PT]) const {}
};

// Where a phase's A fragments ([channel block][K step][tile][lane][16 B]) come from: an LDS slot filled by stage_weights
// (tile configurations: every wave of the workgroup needs the same fragments, so they cross the CU's L1 once instead of
// eight times) or global memory / L2 (whole-image configurations, whose weights do not fit next to the planes).
template <bool LDSW> struct ASrc {
  const char* base;   // LDSW: LDS address of the slot; else the phase's fragments in global memory
  template <int NT> __device__ __forceinline__ void load(int off_bytes, int s, half8 (&af)[NT]) const {
#pragma unroll
    for (int t = 0; t < NT; ++t) af[t] = as_h8(*reinterpret_cast<const u32x4*>(base + off_bytes + (s * NT + t) * 1024));
  }
};
// request the `bytes` (a multiple of 1 KiB) of a phase's fragments into an LDS slot; the pieces are dealt to the waves
__device__ __forceinline__ void stage_weights(const Ctx& cx, const void* src, char* slot, int bytes, int nw) {
  const char* s = reinterpret_cast<const char*>(src) + cx.lane * 16;
  for (int p = cx.wave; p < (bytes >> 10); p += nw) C2F_GLDS16(s + p * 1024, slot + p * 1024);
}

// ---- 1x1 conv + SiLU.  K = KA channels from global srcA, then KB from global srcB, then KL0 from LDS plane 0 and KL1
//      from LDS plane 1 (tile pixels: cv2 over concat(y0 .., y_NB, y_{NB+1})).  UP: srcA is a half-resolution tensor read
//      at (y/2, x/2) (Interp nearest x2 fused, as conv1x1_mfma_kernel's UPS).
//      epi(cb, ok, py, px, v): this lane's 4*NT activated channels (block cb) of region pixel (py, px); ok = a real pixel.
template <class CFG, int NT, int CB, int PT, int KA, int KB, int KL0, int KL1, bool UP, bool LDSW, class EPI, int PSL0 = CFG::PS, int PSL1 = CFG::PS>
__device__ __forceinline__ void pw_phase(const Ctx& cx, const Rg& rg, const char* __restrict__ srcA, int pitchA, const char* __restrict__ srcB,
                                         int pitchB, const char* pl0, const char* pl1, const ASrc<LDSW>& wsrc, const float* __restrict__ bias,
                                         EPI&& epi, int stamp0 = -1) {
  static_assert(KA % 32 == 0 && KB % 8 == 0 && KL0 % 32 == 0 && KL1 % 16 == 0 && (KB % 32 == 0 || KL0 + KL1 == 0),
                "K segments: whole steps, except a tail of whole 8-channel groups at the very end (global srcB, or 16 channels of plane 1)");
  constexpr int SA = KA / 32, SB = cdiv_c(KB, 32), SL0 = KL0 / 32, SL1 = cdiv_c(KL1, 32), SG = SA + SB, S = SG + SL0 + SL1;
  // a last K step that is not full (KB % 32 != 0): lanes whose channel group lies past the pixel's channels re-read group 0
  // of the same pixel (their weights are zero) -- the address stays inside the pixel
  const int tail_off = (4 * (SB - 1) + cx.gam < KB / 8) ? (SB - 1) * 64 : -cx.gam * 16;
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  for (int blk = cx.wave; blk < nblk; blk += CFG::NW) {
    const int cb = blk % CB, pbk = blk / CB;
    unsigned offA[SA > 0 ? PT : 1], offB[SB > 0 ? PT : 1];
    int pb[SL0 + SL1 > 0 ? PT : 1];   // pixel slot index (x 16-byte units are added per plane)
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      int p = (pbk * PT + i) * 16 + cx.sig;
      p = p < rg.R ? p : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      const int gy = rg.gy0 + py, gx = rg.gx0 + px;
      if constexpr (SA > 0) {
        const int ya = UP ? (gy >> 1) : gy, xa = UP ? (gx >> 1) : gx;
        const int HA = UP ? (cx.H >> 1) : cx.H, WA = UP ? (cx.W >> 1) : cx.W;
        offA[i] = (unsigned)(((cx.n * HA + ya) * WA + xa) * pitchA) * 2u + (unsigned)cx.gam * 16u;
      }
      if constexpr (SB > 0) offB[i] = (unsigned)(((cx.n * cx.H + gy) * cx.W + gx) * pitchB) * 2u + (unsigned)cx.gam * 16u;
      if constexpr (SL0 + SL1 > 0) pb[i] = (rg.fy0 + py) * CFG::LW + rg.fx0 + px;
    }
    floatx4 acc[NT][PT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    // (laundered: the fragment addresses are loop-invariant when CB == 1, and LICM then hoists EVERY weight load of the
    //  phase to the top of the kernel, where they are spilled one by one behind s_waitcnt vmcnt(0))
    int woff = (cb * S * NT * 64 + cx.lane) * 16;
    asm volatile("" : "+v"(woff));
    floatx4 bv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
    // (whole-image cv1: 8 waves on the CU and a handful of K steps -- the pixel fragments of up to 5 steps ahead are in flight,
    //  at depth 3 the K loop ran at the L2 round trip: 18 B/clk for the CU)
    constexpr int DB = CFG::DEEP ? deep_depth(S, NT, PT, LDSW) : ((CFG::PERIMG && LDSW) ? min_c(S, 5) : ((NT * PT <= 20 && CFG::C >= 32) ? 3 : 2));
    constexpr int DA = LDSW ? 2 : DB;
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0) }
    kloop<S, DA, DB, NT, PT>(
        acc, [&](int s, half8(&af)[NT]) { wsrc.template load<NT>(woff, s, af); },
        [&](int s, half8(&bf)[PT]) {
#pragma unroll
          for (int i = 0; i < PT; ++i) {
            if (s < SA) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(srcA + (size_t)offA[SA > 0 ? i : 0] + s * 64));
            else if (s < SG && KB % 32 != 0 && s == SG - 1) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(srcB + (size_t)(offB[SB > 0 ? i : 0] + (unsigned)tail_off)));
            else if (s < SG) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(srcB + (size_t)offB[SB > 0 ? i : 0] + (s - SA) * 64));
            else if (s < SG + SL0) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(pl0 + pb[SL0 + SL1 > 0 ? i : 0] * PSL0 + cx.gam * 16 + (s - SG) * 64));
            // (a 16-channel plane 1: the lanes of K groups 2, 3 re-read groups 0, 1 -- their weights are zero)
            else bf[i] = as_h8(*reinterpret_cast<const u32x4*>(pl1 + pb[SL0 + SL1 > 0 ? i : 0] * PSL1 + (KL1 % 32 ? (cx.gam & 1) : cx.gam) * 16 + (s - SG - SL0) * 64));
          }
        },
        NoFix{});
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 1) }
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      epi(cb, ok, py, px, v);
    }
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 2) }
  }
}

// ---- cv2 of the general-K configurations (c = 24 / 48: the concat's segments are not whole K steps).  K group q = 4 s + gam of
//      concat(y0 .. y_{NB+1}) comes from the concat buffer in global memory while q < K2G / 8 (y0 .. y_{NB-1}), from plane 0 for the
//      next c / 8 groups (y_NB) and from plane 1 for the last c / 8 (y_{NB+1}): a per-lane table of source and offset per step,
//      at most one step of a phase mixes global and LDS lanes.  The weights keep the plain channel order of pw_phase.  With every
//      y segment read back from the concat buffer (the first version) the c = 24 module on the 80 x 80 map moved 298 MB per launch,
//      118 MB of it these segments.
template <class CFG, int NT, int CB, int PT, bool LDSW, class EPI>
__device__ __forceinline__ void pw_gk_phase(const Ctx& cx, const Rg& rg, const char* __restrict__ cat, int cat_pitch, const char* pl0, const char* pl1,
                                            const ASrc<LDSW>& wsrc, const float* __restrict__ bias, EPI&& epi, int stamp0 = -1) {
  constexpr int G0 = CFG::K2G / 8, GC = CFG::C / 8, GT = G0 + 2 * GC, S = cdiv_c(GT, 4), PS = CFG::PS;
  static_assert(CFG::PS0 == CFG::PS && G0 >= 1, "one pixel pitch for both planes; y0 comes from the concat buffer");
  int goff[S];            // global lanes: byte offset of the lane's K group inside the pixel
  const char* lbase[S];   // LDS lanes: plane base + offset of the lane's K group inside the pixel
  bool isg[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    int q = 4 * s + cx.gam;
    q = q < GT ? q : GT - 1;   // (the groups past the concat carry zero weights and re-read the last real one)
    isg[s] = q < G0;
    goff[s] = (q < G0 ? q : G0 - 1) * 16;
    const int ql = q < G0 ? 0 : q - G0;
    lbase[s] = ql < GC ? pl0 + ql * 16 : pl1 + (ql - GC) * 16;
  }
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  for (int blk = cx.wave; blk < nblk; blk += CFG::NW) {
    const int cb = blk % CB, pbk = blk / CB;
    unsigned offB[PT];
    int pb[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      int p = (pbk * PT + i) * 16 + cx.sig;
      p = p < rg.R ? p : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      offB[i] = (unsigned)(((cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px) * cat_pitch) * 2u;
      pb[i] = ((rg.fy0 + py) * CFG::LW + rg.fx0 + px) * PS;
    }
    floatx4 acc[NT][PT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    int woff = (cb * S * NT * 64 + cx.lane) * 16;
    asm volatile("" : "+v"(woff));
    floatx4 bv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
    constexpr int DB = deep_depth(S, NT, PT, LDSW);
    constexpr int DA = LDSW ? 2 : DB;
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0) }
    kloop<S, DA, DB, NT, PT>(
        acc, [&](int s, half8(&af)[NT]) { wsrc.template load<NT>(woff, s, af); },
        [&](int s, half8(&bf)[PT]) {
          const bool pure_g = 4 * s + 3 < G0, pure_l = 4 * s >= G0;   // (compile-time after unrolling)
#pragma unroll
          for (int i = 0; i < PT; ++i) {
            if (pure_g) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(cat + (size_t)offB[i] + goff[s]));
            else if (pure_l) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(lbase[s] + pb[i]));
            else if (isg[s]) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(cat + (size_t)offB[i] + goff[s]));
            else bf[i] = as_h8(*reinterpret_cast<const u32x4*>(lbase[s] + pb[i]));
          }
        },
        NoFix{});
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 1) }
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      epi(cb, ok, py, px, v);
    }
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 2) }
  }
}

// ---- 1x1 conv + SiLU of the whole-image configurations whose epilogue stores into the planes its K loop reads (cv2 -> the
//      SPPF's input, SPPF.cv1 -> the pools' input): ONE round of blocks (every accumulator tile of the phase lives in the
//      eight waves' registers), a workgroup barrier between the K loops and the epilogues.  K = KB channels from global srcB
//      (whole steps), then KL0 from plane 0 and KL1 from plane 1; weights from L2.  With the plain pw_phase these two phases ran
//      two rounds of blocks and SPPF.cv1 read cv2's output back from global memory: 46 k cycles for 1600 MFMAs per wave-set.
template <class CFG, int NT, int CB, int PT, int KB, int KL0, int KL1, int DA, class EPI>
__device__ __forceinline__ void pw_sync_phase(const Ctx& cx, const Rg& rg, const char* __restrict__ srcB, int pitchB, const char* pl0, const char* pl1,
                                              const char* __restrict__ w, const float* __restrict__ bias, EPI&& epi, int stamp0 = -1) {
  static_assert(KB % 32 == 0 && KL0 % 32 == 0 && KL1 % 32 == 0, "whole K steps");
  constexpr int SB = KB / 32, SL0 = KL0 / 32, SL1 = KL1 / 32, S = SB + SL0 + SL1, PS = CFG::PS;
  static_assert(cdiv_c(CFG::npt(0), PT) * CB <= CFG::NW && NT * PT <= 28, "one round of blocks");
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  const bool has = cx.wave < nblk;   // wave-uniform
  const int blk = has ? cx.wave : 0;
  const int cb = blk % CB, pbk = blk / CB;
  floatx4 acc[NT][PT];
  if (has) {
    unsigned offB[SB > 0 ? PT : 1];
    int pb[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      int p = (pbk * PT + i) * 16 + cx.sig;
      p = p < rg.R ? p : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      if constexpr (SB > 0) offB[i] = (unsigned)(((cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px) * pitchB) * 2u + (unsigned)cx.gam * 16u;
      pb[i] = ((rg.fy0 + py) * CFG::LW + rg.fx0 + px) * PS + cx.gam * 16;
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    int woff = (cb * S * NT * 64 + cx.lane) * 16;
    asm volatile("" : "+v"(woff));
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0) }
    kloop<S, DA, 2, NT, PT>(   // DA: weight fragments (L2) requested DA - 1 steps ahead
        acc,
        [&](int s_, half8(&af)[NT]) {
#pragma unroll
          for (int t = 0; t < NT; ++t) af[t] = as_h8(*reinterpret_cast<const u32x4*>(w + woff + (s_ * NT + t) * 1024));
        },
        [&](int s_, half8(&bf)[PT]) {
#pragma unroll
          for (int i = 0; i < PT; ++i) {
            if (s_ < SB) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(srcB + (size_t)offB[SB > 0 ? i : 0] + s_ * 64));
            else if (s_ < SB + SL0) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(pl0 + pb[i] + (s_ - SB) * 64));
            else bf[i] = as_h8(*reinterpret_cast<const u32x4*>(pl1 + pb[i] + (s_ - SB - SL0) * 64));
          }
        },
        NoFix{});
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 1) }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 2) }
  if (has) {
    floatx4 bv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      epi(cb, ok, py, px, v);
    }
    if (stamp0 >= 0) { C2F_ISTAMP(stamp0 + 3) }
  }
}

// ---- 3x3 stride-1 conv + SiLU, LDS plane -> epilogue.  K walks (tap, 32-channel block); c = 16: a K step covers two taps
//      (an even number of pixels apart: the conflict-free pairing of the header) x two channel groups.
//      One block per wave (the block shapes guarantee it).  SYNC: a workgroup barrier between the K loop and the epilogue
//      (the epilogue overwrites the plane the K loop reads).
template <class CFG, int PT, bool SYNC, bool LDSW, int PS, int CHOFF, class EPI>
__device__ __forceinline__ void c3_phase(const Ctx& cx, const Rg& rg, const char* pin, const ASrc<LDSW>& wsrc, const float* __restrict__ bias,
                                         EPI&& epi) {
  // PS: pixel pitch of the input plane; CHOFF: byte offset of the conv's input channels inside a pixel
  constexpr int C = CFG::C, NT = CFG::NTM, CB = CFG::CBM, LW = CFG::LW;
  constexpr int SPT = C >= 32 ? C / 32 : 1;
  constexpr int S = CFG::c3_steps;
  constexpr bool GK = CFG::GK;
  // c = 16: taps of step s for the lanes with (g & 1) == 0 / 1
  constexpr int TA[5] = {0, 3, 6, 1, 4}, TB[5] = {2, 5, 8, 7, 4};
  int soff[GK ? S : (C >= 32 ? 1 : 5)];
  if constexpr (GK) {
    // general packing: K group q = 4 s + gam is channel group q % G of tap q / G (G = c / 8 groups per tap); the groups past
    // the last tap carry zero weights and re-read the last real one
    constexpr int G = C / 8;
#pragma unroll
    for (int s = 0; s < S; ++s) {
      int q = 4 * s + cx.gam;
      q = q < 9 * G ? q : 9 * G - 1;
      const int tap = q / G, cg = q - tap * G;
      const int ty = (tap * 11) >> 5;   // tap / 3 for tap < 9
      soff[s] = (ty * LW + tap - 3 * ty) * PS + cg * 16;
    }
  } else if constexpr (C < 32) {
#pragma unroll
    for (int s = 0; s < 5; ++s) {
      const int ta = ((TA[s] / 3) * LW + TA[s] % 3) * PS, tb = ((TB[s] / 3) * LW + TB[s] % 3) * PS;
      soff[s] = (cx.g & 1) ? tb : ta;
    }
  }
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  const bool has = cx.wave < nblk;   // wave-uniform
  const int blk = has ? cx.wave : 0;
  const int cb = blk % CB, pbk = blk / CB;
  floatx4 acc[NT][PT];
  floatx4 bv[NT];
  if (has) {
    int pb[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      int p = (pbk * PT + i) * 16 + cx.sig;
      p = p < rg.R ? p : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      const int slot = (rg.fy0 + py) * LW + rg.fx0 + px;
      pb[i] = (slot - LW - 1) * PS + CHOFF + (GK ? 0 : (C >= 32 ? cx.gam * 16 : (cx.g >> 1) * 16));
    }
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    int woff = (cb * S * NT * 64 + cx.lane) * 16;
    asm volatile("" : "+v"(woff));
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
    kloop<S, (LDSW ? 2 : 4), 2, NT, PT>(
        acc, [&](int s, half8(&af)[NT]) { wsrc.template load<NT>(woff, s, af); },
        [&](int s, half8(&bf)[PT]) {
          if constexpr (C >= 32 && !GK) {
            const int tap = s / SPT, cblk = s % SPT;
            const int off = ((tap / 3) * LW + tap % 3) * PS + cblk * 64;
#pragma unroll
            for (int i = 0; i < PT; ++i) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(pin + pb[i] + off));
          } else {
#pragma unroll
            for (int i = 0; i < PT; ++i) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(pin + pb[i] + soff[s]));
          }
        },
        NoFix{});
  }
  if constexpr (SYNC) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
  }
  if (has) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      epi(cb, ok, py, px, v);
    }
  }
}

// ---- 3x3 stride-2 pad-1 conv + SiLU, pixel operand gathered from global memory (whole-image configurations: the region is
//      the image).  Taps above / left of the image read the centre tap's address instead and are zeroed before use.
template <class CFG, int NT, int CB, int PT, bool LDSW, class EPI>
__device__ __forceinline__ void c3s2_phase(const Ctx& cx, const Rg& rg, const char* __restrict__ src, int pitch, const ASrc<LDSW>& wsrc,
                                           const float* __restrict__ bias, EPI&& epi) {
  // (diagnostic stamps 8 / 9 / 10: wave 0's first block -- K loop start, K loop end, epilogue end)
  constexpr int SPT = CFG::KS2 / 32, S = 9 * SPT;
  const int H2 = 2 * cx.H, W2 = 2 * cx.W;
  const int pixb = pitch * 2, rowb = W2 * pixb;
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  for (int blk = cx.wave; blk < nblk; blk += CFG::NW) {
    const int cb = blk % CB, pbk = blk / CB;
    unsigned base[PT];
    int fl[PT];
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      int p = (pbk * PT + i) * 16 + cx.sig;
      p = p < rg.R ? p : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      const int gy = rg.gy0 + py, gx = rg.gx0 + px;
      base[i] = (unsigned)(((cx.n * H2 + 2 * gy) * W2 + 2 * gx) * pitch) * 2u + (unsigned)cx.gam * 16u;
      fl[i] = (gy == 0 ? 1 : 0) | (gx == 0 ? 2 : 0);
      if (cx.dbg & 2) { base[i] = (unsigned)(rowb + pixb) + (unsigned)cx.lane * 16u; fl[i] = 0; }
    }
    floatx4 acc[NT][PT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
    int woff = (cb * S * NT * 64 + cx.lane) * 16;
    asm volatile("" : "+v"(woff));
    floatx4 bv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
    constexpr int D = (LDSW && PT <= 2) ? 5 : (NT * PT <= 20 ? 3 : 2);
    if (blk == 0) { C2F_ISTAMP(8) }
    kloop<S, (LDSW ? 2 : D), D, NT, PT>(
        acc, [&](int s, half8(&af)[NT]) { wsrc.template load<NT>(woff, s, af); },
        [&](int s, half8(&bf)[PT]) {
          const int tap = s / SPT, cblk = s % SPT;
          const int dy = tap / 3, dx = tap % 3;
          const int toff = (dy - 1) * rowb + (dx - 1) * pixb;
#pragma unroll
          for (int i = 0; i < PT; ++i) {
            const bool inv = (dy == 0 && (fl[i] & 1)) || (dx == 0 && (fl[i] & 2));
            const unsigned o = base[i] + (unsigned)(inv ? 0 : toff);
            bf[i] = as_h8(*reinterpret_cast<const u32x4*>(src + (size_t)o + cblk * 64));
          }
        },
        [&](int s, half8(&bf)[PT]) {
          const int tap = s / SPT;
          const int dy = tap / 3, dx = tap % 3;
          if (dy == 0 || dx == 0) {
#pragma unroll
            for (int i = 0; i < PT; ++i) {
              const bool inv = (dy == 0 && (fl[i] & 1)) || (dx == 0 && (fl[i] & 2));
              const u32x4 m = __builtin_bit_cast(u32x4, bf[i]);
              bf[i] = as_h8(inv ? u32x4{0u, 0u, 0u, 0u} : m);
            }
          }
        });
    if (blk == 0) { C2F_ISTAMP(9) }
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      epi(cb, ok, py, px, v);
    }
    if (blk == 0) { C2F_ISTAMP(10) }
  }
}

// LDS-only phase boundary (no global traffic of this wave has to be complete)
__device__ __forceinline__ void lds_sync() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}

// ---- 5x5 stride-1 pad-2 max pool of the whole image (SPPF, model.ncnn.param:79-83), separable: a horizontal 5-max from
//      plane `pio` into plane `ptmp`, then a vertical 5-max back into `pio` (the pooled map replaces its input).  Window
//      positions outside the image are clamped onto the border pixel: it is inside the window anyway, so the maximum is the
//      same and the loops are branch-free.  gdst != null (bisect aid): the pooled map also goes to global memory.
template <class CFG>
__device__ __forceinline__ void pool_phase(const Ctx& cx, char* pio, char* ptmp, char* gdst, int gpitch) {
  constexpr int CG = CFG::C / 8, LW = CFG::LW, PS = CFG::PS, F = CFG::F, TH = CFG::TH, TW = CFG::TW;
  static_assert(TH == 20 && TW == 20, "pool strips: two strips of 10 outputs per line");
  // One thread per (line, channel group, half line): its ten 5-maxima from shared pair maxima -- p[j] = max(v[j], v[j+1]),
  // out[i] = max(p[i], p[i+2], v[i+4]) -- with the window positions clamped onto the line: 18 loads and 36 vector maxima for 10
  // outputs (a window per output: 50 loads with their index arithmetic and 40 maxima -- that form spent 5 k cycles per pass,
  // three quarters of the SPPF tail).
  auto strip = [&](const char* __restrict__ src, char* __restrict__ dst, int step) {   // position 0 of the line; bytes between positions
    const int half = (threadIdx.x / (20 * CG)) & 1;   // (only threads < 2 * 20 * CG get here)
    const int x0 = 10 * half;
    // two sub-strips of five outputs (nine loads each): the SPPF tail's accumulators stay live across the pools, and
    // fourteen loaded vectors beside them spilled
#pragma unroll
    for (int sub = 0; sub < 2; ++sub) {
      half8 v[9];
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        const int x = min(max(x0 + 5 * sub - 2 + j, 0), 19);
        v[j] = *reinterpret_cast<const half8*>(src + x * step);
      }
      half8 pm[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pm[j] = __builtin_elementwise_max(v[j], v[j + 1]);
#pragma unroll
      for (int i = 0; i < 5; ++i)
        *reinterpret_cast<half8*>(dst + (x0 + 5 * sub + i) * step) = __builtin_elementwise_max(__builtin_elementwise_max(pm[i], pm[i + 2]), v[i + 4]);
    }
  };
  const int t = threadIdx.x;
  const bool work = t < 2 * 20 * CG;
  const int line = (t % (20 * CG)) / CG, cg = t % CG;
  if (work) strip(pio + ((line + F) * LW + F) * PS + cg * 16, ptmp + ((line + F) * LW + F) * PS + cg * 16, PS);   // along x
  lds_sync();
  if (work) strip(ptmp + (F * LW + line + F) * PS + cg * 16, pio + (F * LW + line + F) * PS + cg * 16, LW * PS);   // along y
  lds_sync();
  if (gdst) {   // bisect aid: the pooled map also goes to global memory
    for (int it = threadIdx.x; it < TH * TW * CG; it += CFG::NW * 64) {
      const int pix = it / CG, g8 = it - pix * CG;
      const int y = pix / TW, x = pix - y * TW;
      *reinterpret_cast<half8*>(gdst + (size_t)(((cx.n * cx.H + y) * cx.W + x) * gpitch) * 2 + g8 * 16) =
          *reinterpret_cast<const half8*>(pio + ((y + F) * LW + x + F) * PS + g8 * 16);
    }
  }
}

// ---- SPPF.cv2 over concat(s, p1, p2, p3) without the concat: out = silu(W0 s + W1 p1 + W2 p2 + W3 p3 + b), the four
//      K segments accumulated as the pooled maps appear in plane 0 (each pool replaces its input there), so p1 .. p3 never
//      leave the CU and the conv's pixel operand comes from LDS.  One block per wave, accumulators live across the pools;
//      the next segment's weight fragments are requested before the pool that precedes it.
template <class CFG, class EPI>
__device__ __forceinline__ void sppf_tail(const Ctx& cx, const Rg& rg, char* P0, char* P1, const char* __restrict__ w, const float* __restrict__ bias,
                                          char* gcat2, int gpitch, EPI&& epi) {
  constexpr int C = CFG::C, NT = CFG::NT2, CB = CFG::CB2, PT = cdiv_c(CFG::npt(0), CFG::NW / CB), SPT = C / 32, S = 4 * SPT;
  static_assert(NT * PT <= 52 && SPT == 2, "SPPF tail: block shape");
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  const bool has = cx.wave < nblk;
  const int blk = has ? cx.wave : 0;
  const int cb = blk % CB, pbk = blk / CB;
  int pb[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    int p = (pbk * PT + i) * 16 + cx.sig;
    p = p < rg.R ? p : rg.R - 1;
    int py, px;
    pix_of(rg, p, py, px);
    pb[i] = ((rg.fy0 + py) * CFG::LW + rg.fx0 + px) * CFG::PS + cx.gam * 16;
  }
  floatx4 acc[NT][PT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
  int woff = (cb * S * NT * 64 + cx.lane) * 16;
  asm volatile("" : "+v"(woff));
  floatx4 bv[NT];   // requested behind the last pool (live across the pools it would cost the strips their registers)
  half8 af[SPT][NT];
  auto load_a = [&](int seg) {
#pragma unroll
    for (int s = 0; s < SPT; ++s)
#pragma unroll
      for (int t = 0; t < NT; ++t) af[s][t] = as_h8(*reinterpret_cast<const u32x4*>(w + woff + ((seg * SPT + s) * NT + t) * 1024));
  };
  load_a(0);
#pragma unroll
  for (int seg = 0; seg < 4; ++seg) {
    if (seg > 0) pool_phase<CFG>(cx, P0, P1, gcat2 ? gcat2 + seg * C * 2 : nullptr, gpitch);
    if (seg == 3) {
#pragma unroll
      for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
    }
    if (has) {
#pragma unroll
      for (int s = 0; s < SPT; ++s) {
        half8 bf[PT];
#pragma unroll
        for (int i = 0; i < PT; ++i) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(P0 + pb[i] + s * 64));
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < PT; ++i) acc[t][i] = mma16(af[s][t], bf[i], acc[t][i]);
        __builtin_amdgcn_sched_barrier(0);
      }
      if (seg < 3) {
        __builtin_amdgcn_sched_barrier(0);
        load_a(seg + 1);   // flies during the pool
      }
    }
    if (seg < 3) lds_sync();   // every wave has read plane 0 before the pool overwrites it
  }
  if (has) {
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      epi(cb, ok, py, px, v);
    }
  }
}

template <class CFG>
__global__ __launch_bounds__(CFG::NW * 64, CFG::WPS) void c2f_kernel(const C2fArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int C = CFG::C, NB = CFG::NB, F = CFG::F, LW = CFG::LW, PS = CFG::PS, TH = CFG::TH, TW = CFG::TW;
  constexpr bool AW = CFG::AW;
  constexpr int PS0 = CFG::PS0, Y1OFF = CFG::Y1OFF;
  char* P0 = smem;
  char* P1 = smem + CFG::PLANE0;
  char* WS = smem + CFG::PLANE0 + CFG::PLANE;   // two weight slots (AW)
  Ctx cx;
  cx.lane = threadIdx.x & 63;
  cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cx.g = cx.lane >> 4;
  {
    const int col = cx.lane & 15;
    cx.sig = col < 4 ? 2 * col : (col < 12 ? 2 * (col - 4) + 1 : 2 * (col - 8));
    cx.gam = ((cx.g & 1) << 1) | (cx.g >> 1);
  }
  cx.n = blockIdx.x % a.N;   // image fastest: the tiles of an image (which share halo pixels) meet in one XCD's L2
  const int tile = blockIdx.x / a.N;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  cx.oy0 = ty * TH; cx.ox0 = tx * TW;
  cx.H = a.H; cx.W = a.W;
  cx.st = a.stamps ? a.stamps + (size_t)blockIdx.x * 16 : nullptr;
  cx.dbg = a.debug_store;
  C2F_STAMP(0)
  C2F_STAMP(1)

  // weight slots: phase q (0 = cv1, 1 = a_0, 2 = b_0, .., 2 NB + 1 = cv2) uses slot q & 1; its fragments are requested at
  // the start of phase q - 1, right behind the barrier that retired the slot's previous user, and have landed by the next
  // barrier (__syncthreads waits for the issuing wave's vmcnt)
  auto wslot = [&](int q) { return WS + (q & 1) * CFG::WSLOT; };
  auto stage = [&](int q) {
    if constexpr (AW) {
      if (q == 0) { if constexpr (!CFG::XCV1) stage_weights(cx, a.w[C2F_W_CV1], wslot(0), CFG::WB_CV1, CFG::NW); }
      else if (q == 2 * NB + 1) stage_weights(cx, a.w[C2F_W_CV2], wslot(q), CFG::WB_CV2, CFG::NW);
      else if (q <= 2 * NB) stage_weights(cx, a.w[C2F_W_A0 + q - 1], wslot(q), CFG::WB_M, CFG::NW);
    }
  };
  auto wsrc = [&](int q, int widx) {
    return ASrc<AW>{AW ? wslot(q) : reinterpret_cast<const char*>(a.w[widx])};
  };
  stage(0);
  stage(1);
  const char* src1 = reinterpret_cast<const char*>(a.src1);
  char* cat = reinterpret_cast<char*>(a.cat);
  const bool dbg = (a.debug_store & 1) != 0;

  // ---- [s2] entry conv -> x (global); its weights occupy the (still unused) planes
  if constexpr (CFG::MODE >= 1) {
    stage_weights(cx, a.w[C2F_W_S2], smem, CFG::WB_S2, CFG::NW);
    const Rg rg = make_region<CFG>(cx, 0);
    char* xo = reinterpret_cast<char*>(a.x);
    wg_sync();
    c3s2_phase<CFG, CFG::NT_S2, 1, CFG::PT_S2, true>(cx, rg, reinterpret_cast<const char*>(a.s2_in), a.s2_pitch, ASrc<true>{smem}, a.b[C2F_W_S2],
                                                     GlobalEpi<CFG::NT_S2>{cx, rg, xo, a.x_pitch});
    wg_sync();
  }
  // pixels outside the image must read as zero (the convs' padding): they are never written, so clear the planes once.
  // Interior tiles write every pixel a later phase reads.
  {
    const bool interior = !CFG::PERIMG && cx.oy0 >= F && cx.ox0 >= F && cx.oy0 + TH + F <= a.H && cx.ox0 + TW + F <= a.W;
    if constexpr (CFG::W1_LDS) stage_weights(cx, a.w[C2F_W_CV1], P1, CFG::WB_CV1, CFG::NW);   // plane 1 is cleared behind cv1
    if (!interior) {
      constexpr int NCLR = CFG::W1_LDS ? CFG::PLANE0 : CFG::PLANE0 + CFG::PLANE;
      for (int i = threadIdx.x; i < NCLR / 16; i += CFG::NW * 64) reinterpret_cast<u32x4*>(smem)[i] = u32x4{0u, 0u, 0u, 0u};
    }
  }
  wg_sync();   // staged weights landed, planes cleared (cv1's epilogue stores into plane 0)
  C2F_STAMP(2)

  // ---- cv1 -> y0 | y1: y1 into plane 0 (whole region); into the concat buffer (tile pixels) whatever cv2 reads from there
  if constexpr (CFG::XCV1) {   // (cv1 ran in the launch in front: copy y1 of the region out of the concat buffer, every load in flight)
    const Rg rg = make_region<CFG>(cx, CFG::e_cv1);
    constexpr int CG = C / 8, NTHR = CFG::NW * 64, NPC = cdiv_c(LW * CFG::LH * CG, NTHR);
    u32x4 v[NPC];
    int dst[NPC];
#pragma unroll
    for (int j = 0; j < NPC; ++j) {
      const int it = threadIdx.x + j * NTHR;
      const int pix = it / CG, cg = it - pix * CG;
      const bool valid = pix < rg.R;
      int py, px;
      pix_of(rg, valid ? pix : rg.R - 1, py, px);
      const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
      v[j] = *reinterpret_cast<const u32x4*>(cat + (size_t)((unsigned)gpix * (unsigned)a.cat_pitch) * 2 + C * 2 + cg * 16);
      dst[j] = valid ? ((rg.fy0 + py) * LW + rg.fx0 + px) * PS0 + Y1OFF + cg * 16 : -1;
    }
#pragma unroll
    for (int j = 0; j < NPC; ++j)
      if (dst[j] >= 0) *reinterpret_cast<u32x4*>(P0 + dst[j]) = v[j];
  } else {
    const Rg rg = make_region<CFG>(cx, CFG::e_cv1);
    pw_phase<CFG, CFG::NT1, CFG::CB1, CFG::PT1, CFG::KA, CFG::KB, 0, 0, CFG::UP, AW || CFG::W1_LDS>(
        cx, rg, reinterpret_cast<const char*>(a.src0), a.pitch0, src1, a.pitch1, nullptr, nullptr,
        ASrc < AW || CFG::W1_LDS > {CFG::W1_LDS ? P1 : (AW ? wslot(0) : reinterpret_cast<const char*>(a.w[C2F_W_CV1]))}, a.b[C2F_W_CV1],
        [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NT1]) {
          constexpr int NT = CFG::NT1;
          const int chb = cb * 16 * NT + 4 * NT * cx.g;
          half_t h[4 * NT];
          to_half<NT>(v, h);
          const int fy = rg.fy0 + py, fx = rg.fx0 + px;
          if (ok) {
            if (CFG::Y01) store_h<NT>(P0 + (fy * LW + fx) * PS0 + chb * 2, h);   // y0 | y1 side by side
            else if (chb >= C) store_h<NT>(P0 + (fy * LW + fx) * PS0 + (chb - C) * 2, h);
            if ((chb < CFG::K2G || dbg) && fy >= F && fy < F + TH && fx >= F && fx < F + TW) {
              const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
              store_h<NT>(cat + (size_t)((unsigned)gpix * (unsigned)a.cat_pitch) * 2 + chb * 2, h);
            }
          }
        }, CFG::PERIMG ? -1 : 8);
  }
  wg_sync();
  if constexpr (CFG::W1_LDS) {   // plane 1 held cv1's fragments: now its zero ring
    for (int i = threadIdx.x; i < CFG::PLANE / 16; i += CFG::NW * 64) reinterpret_cast<u32x4*>(P1)[i] = u32x4{0u, 0u, 0u, 0u};
    lds_sync();
  }
  C2F_STAMP(3)

  // ---- bottlenecks: a_k: plane 0 -> plane 1; b_k: plane 1 -> y_{k+2} = y_{k+1} + ..
  //      (not the last: in place in plane 0; the last: into plane 1 behind a barrier when cv2 reads the planes)
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    stage(2 * k + 2);
    {
      const Rg rg = make_region<CFG>(cx, CFG::e_a(k));
      auto epi_a = [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NTM]) {
        constexpr int NT = CFG::NTM;
        const int chb = cb * 16 * NT + 4 * NT * cx.g;
        half_t h[4 * NT];
        to_half<NT>(v, h);
        // (c % 16 != 0: the last lane group owns the padding rows of the second channel tile -- nothing to store)
        if (ok && (C % 16 == 0 || chb < C)) store_h<NT>(P1 + ((rg.fy0 + py) * LW + rg.fx0 + px) * PS + chb * 2, h);
      };
      const ASrc<AW> wa = wsrc(2 * k + 1, C2F_W_A0 + 2 * k);
      const float* ba = a.b[C2F_W_A0 + 2 * k];
      if (k == 0) c3_phase<CFG, CFG::ptm(CFG::e_a(0)), false, AW, PS0, Y1OFF>(cx, rg, P0, wa, ba, epi_a);
      else c3_phase<CFG, CFG::ptm(CFG::e_a(NB - 1)), false, AW, PS0, Y1OFF>(cx, rg, P0, wa, ba, epi_a);
    }
    wg_sync();
    stage(2 * k + 3);
    {
      const Rg rg = make_region<CFG>(cx, CFG::e_b(k));
      const bool last = k == NB - 1;
      auto epi_b = [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NTM]) {
        constexpr int NT = CFG::NTM;
        const int chb0 = cb * 16 * NT + 4 * NT * cx.g;
        const bool real = C % 16 == 0 || chb0 < C;   // (padding rows: see epi_a)
        const int chb = real ? chb0 : 0;
        const int fy = rg.fy0 + py, fx = rg.fx0 + px;
        char* yp = P0 + (fy * LW + fx) * PS0 + Y1OFF + chb * 2;
        half_t r[4 * NT], h[4 * NT];
        load_h<NT>(yp, r);
        // silu rounded to fp16, shortcut added in fp32, rounded again: what a stored conv output + an add kernel give
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int q = 0; q < 4; ++q) h[4 * t + q] = (half_t)((float)(half_t)v[t][q] + (float)r[4 * t + q]);
        if (ok && real) {
          if (!last) store_h<NT>(yp, h);
          else if (CFG::CV2_LDS) store_h<NT>(P1 + (fy * LW + fx) * PS + chb * 2, h);
          if (((2 + k) * C < CFG::K2G || dbg) && fy >= F && fy < F + TH && fx >= F && fx < F + TW) {
            const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
            store_h<NT>(cat + (size_t)((unsigned)gpix * (unsigned)a.cat_pitch) * 2 + ((2 + k) * C + chb) * 2, h);
          }
        }
      };
      const ASrc<AW> wbk = wsrc(2 * k + 2, C2F_W_B0 + 2 * k);
      const float* bbk = a.b[C2F_W_B0 + 2 * k];
      if (k == 0 && NB > 1) c3_phase<CFG, CFG::ptm(CFG::e_b(0)), false, AW, PS, 0>(cx, rg, P1, wbk, bbk, epi_b);
      else c3_phase<CFG, CFG::ptm(CFG::e_b(NB - 1)), CFG::CV2_LDS, AW, PS, 0>(cx, rg, P1, wbk, bbk, epi_b);
    }
    wg_sync();
  }
  C2F_STAMP(4)

  // ---- cv2 over concat(y0 .. y_{NB+1}): the leading segments from the concat buffer (this workgroup's own stores,
  //      published by the barriers), y_NB and y_{NB+1} from the planes (c >= 32) -> out
  {
    const Rg rg = make_region<CFG>(cx, 0);
    char* out = reinterpret_cast<char*>(a.out);
    auto epi_cv2 = [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NT2]) {
          constexpr int NT = CFG::NT2;
          const int chb = cb * 16 * NT + 4 * NT * cx.g;
          half_t h[4 * NT];
          to_half<NT>(v, h);
          const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
          if (ok) store_h<NT>(out + (size_t)((unsigned)gpix * (unsigned)a.out_pitch) * 2 + chb * 2, h);
        };
    // K segments: [concat buffer, K2G channels] [plane 0] [plane 1]; Y01: plane 0 = y0 | y1 (2c), plane 1 = y2 (c)
    if constexpr (CFG::PERIMG) {
      // one round of blocks; MODE 2: the output (2c = COUT channels) also replaces y_NB | y_{NB+1} in the planes -- SPPF.cv1's input
      static_assert(CFG::K2G % 32 == 0 && CFG::CV2_LDS && (CFG::MODE != 2 || CFG::COUT == 2 * C), "whole-image cv2");
      pw_sync_phase<CFG, CFG::NT2, CFG::CB2, CFG::PT2W, CFG::K2G, C, C, 2>(
          cx, rg, cat, a.cat_pitch, P0, P1, reinterpret_cast<const char*>(a.w[C2F_W_CV2]), a.b[C2F_W_CV2],
          [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NT2]) {
            constexpr int NT = CFG::NT2;
            const int chb = cb * 16 * NT + 4 * NT * cx.g;
            half_t h[4 * NT];
            to_half<NT>(v, h);
            const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
            if (ok) {
              store_h<NT>(out + (size_t)((unsigned)gpix * (unsigned)a.out_pitch) * 2 + chb * 2, h);
              if constexpr (CFG::MODE == 2)
                store_h<NT>((chb < C ? P0 : P1) + ((rg.fy0 + py) * LW + rg.fx0 + px) * PS + (chb < C ? chb : chb - C) * 2, h);
            }
          }, 11);
    } else if constexpr (CFG::CV2_TAB) {
      pw_gk_phase<CFG, CFG::NT2, CFG::CB2, CFG::PT2, AW>(cx, rg, cat, a.cat_pitch, P0, P1, wsrc(2 * NB + 1, C2F_W_CV2), a.b[C2F_W_CV2], epi_cv2, 11);
    } else {
      pw_phase<CFG, CFG::NT2, CFG::CB2, CFG::PT2, 0, CFG::K2G, (CFG::CV2_LDS ? (CFG::Y01 ? 2 * C : C) : 0), (CFG::CV2_LDS ? C : 0), false, AW,
               decltype(epi_cv2)&, PS0, PS>(cx, rg, nullptr, 0, cat, a.cat_pitch, P0, P1, wsrc(2 * NB + 1, C2F_W_CV2), a.b[C2F_W_CV2], epi_cv2, 11);
    }
  }
  C2F_STAMP(5)

  // ---- [sppf] cv1 (cv2's output in the planes -> s, plane 0) -> cv2 accumulated over s and the three cascaded pools (sppf_tail)
  if constexpr (CFG::MODE == 2) {
    lds_sync();   // cv2's plane stores
    const Rg rg = make_region<CFG>(cx, 0);
    char* cat2 = reinterpret_cast<char*>(a.cat2);
    pw_sync_phase<CFG, CFG::NTS, CFG::CBS, CFG::PTS, 0, C, C, 2>(
        cx, rg, nullptr, 0, P0, P1, reinterpret_cast<const char*>(a.w[C2F_W_SP1]), a.b[C2F_W_SP1],
        [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NTS]) {
          constexpr int NT = CFG::NTS;
          const int chb = cb * 16 * NT + 4 * NT * cx.g;
          half_t h[4 * NT];
          to_half<NT>(v, h);
          if (ok) {
            store_h<NT>(P0 + ((rg.fy0 + py) * LW + rg.fx0 + px) * PS + chb * 2, h);
            if (dbg) {
              const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
              store_h<NT>(cat2 + (size_t)((unsigned)gpix * (unsigned)a.cat2_pitch) * 2 + chb * 2, h);
            }
          }
        });
    lds_sync();
    C2F_STAMP(6)
    char* out2 = reinterpret_cast<char*>(a.out2);
    sppf_tail<CFG>(cx, rg, P0, P1, reinterpret_cast<const char*>(a.w[C2F_W_SP2]), a.b[C2F_W_SP2], dbg ? cat2 : nullptr, a.cat2_pitch,
                   [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NT2]) {
                     constexpr int NT = CFG::NT2;
                     const int chb = cb * 16 * NT + 4 * NT * cx.g;
                     half_t h[4 * NT];
                     to_half<NT>(v, h);
                     const int gpix = (cx.n * cx.H + rg.gy0 + py) * cx.W + rg.gx0 + px;
                     if (ok) store_h<NT>(out2 + (size_t)((unsigned)gpix * (unsigned)a.out2_pitch) * 2 + chb * 2, h);
                   });
  }
  C2F_STAMP(7)
  C2F_STAMP(15)
}

// ---- stand-alone 3x3 stride-2 conv + SiLU (the downsampling convs between the modules, model.ncnn.param:41,118): one
//      workgroup per 20 x 20 output tile, the weights staged once in LDS, the pixel operand gathered from global memory
//      (every input pixel is touched by 2.25 taps on average; the tile's neighbours share them through L1 / L2).
template <class CFG>
__global__ __launch_bounds__(CFG::NW * 64, 2) void s2conv_kernel(const C2fArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx cx;
  cx.lane = threadIdx.x & 63;
  cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cx.g = cx.lane >> 4;
  {
    const int col = cx.lane & 15;
    cx.sig = col < 4 ? 2 * col : (col < 12 ? 2 * (col - 4) + 1 : 2 * (col - 8));
    cx.gam = ((cx.g & 1) << 1) | (cx.g >> 1);
  }
  cx.n = blockIdx.x % a.N;
  const int tile = blockIdx.x / a.N;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  cx.oy0 = ty * CFG::TH; cx.ox0 = tx * CFG::TW;
  cx.H = a.H; cx.W = a.W;
  cx.st = a.stamps ? a.stamps + (size_t)blockIdx.x * 16 : nullptr;
  cx.dbg = a.debug_store;
  C2F_STAMP(0)
  C2F_STAMP(1)
  stage_weights(cx, a.w[C2F_W_S2], smem, CFG::WBYTES, CFG::NW);
  const Rg rg = make_region<CFG>(cx, 0);
  wg_sync();
  C2F_STAMP(2)
  char* xo = reinterpret_cast<char*>(a.x);
  c3s2_phase<CFG, CFG::NT, CFG::CB, CFG::PT, true>(cx, rg, reinterpret_cast<const char*>(a.s2_in), a.s2_pitch, ASrc<true>{smem}, a.b[C2F_W_S2],
                                                  GlobalEpi<CFG::NT>{cx, rg, xo, a.x_pitch});
  C2F_STAMP(7)
  C2F_STAMP(15)
}
// ---- 3x3 stride-2 conv + SiLU with the INPUT tile staged in LDS (v2's downsampling convs, Cin 24 / 48; round 4).  The gather
//      kernels above fetch every pixel fragment of every tap from global memory: 16-byte pieces per lane, each input pixel 2.25
//      times, and they run at 160-220 TFLOP/s whatever the register ring's depth.  Here a workgroup copies the (2 TH + 1) x
//      (2 TW + 1) input pixels of its TH x TW output tile into an LDS plane once (coalesced 16-byte pieces, zero outside the
//      image = the conv's padding) and the K loop is c3_phase's with a pixel step of two: a plain LDS-fed MFMA loop, general K
//      packing for Cin 24 / 48 (c3_pack's order), the weights of this workgroup's output channels in a second LDS region.
//      OSPLIT workgroups share an output tile (each stages the input tile and computes COUT / OSPLIT channels) when the whole
//      weight set would not fit beside the plane.
template <class CFG>
__global__ __launch_bounds__(CFG::NW * 64, 2) void s2lds_kernel(const C2fArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TH = CFG::TH, TW = CFG::TW, NT = CFG::NT, CB = CFG::CB, PT = CFG::PT, S = CFG::S, LW = CFG::LW, PS = CFG::PS, G = CFG::G;
  char* PL = smem;
  char* WS = smem + CFG::PLANE;
  Ctx cx;
  cx.lane = threadIdx.x & 63;
  cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cx.g = cx.lane >> 4;
  {
    const int col = cx.lane & 15;
    cx.sig = col < 4 ? 2 * col : (col < 12 ? 2 * (col - 4) + 1 : 2 * (col - 8));
    cx.gam = ((cx.g & 1) << 1) | (cx.g >> 1);
  }
  cx.n = blockIdx.x % a.N;
  const int rest = blockIdx.x / a.N;
  const int os = rest % CFG::OSPLIT, tile = rest / CFG::OSPLIT;
  const int ty = tile / a.tiles_x, tx = tile - ty * a.tiles_x;
  cx.oy0 = ty * TH; cx.ox0 = tx * TW;
  cx.H = a.H; cx.W = a.W;
  cx.st = nullptr; cx.dbg = 0;
  // K step -> LDS offset of this lane's K group from the pixel's top-left tap (c3_phase's two forms)
  int soff[S];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if constexpr (CFG::GK) {
      int q = 4 * s + cx.gam;
      q = q < 9 * G ? q : 9 * G - 1;
      const int tap = q / G, cg = q - tap * G;
      const int t3 = (tap * 11) >> 5;   // tap / 3 for tap < 9
      soff[s] = (t3 * LW + tap - 3 * t3) * PS + cg * 16;
    } else {
      constexpr int SPT = CFG::CINH / 32;
      const int tap = s / SPT, cblk = s - tap * SPT;
      const int t3 = (tap * 11) >> 5;
      soff[s] = (t3 * LW + tap - 3 * t3) * PS + cblk * 64 + cx.gam * 16;
    }
  }
  // one block per wave: channel block cb, PT pixel tiles
  const bool has = cx.wave < CFG::NBLK;   // wave-uniform
  const int blk = has ? cx.wave : 0;
  const int cb = blk % CB, pbk = blk / CB;
  int pb[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    int p = (pbk * PT + i) * 16 + cx.sig;
    p = p < TH * TW ? p : TH * TW - 1;
    const int py = p / TW, px = p - py * TW;
    pb[i] = (2 * py * LW + 2 * px) * PS;   // the window's top-left tap: input pixel (2 oy - 1, 2 ox - 1) = plane (2 py, 2 px)
  }
  floatx4 acc[NT][PT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
  const float* bias = a.b[C2F_W_S2] + os * CFG::COUTW;
  floatx4 bv[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
#pragma unroll 1
  for (int h = 0; h < CFG::KSPLIT; ++h) {
    // ---- this pass's weights (COUTW output channels, CINH input channels) -> WS by LDS-DMA; its input channels of the tile -> PL
    stage_weights(cx, reinterpret_cast<const char*>(a.w[C2F_W_S2]) + ((size_t)os * CFG::KSPLIT + h) * CFG::WBYTES, WS, CFG::WBYTES, CFG::NW);
    {
      const int H2 = 2 * a.H, W2 = 2 * a.W, iy0 = 2 * cx.oy0 - 1, ix0 = 2 * cx.ox0 - 1;
      const char* src = reinterpret_cast<const char*>(a.s2_in) + h * CFG::CINH * 2;
      // (every piece of the tile is requested before the first is stored: 6 / 11 loads per thread in flight; in rounds of four
      //  the copy was three exposed memory round trips)
      constexpr int NPIECE = CFG::IH * CFG::IW * G, NTHR = CFG::NW * 64, U = cdiv_c(NPIECE, NTHR);
      for (int it0 = threadIdx.x; it0 < NPIECE; it0 += U * NTHR) {
        u32x4 v[U];
        int dst[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const int it = it0 + u * NTHR;
          const int itc = it < NPIECE ? it : NPIECE - 1;
          const int pix = itc / G, cg = itc - pix * G;
          const int ry = pix / CFG::IW, rx = pix - ry * CFG::IW;
          const int iy = iy0 + ry, ix = ix0 + rx;
          const bool in = it < NPIECE && iy >= 0 && iy < H2 && ix >= 0 && ix < W2;
          const int iyc = in ? iy : 0, ixc = in ? ix : 0;
          const u32x4 q = *reinterpret_cast<const u32x4*>(src + (size_t)((unsigned)((cx.n * H2 + iyc) * W2 + ixc) * (unsigned)a.s2_pitch) * 2 + cg * 16);
          v[u] = in ? q : u32x4{0u, 0u, 0u, 0u};
          dst[u] = it < NPIECE ? (ry * LW + rx) * PS + cg * 16 : -1;
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (dst[u] >= 0) *reinterpret_cast<u32x4*>(PL + dst[u]) = v[u];
      }
    }
    wg_sync();
    if (has) {
      int woff = (cb * S * NT * 64 + cx.lane) * 16;
      asm volatile("" : "+v"(woff));
      const ASrc<true> wsrc{WS};
      kloop<S, 2, 2, NT, PT>(
          acc, [&](int s, half8(&af)[NT]) { wsrc.template load<NT>(woff, s, af); },
          [&](int s, half8(&bf)[PT]) {
#pragma unroll
            for (int i = 0; i < PT; ++i) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(PL + pb[i] + soff[s]));
          },
          NoFix{});
    }
    if (h + 1 < CFG::KSPLIT) lds_sync();   // every wave has read the plane and the weights before the next pass overwrites them
  }
  if (has) {
    char* xo = reinterpret_cast<char*>(a.x);
    half8 w2f[CFG::TSTEPS][NT];
    floatx4 b2v[NT];
    if constexpr (CFG::TAIL) {
#pragma unroll
      for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int ts = 0; ts < CFG::TSTEPS; ++ts) w2f[ts][t] = as_h8(reinterpret_cast<const u32x4*>(a.w[C2F_W_CV1])[(ts * NT + t) * 64 + cx.lane]);
        b2v[t] = *reinterpret_cast<const floatx4*>(a.b[C2F_W_CV1] + 4 * NT * cx.g + 4 * t);
      }
    }
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p < TH * TW;
      const int pc = ok ? p : TH * TW - 1;
      const int py = pc / TW, px = pc - py * TW;
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      half_t hh[4 * NT];
      to_half<NT>(v, hh);
      if constexpr (CFG::TAIL) {   // out2 = silu(W2 . fp16(silu(conv)) + b2): K group g of step 0 = this lane's first 8 channels, of step 1 its last 4
        half8 bq[CFG::TSTEPS];
#pragma unroll
        for (int j = 0; j < 8; ++j) bq[0][j] = hh[j];
        if constexpr (CFG::TSTEPS == 2) {
#pragma unroll
          for (int j = 0; j < 8; ++j) bq[1][j] = j < 4 ? hh[8 + j] : (half_t)0.f;
        }
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          floatx4 o = floatx4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int ts = 0; ts < CFG::TSTEPS; ++ts) o = mma16(w2f[ts][t], bq[ts], o);
          v[t] = silu4(o, b2v[t]);
        }
        to_half<NT>(v, hh);
      }
      const int chb = os * CFG::COUTW + cb * 16 * NT + 4 * NT * cx.g;
      const int gpix = (cx.n * cx.H + cx.oy0 + py) * cx.W + cx.ox0 + px;
      if (ok) store_h<NT>(xo + (size_t)((unsigned)gpix * (unsigned)a.x_pitch) * 2 + chb * 2, hh);
    }
  }
}
// ---- SPPF in one launch for widths whose planes do not fit the whole-image C2f kernel (v2: c = 96 @20x20, yolo_plus
//      model.ncnn.param:75-87): cv1 (1x1 + SiLU) -> s in ONE LDS plane over the whole image -> cv2 accumulated over s and the three
//      cascaded 5x5 max pools as they replace each other in that plane (sppf_tail's scheme).  The pools run IN PLACE: a thread
//      owns ten outputs of one line and channel group, loads their fourteen inputs, and stores behind a workgroup barrier
//      (pool_phase needs a second plane; two planes of 96 channels are 166 KB).  OSPLIT workgroups share an image: each
//      computes s and the pools itself (cheap) and COUT / OSPLIT channels of cv2.  Weights from L2.
template <class CFG>
__device__ __forceinline__ void pool_inplace(char* P0) {
  constexpr int CG = CFG::C / 8, LW = CFG::LW, PS = CFG::PS;
  static_assert(2 * 20 * CG <= CFG::NW * 64, "one thread per (line, channel group, half line)");
  const int t = threadIdx.x;
  const bool work = t < 2 * 20 * CG;
  const int tc = work ? t : 0;
  const int half = tc / (20 * CG), line = (tc % (20 * CG)) / CG, cg = tc % CG;
  const int x0 = 10 * half;
  auto pass = [&](char* base, int step) {   // position 0 of the line; bytes between positions
    half8 o[10];
    if (work) {
      half8 v[14];
#pragma unroll
      for (int j = 0; j < 14; ++j) {
        const int x = min(max(x0 - 2 + j, 0), 19);   // clamped onto the line: the border pixel is inside the window anyway
        v[j] = *reinterpret_cast<const half8*>(base + x * step);
      }
      half8 pm[13];
#pragma unroll
      for (int j = 0; j < 13; ++j) pm[j] = __builtin_elementwise_max(v[j], v[j + 1]);
#pragma unroll
      for (int i = 0; i < 10; ++i) o[i] = __builtin_elementwise_max(__builtin_elementwise_max(pm[i], pm[i + 2]), v[i + 4]);
    }
    lds_sync();   // every thread holds its inputs
    if (work) {
#pragma unroll
      for (int i = 0; i < 10; ++i) *reinterpret_cast<half8*>(base + (x0 + i) * step) = o[i];
    }
    lds_sync();
  };
  pass(P0 + line * LW * PS + cg * 16, PS);        // along x
  pass(P0 + line * PS + cg * 16, LW * PS);        // along y
}
template <class CFG>
__global__ __launch_bounds__(CFG::NW * 64, 2) void sppf_kernel(const C2fArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int LW = CFG::LW, PS = CFG::PS, SPT = CFG::SPT;
  char* P0 = smem;
  Ctx cx;
  cx.lane = threadIdx.x & 63;
  cx.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  cx.g = cx.lane >> 4;
  {
    const int col = cx.lane & 15;
    cx.sig = col < 4 ? 2 * col : (col < 12 ? 2 * (col - 4) + 1 : 2 * (col - 8));
    cx.gam = ((cx.g & 1) << 1) | (cx.g >> 1);
  }
  cx.n = blockIdx.x % a.N;
  const int os = blockIdx.x / a.N;
  cx.oy0 = 0; cx.ox0 = 0;
  cx.H = a.H; cx.W = a.W;
  cx.st = nullptr; cx.dbg = 0;
  const Rg rg = make_region<CFG>(cx, 0);
  // ---- cv1: s = silu(W1 . x + b1), x from global memory (the module in front stored it), s -> P0
  pw_phase<CFG, CFG::NT1, CFG::CB1, CFG::PT1, 0, CFG::CIN, 0, 0, false, false>(
      cx, rg, nullptr, 0, reinterpret_cast<const char*>(a.src1), a.pitch1, nullptr, nullptr, ASrc<false>{reinterpret_cast<const char*>(a.w[C2F_W_SP1])},
      a.b[C2F_W_SP1], [&](int cb, bool ok, int py, int px, const floatx4(&v)[CFG::NT1]) {
        constexpr int NT = CFG::NT1;
        const int chb = cb * 16 * NT + 4 * NT * cx.g;
        half_t h[4 * NT];
        to_half<NT>(v, h);
        if (ok) store_h<NT>(P0 + (py * LW + px) * PS + chb * 2, h);
      });
  lds_sync();
  // ---- cv2 over concat(s, p1, p2, p3): one block per wave, accumulators live across the pools
  constexpr int NT = CFG::NT2, CB = CFG::CB2, PT = CFG::PT2, S = 4 * SPT;
  const int npt = (rg.R + 15) >> 4;
  const int nblk = ((npt + PT - 1) / PT) * CB;
  const bool has = cx.wave < nblk;
  const int blk = has ? cx.wave : 0;
  const int cb = blk % CB, pbk = blk / CB;
  int pb[PT];
#pragma unroll
  for (int i = 0; i < PT; ++i) {
    int p = (pbk * PT + i) * 16 + cx.sig;
    p = p < rg.R ? p : rg.R - 1;
    int py, px;
    pix_of(rg, p, py, px);
    pb[i] = (py * LW + px) * PS + cx.gam * 16;
  }
  floatx4 acc[NT][PT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int i = 0; i < PT; ++i) acc[t][i] = floatx4{0.f, 0.f, 0.f, 0.f};
  int woff = (((os * CB + cb) * S) * NT * 64 + cx.lane) * 16;
  asm volatile("" : "+v"(woff));
  const char* w2 = reinterpret_cast<const char*>(a.w[C2F_W_SP2]);
#pragma unroll 1
  for (int seg = 0; seg < 4; ++seg) {
    if (seg > 0) pool_inplace<CFG>(P0);
    if (has) {
      half8 af[SPT][NT];   // (requested here: a set live across the pool would cost the strips their registers)
#pragma unroll
      for (int s = 0; s < SPT; ++s)
#pragma unroll
        for (int t = 0; t < NT; ++t) af[s][t] = as_h8(*reinterpret_cast<const u32x4*>(w2 + woff + ((seg * SPT + s) * NT + t) * 1024));
#pragma unroll
      for (int s = 0; s < SPT; ++s) {
        half8 bf[PT];
#pragma unroll
        for (int i = 0; i < PT; ++i) bf[i] = as_h8(*reinterpret_cast<const u32x4*>(P0 + pb[i] + s * 64));
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int i = 0; i < PT; ++i) acc[t][i] = mma16(af[s][t], bf[i], acc[t][i]);
      }
    }
    if (seg < 3) lds_sync();   // every wave has read the plane before the pool overwrites it
  }
  if (has) {
    char* out = reinterpret_cast<char*>(a.out2);
    const float* bias = a.b[C2F_W_SP2] + os * CFG::COUTW;
    floatx4 bv[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) bv[t] = *reinterpret_cast<const floatx4*>(bias + cb * 16 * NT + 4 * NT * cx.g + 4 * t);
#pragma unroll
    for (int i = 0; i < PT; ++i) {
      const int p0 = (pbk * PT + i) * 16 + cx.sig;
      const bool ok = p0 < rg.R;
      const int p = ok ? p0 : rg.R - 1;
      int py, px;
      pix_of(rg, p, py, px);
      floatx4 v[NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) v[t] = silu4(acc[t][i], bv[t]);
      half_t h[4 * NT];
      to_half<NT>(v, h);
      const int chb = os * CFG::COUTW + cb * 16 * NT + 4 * NT * cx.g;
      const int gpix = (cx.n * cx.H + py) * cx.W + px;
      if (ok) store_h<NT>(out + (size_t)((unsigned)gpix * (unsigned)a.out2_pitch) * 2 + chb * 2, h);
    }
  }
}
// launch() is an index into the for_each_* lists of c2f_plan.h: the type whose key is the layer's
template <class CFG> bool try_launch(const C2fShape& s, const C2fArgs& a, hipStream_t st) {
  if (!(s == CFG::shape())) return false;
  set_max_dynamic_lds(reinterpret_cast<const void*>(&c2f_kernel<CFG>), CFG::LDS_BYTES);
  const int grid = a.N * a.tiles_x * a.tiles_y;
  LP_LAUNCH(c2f_kernel<CFG>, dim3(grid), dim3(CFG::NW * 64), (size_t)CFG::LDS_BYTES, st, a);
  return true;
}
struct LaunchFn {
  const C2fShape& s; const C2fArgs& a; hipStream_t st;
  template <class CFG> bool operator()() const { return try_launch<CFG>(s, a, st); }
};

// build(): what the packers of c2f_plan.h return, on the device (an empty vector: the launch does not use the slot)
template <class T> void upload(DevBuf& dst, const std::vector<T>& v) {
  if (v.empty()) return;
  dst.alloc(v.size() * sizeof(T), false);
  LP_HIP(hipMemcpy(dst.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
}

// diagnostic stamps (LITEPI_C2F_STAMPS=<file>): 16 words per workgroup, appended to the file after the launch
const char* stamp_file() {
  static const char* file = getenv("LITEPI_C2F_STAMPS");
  return file;
}
DevBuf g_stamp_buf;
unsigned long long* stamp_buffer(size_t nwg) {
  if (g_stamp_buf.bytes < nwg * 16 * 8) g_stamp_buf.alloc(nwg * 16 * 8);
  LP_HIP(hipMemset(g_stamp_buf.p, 0, nwg * 16 * 8));
  return g_stamp_buf.as<unsigned long long>();
}
void dump_stamps(const std::string& name, size_t nwg, hipStream_t st) {
  LP_HIP(hipStreamSynchronize(st));
  std::vector<unsigned long long> hst(nwg * 16);
  LP_HIP(hipMemcpy(hst.data(), g_stamp_buf.p, nwg * 16 * 8, hipMemcpyDeviceToHost));
  FILE* f = fopen(stamp_file(), "a");
  if (!f) return;
  fprintf(f, "# %s %zu\n", name.c_str(), nwg);
  for (size_t i = 0; i < nwg; ++i)
    for (int k = 0; k < 16; ++k) fprintf(f, "%llu%c", hst[i * 16 + k], k == 15 ? '\n' : ' ');
  fclose(f);
}

struct S2LaunchFn {
  const S2ConvLayer& l; C2fArgs& a; hipStream_t st;
  template <class CFG> bool operator()() const {
    if (l.Cin != CFG::CIN || l.Cout != CFG::COUT || l.has_tail != CFG::TAIL) return false;
    a.tiles_x = l.W / CFG::TW; a.tiles_y = l.H / CFG::TH;
    const size_t nwg = (size_t)a.N * a.tiles_x * a.tiles_y * CFG::OSPLIT;
    if (stamp_file() && !CFG::LDS_STAGED) a.stamps = stamp_buffer(nwg);   // (the gather kernel alone writes stamps)
    if constexpr (CFG::LDS_STAGED) {
      set_max_dynamic_lds(reinterpret_cast<const void*>(&s2lds_kernel<CFG>), CFG::LDS_BYTES);
      LP_LAUNCH(s2lds_kernel<CFG>, dim3((unsigned)nwg), dim3(CFG::NW * 64), CFG::LDS_BYTES, st, a);
    } else {
      set_max_dynamic_lds(reinterpret_cast<const void*>(&s2conv_kernel<CFG>), CFG::LDS_BYTES);
      LP_LAUNCH(s2conv_kernel<CFG>, dim3((unsigned)nwg), dim3(CFG::NW * 64), CFG::LDS_BYTES, st, a);
    }
    LP_HIP(hipGetLastError());
    if (a.stamps) dump_stamps(l.name, nwg, st);
    return true;
  }
};

}  // namespace

void C2fLayer::build(const C2fShape& s, int h, int w, const Src& src) {
  LP_CHECK(supported(s, h, w), LP_ERR_STATE, "c2f: unsupported shape");
  sh = s; H = h; W = w;
  const C2fPack p = pack_c2f(s, h, w, src);
  lds_bytes = p.lds_bytes;
  macs_per_image = p.macs_per_image;
  for (int i = 0; i < C2F_NW; ++i) {
    upload(d_w[i], p.w[i]);
    upload(d_b[i], p.b[i]);
  }
}

void S2ConvLayer::build(int cin, int cout, int hout, int wout, const std::vector<float>& w_taps, const std::vector<float>& bias,
                        const std::vector<float>* w_tail, const std::vector<float>* b_tail) {
  LP_CHECK(w_tail ? tail_supported(cin, cout, cout, hout, wout) : supported(cin, cout, hout, wout), LP_ERR_STATE,
           "s2conv: unsupported shape %d -> %d @%dx%d", cin, cout, hout, wout);
  Cin = cin; Cout = cout; H = hout; W = wout;
  has_tail = w_tail != nullptr;
  const S2Pack p = pack_s2(cin, cout, w_taps, bias, w_tail, b_tail);
  upload(d_w, p.w);
  upload(d_b, p.b);
  upload(d_w2, p.w2);
  upload(d_b2, p.b2);
}

void S2ConvLayer::launch(const View& in, const View& out, int N, hipStream_t st) const {
  LP_CHECK(in.base && out.base && in.H == 2 * H && in.W == 2 * W && in.C >= Cin && out.H == H && out.W == W && out.C >= Cout, LP_ERR_STATE,
           "s2conv %s: bad views", name.c_str());
  LP_CHECK((double)N * in.H * in.W * in.pitch * 2.0 < 4294967296.0 && (double)N * H * W * out.pitch * 2.0 < 4294967296.0, LP_ERR_ARG,
           "s2conv: tensor too large for 32-bit byte offsets");
  C2fArgs a;
  memset(&a, 0, sizeof(a));
  a.s2_in = in.base; a.s2_pitch = in.pitch;
  a.x = out.base; a.x_pitch = out.pitch;
  a.w[C2F_W_S2] = d_w.p; a.b[C2F_W_S2] = d_b.as<float>();
  a.N = N; a.H = H; a.W = W;
  if (has_tail) { a.w[C2F_W_CV1] = d_w2.p; a.b[C2F_W_CV1] = d_b2.as<float>(); }
  const bool ok = for_each_s2cfg(S2LaunchFn{*this, a, st});
  LP_CHECK(ok, LP_ERR_STATE, "s2conv %s: no kernel for this shape", name.c_str());
}

void SppfLayer::build(int cin, int c, int cout, int h, int w, const std::vector<float>& w1, const std::vector<float>& b1,
                      const std::vector<float>& w2, const std::vector<float>& b2) {
  LP_CHECK(supported(cin, c, cout, h, w), LP_ERR_STATE, "sppf: unsupported shape %d -> %d -> %d @%dx%d", cin, c, cout, h, w);
  Cin = cin; C = c; Cout = cout; H = h; W = w;
  const SppfPack p = pack_sppf(cin, c, cout, h, w, w1, b1, w2, b2);
  macs_per_image = p.macs_per_image;
  upload(d_w1, p.w1);
  upload(d_b1, p.b1);
  upload(d_w2, p.w2);
  upload(d_b2, p.b2);
}

void SppfLayer::launch(const View& in, const View& out, int N, hipStream_t st) const {
  LP_CHECK(in.base && out.base && in.H == H && in.W == W && in.C >= Cin && out.H == H && out.W == W && out.C >= Cout, LP_ERR_STATE, "sppf %s: bad views", name.c_str());
  LP_CHECK((double)N * H * W * in.pitch * 2.0 < 4294967296.0 && (double)N * H * W * out.pitch * 2.0 < 4294967296.0, LP_ERR_ARG,
           "sppf: tensor too large for 32-bit byte offsets");
  C2fArgs a;
  memset(&a, 0, sizeof(a));
  a.src1 = in.base; a.pitch1 = in.pitch;
  a.out2 = out.base; a.out2_pitch = out.pitch;
  a.w[C2F_W_SP1] = d_w1.p; a.b[C2F_W_SP1] = d_b1.as<float>();
  a.w[C2F_W_SP2] = d_w2.p; a.b[C2F_W_SP2] = d_b2.as<float>();
  a.N = N; a.H = H; a.W = W; a.tiles_x = a.tiles_y = 1;
  typedef SppfCfg CFG;
  set_max_dynamic_lds(reinterpret_cast<const void*>(&sppf_kernel<CFG>), CFG::LDS_BYTES);
  LP_LAUNCH(sppf_kernel<CFG>, dim3(N * CFG::OSPLIT), dim3(CFG::NW * 64), CFG::LDS_BYTES, st, a);
  LP_HIP(hipGetLastError());
}

void C2fLayer::launch(const IO& io, int N, hipStream_t st) const {
  C2fArgs a;
  memset(&a, 0, sizeof(a));
  auto span_ok = [&](const View& v, int mult) { return !v.base || (double)N * v.H * v.W * v.pitch * 2.0 * mult < 4294967296.0; };
  LP_CHECK(span_ok(io.src0, 1) && span_ok(io.src1, 1) && span_ok(io.cat, 1) && span_ok(io.out, 1) && span_ok(io.s2_in, 1) && span_ok(io.x, 1) &&
               span_ok(io.cat2, 1) && span_ok(io.out2, 1), LP_ERR_ARG, "c2f: tensor too large for 32-bit byte offsets");
  LP_CHECK(io.src1.base && io.cat.base && io.out.base && io.src1.H == H && io.src1.W == W && io.cat.H == H && io.out.H == H, LP_ERR_STATE,
           "c2f %s: bad views", name.c_str());
  LP_CHECK((sh.KA > 0) == (io.src0.base != nullptr), LP_ERR_STATE, "c2f %s: src0 mismatch", name.c_str());
  if (sh.KA > 0) LP_CHECK(io.src0.H == (sh.UP ? H / 2 : H) && io.src0.W == (sh.UP ? W / 2 : W) && io.src0.C >= sh.KA, LP_ERR_STATE, "c2f %s: src0 shape", name.c_str());
  LP_CHECK(io.src1.C >= sh.KB && io.cat.C >= (2 + sh.NB) * sh.C && io.out.C >= sh.COUT, LP_ERR_STATE, "c2f %s: view channels", name.c_str());
  a.src0 = io.src0.base; a.pitch0 = io.src0.pitch;
  a.src1 = io.src1.base; a.pitch1 = io.src1.pitch;
  a.cat = io.cat.base; a.cat_pitch = io.cat.pitch;
  a.out = io.out.base; a.out_pitch = io.out.pitch;
  for (int i = 0; i < C2F_NW; ++i) { a.w[i] = d_w[i].p; a.b[i] = d_b[i].as<float>(); }
  if (sh.MODE >= 1) {
    LP_CHECK(io.s2_in.base && io.x.base && io.s2_in.H == 2 * H && io.s2_in.W == 2 * W && io.s2_in.C >= sh.KS2 && io.x.C >= 2 * sh.C, LP_ERR_STATE,
             "c2f %s: entry conv views", name.c_str());
    a.s2_in = io.s2_in.base; a.s2_pitch = io.s2_in.pitch;
    a.x = io.x.base; a.x_pitch = io.x.pitch;
  }
  if (sh.MODE == 2) {
    LP_CHECK(io.cat2.base && io.out2.base && io.cat2.C >= 4 * sh.C && io.out2.C >= sh.COUT, LP_ERR_STATE, "c2f %s: SPPF views", name.c_str());
    a.cat2 = io.cat2.base; a.cat2_pitch = io.cat2.pitch;
    a.out2 = io.out2.base; a.out2_pitch = io.out2.pitch;
  }
  a.N = N; a.H = H; a.W = W;
  const C2fRow* row = find_c2f(sh);
  LP_CHECK(row, LP_ERR_STATE, "c2f %s: no configuration for this shape", name.c_str());
  a.tiles_x = W / row->tw; a.tiles_y = H / row->th;
  // store_all: bisect aid, every y segment goes to the concat buffer.  The layer's own flag, set by the planner from the switch it
  // read at load: a per-process read here could disagree with the blobs that load marked as stored
  static const int dbg_flags = getenv("LITEPI_C2F_DEBUG") ? atoi(getenv("LITEPI_C2F_DEBUG")) : 0;   // see Ctx::dbg
  a.debug_store = (store_all ? 1 : 0) | (dbg_flags & ~1);
  const size_t nwg = (size_t)N * a.tiles_x * a.tiles_y;
  if (stamp_file()) a.stamps = stamp_buffer(nwg);
  const bool ok = for_each_cfg(LaunchFn{sh, a, st});
  LP_CHECK(ok, LP_ERR_STATE, "c2f %s: no kernel for this shape", name.c_str());
  LP_HIP(hipGetLastError());
  if (a.stamps) dump_stamps(name, nwg, st);
}

}  // namespace lp
