// Fused ShuffleNetV2 stage (fp16): every stride-1 InvertedResidual of a stage in ONE launch.
//
// The un-fused classifier spends ~40 launches per batch on GEMMs of a few MFLOP each, all of
// them bound by the ~6 us launch/latency floor.  Here one workgroup (one wave per 16-channel
// tile: 4/8/16 waves) owns 64 pixels (1 ROI at
// 8x8, 4 ROIs at 4x4, 16 ROIs at 2x2) and keeps the stage tensor X = [x_lo | x_hi] resident in
// LDS across all blocks; per block (reference e2e.py:393 -> torchvision InvertedResidual):
//     t1 = relu(W1 . x_hi + b1)            MFMA, A fragments straight from L2 (weights are read
//     t2 = dw3x3(t1) + bd                  VALU                      once per workgroup per block)
//     y  = relu(W2 . t2 + b2)              MFMA
//     X  = channel_shuffle(cat(x_lo, y))   in place: read x_lo, barrier, write interleaved pairs
// MFMA orientation as in conv_kernels.hip: D[out-channel][pixel]; a D fragment holds 4
// consecutive channels of one pixel per lane, which is exactly the 8-byte store the next stage's
// B fragment (8 consecutive channels of one pixel) wants in LDS.
#include "cls_fused.h"

#include "cls_dev.h"   // vector types, wload / gemm_acc / store_relu / shuffle_phys, conv5 epilogue, fc tile, softmax tail

namespace lp {

#define FS_PIX 64  // pixels per workgroup = 4 MFMA column tiles
static_assert(FS_PIX == clsplan::kFusedPix, "cls_plan.h sizes the LDS for 64 pixels");

// One wave = one 16-channel output tile x 4 pixel tiles.  The S weight fragments of a GEMM are requested together (wload) well
// before they are used, so a GEMM costs one L2 round trip that overlaps the preceding phase instead of one per K step.  A wave
// beyond the tile count loads nothing (S = 0: its fragments read as zero) and only moves data.
template <int NW, int SMAX>
__global__ __launch_bounds__(NW * 64) void shuffle_stage_kernel(const FusedStageArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int NTHR = NW * 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, col = lane & 15;
  const int bfp = a.bfp, bf = a.bf, HW = a.HW, W = a.W;
  const int xrow = 2 * bfp * 2 + 16;  // LDS row pitches in bytes: odd number of 16-byte slots
  const int trow = bfp * 2 + 16;
  char* X = smem;
  char* T1 = X + FS_PIX * xrow;
  char* T2 = T1 + FS_PIX * trow;
  const int CGX = 2 * bfp / 8, CGT = bfp / 8;
  const int Tt = bfp / 16, S = (bfp + 31) / 32;
  const bool active = wave < Tt;  // this wave's output tile (waves beyond the tile count only move data)
  const int Sw = active ? S : 0;
  const int ch0 = wave * 16 + 4 * g;
  const int R = *a.m_dyn;
  const int ngroups = (R + a.group - 1) / a.group;
  const half_t* in = reinterpret_cast<const half_t*>(a.in);
  half_t* out = reinterpret_cast<half_t*>(a.out);

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int roi0 = grp * a.group;
    const int nvalid = ((R - roi0) < a.group ? (R - roi0) : a.group) * HW;
    const long pix0 = (long)roi0 * HW;
    // 16-wave workgroups are capped at 128 VGPRs: they keep one fragment set in flight, not two
    constexpr bool PREF_NEXT = NW < 16;
    u32x4 w1f[SMAX], w2f[SMAX];
    if (PREF_NEXT) wload<SMAX>(w1f, a.blk[0].w1, wave, Sw, lane);
    for (int i = tid; i < FS_PIX * CGX; i += NTHR) {
      const int px = i / CGX, cg = i - px * CGX;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (px < nvalid) v = *reinterpret_cast<const u32x4*>(in + (pix0 + px) * a.in_pitch + cg * 8);
      *reinterpret_cast<u32x4*>(X + px * xrow + cg * 16) = v;
    }
    __syncthreads();

    for (int b = 0; b < a.nblk; ++b) {
      const FusedBlockW bw = a.blk[b];
      floatx4 acc[4];
      // ---- t1 = relu(W1 . x_hi + b1) -------------------------------------------------------
      if (!PREF_NEXT) wload<SMAX>(w1f, bw.w1, wave, Sw, lane);
      if (PREF_NEXT) wload<SMAX>(w2f, bw.w2, wave, Sw, lane);  // lands while pw1 + dw run
      if (active) {
        zero_acc<4>(acc);
        gemm_acc<SMAX, 4>(w1f, S, 0, X + bfp * 2, xrow, bfp, 0, lane, acc);
        store_relu<4>(T1, trow, 0, wave, bw.b1, acc, lane);
      }
      if (PREF_NEXT && b + 1 < a.nblk) wload<SMAX>(w1f, a.blk[b + 1].w1, wave, Sw, lane);  // for the next block
      if (!PREF_NEXT) wload<SMAX>(w1f, bw.w2, wave, Sw, lane);  // re-use the one set: lands during dw
      __syncthreads();
      // ---- t2 = dw3x3(t1) + bd (pad 1, stride 1, inside each ROI's WxW map) -------------------
      for (int i = tid; i < FS_PIX * CGT; i += NTHR) {
        const int px = i / CGT, cg = i - px * CGT;
        const int rl = px / HW, pp = px - rl * HW;
        const int y = pp / W, x = pp - y * W;
        float acc8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc8[j] = bw.dwb[cg * 8 + j];
        for (int ky = 0; ky < 3; ++ky) {
          const int yy = y - 1 + ky;
          if (yy < 0 || yy >= W) continue;
          for (int kx = 0; kx < 3; ++kx) {
            const int xx = x - 1 + kx;
            if (xx < 0 || xx >= W) continue;
            const half8 v = *reinterpret_cast<const half8*>(T1 + (rl * HW + yy * W + xx) * trow + cg * 16);
            const float* wr = bw.dw + (ky * 3 + kx) * bfp + cg * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) acc8[j] = fmaf((float)v[j], wr[j], acc8[j]);
          }
        }
        half8 o;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (half_t)acc8[j];
        *reinterpret_cast<half8*>(T2 + px * trow + cg * 16) = o;
      }
      __syncthreads();
      // ---- y = relu(W2 . t2 + b2); X = shuffle(cat(x_lo, y)) in place --------------------------
      half4 x1v[4];
      if (active) {
        zero_acc<4>(acc);
        if (PREF_NEXT) gemm_acc<SMAX, 4>(w2f, S, 0, T2, trow, bfp, 0, lane, acc); else gemm_acc<SMAX, 4>(w1f, S, 0, T2, trow, bfp, 0, lane, acc);
#pragma unroll
        for (int p = 0; p < 4; ++p) x1v[p] = *reinterpret_cast<const half4*>(X + (p * 16 + col) * xrow + ch0 * 2);
      }
      __syncthreads();  // every x_lo value is in registers before any interleaved pair is written
      if (active) {
        const floatx4 bias = *reinterpret_cast<const floatx4*>(bw.b2 + ch0);
#pragma unroll
        for (int p = 0; p < 4; ++p) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = ch0 + i;
            if (c < bf) {
              half2v pr;
              pr[0] = x1v[p][i];
              pr[1] = (half_t)fmaxf(acc[p][i] + bias[i], 0.f);
              *reinterpret_cast<half2v*>(X + (p * 16 + col) * xrow + shuffle_phys(2 * c, bf, bfp) * 2) = pr;
            }
          }
        }
      }
      __syncthreads();
    }

    for (int i = tid; i < FS_PIX * CGX; i += NTHR) {
      const int px = i / CGX, cg = i - px * CGX;
      if (px < nvalid)
        *reinterpret_cast<u32x4*>(out + (pix0 + px) * a.out_pitch + cg * 8) = *reinterpret_cast<const u32x4*>(X + px * xrow + cg * 16);
    }
    __syncthreads();
  }
}

void launch_fused_stage(const FusedStageArgs& a, int max_items, hipStream_t st) {
  const size_t lds = clsplan::fused_stage_lds_bytes(a.bfp);
  LP_CHECK(clsplan::fused_stage_supports(a.bfp, a.HW, a.group), LP_ERR_STATE,
           "fused ShuffleNet stage: unsupported geometry (bfp %d, HW %d)", a.bfp, a.HW);
  const int Tt = a.bfp / 16, S = (a.bfp + 31) / 32;
  int groups = (max_items + a.group - 1) / a.group;
  if (groups > 1024) groups = 1024;
  if (groups < 1) groups = 1;
#define LP_FS(NW, SM)                                                                                          \
  {                                                                                                            \
    set_max_dynamic_lds(reinterpret_cast<const void*>(shuffle_stage_kernel<NW, SM>), 160 * 1024);                                                                                                \
    LP_LAUNCH((shuffle_stage_kernel<NW, SM>), dim3(groups), dim3(NW * 64), lds, st, a);                 \
  }
  if (Tt <= 4 && S <= 2) LP_FS(4, 2) else if (Tt <= 8 && S <= 4) LP_FS(8, 4) else if (Tt <= 16 && S <= 8) LP_FS(16, 8) else
    throw Error(LP_ERR_STATE, "fused ShuffleNet stage: too many channel tiles");
#undef LP_FS
  LP_HIP(hipGetLastError());
}

// ------------------------------------------------------------------------------------
// Fused classifier head (fp16): conv5 1x1 (Cin -> 1024) + ReLU, x.mean([2,3]), fc, softmax,
// arg-max and the scatter of (class, confidence) into the detection records -- reference
// e2e.py:393-396 (torchvision conv5 / mean / fc) + e2e.py:525-526.  One 16-wave workgroup owns
// 16 ROIs (64 pixels of the 2x2 stage-4 map); activations stay in LDS, the 1024-channel conv5
// output never exists in memory: each wave reduces its accumulator tiles over the 4 pixels of a ROI
// with two lane shuffles and writes the fp16 mean straight into the fc operand image.
// ------------------------------------------------------------------------------------
#define FH_ROIS 16
static_assert(FH_ROIS == clsplan::kHeadRois, "cls_plan.h sizes the LDS for 16 ROIs");
__global__ __launch_bounds__(1024) void cls_head_kernel(const FusedHeadArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cin = a.cin_p;                 // physical input channels (two padded halves)
  const int xrow = cin * 2 + 16;
  char* X = smem;                          // [64 px][cin] fp16
  char* Mn = X + 64 * xrow;                // [16 rois][1024] fp16 (mean of relu(conv5))
  float* LG = reinterpret_cast<float*>(Mn + FH_ROIS * clsplan::kMeanRow);  // [16 rois][nc_p] fp32 logits
  const int S5 = (cin + 31) / 32, CGX = cin / 8;
  const int R = *a.m_dyn;
  const int ngroups = (R + FH_ROIS - 1) / FH_ROIS;
  const half_t* in = reinterpret_cast<const half_t*>(a.in);

  for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
    const int roi0 = grp * FH_ROIS;
    const int nroi = (R - roi0) < FH_ROIS ? (R - roi0) : FH_ROIS;
    for (int i = tid; i < 64 * CGX; i += 1024) {
      const int px = i / CGX, cg = i - px * CGX;
      u32x4 v = u32x4{0u, 0u, 0u, 0u};
      if (px < nroi * 4) v = *reinterpret_cast<const u32x4*>(in + ((long)roi0 * 4 + px) * a.in_pitch + cg * 8);
      *reinterpret_cast<u32x4*>(X + px * xrow + cg * 16) = v;
    }
    __syncthreads();
    // ---- conv5: 64 output tiles of 16 channels, 4 per wave; mean over the 4 pixels of each ROI -----
#pragma unroll 1
    for (int tq = 0; tq < 4; ++tq) {
      const int t = wave * 4 + tq;
      floatx4 acc[4];
      zero_acc<4>(acc);
      for (int s0 = 0; s0 < S5; s0 += 8) {
        u32x4 af[8];
        wload<8>(af, a.w5 + ((size_t)t * S5 + s0) * 64, 0, S5 - s0, lane);
        gemm_acc<8, 4>(af, S5 - s0, s0, X, xrow, cin, 0, lane, acc);
      }
      conv5_mean_store<FH_ROIS>(Mn, t, a.b5, acc, lane);
    }
    __syncthreads();
    // ---- fc: logits[roi][class] = Wfc . mean + b, one 16-class tile per wave ------------------------
    if (wave < a.out.nc_p / 16) fc_tile<FH_ROIS>(LG, Mn, a.wfc, a.bfc, a.out.nc_p, wave, lane);
    __syncthreads();
    // ---- softmax + arg-max, one wave per ROI ------------------------------------------------------------
    if (wave < nroi) cls_tail(LG + wave * a.out.nc_p, roi0 + wave, lane, a.out);
    __syncthreads();
  }
}

void launch_fused_head(const FusedHeadArgs& a, int max_items, hipStream_t st) {
  const size_t lds = clsplan::fused_head_lds_bytes(a.cin_p, a.out.nc_p);
  LP_CHECK(clsplan::cls_head_supports(a.cin_p, a.out.nc) && a.out.nc_p == clsplan::class_pad(a.out.nc), LP_ERR_STATE,
           "fused classifier head: unsupported geometry (cin %d, classes %d)", a.cin_p, a.out.nc);
  set_max_dynamic_lds(reinterpret_cast<const void*>(cls_head_kernel), 160 * 1024);
  int groups = (max_items + FH_ROIS - 1) / FH_ROIS;
  if (groups > 512) groups = 512;
  LP_LAUNCH(cls_head_kernel, dim3(groups), dim3(1024), lds, st, a);
  LP_HIP(hipGetLastError());
}

}  // namespace lp
